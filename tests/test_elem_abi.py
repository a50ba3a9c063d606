"""CPU suite: the entry points of include/nlzm_hip_elem.h without a device: the header held to nlzm_amd/_abi.ELEM_TABLE by the means tests/test_abi.py
uses for the main header, the exports, every argument error before the device is asked for, nlzm_hip_choose_elem, every entry failing loudly, the
counters, and the kernels' resources by the compiler's own account."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nlzm_amd
from nlzm_amd import _abi
from tests import elem_model
from tests.test_abi import ADDRESS_ONLY, ctypes_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NODEVICE = -1, -2
KERNELS = ["elem_count_kernel", "elem_total_kernel"]


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def u64(*v):
    return (C.c_uint64 * len(v))(*v)


def header():
    txt = open(os.path.join(ROOT, "include", "nlzm_hip_elem.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)


def test_signature_table_matches_the_header(lib):
    """every row of _abi.ELEM_TABLE against its prototype in include/nlzm_hip_elem.h, as tests/test_abi.py holds TABLE to include/nlzm_hip.h; the two
    tables share no name, and the main header and its table are what they were"""
    found = re.findall(r"([\w\s*]+?)\b(nlzm_hip_\w+)\s*\(([^)]*)\)\s*;", header())
    protos = {name: (ret, [a for a in args.split(",") if a.split() != ["void"]]) for ret, name, args in found}
    assert sorted(protos) == sorted(_abi.ELEM_TABLE) == sorted(_abi.ELEM_SYMBOLS) and len(protos) == 7
    assert not set(_abi.ELEM_TABLE) & set(_abi.TABLE) and len(_abi.TABLE) == 67 and nlzm_amd.ABI_SYMBOLS == list(_abi.TABLE)
    bad = []
    for name, (ret, params) in protos.items():
        restype, argtypes = _abi.ELEM_TABLE[name]
        if restype not in ctypes_for(ret):
            bad.append((name, "returns", " ".join(ret.split()), restype))
        if len(argtypes) != len(params):
            bad.append((name, "takes", len(params), len(argtypes)))
            continue
        for i, (param, have) in enumerate(zip(params, argtypes)):
            if have not in ctypes_for(param):
                bad.append((name, i, " ".join(param.split()), have))
    assert not bad, bad
    assert not set(ADDRESS_ONLY) & set(protos)
    assert '#include "nlzm_hip.h"' in open(os.path.join(ROOT, "include", "nlzm_hip_elem.h")).read()
    main = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    assert not any(name in main for name in protos)


def test_exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", nlzm_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (restype, argtypes) in _abi.ELEM_TABLE.items():
        assert name in exported, name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes, name          # (bind gives a library the rows of both tables)
    for f in ("plane_costs", "choose_elem", "choose_elems", "compress_auto", "compress_tensors"):
        assert callable(getattr(nlzm_amd, f)), f
    text = open(os.path.join(ROOT, "include", "nlzm_hip_elem.h")).read()
    for key in ('"elem_us"', '"elem_bytes"', '"elem_segment_bytes"'):
        assert key in text, key


def forms(lib):
    """every entry that takes ranges, as a call of (buf, n, k, off, len, out) with the rest of its arguments in place"""
    dst, blen, got = (C.c_uint8 * (1 << 20))(), (C.c_uint64 * 4)(), C.c_uint64(0)
    auto = lambda f: lambda b, n, k, o, l, out: f(b, n, k, o, l, out, 16, dst, 1 << 20, blen, C.byref(got))
    return [("plane_costs", lambda b, n, k, o, l, out: lib.nlzm_hip_plane_costs(b, n, k, o, l, out, None), u64(*[0] * 16)),
            ("plane_costs_dev", lambda b, n, k, o, l, out: lib.nlzm_hip_plane_costs_dev(b, n, k, o, l, out, None), u64(*[0] * 16)),
            ("choose_elems", lib.nlzm_hip_choose_elems, (C.c_uint8 * 4)()), ("choose_elems_dev", lib.nlzm_hip_choose_elems_dev, (C.c_uint8 * 4)()),
            ("compress_ranges_auto", auto(lib.nlzm_hip_compress_ranges_auto), (C.c_uint8 * 4)()),
            ("compress_ranges_auto_dev", auto(lib.nlzm_hip_compress_ranges_auto_dev), (C.c_uint8 * 4)())]


def test_argument_errors_need_no_device(lib):
    """E_ARG comes before the device is asked for: the same answer with and without one, and the text names the range"""
    src = (C.c_uint8 * 4096)()
    M = (1 << 64) - 1
    cases = [
        (4096, 2, u64(0, 4000), u64(10, 97), b"range 1 (offset 4000, 97 bytes) runs over the 4096 bytes of the buffer"),
        (4096, 1, u64(M), u64(2), b"range 0 "),
        (4096, 1, u64(0), u64(M), b"range 0 "),
        (4096, 3, u64(0, 0, 4097), u64(10, 10, 0), b"range 2 "),
        (1 << 41, 2, u64(0, 8), u64(10, 1 << 40), b"range 1 (offset 8, 1099511627776 bytes): the statistic takes ranges below 2^40 bytes"),
    ]
    for name, form, out in forms(lib):
        for n, k, off, ln, text in cases:
            assert form(src, n, k, off, ln, out) == E_ARG, name
            assert text in lib.nlzm_hip_last_error(), (name, lib.nlzm_hip_last_error())
        assert form(src, 4096, 0, u64(0), u64(1), out) == E_ARG and b"0 ranges" in lib.nlzm_hip_last_error(), name
        assert form(src, 4096, 65537, u64(0), u64(1), out) == E_ARG and b"65537 ranges" in lib.nlzm_hip_last_error(), name
        assert form(src, 4096, 1, None, u64(1), out) == E_ARG and form(src, 4096, 1, u64(0), None, out) == E_ARG, name
        assert form(src, 4096, 1, u64(0), u64(1), None) == E_ARG and form(None, 4096, 1, u64(0), u64(1), out) == E_ARG, name
    dst, blen, got, el = (C.c_uint8 * 4096)(), (C.c_uint64 * 4)(), C.c_uint64(0), (C.c_uint8 * 4)()
    for f in (lib.nlzm_hip_compress_ranges_auto, lib.nlzm_hip_compress_ranges_auto_dev):
        assert f(src, 4096, 1, u64(0), u64(100), el, 16, None, 4096, blen, C.byref(got)) == E_ARG
        assert f(src, 4096, 1, u64(0), u64(100), el, 16, dst, 4096, blen, None) == E_ARG
    with pytest.raises(ValueError):
        nlzm_amd.plane_costs(bytes(10), [])
    with pytest.raises(ValueError):
        nlzm_amd.choose_elems(bytes(10), [])
    with pytest.raises(ValueError):
        nlzm_amd.compress_auto(bytes(10), [])
    with pytest.raises(ValueError):
        nlzm_amd.choose_elem((1, 2, 3), 5000)
    with pytest.raises(nlzm_amd.NlzmError, match="range 0 "):
        nlzm_amd.plane_costs(bytes(10), [(5, 6)])


def test_choose_elem_needs_no_device(lib):
    rng = np.random.default_rng(20261021)
    for _ in range(2000):
        c = [int(v) >> int(rng.integers(4, 60)) for v in rng.integers(0, 1 << 63, 4, dtype=np.uint64)]
        if rng.integers(0, 3) == 0:
            c[int(rng.integers(1, 4))] = max(0, c[0] - c[0] // 32 + int(rng.integers(-2, 3)))
        n = int(rng.integers(0, 10_000))
        assert lib.nlzm_hip_choose_elem(u64(*c), n) == elem_model.choose(c, n), (c, n)
    assert nlzm_amd.choose_elem((3200, 3100, 9999, 9999), 5000) == 2 and nlzm_amd.choose_elem((3200, 3101, 9999, 9999), 5000) == 1
    assert nlzm_amd.choose_elem((1000, 10, 10, 10), 4095) == 1 and nlzm_amd.choose_elem((1000, 10, 10, 10), 4096) == 2
    assert lib.nlzm_hip_choose_elem(None, 5000) == 1


def test_entries_fail_loudly_without_gpu(lib):
    if not no_gpu():
        pytest.skip("GPU present")
    src = (C.c_uint8 * 8192)()
    for name, form, out in forms(lib):
        assert form(src, 8192, 2, u64(0, 100), u64(5000, 100), out) == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
    for call in (lambda: nlzm_amd.plane_costs(bytes(200), [(0, 100)]), lambda: nlzm_amd.choose_elems(bytes(200), [(0, 100)]),
                 lambda: nlzm_amd.compress_auto(bytes(200), [(0, 200)], dedup=True)):
        with pytest.raises(nlzm_amd.NlzmError):
            call()
    assert nlzm_amd.counter("dedup_ranges") == 0        # (the binding has restored the option)


def test_counters_answer_without_a_device(lib):
    v = C.c_uint64(99)
    for key in ("elem_us", "elem_bytes"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert lib.nlzm_hip_get_counter(b"elem_segment_bytes", C.byref(v)) == 0
    assert v.value >= 4096 and v.value % 16 == 0 and v.value < 1 << 32        # units of sixteen bytes, counters of 32 bits
    assert lib.nlzm_hip_get_counter(b"elem_no_such", C.byref(v)) != 0
    assert lib.nlzm_hip_set_option(b"elem_segment_bytes", 1) == E_ARG and b"unknown option" in lib.nlzm_hip_last_error()        # (no new option)


def test_elem_kernels_resources(lib):
    """both kernels of nlzm_elem.hip by the compiler's own account: no scratch, no spill, no dynamic stack; the count kernel's LDS is 8 x 256 counters
    of four bytes a wave, four waves a workgroup -- 32,768 bytes, the figure of DESIGN.md section 31 --, and the total kernel uses none"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "elem-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kernels = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = [k.split()[0] for k in kernels]
    assert len(kernels) == 2 and all(any(want in n for n in names) for want in KERNELS), names
    for k in kernels:
        num = lambda what: int(re.search(re.escape(what) + r": (\d+)", k).group(1))
        assert num("ScratchSize [bytes/lane]") == 0 and num("SGPRs Spill") == 0 and num("VGPRs Spill") == 0, k
        assert "Dynamic Stack: False" in k, k
        assert num("LDS Size [bytes/block]") == (4 * 8 * 256 * 4 if "elem_count_kernel" in k else 0), k
        assert num("VGPRs") <= 96, k             # (five waves a SIMD: the five workgroups a CU's LDS holds)
    assert "32,768 bytes" in open(os.path.join(ROOT, "DESIGN.md")).read().split("## 31.")[1]
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    for name in KERNELS:
        assert name.encode() in blob, name
