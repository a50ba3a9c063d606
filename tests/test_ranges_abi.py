"""CPU suite: the entry points for blocks of the caller's choosing (nlzm_hip_compress_ranges*) and for content-defined cut points
(nlzm_hip_cut_points*) without a device: the exports, every entry failing loudly, the bound, the counters, the cut kernels' resources, and
the command line's -cdc:B where it needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import nlzm_amd
from tests.cli_tools import cli

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
E_ARG, E_NODEVICE = -1, -2
NEW = ["nlzm_hip_compress_ranges_dev", "nlzm_hip_compress_ranges", "nlzm_hip_compress_ranges_bound", "nlzm_hip_cut_points_dev", "nlzm_hip_cut_points"]


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_exports(lib):
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    for name in NEW:
        assert name in nlzm_amd.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^(int|uint64_t) " + name + r"\(", header, re.M), name
    for name in ("compress_ranges", "cut_points", "cut_ranges"):
        assert callable(getattr(nlzm_amd, name))


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_argument_errors_need_no_device(lib):
    """E_ARG comes before the device is asked for: the same answer with and without one (no launch is made either way)"""
    buf = (C.c_uint8 * 4096)()
    out = (C.c_uint8 * 64)()
    blen, got = (C.c_uint64 * 4)(), C.c_uint64(0)
    cuts, ncuts = (C.c_uint64 * 8)(), C.c_uint32(0)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    bad_ranges = [
        (3, u64(0, 4000, 10), u64(10, 97, 10), b"range 1 "),
        (2, u64(0, 4097), u64(10, 0), b"range 1 "),
        (2, u64((1 << 64) - 1, 0), u64(2, 5), b"range 0 "),
        (1, u64(2), u64((1 << 64) - 1), b"range 0 "),
    ]
    for form in (lib.nlzm_hip_compress_ranges, lib.nlzm_hip_compress_ranges_dev):
        for k, off, ln, text in bad_ranges:
            assert form(buf, 4096, k, off, ln, 16, out, 1 << 40, blen, C.byref(got)) == E_ARG
            assert text in lib.nlzm_hip_last_error() and b"runs over" in lib.nlzm_hip_last_error()
        assert form(buf, 4096, 0, u64(0), u64(1), 16, out, 1 << 40, blen, C.byref(got)) == E_ARG
        assert form(buf, 4096, 65537, u64(0), u64(1), 16, out, 1 << 40, blen, C.byref(got)) == E_ARG
        assert form(buf, 4096, 1, None, u64(1), 16, out, 1 << 40, blen, C.byref(got)) == E_ARG
        assert form(buf, 4096, 1, u64(0), u64(1), 16, None, 1 << 40, blen, C.byref(got)) == E_ARG
    for form in (lib.nlzm_hip_cut_points, lib.nlzm_hip_cut_points_dev):
        for avg_bits, lo, hi in ((0, 32, 64), (31, 32, 64), (12, 31, 64), (12, 0, 64), (12, 65, 64), (12, 32, (1 << 31) + 1)):
            assert form(buf, 4096, avg_bits, lo, hi, cuts, 8, C.byref(ncuts)) == E_ARG, (avg_bits, lo, hi)
            assert lib.nlzm_hip_last_error()
        assert form(buf, 4096, 12, 32, 64, None, 8, C.byref(ncuts)) == E_ARG
        assert form(buf, 4096, 12, 32, 64, cuts, 8, None) == E_ARG


def test_entries_fail_loudly_without_gpu(lib):
    if not no_gpu():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 4096)()
    out = (C.c_uint8 * (1 << 20))()
    blen, got = (C.c_uint64 * 4)(), C.c_uint64(0)
    cuts, ncuts = (C.c_uint64 * 200)(), C.c_uint32(0)
    off, ln = (C.c_uint64 * 2)(0, 100), (C.c_uint64 * 2)(100, 3996)
    calls = {
        "nlzm_hip_compress_ranges": lambda: lib.nlzm_hip_compress_ranges(buf, 4096, 2, off, ln, 16, out, 1 << 20, blen, C.byref(got)),
        "nlzm_hip_compress_ranges_dev": lambda: lib.nlzm_hip_compress_ranges_dev(buf, 4096, 2, off, ln, 16, out, 1 << 20, blen, C.byref(got)),
        "nlzm_hip_cut_points": lambda: lib.nlzm_hip_cut_points(buf, 4096, 4, 32, 64, cuts, 200, C.byref(ncuts)),
        "nlzm_hip_cut_points_dev": lambda: lib.nlzm_hip_cut_points_dev(buf, 4096, 4, 32, 64, cuts, 200, C.byref(ncuts)),
    }
    for name, call in calls.items():
        assert call() == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
    for f in (lambda: nlzm_amd.compress_ranges(bytes(100), [(0, 50), (50, 50)]), lambda: nlzm_amd.cut_points(bytes(4096), 4)):
        with pytest.raises(nlzm_amd.NlzmError):
            f()


def test_bound_is_the_sum_of_the_streams_bounds(lib):
    lens = [0, 1, 5, 4096, 14847, 14848, 14849, 300_000, 1 << 31, 0]
    arr = (C.c_uint64 * len(lens))(*lens)
    for k in (1, 2, 5, len(lens)):
        assert lib.nlzm_hip_compress_ranges_bound(k, arr) == sum(lib.nlzm_hip_compress_bound(l) for l in lens[:k])
    assert lib.nlzm_hip_compress_ranges_bound(0, arr) == 0 and lib.nlzm_hip_compress_ranges_bound(65537, arr) == 0
    assert lib.nlzm_hip_compress_ranges_bound(1, None) == 0
    huge = (C.c_uint64 * 3)(1 << 63, 1 << 63, 1 << 63)             # (each one's own bound fits 64 bits)
    assert lib.nlzm_hip_compress_ranges_bound(1, huge) == lib.nlzm_hip_compress_bound(1 << 63) and lib.nlzm_hip_compress_ranges_bound(3, huge) == 0            # (the sum wraps)
    many = (C.c_uint64 * 65536)(*([7] * 65536))
    assert lib.nlzm_hip_compress_ranges_bound(65536, many) == 65536 * lib.nlzm_hip_compress_bound(7)


def test_cut_ranges():
    assert nlzm_amd.cut_ranges(0, []) == [(0, 0)]
    assert nlzm_amd.cut_ranges(100, []) == [(0, 100)]
    assert nlzm_amd.cut_ranges(100, [40, 72]) == [(0, 40), (40, 32), (72, 28)]
    with pytest.raises(ValueError):
        nlzm_amd.cut_ranges(100, [72, 40])
    with pytest.raises(ValueError):
        nlzm_amd.cut_ranges(100, [101])


def test_counters_answer_without_a_device(lib):
    v = C.c_uint64(0)
    for key in ("cut_us", "cut_candidates", "cut_segment_bytes"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert v.value >= 2048 and v.value % 2048 == 0       # the segment size: 64 lanes' runs of whole bitmap words, known without a device
    assert lib.nlzm_hip_get_counter(b"cut_no_such", C.byref(v)) != 0
    assert lib.nlzm_hip_get_counter(b"container_sets", C.byref(v)) == 0


def test_cut_kernels_resources():
    """both kernels of nlzm_cut.hip by the compiler's own account: no scratch, no spill, no dynamic stack, LDS within 64 KiB"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "cut-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kernels = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = [k.split()[0] for k in kernels]
    assert len(kernels) == 2 and any("cut_scan_kernel" in n for n in names) and any("cut_select_kernel" in n for n in names), names
    for k in kernels:
        num = lambda what: int(re.search(re.escape(what) + r": (\d+)", k).group(1))
        assert num("ScratchSize [bytes/lane]") == 0 and num("SGPRs Spill") == 0 and num("VGPRs Spill") == 0, k
        assert "Dynamic Stack: False" in k, k
        assert num("LDS Size [bytes/block]") <= 65536, k
    assert any(int(re.search(r"LDS Size \[bytes/block\]: (\d+)", k).group(1)) > 32768 for k in kernels)      # (the scan's stage is there)


def test_library_has_the_cut_kernels(lib):
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    assert b"cut_scan_kernel" in blob and b"cut_select_kernel" in blob


def test_cli_usage_and_conflicts(lib, tmp_path):
    usage = cli().stdout
    assert "\t-cdc:B = (this build) c cuts the blocks by content on the GPU" in usage
    # the lines of -blocks:k are word for word what they were
    assert ("\t-blocks:k = (this build) compress k independent blocks, 1 to 65536: as many at once as a launch holds (64), more of them\n"
            "\t            in sets one after another; d/t read the streams back to back\n") in usage
    src = tmp_path / "in.bin"
    src.write_bytes(bytes(5000))
    dst = tmp_path / "out.nlzm"
    for flags in (("-cdc:12", "-blocks:4"), ("-blocks:4", "-cdc:12"), ("-cdc:12", "-gpus:1"), ("-gpus:2", "-blocks:3", "-cdc:12")):
        r = cli(*flags, "c", src, dst)
        assert r.returncode == 255 and "Error: -cdc:B" in r.stdout and "-blocks:k or -gpus:g" in r.stdout, r.stdout
        assert not dst.exists()
    for bad in ("-cdc:9", "-cdc:31", "-cdc:", "-cdc:12x", "-cdc:-3"):
        r = cli(bad, "c", src, dst)
        assert r.returncode == 255 and "B from 10 to 30" in r.stdout and not dst.exists(), (bad, r.stdout)
    r = cli("-cdc:12", "-blocks:1", "h", src)        # (-blocks:1 is no block mode; h needs no device)
    assert r.returncode == 0, r.stdout
    if no_gpu():
        r = cli("-cdc:12", "c", src, dst)
        assert r.returncode == 255 and "Error:" in r.stdout and not dst.exists(), r.stdout
