"""CPU suite: the equal-range finder's entry points (nlzm_hip_equal_ranges*) and the compress path's option "dedup_ranges" without a device: the
exports, every entry failing loudly, a bad range refused and named before anything else, the counters and options, the kernels' resources by the
compiler's own account, and the command line's -dedup where it needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import nlzm_amd
from tests.cli_tools import cli

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
E_ARG, E_NODEVICE = -1, -2
NEW = ["nlzm_hip_equal_ranges_dev", "nlzm_hip_equal_ranges"]
KERNELS = ["dedup_fingerprint_kernel", "dedup_combine_kernel", "dedup_pair_kernel", "dedup_verdict_kernel"]


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_exports(lib):
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    for name in NEW:
        assert name in nlzm_amd.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert not name.startswith("nlzm_hip_decode_")
    declared = set(re.findall(r"^(?:int|void|uint32_t|uint64_t|const char \*) ?(nlzm_hip_\w+)\(", header, re.M))
    assert declared == set(nlzm_amd.ABI_SYMBOLS)
    assert callable(nlzm_amd.equal_ranges)
    for key in ('"dedup_ranges"', '"test_dedup_hash_bits"', '"dedup_distinct"', '"dedup_dup_bytes"', '"dedup_rounds"', '"dedup_pairs"', '"dedup_compared_bytes"',
                '"dedup_us"', '"dedup_segment_bytes"'):
        assert key in header, key


def test_a_bad_range_is_named_before_anything_else(lib):
    """E_ARG comes before the device is asked for: the same answer with and without one (no launch is made either way)"""
    buf = (C.c_uint8 * 4096)()
    first, fp = (C.c_uint32 * 4)(), (C.c_uint64 * 4)()
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    bad_ranges = [
        (3, u64(0, 4000, 10), u64(10, 97, 10), b"range 1 "),
        (2, u64(0, 4097), u64(10, 0), b"range 1 "),
        (2, u64((1 << 64) - 1, 0), u64(2, 5), b"range 0 "),
        (1, u64(2), u64((1 << 64) - 1), b"range 0 "),
    ]
    for form in (lib.nlzm_hip_equal_ranges, lib.nlzm_hip_equal_ranges_dev):
        for k, off, ln, text in bad_ranges:
            assert form(buf, 4096, k, off, ln, first, fp) == E_ARG
            assert text in lib.nlzm_hip_last_error() and b"runs over" in lib.nlzm_hip_last_error()
        assert form(buf, 4096, 0, u64(0), u64(1), first, fp) == E_ARG
        assert form(buf, 4096, 65537, u64(0), u64(1), first, fp) == E_ARG
        assert form(buf, 4096, 1, None, u64(1), first, fp) == E_ARG
        assert form(buf, 4096, 1, u64(0), None, first, fp) == E_ARG
        assert form(buf, 4096, 1, u64(0), u64(1), None, fp) == E_ARG
    with pytest.raises(ValueError):
        nlzm_amd.equal_ranges(bytes(10), [])


def test_entries_fail_loudly_without_gpu(lib):
    if not no_gpu():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 4096)()
    out = (C.c_uint8 * (1 << 20))()
    first, fp = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    blen, got = (C.c_uint64 * 2)(), C.c_uint64(0)
    off, ln = (C.c_uint64 * 2)(0, 100), (C.c_uint64 * 2)(100, 100)
    for name in NEW:
        assert getattr(lib, name)(buf, 4096, 2, off, ln, first, fp) == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
        assert getattr(lib, name)(buf, 4096, 2, off, ln, first, None) == E_NODEVICE, name
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.equal_ranges(bytes(200), [(0, 100), (100, 100)])
    # the compress path with the option on: the same loud failure, the option restored by the binding
    assert lib.nlzm_hip_set_option(b"dedup_ranges", 1) == 0
    try:
        assert lib.nlzm_hip_compress_ranges_dev(buf, 4096, 2, off, ln, 16, out, 1 << 20, blen, C.byref(got)) == E_NODEVICE
        assert lib.nlzm_hip_compress_ranges(buf, 4096, 2, off, ln, 16, out, 1 << 20, blen, C.byref(got)) == E_NODEVICE
        assert lib.nlzm_hip_compress_ranges(buf, 4096, 2, off, (C.c_uint64 * 2)(100, 4000), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
        assert b"range 1 " in lib.nlzm_hip_last_error()
    finally:
        assert lib.nlzm_hip_set_option(b"dedup_ranges", 0) == 0
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.compress_ranges(bytes(100), [(0, 50), (50, 50)], dedup=True)
    assert nlzm_amd.counter("dedup_ranges") == 0


def test_counters_answer_without_a_device(lib):
    v = C.c_uint64(99)
    for key in ("dedup_distinct", "dedup_dup_bytes", "dedup_rounds", "dedup_pairs", "dedup_compared_bytes", "dedup_us", "dedup_gather_us"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert lib.nlzm_hip_get_counter(b"dedup_segment_bytes", C.byref(v)) == 0
    assert v.value >= 1024 and v.value % 16 == 0         # the segment size: whole 16-byte units, known without a device
    assert lib.nlzm_hip_get_counter(b"dedup_no_such", C.byref(v)) != 0


def test_set_option_takes_both_keys(lib):
    v = C.c_uint64(0)
    try:
        for value in (1, 0):
            assert lib.nlzm_hip_set_option(b"dedup_ranges", value) == 0
            assert lib.nlzm_hip_get_counter(b"dedup_ranges", C.byref(v)) == 0 and v.value == value
        for value in (0, 2, 63, 64):
            assert lib.nlzm_hip_set_option(b"test_dedup_hash_bits", value) == 0
        for key, value in ((b"dedup_ranges", 2), (b"dedup_ranges", -1), (b"test_dedup_hash_bits", 65), (b"test_dedup_hash_bits", -1)):
            assert lib.nlzm_hip_set_option(key, value) == E_ARG and b"out of range" in lib.nlzm_hip_last_error(), (key, value)
        assert lib.nlzm_hip_set_option(b"dedup_no_such", 1) == E_ARG and b"unknown option" in lib.nlzm_hip_last_error()
        assert lib.nlzm_hip_get_counter(b"dedup_ranges", C.byref(v)) == 0 and v.value == 0
    finally:
        lib.nlzm_hip_set_option(b"dedup_ranges", 0)
        lib.nlzm_hip_set_option(b"test_dedup_hash_bits", 64)


def test_dedup_kernels_resources():
    """all four kernels of nlzm_dedup.hip by the compiler's own account: no scratch, no spill, no dynamic stack, no LDS"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "dedup-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kernels = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = [k.split()[0] for k in kernels]
    assert len(kernels) == 4 and all(any(want in n for n in names) for want in KERNELS), names
    for k in kernels:
        num = lambda what: int(re.search(re.escape(what) + r": (\d+)", k).group(1))
        assert num("ScratchSize [bytes/lane]") == 0 and num("SGPRs Spill") == 0 and num("VGPRs Spill") == 0, k
        assert "Dynamic Stack: False" in k, k
        assert num("LDS Size [bytes/block]") == 0, k
        assert num("VGPRs") <= 128, k            # (two workgroups of four waves a SIMD at least)


def test_library_has_the_dedup_kernels(lib):
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    for name in KERNELS:
        assert name.encode() in blob, name


def test_cli_usage_and_conflicts(lib, tmp_path):
    usage = cli().stdout
    assert "\t-dedup = (this build) with -cdc:B:" in usage
    # the lines of -cdc:B and -blocks:k are word for word what they were
    assert "\t-cdc:B = (this build) c cuts the blocks by content on the GPU, 2^B bytes on average (B 10 to 30): an edit changes the blocks around it only\n" in usage
    assert ("\t-blocks:k = (this build) compress k independent blocks, 1 to 65536: as many at once as a launch holds (64), more of them\n"
            "\t            in sets one after another; d/t read the streams back to back\n") in usage
    src = tmp_path / "in.bin"
    src.write_bytes(bytes(5000))
    dst = tmp_path / "out.nlzm"
    for flags in (("-dedup",), ("-dedup", "-blocks:4"), ("-blocks:4", "-dedup"), ("-dedup", "-gpus:1"), ("-dedup", "-verify")):
        r = cli(*flags, "c", src, dst)
        assert r.returncode == 255 and "Error: -dedup" in r.stdout and "needs -cdc:B" in r.stdout, r.stdout
        assert not dst.exists()
    r = cli("-dedup", "-cdc:12", "-blocks:1", "h", src)        # (h needs no device and no blocks)
    assert r.returncode == 0, r.stdout
    if no_gpu():
        r = cli("-dedup", "-cdc:12", "c", src, dst)
        assert r.returncode == 255 and "Error:" in r.stdout and not dst.exists(), r.stdout
