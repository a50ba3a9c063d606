"""CPU suite: the byte-plane filter's entry points (nlzm_hip_planes*, nlzm_hip_compress_ranges_typed*, nlzm_hip_decompress_blocks_typed*) without a
device: the exports, every argument error before the device is asked for, every entry failing loudly, the counters, the kernels' resources by the
compiler's own account, nlzm_amd.read_index_typed on good and damaged version-3 files, and the command line's -elem:E where it needs no device -- a
container built here, from the model's planes and the oracle's streams, decoded by host-only `nlzm d` / `t`."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import nlzm_amd
from nlzm_amd import corpus
from tests import oracle_py, planes_model
from tests.cli_tools import cli, write_index

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
E_ARG, E_NODEVICE = -1, -2
NEW = ["nlzm_hip_planes_dev", "nlzm_hip_planes", "nlzm_hip_compress_ranges_typed_dev", "nlzm_hip_compress_ranges_typed",
       "nlzm_hip_decompress_blocks_typed_dev", "nlzm_hip_decompress_blocks_typed"]
KERNELS = ["planes_forward_kernel", "planes_inverse_kernel"]


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def u64(*v):
    return (C.c_uint64 * len(v))(*v)


def u8(*v):
    return (C.c_uint8 * len(v))(*v)


def test_exports(lib):
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    for name in NEW:
        assert name in nlzm_amd.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    declared = set(re.findall(r"^(?:int|void|uint32_t|uint64_t|const char \*) ?(nlzm_hip_\w+)\(", header, re.M))
    assert declared == set(nlzm_amd.ABI_SYMBOLS)
    for f in ("planes", "compress_typed", "decompress_typed", "read_index_typed", "compress_tensors", "decompress_tensors"):
        assert callable(getattr(nlzm_amd, f)), f
    for key in ('"planes_us"', '"planes_bytes"', '"planes_segment_bytes"'):
        assert key in header, key


def test_planes_argument_errors_need_no_device(lib):
    """E_ARG comes before the device is asked for: the same answer with and without one, and the text names the range"""
    src, dst = (C.c_uint8 * 4096)(), (C.c_uint8 * 4096)()
    cases = [
        (2, u64(0, 4000), u64(0, 100), u64(10, 97), u8(2, 2), b"range 1 ", b"source"),
        (2, u64(0, 0), u64(0, 4090), u64(10, 7), u8(2, 2), b"range 1 ", b"destination"),
        (1, u64((1 << 64) - 1), u64(0), u64(2), u8(2), b"range 0 ", b"runs over"),
        (1, u64(0), u64(0), u64((1 << 64) - 1), u8(2), b"range 0 ", b"runs over"),
        (3, u64(0, 0, 0), u64(0, 100, 5), u64(10, 10, 10), u8(2, 4, 8), b"range 0 ", b"overlaps range 2 "),
        (2, u64(0, 0), u64(0, 100), u64(10, 10), u8(2, 3), b"range 1", b"element size 3"),
        (1, u64(0), u64(0), u64(10), u8(0), b"range 0", b"element size 0"),
    ]
    for form in (lib.nlzm_hip_planes, lib.nlzm_hip_planes_dev):
        for inverse in (0, 1):
            for k, so, do, ln, el, name, text in cases:
                assert form(src, 4096, dst, 4096, k, so, do, ln, el, inverse) == E_ARG
                err = lib.nlzm_hip_last_error()
                assert name in err and text in err, err
            assert form(src, 4096, dst, 4096, 0, u64(0), u64(0), u64(1), u8(1), inverse) == E_ARG
            assert form(src, 4096, dst, 4096, 65537, u64(0), u64(0), u64(1), u8(1), inverse) == E_ARG
            for nulled in range(4):
                args = [u64(0), u64(0), u64(1), u8(1)]
                args[nulled] = None
                assert form(src, 4096, dst, 4096, 1, *args, inverse) == E_ARG
            # a buffer pair that overlaps: there is no in-place form
            assert form(src, 4096, src, 4096, 1, u64(0), u64(2048), u64(100), u8(2), inverse) == E_ARG and b"no in-place form" in lib.nlzm_hip_last_error()
            assert form(src, 4096, C.byref(src, 4095), 1, 1, u64(0), u64(0), u64(1), u8(2), inverse) == E_ARG and b"no in-place form" in lib.nlzm_hip_last_error()
    with pytest.raises(ValueError):
        nlzm_amd.planes(bytes(10), [], [])
    with pytest.raises(ValueError):
        nlzm_amd.planes(bytes(10), [(0, 10)], [2, 2])
    with pytest.raises(nlzm_amd.NlzmError, match="element size 5"):
        nlzm_amd.planes(bytes(10), [(0, 10)], [5])


def test_typed_argument_errors_need_no_device(lib):
    src, out = (C.c_uint8 * 4096)(), (C.c_uint8 * (1 << 20))()
    blen, got = (C.c_uint64 * 4)(), C.c_uint64(0)
    for form in (lib.nlzm_hip_compress_ranges_typed, lib.nlzm_hip_compress_ranges_typed_dev):
        assert form(src, 4096, 2, u64(0, 4000), u64(10, 97), u8(2, 4), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
        assert b"range 1 " in lib.nlzm_hip_last_error() and b"runs over" in lib.nlzm_hip_last_error()
        assert form(src, 4096, 2, u64(0, 100), u64(10, 10), u8(2, 6), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
        assert b"range 1" in lib.nlzm_hip_last_error() and b"element size 6" in lib.nlzm_hip_last_error()
        assert form(src, 4096, 2, None, u64(10, 10), u8(2, 4), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
        assert form(src, 4096, 2, u64(0, 100), u64(10, 10), u8(2, 4), 16, None, 1 << 20, blen, C.byref(got)) == E_ARG
        # no element sizes, or every one 1: the untyped call, and its errors
        for el in (None, u8(1, 1)):
            assert form(src, 4096, 2, u64(0, 4000), u64(10, 97), el, 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
            assert b"range 1 " in lib.nlzm_hip_last_error()
        assert form(src, 4096, 0, u64(0), u64(1), u8(2), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
        assert form(src, 4096, 65537, u64(0), u64(1), u8(2), 16, out, 1 << 20, blen, C.byref(got)) == E_ARG
    for form in (lib.nlzm_hip_decompress_blocks_typed, lib.nlzm_hip_decompress_blocks_typed_dev):
        assert form(src, 4096, 2, u64(100, 100), u64(10, 10), u8(2, 5), out, 1 << 20, None, C.byref(got)) == E_ARG
        assert b"range 1" in lib.nlzm_hip_last_error() and b"element size 5" in lib.nlzm_hip_last_error()
    with pytest.raises(ValueError):
        nlzm_amd.compress_typed(bytes(10), [(0, 10)], [2, 2])
    with pytest.raises(ValueError):
        nlzm_amd.decompress_typed(bytes(10), [10], [10, 10], [2])


def test_entries_fail_loudly_without_gpu(lib):
    if not no_gpu():
        pytest.skip("GPU present")
    src, dst = (C.c_uint8 * 4096)(), (C.c_uint8 * (1 << 20))()
    blen, got = (C.c_uint64 * 2)(), C.c_uint64(0)
    off, ln, el = u64(0, 100), u64(100, 100), u8(2, 4)
    for form in (lib.nlzm_hip_planes, lib.nlzm_hip_planes_dev):
        assert form(src, 4096, dst, 4096, 2, off, off, ln, el, 0) == E_NODEVICE
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error()
    for form in (lib.nlzm_hip_compress_ranges_typed, lib.nlzm_hip_compress_ranges_typed_dev):
        assert form(src, 4096, 2, off, ln, el, 16, dst, 1 << 20, blen, C.byref(got)) == E_NODEVICE
        assert form(src, 4096, 2, off, ln, None, 16, dst, 1 << 20, blen, C.byref(got)) == E_NODEVICE
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error()
    for form in (lib.nlzm_hip_decompress_blocks_typed, lib.nlzm_hip_decompress_blocks_typed_dev):
        assert form(src, 4096, 2, ln, ln, el, dst, 1 << 20, None, C.byref(got)) == E_NODEVICE
        assert form(src, 4096, 2, ln, ln, None, dst, 1 << 20, None, C.byref(got)) == E_NODEVICE
    for call in (lambda: nlzm_amd.planes(bytes(200), [(0, 100), (100, 100)], [2, 4]), lambda: nlzm_amd.compress_typed(bytes(200), [(0, 200)], [4], dedup=True),
                 lambda: nlzm_amd.decompress_typed(bytes(200), [200], [100], [4])):
        with pytest.raises(nlzm_amd.NlzmError):
            call()
    assert nlzm_amd.counter("dedup_ranges") == 0        # (the binding has restored the option)


def test_counters_answer_without_a_device(lib):
    v = C.c_uint64(99)
    for key in ("planes_us", "planes_bytes"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert lib.nlzm_hip_get_counter(b"planes_segment_bytes", C.byref(v)) == 0
    assert v.value >= 1024 and v.value % 128 == 0        # the segment size: sixteen whole elements of every size, known without a device
    assert lib.nlzm_hip_get_counter(b"planes_no_such", C.byref(v)) != 0
    assert lib.nlzm_hip_set_option(b"planes_segment_bytes", 1) == E_ARG and b"unknown option" in lib.nlzm_hip_last_error()        # (no new option)


def test_planes_kernels_resources(lib):
    """both kernels of nlzm_planes.hip by the compiler's own account: no scratch, no spill, no dynamic stack, LDS one image of a segment's planes
    per wave -- the segment and sixteen bytes a row of shift, four waves a workgroup"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "planes-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kernels = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = [k.split()[0] for k in kernels]
    assert len(kernels) == 2 and all(any(want in n for n in names) for want in KERNELS), names
    S = nlzm_amd.counter("planes_segment_bytes")
    for k in kernels:
        num = lambda what: int(re.search(re.escape(what) + r": (\d+)", k).group(1))
        assert num("ScratchSize [bytes/lane]") == 0 and num("SGPRs Spill") == 0 and num("VGPRs Spill") == 0, k
        assert "Dynamic Stack: False" in k, k
        assert num("LDS Size [bytes/block]") == 4 * (S + 8 * 16), k
        assert num("VGPRs") <= 128, k            # (four waves a SIMD: the four workgroups a CU's LDS holds)
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    for name in KERNELS:
        assert name.encode() in blob, name


# ---- a typed container built on the CPU: three blocks, e of 2, 4 and 8, a ragged tail ----

HIST = 17


@pytest.fixture(scope="module")
def container(lib):
    rng = np.random.default_rng(corpus.SEED + 170)
    blocks = [
        ((rng.standard_normal(3000) * 0.02).astype("<f4").view("<u4") >> 16).astype("<u2").tobytes(),
        (np.arange(2500) * 3 + 1000).astype("<i4").tobytes(),
        (np.arange(700) * 7).astype("<i8").tobytes() + b"tail",      # (four bytes behind the last whole element)
    ]
    elems = [2, 4, 8]
    streams = [oracle_py.compress(planes_model.forward(b, e), HIST) for b, e in zip(blocks, elems)]
    return {"blocks": blocks, "elems": elems, "streams": streams, "crcs": [zlib.crc32(b) for b in blocks], "whole": zlib.crc32(b"".join(blocks))}


def write_index3(path, c, elems=None, crcs=None, whole=None, **kw):
    write_index(path, c["streams"], [len(b) for b in c["blocks"]], crcs or c["crcs"], c["whole"] if whole is None else whole, version=3, elems=elems or c["elems"], **kw)


def test_read_index_typed(tmp_path, container):
    c = container
    p = tmp_path / "c.idx"
    lens, raws = [len(s) for s in c["streams"]], [len(b) for b in c["blocks"]]
    write_index3(p, c)
    assert nlzm_amd.read_index_typed(p) == (lens, raws, c["crcs"], c["elems"])
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)                       # (read_index goes on refusing version 3)
    # versions 1 and 2 through read_index, every element size 1
    p.write_text(f"NLZMIDX 2 2 30 20 0000ABCD\n0 12 10 00000001\n12 8 20 00000002\n")
    assert nlzm_amd.read_index_typed(p) == ([12, 8], [10, 20], [1, 2], [1, 1])
    p.write_text(f"NLZMIDX 1 2 30 20\n0 12 10\n12 8 20\n")
    assert nlzm_amd.read_index_typed(p) == ([12, 8], [10, 20], None, [1, 1])
    # the damage tests/test_range_abi.py does to versions 1 and 2: raw lengths that do not sum to n_in; block lengths that do not sum to n_out; a gap
    for kw in ({"n_in": sum(raws) + 1}, {"n_in": sum(raws) - 1}, {"n_out": sum(lens) + 1}):
        write_index3(p, c, **kw)
        with pytest.raises(ValueError):
            nlzm_amd.read_index_typed(p)
    offs = [sum(lens[:i]) for i in range(len(lens))]
    write_index3(p, c, offs=offs[:2] + [offs[2] + 1])
    with pytest.raises(ValueError):
        nlzm_amd.read_index_typed(p)
    M = 1 << 64
    damaged = [
        f"NLZMIDX 3 2 100 {M - 1} 00000000\n0 50 60 00000000 2\n50 {M - 40} 40 00000000 2\n",       # an off + len that wraps 64 bits
        f"NLZMIDX 3 2 {M - 1} 100 00000000\n0 50 {M - 5} 00000000 2\n50 50 10 00000000 2\n",       # raw lengths whose sum wraps
        f"NLZMIDX 3 1 10 {M + 8} 00000000\n0 {M + 8} 10 00000000 2\n",                             # a field beyond 64 bits
        "NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000\n",                                            # no element size
        "NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000 3\n",                                          # an element size that is none
        "NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000 2 7\n",                                        # a field too many
        "NLZMIDX 3 1 10 8 100000000\n0 8 10 00000000 2\n",                                         # a CRC32 beyond 32 bits
        "NLZMIDX 3 1 10 8\n0 8 10 00000000 2\n",                                                   # no CRC32 of the whole file
        "NLZMIDX 4 1 10 8 00000000\n0 8 10 00000000 2\n",
    ]
    for text in damaged:
        p.write_text(text)
        with pytest.raises(ValueError):
            nlzm_amd.read_index_typed(p)


def test_cli_usage_and_conflicts(lib, tmp_path):
    usage = cli().stdout
    assert "\t-elem:E = (this build) c compresses every block's byte planes at element size E (2, 4 or 8)" in usage
    # the lines of -cdc:B, -dedup and -crc are word for word what they were
    assert "\t-cdc:B = (this build) c cuts the blocks by content on the GPU, 2^B bytes on average (B 10 to 30): an edit changes the blocks around it only\n" in usage
    assert "\t-dedup = (this build) with -cdc:B: a block whose bytes an earlier block holds is not compressed again, its stream is a copy (the same container)\n" in usage
    assert ("\t-crc = (this build) c hashes every block on the GPU and keeps the CRC32s in [output].idx (NLZMIDX 2), for one stream too;\n"
            "\t       d / t compare what they decode with an index that holds CRC32s and exit with status -4 if a block differs\n") in usage
    src = tmp_path / "in.bin"
    src.write_bytes(bytes(5000))
    dst = tmp_path / "out.nlzm"
    for flag in ("-elem:3", "-elem:1", "-elem:16", "-elem:", "-elem:4x", "-elem:0"):
        r = cli(flag, "c", src, dst)
        assert r.returncode == 255 and "Error: -elem:E takes E of 2, 4 or 8" in r.stdout and not dst.exists(), (flag, r.stdout)
    for flags in (("-elem:4", "-gpus:1"), ("-gpus:2", "-blocks:2", "-elem:8")):
        r = cli(*flags, "c", src, dst)
        assert r.returncode == 255 and "Error: -elem:E" in r.stdout and "-gpus:g" in r.stdout and not dst.exists(), r.stdout
    r = cli("-elem:4", "h", src)                     # (h needs no device and no blocks)
    assert r.returncode == 0, r.stdout
    if no_gpu():
        for flags in (("-elem:4",), ("-elem:2", "-blocks:3"), ("-elem:8", "-cdc:12")):
            r = cli(*flags, "c", src, dst)
            assert r.returncode == 255 and "Error:" in r.stdout and not dst.exists(), r.stdout


def test_cli_decodes_a_typed_container_on_the_host(tmp_path, container):
    """host-only d and t on the container built above: the raw bytes and `CRC32 ok`; a flipped elem column: the CRC mismatch and exit status -4;
    x and -steps:K: one clear error line and exit status -1"""
    c = container
    f = tmp_path / "c.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    write_index3(tmp_path / "c.nlzm.idx", c)
    raw = b"".join(c["blocks"])
    back = tmp_path / "back.bin"
    r = cli("d", f, back)
    assert r.returncode == 0 and "CRC32 ok (3 blocks)" in r.stdout and "Blocks: 3" in r.stdout, r.stdout
    assert back.read_bytes() == raw
    assert f"Done (output CRC32 {zlib.crc32(raw):X}," in r.stdout
    r = cli("t", f)
    assert r.returncode == 0 and "CRC32 ok (3 blocks)" in r.stdout, r.stdout
    # one block alone (e = 8, the ragged tail): the single-stream path
    one = tmp_path / "one.nlzm"
    one.write_bytes(c["streams"][2])
    (tmp_path / "one.nlzm.idx").write_text(f"NLZMIDX 3 1 {len(c['blocks'][2])} {len(c['streams'][2])} {c['crcs'][2]:08X}\n0 {len(c['streams'][2])} {len(c['blocks'][2])} {c['crcs'][2]:08X} 8\n")
    back1 = tmp_path / "back1.bin"
    r = cli("d", one, back1)
    assert r.returncode == 0 and "CRC32 ok (1 blocks)" in r.stdout and back1.read_bytes() == c["blocks"][2], r.stdout
    # a flipped elem column
    write_index3(tmp_path / "c.nlzm.idx", c, elems=[2, 8, 8])
    r = cli("t", f)
    assert r.returncode == 252 and "CRC32 MISMATCH in block 2" in r.stdout, r.stdout
    back2 = tmp_path / "back2.bin"
    r = cli("d", f, back2)
    assert r.returncode == 252 and "CRC32 MISMATCH in block 2" in r.stdout and back2.read_bytes() != raw, r.stdout
    # x and -steps:K do not read typed blocks
    write_index3(tmp_path / "c.nlzm.idx", c)
    part = tmp_path / "part.bin"
    r = cli("-range:0:10", "x", f, part)
    assert r.returncode == 255 and r.stdout.count("Error:") == 1 and "NLZMIDX 3" in r.stdout and not part.exists(), r.stdout
    r = cli("-gpu", "-steps:2", "t", f)
    assert r.returncode == 255 and r.stdout.count("Error:") == 1 and "NLZMIDX 3" in r.stdout, r.stdout
    # an index that does not fit the file: without it the planes cannot be undone
    write_index3(tmp_path / "c.nlzm.idx", c, n_out=sum(len(s) for s in c["streams"]) + 1)
    back3 = tmp_path / "back3.bin"
    r = cli("d", f, back3)
    assert r.returncode == 255 and "cannot be undone" in r.stdout and not back3.exists(), r.stdout
