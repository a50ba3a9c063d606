"""CPU suite: the range reader's entry points without a device, its counters' names, its gather kernel's ISA, nlzm_amd.read_index, and the
command line's `x` on the host path (`-gpu x` shares the plan's arithmetic and the index code and is run by tests/test_gpu_range.py).
Streams are the oracle's, the index is written here, the CRCs are zlib's."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import nlzm_amd
from nlzm_amd import corpus
from tests import oracle_py
from tests.cli_tools import cli, write_index

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
E_NODEVICE = -2
STATUS_CRC = 256 - 4                                  # the command line's -4
COUNTERS = ("range_blocks_decoded", "range_blocks_direct", "range_blocks_checked", "range_decoded_bytes", "range_returned_bytes",
            "range_scratch_bytes", "range_pieces", "range_us")


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_symbols_are_exported(lib):
    for name in ("nlzm_hip_read_ranges_dev", "nlzm_hip_read_ranges"):
        assert name in nlzm_amd.ABI_SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    assert "int nlzm_hip_read_ranges_dev(" in header and "int nlzm_hip_read_ranges(" in header


def test_range_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 64)()
    n, bad = C.c_uint64(0), C.c_uint32(0)
    one, zero = (C.c_uint64 * 1)(8), (C.c_uint64 * 1)(0)
    for name in ("nlzm_hip_read_ranges", "nlzm_hip_read_ranges_dev"):
        assert getattr(lib, name)(buf, 8, 1, one, one, None, 1, zero, one, buf, 64, C.byref(n), C.byref(bad)) == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.read_ranges(bytes.fromhex("000a000e00000000"), [(0, 0)])
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.read_range(bytes.fromhex("000a000e00000000"), 0, 0)


def test_range_counters_are_known_names(lib):
    v = C.c_uint64(0)
    for key in COUNTERS:
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert lib.nlzm_hip_get_counter(b"range_chunk_bytes", C.byref(v)) == 0 and v.value >= 1024 and v.value % 1024 == 0
    assert lib.nlzm_hip_get_counter(b"range_no_such", C.byref(v)) != 0


def test_gather_kernel_has_no_scratch_flat_or_calls():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "asmcheck-range"], capture_output=True, text=True)
    assert r.returncode == 0 and "asmcheck-range: ok" in r.stdout, r.stdout + r.stderr


def test_library_has_the_gather_kernel(lib):
    assert b"range_gather_kernel" in open(nlzm_amd.LIB_PATH, "rb").read()


# ---- the container: five blocks, the third of raw length 0 ----

SIZES = [60_000, 45_001, 0, 70_003, 30_000]


@pytest.fixture(scope="module")
def container(lib):
    data = corpus.mixed(sum(SIZES), corpus.SEED + 51)
    raw = data.tobytes()
    starts = [sum(SIZES[:i]) for i in range(len(SIZES) + 1)]
    blocks = [raw[starts[i]:starts[i + 1]] for i in range(len(SIZES))]
    streams = [oracle_py.compress(np.frombuffer(b, dtype=np.uint8), 17) for b in blocks]
    return {"data": raw, "starts": starts, "streams": streams, "crcs": [zlib.crc32(b) for b in blocks], "whole": zlib.crc32(raw)}


def test_read_index(tmp_path, container):
    c = container
    p = tmp_path / "c.idx"
    lens = [len(s) for s in c["streams"]]
    write_index(p, c["streams"], SIZES, c["crcs"], c["whole"])
    assert nlzm_amd.read_index(p) == (lens, SIZES, c["crcs"])
    write_index(p, c["streams"], SIZES, c["crcs"], c["whole"], version=1)
    assert nlzm_amd.read_index(p) == (lens, SIZES, None)
    # raw lengths that do not sum to n_in; block lengths that do not sum to n_out; a gap between two blocks
    for kw in ({"n_in": sum(SIZES) + 1}, {"n_in": sum(SIZES) - 1}, {"n_out": sum(lens) + 1}):
        write_index(p, c["streams"], SIZES, c["crcs"], c["whole"], **kw)
        with pytest.raises(ValueError):
            nlzm_amd.read_index(p)
    offs = [sum(lens[:i]) for i in range(len(lens))]
    write_index(p, c["streams"], SIZES, c["crcs"], c["whole"], offs=offs[:2] + [offs[2] + 1] + offs[3:])
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)
    # an off + len that wraps 64 bits: two blocks, the second's length 2^64 - (its offset) + 8 taken modulo 2^64
    M = 1 << 64
    p.write_text(f"NLZMIDX 1 2 100 {M - 1}\n0 50 60\n50 {M - 40} 40\n")
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)
    p.write_text(f"NLZMIDX 1 2 {M - 1} 100\n0 50 {M - 5}\n50 50 10\n")          # raw lengths whose sum wraps
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)
    p.write_text(f"NLZMIDX 1 1 10 {M + 8}\n0 {M + 8} 10\n")                       # a field beyond 64 bits
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)
    p.write_text("NLZMIDX 3 1 10 8\n0 8 10\n")
    with pytest.raises(ValueError):
        nlzm_amd.read_index(p)


def setup(tmp_path, c, crcs=None, cut=None):
    f = tmp_path / "c.nlzm"
    blob = b"".join(c["streams"])
    f.write_bytes(blob if cut is None else blob[:cut])
    write_index(tmp_path / "c.nlzm.idx", c["streams"], SIZES, c["crcs"] if crcs is None else crcs, c["whole"])
    return f


def x(f, out, ranges, *flags):
    return cli(*flags, *[f"-range:{o}:{l}" for o, l in ranges], "x", f, out)


def slices(c, ranges):
    return b"".join(c["data"][o:o + l] for o, l in ranges)


def test_cli_x_ranges(tmp_path, container):
    c = container
    st, total = c["starts"], sum(SIZES)
    f = setup(tmp_path, c)
    sets = {
        "inside one block": ([(1000, 4096), (st[3] + 5, 77)], 2, 0),
        "across three blocks, over the block of raw length 0": ([(st[1] + 40_000, 5001 + 70_003 + 10)], 3, 2),      # (block 2 to its end, block 4 whole)
        "empty ranges": ([(0, 0), (total, 0), (st[2], 0), (777, 0)], 0, 0),
        "the last byte": ([(total - 1, 1)], 1, 1),
        "the whole container, a repeat, an overlap, out of order": ([(0, total), (st[4], 100), (st[4], 100), (50, 100), (10, 100)], 4, 4),
    }
    for what, (ranges, read, full) in sets.items():
        out = tmp_path / "o.bin"
        r = x(f, out, ranges)
        assert r.returncode == 0, (what, r.stdout + r.stderr)
        assert out.read_bytes() == slices(c, ranges), what
        assert f"Blocks: 5, {read} of them read" in r.stdout and f"CRC32 ok ({full} of {read} blocks read in full)" in r.stdout, (what, r.stdout)
        out.unlink()
    # an existing output is refused, like d; a range past the end is an error; so is one whose off + len wraps
    out = tmp_path / "o.bin"
    out.write_bytes(b"keep")
    r = x(f, out, [(0, 1)])
    assert r.returncode == 255 and "already exists" in r.stdout and out.read_bytes() == b"keep"
    out.unlink()
    for bad in ((total, 1), (total - 1, 2), ((1 << 64) - 1, 2)):
        r = x(f, out, [bad])
        assert r.returncode == 255 and "runs over" in r.stdout and not out.exists(), r.stdout
    # a version-1 index: the same bytes, nothing said about CRCs
    write_index(tmp_path / "c.nlzm.idx", c["streams"], SIZES, c["crcs"], c["whole"], version=1)
    r = x(f, out, [(st[3] - 10, 20)])
    assert r.returncode == 0 and "CRC32" not in r.stdout.replace("output CRC32", "") and out.read_bytes() == slices(c, [(st[3] - 10, 20)]), r.stdout


def test_cli_x_wrong_crc(tmp_path, container):
    c = container
    st = c["starts"]
    crcs = list(c["crcs"])
    crcs[3] ^= 0x00010000                                  # block 4, counted from 1
    f = setup(tmp_path, c, crcs=crcs)
    out = tmp_path / "o.bin"
    ranges = [(st[3] + 100, SIZES[3] - 100)]               # to the block's last byte: read in full
    r = x(f, out, ranges)
    assert r.returncode == STATUS_CRC, (r.returncode, r.stdout)
    assert f"CRC32 MISMATCH in block 4 (index says {crcs[3]:08X}, decoded {c['crcs'][3]:08X})" in r.stdout and "CRC32 ok" not in r.stdout, r.stdout
    assert out.read_bytes() == slices(c, ranges)           # what decoded is written all the same
    out.unlink()
    ranges = [(st[3] + 100, SIZES[3] - 101), (st[4], SIZES[4])]      # one byte short of its end: read in part, the wrong CRC goes unnoticed
    r = x(f, out, ranges)
    assert r.returncode == 0 and "CRC32 ok (1 of 2 blocks read in full)" in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    assert out.read_bytes() == slices(c, ranges)


def test_cli_x_truncated_container(tmp_path, container):
    """only the needed blocks' byte spans are read: a file cut off behind them still serves the range, one cut inside them does not"""
    c = container
    st = c["starts"]
    lens = [len(s) for s in c["streams"]]
    f = setup(tmp_path, c, cut=sum(lens[:2]) + 3)
    out = tmp_path / "o.bin"
    ranges = [(st[1] - 50, 100), (st[2] - 1, 1)]
    r = x(f, out, ranges)
    assert r.returncode == 0 and "Blocks: 5, 2 of them read" in r.stdout, r.stdout
    assert out.read_bytes() == slices(c, ranges)
    out.unlink()
    r = x(f, out, [(st[3], 10)])
    assert r.returncode == 255 and "cut off inside block 4" in r.stdout and not out.exists(), r.stdout


def test_cli_x_without_an_index(tmp_path, container):
    c = container
    st = c["starts"]
    f = tmp_path / "n.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    out = tmp_path / "o.bin"
    ranges = [(st[1] + 7, 50_000), (3, 5)]
    r = x(f, out, ranges)
    assert r.returncode == 0 and "no usable" in r.stdout and "CRC32 ok" not in r.stdout, r.stdout
    assert out.read_bytes() == slices(c, ranges)


def test_cli_usage_and_bad_flag(lib):
    r = cli()
    assert "Commands:" in r.stdout and "-range:off:len" in r.stdout
    for bad in ("-range:5", "-range:5:", "-range::5", "-range:5:6x", "-range:-1:2", "-range:1:-2", "-range: 1:2", "-range:+1:2", "-range:18446744073709551616:1",
                "-range:1:99999999999999999999"):
        r = cli(bad, "x", "a", "b")
        assert r.returncode == 255 and "Unrecognized flag" in r.stdout, (bad, r.stdout)
