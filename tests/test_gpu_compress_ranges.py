"""GPU suite (-m gpu): blocks of the caller's choosing (nlzm_hip_compress_ranges*) against the oracle run on every range's bytes, the read side
on what they make, and the command line's -cdc:B.  Every check is exact.  Inputs are at most 600 KB; only streams a compressor made are
handed to the device."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cut_model, oracle_py
from tests.cli_tools import cli

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
HIST = 16


@pytest.fixture(scope="module")
def nine(gpu):
    """300 KB of corpus.mixed and nine ranges for one set: lengths 0, 1, 5, 4,096, one longer than a chunk of its own geometry, one that overlaps
    it, one repeated, one that ends exactly at n; given out of order.  The oracle's streams are made once."""
    data = corpus.mixed(300_000, corpus.SEED + 91)
    n = int(data.size)
    long_len = 40_000
    assert long_len > gpu.geometry(long_len, HIST)["chunk_size"]
    ranges = [(n - 7_000, 7_000), (123_456, 4_096), (n, 0), (50_000, long_len), (70_001, 33_333), (17, 1), (123_456, 4_096), (200_000, 5), (0, 0)]
    return {"data": data, "n": n, "ranges": ranges, "want": [oracle_py.compress(data[o:o + l], HIST) for o, l in ranges]}


def test_nine_ranges_in_one_set(gpu, nine):
    got = gpu.compress_ranges(nine["data"], nine["ranges"], HIST)
    assert gpu.counter("container_sets") == 1
    assert [len(s) for s in got] == [len(s) for s in nine["want"]]
    assert got == nine["want"]


def test_seventy_ranges_run_in_sets(gpu):
    """70 ranges of 0 to 20 KB over 600 KB: more than a launch holds, so consecutive ranges go in sets"""
    data = corpus.mixed(600_000, corpus.SEED + 92)
    rng = np.random.default_rng(corpus.SEED + 93)
    ranges = []
    for i in range(70):
        ln = 0 if i in (3, 40, 69) else int(rng.integers(0, 20_001))
        ranges.append((int(rng.integers(0, data.size - ln + 1)), ln))
    got = gpu.compress_ranges(data, ranges, HIST)
    assert gpu.counter("container_sets") > 1
    for i, ((o, l), s) in enumerate(zip(ranges, got)):
        assert s == oracle_py.compress(data[o:o + l], HIST), i
    # ... and with fewer blocks a set the sets are other ones, the bytes the same
    gpu.set_option("container_set_blocks", 16)
    try:
        again = gpu.compress_ranges(data, ranges, HIST)
        assert gpu.counter("container_sets") == 5 and again == got
    finally:
        gpu.set_option("container_set_blocks", 32)


def test_the_equal_partitions_ranges_give_compress_blocks_bytes(gpu, nine):
    data, n = nine["data"], nine["n"]
    for k in (1, 5, 9):
        ranges = [shard.block_range(n, k, i) for i in range(k)]
        assert gpu.compress_ranges(data, [(lo, hi - lo) for lo, hi in ranges], HIST) == gpu.compress_blocks(data, k, HIST)


def ranges_dev(lib, src, n, ranges, dst, cap):
    k = len(ranges)
    off, ln = (C.c_uint64 * k)(*[o for o, _ in ranges]), (C.c_uint64 * k)(*[l for _, l in ranges])
    blen, got = (C.c_uint64 * k)(), C.c_uint64(0)
    rc = lib.nlzm_hip_compress_ranges_dev(src.data_ptr(), n, k, off, ln, HIST, dst.data_ptr(), cap, blen, C.byref(got))
    return rc, [int(x) for x in blen], int(got.value), int(lib.nlzm_hip_compress_ranges_bound(k, ln))


def test_dev_form_errors_and_the_call_after(gpu, nine):
    """the _dev form on torch tensors with dst_cap exactly the bound; a capacity one short and a range over n return their codes, nothing is
    left open, and the next call works"""
    lib = gpu.load_library()
    n, ranges = nine["n"], nine["ranges"]
    src = torch.zeros(n + 128, dtype=torch.uint8, device="cuda:0")       # (128 readable bytes behind the input)
    src[:n] = torch.from_numpy(nine["data"]).to("cuda:0")
    k = len(ranges)
    bound = int(lib.nlzm_hip_compress_ranges_bound(k, (C.c_uint64 * k)(*[l for _, l in ranges])))
    dst = torch.zeros(bound, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    rc, blen, got, b = ranges_dev(lib, src, n, ranges, dst, bound - 1)
    assert rc == E_CAPACITY and b == bound and b"dst_cap" in lib.nlzm_hip_last_error()
    bad = list(ranges)
    bad[4] = (n - 10, 11)
    rc, _, _, _ = ranges_dev(lib, src, n, bad, dst, bound)
    assert rc == E_ARG and b"range 4 " in lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_blocks_step(0, None, None, None) == E_ARG and b"no open block set" in lib.nlzm_hip_last_error()

    rc, blen, got, _ = ranges_dev(lib, src, n, ranges, dst, bound)
    assert rc == 0, lib.nlzm_hip_last_error()
    assert blen == [len(s) for s in nine["want"]] and got == sum(blen)
    assert dst[:got].cpu().numpy().tobytes() == b"".join(nine["want"])
    assert lib.nlzm_hip_blocks_step(0, None, None, None) == E_ARG         # (the call has closed its set)


def test_round_trip_through_the_read_side(gpu, nine):
    data, ranges, streams = nine["data"], nine["ranges"], nine["want"]
    blob, k = b"".join(streams), len(ranges)
    raw = data.tobytes()
    assert gpu.decompress_blocks(blob, k) == [raw[o:o + l] for o, l in ranges]
    lens, raws = [len(s) for s in streams], [l for _, l in ranges]
    starts = np.concatenate([[0], np.cumsum(raws)]).tolist()
    content = b"".join(raw[o:o + l] for o, l in ranges)
    want = [(0, 10), (starts[3] - 3, 50), (starts[4] + 100, 35_000), (len(content) - 5, 5), (len(content), 0)]
    crcs = [zlib.crc32(raw[o:o + l]) for o, l in ranges]
    assert gpu.read_ranges(blob, want, k, lens, raws, crcs) == [content[o:o + l] for o, l in want]
    assert gpu.check(blob, crcs, k, raws) == k


def test_cli_cdc(gpu, tmp_path):
    """-cdc:12 -crc c, then t, -gpu t, d and x -range across a cut: the output is the input, the index's raw lengths are the model's blocks"""
    data = corpus.mixed(200_000, corpus.SEED + 94)
    raw = data.tobytes()
    src, out = tmp_path / "in.bin", tmp_path / "c.nlzm"
    src.write_bytes(raw)
    r = cli("-window:16", "-cdc:12", "-crc", "c", src, out)
    blocks = cut_model.blocks(len(raw), cut_model.cut_points(data, 12))
    assert r.returncode == 0 and f"Blocks: {len(blocks)} (cut by content)" in r.stdout and "Block index:" in r.stdout, r.stdout
    lens, raws, crcs = nlzm_amd.read_index(str(out) + ".idx")
    assert open(str(out) + ".idx").read().startswith(f"NLZMIDX 2 {len(blocks)} {len(raw)} ")
    assert raws == [l for _, l in blocks] and crcs == [zlib.crc32(raw[o:o + l]) for o, l in blocks]
    blob = out.read_bytes()
    assert sum(lens) == len(blob)
    for i in (0, 1, len(blocks) // 2, len(blocks) - 1):
        at = sum(lens[:i])
        o, l = blocks[i]
        assert blob[at: at + lens[i]] == oracle_py.compress(data[o:o + l], 16), i
    for flags in ((), ("-gpu",)):
        r = cli(*flags, "t", out)
        assert r.returncode == 0 and f"CRC32 ok ({len(blocks)} blocks)" in r.stdout and f"Blocks: {len(blocks)}" in r.stdout, r.stdout
    back = tmp_path / "back.bin"
    r = cli("d", out, back)
    assert r.returncode == 0 and back.read_bytes() == raw, r.stdout
    cut = blocks[3][0]                               # a range across the cut in front of block 3, and one across the last
    part = tmp_path / "part.bin"
    r = cli(f"-range:{cut - 700}:1500", f"-range:{blocks[-1][0] - 1}:2", "x", out, part)
    assert r.returncode == 0 and part.read_bytes() == raw[cut - 700: cut + 800] + raw[blocks[-1][0] - 1: blocks[-1][0] + 1], r.stdout
    # without -crc the index is written too (NLZMIDX 1), and -verify decodes a container that is not the equal partition's
    out2 = tmp_path / "v.nlzm"
    r = cli("-window:16", "-cdc:12", "-verify", "c", src, out2)
    assert r.returncode == 0 and "Verified" in r.stdout and f"Blocks: {len(blocks)} (cut by content)" in r.stdout, r.stdout
    assert open(str(out2) + ".idx").read().startswith(f"NLZMIDX 1 {len(blocks)} {len(raw)} ")
    assert nlzm_amd.read_index(str(out2) + ".idx")[1] == raws and out2.read_bytes() == blob
