"""GPU suite (-m gpu): the equal-range finder on the device (nlzm_hip_equal_ranges*) against the numpy model (tests/dedup_model.py), the compress
path with option "dedup_ranges" against the same call without it and against the oracle run on every range's bytes, and the command line's
-dedup.  Every check is exact.  Inputs are at most 600 KB; the kernels' bounds are held on the CPU (tests/test_dedup_sim.py), and only streams a
compressor made are handed to the device."""
import ctypes as C
import re

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus
from tests import cut_model, dedup_model, oracle_py
from tests.cli_tools import cli

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
HIST = 16


@pytest.fixture(scope="module")
def pieces(gpu):
    """One buffer of about 270 KB built from pieces, and a range list over it: two copies of 2S + 31 random bytes at misalignments 3 and 9, whose
    prefixes give duplicates of the lengths 0, 1, 15, 16, 17, S - 1, S, S + 1, 2S + 31 and, shifted by 0 .. 15, at every misalignment; four
    near-copies of the first S + 1 bytes that differ in only the first byte, only the last, or the byte on either side of the chunk boundary;
    overlapping ranges of zeros; a repeated (off, len); several empties.  The model's answers are made once."""
    S = gpu.counter("dedup_segment_bytes")
    assert S == dedup_model.SEGMENT
    rng = np.random.default_rng(corpus.SEED + 140)
    P = rng.integers(0, 256, 2 * S + 31, dtype=np.uint8)
    room = (P.size + 255) // 256 * 256
    near = (S + 1 + 255) // 256 * 256 + 256
    A, B = 3, room + 256 + 9
    Q = [B + room + 256 + i * near + m for i, m in enumerate((1, 6, 11, 14))]
    Z = Q[-1] + near
    flat = rng.integers(1, 256, Z + 5120, dtype=np.uint8)
    flat[A: A + P.size] = P
    flat[B: B + P.size] = P
    for q in Q:
        flat[q: q + S + 1] = P[: S + 1]
    flat[Q[0]] ^= 0x01
    flat[Q[1] + S] ^= 0x80               # the last byte
    flat[Q[2] + S - 1] ^= 0x10           # the last byte of the first chunk
    flat[Q[3] + S] ^= 0x04               # the first byte of the second chunk ... which is Q[1]'s spot with another bit
    flat[Z: Z + 5000] = 0
    n = int(flat.size)
    ranges = []
    for L in (0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S + 31):
        ranges += [(A, L), (B, L)]
    ranges += [(q, S + 1) for q in Q]
    for j in range(16):
        ranges += [(B + 40 + j, 100 + j), (A + 40 + j, 100 + j)]
    ranges += [(Z, 3000), (Z + 1, 3000), (Z + 17, 3000), (Z + 17, 2999)]
    ranges += [(A + 50, 1234), (n, 0), (A + 50, 1234), (777, 0), (A + 51, 1234)]
    first = dedup_model.first_of(flat, ranges)
    assert dedup_model.distinct(first) <= len(ranges) - 30 and len({flat[q: q + S + 1].tobytes() for q in Q}) == 4
    dev = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 256 == 0
    return {"S": S, "flat": flat, "n": n, "dev": dev, "ranges": ranges, "first": first, "fps": dedup_model.fingerprints(flat, ranges)}


def equal_ranges_c(lib, form, ptr, n, ranges, want_fp=True):
    k = len(ranges)
    off, ln = (C.c_uint64 * k)(*[o for o, _ in ranges]), (C.c_uint64 * k)(*[l for _, l in ranges])
    first, fp = (C.c_uint32 * k)(*([0xDEAD] * k)), (C.c_uint64 * k)()
    rc = form(ptr, n, k, off, ln, first, fp if want_fp else None)
    return rc, [int(x) for x in first], [int(x) for x in fp]


def test_equal_ranges_against_the_model(gpu, pieces):
    """first_of and the fingerprints through the _dev form, the host form and the binding; the counters of the call"""
    lib = gpu.load_library()
    flat, n, ranges = pieces["flat"], pieces["n"], pieces["ranges"]
    rc, first, fps = equal_ranges_c(lib, lib.nlzm_hip_equal_ranges_dev, pieces["dev"].data_ptr(), n, ranges)
    assert rc == 0, lib.nlzm_hip_last_error()
    assert fps == pieces["fps"]
    assert first == pieces["first"]
    assert gpu.counter("dedup_distinct") == dedup_model.distinct(first) and gpu.counter("dedup_dup_bytes") == dedup_model.dup_bytes(first, ranges)
    assert gpu.counter("dedup_rounds") == 1 and gpu.counter("dedup_pairs") > 0 and gpu.counter("dedup_compared_bytes") > 0 and gpu.counter("dedup_us") > 0
    rc, first, _ = equal_ranges_c(lib, lib.nlzm_hip_equal_ranges_dev, pieces["dev"].data_ptr(), n, ranges, want_fp=False)
    assert rc == 0 and first == pieces["first"]
    rc, first, fps = equal_ranges_c(lib, lib.nlzm_hip_equal_ranges, flat.ctypes.data, n, ranges)
    assert rc == 0 and (first, fps) == (pieces["first"], pieces["fps"])
    got_fp = []
    assert gpu.equal_ranges(flat, ranges, got_fp) == pieces["first"] and got_fp == pieces["fps"]
    assert gpu.equal_ranges(flat.tobytes(), ranges[:1]) == [0]
    assert gpu.equal_ranges(b"", [(0, 0), (0, 0)]) == [0, 0]


@pytest.mark.parametrize("bits", [0, 2])
def test_collision_rounds(gpu, pieces, bits):
    """the same list with every fingerprint cut to `bits` bits: the same first_of, in more than one round (five contents of S + 1 bytes cannot have
    four fingerprints of two bits)"""
    gpu.set_option("test_dedup_hash_bits", bits)
    try:
        assert gpu.equal_ranges(pieces["flat"], pieces["ranges"]) == pieces["first"]
        assert gpu.counter("dedup_rounds") > 1
        assert gpu.counter("dedup_distinct") == dedup_model.distinct(pieces["first"])
    finally:
        gpu.set_option("test_dedup_hash_bits", 64)


def ranges_dev(lib, src, n, ranges, dst, cap):
    k = len(ranges)
    off, ln = (C.c_uint64 * k)(*[o for o, _ in ranges]), (C.c_uint64 * k)(*[l for _, l in ranges])
    blen, got = (C.c_uint64 * k)(), C.c_uint64(0)
    rc = lib.nlzm_hip_compress_ranges_dev(src.data_ptr(), n, k, off, ln, HIST, dst.data_ptr(), cap, blen, C.byref(got))
    return rc, [int(x) for x in blen], int(got.value), int(lib.nlzm_hip_compress_ranges_bound(k, ln))


@pytest.fixture(scope="module")
def awkward(gpu):
    """300 KB of corpus.mixed and test_gpu_compress_ranges.py's kind of list -- lengths 0, 1, 5, 4,096, one longer than a chunk of its own geometry, one
    that overlaps it, one repeated, one that ends at n, out of order -- plus three copies of one 5 KB piece at different alignments, a near-copy one
    byte off and two empties.  The oracle's streams are made once, one per distinct content."""
    data = corpus.mixed(300_000, corpus.SEED + 141).copy()
    n = int(data.size)
    piece = data[10_000: 15_000].copy()
    data[220_003: 225_003] = piece
    data[260_007: 265_007] = piece
    data[280_001: 285_001] = piece
    data[280_001 + 2_500] ^= 0x20
    ranges = [(n - 7_000, 7_000), (123_456, 4_096), (n, 0), (50_000, 40_000), (70_001, 33_333), (17, 1), (123_456, 4_096), (200_000, 5), (0, 0),
              (260_007, 5_000), (10_000, 5_000), (5, 0), (280_001, 5_000), (220_003, 5_000), (n, 0)]
    first = dedup_model.first_of(data, ranges)
    assert dedup_model.distinct(first) == 9
    made = {}
    want = [made.setdefault(f, oracle_py.compress(data[o:o + l], HIST)) if f == i else made[f] for i, ((o, l), f) in enumerate(zip(ranges, first))]
    return {"data": data, "n": n, "ranges": ranges, "first": first, "want": want}


def test_awkward_ranges_with_duplicates(gpu, awkward):
    data, ranges, want = awkward["data"], awkward["ranges"], awkward["want"]
    plain = gpu.compress_ranges(data, ranges, HIST)
    assert gpu.counter("container_sets") == 1
    deduped = gpu.compress_ranges(data, ranges, HIST, dedup=True)
    assert gpu.counter("container_sets") == 1 and gpu.counter("dedup_ranges") == 0
    assert [len(s) for s in deduped] == [len(s) for s in plain] == [len(s) for s in want]
    assert deduped == plain
    assert deduped == want
    assert gpu.counter("dedup_distinct") == dedup_model.distinct(awkward["first"]) and gpu.counter("dedup_rounds") == 1
    assert gpu.counter("dedup_dup_bytes") == dedup_model.dup_bytes(awkward["first"], ranges)
    assert gpu.stats()["in_bytes"] == sum(l for i, (_, l) in enumerate(ranges) if awkward["first"][i] == i)      # (the streams that were compressed)


def test_seventy_ranges_twenty_distinct(gpu):
    """70 ranges that hold 20 contents, each content stored at two places of the buffer: with the option one set of 20 streams, without it sets of
    70; the same bytes, and the read side gives back every range's bytes"""
    rng = np.random.default_rng(corpus.SEED + 142)
    src = corpus.mixed(200_000, corpus.SEED + 143)
    flat = np.zeros(200_000, dtype=np.uint8)
    places = []
    at = 0
    for p in range(20):
        ln = 0 if p == 7 else int(rng.integers(1, 4_001))
        o = int(rng.integers(0, src.size - ln + 1))
        two = []
        for _ in range(2):
            at += int(rng.integers(1, 40))
            flat[at: at + ln] = src[o: o + ln]
            two.append((at, ln))
            at += ln
        places.append(two)
    order = list(range(20)) + [int(x) for x in rng.integers(0, 20, 50)]
    ranges = [places[p][int(rng.integers(0, 2))] for p in order]
    first = dedup_model.first_of(flat, ranges)
    assert dedup_model.distinct(first) == 20 and len(ranges) == 70
    deduped = gpu.compress_ranges(flat, ranges, HIST, dedup=True)
    assert gpu.counter("container_sets") == 1 and gpu.counter("dedup_distinct") == 20
    plain = gpu.compress_ranges(flat, ranges, HIST)
    assert gpu.counter("container_sets") > 1
    assert deduped == plain
    raw = flat.tobytes()
    assert gpu.decompress_blocks(b"".join(deduped), 70) == [raw[o:o + l] for o, l in ranges]


def test_no_duplicates_runs_what_runs_without_the_option(gpu, awkward):
    data, ranges, first, want = awkward["data"], awkward["ranges"], awkward["first"], awkward["want"]
    own = [i for i, f in enumerate(first) if f == i and ranges[i][1] <= 7_000]
    distinct = [ranges[i] for i in own]
    assert len(distinct) >= 6 and dedup_model.distinct(dedup_model.first_of(data, distinct)) == len(distinct)
    got = gpu.compress_ranges(data, distinct, HIST, dedup=True)
    assert gpu.counter("dedup_distinct") == len(distinct) and gpu.counter("dedup_dup_bytes") == 0 and gpu.counter("container_sets") == 1
    assert gpu.counter("dedup_gather_us") == 0           # (nothing was placed: the streams were written where they lie)
    assert got == [want[i] for i in own]


def test_errors_with_the_option_on_and_the_call_after(gpu, awkward):
    """the _dev form on torch tensors with the option on: a capacity one short and a range over n return their codes, nothing is left open, and
    the next call works, with dst_cap exactly the bound"""
    lib = gpu.load_library()
    n, data = awkward["n"], awkward["data"]
    ranges = [(10_000, 5_000), (17, 1), (220_003, 5_000), (n, 0), (280_001, 5_000), (260_007, 5_000), (0, 0)]
    want = [awkward["want"][awkward["ranges"].index(r)] for r in ranges]
    src = torch.zeros(n + 128, dtype=torch.uint8, device="cuda:0")       # (128 readable bytes behind the input)
    src[:n] = torch.from_numpy(data).to("cuda:0")
    k = len(ranges)
    bound = int(lib.nlzm_hip_compress_ranges_bound(k, (C.c_uint64 * k)(*[l for _, l in ranges])))
    dst = torch.zeros(bound, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.set_option("dedup_ranges", 1)
    try:
        rc, _, _, b = ranges_dev(lib, src, n, ranges, dst, bound - 1)
        assert rc == E_CAPACITY and b == bound and b"dst_cap" in lib.nlzm_hip_last_error()
        bad = list(ranges)
        bad[4] = (n - 10, 11)
        rc, _, _, _ = ranges_dev(lib, src, n, bad, dst, bound)
        assert rc == E_ARG and b"range 4 " in lib.nlzm_hip_last_error()
        assert lib.nlzm_hip_blocks_step(0, None, None, None) == E_ARG and b"no open block set" in lib.nlzm_hip_last_error()
        rc, blen, got, _ = ranges_dev(lib, src, n, ranges, dst, bound)
        assert rc == 0, lib.nlzm_hip_last_error()
        assert blen == [len(s) for s in want] and got == sum(blen)
        assert dst[:got].cpu().numpy().tobytes() == b"".join(want)
        assert gpu.counter("dedup_distinct") == 4 and gpu.counter("dedup_gather_us") > 0
        assert lib.nlzm_hip_blocks_step(0, None, None, None) == E_ARG         # (the call has closed its set)
    finally:
        gpu.set_option("dedup_ranges", 0)


def test_cli_dedup(gpu, tmp_path):
    """-dedup -cdc:10 c on A + B + A' + A (A: 40 KB of text, A': A with 100 bytes inserted): the container and the index are byte for byte those
    without -dedup, the printed count is the model's, and t passes"""
    A = corpus.syn_text(40_000).tobytes()
    B = corpus.mixed(30_000, corpus.SEED + 144).tobytes()
    ins = np.random.default_rng(corpus.SEED + 145).integers(0, 256, 100, dtype=np.uint8).tobytes()
    raw = A + B + A[:20_000] + ins + A[20_000:] + A
    data = np.frombuffer(raw, dtype=np.uint8)
    blocks = cut_model.blocks(len(raw), cut_model.cut_points(data, 10))
    first = dedup_model.first_of(data, blocks)
    d = len(blocks) - dedup_model.distinct(first)
    assert d >= 1
    src, plain, dedup = tmp_path / "in.bin", tmp_path / "plain.nlzm", tmp_path / "dedup.nlzm"
    src.write_bytes(raw)
    r = cli("-window:16", "-dedup", "-cdc:10", "-crc", "c", src, dedup)
    assert r.returncode == 0 and f"Blocks: {len(blocks)} (cut by content)" in r.stdout, r.stdout
    m = re.search(r"^Duplicates: (\d+) of (\d+) blocks \((\d+) bytes\) not compressed again$", r.stdout, re.M)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (d, len(blocks), dedup_model.dup_bytes(first, blocks)), r.stdout
    r = cli("-window:16", "-cdc:10", "-crc", "c", src, plain)
    assert r.returncode == 0 and "Duplicates:" not in r.stdout, r.stdout
    assert dedup.read_bytes() == plain.read_bytes()
    assert open(str(dedup) + ".idx", "rb").read() == open(str(plain) + ".idx", "rb").read()
    r = cli("t", dedup)
    assert r.returncode == 0 and f"CRC32 ok ({len(blocks)} blocks)" in r.stdout, r.stdout
