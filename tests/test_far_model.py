"""The sparse model of a far buffer (tests/far_model.py) against the dense models -- zlib.crc32, dedup_model.fingerprint, cut_model.cut_points --
on a buffer of 640 KB with the far buffer's layout: islands at the start, across the middle of the "line", across the line, ending at n.
No GPU; what tests/test_gpu_far.py and the simulator's far mode are held to is held here first."""
import zlib

import numpy as np
import pytest

from tests import cut_model, dedup_model, far_model

S = far_model.S
LINE, TAIL, U = 1 << 19, 1 << 17, 4096
SEED = 20260


@pytest.fixture(scope="module")
def small():
    m = far_model.layout(LINE, TAIL, U, far_model.FILL, SEED)
    return m, m.dense()


def test_append_is_zlibs_combine():
    rng = np.random.default_rng(SEED + 1)
    for la in (0, 1, 7, 1000):
        for lb in (0, 1, 2, 3, 255, 256, 65_537, 1_000_003):
            a, b = rng.integers(0, 256, la, dtype=np.uint8).tobytes(), rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
            for seed in (0, 0xDEADBEEF):
                got = far_model.crc32_append_len(zlib.crc32(a, seed), zlib.crc32(b), lb)
                assert got == zlib.crc32(a + b, seed), (la, lb, seed)
    for z in (0, 1, 65_536, 65_537, 131_075, 5_000_001):
        assert far_model.crc32_of_fill(0x5A, z) == zlib.crc32(b"\x5A" * z), z


def test_append_beyond_4_gib_is_zlib_over_that_many_bytes():
    """the one place where zlib itself reads more than 2^32 bytes: a reused chunk of 64 MiB, 2^32 + 2^22 + 3 bytes in all"""
    z = (1 << 32) + (1 << 22) + 3
    chunk = b"\x5A" * (1 << 26)
    crc = 0x1234
    for _ in range(z >> 26):
        crc = zlib.crc32(chunk, crc)
    crc = zlib.crc32(chunk[: z & ((1 << 26) - 1)], crc)
    assert far_model.crc32_append_len(0x1234, far_model.crc32_of_fill(0x5A, z), z) == crc


def test_layout(small):
    m, x = small
    assert x.size == LINE + TAIL == m.n and [o for o, _ in m.islands][0] == 0 and m.islands[-1][0] + m.islands[-1][1].size == m.n
    assert any(o < LINE // 2 < o + b.size for o, b in m.islands) and any(o + 2 * U < LINE < o + b.size - 2 * U for o, b in m.islands)
    hole = np.ones(m.n, dtype=bool)
    for o, b in m.islands:
        assert np.array_equal(x[o: o + b.size], b) and (o % 16 != 0 or o == 0) and ((o + b.size) % 16 != 0 or o + b.size == m.n)
        hole[o: o + b.size] = False
    assert (x[hole] == m.fill).all() and hole.sum() > m.n // 2
    f = far_model.far(SEED)
    assert f.n == (1 << 32) + (1 << 22) and all(64 << 10 <= b.size <= 256 << 10 for _, b in f.islands)
    o, b = next((o, b) for o, b in f.islands if o < 1 << 32 < o + b.size)
    assert o + 2 * S + 16 <= 1 << 32 and (1 << 32) + 2 * S + 16 <= o + b.size
    assert any(o < 1 << 31 < o + b.size for o, b in f.islands)


def test_read_and_crc32_against_zlib(small):
    m, x = small
    for off, ln in far_model.edge_ranges(LINE, m.n, S):
        assert np.array_equal(m.read(off, ln), x[off: off + ln]), (off, ln)
        assert m.crc32(off, ln) == zlib.crc32(x[off: off + ln]), (off, ln)
    assert m.crc32(0, m.n, 0xCAFE) == zlib.crc32(x, 0xCAFE)
    rng = np.random.default_rng(SEED + 2)
    for _ in range(200):
        off = int(rng.integers(0, m.n))
        ln = int(rng.integers(0, m.n - off + 1))
        assert m.crc32(off, ln, 7) == zlib.crc32(x[off: off + ln], 7), (off, ln)


def test_fingerprint_against_the_dense_model(small):
    m, x = small
    ranges = [r for i, r in enumerate(far_model.edge_ranges(LINE, m.n, S)) if i % 4 == 0 or r[1] > 3 * S]
    rng = np.random.default_rng(SEED + 3)
    for _ in range(40):
        off = int(rng.integers(0, m.n))
        ranges.append((off, int(rng.integers(0, m.n - off + 1))))
    for off, ln in ranges:
        assert m.fingerprint(off, ln) == dedup_model.fingerprint(x[off: off + ln]), (off, ln)
    # the vectorised term is the scalar one
    h = rng.integers(0, 1 << 63, 50, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert [int(v) for v in far_model.splitmix64_vec(h)] == [dedup_model.splitmix64(int(v)) for v in h]


@pytest.mark.parametrize("avg_bits,lo,hi", [(8, 32, 1 << 31), (10, 256, 4096), (12, 4096, 65_536), (12, 1024, 1 << 17), (6, 64, 300)])
def test_cut_points_against_the_dense_model(small, avg_bits, lo, hi):
    m, x = small
    cuts, ncand = m.cut_points(avg_bits, lo, hi)
    assert ncand == cut_model.candidates(x, avg_bits).size
    assert cuts == cut_model.cut_points(x, avg_bits, lo, hi)


def test_a_fill_that_is_a_candidate_is_refused():
    """the model's one assumption: find a byte whose run of 32 is a candidate at avg_bits = 1 and see the assertion"""
    b = next(b for b in range(256) if int(cut_model.hashes(np.full(32, b, dtype=np.uint8))[31]) >> 31 == 0)
    with pytest.raises(AssertionError, match="choose another fill"):
        far_model.layout(LINE, TAIL, U, b, SEED).candidates(1)


def test_one_altered_island_byte_changes_what_it_should(small):
    m, x = small
    o, b = m.islands[2]
    cand = m.candidates(10)
    p = int(cand[(cand >= o) & (cand < o + b.size)][3])         # a candidate position inside the island across the line
    other = b.copy()
    other[p - o] ^= 0x40
    m2 = far_model.Far(m.n, m.fill, [(io, other if io == o else ib) for io, ib in m.islands])
    x2 = x.copy()
    x2[p] ^= 0x40
    assert np.array_equal(m2.dense(), x2)
    for off, ln in [(0, m.n), (p, 1), (p - 5 * S, 6 * S), (p - 100, 101), (o, b.size)]:                     # ranges that hold the byte
        assert m2.crc32(off, ln) == zlib.crc32(x2[off: off + ln]) != m.crc32(off, ln), (off, ln)
        assert m2.fingerprint(off, ln) == dedup_model.fingerprint(x2[off: off + ln]) != m.fingerprint(off, ln), (off, ln)
    for off, ln in [(0, p), (p + 1, m.n - p - 1), (p + 1, 0)]:                                               # and ranges that do not
        assert m2.crc32(off, ln) == m.crc32(off, ln) and m2.fingerprint(off, ln) == m.fingerprint(off, ln), (off, ln)
    assert p not in m2.candidates(10)
    assert m2.cut_points(10, 32, 1 << 31) == (cut_model.cut_points(x2, 10, 32, 1 << 31), cut_model.candidates(x2, 10).size) != m.cut_points(10, 32, 1 << 31)


def test_periodic_against_the_dense_model():
    rng = np.random.default_rng(SEED + 4)
    chunk = rng.integers(0, 256, 2 * S, dtype=np.uint8)
    n = 21 * S + 100
    patch = 17 * S + 5
    m = far_model.Periodic(n, chunk, {patch: int(chunk[patch % chunk.size]) ^ 1})
    x = np.tile(chunk, 11)[:n].copy()
    x[patch] ^= 1
    assert np.array_equal(m.read(0, n), x) and np.array_equal(m.read(patch - 3, 9), x[patch - 3: patch + 6])
    L = 14 * S + 77
    for off in (0, 2 * S, 4 * S, 3 * S, 5 * S):
        assert m.fingerprint(off, L) == dedup_model.fingerprint(x[off: off + L]), off
    assert m.fingerprint(0, L) == m.fingerprint(2 * S, L) != m.fingerprint(4 * S, L)          # (only the third range holds the altered byte)
    assert m.fingerprint(0, L) != m.fingerprint(S, L)


def test_the_far_buffer_itself_is_consistent():
    """at full size there is no dense model; the sparse answers must at least agree with themselves: a CRC32 over all n bytes is the append of
    its parts at any split, a fingerprint over all n is the one made from the segment hashes of read(), and the cut list obeys the rule's bounds"""
    f = far_model.far(SEED)
    whole = f.crc32(0, f.n, 9)
    for k in (1, (1 << 31) + 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, f.n - 1):
        assert far_model.crc32_append_len(f.crc32(0, k, 9), f.crc32(k, f.n - k), f.n - k) == whole, k
    nseg = f.n // S
    h = np.full(nseg, dedup_model.segment_h(np.full(S, f.fill, dtype=np.uint8)), dtype=np.uint64)
    for g in range(nseg):
        if f.touching(g * S, S):
            h[g] = dedup_model.segment_h(f.read(g * S, S))
    acc = 0
    for g in np.flatnonzero(h != h[nseg // 3]).tolist() + [nseg // 3]:
        acc += dedup_model.splitmix64((int(h[g]) + (g + 1) * dedup_model.GOLDEN) & dedup_model.M64)
    fill_term = far_model.splitmix64_vec(h + np.arange(1, nseg + 1, dtype=np.uint64) * far_model.GOLDEN)
    same = np.flatnonzero(h == h[nseg // 3])
    acc += int(np.sum(fill_term[same], dtype=np.uint64)) - int(fill_term[nseg // 3])
    assert f.fingerprint(0, f.n) == dedup_model.splitmix64((acc & dedup_model.M64) ^ dedup_model.splitmix64(f.n))
    cuts, ncand = f.cut_points(12, 4096, 1 << 26)
    edges = [0] + cuts + [f.n]
    assert all(4096 <= b - a <= 1 << 26 for a, b in zip(edges[:-2], edges[1:-1])) and 0 < f.n - cuts[-1] <= 1 << 26
    assert any(c > 1 << 32 for c in cuts) and any(b - a == 1 << 26 for a, b in zip(edges, edges[1:])) and ncand > 100
