"""CPU suite: the numpy model of the content-defined cut rule (tests/cut_model.py) against a byte-at-a-time restatement of the rule's text, the
block-length bounds, the smallest inputs, inputs of equal bytes, and the property the rule is there for: an edit changes the blocks around it
and no others."""
import zlib

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import cut_model

M32 = (1 << 32) - 1


def slow_candidates(data: bytes, avg_bits):
    gear = [cut_model.splitmix64(b) >> 32 for b in range(256)]
    cand = set()
    for p in range(31, len(data)):
        h = 0
        for j in range(32):
            h = (h + (gear[data[p - j]] << j)) & M32
        if h >> (32 - avg_bits) == 0:
            cand.add(p)
    return cand


def slow_cuts(data: bytes, avg_bits, min_len, max_len, cand=None):
    """the rule as its text reads, one byte at a time, in Python integers"""
    n = len(data)
    cand = slow_candidates(data, avg_bits) if cand is None else cand
    cuts, s = [], 0
    while n - s > min_len:
        hi = min(s + max_len, n)
        e = next((b for b in range(s + min_len, hi + 1) if b - 1 in cand), hi)
        if e >= n:
            break
        cuts.append(e)
        s = e
    return cuts, sorted(cand)


def rolling_hashes(data: bytes):
    """h = (h << 1) + G[byte]: the gear hash the sum is"""
    gear = [cut_model.splitmix64(b) >> 32 for b in range(256)]
    h, out = 0, []
    for b in data:
        h = ((h << 1) + gear[b]) & M32
        out.append(h)
    return out


def test_table():
    assert cut_model.splitmix64(0) == 0xE220A8397B1DCDAF          # (the generator's first output from state 0, as published)
    assert cut_model.GEAR[0] == 0xE220A839 and len(set(cut_model.GEAR.tolist())) == 256


@pytest.mark.parametrize("avg_bits", [1, 4, 8])
def test_model_against_the_byte_at_a_time_rule(avg_bits):
    rng = np.random.default_rng(corpus.SEED + 70 + avg_bits)
    inputs = [rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), corpus.syn_text(3000).tobytes(), bytes(700), b"\xff" * 700, b"ab" * 400]
    for data in inputs:
        known = slow_candidates(data, avg_bits)
        for min_len, max_len in ((32, 32), (32, 100), (40, 1000), (64, 1 << 31)):
            cuts, cand = slow_cuts(data, avg_bits, min_len, max_len, known)
            assert cut_model.candidates(data, avg_bits).tolist() == cand
            assert cut_model.cut_points(data, avg_bits, min_len, max_len) == cuts
        h = cut_model.hashes(data).tolist()
        assert h[31:] == rolling_hashes(data)[31:]


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33])
def test_smallest_inputs(n):
    data = np.random.default_rng(corpus.SEED + 71).integers(0, 256, 64, dtype=np.uint8).tobytes()[:n]
    for avg_bits in (1, 4, 12):
        got = cut_model.cut_points(data, avg_bits, 32, 64)
        assert got == slow_cuts(data, avg_bits, 32, 64)[0]
        assert got in ([], [32])                    # (only 33 bytes can be cut, at 32, when position 31 is a candidate)
        assert cut_model.blocks(n, got)[0][0] == 0 and sum(l for _, l in cut_model.blocks(n, got)) == n
    assert cut_model.cut_points(b"", 12) == [] and cut_model.blocks(0, []) == [(0, 0)]


def test_block_length_bounds():
    data = corpus.mixed(300_000, corpus.SEED + 72)
    for avg_bits, min_len, max_len in ((1, 32, 32), (4, 32, 64), (10, None, None), (12, None, None), (12, 100, 2000), (14, 32, 1 << 31)):
        cuts = cut_model.cut_points(data, avg_bits, min_len, max_len)
        lo, hi = cut_model.defaults(avg_bits) if min_len is None else (min_len, max_len)
        bl = cut_model.blocks(data.size, cuts)
        assert cuts == sorted(set(cuts)) and all(0 < c < data.size for c in cuts)
        assert all(lo <= l <= hi for _, l in bl[:-1]) and 0 < bl[-1][1] <= hi
        assert sum(l for _, l in bl) == data.size
    assert cut_model.defaults(12) == (1 << 10, 1 << 14) and cut_model.defaults(4) == (32, 64) and cut_model.defaults(1) == (32, 32) and cut_model.defaults(30) == (1 << 28, 1 << 31)


def test_equal_bytes():
    """every position has the same hash: all are candidates or none is, and the blocks are min_len or max_len long"""
    for byte in (0, 0xFF, 0x41):
        data = bytes([byte]) * 10_000
        for avg_bits in (1, 2, 4, 12):
            c = cut_model.candidates(data, avg_bits)
            assert c.size in (0, len(data) - 31)
            cuts = cut_model.cut_points(data, avg_bits, 40, 1000)
            step = 40 if c.size else 1000
            assert cuts == list(range(step, len(data), step))


def test_an_edit_changes_the_blocks_around_it_only():
    """corpus.mixed(2,000,000), avg_bits 14 with its default lengths, 1,000 random bytes inserted at 1,000,000: at most 3 blocks of the edited
    input have a CRC32 that no block of the original has.  (The model gives 1; the equal partition would give about half of all blocks.)"""
    data = corpus.mixed(2_000_000, corpus.SEED + 77).tobytes()
    ins = np.random.default_rng(corpus.SEED + 79).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    edited = data[:1_000_000] + ins + data[1_000_000:]
    a = cut_model.blocks(len(data), cut_model.cut_points(data, 14))
    b = cut_model.blocks(len(edited), cut_model.cut_points(edited, 14))
    assert 60 <= len(a) <= 250
    have = {zlib.crc32(data[o:o + l]) for o, l in a}
    new = [i for i, (o, l) in enumerate(b) if zlib.crc32(edited[o:o + l]) not in have]
    print(f"blocks {len(a)} -> {len(b)}, new in the edited input: {len(new)}")
    assert len(new) <= 3
