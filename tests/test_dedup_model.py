"""CPU suite: the numpy model of the equal-range finder (tests/dedup_model.py) against a byte-at-a-time restatement of the fingerprint rule's
text, the properties the rule promises (a function of bytes and length; keys by position, so exchanged pieces do not collide by construction),
and first_of against brute-force comparison on a few hundred small random range lists over a two-letter alphabet, where equal ranges abound."""
import numpy as np
import pytest

from nlzm_amd import corpus
from tests import dedup_model

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
S = dedup_model.SEGMENT


def slow_mix32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def slow_fingerprint(data: bytes) -> int:
    """the rule as its text reads, one byte at a time, in Python integers"""
    n = len(data)
    acc = 0
    for g in range((n + S - 1) // S):
        seg = data[g * S: (g + 1) * S]
        units = (len(seg) + 15) // 16
        w = [0] * (4 * units)
        for b, byte in enumerate(seg):
            w[b >> 2] |= byte << (8 * (b & 3))
        h = 0
        for u in range(units):
            for j in (4 * u, 4 * u + 2):
                h = (h + ((w[j] + slow_mix32(j + 1)) & M32) * ((w[j + 1] + slow_mix32(j + 2)) & M32)) & M64
        acc = (acc + dedup_model.splitmix64((h + (g + 1) * dedup_model.GOLDEN) & M64)) & M64
    return dedup_model.splitmix64(acc ^ dedup_model.splitmix64(n))


def test_constants():
    assert dedup_model.splitmix64(0) == 0xE220A8397B1DCDAF          # (the generator's first output from state 0, as published)
    assert [int(k) for k in dedup_model.KEYS[:3]] == [slow_mix32(1), slow_mix32(2), slow_mix32(3)]
    assert len(set(dedup_model.KEYS.tolist())) == S // 4             # (mix32 is a bijection: no key is used twice in a segment)
    assert S % 16 == 0


def test_model_against_the_byte_at_a_time_rule():
    rng = np.random.default_rng(corpus.SEED + 100)
    kinds = [rng.integers(0, 256, 2 * S + 31, dtype=np.uint8).tobytes(), corpus.syn_text(2 * S + 31).tobytes(), bytes(2 * S + 31), b"\xff" * (2 * S + 31)]
    lengths = list(range(0, 70)) + [255, 256, 1000, S - 1, S, S + 1, 2 * S + 31]
    for data in kinds:
        for n in lengths:
            assert dedup_model.fingerprint(data[:n]) == slow_fingerprint(data[:n]), n
    assert dedup_model.fingerprint(b"") == dedup_model.splitmix64(dedup_model.splitmix64(0))


def test_a_function_of_bytes_and_length():
    rng = np.random.default_rng(corpus.SEED + 101)
    piece = rng.integers(0, 256, S + 777, dtype=np.uint8)
    buf = np.zeros(4 * S, dtype=np.uint8)
    fps = set()
    for at in (0, 1, 7, 15, 16, 4097):
        buf[:] = rng.integers(0, 256, buf.size, dtype=np.uint8)
        buf[at: at + piece.size] = piece
        fps.add(dedup_model.fingerprints(buf, [(at, piece.size)])[0])
    assert len(fps) == 1
    # the length goes into it: zeros of every length 0 .. 40 (whose padded words are the same within a unit) all differ, and so do their neighbours at S
    zeros = bytes(2 * S)
    lens = list(range(41)) + [S - 1, S, S + 1, 2 * S]
    assert len({dedup_model.fingerprint(zeros[:n]) for n in lens}) == len(lens)


def test_exchanged_pieces_do_not_collide():
    """pages in another order, words in another order, segments in another order: the keys depend on the position, not on it modulo a period"""
    rng = np.random.default_rng(corpus.SEED + 102)
    x = rng.integers(0, 256, 4 * S, dtype=np.uint8)
    base = dedup_model.fingerprint(x)
    for unit in (4, 8, 16, 64, 4096, S):
        for a, b in ((0, 1), (0, 2), (1, 3), (2, (4 * S) // unit - 1)):
            y = x.copy()
            y[a * unit: (a + 1) * unit], y[b * unit: (b + 1) * unit] = x[b * unit: (b + 1) * unit], x[a * unit: (a + 1) * unit]
            assert dedup_model.fingerprint(y) != base, (unit, a, b)
    # a single changed byte anywhere changes it
    for at in (0, 1, 15, 16, S - 1, S, 4 * S - 1):
        y = x.copy()
        y[at] ^= 1
        assert dedup_model.fingerprint(y) != base


def brute_first_of(data: bytes, ranges):
    out = []
    for i, (o, l) in enumerate(ranges):
        out.append(next(j for j in range(i + 1) if ranges[j][1] == l and data[ranges[j][0]: ranges[j][0] + l] == data[o: o + l]))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_first_of_against_brute_force(seed):
    """a hundred range lists a seed over 'ab' strings: up to 40 ranges of 0 .. 6 bytes, overlapping, repeated, unordered"""
    rng = np.random.default_rng(corpus.SEED + 110 + seed)
    dups = 0
    for _ in range(100):
        n = int(rng.integers(0, 60))
        data = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), n).astype(np.uint8)
        k = int(rng.integers(1, 41))
        ranges = []
        for _ in range(k):
            o = int(rng.integers(0, n + 1))
            ranges.append((o, int(rng.integers(0, min(6, n - o) + 1))))
        got = dedup_model.first_of(data, ranges)
        assert got == brute_first_of(data.tobytes(), ranges)
        assert all(f <= i and got[f] == f for i, f in enumerate(got))
        assert dedup_model.distinct(got) == len(set(got))
        assert dedup_model.dup_bytes(got, ranges) == sum(l for i, (_, l) in enumerate(ranges) if got[i] != i)
        fps = dedup_model.fingerprints(data, ranges)
        assert all(fps[i] == fps[f] for i, f in enumerate(got))
        dups += k - dedup_model.distinct(got)
    assert dups > 500
