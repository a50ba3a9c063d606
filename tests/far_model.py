"""A sparse model of a buffer longer than 2^32 bytes.  TEST INFRASTRUCTURE ONLY.

The buffer is one fill byte everywhere except a few islands of seeded random bytes; the model answers what the range entry points compute --
CRC32, the fingerprint of tests/dedup_model.py, the cut points of tests/cut_model.py -- for any range, without ever holding the buffer:

  read         fill, with the islands laid over it (small ranges only)
  CRC32        zlib over the island bytes; a stretch of z fill bytes is appended with zlib's combine rule, restated here over GF(2)
               (crc(A || B) = x^(8 |B|) * crc(A) + crc(B)), and the CRC of the stretch itself is made by doubling -- never the library's combine
  fingerprint  a whole fill segment has ONE segment_h; the segments an island touches and a ragged last one are hashed from read();
               the term splitmix64(h(g) + (g + 1) * GOLDEN) is vectorised in uint64 over all segments
  cut points   32 fill bytes in a row are no candidate (asserted), so candidates lie only where the 32-byte window holds an island byte:
               cut_model.candidates on every island with 31 bytes of context on either side; the greedy rule restated over that sorted list

`Periodic` is the second kind of buffer the device tests use: one chunk of P bytes repeated, with single bytes altered, for ranges that are
longer than 2^32 and equal.  tests/test_far_model.py holds every answer to the dense models on a buffer of a few hundred KB with the same layout."""
from __future__ import annotations

import zlib

import numpy as np

from tests import cut_model, dedup_model

S = dedup_model.SEGMENT
GOLDEN = np.uint64(dedup_model.GOLDEN)
READ_MAX = 1 << 26          # read() is for small ranges: nobody asks the model for 4 GiB of bytes

# ---- CRC32: zlib's combine over GF(2) -------------------------------------------------------------------------------------------


def _times(mat, vec: int) -> int:
    out, i = 0, 0
    while vec:
        if vec & 1:
            out ^= mat[i]
        vec >>= 1
        i += 1
    return out


def _square(mat):
    return [_times(mat, mat[i]) for i in range(32)]


def crc32_append_len(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC32 of A || B from the CRC32s of A and B and |B|: the operator "shift by one zero bit" is squared up to "shift by one byte",
    then squared once per bit of len_b and applied where that bit is set"""
    if len_b == 0:
        return crc_a
    odd = [0xEDB88320] + [1 << i for i in range(31)]       # one zero bit
    even = _square(odd)                                     # two
    odd = _square(even)                                     # four
    while True:
        even = _square(odd)                                 # (the first time round: eight bits, one byte)
        if len_b & 1:
            crc_a = _times(even, crc_a)
        len_b >>= 1
        if not len_b:
            break
        odd = _square(even)
        if len_b & 1:
            crc_a = _times(odd, crc_a)
        len_b >>= 1
        if not len_b:
            break
    return crc_a ^ crc_b


def crc32_of_fill(fill: int, z: int) -> int:
    """CRC32 of z bytes of `fill`, by doubling"""
    if z <= 1 << 16:
        return zlib.crc32(bytes([fill]) * z)
    half = crc32_of_fill(fill, z // 2)
    both = crc32_append_len(half, half, z // 2)
    return zlib.crc32(bytes([fill]), both) if z & 1 else both


# ---- the fingerprint from a list of segment hashes --------------------------------------------------------------------------------


def splitmix64_vec(x: np.ndarray) -> np.ndarray:
    """dedup_model.splitmix64 on a uint64 array (arithmetic wraps: modulo 2^64)"""
    x = x + GOLDEN
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def fingerprint_of_segments(h: np.ndarray, n: int) -> int:
    """F of a range of n bytes whose segment g has segment_h h[g]"""
    assert h.dtype == np.uint64 and h.size == (n + S - 1) // S
    g1 = np.arange(1, h.size + 1, dtype=np.uint64)
    acc = int(np.sum(splitmix64_vec(h + g1 * GOLDEN), dtype=np.uint64)) if h.size else 0
    return dedup_model.splitmix64(acc ^ dedup_model.splitmix64(n))


# ---- fill and islands ------------------------------------------------------------------------------------------------------------


class Far:
    def __init__(self, n: int, fill: int, islands):
        """islands: (offset, uint8 array), apart from one another and inside [0, n)"""
        self.n, self.fill = int(n), int(fill)
        self.islands = sorted(((int(o), np.ascontiguousarray(b, dtype=np.uint8)) for o, b in islands), key=lambda t: t[0])
        at = 0
        for o, b in self.islands:
            assert at <= o and b.size > 0 and o + b.size <= self.n, (o, b.size)
            at = o + b.size
        self._starts = np.array([o for o, _ in self.islands], dtype=np.int64)
        self._ends = np.array([o + b.size for o, b in self.islands], dtype=np.int64)
        self._fill_h = dedup_model.segment_h(np.full(S, self.fill, dtype=np.uint8))

    def with_islands(self, more):
        return Far(self.n, self.fill, self.islands + list(more))

    def touching(self, off: int, length: int):
        """the islands that meet [off, off + length)"""
        lo = int(np.searchsorted(self._ends, off, side="right"))
        hi = int(np.searchsorted(self._starts, off + length, side="left"))
        return self.islands[lo:hi]

    def read(self, off: int, length: int) -> np.ndarray:
        assert 0 <= off and 0 <= length <= READ_MAX and off + length <= self.n, (off, length)
        out = np.full(length, self.fill, dtype=np.uint8)
        for o, b in self.touching(off, length):
            a, e = max(o, off), min(o + b.size, off + length)
            out[a - off: e - off] = b[a - o: e - o]
        return out

    def crc32(self, off: int, length: int, seed: int = 0) -> int:
        assert 0 <= off and 0 <= length and off + length <= self.n
        crc, at, end = seed, off, off + length
        for o, b in self.touching(off, length):
            a, e = max(o, off), min(o + b.size, end)
            if a > at:
                crc = crc32_append_len(crc, crc32_of_fill(self.fill, a - at), a - at)
            crc = zlib.crc32(b[a - o: e - o].tobytes(), crc)
            at = e
        return crc32_append_len(crc, crc32_of_fill(self.fill, end - at), end - at)

    def fingerprint(self, off: int, length: int) -> int:
        assert 0 <= off and 0 <= length and off + length <= self.n
        nseg = (length + S - 1) // S
        h = np.full(nseg, self._fill_h, dtype=np.uint64)
        own = set()
        for o, b in self.touching(off, length):
            a, e = max(o, off), min(o + b.size, off + length)
            own.update(range((a - off) // S, (e - 1 - off) // S + 1))
        if length % S:
            own.add(nseg - 1)
        for g in own:
            h[g] = dedup_model.segment_h(self.read(off + g * S, min(S, length - g * S)))
        return fingerprint_of_segments(h, length)

    def candidates(self, avg_bits: int) -> np.ndarray:
        """every candidate position of the whole buffer, ascending (int64)"""
        run = np.full(32, self.fill, dtype=np.uint8)
        assert int(cut_model.hashes(run)[31]) >> (32 - avg_bits) != 0, "32 fill bytes are a cut candidate at this avg_bits: choose another fill"
        spans = []                                  # the islands with 31 bytes on either side, merged where those meet
        for o, b in self.islands:
            a, e = max(0, o - 31), min(self.n, o + b.size + 31)
            if spans and a <= spans[-1][1]:
                spans[-1][1] = e
            else:
                spans.append([a, e])
        out = []
        for a, e in spans:
            c = cut_model.candidates(self.read(a, e - a), avg_bits).astype(np.int64) + a       # (positions below a + 31 are left out there:
            out.append(c)                                                                       #  all fill, or below 31 of the buffer)
        return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)

    def cut_points(self, avg_bits: int, min_len: int, max_len: int):
        """(the cuts, the number of candidates): the selection rule of cut_model's docstring, over the sparse list"""
        assert 1 <= avg_bits <= 30 and 32 <= min_len <= max_len <= 1 << 31
        cand = self.candidates(avg_bits)
        bounds = cand + 1
        cuts, s = [], 0
        while self.n - s > min_len:
            hi = min(s + max_len, self.n)
            i = int(np.searchsorted(bounds, s + min_len))
            e = int(bounds[i]) if i < bounds.size and bounds[i] <= hi else hi
            if e >= self.n:
                break
            cuts.append(e)
            s = e
        return cuts, int(cand.size)

    def dense(self) -> np.ndarray:
        """the whole buffer (the scaled-down layout only)"""
        return self.read(0, self.n)


def layout(line: int, tail: int, u: int, fill: int, seed: int) -> Far:
    """n = line + tail bytes of `fill` with four islands, their sizes in units of u bytes: at the very start; straddling line / 2; straddling
    `line` with three units on either side (so at least two whole segments of a range that starts anywhere); ending exactly at n.  No island
    starts or ends on a multiple of 16.  The far buffer is layout(2^32, 2^22, 32 KiB): islands of 64 to 256 KiB."""
    n = line + tail
    rng = np.random.default_rng(seed)
    spans = [(0, 4 * u + 5), (line // 2 - 2 * u - 3, line // 2 + 2 * u + 9), (line - 3 * u - 3, line + 3 * u + 5), (n - 2 * u - 7, n)]
    return Far(n, fill, [(a, rng.integers(0, 256, e - a, dtype=np.uint8)) for a, e in spans])


LINE, TAIL, FILL = 1 << 32, 1 << 22, 0x5A
N = LINE + TAIL


def far(seed: int) -> Far:
    return layout(LINE, TAIL, S, FILL, seed)


PIECE = 2 * S + 31
STRIDE = (PIECE + 255) // 256 * 256 + 256


def with_copies(m: Far, line: int, below: int, above: int):
    """the equal-range finder's material: the PIECE bytes that start S + 11 below the line (inside the island across it) copied to sixteen places
    from `below` and sixteen from `above`, copy j at misalignment j, and one near-copy behind those above that differs in its last byte.
    Returns the model with these islands and {"across": offset, "below": [...], "above": [...], "near": offset}."""
    assert below % 16 == 0 and above % 16 == 0
    at = line - S - 11
    piece = m.read(at, PIECE)
    lo = [below + j * STRIDE + j for j in range(16)]
    hi = [above + j * STRIDE + j for j in range(16)]
    near = above + 16 * STRIDE + 3
    other = piece.copy()
    other[-1] ^= 0x01
    return m.with_islands([(o, piece) for o in lo + hi] + [(near, other)]), {"across": at, "below": lo, "above": hi, "near": near}


def far_with_copies(seed: int):
    return with_copies(far(seed), LINE, LINE - (1 << 21), LINE + (1 << 20))


def edge_ranges(line, n, seg, long=70_001):
    """the shape of the device test's list: starts at line + d, d = -17 .. 17, and at line / 2 + d, with lengths round 16, round the segment and `long`;
    ranges that end at the line, one behind it and at n; empty ranges; the whole buffer and the whole but one byte at either end"""
    out = []
    for mid in (line, line // 2):
        for d in range(-17, 18):
            for j, ln in enumerate((0, 1, 15, 16, 17, seg - 1, seg, seg + 1, long)):
                if (d + j) % 3 == 0 or ln <= 17:
                    out.append((mid + d, ln))
        for ln in (1, 17, seg + 1, 3 * seg + 5):
            out += [(mid - ln, ln), (mid + 1 - ln, ln)]
    for ln in (0, 1, 17, seg + 1, 3 * seg + 5):
        out.append((n - ln, ln))
    return out + [(0, n), (1, n - 2), (line - 5, n - line + 5)]


REGIONS = ("below", "across", "above")


def region_start(line: int, region: str, n: int, mis: int, slot: int) -> int:
    """a 16-byte aligned start in `region` of the line for n bytes, plus mis; `slot` keeps starts of one region apart (below and above)"""
    if region == "below":
        return line - 3 * S + 16 * slot + mis
    if region == "across":
        return line - (n // 2 + 15) // 16 * 16 + mis
    return line + 16 + 16 * slot + mis


def planes_calls(line: int, seg: int):
    """the byte planes' small cases: e in 1, 2, 4, 8; lengths from a few hundred bytes to two segments and a ragged tail; the source below, across and
    above the line and the destination below, across and above it -- all nine pairs -- at misalignments 0, 3 and 9.  One destination range can lie
    across the line at a time, so a call holds three ranges (one source region, the three destination regions): 36 calls of (src_off, dst_off,
    len, e).  The sources lie inside the island across the line (3 S on either side), the destinations below and above 2 MiB off it."""
    lengths = (333, 1000 + 7, seg - 1, seg + 1, seg + 19, 2 * seg + 11)
    calls = []
    for e in (1, 2, 4, 8):
        for mi, mis in enumerate((0, 3, 9)):
            for sreg in REGIONS:
                ranges = []
                for di, dreg in enumerate(REGIONS):
                    n = lengths[(len(calls) + di) % len(lengths)]
                    s = region_start(line, sreg, n, mis, di)
                    d = region_start(line, dreg, n, (3, 9, 0)[mi], 0) + (-(1 << 21) if dreg == "below" else (1 << 21) if dreg == "above" else 0)
                    ranges.append((s, d, n, e))
                calls.append(ranges)
    return calls


# ---- one chunk, repeated ------------------------------------------------------------------------------------------------------------


class Periodic:
    def __init__(self, n: int, chunk, patches=None):
        """x[i] = chunk[i mod P], but for `patches`: {offset: byte}.  P is a multiple of the segment, so that a range that starts on a
        multiple of the segment sees the chunk's own segments in turn."""
        self.n, self.chunk = int(n), np.ascontiguousarray(chunk, dtype=np.uint8)
        self.patches = dict(patches or {})
        assert self.chunk.size % S == 0
        self._h = np.array([dedup_model.segment_h(self.chunk[j: j + S]) for j in range(0, self.chunk.size, S)], dtype=np.uint64)

    def read(self, off: int, length: int) -> np.ndarray:
        assert 0 <= off and 0 <= length <= READ_MAX and off + length <= self.n
        out = self.chunk[(off + np.arange(length, dtype=np.int64)) % self.chunk.size]
        for p, b in self.patches.items():
            if off <= p < off + length:
                out[p - off] = b
        return out

    def fingerprint(self, off: int, length: int) -> int:
        assert off % S == 0 and 0 <= length and off + length <= self.n
        nseg = (length + S - 1) // S
        h = self._h[(off // S + np.arange(nseg, dtype=np.int64)) % self._h.size]
        own = {(p - off) // S for p in self.patches if off <= p < off + length}
        if length % S:
            own.add(nseg - 1)
        for g in own:
            h[g] = dedup_model.segment_h(self.read(off + g * S, min(S, length - g * S)))
        return fingerprint_of_segments(h, length)
