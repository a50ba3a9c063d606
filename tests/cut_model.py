"""The content-defined cut rule restated in numpy, independently of the C++ (nlzm_amd/csrc/nlzm_cut.h): what tests/test_cut_model.py holds
to a byte-at-a-time restatement, and what the simulator harness (tests/test_cut_sim.py) and the device (tests/test_gpu_cut.py) are held to.

  table       G[b] = the upper 32 bits of splitmix64(b), b = 0 .. 255
  hash        h(p) = sum over j = 0 .. 31 of G[x[p - j]] << j, modulo 2^32, for p >= 31 (the gear hash h = (h << 1) + G[byte])
  candidate   p where the top avg_bits bits of h(p) are zero; its boundary is p + 1
  selection   s = 0; while n - s > min_len: e = the first candidate boundary in [s + min_len, min(s + max_len, n)], or that upper end;
              stop if e >= n; record the cut e; s = e
"""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


GEAR = np.array([splitmix64(b) >> 32 for b in range(256)], dtype=np.uint32)


def defaults(avg_bits: int):
    """(min_len, max_len) where the caller gives none: 2^(avg_bits - 2) and 2^(avg_bits + 2), held to what the entry points accept (32 at least,
    2^31 at most, min_len <= max_len)"""
    lo = max(32, 1 << max(0, avg_bits - 2))
    return lo, max(lo, min(1 << 31, 1 << (avg_bits + 2)))


def _bytes(data) -> np.ndarray:
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.astype(np.uint8, copy=False).ravel()


def hashes(data) -> np.ndarray:
    """h(p) for every p (uint32); the entries below 31 mean nothing"""
    x = _bytes(data)
    g = GEAR[x]
    h = np.zeros(x.size, dtype=np.uint32)
    for j in range(min(32, x.size)):
        h[j:] += g[: x.size - j] << np.uint32(j)        # (uint32 arithmetic wraps: modulo 2^32)
    return h


def candidates(data, avg_bits: int) -> np.ndarray:
    """the candidate positions, ascending"""
    h = hashes(data)
    c = np.flatnonzero((h >> np.uint32(32 - avg_bits)) == 0)
    return c[c >= 31]


def cut_points(data, avg_bits: int, min_len=None, max_len=None) -> list:
    x = _bytes(data)
    n = int(x.size)
    d = defaults(avg_bits)
    min_len, max_len = d[0] if min_len is None else min_len, d[1] if max_len is None else max_len
    assert 1 <= avg_bits <= 30 and 32 <= min_len <= max_len <= 1 << 31
    bounds = candidates(x, avg_bits) + 1
    cuts, s = [], 0
    while n - s > min_len:
        hi = min(s + max_len, n)
        i = int(np.searchsorted(bounds, s + min_len))
        e = int(bounds[i]) if i < bounds.size and bounds[i] <= hi else hi
        if e >= n:
            break
        cuts.append(e)
        s = e
    return cuts


def blocks(n: int, cuts) -> list:
    """[(offset, length)] of the pieces between the cuts"""
    edges = [0] + list(cuts) + [n]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]
