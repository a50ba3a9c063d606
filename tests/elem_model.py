"""The rule that chooses a typed range's element size from plane statistics (nlzm_amd/csrc/nlzm_elem.h, nlzm_elem_plan.h) restated in numpy and
Python integers.  TEST INFRASTRUCTURE ONLY.

For a range x of n bytes, M = n div 8: H[c][v] is the number of i < 8 M with i mod 8 = c and x[i] = v -- i counted from the range's own first byte; the
n mod 8 bytes behind are in no histogram.  The planes of element size e are P(e, j)[v] = the sum over c = j (mod e) of H[c][v], j < e.

L(n) is the binary logarithm in 2^-16 bits, fixed point: L(0) = L(1) = 0; for n >= 2, k = floor(log2 n), x = floor(n 2^31 / 2^k), r = k 2^16, and for
i = 15 .. 0: x = floor(x^2 / 2^31); if x >= 2^32: x = floor(x / 2), r += 2^i.  Every step fits unsigned 64 bits.

cost(h) = N L(N) - sum h[v] L(h[v]) + floor(K L(N) / 2) modulo 2^64, for a histogram of total N with K non-zero bins: its order-0 code length and
half a logarithm of N per used bin of model.  C_e = the sum over j < e of cost(P(e, j)).

choose(C, n) = 1 when n < MIN_LEN; otherwise b = the e of smallest C_e (ties to the smaller e), and the answer is b unless b != 1 and
C_b + floor(C_1 / SHARE) > C_1, in which case it is 1.  tests/test_elem_model.py holds all of this to a byte-at-a-time restatement."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

ELEMS = (1, 2, 4, 8)
MIN_LEN = 4096          # a shorter range is left at e = 1
SHARE = 32              # a plane split has to save more than C_1 / SHARE
MAX_LEN = 1 << 40       # N L(N) fits 64 bits below
MASK = (1 << 64) - 1


def _arr(x) -> np.ndarray:
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8) if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def hist(x) -> np.ndarray:
    """H, shape (8, 256), uint64"""
    x = _arr(x)
    m = x.size // 8
    a = x[: 8 * m].reshape(m, 8)
    return np.stack([np.bincount(a[:, c], minlength=256) for c in range(8)]).astype(np.uint64)


@lru_cache(maxsize=1 << 16)
def L(n: int) -> int:
    n = int(n)
    if n < 2:
        return 0
    k = n.bit_length() - 1
    x = (n << 31) >> k
    r = k << 16
    for i in range(15, -1, -1):
        x = (x * x) >> 31
        if x >> 32:
            x >>= 1
            r += 1 << i
    return r


def cost(h) -> int:
    h = [int(v) for v in h]
    n = sum(h)
    return (n * L(n) - sum(v * L(v) for v in h if v) + (sum(1 for v in h if v) * L(n)) // 2) & MASK


def costs_of_hist(H) -> tuple:
    H = np.asarray(H, dtype=np.uint64)
    return tuple(sum(cost(H[j::e].sum(axis=0)) for j in range(e)) & MASK for e in ELEMS)


def costs(x) -> tuple:
    """(C_1, C_2, C_4, C_8) of the bytes x"""
    return costs_of_hist(hist(x))


def choose(C, n: int) -> int:
    if n < MIN_LEN:
        return 1
    b = min(range(4), key=lambda i: (int(C[i]), i))
    if b and int(C[b]) + int(C[0]) // SHARE > int(C[0]):
        return 1
    return ELEMS[b]


def choose_for(x) -> int:
    x = _arr(x)
    return choose(costs(x), int(x.size))
