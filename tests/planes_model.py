"""The byte-plane rule of typed ranges (nlzm_amd/csrc/nlzm_planes.h) restated in numpy.  TEST INFRASTRUCTURE ONLY.

For a range x of n bytes and an element size e in {1, 2, 4, 8}, m = n div e: planes_e(x) = y with y[j m + i] = x[i e + j] for 0 <= j < e,
0 <= i < m, and y[e m + t] = x[e m + t] for the n - e m tail bytes.  e = 1 is the identity; both directions keep the length; elements are
counted from the range's own first byte.  tests/test_planes_model.py holds this to a byte-at-a-time restatement."""
from __future__ import annotations

import numpy as np

ELEMS = (1, 2, 4, 8)


def _arr(x) -> np.ndarray:
    """the bytes of x: an array of any type is viewed, not converted"""
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8) if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def forward(x, e: int) -> bytes:
    if e not in ELEMS:
        raise ValueError("element size: 1, 2, 4 or 8")
    x = _arr(x)
    m = x.size // e
    return x[: e * m].reshape(m, e).T.tobytes() + x[e * m:].tobytes()


def inverse(y, e: int) -> bytes:
    if e not in ELEMS:
        raise ValueError("element size: 1, 2, 4 or 8")
    y = _arr(y)
    m = y.size // e
    return y[: e * m].reshape(e, m).T.tobytes() + y[e * m:].tobytes()


def apply(x, e: int, inv: bool = False) -> bytes:
    return inverse(x, e) if inv else forward(x, e)
