"""CPU suite: the numpy model of the byte-plane rule (tests/planes_model.py) against a byte-at-a-time restatement of the rule's text, inverse(forward)
the identity, and what the filter is there for, by the CPU oracle at window 22: an int32 index array compresses to at most half of what it does raw."""
import numpy as np
import pytest

from nlzm_amd import corpus
from tests import oracle_py, planes_model


def slow_forward(x: bytes, e: int) -> bytes:
    """the rule as its text reads, one byte at a time"""
    n = len(x)
    m = n // e
    y = bytearray(n)
    for j in range(e):
        for i in range(m):
            y[j * m + i] = x[i * e + j]
    for t in range(n - e * m):
        y[e * m + t] = x[e * m + t]
    return bytes(y)


def slow_inverse(y: bytes, e: int) -> bytes:
    n = len(y)
    m = n // e
    x = bytearray(n)
    for j in range(e):
        for i in range(m):
            x[i * e + j] = y[j * m + i]
    for t in range(n - e * m):
        x[e * m + t] = y[e * m + t]
    return bytes(x)


@pytest.mark.parametrize("e", planes_model.ELEMS)
def test_model_against_the_byte_at_a_time_rule(e):
    rng = np.random.default_rng(corpus.SEED + 140 + e)
    for n in list(range(0, 70)) + [127, 128, 129, 1000, 1001, 1003, 1007]:
        x = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        y = planes_model.forward(x, e)
        assert y == slow_forward(x, e) and len(y) == n
        assert planes_model.inverse(y, e) == x == slow_inverse(y, e)
        assert planes_model.inverse(x, e) == slow_inverse(x, e)
        assert planes_model.apply(x, e) == y and planes_model.apply(y, e, True) == x
        if e == 1:
            assert y == x


def test_known_answers():
    x = bytes(range(11))
    assert planes_model.forward(x, 2) == bytes([0, 2, 4, 6, 8, 1, 3, 5, 7, 9, 10])
    assert planes_model.forward(x, 4) == bytes([0, 4, 1, 5, 2, 6, 3, 7, 8, 9, 10])
    assert planes_model.forward(x, 8) == bytes([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
    assert planes_model.forward(np.arange(3, dtype="<u4"), 4) == bytes([0, 1, 2] + [0] * 9)
    for bad in (0, 3, 16):
        with pytest.raises(ValueError):
            planes_model.forward(x, bad)
        with pytest.raises(ValueError):
            planes_model.inverse(x, bad)


def test_index_arrays_compress_to_half_at_most():
    """(np.arange(4096) * 3 + 1000).astype(np.int32) at window 22: measured 526 bytes through planes_4 against 6,442 raw"""
    x = (np.arange(4096) * 3 + 1000).astype("<i4").tobytes()
    raw, typed = oracle_py.compress(x, 22), oracle_py.compress(planes_model.forward(x, 4), 22)
    print(f"int32 arange * 3 + 1000: raw {len(raw)}, planes {len(typed)}")
    assert 2 * len(typed) <= len(raw)
    assert planes_model.inverse(oracle_py.decompress(typed), 4) == x


def test_bf16_weights_are_recorded():
    """bf16 N(0, 0.02^2): recorded, not gated (measured at 2^20 elements: planes / raw = 0.858; here 2^16 elements, for the suite's time)"""
    rng = np.random.default_rng(corpus.SEED + 145)
    w = (rng.standard_normal(1 << 16) * 0.02).astype("<f4")
    x = (w.view("<u4") >> 16).astype("<u2").tobytes()          # (truncated to bf16)
    raw, typed = oracle_py.compress(x, 22), oracle_py.compress(planes_model.forward(x, 2), 22)
    print(f"bf16 weights, {len(x)} bytes: raw {len(raw)}, planes {len(typed)}, planes / raw {len(typed) / len(raw):.3f}")
    assert planes_model.inverse(oracle_py.decompress(typed), 2) == x
