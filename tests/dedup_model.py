"""The equal-range finder restated in numpy, independently of the C++ (nlzm_amd/csrc/nlzm_dedup.h, nlzm_dedup_plan.h): what
tests/test_dedup_model.py holds to a byte-at-a-time restatement, and what the simulator harness (tests/test_dedup_sim.py) and the device
(tests/test_gpu_dedup.py) are held to.

  segments     a range of n bytes is cut into segments of SEGMENT bytes from its own first byte; segment g holds m = min(SEGMENT, n - g SEGMENT) bytes
  words        a segment's bytes, zeros behind them up to a multiple of 16, as little-endian 32-bit words w[0 .. 4U), U = ceil(m / 16)
  keys         K(j) = mix32(j + 1); mix32: x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16 (modulo 2^32)
  segment      h = sum over u < U of ((w[4u] + K(4u)) mod 2^32) * ((w[4u+1] + K(4u+1)) mod 2^32)
                                   + ((w[4u+2] + K(4u+2)) mod 2^32) * ((w[4u+3] + K(4u+3)) mod 2^32), modulo 2^64
  fingerprint  F = splitmix64((sum over g of splitmix64(h(g) + (g + 1) * 0x9E3779B97F4A7C15) mod 2^64) XOR splitmix64(n))
  first_of     first_of[i] = the smallest j <= i whose range holds the same bytes as range i
"""
import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
SEGMENT = 32768
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(x: int) -> int:
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mix32(x):
    """on a uint32 array (arithmetic wraps: modulo 2^32)"""
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


KEYS = mix32(np.arange(1, SEGMENT // 4 + 1, dtype=np.uint32))       # K(j), j = 0 .. SEGMENT / 4 - 1


def _bytes(data) -> np.ndarray:
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.astype(np.uint8, copy=False).ravel()


def segment_h(seg) -> int:
    x = _bytes(seg)
    assert 1 <= x.size <= SEGMENT
    pad = np.zeros((x.size + 15) // 16 * 16, dtype=np.uint8)
    pad[: x.size] = x
    a = (pad.view("<u4") + KEYS[: pad.size // 4]).astype(np.uint64)      # (the uint32 sum has wrapped)
    return int(np.sum(a[0::2] * a[1::2], dtype=np.uint64))                 # (uint64 arithmetic wraps: modulo 2^64)


def fingerprint(data) -> int:
    x = _bytes(data)
    acc = 0
    for g in range((x.size + SEGMENT - 1) // SEGMENT):
        acc = (acc + splitmix64((segment_h(x[g * SEGMENT: (g + 1) * SEGMENT]) + (g + 1) * GOLDEN) & M64)) & M64
    return splitmix64(acc ^ splitmix64(int(x.size)))


def fingerprints(data, ranges) -> list:
    x = _bytes(data)
    return [fingerprint(x[o: o + l]) for o, l in ranges]


def first_of(data, ranges) -> list:
    x = _bytes(data)
    seen, out = {}, []
    for i, (o, l) in enumerate(ranges):
        out.append(seen.setdefault(x[o: o + l].tobytes(), i))
    return out


def distinct(first) -> int:
    return sum(1 for i, f in enumerate(first) if f == i)


def dup_bytes(first, ranges) -> int:
    return sum(l for i, ((_, l), f) in enumerate(zip(ranges, first)) if f != i)
