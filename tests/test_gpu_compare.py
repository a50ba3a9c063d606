"""GPU suite (-m gpu): compare_kernel (nlzm_amd/csrc/nlzm_decode.hip), which is verify's whole verdict, through nlzm_hip_verify_dev against
numpy.  The reference for every call is np.flatnonzero(a[:m] != b[:m]) -- its first element, or m when there is none -- with m =
min(decoded, n).  Only well-formed streams go to the device (tests/test_gpu_decode.py's policy); what differs is the ORIGINAL.

The small stream holds 3 * 4096 + 7 bytes: 4096 bytes are one workgroup's share (256 threads of 16 bytes), so the launch has four
workgroups, a last full 16-byte load and a 7-byte tail.  The original lies on the device behind 16 bytes of slack and is handed over at
misalignments 0 (the 16-byte-load path), 1, 4, 8 and 15 (the byte loop).  One byte is flipped in place and flipped back after the call.
12 s on an MI355X: a call on the small stream takes 5 ms (the 675 single flips 3.4 s), the stride loop's nine decodes of 33.5 MB 6.4 s."""
import ctypes as C

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

from nlzm_amd import corpus, shard
from tests import oracle_py

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 7
MISALIGN = [0, 1, 4, 8, 15]
MASKS = [0x01, 0x80, 0xFF]          # (0x80: the one a ctz-to-byte slip gets wrong)


def reference(a, b, decoded):
    m = min(decoded, len(b))
    d = np.flatnonzero(a[:m] != b[:m])
    return int(d[0]) if d.size else m


class Pair:
    """a stream on the device and copies of the original at every misalignment; call(): one nlzm_hip_verify_dev"""

    def __init__(self, gpu, data, stream, nblocks=1, blen=None, misalign=MISALIGN, extra=0):
        self.lib, self.data, self.n, self.k = gpu.load_library(), np.ascontiguousarray(data), int(data.size), nblocks
        self.blen = (C.c_uint64 * nblocks)(*blen) if blen is not None else None
        s = np.frombuffer(stream, dtype=np.uint8)
        self.d_src, self.slen = torch.from_numpy(s.copy()).to("cuda:0"), s.size
        self.host = np.concatenate([self.data, np.full(extra, 0x55, dtype=np.uint8)])      # (what lies behind the original: part of it when n says so)
        self.orig = {}
        for a in misalign:
            t = torch.zeros(16 + self.host.size + 16, dtype=torch.uint8, device="cuda:0")
            assert t.data_ptr() % 16 == 0
            t[a:a + self.host.size].copy_(torch.from_numpy(self.host))
            self.orig[a] = t
        torch.cuda.synchronize()

    def call(self, a, flips=(), n=None):
        """the original at misalignment a with the (position, mask) flips applied for the call; -> (first, decoded_len, numpy's answer)"""
        n = self.n if n is None else n
        t, b = self.orig[a], self.host.copy()
        for p, m in flips:
            t[a + p:a + p + 1] ^= m
            b[p] ^= m
        torch.cuda.synchronize()
        first, dlen = C.c_uint64(1 << 63), C.c_uint64(1 << 63)
        rc = self.lib.nlzm_hip_verify_dev(self.d_src.data_ptr(), self.slen, self.k, self.blen, t.data_ptr() + a, n, C.byref(first), C.byref(dlen))
        for p, m in flips:
            t[a + p:a + p + 1] ^= m
        assert rc == 0, self.lib.nlzm_hip_last_error()
        return int(first.value), int(dlen.value), reference(self.data, b[:n], self.n)

    def restored(self):
        return all(bool(torch.equal(t[a:a + self.host.size].cpu(), torch.from_numpy(self.host))) for a, t in self.orig.items())


@pytest.fixture(scope="module")
def small(gpu):
    data = corpus.syn_text(N, corpus.SEED + 71)
    return Pair(gpu, data, oracle_py.compress(data, 15))


def positions():
    return list(range(0, 48)) + list(range(4080, 4112)) + list(range(8176, 8208)) + list(range(N - 23, N))


def test_untouched_is_equal_at_every_misalignment(small):
    for a in MISALIGN:
        assert small.call(a) == (N, N, N), a


def test_single_flips(small):
    """every offset 0 .. 47 (each byte of three 16-byte loads), the workgroup boundaries at 4096 and 8192 with 16 bytes on either side, the last
    full load and the 7-byte tail up to the last byte; the three masks in turn, every misalignment"""
    bad = []
    calls = 0
    for ai, a in enumerate(MISALIGN):
        for pi, p in enumerate(positions()):
            mask = MASKS[(pi + ai) % 3]
            first, dlen, want = small.call(a, [(p, mask)])
            calls += 1
            assert want == p
            if (first, dlen) != (want, N):
                bad.append((a, p, hex(mask), first, dlen))
    assert not bad, bad[:20]
    assert calls == 5 * 135
    # the aligned path has seen every mask at every byte of a dword, and 0x80 at every byte of a 16-byte load
    seen = {(p % 4, MASKS[pi % 3]) for pi, p in enumerate(positions())}
    assert len(seen) == 12 and {p % 16 for pi, p in enumerate(positions()) if MASKS[pi % 3] == 0x80} == set(range(16))
    assert small.restored()


PAIRS = [("one dword, bytes 1 and 3", 4096 + 80 + 1, 4096 + 80 + 3),
         ("one 16-byte load, word 1 and word 3", 2 * 4096 + 160 + 5, 2 * 4096 + 160 + 13),
         ("one 16-byte load, word 0 and word 3", 160 + 3, 160 + 12),
         ("neighbouring lanes", 16 * 20 + 9, 16 * 21 + 2),
         ("different waves", 16 * 10 + 3, 16 * 70 + 1),
         ("different workgroups", 100, 2 * 4096 + 50),
         ("the last workgroup and the first", 3 * 4096 + 2, 7),
         ("the tail's neighbour and the tail", N - 10, N - 3),
         ("both in the tail", N - 6, N - 1)]


@pytest.mark.parametrize("a", [0, 1])
def test_two_differences_the_earlier_wins(small, a):
    bad = []
    for name, p, q in PAIRS:
        for flips in ([(p, 0x80), (q, 0x01)], [(q, 0xFF), (p, 0x80)], [(p, 0x01), (q, 0x80)]):
            first, dlen, want = small.call(a, flips)
            assert want == min(p, q)
            if (first, dlen) != (want, N):
                bad.append((name, flips, first, dlen))
    assert not bad, bad
    assert small.restored()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17])
def test_short_lengths(gpu, n):
    """streams of 0, 1, 15, 16 and 17 bytes (empty, one_byte and three made the same way): equal; the last byte flipped; an original that is
    longer than the decode, with a flipped byte behind the decoded length: first == decoded, and the decoded length says which it was"""
    data = corpus.make("random", 0, corpus.SEED) if n == 0 else corpus.syn_text(n, corpus.SEED)
    pair = Pair(gpu, data, oracle_py.compress(data, 22 if n == 0 else 15), misalign=[0, 1], extra=9)
    for a in (0, 1):
        assert pair.call(a) == (n, n, n)
        if n:
            for mask in MASKS:
                assert pair.call(a, [(n - 1, mask)]) == (n - 1, n, n - 1)
            assert pair.call(a, [(0, 0x80)]) == (0, n, 0)
        # the original longer than the stream's bytes
        assert pair.call(a, [(n + 4, 0xFF)], n=n + 9) == (n, n, n)
        assert pair.call(a, n=n + 9) == (n, n, n)
        if n:
            assert pair.call(a, [(n - 1, 0x01), (n + 1, 0x01)], n=n + 9) == (n - 1, n, n - 1)
    assert pair.restored()


def test_the_stride_loop(gpu):
    """2 * 2^24 + 53 bytes: the launch is 4096 workgroups of 256 threads of 16 bytes, so the first threads make three iterations.  Sixteen blocks
    at window 20, their lengths given (one decode pass); flips on both sides of every stride boundary, in the third iteration's first load and
    in the last byte of its tail, and a pair that one thread meets in its first and in its second iteration."""
    S = 1 << 24
    n, k = 2 * S + 16 * 3 + 5, 16
    data = corpus.syn_text(n, corpus.SEED + 72)
    blocks = gpu.compress_blocks(data, k, 20)
    assert [hi - lo for lo, hi in (shard.block_range(n, k, i) for i in range(k))][0] == (n + k - 1) // k
    pair = Pair(gpu, data, b"".join(blocks), nblocks=k, blen=[len(b) for b in blocks], misalign=[0])
    assert pair.call(0) == (n, n, n)
    assert gpu.counter("decode_passes") == 1
    for i, p in enumerate((5, S - 1, S, S + 16, 2 * S - 1, 2 * S, n - 1)):          # (a call decodes 2 MB per wave: some 0.3 s)
        assert pair.call(0, [(p, MASKS[i % 2])]) == (p, n, p), p
    assert pair.call(0, [(S + 5, 0x80), (7, 0x80)]) == (7, n, 7)
    assert pair.restored()
