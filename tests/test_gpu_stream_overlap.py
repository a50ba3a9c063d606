"""GPU suite (-m gpu): a single stream's launches run one ahead of the host (nlzm_hip.cpp, stream_step).  The pre-pass and the
launch of k + 1 are queued before launch k is collected, on two launch sets used alternately; the frames of launch k are coded and gathered beside
launch k + 1; round_open_kernel / round_close_kernel set the progress words and copy aside what the host checks.  The stream must not change.

Input: corpus.syn_text at window 18 (chunks of 60,928 bytes: 300,000 bytes are 5 chunks, 620,000 are 11).  Every stream: SHA-256, length and the
operation counters against tests/oracle_py.compress(..., want_stats=True).
  300,000 bytes at batch_chunks 1 and 2   both sets in use; at 2 the last launch is short (one chunk)
  620,000 bytes at batch_chunks 1         eleven launches: each set used again and again while the other's coder and gather may be in flight
  stepping through the C ABI              max_chunks 1, and max_chunks 3 at batch_chunks 2 (a call = a full launch and a short one): every call drains
  test_fail_launch                        launch 1 and the last launch fail: reported with their own chunk range, at once; the library works afterwards"""
import ctypes as C
import functools
import hashlib
import time

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import oracle_py

pytestmark = pytest.mark.gpu

OPS = ("bt_calls", "bt_tests", "cmp_bytes", "ht_rows", "rk_probes", "rk_inserts", "positions", "nice_positions", "segments")
HIST_BITS = 18
SIZES = (300_000, 620_000)


def digest(stream: bytes):
    return hashlib.sha256(stream).hexdigest(), len(stream)


@functools.lru_cache(maxsize=None)
def text(n):
    return corpus.syn_text(n)


@functools.lru_cache(maxsize=None)
def want(n):
    """-> the oracle's stream, its (sha, length), its operation counters: computed once per size"""
    stream, ost = oracle_py.compress(text(n), HIST_BITS, want_stats=True)
    return stream, digest(stream), {k: ost["cmp_bytes_needed" if k == "cmp_bytes" else k] for k in OPS}


def check(gpu, got: bytes, n):
    _, dg, ops = want(n)
    assert digest(got) == dg
    st = gpu.stats()
    assert {k: st[k] for k in OPS} == ops


def nchunks(gpu, n):
    return -(-n // gpu.geometry(n, HIST_BITS)["chunk_size"])


@pytest.mark.parametrize("n,batch", [(300_000, 1), (300_000, 2), (620_000, 1)])
def test_one_call(gpu, n, batch):
    assert (nchunks(gpu, 300_000), nchunks(gpu, 620_000)) == (5, 11)      # (an odd number of chunks: batch 2 ends in a short launch)
    gpu.set_option("batch_chunks", batch)
    try:
        got = gpu.compress(text(n), HIST_BITS)
        launches = gpu.timing()["match_parse_launches"]
    finally:
        gpu.set_option("batch_chunks", 32)
    check(gpu, got, n)
    assert launches == -(-nchunks(gpu, n) // batch)


@pytest.mark.parametrize("max_chunks,batch", [(1, 1), (3, 2)])
def test_stepping_through_the_c_abi(gpu, max_chunks, batch):
    """after every call in_done and out_done are monotonic and dst[:out_done] is the final stream's prefix; the finished stream is the one-call stream"""
    n = 620_000
    data, final = text(n), want(n)[0]
    lib = gpu.load_library()
    hip = C.CDLL("libamdhip64.so")                              # (the runtime the library is linked against: device buffers for the test)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    cap = int(lib.nlzm_hip_compress_bound(n))
    d_in, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_in), n + 512) == 0 and hip.hipMalloc(C.byref(d_out), cap) == 0
    gpu.set_option("batch_chunks", batch)
    try:
        assert hip.hipMemset(d_in, 0, n + 512) == 0 and hip.hipMemcpy(d_in, data.ctypes.data, n, 1) == 0
        assert lib.nlzm_hip_stream_begin(d_in, n, HIST_BITS, d_out, cap) == 0, lib.nlzm_hip_last_error().decode()
        done, out, fin = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        last_in, last_out, calls = 0, 4, 0
        host = np.empty(cap, dtype=np.uint8)
        while not fin.value:
            assert lib.nlzm_hip_stream_step(max_chunks, C.byref(done), C.byref(out), C.byref(fin)) == 0, lib.nlzm_hip_last_error().decode()
            assert done.value > last_in and out.value > last_out
            last_in, last_out = done.value, out.value
            assert hip.hipMemcpy(host.ctypes.data, d_out, out.value, 2) == 0
            assert host[: out.value].tobytes() == final[: out.value], f"after call {calls}"
            calls += 1
            assert calls <= 11
        assert done.value == n and calls == -(-nchunks(gpu, n) // max_chunks)
        total = C.c_uint64(0)
        assert lib.nlzm_hip_stream_finish(C.byref(total)) == 0, lib.nlzm_hip_last_error().decode()
        assert hip.hipMemcpy(host.ctypes.data, d_out, total.value, 2) == 0
        check(gpu, host[: total.value].tobytes(), n)
    finally:
        gpu.set_option("batch_chunks", 32)
        hip.hipFree(d_in); hip.hipFree(d_out)


@pytest.mark.parametrize("which", ["second", "last"])
def test_failing_launch_is_reported_with_its_chunks(gpu, which):
    """test_fail_launch at batch_chunks 1: launch k is chunks [k, k + 1).  Launch 1 fails with its successor queued behind it (which must leave at
    once: round_open_kernel hands the sticky error on); the last launch fails with nothing behind it.  The bound is the block-set test's (8 s)."""
    n = 620_000
    k = 1 if which == "second" else nchunks(gpu, n) - 1
    gpu.set_option("batch_chunks", 1)
    gpu.set_option("test_fail_launch", k)
    try:
        t0 = time.perf_counter()
        with pytest.raises(gpu.NlzmError, match=rf"device error \d+ in chunks \[{k},{k + 1}\)"):
            gpu.compress(text(n), HIST_BITS)
        dt = time.perf_counter() - t0
        assert dt < 8.0, f"the failing stream took {dt:.1f} s to come back"
    finally:
        gpu.set_option("test_fail_launch", -1)
    try:
        got = gpu.compress(text(n), HIST_BITS)
    finally:
        gpu.set_option("batch_chunks", 32)
    check(gpu, got, n)
