"""Measurements of the range reader (not a test; DESIGN.md section 18 holds the results, profiles/range_measure.txt the log).

    python tests/gpu_range.py [--out DIR] [--label NAME] [--cache DIR] [full] [ranges]        (default: both parts)

  full     the single-stream text case of tests/gpu_decode.py (the first 100 MB of the 1e9-byte stand-in, -window:28) decoded whole: did the
           decoder role's prefix mode cost the common path anything?  Run once on this tree and once with --lib naming a build of the parent
           commit, in one session on one box (--label says which is which; --cache DIR keeps input and stream between the two, so that both
           decode the same bytes and only one compresses; --lib PATH opens that library here, with the few entry points this part calls, so
           that the binding need not know a library without the range reader); the comparison is made by hand from the two "full" lines: the margin is twice the
           parent's own (max - min) / median of that session.
  ranges   the 32-block container of the 1e9-byte stand-in: 4 KiB ranges that end at 1 %, 50 % and 99 % of a block beside that block decoded
           whole (GATE: the 50 % read takes less device time than the whole block), and 1,000 ranges of 4 KiB spread over all blocks in one call.

Buffers resident, one warm-up dropped, three timed runs, device time from the library's events (profiler off)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import bench
import nlzm_amd
from nlzm_amd import corpus

args = sys.argv[1:]


def opt(name, default):
    if name in args:
        v = args[args.index(name) + 1]
        del args[args.index(name): args.index(name) + 2]
        return v
    return default


out_dir = opt("--out", os.path.join(ROOT, "profiles"))
label = opt("--label", "this tree")
cache = opt("--cache", None)
other_lib = opt("--lib", None)
parts = args or ["full", "ranges"]
os.makedirs(out_dir, exist_ok=True)
log = open(os.path.join(out_dir, "range_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


N1G, K, W, N100 = bench.STREAM_BYTES, 32, bench.WINDOW, 100_000_000
cached = cache and os.path.exists(os.path.join(cache, "stream.bin")) and "ranges" not in parts
t0 = time.time()
host_1g = None if cached else bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0))))      # (forks: before the GPU is touched)
say(f"# [{label}] library {'given by --lib' if other_lib else 'nlzm_amd/libnlzm_hip.so'}; stand-in {'from the cache' if cached else f'made in {time.time() - t0:.1f} s'}; parts: {parts}")

import torch

if other_lib:
    if parts != ["full"]:
        raise SystemExit("--lib: only the part `full`")
    lib = nlzm_amd._abi.bind(C.CDLL(other_lib))
else:
    lib = nlzm_amd.load_library()
if lib.nlzm_hip_init(0):
    raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())
dev = torch.device("cuda:0")


def chk(rc):
    if rc:
        raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())


def counter(key):
    v = C.c_uint64(0)
    chk(lib.nlzm_hip_get_counter(key.encode(), C.byref(v)))
    return int(v.value)


def to_dev(a, pad=4096):
    t = torch.zeros(a.size + pad, dtype=torch.uint8, device=dev)
    t[:a.size].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


def spread(v):
    return {"runs": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "spread_over_median": round((max(v) - min(v)) / statistics.median(v), 5)}


if "full" in parts:
    if cached:
        data = np.fromfile(os.path.join(cache, "input.bin"), dtype=np.uint8)
        stream = np.fromfile(os.path.join(cache, "stream.bin"), dtype=np.uint8)
        d_in, d_s, s_len = to_dev(data), to_dev(stream), stream.size
    else:
        d_in = to_dev(host_1g[:N100])
        cap = int(lib.nlzm_hip_compress_bound(N100))
        d_s = torch.empty(cap, dtype=torch.uint8, device=dev)
        m = C.c_uint64(0)
        t = time.time()
        chk(lib.nlzm_hip_compress_dev(d_in.data_ptr(), N100, W, d_s.data_ptr(), cap, C.byref(m)))
        s_len = m.value
        say(f"# 100 MB of the stand-in: stream {s_len} bytes, compressed in {time.time() - t:.1f} s")
        if cache:
            os.makedirs(cache, exist_ok=True)
            host_1g[:N100].tofile(os.path.join(cache, "input.bin"))
            d_s[:s_len].cpu().numpy().tofile(os.path.join(cache, "stream.bin"))
    d_back = torch.empty(N100, dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    ms, cyc = [], []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_s.data_ptr(), s_len, d_back.data_ptr(), N100, C.byref(m)))
        assert m.value == N100
        if i:
            ms.append(counter("decode_us") / 1000)
            cyc.append(counter("decode_cycles"))
    assert bool(torch.equal(d_back, d_in[:N100]))
    say(json.dumps({"full": "stand_in_100m_w28", "label": label, "device_ms": spread(ms), "MB_per_s": round(N100 / statistics.median(ms) / 1000, 3),
                    "wave_cycles": cyc, "cycles_per_byte": round(statistics.median(cyc) / N100, 2)}))
    del d_in, d_s, d_back

if "ranges" in parts:
    d1g = to_dev(host_1g)
    cap = int(lib.nlzm_hip_compress_bound(N1G)) + K * (16 + 131072)
    d_c = torch.empty(cap, dtype=torch.uint8, device=dev)
    blen, total = (C.c_uint64 * K)(), C.c_uint64(0)
    t = time.time()
    chk(lib.nlzm_hip_compress_blocks_dev(d1g.data_ptr(), N1G, K, W, d_c.data_ptr(), cap, blen, C.byref(total)))
    say(f"# 32-block container of the stand-in: {total.value} bytes, compressed in {time.time() - t:.1f} s")
    per = (N1G + K - 1) // K
    raws = (C.c_uint64 * K)(*[min(N1G, (i + 1) * per) - min(N1G, i * per) for i in range(K)])
    B = 5
    b_off, b_start = sum(blen[i] for i in range(B)), B * per
    d_back = torch.empty(per, dtype=torch.uint8, device=dev)
    m, bad = C.c_uint64(0), C.c_uint32(0)
    whole = []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_c.data_ptr() + b_off, blen[B], d_back.data_ptr(), raws[B], C.byref(m)))
        if i:
            whole.append(counter("decode_us") / 1000)
    assert bool(torch.equal(d_back[:raws[B]], d1g[b_start:b_start + raws[B]]))
    say(json.dumps({"ranges": f"block {B} decoded whole (nlzm_hip_decompress_dev)", "bytes": raws[B], "device_ms": spread(whole)}))
    KEYS = ("range_us", "range_decode_us", "range_gather_us", "range_blocks_decoded", "range_blocks_direct", "range_decoded_bytes", "range_scratch_bytes", "range_pieces")

    def read(ranges, what):
        k = len(ranges)
        off, ln = (C.c_uint64 * k)(*[o for o, _ in ranges]), (C.c_uint64 * k)(*[l for _, l in ranges])
        want = sum(l for _, l in ranges)
        d_out = torch.empty(want, dtype=torch.uint8, device=dev)
        rows = []
        for i in range(4):
            torch.cuda.synchronize()
            chk(lib.nlzm_hip_read_ranges_dev(d_c.data_ptr(), total.value, K, blen, raws, None, k, off, ln, d_out.data_ptr(), want, C.byref(m), C.byref(bad)))
            if i:
                rows.append({key: counter(key) for key in KEYS})
        at = 0
        for o, l in ranges[:50]:
            assert bool(torch.equal(d_out[at:at + l], d1g[o:o + l])), (what, o, l)
            at += l
        med = statistics.median(r["range_us"] for r in rows) / 1000
        say(json.dumps({"ranges": what, "ranges_in_call": k, "returned_bytes": want, "device_ms": spread([r["range_us"] / 1000 for r in rows]),
                        "decode_ms": [round(r["range_decode_us"] / 1000, 2) for r in rows], "gather_ms": [round(r["range_gather_us"] / 1000, 3) for r in rows],
                        "counters": {key: rows[-1][key] for key in KEYS[3:]}}))
        return med

    med = {}
    for pct in (1, 50, 99):
        end = b_start + raws[B] * pct // 100
        med[pct] = read([(end - 4096, 4096)], f"4 KiB ending at {pct} % of block {B}")
    w = statistics.median(whole)
    say(json.dumps({"gate": "a 4 KiB read that ends at 50 % of a block takes less than the block decoded whole", "read_ms": round(med[50], 2), "whole_ms": round(w, 2),
                    "ratio": round(med[50] / w, 3), "pass": med[50] < w}))
    rng = np.random.default_rng(corpus.SEED + 18)
    read([(int(o), 4096) for o in rng.integers(0, N1G - 4096, 1000)], "1,000 ranges of 4 KiB spread over all blocks")

say("# done")
