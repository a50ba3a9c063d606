"""Measurements of the byte-plane filter and of the typed compress call (not a test; DESIGN.md section 27 holds the results,
profiles/planes_measure.txt the log).

    python tests/gpu_planes.py [--out DIR] PART ...

Buffers resident, profiler off, one warm-up dropped, three timed runs; device times are the library's events round the one launch.

  rate        nlzm_hip_planes_dev, ONE range, forward and inverse, e = 1, 2, 4, 8, on the first 100 MB of bench.py's 1e9-byte stand-in and on the stand-in
              whole: "planes_us", bytes per second (e = 1 is the same launch copying)
  gather      the range reader's gather launch moving 100 MB in the same process: a container of 50 MB of the stand-in, cut by content at avg_bits 20,
              read twice in one nlzm_hip_read_ranges_dev call, so that no block is decoded in place: "range_gather_us"
  share       THE GATE: nlzm_hip_compress_ranges_typed_dev on 100 MB of the stand-in cut at avg_bits 20, -window:28, e = 2: the filter's device time
              ("planes_us") is at most 1 % of the call's wall time
  sizes       container sizes of the typed against the untyped call, 100 MB each of seeded bf16 N(0, 0.02^2) weights (e = 2) and int32 Zipf ids (e = 4),
              cut into 32 equal ranges of whole elements, -window:22"""
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
parts = args
os.makedirs(out_dir, exist_ok=True)
log = open(os.path.join(out_dir, "planes_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def spread(v):
    return {"runs": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "max_minus_min": round(max(v) - min(v), 2)}


N1G, W, AVG = bench.STREAM_BYTES, bench.WINDOW, 20
MIN_LEN, MAX_LEN = 1 << (AVG - 2), 1 << (AVG + 2)
TEXT = 100_000_000
t0 = time.time()
host_1g = bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0))))       # (forks: before the GPU is touched)
say(f"# stand-in made in {time.time() - t0:.1f} s; parts: {parts}")

import torch

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


def u64(*v):
    return (C.c_uint64 * len(v))(*v)


d_in = torch.zeros(N1G + 4096, dtype=torch.uint8, device=dev)
d_in[:N1G].copy_(torch.from_numpy(host_1g))
torch.cuda.synchronize()


def blocks_of(d_buf, n):
    """the content-cut blocks of the n bytes at d_buf as ctypes arrays"""
    cap = n // MIN_LEN
    cuts, got = (C.c_uint64 * cap)(), C.c_uint32(0)
    chk(lib.nlzm_hip_cut_points_dev(d_buf.data_ptr(), n, AVG, MIN_LEN, MAX_LEN, cuts, cap, C.byref(got)))
    edges = [0] + [int(cuts[i]) for i in range(got.value)] + [n]
    k = len(edges) - 1
    return k, (C.c_uint64 * k)(*edges[:-1]), (C.c_uint64 * k)(*[b - a for a, b in zip(edges, edges[1:])])


def typed_sizes(name, host, e, k=32):
    """the container of k equal ranges of whole elements of `host`, typed and untyped, -window:22"""
    n = int(host.size)
    per = -(-n // k) // e * e + e
    offs = [min(i * per, n) for i in range(k)]
    lens = [min(per, n - o) for o in offs]
    d = torch.zeros(n + 4096, dtype=torch.uint8, device=dev)
    d[:n].copy_(torch.from_numpy(host))
    off, ln = u64(*offs), u64(*lens)
    need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
    d_out = torch.empty(need, dtype=torch.uint8, device=dev)
    blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
    torch.cuda.synchronize()
    got = {}
    for label, el in (("untyped", None), ("typed", (C.c_uint8 * k)(*[e] * k))):
        t = time.perf_counter()
        chk(lib.nlzm_hip_compress_ranges_typed_dev(d.data_ptr(), n, k, off, ln, el, 22, d_out.data_ptr(), need, blen, C.byref(total)))
        torch.cuda.synchronize()
        got[label] = {"bytes": int(total.value), "wall_ms": round(1000 * (time.perf_counter() - t), 1)}
    say(json.dumps({"what": "container sizes, -window:22", "input": name, "bytes": n, "ranges": k, "elem": e, **got, "typed_over_untyped": round(got["typed"]["bytes"] / got["untyped"]["bytes"], 4),
                    "planes_us": counter("planes_us")}))
    del d, d_out


for part in parts:
    if part == "rate":
        d_out = torch.empty(N1G + 4096, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for name, n in (("text 100 MB", TEXT), ("stand-in 1e9", N1G)):
            for e in (1, 2, 4, 8):
                for inverse in (0, 1):
                    us = []
                    for i in range(4):
                        chk(lib.nlzm_hip_planes_dev(d_in.data_ptr(), n, d_out.data_ptr(), n, 1, u64(0), u64(0), u64(n), (C.c_uint8 * 1)(e), inverse))
                        if i:
                            us.append(counter("planes_us"))
                    say(json.dumps({"what": "planes", "input": name, "elem": e, "direction": "inverse" if inverse else "forward", "planes_us": spread(us),
                                    "GB_per_s": round(n / statistics.median(us) / 1000, 1), "planes_bytes": counter("planes_bytes")}))
        del d_out
    elif part == "gather":
        n = TEXT // 2
        k, off, ln = blocks_of(d_in, n)
        need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
        d_c = torch.empty(need, dtype=torch.uint8, device=dev)
        blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
        chk(lib.nlzm_hip_compress_ranges_dev(d_in.data_ptr(), n, k, off, ln, W, d_c.data_ptr(), need, blen, C.byref(total)))
        d_back = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        got, bad = C.c_uint64(0), C.c_uint32(0)
        torch.cuda.synchronize()
        us = []
        for i in range(4):
            chk(lib.nlzm_hip_read_ranges_dev(d_c.data_ptr(), int(total.value), k, blen, ln, None, 2, u64(0, 0), u64(n, n), d_back.data_ptr(), 2 * n, C.byref(got), C.byref(bad)))
            if i:
                us.append(counter("range_gather_us"))
        same = bool(torch.equal(d_back[:n], d_in[:n]) and torch.equal(d_back[n:], d_in[:n]))
        say(json.dumps({"what": "gather launch", "moved_bytes": 2 * n, "pieces": counter("range_pieces"), "range_gather_us": spread(us),
                        "GB_per_s": round(2 * n / statistics.median(us) / 1000, 1), "bytes_are_the_input_twice": same}))
        del d_c, d_back
    elif part == "share":
        k, off, ln = blocks_of(d_in, TEXT)
        el = (C.c_uint8 * k)(*[2] * k)
        need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
        d_out = torch.empty(need, dtype=torch.uint8, device=dev)
        blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
        ms, us = [], []
        for i in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            chk(lib.nlzm_hip_compress_ranges_typed_dev(d_in.data_ptr(), TEXT, k, off, ln, el, W, d_out.data_ptr(), need, blen, C.byref(total)))
            torch.cuda.synchronize()
            if i:
                ms.append(1000 * (time.perf_counter() - t))
                us.append(counter("planes_us"))
        share = statistics.median(us) / 1000 / statistics.median(ms)
        say(json.dumps({"what": "compress_ranges_typed_dev, the filter's share", "input": "text 100 MB", "blocks": k, "elem": 2, "wall_ms": spread(ms), "planes_us": spread(us),
                        "MB_per_s_of_the_call": round(TEXT / statistics.median(ms) / 1000, 1), "filter_share_of_the_call": round(share, 6), "gate_at_most": 0.01,
                        "gate": "PASS" if share <= 0.01 else "FAIL"}))
        del d_out
        if share > 0.01:
            raise SystemExit("the filter's device time is more than 1 % of the typed call")
    elif part == "sizes":
        rng = np.random.default_rng(corpus.SEED + 180)
        w = (rng.standard_normal(TEXT // 2) * 0.02).astype("<f4")
        typed_sizes("bf16 N(0, 0.02^2), 5e7 elements", (w.view("<u4") >> 16).astype("<u2").view(np.uint8), 2)
        ids = np.minimum(rng.zipf(1.2, TEXT // 4), (1 << 31) - 1).astype("<i4")
        typed_sizes("int32 Zipf(1.2) ids, 2.5e7 elements", ids.view(np.uint8), 4)
    else:
        raise SystemExit(f"unknown part {part}")

say("# done")
