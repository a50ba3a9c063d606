"""Measurements of the equal-range finder and of the compress path with option "dedup_ranges" (not a test; DESIGN.md section 26 holds the
results, profiles/dedup_measure.txt the log).

    python tests/gpu_dedup.py [--out DIR] PART ...

Inputs: the first 100 MB of bench.py's 1e9-byte stand-in ("text") and the stand-in whole, cut by content at avg_bits 20 with the default lengths,
compressed at -window:28.  Buffers resident, profiler off, one warm-up dropped, three timed runs.

  finder      nlzm_hip_equal_ranges_dev over the content-cut blocks of both inputs: "dedup_us" (all its launches), bytes per second, pairs, rounds
  free        a duplicate-free input, the text's blocks: nlzm_hip_compress_ranges_dev wall ms with the option off and on, alternating; the finder's
              share of the call with the option on
  edited      the case the option is for: the text followed by the same text with 1,000 bytes inserted in its middle, cut by content as one buffer:
              wall ms with the option off and on, alternating; how many blocks were copies
  free1g      the stand-in whole with the option on, ONE run (27 s; after the parts before it, which have warmed the device): the finder's share of
              the same call's wall time"""
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
log = open(os.path.join(out_dir, "dedup_measure.txt"), "a")


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


def on_and_off(d_buf, n, k, off, ln, rounds):
    """compress_ranges_dev with the option off and on, alternating, after one warm-up of each; wall ms, and the on runs' counters"""
    need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
    d_out = torch.empty(need, dtype=torch.uint8, device=dev)
    blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
    ms = {0: [], 1: []}
    info = {}
    for i in range(rounds + 1):
        for on in (0, 1):
            chk(lib.nlzm_hip_set_option(b"dedup_ranges", on))
            torch.cuda.synchronize()
            t = time.perf_counter()
            chk(lib.nlzm_hip_compress_ranges_dev(d_buf.data_ptr(), n, k, off, ln, W, d_out.data_ptr(), need, blen, C.byref(total)))
            torch.cuda.synchronize()
            if i:
                ms[on].append(1000 * (time.perf_counter() - t))
            info[on] = {"out_bytes": int(total.value), "sets": counter("container_sets")}
            if on:
                info[on].update({"dedup_us": counter("dedup_us"), "dedup_gather_us": counter("dedup_gather_us"), "distinct": counter("dedup_distinct"),
                                 "dup_bytes": counter("dedup_dup_bytes"), "pairs": counter("dedup_pairs"), "rounds": counter("dedup_rounds")})
    chk(lib.nlzm_hip_set_option(b"dedup_ranges", 0))
    del d_out
    return ms, info


for part in parts:
    if part == "finder":
        for name, n in (("text 100 MB", TEXT), ("stand-in 1e9", N1G)):
            k, off, ln = blocks_of(d_in, n)
            first, us = (C.c_uint32 * k)(), []
            for i in range(4):
                chk(lib.nlzm_hip_equal_ranges_dev(d_in.data_ptr(), n, k, off, ln, first, None))
                if i:
                    us.append(counter("dedup_us"))
            say(json.dumps({"what": "equal_ranges", "input": name, "blocks": k, "dedup_us": spread(us), "GB_per_s": round(n / statistics.median(us) / 1000, 1),
                            "distinct": counter("dedup_distinct"), "pairs": counter("dedup_pairs"), "rounds": counter("dedup_rounds")}))
    elif part in ("free", "edited"):
        if part == "free":
            name, d_buf, n = "text 100 MB, no duplicates", d_in, TEXT
        else:
            ins = np.random.default_rng(corpus.SEED + 150).integers(0, 256, 1000, dtype=np.uint8)
            both = np.concatenate([host_1g[:TEXT], host_1g[:TEXT // 2], ins, host_1g[TEXT // 2: TEXT]])
            name, n = "text 100 MB + the same with 1,000 bytes inserted in its middle", int(both.size)
            d_buf = torch.zeros(n + 4096, dtype=torch.uint8, device=dev)
            d_buf[:n].copy_(torch.from_numpy(both))
            torch.cuda.synchronize()
        k, off, ln = blocks_of(d_buf, n)
        ms, info = on_and_off(d_buf, n, k, off, ln, 3)
        off_med, on_med = statistics.median(ms[0]), statistics.median(ms[1])
        say(json.dumps({"what": "compress_ranges, option off / on alternating", "input": name, "bytes": n, "blocks": k, "off_wall_ms": spread(ms[0]), "on_wall_ms": spread(ms[1]),
                        "on_over_off": round(on_med / off_med, 4), "on_minus_off_ms": round(on_med - off_med, 2), "off": info[0], "on": info[1],
                        "copies": k - info[1]["distinct"], "same_bytes_out": info[0]["out_bytes"] == info[1]["out_bytes"],
                        "finder_share_of_the_on_call": round(info[1]["dedup_us"] / 1000 / on_med, 6)}))
    elif part == "free1g":
        k, off, ln = blocks_of(d_in, N1G)
        need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
        d_out = torch.empty(need, dtype=torch.uint8, device=dev)
        blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
        chk(lib.nlzm_hip_set_option(b"dedup_ranges", 1))
        torch.cuda.synchronize()
        t = time.perf_counter()
        chk(lib.nlzm_hip_compress_ranges_dev(d_in.data_ptr(), N1G, k, off, ln, W, d_out.data_ptr(), need, blen, C.byref(total)))
        torch.cuda.synchronize()
        wall = 1000 * (time.perf_counter() - t)
        chk(lib.nlzm_hip_set_option(b"dedup_ranges", 0))
        say(json.dumps({"what": "compress_ranges, option on, once", "input": "stand-in 1e9, no duplicates", "blocks": k, "wall_ms": round(wall, 2), "dedup_us": counter("dedup_us"),
                        "distinct": counter("dedup_distinct"), "sets": counter("container_sets"), "finder_share_of_the_call": round(counter("dedup_us") / 1000 / wall, 6)}))
        del d_out
    else:
        raise SystemExit(f"unknown part {part}")

say("# done")
