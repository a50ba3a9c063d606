"""Measurements of the content-defined cut pass and of containers cut by content (not a test; DESIGN.md section 25 holds the results,
profiles/cut_measure.txt the log).

    python tests/gpu_cut.py [--out DIR] [--cache DIR] PART ...

Inputs: the first 100 MB of bench.py's 1e9-byte stand-in ("text") and the stand-in whole, at avg_bits 20 with the default lengths and -window:28.
Buffers resident, profiler off, one warm-up dropped, three timed runs.

  cut         device time of the cut pass ("cut_us": both launches) on both inputs, bytes per second, cuts and candidates
  compress    both inputs through nlzm_hip_compress_ranges_dev with the content's cuts and through nlzm_hip_compress_blocks_dev with the same
              number of blocks: wall ms round the one call, MB/s, output bytes, sets
  cli         `nlzm -window:28 -cdc:20 c` on both inputs as files: wall seconds of the command, and the cut pass's share of it (the cut pass timed
              in this process on the same bytes)"""
import ctypes as C
import json
import os
import statistics
import subprocess
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
cache = opt("--cache", "/tmp/nlzm_cut_cache")
parts = args
os.makedirs(out_dir, exist_ok=True)
os.makedirs(cache, exist_ok=True)
log = open(os.path.join(out_dir, "cut_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def spread(v):
    return {"runs": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "max_minus_min": round(max(v) - min(v), 2)}


N1G, W, AVG = bench.STREAM_BYTES, bench.WINDOW, 20
MIN_LEN, MAX_LEN = 1 << (AVG - 2), 1 << (AVG + 2)
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
CAP = int(N1G * 0.6)
d_c = torch.empty(CAP, dtype=torch.uint8, device=dev)
INPUTS = [("text 100 MB", 100_000_000), ("stand-in 1e9", N1G)]
cut_us = {}


def cut(n, runs=4):
    cap = n // MIN_LEN
    cuts, got, us = (C.c_uint64 * cap)(), C.c_uint32(0), []
    for i in range(runs):
        chk(lib.nlzm_hip_cut_points_dev(d_in.data_ptr(), n, AVG, MIN_LEN, MAX_LEN, cuts, cap, C.byref(got)))
        if i:
            us.append(counter("cut_us"))
    return [int(cuts[i]) for i in range(got.value)], us


def timed(call, runs=4):
    ms = []
    for i in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        chk(call())
        torch.cuda.synchronize()
        if i:
            ms.append(1000 * (time.perf_counter() - t))
    return ms


for part in parts:
    if part == "cut":
        for name, n in INPUTS:
            cuts, us = cut(n)
            cut_us[n] = statistics.median(us)
            lens = np.diff(np.array([0] + cuts + [n]))
            say(json.dumps({"what": "cut", "input": name, "avg_bits": AVG, "cut_us": spread(us), "GB_per_s": round(n / statistics.median(us) / 1000, 1), "cuts": len(cuts),
                            "candidates": counter("cut_candidates"), "block_bytes_min_mean_max": [int(lens.min()), int(lens.mean()), int(lens.max())],
                            "blocks_forced_at_the_maximum": int((lens[:-1] == MAX_LEN).sum())}))
    elif part == "compress":
        for name, n in INPUTS:
            cuts, _ = cut(n, runs=1)
            k = len(cuts) + 1
            edges = [0] + cuts + [n]
            off, ln = (C.c_uint64 * k)(*edges[:-1]), (C.c_uint64 * k)(*[b - a for a, b in zip(edges, edges[1:])])
            blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
            need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
            d_out = d_c if need <= CAP else torch.empty(need, dtype=torch.uint8, device=dev)
            runs = 4 if n < N1G else 3
            ms = timed(lambda: lib.nlzm_hip_compress_ranges_dev(d_in.data_ptr(), n, k, off, ln, W, d_out.data_ptr(), d_out.numel(), blen, C.byref(total)), runs)
            say(json.dumps({"what": "compress by content", "input": name, "blocks": k, "wall_ms": spread(ms), "MB_per_s": round(n / statistics.median(ms) / 1000, 2),
                            "out_bytes": int(total.value), "sets": counter("container_sets"), "redo": counter("block_redo_streams")}))
            ms = timed(lambda: lib.nlzm_hip_compress_blocks_dev(d_in.data_ptr(), n, k, W, d_out.data_ptr(), d_out.numel(), blen, C.byref(total)), runs)
            say(json.dumps({"what": "compress -blocks:k", "input": name, "blocks": k, "wall_ms": spread(ms), "MB_per_s": round(n / statistics.median(ms) / 1000, 2),
                            "out_bytes": int(total.value), "sets": counter("container_sets"), "redo": counter("block_redo_streams")}))
            del d_out
    elif part == "cli":
        for name, n in INPUTS:
            if n not in cut_us:
                cut_us[n] = statistics.median(cut(n)[1])
            src, dst = os.path.join(cache, f"in_{n}.bin"), os.path.join(cache, f"out_{n}.nlzm")
            host_1g[:n].tofile(src)
            for p in (dst, dst + ".idx"):
                if os.path.exists(p):
                    os.remove(p)
            t = time.perf_counter()
            r = subprocess.run([nlzm_amd.CLI_PATH, f"-window:{W}", f"-cdc:{AVG}", "c", src, dst], capture_output=True, text=True)
            wall = time.perf_counter() - t
            tail = [l for l in r.stdout.replace("\r", "\n").splitlines() if l.startswith(("Blocks:", "Done", "Error"))]
            say(json.dumps({"what": "nlzm -cdc c", "input": name, "rc": r.returncode, "wall_s": round(wall, 2), "cut_ms": round(cut_us[n] / 1000, 2),
                            "cut_share_of_the_command": round(cut_us[n] / 1e6 / wall, 5), "says": tail}))
            for p in (src, dst, dst + ".idx"):
                if os.path.exists(p):
                    os.remove(p)
    else:
        raise SystemExit(f"unknown part {part}")

say("# done")
