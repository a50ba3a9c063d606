"""Measurements of the element-size statistic and of the auto compress call (not a test; DESIGN.md section 31 holds the results,
profiles/elem_measure.txt the log).

    python tests/gpu_elem.py [--out DIR] PART ...

Buffers resident, profiler off, one warm-up dropped, three timed runs; device times are the library's events round its launches.

  rate        nlzm_hip_plane_costs_dev: "elem_us" and bytes per second for ONE range of the first 100 MB of bench.py's 1e9-byte stand-in, of the stand-in
              whole, of 100 MB of zeros (every lane on one counter: the counters' worst input) and of 100 MB of random bytes; and for 65,536 ranges of
              1.5 KB each.  For orientation the byte planes' launch (nlzm_hip_planes_dev, e = 2, forward) on the 100 MB of text in the same process
  share       THE GATE: nlzm_hip_compress_ranges_auto_dev on 100 MB cut at avg_bits 20, -window:28, for the text and for the zeros: the statistic's
              device time ("elem_us") is at most 1 % of the call's wall time
  sizes       container sizes, 100 MB in 32 equal ranges, -window:22: auto against untyped against the known e for seeded bf16 N(0, 0.02^2) weights
              (e = 2) and int32 Zipf ids (e = 4) -- section 27's inputs --, and for a mixed buffer of both plus text auto against every fixed e"""
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
log = open(os.path.join(out_dir, "elem_measure.txt"), "a")


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


def resident(host):
    d = torch.zeros(int(host.size) + 4096, dtype=torch.uint8, device=dev)
    d[: host.size].copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    return d


def blocks_of(d_buf, n):
    """the content-cut blocks of the n bytes at d_buf as ctypes arrays"""
    cap = n // MIN_LEN
    cuts, got = (C.c_uint64 * cap)(), C.c_uint32(0)
    chk(lib.nlzm_hip_cut_points_dev(d_buf.data_ptr(), n, AVG, MIN_LEN, MAX_LEN, cuts, cap, C.byref(got)))
    edges = [0] + [int(cuts[i]) for i in range(got.value)] + [n]
    k = len(edges) - 1
    return k, (C.c_uint64 * k)(*edges[:-1]), (C.c_uint64 * k)(*[b - a for a, b in zip(edges, edges[1:])])


def equal_ranges(n, k, e=8):
    per = -(-n // k) // e * e + e
    offs = [min(i * per, n) for i in range(k)]
    return offs, [min(per, n - o) for o in offs]


def container(d, n, offs, lens, mode, elems=None):
    """one container of the ranges: mode "auto", or "typed" with elems (None: untyped); (bytes, wall ms, the elems used)"""
    k = len(offs)
    off, ln = u64(*offs), u64(*lens)
    need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
    d_out = torch.empty(need, dtype=torch.uint8, device=dev)
    blen, total, el = (C.c_uint64 * k)(), C.c_uint64(0), (C.c_uint8 * k)(*(elems or [0] * k))
    torch.cuda.synchronize()
    t = time.perf_counter()
    if mode == "auto":
        chk(lib.nlzm_hip_compress_ranges_auto_dev(d.data_ptr(), n, k, off, ln, el, 22, d_out.data_ptr(), need, blen, C.byref(total)))
    else:
        chk(lib.nlzm_hip_compress_ranges_typed_dev(d.data_ptr(), n, k, off, ln, el if elems else None, 22, d_out.data_ptr(), need, blen, C.byref(total)))
    torch.cuda.synchronize()
    return {"bytes": int(total.value), "wall_ms": round(1000 * (time.perf_counter() - t), 1)}, [int(e) for e in el]


for part in parts:
    if part == "rate":
        rng = np.random.default_rng(corpus.SEED + 340)
        d_zero = torch.zeros(TEXT + 4096, dtype=torch.uint8, device=dev)
        d_rand = resident(rng.integers(0, 256, TEXT, dtype=np.uint8))
        cost = (C.c_uint64 * 4)()
        med = {}
        for name, d, n in (("text 100 MB", d_in, TEXT), ("stand-in 1e9", d_in, N1G), ("zeros 100 MB", d_zero, TEXT), ("random 100 MB", d_rand, TEXT)):
            us = []
            for i in range(4):
                chk(lib.nlzm_hip_plane_costs_dev(d.data_ptr(), n, 1, u64(0), u64(n), cost, None))
                if i:
                    us.append(counter("elem_us"))
            med[name] = statistics.median(us)
            say(json.dumps({"what": "plane_costs, one range", "input": name, "elem_us": spread(us), "GB_per_s": round(n / med[name] / 1000, 1), "elem_bytes": counter("elem_bytes"),
                            "costs": [int(c) for c in cost], "choice": int(lib.nlzm_hip_choose_elem(cost, n))}))
        say(json.dumps({"what": "zeros against random", "zeros_over_random": round(med["zeros 100 MB"] / med["random 100 MB"], 2)}))
        k, piece = 65536, 1536
        offs = [(i * 1517) % (TEXT - piece) for i in range(k)]
        off, ln, costs = u64(*offs), u64(*[piece] * k), (C.c_uint64 * (4 * k))()
        us = []
        for i in range(4):
            chk(lib.nlzm_hip_plane_costs_dev(d_in.data_ptr(), TEXT, k, off, ln, costs, None))
            if i:
                us.append(counter("elem_us"))
        say(json.dumps({"what": "plane_costs, 65,536 ranges of 1,536 bytes", "input": "text 100 MB", "elem_us": spread(us), "GB_per_s": round(k * piece / statistics.median(us) / 1000, 1),
                        "elem_bytes": counter("elem_bytes")}))
        d_out = torch.empty(TEXT + 4096, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        us = []
        for i in range(4):
            chk(lib.nlzm_hip_planes_dev(d_in.data_ptr(), TEXT, d_out.data_ptr(), TEXT, 1, u64(0), u64(0), u64(TEXT), (C.c_uint8 * 1)(2), 0))
            if i:
                us.append(counter("planes_us"))
        say(json.dumps({"what": "for orientation: the planes launch, e = 2, forward", "input": "text 100 MB", "planes_us": spread(us), "GB_per_s": round(TEXT / statistics.median(us) / 1000, 1)}))
        del d_zero, d_rand, d_out
    elif part == "share":
        d_zero = torch.zeros(TEXT + 4096, dtype=torch.uint8, device=dev)
        worst = 0.0
        for name, d in (("text 100 MB", d_in), ("zeros 100 MB", d_zero)):
            k, off, ln = blocks_of(d, TEXT)
            el = (C.c_uint8 * k)()
            need = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
            d_out = torch.empty(need, dtype=torch.uint8, device=dev)
            blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
            ms, us = [], []
            for i in range(4):
                torch.cuda.synchronize()
                t = time.perf_counter()
                chk(lib.nlzm_hip_compress_ranges_auto_dev(d.data_ptr(), TEXT, k, off, ln, el, W, d_out.data_ptr(), need, blen, C.byref(total)))
                torch.cuda.synchronize()
                if i:
                    ms.append(1000 * (time.perf_counter() - t))
                    us.append(counter("elem_us"))
            share = statistics.median(us) / 1000 / statistics.median(ms)
            worst = max(worst, share)
            say(json.dumps({"what": "compress_ranges_auto_dev, the statistic's share", "input": name, "blocks": k, "chosen": sorted(set(int(e) for e in el)), "wall_ms": spread(ms),
                            "elem_us": spread(us), "MB_per_s_of_the_call": round(TEXT / statistics.median(ms) / 1000, 1), "container_bytes": int(total.value),
                            "statistic_share_of_the_call": round(share, 6), "gate_at_most": 0.01, "gate": "PASS" if share <= 0.01 else "FAIL"}))
            del d_out
        del d_zero
        if worst > 0.01:
            raise SystemExit("the statistic's device time is more than 1 % of the auto call")
    elif part == "sizes":
        rng = np.random.default_rng(corpus.SEED + 180)           # (section 27's inputs, from its seed)
        w = (rng.standard_normal(TEXT // 2) * 0.02).astype("<f4")
        bf16 = (w.view("<u4") >> 16).astype("<u2").view(np.uint8)
        ids = np.minimum(rng.zipf(1.2, TEXT // 4), (1 << 31) - 1).astype("<i4").view(np.uint8)
        for name, host, e in (("bf16 N(0, 0.02^2), 5e7 elements", bf16, 2), ("int32 Zipf(1.2) ids, 2.5e7 elements", ids, 4)):
            n = int(host.size)
            d = resident(host)
            offs, lens = equal_ranges(n, 32)
            got = {"untyped": container(d, n, offs, lens, "typed")[0], "known": container(d, n, offs, lens, "typed", [e] * 32)[0]}
            got["auto"], chosen = container(d, n, offs, lens, "auto")
            say(json.dumps({"what": "container sizes, -window:22", "input": name, "bytes": n, "ranges": 32, "known_elem": e, "chosen": sorted(set(chosen)), **got,
                            "auto_over_untyped": round(got["auto"]["bytes"] / got["untyped"]["bytes"], 4), "auto_over_known": round(got["auto"]["bytes"] / got["known"]["bytes"], 4),
                            "elem_us": counter("elem_us")}))
            del d
        # a mixed buffer: eleven ranges of bf16, eleven of Zipf ids, ten of text, 3,125,000 bytes each
        per = TEXT // 32
        mixed = np.concatenate([bf16[: 11 * per], ids[: 11 * per], host_1g[: 10 * per]])
        n = int(mixed.size)
        d = resident(mixed)
        offs, lens = [i * per for i in range(32)], [per] * 32
        got = {"auto": None}
        got["auto"], chosen = container(d, n, offs, lens, "auto")
        for e in (1, 2, 4, 8):
            got[f"e{e}"] = container(d, n, offs, lens, "typed", [e] * 32 if e > 1 else None)[0]
        say(json.dumps({"what": "container sizes, -window:22", "input": "mixed: 11 ranges bf16, 11 ranges Zipf ids, 10 ranges text", "bytes": n, "ranges": 32, "chosen": chosen, **got,
                        "auto_over_best_fixed": round(got["auto"]["bytes"] / min(got[f"e{e}"]["bytes"] for e in (1, 2, 4, 8)), 4)}))
        del d
    else:
        raise SystemExit(f"unknown part {part}")

say("# done")
