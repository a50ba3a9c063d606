"""Measurements of the stepping decoder (not a test; DESIGN.md section 20 holds the results, profiles/decode_steps_measure.txt the log).

    python tests/gpu_decode_steps.py [--out DIR] [--label NAME] [--cache DIR] [full] [steps] [walk]        (default: all three parts)

  full     the single-stream text case of tests/gpu_decode.py (the first 100 MB of the 1e9-byte stand-in, -window:28) decoded whole by
           nlzm_hip_decompress_dev: did building the stepping form beside it cost the one-shot kernel anything?  Run on this tree and, with
           NLZM_LIB naming a build of the parent commit, on the parent, alternating, in one session on one box (--label says which is
           which; --cache DIR keeps input and stream between the runs, so that all decode the same bytes and only one compresses).  The
           comparison is made by hand from the "full" lines: the margin is twice the parent's own (max - min) / median of that session.
  steps    the same stream in steps of 1, 8 and 64 frames against the one-shot decode of `full` in the same process (so `steps` needs
           `full`).  GATE: the total device time in steps of 8 frames stays within 1 % plus twice the one-shot's spread of the one-shot's median.
  walk     block 5 of the 32-block container of the stand-in read front to back with nlzm_amd.Decoder.read in 32 reads, against that block
           decoded whole.  GATE: the same 1 % plus twice the whole decode's spread.

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
parts = args or ["full", "steps", "walk"]
if "steps" in parts and "full" not in parts:
    raise SystemExit("steps: needs full in the same process")
os.makedirs(out_dir, exist_ok=True)
log = open(os.path.join(out_dir, "decode_steps_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


N1G, K, W, N100 = bench.STREAM_BYTES, 32, bench.WINDOW, 100_000_000
cached = cache and os.path.exists(os.path.join(cache, "stream.bin")) and "walk" not in parts
t0 = time.time()
host_1g = None if cached else bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0))))      # (forks: before the GPU is touched)
say(f"# [{label}] library {'given by NLZM_LIB' if os.environ.get('NLZM_LIB') else 'nlzm_amd/libnlzm_hip.so'}; stand-in {'from the cache' if cached else f'made in {time.time() - t0:.1f} s'}; parts: {parts}")

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


def to_dev(a, pad=4096):
    t = torch.zeros(a.size + pad, dtype=torch.uint8, device=dev)
    t[:a.size].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


def spread(v):
    return {"runs": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "spread_over_median": round((max(v) - min(v)) / statistics.median(v), 5)}


def gate(what, got, ref):
    med, rel = statistics.median(ref), (max(ref) - min(ref)) / statistics.median(ref)
    bound = med * (1 + 0.01 + 2 * rel)
    say(json.dumps({"gate": what, "ms": round(statistics.median(got), 2), "reference_ms": round(med, 2), "bound_ms": round(bound, 2),
                    "ratio": round(statistics.median(got) / med, 5), "pass": statistics.median(got) <= bound}))


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
    one, cyc = [], []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_s.data_ptr(), s_len, d_back.data_ptr(), N100, C.byref(m)))
        assert m.value == N100
        if i:
            one.append(counter("decode_us") / 1000)
            cyc.append(counter("decode_cycles"))
    assert bool(torch.equal(d_back, d_in[:N100]))
    say(json.dumps({"full": "stand_in_100m_w28", "label": label, "device_ms": spread(one), "MB_per_s": round(N100 / statistics.median(one) / 1000, 3),
                    "wave_cycles": cyc, "cycles_per_byte": round(statistics.median(cyc) / N100, 2)}))

    if "steps" in parts:
        raw, done, fin, ms = (C.c_uint64 * 1)(N100), (C.c_uint64 * 1)(), C.c_int(0), C.c_double(0)
        totals = {}
        for per in (1, 8, 64):
            rows, launches = [], 0
            for i in range(4):
                d_back.zero_()
                torch.cuda.synchronize()
                chk(lib.nlzm_hip_decode_begin_dev(d_s.data_ptr(), s_len, 1, None, raw, d_back.data_ptr(), N100, 0))
                total, fin.value = 0.0, 0
                while not fin.value:
                    chk(lib.nlzm_hip_decode_step(per, None, done, C.byref(fin), C.byref(ms)))
                    total += ms.value
                launches = counter("decode_steps")
                chk(lib.nlzm_hip_decode_finish(None, None))
                if i:
                    rows.append(total)
            assert bool(torch.equal(d_back, d_in[:N100]))
            totals[per] = rows
            over = (statistics.median(rows) - statistics.median(one)) / launches
            say(json.dumps({"steps": f"{per} frames a step", "launches": launches, "device_ms": spread(rows), "ratio_to_one_shot": round(statistics.median(rows) / statistics.median(one), 5),
                            "overhead_us_per_step": round(1000 * over, 1), "state_bytes": counter("decode_state_bytes")}))
        gate("the decode in steps of 8 frames within 1 % + twice the one-shot's spread of the one-shot", totals[8], one)
    del d_in, d_s, d_back

if "walk" in parts:
    d1g = to_dev(host_1g)
    cap = int(lib.nlzm_hip_compress_bound(N1G)) + K * (16 + 131072)
    d_c = torch.empty(cap, dtype=torch.uint8, device=dev)
    blen, total = (C.c_uint64 * K)(), C.c_uint64(0)
    t = time.time()
    chk(lib.nlzm_hip_compress_blocks_dev(d1g.data_ptr(), N1G, K, W, d_c.data_ptr(), cap, blen, C.byref(total)))
    say(f"# 32-block container of the stand-in: {total.value} bytes, compressed in {time.time() - t:.1f} s")
    per = (N1G + K - 1) // K
    raws = [min(N1G, (i + 1) * per) - min(N1G, i * per) for i in range(K)]
    B = 5
    b_off, b_start = sum(blen[i] for i in range(B)), B * per
    d_back = torch.empty(per, dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    whole = []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_c.data_ptr() + b_off, blen[B], d_back.data_ptr(), raws[B], C.byref(m)))
        if i:
            whole.append(counter("decode_us") / 1000)
    say(json.dumps({"walk": f"block {B} decoded whole (nlzm_hip_decompress_dev)", "bytes": raws[B], "device_ms": spread(whole)}))
    blob = d_c[:total.value].cpu().numpy()
    want = host_1g[b_start:b_start + raws[B]]
    READS = 32
    piece = -(-raws[B] // READS)
    rows, launches = [], 0
    for i in range(4):
        with nlzm_amd.Decoder(blob, K, list(blen), raws) as d:
            for r in range(READS):
                lo = r * piece
                got = d.read(b_start + lo, min(piece, raws[B] - lo))
                assert got == want[lo:lo + len(got)].tobytes(), r
            launches = counter("decode_steps")
            assert d.done[B] == raws[B] and sum(d.done) == raws[B]
            if i:
                rows.append(d.device_ms)
    say(json.dumps({"walk": f"block {B} front to back in {READS} reads of nlzm_amd.Decoder.read", "launches": launches, "device_ms": spread(rows),
                    "ratio_to_whole": round(statistics.median(rows) / statistics.median(whole), 5)}))
    gate("a block walked in 32 reads within 1 % + twice the whole decode's spread of the block decoded whole", rows, whole)

say("# done")
