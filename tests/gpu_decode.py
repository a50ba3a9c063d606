"""Measurements of the device decoder (not a test; DESIGN.md section 16 holds the results, profiles/decode_*.txt the logs).

    python tests/gpu_decode.py [--out DIR] [chain] [blocks] [cli] [verify]        (default: all four parts)

  chain    wave cycles per rANS symbol and per output byte from the kernel's counters, on single streams made by the library's own compressor
           in this command: the first 100 MB of the 1e9-byte stand-in, 100 MB of wiki-shaped markup, 8 MB of random bytes; beside a floor from
           the machine constants of DESIGN.md section 9 (`achieved_over_bound`, as bench.py's latency bound for the parser)
  blocks   the 32-block container of the 1e9-byte stand-in: device time of the set, of its slowest stream alone, the ratio (GATE: <= 1.25)
  cli      `nlzm t` (host, one thread per block) against `nlzm -gpu t` and the bare device time, same files
  verify   `nlzm c -verify` against `nlzm c`: wall and device time, the 32-block container and one 100 MB stream

Input and output resident, one warm-up decode dropped, three timed runs, device time from the library's events (profiler off)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import bench
import nlzm_amd
from nlzm_amd import corpus

args = sys.argv[1:]
out_dir = os.path.join(ROOT, "profiles")
if "--out" in args:
    out_dir = args[args.index("--out") + 1]
    del args[args.index("--out"): args.index("--out") + 2]
parts = args or ["chain", "blocks", "cli", "verify"]
os.makedirs(out_dir, exist_ok=True)
log = open(os.path.join(out_dir, "decode_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


N1G, K, W = bench.STREAM_BYTES, 32, bench.WINDOW
need_1g = any(p in parts for p in ("chain", "blocks", "cli", "verify"))
t0 = time.time()
host_1g = bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0)))) if need_1g else None      # (forks: before the GPU is touched)
say(f"# stand-in made in {time.time() - t0:.1f} s; parts: {parts}")

import torch

nlzm_amd.init(0)
lib = nlzm_amd.load_library()
dev = torch.device("cuda:0")
COUNTERS = ("decode_syms", "decode_raw_ops", "decode_n_literal", "decode_n_dict", "decode_n_rep", "decode_out_bytes", "decode_ring_bytes", "decode_global_bytes",
            "decode_cycles", "decode_window_cycles", "decode_copy_cycles", "decode_max_stream_cycles", "decode_slowest_stream", "decode_us")


def chk(rc):
    if rc:
        raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())


def to_dev(a, pad=4096):
    t = torch.zeros(a.size + pad, dtype=torch.uint8, device=dev)
    t[:a.size].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


def compress_single(d_in, n, w):
    cap = int(lib.nlzm_hip_compress_bound(n))
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    torch.cuda.synchronize()
    t = time.time()
    chk(lib.nlzm_hip_compress_dev(d_in.data_ptr(), n, w, d_out.data_ptr(), cap, C.byref(m)))
    return d_out, m.value, time.time() - t


def counters():
    return {k: nlzm_amd.counter(k) for k in COUNTERS}


def decode_runs(d_stream_ptr, stream_len, n, runs=3):
    """one warm-up, `runs` timed decodes into a resident buffer; -> (list of counter dicts, output tensor)"""
    d_back = torch.empty(max(1, n), dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    res = []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_stream_ptr, stream_len, d_back.data_ptr(), n, C.byref(m)))
        assert m.value == n
        if i:
            res.append(counters())
    return res, d_back


# The floor of the symbol chain, from DESIGN.md section 9's constants, for the design built (model in registers, windows in registers): a wave alone
# on its SIMD issues one dependent instruction per LAT_ISSUE cycles, and a symbol cannot take fewer instructions than: the slot mask, the compare
# of all lanes, mask / count / index (4), two readlanes, freq, the multiply-add of the state (4), the test for renormalisation, the rotation of the
# four states (4), mix / shift / add / select of the adaptation (5), the choice of the register before and after (2 x 3 on average) = 27; a
# renormalisation (every second symbol on text: two bytes per 16 bits of state) two window reads of 7 instructions and the merge (4) = 18; a raw-bit
# op 12; a literal's store 4; a match's 64-byte step one LDS read and one LDS write that wait for each other (2 x LAT_LDS) and 10 instructions.
def chain_floor(c, stream_len):
    I = bench.LAT_ISSUE
    ops = c["decode_n_literal"] + c["decode_n_dict"] + c["decode_n_rep"]
    match_bytes = c["decode_ring_bytes"] + c["decode_global_bytes"]
    matches = c["decode_n_dict"] + c["decode_n_rep"]
    steps = matches + match_bytes / 64.0
    return (c["decode_syms"] * 27 * I + (stream_len / 2.0) * 18 * I + c["decode_raw_ops"] * 12 * I + c["decode_n_literal"] * 4 * I + ops * 6 * I
            + steps * (2 * bench.LAT_LDS + 10 * I))


def report_chain(name, res, stream_len, n):
    for c in res:
        cyc, syms = c["decode_cycles"], max(1, c["decode_syms"])
        floor = chain_floor(c, stream_len)
        say(json.dumps({"chain": name, "bytes": n, "stream_bytes": stream_len, "device_ms": round(c["decode_us"] / 1000, 1), "MB_per_s": round(n / max(1, c["decode_us"]), 2),
                        "syms_per_byte": round(syms / n, 3), "cycles_per_sym": round(cyc / syms, 1), "cycles_per_byte": round(cyc / n, 1),
                        "window_wait_share": round(c["decode_window_cycles"] / cyc, 4), "copy_share": round(c["decode_copy_cycles"] / cyc, 4),
                        "ring_bytes": c["decode_ring_bytes"], "global_bytes": c["decode_global_bytes"], "GHz": round(cyc / max(1, c["decode_us"]) / 1000, 2),
                        "floor_cycles_per_sym": round(floor / syms, 1), "achieved_over_bound": round(cyc / floor, 2)}))


tmp = tempfile.mkdtemp(prefix="nlzm_decode_")
single = {}
if "chain" in parts or "cli" in parts:
    d100 = to_dev(host_1g[:100_000_000])
    d_s, s_len, t = compress_single(d100, 100_000_000, W)
    say(f"# 100 MB of the stand-in: stream {s_len} bytes, compressed in {t:.1f} s")
    single["text"] = (d100, d_s, s_len, 100_000_000)

if "chain" in parts:
    res, back = decode_runs(single["text"][1].data_ptr(), single["text"][2], 100_000_000)
    assert bool(torch.equal(back, single["text"][0][:100_000_000]))
    report_chain("stand_in_100m_w28", res, single["text"][2], 100_000_000)
    del back
    for name, kind, n, w in (("xml_100m_w26", "xml_like", 100_000_000, 26), ("random_8m_w22", "random", 8_000_000, 22)):
        data = corpus.make(kind, n, corpus.SEED + 5)
        d_in = to_dev(data)
        d_s, s_len, t = compress_single(d_in, n, w)
        say(f"# {name}: stream {s_len} bytes, compressed in {t:.1f} s")
        res, back = decode_runs(d_s.data_ptr(), s_len, n)
        assert bool(torch.equal(back, d_in[:n]))
        report_chain(name, res, s_len, n)
        del d_in, d_s, back

container = None
if "blocks" in parts or "cli" in parts:
    d1g = to_dev(host_1g)
    cap = int(lib.nlzm_hip_compress_bound(N1G)) + K * (16 + 131072)
    d_c = torch.empty(cap, dtype=torch.uint8, device=dev)
    blen, total = (C.c_uint64 * K)(), C.c_uint64(0)
    t = time.time()
    chk(lib.nlzm_hip_compress_blocks_dev(d1g.data_ptr(), N1G, K, W, d_c.data_ptr(), cap, blen, C.byref(total)))
    say(f"# 32-block container of the stand-in: {total.value} bytes, compressed in {time.time() - t:.1f} s")
    per = (N1G + K - 1) // K
    raws = (C.c_uint64 * K)(*[min(N1G, (i + 1) * per) - min(N1G, i * per) for i in range(K)])
    container = (d1g, d_c, blen, total.value, raws)

if "blocks" in parts:
    d1g, d_c, blen, c_len, raws = container
    d_back = torch.empty(N1G, dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    set_ms, slow = [], None
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_blocks_dev(d_c.data_ptr(), c_len, K, blen, raws, d_back.data_ptr(), N1G, None, C.byref(m)))
        if i:
            c = counters()
            set_ms.append(c["decode_us"] / 1000)
            slow = c["decode_slowest_stream"]
            say(json.dumps({"blocks": "set of 32", "device_ms": round(set_ms[-1], 1), "MB_per_s": round(N1G / c["decode_us"], 1), "slowest_stream": slow,
                            "slowest_stream_cycles": c["decode_max_stream_cycles"], "GHz_slowest": round(c["decode_max_stream_cycles"] / c["decode_us"] / 1000, 2),
                            "cycles_per_sym": round(c["decode_cycles"] / c["decode_syms"], 1)}))
    assert bool(torch.equal(d_back, d1g[:N1G]))
    off = sum(blen[i] for i in range(slow))
    alone = []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_dev(d_c.data_ptr() + off, blen[slow], d_back.data_ptr(), raws[slow], C.byref(m)))
        if i:
            c = counters()
            alone.append(c["decode_us"] / 1000)
            say(json.dumps({"blocks": f"stream {slow} alone", "device_ms": round(alone[-1], 1), "cycles": c["decode_cycles"], "GHz": round(c["decode_cycles"] / c["decode_us"] / 1000, 2)}))
    ratio = min(set_ms) / min(alone)
    say(json.dumps({"gate": "streams do not slow each other", "set_ms": round(min(set_ms), 1), "slowest_alone_ms": round(min(alone), 1), "ratio": round(ratio, 3),
                    "limit": 1.25, "pass": ratio <= 1.25}))
    del d_back


def cli(*a):
    t = time.time()
    r = subprocess.run([nlzm_amd.CLI_PATH] + [str(x) for x in a], capture_output=True, text=True)
    wall = time.time() - t
    if r.returncode:
        raise SystemExit(f"nlzm {a}: {r.stdout[-600:]}{r.stderr[-300:]}")
    return wall, r.stdout


if "cli" in parts:
    d1g, d_c, blen, c_len, raws = container
    f_blocks, f_one = os.path.join(tmp, "blocks.nlzm"), os.path.join(tmp, "one.nlzm")
    d_c[:c_len].cpu().numpy().tofile(f_blocks)
    with open(f_blocks + ".idx", "w") as fi:
        fi.write(f"NLZMIDX 1 {K} {N1G} {c_len}\n")
        off = 0
        for i in range(K):
            fi.write(f"{off} {blen[i]} {raws[i]}\n")
            off += blen[i]
    single["text"][1][:single["text"][2]].cpu().numpy().tofile(f_one)
    nlzm_amd.shutdown()                                 # (the command line opens the device itself)
    for name, f, n in (("one 100 MB stream", f_one, 100_000_000), ("32-block container of 1e9", f_blocks, N1G)):
        for flag in ([], ["-gpu"]):
            walls = []
            for i in range(3):
                wall, out = cli(*flag, "t", f)
                walls.append(wall)
            say(json.dumps({"cli": name, "command": " ".join(["nlzm"] + flag + ["t"]), "wall_s": [round(w, 2) for w in walls], "best_MB_per_s": round(n / min(walls) / 1e6, 1),
                            "crc": re.search(r"CRC32 ([0-9A-F]+)", out).group(1)}))
    nlzm_amd.init(0)

if "verify" in parts:
    nlzm_amd.shutdown()
    f_in1g, f_in100 = os.path.join(tmp, "in1g.bin"), os.path.join(tmp, "in100.bin")
    host_1g.tofile(f_in1g)
    host_1g[:100_000_000].tofile(f_in100)
    for name, f, flags in (("32-block container of 1e9", f_in1g, [f"-window:{W}", f"-blocks:{K}"]), ("one 100 MB stream", f_in100, [f"-window:{W}"])):
        row = {"verify": name}
        for v in ([], ["-verify"]):
            o = os.path.join(tmp, "out.nlzm")
            for x in (o, o + ".idx"):
                if os.path.exists(x):
                    os.remove(x)
            wall, out = cli(*flags, *v, "c", f, o)
            key = "c_verify" if v else "c"
            row[key + "_wall_s"] = round(wall, 2)
            row[key + "_done_s"] = float(re.search(r"Done \(input CRC32 [0-9A-F]+, ([\d.]+) sec", out).group(1))
            mv = re.search(r"Verified \(([\d.]+) sec, ([\d.]+) of them", out)
            if mv:
                row["verify_wall_s"], row["verify_device_s"] = float(mv.group(1)), float(mv.group(2))
        say(json.dumps(row))

for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
say("# done")
