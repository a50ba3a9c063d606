"""Measurements of the device CRC32 (not a test; DESIGN.md section 17 holds the results, profiles/crc_measure.txt the log).

    python tests/gpu_crc.py [--out DIR] [gate] [floor] [cli] [loop]        (default: gate floor cli)

  gate     nlzm_hip_crc32_dev on the 1e9 resident bytes of the benchmark's stand-in against what it replaces for a caller whose data is in HBM:
           a device-to-host copy of the same bytes plus crc_calc over them on one host core (`nlzm h` on a file of those bytes, less the time
           the file takes to read), same run, same box.  GATE: the slowest device run < copy + host CRC, no margin.
  floor    hipMemcpyDtoD of the same bytes (the memory floor: it reads and writes them), the CRC's fraction of it and of the HBM roofline; and the
           same kernel on 64 MB that stay in the Infinity Cache, hashed sixteen times in one call's worth of bytes -- if the rate does not move
           when HBM is out of the picture, HBM was not the limit
  cli      `nlzm c -crc` against `nlzm c`: wall time, one run each, the 32-block container of the 1e9 bytes and one 100 MB stream
  loop     ten CRC calls on the resident 1e9 bytes and nothing else: what a profiler run wraps

1e9 resident bytes, one warm-up dropped, three runs, device time from the library's events ("crc_us"), profiler off."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib

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
parts = args or ["gate", "floor", "cli"]
os.makedirs(out_dir, exist_ok=True)
log = open(os.path.join(out_dir, "crc_measure.txt"), "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


N1G, K, W = bench.STREAM_BYTES, 32, bench.WINDOW
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12           # bytes per second: the data sheet's, and what streaming kernels reach on this part
t0 = time.time()
host_1g = bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0))))      # (forks: before the GPU is touched)
say(f"# stand-in made in {time.time() - t0:.1f} s; parts: {parts}")

import torch

nlzm_amd.init(0)
lib = nlzm_amd.load_library()
dev = torch.device("cuda:0")
G = nlzm_amd.counter("crc_segment_bytes")


def chk(rc):
    if rc:
        raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())


def crc_runs(ptr, n, runs=3):
    """one warm-up, `runs` timed calls -> (crc, [device microseconds])"""
    out, us = C.c_uint32(0), []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_crc32_dev(ptr, n, 0, C.byref(out)))
        if i:
            us.append(nlzm_amd.counter("crc_us"))
    return out.value, us


d1g = torch.from_numpy(host_1g).to(dev)
torch.cuda.synchronize()
tmp = tempfile.mkdtemp(prefix="nlzm_crc_")


def cli(*a):
    t = time.time()
    r = subprocess.run([nlzm_amd.CLI_PATH] + [str(x) for x in a], capture_output=True, text=True)
    wall = time.time() - t
    if r.returncode:
        raise SystemExit(f"nlzm {a}: {r.stdout[-600:]}{r.stderr[-300:]}")
    return wall, r.stdout


dev_us = None
if "gate" in parts or "floor" in parts:
    crc, dev_us = crc_runs(d1g.data_ptr(), N1G)
    say(json.dumps({"crc32_dev": "1e9 resident bytes", "segment_bytes": G, "crc": f"{crc:08X}", "device_us": dev_us, "GB_per_s": [round(N1G / u / 1e3, 1) for u in dev_us]}))

if "gate" in parts:
    want = zlib.crc32(host_1g)
    assert crc == want, (hex(crc), hex(want))
    d2h = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.time()
        back = d1g.cpu()
        d2h.append(time.time() - t)
    del back
    f = os.path.join(tmp, "in1g.bin")
    host_1g.tofile(f)
    reads, hs = [], []
    for _ in range(2):
        t = time.time()
        with open(f, "rb") as fh:
            blob = fh.read()
        reads.append(time.time() - t)
        del blob
        wall, out = cli("h", f)
        hs.append(wall)
        assert out.splitlines()[-1] == f"{want:X}"
    host_crc = min(hs) - min(reads)                  # (crc_calc alone: the command's wall time less what reading the file takes)
    replaced = min(d2h) + host_crc
    worst = max(dev_us) / 1e6
    say(json.dumps({"gate": "crc32_dev < device-to-host copy + crc_calc on one host core", "device_s_slowest_of_3": round(worst, 6), "d2h_s": [round(x, 3) for x in d2h],
                    "nlzm_h_wall_s": [round(x, 3) for x in hs], "file_read_s": [round(x, 3) for x in reads], "host_crc_s": round(host_crc, 3),
                    "replaced_s": round(replaced, 3), "ratio": round(replaced / worst, 1), "pass": worst < replaced}))
    os.remove(f)

if "floor" in parts:
    d2 = torch.empty_like(d1g)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copy_us = []
    for i in range(4):
        torch.cuda.synchronize()
        ev[0].record()
        d2.copy_(d1g)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            copy_us.append(round(1e3 * ev[0].elapsed_time(ev[1])))
    del d2
    best = min(dev_us)
    say(json.dumps({"floor": "hipMemcpyDtoD of the 1e9 bytes (reads and writes them)", "copy_us": copy_us, "copy_GB_per_s_read_plus_write": round(2 * N1G / min(copy_us) / 1e3, 1),
                    "crc_us": best, "crc_over_copy": round(best / min(copy_us), 2), "crc_GB_per_s": round(N1G / best / 1e3, 1),
                    "share_of_hbm_peak": round(N1G / best * 1e6 / HBM_PEAK, 3), "share_of_hbm_achievable": round(N1G / best * 1e6 / HBM_ACHIEVABLE, 3)}))
    # the same bytes per call out of the Infinity Cache: sixteen ranges that are all the same 64 MB
    n_small, rep = 64_000_000, 16
    off, ln, out = (C.c_uint64 * rep)(*([0] * rep)), (C.c_uint64 * rep)(*([n_small] * rep)), (C.c_uint32 * rep)()
    us = []
    for i in range(4):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_crc32_ranges_dev(d1g.data_ptr(), N1G, rep, off, ln, out))
        if i:
            us.append(nlzm_amd.counter("crc_us"))
    assert len(set(out)) == 1
    say(json.dumps({"floor": "16 x the same 64 MB in one call (served by the Infinity Cache)", "bytes": n_small * rep, "device_us": us,
                    "GB_per_s": round(n_small * rep / min(us) / 1e3, 1), "against_1e9_from_hbm_GB_per_s": round(N1G / best / 1e3, 1)}))

if "loop" in parts:
    for _ in range(3):
        crc, us = crc_runs(d1g.data_ptr(), N1G)
    say(json.dumps({"loop": "ten calls on the resident 1e9 bytes", "last_device_us": us}))

if "cli" in parts:
    del d1g
    nlzm_amd.shutdown()                                 # (the command line opens the device itself)
    f_in1g, f_in100 = os.path.join(tmp, "in1g.bin"), os.path.join(tmp, "in100.bin")
    host_1g.tofile(f_in1g)
    host_1g[:100_000_000].tofile(f_in100)
    for name, f, flags in (("32-block container of 1e9", f_in1g, [f"-window:{W}", f"-blocks:{K}"]), ("one 100 MB stream", f_in100, [f"-window:{W}"])):
        row = {"cli": name}
        for v in ([], ["-crc"]):
            o = os.path.join(tmp, "out.nlzm")
            for x in (o, o + ".idx"):
                if os.path.exists(x):
                    os.remove(x)
            wall, out = cli(*flags, *v, "c", f, o)
            key = "c_crc" if v else "c"
            row[key + "_wall_s"] = round(wall, 2)
            m = re.search(r"Done \(input CRC32 ([0-9A-F]+), ([\d.]+) sec", out)
            row[key + "_done_s"], row[key + "_crc"] = float(m.group(2)), m.group(1)
            if v:
                row["index"] = open(o + ".idx").readline().strip()
        say(json.dumps(row))

for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
say("# done")
