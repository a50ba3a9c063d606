"""Measurements of containers compressed in sets and of the small-ring decode kernel (not a test; DESIGN.md section 21 holds the results,
profiles/container_measure.txt the log).

    python tests/gpu_container.py [--out DIR] [--label NAME] [--cache DIR] PART ...

Input: the 1e9-byte stand-in of bench.py at -window:28.  Buffers resident, profiler off, one warm-up dropped, three timed runs; decode device time
from the library's events ("decode_us"), compress time on the wall clock round the one call (its begin and finish are what a change of the
one-shot form could cost) with the device time of its steps in the `stage_report` lines beside it.  A build of the parent commit, or one with another small ring,
is loaded through NLZM_LIB; --label says which library a line comes from, --cache DIR hands files from one process to the next.

  gate12      32 blocks through nlzm_hip_compress_blocks_dev, and that container's decode (nlzm_hip_decompress_blocks_dev): run with this tree and
              with the parent, `verdict` compares.
  make1024    a 1024-block container made in sets, kept in the cache
  dec1024:R   ... decoded with decode_ring = R (a library without the option -- the parent -- takes R = none)
  verdict     gates 1 - 3 from the log's lines: this tree's median <= the parent's median + 2 x the parent's (max - min); the small ring stays the
              automatic choice only if its median lies below the parent's 64 KiB median by more than 2 x the parent's (max - min)
  widths      compress at 64, 65, 256 and 4096 blocks with stage_report on (32 and 1024 are gate12's and make1024's), every container decoded with
              the automatic choice and written to the cache with its index for `nlzm t`
  file        the stand-in as a file in the cache (for `nlzm c` and `nlzm c -verify` at 1024 blocks)
  ranges      a 4 KiB read that ends 50 % into a block, at 32 and at 1024 blocks"""
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
cache = opt("--cache", "/tmp/nlzm_container_cache")
parts = args
os.makedirs(out_dir, exist_ok=True)
os.makedirs(cache, exist_ok=True)
LOG = os.path.join(out_dir, "container_measure.txt")
log = open(LOG, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def spread(v):
    return {"runs": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "max_minus_min": round(max(v) - min(v), 2)}


if parts == ["verdict"]:
    rows = [json.loads(l) for l in open(LOG) if l.startswith("{")]

    def last(**kw):
        hit = [r for r in rows if all(r.get(k) == v for k, v in kw.items())]
        return hit[-1] if hit else None

    def gate(name, mine, ref, must_win=False):
        if not mine or not ref:
            say(json.dumps({"gate": name, "error": "a run is missing"}))
            return
        m, p, sp = mine["ms"]["median"], ref["ms"]["median"], ref["ms"]["max_minus_min"]
        ok = m < p - 2 * sp if must_win else m <= p + 2 * sp
        say(json.dumps({"gate": name, "this_ms": m, "parent_ms": p, "parent_max_minus_min": sp, "bound_ms": round(p - 2 * sp if must_win else p + 2 * sp, 2),
                        "ratio": round(m / p, 4), "pass": ok}))

    gate("1: one set of 32 blocks is not slower (wall ms of nlzm_hip_compress_blocks_dev)", last(what="compress32", label="this tree"), last(what="compress32", label="parent"))
    gate("2: the 32-block container's decode is what it was (device ms)", last(what="decode32", label="this tree"), last(what="decode32", label="parent"))
    ref = last(what="dec1024", label="parent")
    gate("3a: 1024 blocks, this tree's 64 KiB kernel against the parent's (device ms)", last(what="dec1024", label="this tree", ring=65536), ref)
    gate("3b: 1024 blocks, the 16 KiB ring must win by more than twice the parent's spread", last(what="dec1024", label="this tree", ring=16384), ref, must_win=True)
    gate("3c: 1024 blocks, the 8 KiB ring must win by more than twice the parent's spread", last(what="dec1024", label="ring 8 KiB", ring=8192), ref, must_win=True)
    raise SystemExit(0)

N1G, W = bench.STREAM_BYTES, bench.WINDOW
t0 = time.time()
host_1g = bench.stand_in(N1G, corpus.SEED, min(16, len(os.sched_getaffinity(0))))       # (forks: before the GPU is touched)
say(f"# [{label}] library {os.environ.get('NLZM_LIB') or 'nlzm_amd/libnlzm_hip.so'}; stand-in made in {time.time() - t0:.1f} s; parts: {parts}")

import torch

lib = nlzm_amd.load_library()
if lib.nlzm_hip_init(0):
    raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())
dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count


def chk(rc):
    if rc:
        raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())


def counter(key, default=None):
    v = C.c_uint64(0)
    if lib.nlzm_hip_get_counter(key.encode(), C.byref(v)):
        if default is None:
            raise SystemExit("library error: " + lib.nlzm_hip_last_error().decode())
        return default
    return int(v.value)


def to_dev(a, pad=4096):
    t = torch.zeros(a.size + pad, dtype=torch.uint8, device=dev)
    t[:a.size].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


d_in = to_dev(host_1g)
d_back = torch.empty(N1G, dtype=torch.uint8, device=dev)
CAP = int(N1G * 0.5)                                  # (the stand-in compresses to 22 - 31 % at these widths; dst_cap is checked by the library)
d_c = torch.empty(CAP, dtype=torch.uint8, device=dev)


def raws_of(k):
    per = -(-N1G // k)
    return [min(N1G, (i + 1) * per) - min(N1G, i * per) for i in range(k)]


def compress(k, runs=1):
    """-> (wall ms of every run, block lengths, total)"""
    blen, total, ms = (C.c_uint64 * k)(), C.c_uint64(0), []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        chk(lib.nlzm_hip_compress_blocks_dev(d_in.data_ptr(), N1G, k, W, d_c.data_ptr(), CAP, blen, C.byref(total)))
        torch.cuda.synchronize()
        ms.append(1000 * (time.perf_counter() - t))
    return ms, blen, int(total.value)


def decode(d_src, src_len, k, blen, runs=4, check=True):
    """the container at d_src decoded `runs` times, the first dropped -> device ms of the others"""
    raws = (C.c_uint64 * k)(*raws_of(k))
    total, ms = C.c_uint64(0), []
    for i in range(runs):
        torch.cuda.synchronize()
        chk(lib.nlzm_hip_decompress_blocks_dev(d_src.data_ptr(), src_len, k, blen, raws, d_back.data_ptr(), N1G, None, C.byref(total)))
        assert total.value == N1G
        if i:
            ms.append(counter("decode_us") / 1000)
    if check:
        assert bool(torch.equal(d_back, d_in[:N1G]))
    return ms


def save(name, k, blen, total):
    """container and NLZMIDX 1 index into the cache (for `nlzm t`, and for the next process)"""
    d_c[:total].cpu().numpy().tofile(os.path.join(cache, name))
    with open(os.path.join(cache, name + ".idx"), "w") as f:
        f.write(f"NLZMIDX 1 {k} {N1G} {total}\n")
        off = 0
        for ln, raw in zip(blen, raws_of(k)):
            f.write(f"{off} {ln} {raw}\n")
            off += ln


def load(name, k):
    blob = np.fromfile(os.path.join(cache, name), dtype=np.uint8)
    lens = [int(l.split()[1]) for l in open(os.path.join(cache, name + ".idx")).read().splitlines()[1:]]
    assert len(lens) == k and sum(lens) == blob.size
    return to_dev(blob), blob.size, (C.c_uint64 * k)(*lens)


for part in parts:
    if part == "gate12":
        ms, blen, total = compress(32, runs=4)
        say(json.dumps({"what": "compress32", "label": label, "ms": spread(ms[1:]), "MB_per_s": round(N1G / statistics.median(ms[1:]) / 1000, 2), "out_bytes": total,
                        "sets": counter("container_sets", -1)}))
        dms = decode(d_c, total, 32, blen)
        say(json.dumps({"what": "decode32", "label": label, "ms": spread(dms), "MB_per_s": round(N1G / statistics.median(dms) / 1000, 2), "ring": counter("decode_ring_size", -1)}))
    elif part == "make1024":
        chk(lib.nlzm_hip_set_option(b"stage_report", 0))
        ms, blen, total = compress(1024)
        say(json.dumps({"what": "compress", "label": label, "blocks": 1024, "wall_ms": round(ms[0], 1), "MB_per_s": round(N1G / ms[0] / 1000, 2), "out_bytes": total,
                        "sets": counter("container_sets"), "pool_bytes": counter("block_pool_bytes"), "redo": counter("block_redo_streams")}))
        save("c1024.nlzm", 1024, blen, total)
    elif part.startswith("dec1024"):
        ring = part.split(":")[1] if ":" in part else "none"
        d_s, s_len, blen = load("c1024.nlzm", 1024)
        if ring != "none":
            chk(lib.nlzm_hip_set_option(b"decode_ring", int(ring)))
        dms = decode(d_s, s_len, 1024, blen)
        say(json.dumps({"what": "dec1024", "label": label, "asked": ring, "ring": counter("decode_ring_size", 65536), "ms": spread(dms),
                        "MB_per_s": round(N1G / statistics.median(dms) / 1000, 2), "ring_bytes": counter("decode_ring_bytes"), "global_bytes": counter("decode_global_bytes")}))
        if ring != "none":
            chk(lib.nlzm_hip_set_option(b"decode_ring", 0))
        del d_s
    elif part == "widths":
        for k in (64, 65, 256, 4096):
            chk(lib.nlzm_hip_set_option(b"stage_report", 1 if k <= 256 else 0))      # (a line per set on stderr: 128 sets would be the log)
            say(f"# compress, {k} blocks (stage_report lines follow on stderr)")
            ms, blen, total = compress(k)
            chk(lib.nlzm_hip_set_option(b"stage_report", 0))
            say(json.dumps({"what": "compress", "label": label, "blocks": k, "wall_ms": round(ms[0], 1), "MB_per_s": round(N1G / ms[0] / 1000, 2), "out_bytes": total,
                            "sets": counter("container_sets"), "pool_bytes": counter("block_pool_bytes"), "redo": counter("block_redo_streams")}))
            dms = decode(d_c, total, k, blen, runs=3)
            say(json.dumps({"what": "decode", "label": label, "blocks": k, "ring": counter("decode_ring_size"), "ms": spread(dms), "MB_per_s": round(N1G / statistics.median(dms) / 1000, 2)}))
            if k in (256, 4096):
                save(f"c{k}.nlzm", k, blen, total)
    elif part == "ranges":
        for k in (32, 1024):
            ms, blen, total = compress(k)
            raws = raws_of(k)
            b = k // 2
            off = sum(raws[:b]) + raws[b] // 2 - 4096
            roff, rlen, got = (C.c_uint64 * 1)(off), (C.c_uint64 * 1)(4096), C.c_uint64(0)
            us, wall = [], []
            for i in range(4):
                torch.cuda.synchronize()
                t = time.perf_counter()
                chk(lib.nlzm_hip_read_ranges_dev(d_c.data_ptr(), total, k, blen, (C.c_uint64 * k)(*raws), None, 1, roff, rlen, d_back.data_ptr(), 4096, C.byref(got), None))
                torch.cuda.synchronize()
                if i:
                    wall.append(1000 * (time.perf_counter() - t))
                    us.append(counter("range_us") / 1000)
            assert bool(torch.equal(d_back[:4096], d_in[off:off + 4096]))
            say(json.dumps({"what": "range4k", "label": label, "blocks": k, "block_bytes": raws[b], "device_ms": spread(us), "wall_ms": spread(wall),
                            "decoded_bytes": counter("range_decoded_bytes"), "ring": counter("decode_ring_size")}))
    elif part == "file":
        host_1g.tofile(os.path.join(cache, "standin.bin"))
    else:
        raise SystemExit(f"unknown part {part}")

say(f"# [{label}] done")
