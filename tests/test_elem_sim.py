"""CPU suite: the count role and the total role of the element-size statistic (nlzm_amd/csrc/nlzm_elem.h) compiled for the host with every GPU lane a
fiber (tests/host_sim/elem_sim.cpp, a UBSan build, a program of its own), against the model (tests/elem_model.py): every cost and -- through the CRC32
of a range's 2,048 totals -- every counter, exact.  The harness is compiled here with one line that carries the flags of the Makefile's FIBER + UBSAN
rows (tests/host_sim/Makefile's table is not this change's to touch).

Every source lies in a mapping of its own between two PROT_NONE pages -- at the asked misalignment behind the page in front, or with its last byte
flush against the page behind --, so a read outside a range that leaves the mapping ends the harness; the totals and the costs lie between canaries;
LDS starts poisoned.  The case list is dealt to eight harness processes."""
import os
import re
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import elem_model, simkit

SIM = os.path.join(simkit.SIMDIR, "elem_sim_san")
SHARDS = 8
FLAGS = "-O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function -fsanitize=undefined -fno-sanitize-recover=undefined".split()
sh = partial(simkit.sh, timeout=900, env={"NLZM_SIM_POISON": "7"})


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    mk = open(os.path.join(simkit.SIMDIR, "Makefile")).read()
    fiber, ubsan = (re.search(rf"^{name}\s*=\s*(.*)$", mk, re.M).group(1).split() for name in ("FIBER", "UBSAN"))
    assert FLAGS == fiber + ubsan                    # (the rows' flags as they stand)
    r = subprocess.run(["g++", *FLAGS, "-MMD", "-MP", "-MF", SIM + ".d", "-MT", "elem_sim_san", "-o", SIM, "elem_sim.cpp"], cwd=simkit.SIMDIR, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    deps = open(SIM + ".d").read()
    assert "nlzm_amd/csrc/nlzm_elem.h" in deps and "nlzm_amd/csrc/nlzm_elem_plan.h" in deps and "nlzm_amd/csrc/xw.h" in deps
    d = tmp_path_factory.mktemp("elem_sim")
    (d / "g.txt").write_text("G\n")
    (d / "none.bin").write_bytes(b"")
    r = sh([SIM, d / "none.bin", d / "g.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    S = int(r.stdout.split()[0])
    assert S % 16 == 0
    # bytes that tell their classes apart: typed content (fp32 weights, small int64), text, a stretch of one repeated byte, one of a counter
    rng = np.random.default_rng(corpus.SEED + 300)
    n = 2 * S + 300
    data = np.concatenate([(rng.standard_normal(n // 8) * 0.02).astype("<f4").view(np.uint8), rng.integers(0, 1000, n // 16 + 8, dtype="<i8").view(np.uint8)])[:n].copy()
    data[3000:5000] = corpus.syn_text(2000)
    data[6000:7100] = 0x41
    data[8000:9100] = np.arange(1100, dtype=np.uint32).astype(np.uint8)
    (d / "data.bin").write_bytes(data.tobytes())
    return {"dir": d, "S": S, "data": data, "n": 0, "memo": {}}


def want(sim, s, n):
    key = (s, n)
    if key not in sim["memo"]:
        x = sim["data"][s: s + n]
        H = elem_model.hist(x)
        sim["memo"][key] = (elem_model.costs_of_hist(H), f"{zlib.crc32(H.astype('<u8').tobytes()):08x}")
    return sim["memo"][key]


def run_launches(sim, launches, name="data.bin"):
    """launches: [(hist, [(mode, salign, start, n), ...])]; every range's costs, and its totals where they were kept, are held to the model"""
    d = sim["dir"]
    sim["n"] += 1
    shards = [launches[i::SHARDS] for i in range(SHARDS)]
    for i, sl in enumerate(shards):
        # (the launch's shape moves with the case: one to four waves per workgroup, one to three workgroups striding over the segments)
        (d / f"cases_{sim['n']}_{i}.txt").write_text("".join(
            f"L {64 * (1 + (j + len(rs)) % 4)} {1 + (j + rs[0][3]) % 3} {len(rs)} {hist}\n" + "".join(f"{m} {sa} {s} {n}\n" for m, sa, s, n in rs)
            for j, (hist, rs) in enumerate(sl)))
    with ThreadPoolExecutor(SHARDS) as ex:
        rs = list(ex.map(lambda i: sh([SIM, d / name, d / f"cases_{sim['n']}_{i}.txt"]), range(SHARDS)))
    bad = []
    for i, r in enumerate(rs):
        assert r.returncode == 0 and "elem_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]       # (-11: a read left a range)
        lines = r.stdout.splitlines()[:-1]
        assert len(lines) == sum(len(rs_) for _, rs_ in shards[i])
        at = 0
        for hist, ranges in shards[i]:
            for (m, sa, s, n) in ranges:
                got = lines[at].split()
                at += 1
                costs, crc = want(sim, s, n)
                wide = (n // 8 * 8 + sim["S"] - 1) // sim["S"] > 1
                if tuple(int(g) for g in got[:4]) != costs or got[4] != (crc if hist or wide else "-"):
                    bad.append((hist, m, sa, s, n, got, costs, crc))
    assert not bad, bad[:4]


def grouped(ranges, per=8):
    return [ranges[i: i + per] for i in range(0, len(ranges), per)]


@pytest.mark.parametrize("hist", [0, 1])
def test_every_length_against_the_model(sim, hist):
    """every n from 0 to 2,100 and S - 1, S, S + 1, 2S + 11; sources behind the page in front and against the page behind in turn"""
    S = sim["S"]
    rs = [("FB"[n % 2], n % 16, (3 * n) % 251 + (2900 if n % 3 == 0 else 5900 if n % 3 == 1 else 0), n) for n in range(0, 2101)]
    for n in (S - 1, S, S + 1, 2 * S + 11):
        rs += [("F", 0, 7, n), ("B", 0, 11, n), ("F", 9, 13, n)]
    run_launches(sim, [(hist, g) for g in grouped(rs)])


def test_every_source_misalignment(sim):
    """every source misalignment from 0 to 15 for some twenty lengths, the ones round the segment size among them"""
    S = sim["S"]
    lengths = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 33, 127, 128, 129, 1000, 1023, 1025, 4095, 4096]
    rs = [("F", sa, (5 * n + sa) % 251, n) for n in lengths for sa in range(16)]
    rs += [("F", sa, sa, n) for sa in range(16) for n in ((S - 1, S, S + 1, 2 * S + 11)[sa % 4], (S + 1, 2 * S + 11, S - 1, S)[sa % 4])]
    run_launches(sim, [(i % 2, g) for i, g in enumerate(grouped(rs))])


def test_hundreds_of_ranges_in_one_launch(sim):
    """one launch of 600 ranges of one buffer that overlap, repeat and include empty ones, three of them longer than a segment; with and without the
    histograms"""
    S = sim["S"]
    rng = np.random.default_rng(corpus.SEED + 301)
    rs = []
    for i in range(600):
        n = 0 if i % 37 == 5 else int(rng.integers(1, 3000))
        s = int(rng.integers(0, 12000))
        rs.append(("D", 0, s, n) if i % 11 else rs[i - 3] if i > 3 else ("D", 0, 0, 64))
    rs[100], rs[300], rs[301] = ("D", 0, 3, S + 1000), ("D", 0, 50, 2 * S + 11), ("D", 0, 50, 2 * S + 11)
    run_launches(sim, [(0, rs), (1, rs), (0, rs[::-1])])


def test_one_repeated_byte_and_a_counter(sim):
    """buffers of one repeated byte (every lane on one counter) and of a counter i mod 256 (every lane on one bank, but for the lanes' order)"""
    S, d = sim["S"], sim["dir"]
    keep = sim["data"], sim["memo"]
    try:
        for name, data in (("same.bin", np.full(2 * S + 300, 0x5A, dtype=np.uint8)), ("count.bin", np.arange(2 * S + 300, dtype=np.uint32).astype(np.uint8))):
            (d / name).write_bytes(data.tobytes())
            sim["data"], sim["memo"] = data, {}
            rs = [("FB"[i % 2], (3 * i) % 16, i % 7, n) for i, n in enumerate((0, 8, 16, 24, 1000, 1024, 1032, 4096, 16 * 64, 16 * 64 + 8, 16 * 65, 16 * 256, 16 * 257 + 8, S - 1, S, S + 1, 2 * S + 11))]
            run_launches(sim, [(i % 2, g) for i, g in enumerate(grouped(rs))], name)
    finally:
        sim["data"], sim["memo"] = keep


def test_the_segment_size_is_the_librarys(sim):
    import nlzm_amd
    nlzm_amd.build()
    assert nlzm_amd.counter("elem_segment_bytes") == sim["S"]
