"""CPU suite: the host plan of the element-size statistic (nlzm_amd/csrc/nlzm_elem_plan.h), which the entry points of include/nlzm_hip_elem.h run before
any launch: the argument checks, the launch's table, the scratch layout and the choice.  The plan is plain C++ with no device in it; the harness
(tests/host_sim/elem_plan_sim.cpp) is a program of its own under AddressSanitizer and UBSan and includes the header the library includes.  It is compiled
here with one line that carries the flags of the Makefile's PLAIN + BOTH rows (tests/host_sim/Makefile's table is not this change's to touch).

The sweep (in the harness): random range lists against brute force, the table and the scratch against their definitions, elem::choose against a
restatement in 128-bit integers, k = 1 and k = 65,536, offsets that wrap, lengths round 2^40.  Here: lists written by this file, what the errors say,
and the choice against tests/elem_model.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import elem_model, simkit

E_ARG = -1
FLAGS = "-O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined".split()


@pytest.fixture(scope="module")
def sim():
    mk = open(os.path.join(simkit.SIMDIR, "Makefile")).read()
    plain, both = (re.search(rf"^{name}\s*=\s*(.*)$", mk, re.M).group(1).split() for name in ("PLAIN", "BOTH"))
    assert FLAGS == plain + both                     # (the rows' flags as they stand)
    out = os.path.join(simkit.SIMDIR, "elem_plan_sim_san")
    r = subprocess.run(["g++", *FLAGS, "-MMD", "-MP", "-MF", out + ".d", "-MT", "elem_plan_sim_san", "-o", out, "elem_plan_sim.cpp"], cwd=simkit.SIMDIR, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nlzm_amd/csrc/nlzm_elem_plan.h" in open(out + ".d").read()
    return out


def run(sim, *args):
    r = simkit.sh([sim, *args], 600)
    assert r.returncode == 0 and "elem_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def check(sim, tmp_path, ranges, n=1 << 20, segment=65536, hist=0):
    (tmp_path / "ranges.txt").write_text("".join(f"{a} {b}\n" for a, b in ranges))
    return run(sim, "check", n, segment, hist, tmp_path / "ranges.txt")


def test_sweep(sim):
    assert re.search(r"sweep: cases=\d+ refused=\d+", run(sim, "sweep"))


def test_library_and_harnesses_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    host = open(os.path.join(csrc, "nlzm_hip_elem.cpp")).read()
    assert '#include "nlzm_elem_plan.h"' in host
    for name in ("elem::check_ranges(", "elem::Table", "elem::Scratch", "elem::choose("):
        assert name in host, name
    assert "runs over" not in host and "2^40" not in host          # (the checks are the plan's, not copies in the host file)
    for harness in ("elem_plan_sim.cpp", "elem_sim.cpp"):
        text = open(os.path.join(simkit.SIMDIR, harness)).read()
        assert "nlzm_elem_plan.h" in text and "elem::check_ranges(" in text and "elem::Table" in text, harness
    plan = open(os.path.join(csrc, "nlzm_elem_plan.h")).read()
    assert "hip_runtime" not in plan and "__device__" not in plan and "xw.h" not in plan          # (no device in it)
    for const in (r"kMinLen = 4096;", r"kShare = 32;", r"kMaxLen = 1ull << 40;"):
        assert const in plan, const
    assert (elem_model.MIN_LEN, elem_model.SHARE, elem_model.MAX_LEN) == (4096, 32, 1 << 40)


def test_the_table(sim, tmp_path):
    S = 65536
    ranges = [(0, 8), (5, 0), (100, S + 7), (3, 7), (0, S + 8), (9, 3 * S), (1, S)]
    out = check(sim, tmp_path, ranges).splitlines()
    # ranges 2 (S + 7 bytes: S whole ones), 3 (under eight bytes) and 6 are not wide; 4 (two segments) and 5 are
    assert out[0] == f"ok nsegs 8 nwide 2 slots 2 scratch {8 * (4 * 7 + 1 + 2) + 32 * 7 + 2 * 16384}"
    assert out[1] == "0 1 1 2 2 4 7 8" and out[2] == "- - - - 0 1 -" and out[3] == "4 5"
    out = check(sim, tmp_path, ranges, hist=1).splitlines()
    assert out[0] == f"ok nsegs 8 nwide 2 slots 7 scratch {8 * (4 * 7 + 1 + 2) + 32 * 7 + 7 * 16384}"
    assert out[2] == "0 1 2 3 4 5 6" and out[3] == "4 5"
    out = check(sim, tmp_path, [(0, 100), (0, 15), (0, 16), (0, 17)], segment=16).splitlines()
    assert out[0].startswith("ok nsegs 9 nwide 1 ") and out[1] == "0 6 7 8 9"


def test_every_error_names_its_range(sim, tmp_path):
    M = 1 << 64
    cases = [
        ([(0, 10), (9991, 10)], 10000, "range 1 (offset 9991, 10 bytes) runs over the 10000 bytes of the buffer"),
        ([(M - 1, 2)], 10000, "range 0 "),
        ([(0, 10), (20, M - 1)], 10000, "range 1 "),
        ([(0, 10), (0, 1 << 40)], 1 << 41, "range 1 (offset 0, 1099511627776 bytes): the statistic takes ranges below 2^40 bytes"),
    ]
    for ranges, n, text in cases:
        out = check(sim, tmp_path, ranges, n=n)
        assert out.startswith(f"error {E_ARG} ") and text in out, (ranges, out)
    assert check(sim, tmp_path, [(0, (1 << 40) - 1)], n=1 << 40).startswith("ok ")
    assert check(sim, tmp_path, [(10000, 0), (0, 10000), (3, 0)], n=10000).startswith("ok ")      # (empty ranges, one at the buffer's end)


def test_choose_is_the_models(sim):
    """the plan's choice against tests/elem_model.py: costs of real inputs, and the three rules at their edges"""
    rng = np.random.default_rng(corpus.SEED + 310)
    cases = [((100, 90, 80, 70), 4095), ((100, 90, 80, 70), 4096), ((3200, 3100, 3100, 3100), 5000), ((3200, 3101, 3101, 3101), 5000),
             ((50, 50, 50, 50), 9000), ((90, 50, 50, 50), 9000), ((90, 60, 50, 50), 9000), ((0, 0, 0, 0), 1 << 30), ((1 << 59, (1 << 59) - (1 << 54), 1 << 59, 1 << 59), 1 << 39)]
    w = (rng.standard_normal(4096) * 0.02).astype("<f4")
    for x in (w.tobytes(), (w.view("<u4") >> 16).astype("<u2").tobytes(), corpus.syn_text(9000).tobytes(), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()):
        cases.append((elem_model.costs(x), len(x)))
    for c, n in cases:
        got = int(run(sim, "choose", *c, n).split()[0])
        assert got == elem_model.choose(c, n), (c, n, got)
