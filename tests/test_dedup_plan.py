"""CPU suite: the class plan of the equal-range finder (nlzm_amd/csrc/nlzm_dedup_plan.h), which nlzm_hip_equal_ranges* runs on the fingerprints
and the pair role's verdicts.  The plan is plain C++ with no device in it; the harness (tests/host_sim/dedup_plan_sim.cpp) is a program of its own
under AddressSanitizer and UBSan and includes the header the library includes.

The sweep (in the harness): random range lists over a two-letter alphabet with the fingerprints masked to 0, 2 and 64 bits against brute force;
every round held to the plan's rules, so that every element is resolved exactly once; the rounds at most a group's distinct contents, one with
sound fingerprints; the identical-(off, len) and the empty shortcut; k = 1 and k = 65,536; a range over the buffer refused and named.  Here: plans
of range lists written by this file against tests/dedup_model.py."""
import os
import re

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import dedup_model, simkit



@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("dedup_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("dedup_plan_sim_san")
    assert "nlzm_amd/csrc/nlzm_dedup_plan.h" in simkit.compiled_from("dedup_plan_sim_san")
    return sim


def run(sim, *args):
    r = simkit.sh([sim, *args], 600)
    assert r.returncode == 0 and "dedup_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def plan(sim, tmp_path, data, ranges, bits):
    (tmp_path / "data.bin").write_bytes(bytes(data))
    (tmp_path / "ranges.txt").write_text("".join(f"{o} {l}\n" for o, l in ranges))
    out = run(sim, "plan", bits, tmp_path / "data.bin", tmp_path / "ranges.txt")
    if out.startswith("error"):
        return out, None
    first = [int(x) for x in out.splitlines()[0].split()[1:]]
    return first, {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", out.splitlines()[1])}


def test_sweep(sim):
    assert re.search(r"sweep: cases=\d+", run(sim, "sweep"))


def test_library_and_harness_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    host = open(os.path.join(csrc, "nlzm_hip_dedup.cpp")).read()
    assert '#include "nlzm_dedup_plan.h"' in host and "dedup::class_plan(" in host and "dedup::check_ranges(" in host
    harness = open(os.path.join(simkit.SIMDIR, "dedup_plan_sim.cpp")).read()
    assert "dedup::class_plan(" in harness and "dedup::check_ranges(" in harness


@pytest.mark.parametrize("bits", [0, 2, 64])
def test_plans_against_the_model(sim, tmp_path, bits):
    rng = np.random.default_rng(corpus.SEED + 130 + bits)
    for k in (1, 2, 9, 70, 1000):
        n = 200
        data = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), n).astype(np.uint8)
        ranges = []
        for _ in range(k):
            o = int(rng.integers(0, n + 1))
            ranges.append((o, int(rng.integers(0, min(9, n - o) + 1))))
        first, st = plan(sim, tmp_path, data, ranges, bits)
        want = dedup_model.first_of(data, ranges)
        assert first == want
        assert st["distinct"] == dedup_model.distinct(want) and st["dup_bytes"] == dedup_model.dup_bytes(want, ranges)
        if bits == 64:
            assert st["rounds"] <= 1
        assert st["pairs"] <= k * max(1, st["rounds"])


def test_collisions_cost_rounds_not_answers(sim, tmp_path):
    """five contents of one length under no fingerprint at all: five rounds at most, more than one, the same classes"""
    data = b"aaaa" + b"bbbb" + b"cccc" + b"dddd" + b"eeee" + b"aaaabbbb"
    ranges = [(0, 4), (4, 4), (20, 4), (8, 4), (24, 4), (12, 4), (16, 4), (0, 4), (17, 0), (3, 0)]
    sound, st64 = plan(sim, tmp_path, data, ranges, 64)
    blind, st0 = plan(sim, tmp_path, data, ranges, 0)
    assert sound == blind == [0, 1, 0, 3, 1, 5, 6, 0, 8, 8] == dedup_model.first_of(data, ranges)
    assert st64["rounds"] == 1 and st64["pairs"] == 2 and st64["compared_bytes"] == 8
    assert 1 < st0["rounds"] <= 5 and st0["pairs"] > st64["pairs"]


def test_a_range_over_the_buffer_is_named(sim, tmp_path):
    out, _ = plan(sim, tmp_path, bytes(1000), [(0, 10), (990, 11), (5, 5)], 64)
    assert out.startswith("error -1 range 1 ") and "runs over" in out
    out, _ = plan(sim, tmp_path, bytes(1000), [(0, 10), (990, 10), (1000, 0), ((1 << 64) - 1, 2)], 64)
    assert out.startswith("error -1 range 3 ")
