"""CPU suite: the plan of a call on ranges of the caller's choosing (nlzm_amd/csrc/nlzm_container_plan.h, make_ranges_plan), which
nlzm_hip_compress_ranges* runs.  The plan is plain C++ with no device in it; the harness (tests/host_sim/ranges_plan_sim.cpp) is a program of
its own under AddressSanitizer and UBSan and includes the header the library includes.

The sweep (in the harness): k <= capacity gives one set; 65 ranges by 32 are 22 + 22 + 21; 65,536 ranges; empty ranges only; a range over n,
also where off + len wraps, refused and named; a bound sum that would wrap.  Here: plans of ranges written by this file, and the equal
partition's ranges, which give the sets make_plan gives."""
import os
import re

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import simkit


def bound(n):
    return 16 + 131072 + (n // 14848 + 1) * 16384


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("ranges_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("ranges_plan_sim_san")
    assert "nlzm_amd/csrc/nlzm_container_plan.h" in simkit.compiled_from("ranges_plan_sim_san")
    return sim


def run(sim, *args):
    r = simkit.sh([sim, *args], 600)
    assert r.returncode == 0 and "ranges_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def plan(sim, tmp_path, n, ranges, set_blocks=32, capacity=64):
    f = tmp_path / "ranges.txt"
    f.write_text("".join(f"{o} {l}\n" for o, l in ranges))
    return run(sim, "plan", n, set_blocks, capacity, f)


def test_sweep(sim):
    assert re.search(r"sweep: cases=\d+", run(sim, "sweep"))


def test_library_and_harness_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    blocks = open(os.path.join(csrc, "nlzm_hip_blocks.cpp")).read()
    assert '#include "nlzm_container_plan.h"' in blocks and "container::make_ranges_plan(" in blocks
    assert "make_ranges_plan(" in open(os.path.join(simkit.SIMDIR, "ranges_plan_sim.cpp")).read()


def test_sets_of_random_ranges(sim, tmp_path):
    rng = np.random.default_rng(corpus.SEED + 80)
    n = 600_000
    for k, set_blocks, capacity in ((9, 32, 64), (64, 7, 64), (65, 32, 64), (70, 32, 64), (70, 64, 64), (200, 16, 16), (1000, 40, 64)):
        ranges = []
        for _ in range(k):
            off = int(rng.integers(0, n + 1))
            ranges.append((off, int(rng.integers(0, min(20_000, n - off) + 1))))
        out = plan(sim, tmp_path, n, ranges, set_blocks, capacity)
        m = re.search(r"^sets (\d+) out_bound (\d+)$", out, re.M)
        sets = [tuple(map(int, s)) for s in re.findall(r"^set (\d+) (\d+) (\d+)$", out, re.M)]
        want_sets = 1 if k <= capacity else -(-k // set_blocks)
        assert int(m.group(1)) == want_sets == len(sets) and int(m.group(2)) == sum(bound(l) for _, l in ranges)
        counts = [c for _, c, _ in sets]
        assert sum(counts) == k and max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True)
        for first, count, longest in sets:
            assert longest == max(l for _, l in ranges[first: first + count])


def test_a_range_over_the_input_is_named(sim, tmp_path):
    out = plan(sim, tmp_path, 1000, [(0, 10), (990, 11), (5, 5)])
    assert out.startswith("error -1 range 1 ") and "runs over" in out
    out = plan(sim, tmp_path, 1000, [(0, 10), (990, 10), (1000, 0), ((1 << 64) - 1, 2)])
    assert out.startswith("error -1 range 3 ")


@pytest.mark.parametrize("nblocks", [1, 32, 64, 65, 66, 129, 1000, 65536])
def test_the_equal_partition_gives_make_plans_sets(sim, nblocks):
    for set_blocks, capacity in ((32, 64), (7, 16), (64, 64)):
        for n in (0, 1, nblocks - 1, nblocks, 10 ** 6 + 1):
            out = run(sim, "equal", n, nblocks, set_blocks, capacity)
            assert int(re.search(r"equal: sets=(\d+)", out).group(1)) == (1 if nblocks <= capacity else -(-nblocks // set_blocks))
