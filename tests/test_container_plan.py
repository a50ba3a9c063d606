"""CPU suite: the plan of a container compressed in sets (nlzm_amd/csrc/nlzm_container_plan.h), which nlzm_hip_compress_blocks* runs when a
container has more blocks than one persistent launch holds.  The plan is plain C++ with no device in it; the harness
(tests/host_sim/container_plan_sim.cpp) is a program of its own under AddressSanitizer and UBSan and includes the header the library includes.

The sweep (in the harness): nblocks in {1, 32, 64, 65, 66, 127, 128, 129, 1000, 65536} x set_blocks in {1, 7, 32, 64} x capacity {16, 64} x
n in {0, 1, nblocks - 1, nblocks, 10^6 + 1, and two near 2^63} -- every block in exactly one set, in order; set sizes at most the capacity and within one
of each other; nblocks <= capacity gives one set; the sets' byte ranges tile [0, n); no off + len runs over n.  Here: the block ranges a plan
prints are shard.block_range's."""
import os
import re

import pytest

from nlzm_amd import shard
from tests import simkit

NBLOCKS = [1, 32, 64, 65, 66, 127, 128, 129, 1000, 65536]
SET_BLOCKS = [1, 7, 32, 64]
CAPACITY = [16, 64]


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("container_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("container_plan_sim_san")
    assert "nlzm_amd/csrc/nlzm_container_plan.h" in simkit.compiled_from("container_plan_sim_san")
    return sim


def run(sim, *args):
    r = simkit.sh([sim, *args], 600)
    assert r.returncode == 0 and "container_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_sweep(sim):
    out = run(sim, "sweep")
    m = re.search(r"sweep: combinations=(\d+) refused=(\d+)", out)
    assert int(m.group(1)) == len(NBLOCKS) * len(SET_BLOCKS) * len(CAPACITY) * 7
    assert int(m.group(2)) == len(NBLOCKS) * 2 * 7            # set_blocks 32 and 64 at a capacity of 16: refused, nothing planned


def test_library_and_harness_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    assert '#include "nlzm_container_plan.h"' in open(os.path.join(csrc, "nlzm_hip_blocks.cpp")).read()
    assert "nlzm_container_plan.h" in open(os.path.join(simkit.SIMDIR, "container_plan_sim.cpp")).read()
    text = open(os.path.join(csrc, "nlzm_container_plan.h")).read()
    assert "hip" not in text.lower().replace("nlzm_hip", "")          # no device in it


@pytest.mark.parametrize("capacity", CAPACITY)
@pytest.mark.parametrize("nblocks", [n for n in NBLOCKS if n <= 1000])
def test_block_ranges_are_the_shards(sim, nblocks, capacity):
    for set_blocks in (s for s in SET_BLOCKS if s <= capacity):
        for n in (0, 1, nblocks - 1, nblocks, 10 ** 6 + 1):
            out = run(sim, "plan", n, nblocks, set_blocks, capacity)
            sets = [tuple(map(int, m)) for m in re.findall(r"^set (\d+) (\d+) (\d+) (\d+)$", out, re.M)]
            blocks = [tuple(map(int, m)) for m in re.findall(r"^block (\d+) (\d+) (\d+)$", out, re.M)]
            assert [b[0] for b in blocks] == list(range(nblocks))
            assert [(lo, hi) for _, lo, hi in blocks] == [shard.block_range(n, nblocks, i) for i in range(nblocks)]
            want_sets = 1 if nblocks <= capacity else -(-nblocks // set_blocks)
            assert len(sets) == want_sets
            counts = [c for _, c, _, _ in sets]
            assert sum(counts) == nblocks and max(counts) - min(counts) <= 1 and max(counts) <= capacity
            for first, count, off, ln in sets:
                assert off == blocks[first][1] and off + ln == blocks[first + count - 1][2]


def test_largest_container(sim):
    """65536 blocks by 32: 2048 sets of 32, every block a shard (one plan, held whole)"""
    n = 10 ** 6 + 1
    out = run(sim, "plan", n, 65536, 32, 64)
    sets = re.findall(r"^set (\d+) (\d+) (\d+) (\d+)$", out, re.M)
    assert len(sets) == 2048 and {int(s[1]) for s in sets} == {32}
    blocks = [tuple(map(int, m)) for m in re.findall(r"^block (\d+) (\d+) (\d+)$", out, re.M)]
    assert len(blocks) == 65536
    for i in (0, 1, 31, 32, 33, 1000, 62499, 62500, 62501, 65535):
        assert blocks[i][1:] == shard.block_range(n, 65536, i)
    assert sum(hi - lo for _, lo, hi in blocks) == n
