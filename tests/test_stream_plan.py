"""CPU suite: the launch plan of a single stream (nlzm_amd/csrc/nlzm_stream_plan.h) -- chunks per launch, and one launch set or two -- which
stream_begin makes from the device's free memory.  The plan is plain C++ with no device in it; the harness (tests/host_sim/stream_plan_sim.cpp)
is a program of its own under AddressSanitizer and UBSan and includes the header the library includes.

The rule: room = 0.6 * free - table; a launch that does not fit the room is cut to what fits (today's rule, kept); a second launch set is counted
like the first, so depth 2 needs room for two uncut launches -- and a stream of more chunks than one launch.  Hand-made figures either side of
every threshold: 1,000 bytes per chunk, launches of 10 chunks."""
import os
import re

import pytest

from tests import simkit

PER_CHUNK, BATCH, NCHUNKS = 1000, 10, 100


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("stream_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("stream_plan_sim_san")
    assert "nlzm_amd/csrc/nlzm_stream_plan.h" in simkit.compiled_from("stream_plan_sim_san")
    return sim


def plan(sim, free, table=0, per_chunk=PER_CHUNK, batch=BATCH, nchunks=NCHUNKS):
    r = simkit.sh([sim, "plan", free, table, per_chunk, batch, nchunks], 60)
    assert r.returncode == 0 and "stream_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^plan (\d+) (\d+)$", r.stdout, re.M)
    return int(m.group(1)), int(m.group(2))


# room = 0.6 * free: 20,004 / 19,998 either side of two launches (20,000); 10,002 / 9,996 either side of one (10,000)
@pytest.mark.parametrize("free,want", [
    (10 ** 9, (10, 2)),         # plenty
    (33_340, (10, 2)),          # room 20,004: two launch sets just fit
    (33_330, (10, 1)),          # room 19,998: the second does not -- today's order
    (16_670, (10, 1)),          # room 10,002: one uncut launch
    (16_660, (9, 1)),           # room 9,996: the launch is cut down, and a cut launch has no second set
    (5_000, (3, 1)),            # room 3,000
    (1_000, (10, 1)),           # room 600, less than a chunk: the batch stays and the allocation says what is wrong (as before)
])
def test_thresholds(sim, free, want):
    assert plan(sim, free) == want


def test_the_prefilter_table_comes_off_the_room(sim):
    assert plan(sim, 43_340, table=6_000) == (10, 2)            # room 26,004 - 6,000
    assert plan(sim, 43_340, table=6_010) == (10, 1)
    assert plan(sim, 43_340, table=16_010) == (9, 1)            # room 9,994


def test_a_stream_of_one_launch_has_one_set(sim):
    """nothing is queued across calls: without a second launch there is nothing to queue ahead, whatever the room"""
    assert plan(sim, 10 ** 9, nchunks=10) == (10, 1)
    assert plan(sim, 10 ** 9, nchunks=11) == (10, 2)
    assert plan(sim, 10 ** 9, batch=1, nchunks=1) == (1, 1)
    assert plan(sim, 10 ** 9, batch=1, nchunks=2) == (1, 2)


def test_library_and_harness_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    assert '#include "nlzm_stream_plan.h"' in open(os.path.join(csrc, "nlzm_hip.cpp")).read()
    assert "stream_plan::make_plan(" in open(os.path.join(csrc, "nlzm_hip.cpp")).read()
    assert "nlzm_stream_plan.h" in open(os.path.join(simkit.SIMDIR, "stream_plan_sim.cpp")).read()
    text = open(os.path.join(csrc, "nlzm_stream_plan.h")).read()
    assert "hip" not in text.lower().replace("nlzm_hip", "")          # no device in it
