"""GPU suite (-m gpu): the stages of the persistent kernel read the launch's arguments role by role, and what only a rare branch needs inside
that branch.  A field that is dropped or copied wrong on the way shows at the smallest shapes that use it: state carried
from one launch to the next and positions beyond 2W, a block set (the arguments come from the pack in device memory), pair lists beyond four
record-setters (the extension arena's fields), the carried RK256 match and the u16 cap, hot-bin waves, and the stage report's event counters.

Every case: the stream's SHA-256 and length and the operation counters of nlzm_amd.stats() against tests/oracle_py.compress(..., want_stats=True)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

import bench
from nlzm_amd import corpus, shard
from tests import cases, oracle_py

pytestmark = pytest.mark.gpu

# the operation counters both sides keep; the oracle's cmp_bytes_needed is what the pipeline's cmp_bytes counts
OPS = ("bt_calls", "bt_tests", "cmp_bytes", "ht_rows", "rk_probes", "rk_inserts", "positions", "nice_positions", "segments")
N, HIST_BITS = 300_000, 18
# the counters of bench.STAGE_COUNTERS that count events, not cycles
EVENTS = tuple(k for k in bench.STAGE_COUNTERS if not k.endswith("_cycles"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tests", "golden", "stage_views_parent_counters.json")


def digest(stream: bytes):
    return hashlib.sha256(stream).hexdigest(), len(stream)


def op_counters(ost: dict) -> dict:
    return {k: ost["cmp_bytes_needed" if k == "cmp_bytes" else k] for k in OPS}


@functools.lru_cache(maxsize=None)
def text():
    return corpus.syn_text(N)


@functools.lru_cache(maxsize=None)
def want_text():
    """-> (sha, length), operation counters of the oracle for the 300,000 bytes as one stream"""
    stream, ost = oracle_py.compress(text(), HIST_BITS, want_stats=True)
    return digest(stream), op_counters(ost)


def check(gpu, got: bytes, want):
    assert digest(got) == want[0]
    st = gpu.stats()
    assert {k: st[k] for k in OPS} == want[1]


def test_two_launches_carry_the_state(gpu):
    """three chunks in two launches: what a launch leaves for the next, and positions beyond 2W"""
    gpu.set_option("batch_chunks", 2)
    try:
        got = gpu.compress(text(), HIST_BITS)
    finally:
        gpu.set_option("batch_chunks", 32)
    check(gpu, got, want_text())


BLOCK_SET_CHILD = """
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import nlzm_amd
from nlzm_amd import corpus
nlzm_amd.init(0)
got = nlzm_amd.compress_blocks(corpus.syn_text(int(sys.argv[2])), 2, int(sys.argv[3]))
print(json.dumps({"streams": [[hashlib.sha256(s).hexdigest(), len(s)] for s in got], "stats": nlzm_amd.stats()}))
nlzm_amd.shutdown()
"""


def test_block_set_of_two(gpu):
    """the same bytes as a block set of two blocks (pipeline2_multi_kernel: the arguments lie in device memory).  In a process of its own: the
    library's counters after a block set are the set's only while no single stream of an earlier call is still open in the process."""
    data = text()
    r = subprocess.run([sys.executable, "-c", BLOCK_SET_CHILD, ROOT, str(N), str(HIST_BITS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    total = {k: 0 for k in OPS}
    for i in range(2):
        lo, hi = shard.block_range(data.size, 2, i)
        ref, ost = oracle_py.compress(data[lo:hi], HIST_BITS, want_stats=True)
        assert tuple(got["streams"][i]) == digest(ref), f"block {i}"
        for k, v in op_counters(ost).items():
            total[k] += v
    assert {k: got["stats"][k] for k in OPS} == total


@pytest.mark.parametrize("name", ["spines_400k_w18", "u16cut_734k_w24"])
def test_rare_paths(gpu, name):
    """pair lists beyond four record-setters (the extension fields are read where a fifth pair turns up); the carried RK256 match and the u16 cap"""
    case = next(c for c in cases.CASES if c[0] == name)
    data = cases.make_case(case)
    stream, ost = oracle_py.compress(data, case[4], want_stats=True)
    check(gpu, gpu.compress(data, case[4]), (digest(stream), op_counters(ost)))


def test_hot_bin_waves_at_this_size(gpu):
    """hot-bin waves from 64 positions a bin on: they run at this size"""
    gpu.set_option("batch_chunks", 2); gpu.set_option("hot_min", 64)
    try:
        got = gpu.compress(text(), HIST_BITS)
        hot = gpu.counter("hot_bin_calls")
    finally:
        gpu.set_option("hot_min", 0); gpu.set_option("batch_chunks", 32)
    check(gpu, got, want_text())
    assert hot > 0


# Which event counters the data alone decides, and which hang on how the stages' waits fall: the parser stage cuts a block short when the records it
# waits for have not come after kGatherRounds loader steps (parser_blocks, and parser_passes with it); a worker lane's call is timed, and its
# tests counted in worker_call_tests, only when its fate was known when it started; a helper's job is taken over only if it is done in time.
# The parent's own two runs of the fixture differ in exactly such counters (parser_passes by 1 in 35,424, worker_call_tests by 53 in 1,229,537).
EXACT = ("positions", "helper_jobs", "worker_calls", "hot_bin_calls")
TIMED = ("parser_passes", "parser_blocks", "worker_call_tests")     # within 0.1 % of the parent's: 25 times what its own runs differ by
TIMED_REL = 1e-3


def test_stage_report_events_are_the_parents(gpu, capfd):
    """with the stage report on, the event counters of bench.STAGE_COUNTERS against what the parent's library counted for the same input
    (tests/golden/stage_views_parent_counters.json: a build of the parent commit, same machine): equal where the data decides the count;
    where the stages' timing has a say (above), within 0.1 % of the parent's, and the helper's take-overs within what its jobs allow"""
    with open(PARENT) as f:
        parent = json.load(f)["counters"]
    assert set(EVENTS) == set(EXACT) | set(TIMED) | {"helper_taken", "helper_taken_nodes"}
    gpu.set_option("batch_chunks", 2); gpu.set_option("stage_report", 1)
    try:
        got = gpu.compress(text(), HIST_BITS)
    finally:
        gpu.set_option("stage_report", 0); gpu.set_option("batch_chunks", 32)
    assert "cycles/position" in capfd.readouterr().err
    check(gpu, got, want_text())
    mine = {k: gpu.counter(k) for k in EVENTS}
    print(mine)
    assert {k: mine[k] for k in EXACT} == {k: parent[k] for k in EXACT}
    for k in TIMED:
        assert abs(mine[k] - parent[k]) <= TIMED_REL * parent[k], k
    assert mine["helper_taken"] <= mine["helper_jobs"] and mine["helper_taken_nodes"] <= 4096 * mine["helper_taken"]
