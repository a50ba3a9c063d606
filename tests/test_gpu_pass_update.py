"""GPU suite (-m gpu): the parser's pass update computes what it computed.  The update asks for its LDS words in
every lane and chooses between values where it used to branch, in the parser stage and in the helper parsers alike; each arm of it is
reached here at the smallest input that has it, and the stream's SHA-256 and length and the operation counters of nlzm_amd.stats() are held
against tests/oracle_py.compress(..., want_stats=True).  A pass that computes what it computed also takes the same number of passes: the
parser's pass and block counters against a build of the parent commit (tests/golden/pass_update_parent_counters.json)."""
import functools
import hashlib
import json
import os

import pytest

from nlzm_amd import corpus
from tests import cases, oracle_py

pytestmark = pytest.mark.gpu

OPS = ("bt_calls", "bt_tests", "cmp_bytes", "ht_rows", "rk_probes", "rk_inserts", "positions", "nice_positions", "segments")
N, HIST_BITS = 300_000, 18
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tests", "golden", "pass_update_parent_counters.json")
# what each input reaches in the update
ARMS = {
    "random_100k_w15": "literal runs across whole blocks, node 0 / kSrcNone",
    "runs_300k_w15": "rep winners, probe winners (rank >= kRankProbe)",
    "dups_400k_w16": "dict winners that shift the set, sources in finished blocks (nrep)",
    "xml_400k_w19": "many short segments: istar < nb, blocks shorter than 64",
}
# the counters the stages' timing has a say in (tests/test_gpu_stage_views.py): within 0.1 % of the parent's, 25 times what the parent's
# own two runs differ by there
TIMED_REL = 1e-3


def digest(stream: bytes):
    return hashlib.sha256(stream).hexdigest(), len(stream)


def op_counters(ost: dict) -> dict:
    return {k: ost["cmp_bytes_needed" if k == "cmp_bytes" else k] for k in OPS}


@functools.lru_cache(maxsize=None)
def text():
    return corpus.syn_text(N)


@functools.lru_cache(maxsize=None)
def want_text():
    stream, ost = oracle_py.compress(text(), HIST_BITS, want_stats=True)
    return digest(stream), op_counters(ost)


def check(gpu, got: bytes, want):
    assert digest(got) == want[0]
    st = gpu.stats()
    assert {k: st[k] for k in OPS} == want[1]


@pytest.mark.parametrize("name", sorted(ARMS))
def test_arms_of_the_update(gpu, name):
    case = next(c for c in cases.CASES if c[0] == name)
    data = cases.make_case(case)
    stream, ost = oracle_py.compress(data, case[4], want_stats=True)
    check(gpu, gpu.compress(data, case[4]), (digest(stream), op_counters(ost)))


def test_two_launches(gpu):
    """three chunks in two launches: the pass loop across what one launch leaves for the next"""
    gpu.set_option("batch_chunks", 2)
    try:
        got = gpu.compress(text(), HIST_BITS)
    finally:
        gpu.set_option("batch_chunks", 32)
    check(gpu, got, want_text())


@pytest.mark.parametrize("helper", [0, 1])
def test_helper_off_and_on(gpu, helper):
    """the helper parsers run their own inlined copy of the update; segments of this input run into the forced cut"""
    gpu.set_option("parser_helper", helper)
    try:
        got = gpu.compress(text(), HIST_BITS)
    finally:
        gpu.set_option("parser_helper", 1)
    check(gpu, got, want_text())


def test_passes_and_blocks_are_the_parents(gpu, capfd):
    """parser_passes and parser_blocks of the 300,000 bytes (batch_chunks 2, stage report on) against the parent's library on the same machine"""
    with open(PARENT) as f:
        parent = json.load(f)["counters"]
    gpu.set_option("batch_chunks", 2); gpu.set_option("stage_report", 1)
    try:
        got = gpu.compress(text(), HIST_BITS)
    finally:
        gpu.set_option("stage_report", 0); gpu.set_option("batch_chunks", 32)
    capfd.readouterr()
    check(gpu, got, want_text())
    mine = {k: gpu.counter(k) for k in ("parser_passes", "parser_blocks")}
    print(mine)
    for k, v in mine.items():
        assert abs(v - parent[k]) <= TIMED_REL * parent[k], k
