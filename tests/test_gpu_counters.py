"""GPU suite (-m gpu): the compress side's named counters (nlzm_hip_get_counter) and the stage report on real data.
A wrong slot costs no byte of output, so parity cannot see it: what holds here are relations that the writers in nlzm_v2.h /
nlzm_kernels.hip keep by construction (a wait is part of its stage's total, a slow block is a block, ...), and that the report's
first line is made of the counters of the same names."""
import re

import pytest

from nlzm_amd import corpus

pytestmark = pytest.mark.gpu

# every name of the compress side's table (nlzm_report.h: compress_counter)
NAMES = ["finder_blocks", "table_blocks", "parser_blocks", "parser_passes",
         "finder_wait_cycles", "finder_total_cycles", "table_wait_cycles", "table_total_cycles",
         "parser_wait_cycles", "parser_total_cycles", "parser_emit_cycles", "parser_setup_cycles", "parser_pass_cycles",
         "finder_bt_wait_cycles", "table_slow_blocks", "rk_cut_short_grown", "rk_cut_short_ties", "rk_cut_short_ties_won",
         "table_shape_changes", "table_wide_launches", "finder_seg_own", "finder_seg_waited",
         "helper_jobs", "helper_taken", "helper_taken_nodes", "helper_wait_cycles", "helper_jobs_done", "helper_blocks", "helper_passes",
         "worker_call_cycles", "worker_call_tests", "worker_calls", "hot_bin_calls", "positions"]
N, HIST_BITS, BATCH = 300_000, 16, 8     # chunks of 14,848 bytes: 21 chunks in three launches, so the counters add up across launches


def compress_and_read(gpu, report):
    data = corpus.syn_text(N)
    gpu.set_option("batch_chunks", BATCH)
    gpu.set_option("stage_report", report)
    try:
        gpu.compress(data, HIST_BITS)
    finally:
        gpu.set_option("stage_report", 0)       # (before any counter is read: a read of an open stream prints the report again)
        gpu.set_option("batch_chunks", 32)
    return {k: gpu.counter(k) for k in NAMES}   # (counter() raises unless the library answers 0)


def test_counters_answer_and_keep_their_order(gpu, capfd):
    c = compress_and_read(gpu, 0)
    assert capfd.readouterr().err == ""
    print(c)
    assert c["positions"] == N
    for stage in ("finder", "table", "parser"):
        assert c[stage + "_wait_cycles"] <= c[stage + "_total_cycles"], stage
        assert c[stage + "_total_cycles"] > 0, stage
    assert c["finder_bt_wait_cycles"] <= c["finder_wait_cycles"]
    assert c["table_slow_blocks"] <= c["table_blocks"]
    assert 1 <= c["parser_blocks"] <= c["parser_passes"]
    assert c["helper_taken"] <= c["helper_jobs"]
    assert c["hot_bin_calls"] <= c["worker_calls"]
    assert 0 < c["worker_calls"]


def test_report_line_is_made_of_the_named_counters(gpu, capfd):
    c = compress_and_read(gpu, 1)
    err = capfd.readouterr().err
    print(err)
    first = next(l for l in err.splitlines() if l.startswith("cycles/position"))
    m = re.search(r"finder: total (\d+) wait (\d+) .*\| table: total (\d+) wait (\d+) \|", first)
    assert m, first
    want = [round(c[k] / c["positions"]) for k in ("finder_total_cycles", "finder_wait_cycles", "table_total_cycles", "table_wait_cycles")]
    assert [int(x) for x in m.groups()] == want, first
