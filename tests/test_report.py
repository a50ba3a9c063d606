"""CPU suite: the compress pipeline's reports (nlzm_amd/csrc/nlzm_report.h: stage_report, worker_report, the eight figures of a block
set's table, the counter names, the stage part of a launch's error text) on synthetic structs in which every slot holds a value of its
own (tests/host_sim/report_sim.cpp, a UBSan + AddressSanitizer build), byte for byte against tests/golden/report_*.txt.

The golden files are what the report code printed BEFORE the slots had names: that commit's stage_report, worker_report, kProf table,
acct lines and error format, pasted into a scratch harness and run on the same structs.  A swapped pair of slot names, a run's width off
by one or a hot_class column off by one changes a line here, and the test names it."""
import os

import pytest

from tests import simkit

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sim():
    return simkit.build("report_sim_san")[0]


@pytest.mark.parametrize("what", ["all", "fine", "gates", "cold", "acct", "counters", "error"])
def test_report_text_is_unchanged(sim, what):
    """all: every slot set, hot bins on; fine: the same with small divisors, so that no two slots round to the same figure; gates: every conditional section's gate zero (then hot_steps too); cold: hot bins off;
    acct / counters / error: the block set's rows, every counter name (and an unknown one), the error text's stage part"""
    r = simkit.sh([sim, what], 60)
    assert r.returncode == 0, r.stdout + r.stderr
    want = open(os.path.join(HERE, "golden", f"report_{what}.txt")).read()
    got_lines, want_lines = r.stdout.splitlines(), want.splitlines()
    for i, (g, w) in enumerate(zip(got_lines, want_lines)):
        assert g == w, f"report_{what}.txt line {i + 1}"
    assert len(got_lines) == len(want_lines)
    assert r.stdout == want
