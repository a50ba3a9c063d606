"""The parser's pass update stays as short as it was made: tests/isa_pass.py counts, in the compiler's assembly, the
instructions, LDS waits and exec-mask instructions of every inlined copy of the update and the dependent LDS round trips among them;
tests/golden/isa_pass_budget.json holds the parent commit's figures and what this code reached.  A change that puts a load back behind a
condition, or a ladder of branches back around the winners' sets, fails here without a GPU.  Also held: the compiler's resource line
(no scratch, no VGPR spill, two waves per SIMD)."""
import json
import os
import shutil

import pytest

from tests import isa_pass

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
BUDGET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isa_pass_budget.json")


@pytest.fixture(scope="module")
def measured():
    result = isa_pass.measure()
    print(isa_pass.report(result))
    return result


@pytest.fixture(scope="module")
def budget():
    with open(BUDGET) as f:
        return json.load(f)


@pytest.mark.parametrize("kernel", isa_pass.KERNELS)
def test_update_within_its_figures(measured, budget, kernel):
    copies, caps = measured[kernel]["copies"], budget["this"][kernel]
    assert len(copies) == len(caps)
    over = [f"copy {n}: {what} {got[what]} > {cap[what]}" for n, (got, cap) in enumerate(zip(copies, caps)) for what in isa_pass.FIGURES
            if got[what] > cap[what]]
    assert not over, over


@pytest.mark.parametrize("kernel", isa_pass.KERNELS)
def test_recorded_figures_are_below_the_parents(budget, kernel):
    """(of the budget file itself: what it records for this code is strictly shorter than the parent's update, in instructions and in round trips)"""
    mine, parent = budget["this"][kernel], budget["parent"][kernel]
    assert len(mine) == len(parent)
    for got, was in zip(mine, parent):
        assert got["instructions"] < was["instructions"]
        assert got["lds_round_trips"] < was["lds_round_trips"]


@pytest.mark.parametrize("kernel", isa_pass.KERNELS)
def test_no_scratch_no_spill_two_waves(measured, kernel):
    res = measured[kernel]["resources"]
    assert res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0
    assert res["Occupancy [waves/SIMD]"] == 2
