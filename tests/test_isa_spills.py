"""The persistent kernels' scalar-register spill moves stay within a budget, region by region: tests/isa_spills.py
counts them in the compiler's assembly (the lane moves `v_writelane_b32 vX, sN, imm` / `v_readlane_b32 sN, vX, imm` on the spill VGPRs, and
nothing else), tests/golden/isa_spill_budget.json holds what the code reached when the budget was written, plus 10 %.  A change that brings
the spills back -- a role that takes the launch's arguments as values of the kernel again, wave-uniform counters alive across a stage's
loop -- fails here, without a GPU.  Also held: two waves per SIMD, the LDS image's size, no scratch."""
import json
import os
import shutil

import pytest

from tests import isa_spills

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
BUDGET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isa_spill_budget.json")


@pytest.fixture(scope="module")
def measured():
    result = isa_spills.measure()
    print(isa_spills.report(result))
    return result


@pytest.fixture(scope="module")
def budget():
    with open(BUDGET) as f:
        return json.load(f)


@pytest.mark.parametrize("kernel", isa_spills.KERNELS)
def test_spill_moves_within_budget(measured, budget, kernel):
    over = []
    for region in isa_spills.REGIONS:
        row, cap = measured[kernel]["regions"][region], budget[kernel]["regions"][region]
        for what in ("spill_stores", "spill_reloads"):
            if row[what] > cap[what]:
                over.append(f"{region}: {what} {row[what]} > {cap[what]}")
    assert not over, over


@pytest.mark.parametrize("kernel", isa_spills.KERNELS)
def test_occupancy_lds_scratch(measured, budget, kernel):
    res = measured[kernel]["resources"]
    assert res["Occupancy [waves/SIMD]"] == 2
    assert res["LDS Size [bytes/block]"] == budget[kernel]["lds_bytes"]
    assert res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0
