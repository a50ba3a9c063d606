"""CPU suite: the simulation half of nlzm_amd/csrc/xw.h, primitive by primitive, against the model (tests/xw_model.py) -- the same probe role
(tests/xw_probe/xw_probe.h) and the same model that tests/test_gpu_xw.py holds the gfx950 half to, so that "the two builds agree" is
checked from both sides.  Also here: the checker's own test (a table with one word altered must fail, and name the word), and the
simulator's refusal to hand a live lane the value of a lane that has left the role.  2 s, nearly all of it the harness's build."""
import os

import numpy as np
import pytest

from tests import simkit
from tests import xw_model as xm

SIM = os.path.join(simkit.SIMDIR, "xw_probe_sim_san")


def run_sim(d, table, tag):
    table.input().tofile(d / f"in_{tag}.bin")
    return simkit.sh([SIM, d / f"in_{tag}.bin", d / f"out0_{tag}.bin", d / f"out1_{tag}.bin"], 300)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    simkit.build("xw_probe_sim_san")
    d = tmp_path_factory.mktemp("xw_probe")
    T = xm.Table(strict=True)
    r = run_sim(d, T, "strict")
    assert r.returncode == 0 and "xw_probe_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]        # (-11: an index left a table; 3: the simulator's own checks)
    return {"dir": d, "T": T, "out0": np.fromfile(d / "out0_strict.bin", dtype=np.uint32), "out1": np.fromfile(d / "out1_strict.bin", dtype=np.uint32)}


def test_every_primitive_against_the_model(sim):
    """the cross-lane primitives on all the vectors, the LDS and agent-scope operations, opaque and the clocks, and the waves with exited lanes:
    every asserted word of the first launch's table is the model's"""
    T = sim["T"]
    assert T.nc > 300 and {c["op"] for c in T.cases} == set(xm.OPS)
    msgs = xm.compare(sim["out0"], *T.expected())
    assert not msgs, "\n".join(msgs)


def test_second_launch_reads_what_the_first_wrote(sim):
    msgs = xm.compare(sim["out1"], *sim["T"].expected2())
    assert not msgs, "\n".join(msgs)


def test_what_the_hardware_orders_holds_as_a_property(sim):
    msgs = xm.check_properties(sim["T"], sim["out0"], sim["out1"])
    assert not msgs, "\n".join(msgs)


def test_exit_cases_cover_defined_and_undefined_slots(sim):
    """the waves with exited lanes assert something for every primitive, and every primitive that reads other lanes also has slots that are
    only recorded (else the cases have stopped covering the contract's new sentence)"""
    T = sim["T"]
    want, check, label = T.expected()
    for p, (pname, live) in enumerate(xm.EXIT_PATTERNS):
        seen, left = set(), set()
        for i, c in enumerate(T.exit_cases):
            vals, ok = T.exit_model[p][i]
            if (T.exit_flags[i] >> p) & 1:
                left.add(c["op"])
            if any(live[l] and ok[l] for l in range(64)):
                seen.add(c["op"])
        # (lane 0 is among every third lane: no prefix there is made of live lanes alone, and the scans are only recorded)
        assert seen == set(xm.OPS) - ({"scan_max", "scan_add", "scan_min_i32"} if not live[0] else set()), (pname, set(xm.OPS) - seen)
        assert {"readlane", "shfl"} <= left, (pname, left)
    assert {"scan_max", "scan_add", "scan_min_i32", "lane_below", "shfl_up"} <= {c["op"] for i, c in enumerate(T.exit_cases) if T.exit_flags[i] & 2}
    # exited lanes wrote nothing
    dead = [T.o_exit + (p * T.ne + i) * 128 + 2 * l + h for p, (_, live) in enumerate(xm.EXIT_PATTERNS) for i in range(T.ne) for l in range(64) if not live[l] for h in (0, 1)]
    assert (sim["out0"][dead] == xm.SENTINEL).all() and check[dead].all()


def test_the_checker_names_every_altered_word():
    """the model's own table with ONE word changed in each primitive's section (and in each other section): the comparison fails, once, and names
    that section, case and lane"""
    T = xm.Table(strict=False)
    want, check, label = T.expected()
    assert not xm.compare(want.copy(), want, check, label)
    sections = {}
    for i in np.flatnonzero(check):
        sections.setdefault(label[i][0], []).append(int(i))
    assert set(xm.OPS) <= set(sections) and {"lds_add", "lds_or", "lds_max", "lds_add64", "lds_min64", "lds_st/lds_ld", "st_agent128/ld_agent128",
                                             "st_agent/ld_agent", "st_agent64/ld_agent64", "cas_agent", "opaque", "tick", "clock100", "lane()", "wave()",
                                             "thread()"} <= set(sections)
    rng = np.random.default_rng(5)
    for name, idx in sections.items():
        for i in (idx[0], idx[-1], idx[int(rng.integers(0, len(idx)))]):
            got = want.copy()
            got[i] ^= np.uint32(1 << int(rng.integers(0, 32)))
            msgs = xm.compare(got, want, check, label)
            assert len(msgs) == 1, (name, i, msgs)
            assert msgs[0].startswith(f"{name}: case {label[i][1]}, {label[i][2]}: got 0x{int(got[i]):08X}, want 0x{int(want[i]):08X}"), msgs
    want2, check2, label2 = T.expected2()
    got = want2.copy()
    got[32 * 200 + 13] ^= np.uint32(0x80000000)
    msgs = xm.compare(got, want2, check2, label2)
    assert len(msgs) == 1 and "ld_agent128 of the second slot, word 1" in msgs[0] and "thread 200" in msgs[0], msgs
    # the properties' checks fail too
    out0, out1 = want.copy(), want2.copy()
    out0[T.o_lds + xm.L_INC:T.o_lds + xm.L_INC + 256] = np.arange(256)
    out0[T.o_agent + 13:T.o_agent + 13 + 16 * 256:16] = 8
    out0[T.o_agent + 16 * 7 + 13] = 0
    out1[26::32] = 8
    assert not xm.check_properties(T, out0, out1)
    out0[T.o_lds + xm.L_INC + 9] = 8
    assert any("lds_inc" in m for m in xm.check_properties(T, out0, out1))
    out0[T.o_agent + 16 * 9 + 13] = 0
    assert any("2 threads were returned 0" in m for m in xm.check_properties(T, out0, out1))


def test_the_simulator_refuses_reads_of_exited_lanes(sim):
    """the same table without `strict`: the waves with exited lanes run the cases in which a live lane's source has left the role, and the
    simulator ends the run with its own message instead of handing out the exited fiber's last argument"""
    r = run_sim(sim["dir"], xm.Table(strict=False), "loose")
    assert r.returncode == 3 and "a live lane reads an exited lane" in r.stderr, r.stdout[-500:] + r.stderr[-1500:]
