"""CPU suite: the host plan of the byte-plane filter (nlzm_amd/csrc/nlzm_planes_plan.h), which the nlzm_hip_planes* and the typed entry points run
before any launch: the argument checks, the destination-overlap check, the launch's table, the runs a host-buffer call copies back and the typed
calls' scratch layout.  The plan is plain C++ with no device in it; the harness (tests/host_sim/planes_plan_sim.cpp) is a program of its own under
AddressSanitizer and UBSan and includes the header the library includes.

The sweep (in the harness): random range lists against brute force over a bitmap of the destination; the table, the runs and the layout against
their definitions; k = 1 and k = 65,536; offsets and sums that wrap 64 bits.  Here: lists written by this file, and what the errors say."""
import os
import re

import pytest

from tests import simkit

E_ARG = -1


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("planes_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("planes_plan_sim_san")
    assert "nlzm_amd/csrc/nlzm_planes_plan.h" in simkit.compiled_from("planes_plan_sim_san")
    return sim


def run(sim, *args):
    r = simkit.sh([sim, *args], 600)
    assert r.returncode == 0 and "planes_plan_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def check(sim, tmp_path, ranges, src_len=10000, dst_len=10000, src_at=1 << 20, dst_at=1 << 21, segment=8192):
    (tmp_path / "ranges.txt").write_text("".join(f"{a} {b} {c} {e}\n" for a, b, c, e in ranges))
    return run(sim, "check", src_at, src_len, dst_at, dst_len, segment, tmp_path / "ranges.txt")


def test_sweep(sim):
    assert re.search(r"sweep: cases=\d+ refused=\d+", run(sim, "sweep"))


def test_library_and_harnesses_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    host = open(os.path.join(csrc, "nlzm_hip_planes.cpp")).read()
    assert '#include "nlzm_planes_plan.h"' in host
    for name in ("planes::check_ranges(", "planes::check_elems(", "planes::check_typed_ranges(", "planes::Table", "planes::Layout", "planes::runs("):
        assert name in host, name
    assert "runs over" not in host                  # (the typed calls' range check is the plan's, not a copy in the host file)
    harness = open(os.path.join(simkit.SIMDIR, "planes_plan_sim.cpp")).read()
    for name in ("planes::check_ranges(", "planes::check_typed_ranges(", "planes::Table", "planes::Layout", "planes::runs("):
        assert name in harness, name
    plan = open(os.path.join(csrc, "nlzm_planes_plan.h")).read()
    assert "hip_runtime" not in plan and "__device__" not in plan          # (no device in it)


def test_the_table(sim, tmp_path):
    out = check(sim, tmp_path, [(0, 0, 8192, 2), (5, 9000, 0, 4), (100, 8192, 8193, 8), (0, 20000, 1, 1)], src_len=30000, dst_len=30000)
    assert out.splitlines()[0] == "ok nsegs 4 bytes 16386 runs 2"      # (the first and the third destination lie back to back)
    assert out.splitlines()[1] == "0 1 1 3 4"
    out = check(sim, tmp_path, [(0, 0, 100, 2), (0, 100, 100, 4), (0, 200, 100, 8)], segment=16)
    assert out.splitlines()[0] == "ok nsegs 21 bytes 300 runs 1" and out.splitlines()[1] == "0 7 14 21"


def test_every_error_names_its_range(sim, tmp_path):
    M = 1 << 64
    cases = [
        ([(0, 0, 10, 2), (9991, 100, 10, 2)], "range 1 ", "runs over the 10000 bytes of the source"),
        ([(0, 9991, 10, 2)], "range 0 ", "runs over the 10000 bytes of the destination"),
        ([(M - 1, 0, 2, 2)], "range 0 ", "source"),
        ([(0, 0, 10, 2), (0, 20, M - 1, 1)], "range 1 ", "runs over"),
        ([(0, 0, 10, 2), (0, 20, 10, 3)], "range 1", "element size 3"),
        ([(0, 0, 10, 0)], "range 0", "element size 0"),
        ([(0, 0, 10, 16)], "range 0", "element size 16"),
        ([(0, 100, 10, 2), (50, 0, 10, 4), (0, 109, 5, 1)], "range 0 ", "overlaps range 2 "),
        ([(0, 0, 100, 2), (0, 10, 5, 2), (0, 200, 5, 2)], "range 0 ", "overlaps range 1 "),
        ([(0, 50, 10, 2), (0, 50, 10, 2)], "range 0 ", "overlaps range 1 "),
    ]
    for ranges, name, text in cases:
        out = check(sim, tmp_path, ranges)
        assert out.startswith(f"error {E_ARG} ") and name in out and text in out, (ranges, out)
    # empty ranges overlap nothing, wherever they point; ranges that touch do not overlap
    assert check(sim, tmp_path, [(0, 5, 10, 2), (0, 7, 0, 2), (0, 15, 10, 4), (3, 10000, 0, 8)]).startswith("ok ")


def test_the_buffers_may_not_overlap(sim, tmp_path):
    ok = [(0, 0, 10, 2)]
    for src_at, dst_at in ((1000, 1000), (1000, 1999), (1999, 1000), (1000, 1500)):
        out = check(sim, tmp_path, ok, src_len=1000, dst_len=1000, src_at=src_at, dst_at=dst_at)
        assert out.startswith(f"error {E_ARG} ") and "no in-place form" in out, (src_at, dst_at, out)
    for src_at, dst_at in ((1000, 2000), (2000, 1000), (0, (1 << 64) - 1000)):
        assert check(sim, tmp_path, ok, src_len=1000, dst_len=1000, src_at=src_at, dst_at=dst_at).startswith("ok "), (src_at, dst_at)
