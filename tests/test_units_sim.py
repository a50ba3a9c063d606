"""CPU suite: the unit table of the range kernels (nlzm_amd/csrc/nlzm_units.h) -- units::count, units::prefix, units::owner_of and units::blocks_for,
the one implementation the gather role, the CRC's segments, the equal-range finder, the byte planes, their host tables and their launches share.  The
harness (tests/host_sim/units_sim.cpp) is a program of its own under AddressSanitizer and UBSan and includes the header the library includes; every
number it prints is held to Python's own integers and to bisect."""
import os
from bisect import bisect_right

import pytest

from tests import simkit

CSRC = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
G4 = 1 << 32
UNITS = (32768, 65536, 1)


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("units_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("units_sim_san")
    assert "nlzm_amd/csrc/nlzm_units.h" in simkit.compiled_from("units_sim_san")
    return sim


def run(sim, tmp_path, lines):
    """one output line per case line: lists of integers"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line in lines))
    r = simkit.sh([sim, path], 60)
    assert r.returncode == 0 and r.stdout.endswith("units_sim: OK\n"), r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()[:-1]
    assert len(out) == len(lines)
    return [[int(v) for v in line.split()] for line in out]


def ceil(a, b):
    return -(-a // b)


def prefix(lens, unit):
    t = [0]
    for l in lens:
        t.append(t[-1] + ceil(l, unit))
    return t


def lengths(unit):
    return [0, 1, unit - 1, unit, unit + 1, G4 - 1, G4, G4 + 1, (1 << 64) - 1]


def test_count_against_pythons_integers(sim, tmp_path):
    cases = [(l, u) for u in UNITS for l in lengths(u)]
    got = run(sim, tmp_path, [f"C {l} {u}" for l, u in cases])
    for (l, u), g in zip(cases, got):
        assert g == [ceil(l, u)], (l, u)
    assert run(sim, tmp_path, [f"C {(1 << 64) - 1} 2"]) == [[1 << 63]]          # (len + unit - 1 wraps to 0 here)


def test_prefix_against_pythons_integers(sim, tmp_path):
    cases = []
    for u in UNITS:
        cases.append((u, lengths(u)[:-1]))                   # every length but the last, whose units alone fill 64 bits at unit 1
        cases.append((u, lengths(u)[:-1][::-1]))
        cases.append((u, [(1 << 64) - 1]))                   # ... which stands alone
        cases.append((u, [0]))
        cases.append((u, [0, 0, 5, 0, u, 0, 0, 1, 0]))
    # tables whose totals pass 2^32: by many units of one entry, and by the sum of entries that each stay below
    cases.append((1, [G4 - 1, 1, 1, 0, 7]))
    cases.append((32768, [1 << 47, 0, 3 * (1 << 45) + 1, 0, 7]))
    cases.append((65536, [(1 << 47) - 1] * 5))
    got = run(sim, tmp_path, [f"P {u} {len(lens)} " + " ".join(str(l) for l in lens) for u, lens in cases])
    for (u, lens), g in zip(cases, got):
        assert g == prefix(lens, u), (u, lens)
        assert all(v < 1 << 64 for v in g)
    assert got[-3][-1] > G4 and got[-2][1] == G4 and got[-1][-1] > G4


def owner_cases():
    """(table, n): the units asked are the first and the last of every entry that owns any"""
    tables = [prefix([5], 1), prefix([1], 32768), prefix([(1 << 64) - 1], 1)]       # n = 1
    for u in (1, 2, 32768):
        tables.append(prefix([0, 0, 5, 0, u, 0, 0, 1, 0], u))                       # empty entries at the front, in the middle, at the back, in runs
    tables.append(prefix([3, 0, 0, 0, 0, 0, 0, 9], 2))
    tables.append(prefix([7] * 33, 3))                                               # no empty entry; n no power of two
    tables.append(prefix([1 << 47, 0, 3 * (1 << 45) + 1, 0, 7, 0], 32768))           # entries beyond unit 2^32
    tables.append(prefix([G4 - 1, 1, 0, 1, G4 + 5, 0, 0, 2], 1))
    return tables


def test_owner_of_against_bisect(sim, tmp_path):
    tables = owner_cases()
    asked = []
    for t in tables:
        n = len(t) - 1
        us = []
        for i in range(n):
            if t[i + 1] > t[i]:
                us += [t[i], t[i + 1] - 1]
        assert us
        asked.append(us)
    got = run(sim, tmp_path, [f"O {len(t) - 1} " + " ".join(map(str, t)) + f" {len(us)} " + " ".join(map(str, us)) for t, us in zip(tables, asked)])
    for t, us, g in zip(tables, asked, got):
        n = len(t) - 1
        want = [bisect_right(t[:n], u) - 1 for u in us]
        assert g == want, (t, us)
        for u, r in zip(us, g):
            assert t[r] <= u < t[r + 1]                      # (the owner is an entry that owns the unit, never an empty one)
    assert any(u >= G4 for us in asked for u in us)


def test_blocks_for(sim, tmp_path):
    cases = []
    for M in (1 << 20, 1 << 22, 7):
        cases += [(1, 4, M), (4, 4, M), (5, 4, M), (4 * M, 4, M), (4 * M + 1, 4, M)]
        cases += [(n, 1, M) for n in (1, M, M + 1)]
    cases.append((1 << 40, 4, 1 << 20))
    got = run(sim, tmp_path, [f"B {n} {per} {M}" for n, per, M in cases])
    for (n, per, M), g in zip(cases, got):
        assert g == [min(ceil(n, per), M)], (n, per, M)
        assert 1 <= g[0] <= M and g[0] * per >= min(n, M * per)      # (a wave for every unit, until the cap)


def test_one_definition():
    """the role headers hold no owner search and no pointer cast of their own, and the program that runs each role on the CPU was compiled
    from the shared table"""
    for name, program in (("nlzm_range.h", "range_sim"), ("nlzm_crc.h", "crc_sim_san"), ("nlzm_planes.h", "planes_sim_san"), ("nlzm_dedup.h", "dedup_sim_san")):
        text = open(os.path.join(CSRC, name)).read()
        assert "while (hi - lo > 1)" not in text and "units::owner_of(" in text and '#include "nlzm_units.h"' in text, name
        assert {"nlzm_amd/csrc/nlzm_units.h", "nlzm_amd/csrc/" + name} <= simkit.compiled_from(program), program
    assert open(os.path.join(CSRC, "nlzm_units.h")).read().count("while (hi - lo > 1)") == 1
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp")) and name not in ("nlzm_units.h", "nlzm_kernels.hip", "xw.h"):
            assert "address_space(1)" not in open(os.path.join(CSRC, name)).read(), name
