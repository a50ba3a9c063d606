"""CPU suite: the host tables of the range entry points for lengths nobody can allocate -- crc::SegTable (nlzm_read_plan.h), planes::check_ranges,
planes::Table and planes::Layout (nlzm_planes_plan.h), container::make_ranges_plan (nlzm_container_plan.h), dedup::check_ranges (nlzm_dedup_plan.h)
and units::prefix (nlzm_units.h).  The harness (tests/host_sim/far_plan_sim.cpp) is a program of its own under AddressSanitizer and UBSan and includes the
headers the library includes; every number it prints is held to Python's integers: ranges of 2^32 - 1, 2^32, 2^32 + 1 and 2^40 bytes in a buffer
of 2^41, seg0, nsegs, the byte totals, and every refusal."""
import os

import pytest

from tests import simkit
from tests.simkit import SIMDIR

CRC_SEG, PLANES_SEG, DEDUP_SEG = 32768, 8192, 32768
BUF = 1 << 41
G4 = 1 << 32


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("far_plan_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("far_plan_sim_san")
    assert {"nlzm_amd/csrc/" + h for h in ("nlzm_read_plan.h", "nlzm_planes_plan.h", "nlzm_container_plan.h", "nlzm_dedup_plan.h", "nlzm_units.h")} <= simkit.compiled_from("far_plan_sim_san")
    return sim


def tables(sim, tmp_path, cases):
    """cases: (buf_len, [(off, len)]); returns per case {"crc": [...], "planes": [...], "ranges": [...], "dedup": [...]}: integers, or ("error", code, text)"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"T {n} {CRC_SEG} {PLANES_SEG} {DEDUP_SEG} {len(r)} " + " ".join(f"{o} {l}" for o, l in r) + "\n" for n, r in cases))
    r = simkit.sh([sim, path], 120)
    assert r.returncode == 0 and r.stdout.endswith("far_plan_sim: OK\n"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()[:-1]
    assert len(lines) == 4 * len(cases)
    out = []
    for i in range(len(cases)):
        d = {}
        for line in lines[4 * i: 4 * i + 4]:
            name, rest = line.split(" ", 1) if " " in line else (line, "")
            if rest.startswith("error"):
                parts = rest.split(" ", 2)
                d[name] = ("error", int(parts[1]), parts[2])
            else:
                d[name] = [int(v) for v in rest.split()]
        assert list(d) == ["crc", "planes", "ranges", "dedup"]
        out.append(d)
    return out


def ceil(a, b):
    return -(-a // b)


def prefix(lens, unit):
    t = [0]
    for l in lens:
        t.append(t[-1] + ceil(l, unit))
    return t


def bound(n):
    return 16 + 131072 + (n // 14848 + 1) * 16384


def want(buf_len, ranges):
    lens = [l for _, l in ranges]
    k = len(ranges)
    crc = prefix(lens, CRC_SEG)
    pl = prefix(lens, PLANES_SEG)
    nsets = 1 if k <= 64 else ceil(k, 32)
    base, more = divmod(k, nsets)
    sets, at = [], 0
    for s in range(nsets):
        count = base + (1 if s < more else 0)
        sets += [at, count, max(lens[at: at + count])]
        at += count
    return {"crc": [crc[-1], sum(lens)] + crc, "planes": [pl[-1], sum(lens), sum(lens), sum(lens) + 128] + pl,
            "ranges": [nsets, sum(bound(l) for l in lens)] + sets, "dedup": prefix(lens, DEDUP_SEG)}


LONG = [G4 - 1, G4, G4 + 1, 1 << 40]


def test_long_ranges_against_pythons_integers(sim, tmp_path):
    cases = []
    for ln in LONG:
        for off in (0, 1, G4 - 1, G4, BUF - ln):
            cases.append((BUF, [(off, ln)]))
    # all four in one call, among short and empty ranges, in both orders; ranges that overlap; 70 ranges (three sets) with a long one in each set
    mixed = [(5, 0), (0, G4 - 1), (G4 - 1, 1), (7, G4), (G4, CRC_SEG), (G4 + 1, G4 + 1), (1 << 40, 1 << 40), (BUF, 0), (BUF - 1, 1), (3, PLANES_SEG + 1)]
    cases += [(BUF, mixed), (BUF, mixed[::-1])]
    seventy = [((i * 977) << 20, (G4 + i if i % 23 == 0 else 1 << 40 if i == 40 else i * 1000 + 1)) for i in range(70)]
    cases.append((BUF, seventy))
    got = tables(sim, tmp_path, cases)
    for (n, ranges), g in zip(cases, got):
        assert g == want(n, ranges), (n, ranges[:12])
    # seg0 passes 2^32 where the lengths pass 2^47: the tables are 64-bit words
    n, ranges = 1 << 63, [(0, 1 << 45), (5, (1 << 45) - 3 * CRC_SEG + 1), (9, 12345)]
    g = tables(sim, tmp_path, [(n, ranges)])[0]
    assert g == want(n, ranges) and g["planes"][0] > G4 and g["crc"][0] == (1 << 31) - 1


def test_refusals(sim, tmp_path):
    over = [
        (BUF, [(0, 10), (BUF - G4, G4 + 1)], 1),             # one byte over the buffer's end, behind 2^32
        (BUF, [(BUF + 1, 0)], 0),                            # starts behind the end
        (BUF, [(0, G4), ((1 << 64) - 1, 2), (0, 1)], 1),     # off + len wraps
        (G4, [(G4 - 1, 1), (1, G4)], 1),                     # a buffer of exactly 2^32 bytes
        (G4 + 1, [(1, G4), (2, G4)], 1),
    ]
    for (n, ranges, bad), g in zip(over, tables(sim, tmp_path, [(n, r) for n, r, _ in over])):
        for name in ("crc", "planes", "dedup"):
            assert g[name][:2] == ("error", -1) and g[name][2].startswith(f"range {bad} ") and "runs over" in g[name][2], (name, g[name])
        assert g["ranges"][:2] == ("error", -1) and g["ranges"][2].startswith(f"{bad} range {bad} "), g["ranges"]
        o, l = ranges[bad]
        assert f"offset {o}, {l} bytes" in g["crc"][2] and f"the {n} bytes" in g["crc"][2]
    # more segments than a launch's table may hold: 2^31 of the CRC's, 2^40 of the planes' -- the other tables still stand
    n = 1 << 63
    ranges = [(0, 1 << 46), (1, 1 << 46), (2, 1)]
    g = tables(sim, tmp_path, [(n, ranges)])[0]
    w = want(n, ranges)
    assert g["crc"][:2] == ("error", -1) and "2^31 segments" in g["crc"][2]
    assert (g["planes"], g["ranges"], g["dedup"]) == (w["planes"], w["ranges"], w["dedup"])
    ranges = [(0, 1 << 53), (7, 1)]
    g = tables(sim, tmp_path, [(n, ranges)])[0]
    assert g["planes"][:2] == ("error", -1) and "2^40 segments" in g["planes"][2] and g["dedup"] == want(n, ranges)["dedup"]
    # lengths that do not sum in 64 bits: the scratch layout and the bound refuse, each in its words
    ranges = [(0, 1 << 63), (0, 1 << 63)]
    g = tables(sim, tmp_path, [((1 << 64) - 1, ranges)])[0]
    assert g["planes"][:2] == ("error", -1) and "do not sum in 64 bits" in g["planes"][2]
    three = tables(sim, tmp_path, [((1 << 64) - 1, ranges + [(0, 1 << 63)])])[0]
    assert three["ranges"][:2] == ("error", -1) and "do not sum in 64 bits" in three["ranges"][2]


def test_library_and_harness_read_the_same_headers():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    # the library's host file and the roles' harness use the shared table (nlzm_units.h, through the headers they include) and hold no copy of it
    host = open(os.path.join(csrc, "nlzm_hip_dedup.cpp")).read()
    assert '#include "nlzm_dedup_plan.h"' in host and "units::prefix(" in host and "std::vector<unsigned long long> prefix" not in host
    roles = open(os.path.join(SIMDIR, "dedup_sim.cpp")).read()
    assert "units::prefix(" in roles and "std::vector<unsigned long long> prefix" not in roles
    assert "nlzm_amd/csrc/nlzm_units.h" in simkit.compiled_from("dedup_sim_san")
    assert "prefix(uint32_t n, unsigned long long unit, Len len_of)" in open(os.path.join(csrc, "nlzm_units.h")).read()
    for name in ("nlzm_dedup.h", "nlzm_read_plan.h"):
        assert '#include "nlzm_units.h"' in open(os.path.join(csrc, name)).read(), name
    harness = open(os.path.join(SIMDIR, "far_plan_sim.cpp")).read()
    for name in ("crc::SegTable", "planes::Table", "planes::Layout", "planes::check_ranges(", "container::make_ranges_plan(", "units::prefix(", "dedup::check_ranges("):
        assert name in harness, name
    for src, name in (("nlzm_hip_crc.cpp", "crc::SegTable"), ("nlzm_hip_planes.cpp", "planes::Table"), ("nlzm_hip_blocks.cpp", "make_ranges_plan(")):
        assert name in open(os.path.join(csrc, src)).read(), (src, name)
