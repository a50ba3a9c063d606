"""CPU suite: what the range reader adds to the device code, compiled for the host with every GPU lane a fiber
(tests/host_sim/range_sim.cpp): the decoder role's prefix mode (nlzm_amd/csrc/nlzm_decode.h, dec::kPrefix) against the host decoder, and
the gather role (nlzm_amd/csrc/nlzm_range.h) against memcpy; and the plan the library's host side makes of a call
(nlzm_amd/csrc/nlzm_read_plan.h: the same text the library and the command line compile), carried out with memcpy.

Prefix mode: a decode with the flag ends successfully at `cap`; the harness gives the destination exactly cap bytes, misaligned by
cap % 16, between two canary regions, and holds out_len, every byte, and the role's ring / memory byte counters against what the host
decoder's parse says a decode cut at cap must serve from each side.  Most stops run in the 512-byte-ring build, where matches come from
memory and are cut there.  Gather: buffers lie between PROT_NONE pages, a read or write that leaves one ends the harness.

All runs (one process each, the caps of a stream dealt to several) are started together when the first test asks for one, the longest
first, and every test takes the results of its own runs: 33 s on eight cores from a clean tree (5 s of it the two builds of the harness;
240 s of CPU time in all), measured with nothing else running."""
import os
import re

import numpy as np
import pytest

from tests import cases, oracle_py, simkit
from tests.simkit import sh

WORKERS = max(1, min(8, os.cpu_count() or 2))
GATHER_SHARDS = 4


def case_of(name):
    return next(c for c in cases.CASES if c[0] == name)


def caps_of(name, raw):
    if name in ("tiny_1000", "under_2k"):
        return list(range(0, raw + 2))                                     # EVERY cap from 0 to the raw length + 1
    if name == "chunk_plus1":
        return sorted(set(range(0, raw + 2, 13)) | set(range(raw + 2 - 300, raw + 2)))      # every 13th, and the last 300
    if name == "runs_300k_w18":
        return [int(x) for x in np.linspace(1, 20_000, 300)]               # 300 caps spread over its first 20,000 bytes
    raise KeyError(name)


# (build, stream, processes its caps are dealt to), the longest first
PREFIX_RUNS = [("tiny", "chunk_plus1", 8), ("tiny", "under_2k", 3), ("norm", "under_2k", 3), ("tiny", "runs_300k_w18", 2), ("tiny", "tiny_1000", 1),
               ("norm", "tiny_1000", 1)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    SIM, SIM_TINY = simkit.build("range_sim", "range_sim_tiny", jobs=2)
    d = tmp_path_factory.mktemp("range_sim")
    raws = {}
    for n in sorted({n for _, n, _ in PREFIX_RUNS}):
        data = cases.make_case(case_of(n))
        raws[n] = int(data.size)
        (d / f"{n}.nlzm").write_bytes(oracle_py.compress(data, case_of(n)[4]))
    (d / "g.txt").write_text("G\n")
    G = int(sh([SIM, "gather", d / "g.txt"], 900).stdout.split()[0])
    jobs, caps = [], {}
    for build, n, parts in PREFIX_RUNS:
        caps[n] = caps_of(n, raws[n])
        for s in range(parts):
            f = d / f"caps_{build}_{n}_{s}.txt"
            f.write_text("".join(f"1 {c}\n" for c in caps[n][s::parts]))
            jobs.append((("prefix", build, n, s), [SIM_TINY if build == "tiny" else SIM, "prefix", d / f"{n}.nlzm", f]))
    f = d / "noflag.txt"
    f.write_text("".join(f"0 {c}\n" for c in (0, 1, 500, raws["tiny_1000"] - 1, raws["tiny_1000"], raws["tiny_1000"] + 1)))
    jobs.append((("noflag",), [SIM_TINY, "prefix", d / "tiny_1000.nlzm", f]))
    for s in range(GATHER_SHARDS):
        f = d / f"gather_{s}.txt"
        f.write_text(f"S 0 80 {s} {GATHER_SHARDS}\nS {G - 17} {G + 17} {s} {GATHER_SHARDS}\nS {2 * G - 17} {2 * G + 17} {s} {GATHER_SHARDS}\n")
        jobs.append((("gather", s), [SIM, "gather", f]))
    f = d / "mixed.txt"
    f.write_text("M 11 300\nM 12 300\nM 13 0\n")
    jobs.append((("mixed",), [SIM, "gather", f]))
    jobs.append((("plan",), [SIM, "plan"]))
    started = simkit.Runs(WORKERS)
    for key, cmd in jobs:
        started.submit(key, cmd, timeout=900)
    yield {"runs": started, "raws": raws, "caps": caps, "G": G}
    started.close()


def ok(runs, key):
    return runs["runs"].ok(key, "range_sim: OK").stdout      # (-11: an access left a buffer)


def prefix_rows(runs, build, name):
    """(cap, out_len, global_bytes, cut_global) of every run of the stream in that build; the harness has compared bytes, canaries and counters"""
    parts = next(p for b, n, p in PREFIX_RUNS if (b, n) == (build, name))
    rows, ring = [], None
    for s in range(parts):
        out = ok(runs, ("prefix", build, name, s))
        ring = int(re.search(r"ring=(\d+)", out).group(1))
        rows += [tuple(map(int, l.split())) for l in out.splitlines() if re.fullmatch(r"\d+ \d+ \d+ \d+", l)]
    return sorted(rows), ring


TINY = ["tiny_1000", "under_2k", "chunk_plus1", "runs_300k_w18"]


@pytest.mark.parametrize("name", TINY)
def test_prefix_stops_in_the_tiny_ring(runs, name):
    """the 512-byte ring: every asked cap ran and out_len = min(cap, raw); bytes, canaries and the two byte counters were held against the
    host decoder by the harness, run by run"""
    rows, ring = prefix_rows(runs, "tiny", name)
    raw = runs["raws"][name]
    assert ring == 512
    assert [r[0] for r in rows] == sorted(runs["caps"][name])
    assert all(out_len == min(cap, raw) for cap, out_len, _, _ in rows)
    if name in ("tiny_1000", "under_2k"):
        assert len(rows) == raw + 2
    print(name, "memory-served bytes over the truncated runs:", sum(r[2] for r in rows), "of them in the ops that were cut:", sum(r[3] for r in rows))


def test_truncated_runs_and_cut_ops_were_served_from_memory(runs):
    """The sums over the tiny-ring runs of the four inputs: match bytes served from memory in the truncated runs, and in the ops that were cut.
    Both must be non-zero, else the inputs have stopped covering the memory path and the cut inside it.  The two sums are taken over the
    four inputs together: under_2k and chunk_plus1 carry them (measured: 0.66 M and 3.2 M bytes, 108 k and 2.7 k of them in cut ops);
    tiny_1000 has no match farther back than 512 bytes, and the first 20,000 bytes of runs_300k_w18 hold only periodic matches with
    dv + lv <= 512, which the role serves from the ring in any build -- there the cut runs through the ring's periodic form."""
    rows = [r for name in TINY for r in prefix_rows(runs, "tiny", name)[0]]
    total, cut = sum(r[2] for r in rows), sum(r[3] for r in rows)
    print("memory-served bytes over all truncated runs:", total, "in cut ops:", cut)
    assert total > 0 and cut > 0, (total, cut)


@pytest.mark.parametrize("name", ["tiny_1000", "under_2k"])
def test_prefix_stops_in_the_normal_ring(runs, name):
    rows, ring = prefix_rows(runs, "norm", name)
    raw = runs["raws"][name]
    assert ring > 512 and len(rows) == raw + 2
    assert all(out_len == min(cap, raw) for cap, out_len, _, _ in rows)


def test_without_the_flag_a_small_cap_is_still_an_error(runs):
    """flags = 0: cap below the raw length is kErrCapacity with nothing written at or behind dst + cap; at and above it the stream decodes"""
    ok(runs, ("noflag",))


@pytest.mark.parametrize("shard", range(GATHER_SHARDS))
def test_gather_every_phase_and_length(runs, shard):
    """source misalignment 0 .. 15 x destination misalignment 0 .. 15 x lengths 0 .. 80 and round one and two chunk sizes (- 17 .. + 17), each
    with both sides behind the front guard page and with either and both flush against the guard page behind, against memcpy"""
    out = ok(runs, ("gather", shard))
    n_lengths = sum(len(range(lo + shard, hi + 1, GATHER_SHARDS)) for lo, hi in ((0, 80), (runs["G"] - 17, runs["G"] + 17), (2 * runs["G"] - 17, 2 * runs["G"] + 17)))
    assert int(re.search(r"cases=(\d+)", out).group(1)) == 4 * 256 * n_lengths


def test_gather_300_pieces_in_one_launch(runs):
    out = ok(runs, ("mixed",))
    rows = [tuple(map(int, re.findall(r"=(\d+)", l))) for l in out.splitlines() if l.startswith("pieces=")]
    assert [r[0] for r in rows] == [300, 300, 0]
    assert all(empty >= 20 and big >= 1 for k, empty, big, _ in rows[:2])


def test_plan_of_every_range_and_every_pair(runs):
    """The library's make_plan and pack_pieces on a container of six blocks of raw lengths 5, 0, 7, 3, 0, 4: every single range inside its 19
    bytes (210, the empty ones and off == 19 among them) and every ordered pair of them (44,100).  Per plan the harness holds need[b]
    (the furthest byte any range wants of b; 0 for untouched and empty blocks), direct (exactly one range uses the block and starts at or
    before its first byte), scratch (the sum of need over the needed non-direct blocks) and the piece list (none of a direct block) against
    the definitions written out block by block, then carries the plan out -- every needed block's first need[b] bytes copied to place[b],
    the packed pieces moved -- and compares the destination with the slices back to back, destination and scratch between canaries.
    Seven of the plans, (3, 10) + (0, 19) among them, have the real gather role move the packed pieces in the fiber simulator.  The
    errors: E_ARG for off = 2^64 - 1, len = 2, for off = 20, len = 0 and for raw lengths that wrap 64 bits; E_CAPACITY for dst_cap one
    below the sum (and none for dst_cap equal to it).  Half a second."""
    out = ok(runs, ("plan",))
    got = tuple(map(int, re.search(r"plans=(\d+) role_plans=(\d+) errors=(\d+)", out).groups()))
    assert got == (210 + 210 * 210, 7, 4), got
