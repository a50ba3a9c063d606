"""CPU suite: the decoder role at the ring of decode_small_kernel (nlzm_amd/csrc/nlzm_decode_small.hip, 16 KiB), compiled for the host with
every GPU lane a fiber (tests/host_sim/decode_small_sim.cpp; decode_small_sim in tests/host_sim/Makefile), against the host decoder and
against the 64 KiB build beside it there (decode_sim).

What a smaller ring changes is where a match's bytes come from: distances up to the ring are served from LDS, farther ones from memory, and
the unflushed part of the ring is a larger share of it.  So: streams whose matches reach 16 KiB + 1 .. 64 KiB back (the big ring's side there, the
small ring's memory side here), destinations misaligned by 0, 1, 7 and 15 bytes between PROT_NONE pages, prefix mode cut at 40 offsets, and the first
100 damaged streams of decode_sim's list held to the host decoder's rc AND its reason.  The per-stream byte counters at 16 KiB are
recorded in tests/golden/decode_small_ring.json, where tests/test_gpu_container.py finds what the kernel must report on the device.

All runs (one process each) start together when the first test asks for one; every test takes the result of its own."""
import json
import os
import re

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import cases, oracle_py, simkit

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "decode_small_ring.json")
WORKERS = max(1, min(8, os.cpu_count() or 2))
RING = 16384

NAMES = ["chunk_plus1", "dense_150k_w17", "text_200k_w15", "dups_400k_w16", "dups_600k_w20"]
REACH = ("reach_120k_w17", 120_000, 31, 17)            # syn_text whose matches reach between 16 KiB and 64 KiB back (name, size, seed offset, window bits)
STREAMS = NAMES + [REACH[0]]
MISALIGN = [0, 1, 7, 15]
CUTS, CUT_SHARDS = 40, 4
MUTANT_OF, MUTANT_SEED, MUTANT_FLIPS, MUTANT_COUNT = "tiny_1000", 7, 200, 100      # (tests/test_decode_sim.py: MUTANTS[0], seed 7)
WRAP_OF, WRAP_FLIPS, WRAP_COUNT, WRAP_SHARDS = "text_200k_w15", 200, 24, 4           # ... and damaged streams long enough to lap the 16 KiB ring


def stream_input(name):
    """(input bytes as an array, window bits) of a stream of this file: a case of tests/cases.py, or the reach stream"""
    if name == REACH[0]:
        return corpus.syn_text(REACH[1], corpus.SEED + REACH[2]), REACH[3]
    c = next(c for c in cases.CASES if c[0] == name)
    return cases.make_case(c), c[4]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    SMALL, BIG = simkit.build("decode_small_sim", "decode_sim", jobs=3)
    d = tmp_path_factory.mktemp("decode_small_sim")
    inputs, streams = {}, {}
    for n in STREAMS + [MUTANT_OF]:       # (WRAP_OF is one of STREAMS)
        data, bits = stream_input(n)
        inputs[n] = data.tobytes()
        streams[n] = oracle_py.compress(data, bits)
        (d / f"{n}.nlzm").write_bytes(streams[n])
    jobs = []                                              # (key, command), the longest first
    for n in sorted(STREAMS, key=lambda n: -len(streams[n])):
        jobs.append((("big", n), [BIG, "decode", d / f"{n}.nlzm", d / f"{n}.big.out"]))
        for m in MISALIGN:
            jobs.append((("small", n, m), [SMALL, "decode", d / f"{n}.nlzm", d / f"{n}.{m}.out", m]))
    for s in range(CUT_SHARDS):
        jobs.append((("prefix", s), [SMALL, "prefix", d / "dense_150k_w17.nlzm", CUTS, s, CUT_SHARDS]))
    jobs.append((("mutants",), [SMALL, "mutants", d / f"{MUTANT_OF}.nlzm", MUTANT_SEED, MUTANT_FLIPS, MUTANT_COUNT]))
    for s in range(WRAP_SHARDS):       # (another seed per process: four different lists of six)
        jobs.append((("wrap", s), [SMALL, "mutants", d / f"{WRAP_OF}.nlzm", MUTANT_SEED + 1 + s, WRAP_FLIPS, WRAP_COUNT // WRAP_SHARDS]))
    started = simkit.Runs(WORKERS)
    for key, cmd in jobs:
        started.submit(key, cmd, timeout=900)
    yield {"runs": started, "dir": d, "inputs": inputs, "streams": streams}
    started.close()


def ok(runs, key):
    return runs["runs"].ok(key, "decode_sim: OK").stdout


def field(out, name):
    line = next(l for l in out.splitlines() if l.startswith("rc="))
    return int(re.search(rf"\b{name}=(-?\d+)", line).group(1))


@pytest.mark.parametrize("misalign", MISALIGN)
@pytest.mark.parametrize("name", STREAMS)
def test_small_ring_decodes_to_the_input(runs, name, misalign):
    """bytes and counters are the host decoder's (the harness compares them, and both byte counters against the parse); here: the ring is
    the small kernel's, the output the stream's input, whatever the destination's alignment"""
    out = ok(runs, ("small", name, misalign))
    assert f"ring={RING} " in out and f"misalign={misalign}" in out
    assert field(out, "rc") == 0 and field(out, "out_len") == len(runs["inputs"][name])
    assert (runs["dir"] / f"{name}.{misalign}.out").read_bytes() == runs["inputs"][name]


@pytest.mark.parametrize("name", STREAMS)
def test_byte_counters_against_the_big_ring(runs, name):
    """Every match byte is served by one side or the other: the two builds agree on the sum, and what the small ring cannot reach goes to
    memory -- never the other way.  The counters do not depend on the destination's alignment, and they are the recorded ones."""
    big = ok(runs, ("big", name))
    assert "ring=65536 " in big
    small = [ok(runs, ("small", name, m)) for m in MISALIGN]
    pairs = {(field(o, "ring_bytes"), field(o, "global_bytes")) for o in small}
    assert len(pairs) == 1
    ring_b, glob_b = pairs.pop()
    assert ring_b + glob_b == field(big, "ring_bytes") + field(big, "global_bytes")
    assert glob_b >= field(big, "global_bytes")
    gold = json.load(open(GOLDEN))
    assert gold["ring"] == RING
    assert gold["streams"][name] == {"ring_bytes": ring_b, "global_bytes": glob_b, "out_len": len(runs["inputs"][name])}


def test_reach_stream_reaches_between_the_rings(runs):
    """at least 100 KB of syn_text at a window of 2^17 or more, with matches from 16 KiB + 1 to 64 KiB back: LDS in the big kernel, memory in the small one"""
    assert REACH[1] >= 100_000 and REACH[3] >= 17
    out = ok(runs, ("small", REACH[0], 0))
    mid = int(re.search(r"mid_bytes=(\d+)", out).group(1))
    assert mid >= 1000
    big = ok(runs, ("big", REACH[0]))
    assert field(out, "global_bytes") - field(big, "global_bytes") == mid


def test_prefix_mode_at_forty_cuts(runs):
    """dense_150k_w17 cut at 40 offsets from 1 to its end, the destination's last byte against a page that may not be written: exactly the prefix"""
    ran, cuts = 0, set()
    for s in range(CUT_SHARDS):
        out = ok(runs, ("prefix", s))
        ran += int(re.search(r"prefix: cuts=40 ran=(\d+)", out).group(1))
        cuts |= {int(c) for c in re.findall(r"^cut (\d+) ok$", out, re.M)}
    n = len(runs["inputs"]["dense_150k_w17"])
    assert ran == CUTS and len(cuts) == CUTS and min(cuts) == 1 and max(cuts) == n
    assert sum(1 for c in cuts if RING < c) > CUTS // 2        # (most cuts lie behind the ring's first lap)


def test_first_hundred_mutants_same_verdict_and_reason(runs):
    """the first 100 damaged streams of decode_sim's list (tests/test_decode_sim.py: tiny_1000, seed 7, 200 flips): accepted ones decode to the host
    decoder's bytes, rejected ones are rejected with its code"""
    out = ok(runs, ("mutants",))
    m = re.search(r"mutants=(\d+) ran=(\d+) accepted=(\d+) rejected=(\d+)", out)
    assert int(m.group(1)) == MUTANT_FLIPS + 16 and int(m.group(2)) == MUTANT_COUNT
    assert int(m.group(3)) + int(m.group(4)) == MUTANT_COUNT and int(m.group(4)) >= 10


def test_damaged_streams_that_lap_the_ring(runs):
    """tiny_1000 never fills a 16 KiB ring: 24 single-bit flips of text_200k_w15 (half of them anywhere in its 60 KB, so that most decodes run for laps of
    the ring before the damage shows, if it shows) -- the same verdict, reason and bytes as the host decoder's"""
    ran = 0
    for s in range(WRAP_SHARDS):
        m = re.search(r"mutants=(\d+) ran=(\d+) accepted=(\d+) rejected=(\d+)", ok(runs, ("wrap", s)))
        ran += int(m.group(2))
    assert ran == WRAP_COUNT
