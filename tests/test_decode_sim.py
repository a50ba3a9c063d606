"""CPU suite: the device decoder's role (nlzm_amd/csrc/nlzm_decode.h), compiled for the host with every GPU lane a fiber
(tests/host_sim/decode_sim.cpp), decodes the reference's streams to their inputs and agrees with the host decoder
(nlzm_amd/csrc/nlzm_host_decode.h, the specification) on damaged ones.

The simulator decodes ~60,000 rANS symbols per second on one core (a symbol is five cross-lane operations of 64 fibers), so a
literal-heavy case costs the most: random_100k_w15 5 s, dups_600k_w20 12 s, dups_400k_w16 9 s, xml_400k_w19 / runs_300k_w18 /
text_200k_w15 3 - 5 s, the rest under a second; size-only mode costs the same again; a ring-edge input 4 - 8 s; a mutant of
random_100k_w15 up to 5 s (most are rejected early).  All runs (one process each) are started together when the first test asks
for one, the longest first, and every test takes the result of its own run: 130 s on eight cores with the harnesses built (the three
builds, made beside each other, add 12 s; 820 s of CPU time in all -- every damaged stream is decoded twice), measured with nothing else running.

Mutants run in a UBSan build; AddressSanitizer does not follow the fibers' hand-switched stacks (it reports the first switch), so
instead every buffer the role sees lies in a mapping of its own between two PROT_NONE pages, and what the pages enclose beside it is a
canary that is checked after every launch.  Well-formed streams are decoded at addresses that are misaligned on purpose, canaries on
both sides; every damaged stream is decoded twice, source and destination flush against the page behind them and starting right behind
the page in front, so that a read outside [src, src + len) or a write outside [dst, dst + cap) ends the harness with SIGSEGV.  The
split of a container (dec::split_walk, the body of the device's split kernel) runs in the same harness, against the host's."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from nlzm_amd import corpus, shard
from tests import cases, oracle_py, simkit
from tests.simkit import sh

HERE = os.path.dirname(os.path.abspath(__file__))
WORKERS = max(1, min(8, os.cpu_count() or 2))

NAMES = ["empty", "one_byte", "tiny_1000", "under_2k", "chunk_plus1", "overlap_265", "text_200k_w15", "runs_300k_w18", "random_100k_w15",
         "dups_400k_w16", "dups_600k_w20", "cutnice_60k_w17", "dense_150k_w17", "xml_400k_w19"]
GOLD = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "streams.json")))["cases"]}
HEX = [n for n in NAMES if "stream_hex" in GOLD[n]]
PREFIXES = ["0", "37", "1000", "half", "minus150"]        # bytes in front of the ring-edge construction (half: R / 2, minus150: R - 150)
EDGES = [-1, 0, 1]                                         # D - R
# (stream, single-bit flips, processes the list is dealt to)
MUTANTS = [("tiny_1000", 200, 1), ("chunk_plus1", 200, 4), ("random_100k_w15", 100, 10)]
BLOCKS_K = 5
SPLIT = ["empty", "one_byte", "tiny_1000", "under_2k", "chunk_plus1"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def case_of(name):
    return next(c for c in cases.CASES if c[0] == name)


def edge_input(ring, d_off, prefix):
    """prefix + a random block B of 300 bytes + D - 300 random bytes + B again: the second B is a match at distance exactly D"""
    npre = {"0": 0, "37": 37, "1000": 1000, "half": ring // 2, "minus150": ring - 150}[prefix]
    D = ring + d_off
    rng = np.random.default_rng(corpus.SEED + 1000 * (d_off + 2) + npre)
    B = rng.integers(0, 256, 300, dtype=np.uint8)
    return np.concatenate([rng.integers(0, 256, npre, dtype=np.uint8), B, rng.integers(0, 256, D - 300, dtype=np.uint8), B]), D


def blocks_input():
    data = corpus.mixed(700_000, corpus.SEED + 9)          # (the input of test_abi.py::test_cli_decodes_streams_back_to_back)
    return data, [shard.block_range(data.size, BLOCKS_K, i) for i in range(BLOCKS_K)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    SIM, SIM_TINY, SIM_SAN = simkit.build("decode_sim", "decode_sim_tiny", "decode_sim_san", jobs=3)     # (three builds of the harness, beside each other)
    d = tmp_path_factory.mktemp("decode_sim")
    streams, inputs = {}, {}
    for n in NAMES:
        inputs[n] = cases.make_case(case_of(n)).tobytes()
        streams[n] = oracle_py.compress(np.frombuffer(inputs[n], dtype=np.uint8), case_of(n)[4])
        (d / f"{n}.nlzm").write_bytes(streams[n])
    for n in HEX:
        (d / f"{n}.hex.nlzm").write_bytes(bytes.fromhex(GOLD[n]["stream_hex"]))
    ring = int(re.search(r"ring=(\d+)", sh([SIM, "decode", d / "empty.nlzm", d / "empty.probe"]).stdout).group(1))
    edge = {}
    for pre in PREFIXES:
        for off in EDGES:
            data, D = edge_input(ring, off, pre)
            (d / f"edge_{pre}_{off}.nlzm").write_bytes(oracle_py.compress(data, 20))
            edge[(pre, off)] = (data.tobytes(), D)
    bdata, branges = blocks_input()
    (d / "blocks.nlzm").write_bytes(b"".join(oracle_py.compress(bdata[lo:hi], 18) for lo, hi in branges))

    (d / "split.nlzm").write_bytes(b"".join(streams[n] for n in SPLIT))
    jobs = []                                              # (key, command), the longest first
    for n, flips, parts in MUTANTS:
        if n == "random_100k_w15":
            jobs += [(("mutants", n, s), [SIM_SAN, "mutants", d / f"{n}.nlzm", 7, flips, s, parts]) for s in range(parts)]
    for n in sorted(NAMES, key=lambda n: -len(streams[n])):
        jobs.append((("case", n), [SIM, "decode", d / f"{n}.nlzm", d / f"{n}.out"]))
        jobs.append((("size", n), [SIM, "decode", d / f"{n}.nlzm", d / f"{n}.none", "size"]))
    for given in (1, 0):
        jobs.append((("blocks", given), [SIM, "blocks", d / "blocks.nlzm", d / f"blocks{given}.out", given]))
    for n in ("dups_400k_w16", "runs_300k_w18"):
        jobs.append((("tiny", n), [SIM_TINY, "decode", d / f"{n}.nlzm", d / f"{n}.tiny.out"]))
    for key in edge:
        jobs.append((("edge",) + key, [SIM, "decode", d / f"edge_{key[0]}_{key[1]}.nlzm", d / f"edge_{key[0]}_{key[1]}.out"]))
    for n, flips, parts in MUTANTS:
        if n != "random_100k_w15":
            jobs += [(("mutants", n, s), [SIM_SAN, "mutants", d / f"{n}.nlzm", 7, flips, s, parts]) for s in range(parts)]
    for n in HEX:
        jobs.append((("hex", n), [SIM, "decode", d / f"{n}.hex.nlzm", d / f"{n}.hex.out"]))
    jobs.append((("split",), [SIM_SAN, "split", d / "split.nlzm"]))
    started = simkit.Runs(WORKERS)
    for key, cmd in jobs:
        started.submit(key, cmd)
    yield {"runs": started, "dir": d, "streams": streams, "inputs": inputs, "ring": ring, "edge": edge, "blocks": (bdata.tobytes(), branges)}
    started.close()


def ok(runs, key):
    return runs["runs"].ok(key, "decode_sim: OK").stdout


def field(out, name):
    line = next(l for l in out.splitlines() if l.startswith("rc="))
    return int(re.search(rf"\b{name}=(-?\d+)", line).group(1))


@pytest.mark.parametrize("name", NAMES)
def test_reference_stream_decodes_to_its_input(runs, name):
    """hist_bits 10 / 11 / 14, a frame boundary +- 1, literal-only data, runs (dv = 1: periodic copies), rebased windows and -- dups_600k_w20 --
    matches farther back than the ring.  The stream is the reference's (its SHA-256 is the fixture's), the output the fixture's input."""
    assert sha(runs["streams"][name]) == GOLD[name]["stream_sha256"]
    out = ok(runs, ("case", name))
    assert field(out, "rc") == 0 and field(out, "out_len") == GOLD[name]["size"]
    assert sha((runs["dir"] / f"{name}.out").read_bytes()) == GOLD[name]["input_sha256"]
    if name == "dups_600k_w20":
        assert field(out, "global_bytes") > 100_000 and field(out, "ring_bytes") > 100_000


@pytest.mark.parametrize("name", HEX)
def test_fixture_bytes_decode(runs, name):
    ok(runs, ("hex", name))
    assert sha((runs["dir"] / f"{name}.hex.out").read_bytes()) == GOLD[name]["input_sha256"]


@pytest.mark.parametrize("name", NAMES)
def test_size_only_mode(runs, name):
    """dst = NULL: the length, and nothing stored (the harness keeps a patterned buffer beside the role and finds it untouched; the role
    itself is handed no pointer in this mode, so there is nothing it could write through)."""
    out = ok(runs, ("size", name))
    assert field(out, "rc") == 0 and field(out, "out_len") == GOLD[name]["size"]


@pytest.mark.parametrize("prefix", PREFIXES)
def test_ring_edges(runs, prefix):
    """A match longer than 64 at distance exactly D = R - 1, R, R + 1 (R: the ring's size, which is also the farthest distance it serves),
    moved across the flush points by the prefix.  The parse must hold that match (else the case has stopped covering the edge); D <= R is
    served from the ring, R + 1 from memory, so that each prefix sees both sides (one input cannot: its far match lies on one side), and the harness
    checks the role's two byte counters against what the host decoder's parse says each side must have served."""
    R = runs["ring"]
    sides = set()
    for off in EDGES:
        data, D = runs["edge"][(prefix, off)]
        out = ok(runs, ("edge", prefix, off))
        longm = [tuple(map(int, l.split()[1:3])) for l in out.splitlines() if l.startswith("longmatch ")]
        hit = [lv for dv, lv in longm if dv == D]
        assert hit and max(hit) > 64, (D, longm[:10])
        assert (runs["dir"] / f"edge_{prefix}_{off}.out").read_bytes() == data
        ring_b, glob_b = field(out, "ring_bytes"), field(out, "global_bytes")
        if D <= R:
            assert ring_b >= sum(hit)
            sides.add("ring")
        else:
            assert glob_b >= sum(hit)
            sides.add("global")
    assert sides == {"ring", "global"}


@pytest.mark.parametrize("name", ["dups_400k_w16", "runs_300k_w18"])
def test_tiny_ring(runs, name):
    """The smallest ring the role allows (512 bytes: an op's 267 bytes and what is not flushed yet must fit): copies straddle flushes constantly,
    and in dups most match bytes come from memory (distances beyond 512)."""
    out = ok(runs, ("tiny", name))
    assert "ring=512" in out
    assert sha((runs["dir"] / f"{name}.tiny.out").read_bytes()) == GOLD[name]["input_sha256"]
    if name.startswith("dups"):      # (the harness has checked both counters against the parse; here: the case is mostly the memory path)
        assert field(out, "global_bytes") > field(out, "ring_bytes") > 0


@pytest.mark.parametrize("given", [1, 0])
def test_block_set_in_one_launch(runs, given):
    """Five streams back to back as five workgroups of one launch; without the lengths a size-only launch finds them first."""
    data, ranges = runs["blocks"]
    out = ok(runs, ("blocks", given))
    raw = list(map(int, re.search(r"raw_len_out=([\d,]+)", out).group(1).split(",")))
    assert raw == [hi - lo for lo, hi in ranges]
    assert (runs["dir"] / f"blocks{given}.out").read_bytes() == data


@pytest.mark.parametrize("name,flips,parts", MUTANTS)
def test_mutants_agree_with_host_decoder(runs, name, flips, parts):
    """Single-bit flips (half of them in the first frame's header and states), truncation at each of the last 16 bytes, header edits, dst_cap one
    byte short: the role and the host decoder agree on accepted / rejected and on every byte of what is accepted, every run ends, and no
    canary byte in front of or behind the stream and the output changes."""
    total = ran = 0
    for s in range(parts):
        out = ok(runs, ("mutants", name, s))
        m = re.search(r"mutants=(\d+) ran=(\d+)", out)
        total, ran = int(m.group(1)), ran + int(m.group(2))
    assert total == ran == flips + 16 + 4 + 5 + 1


def test_split_walk_agrees_with_the_host_split(runs):
    """dec::split_walk, which the device's split kernel runs in one lane, against nlzm_host::split_streams: a container of five small streams cut
    at EVERY length from 0 to its end, each cut with its last byte flush against a PROT_NONE page, walked for 1 .. 7 blocks -- the lengths
    found and bad = found + 1 are the host's; then header edits of three frames (nb 0, 11 and 0xFFFFFFFF, nr 15, a sum that runs over the end
    by one byte and one that ends exactly there, both sizes 0xFFFFFFFF, a terminator in a frame's place) held to the host's verdict likewise.
    Every failure exit of the walk is taken; a read outside the span is a SIGSEGV of the harness."""
    out = ok(runs, ("split",))
    m = re.search(r"split: streams=5 bytes=(\d+) cuts=(\d+) edits=(\d+) rejected=(\d+)", out)
    size = sum(len(runs["streams"][n]) for n in SPLIT)
    assert m and int(m.group(1)) == size and int(m.group(2)) == size + 1 and int(m.group(3)) == 24 and int(m.group(4)) >= 12
