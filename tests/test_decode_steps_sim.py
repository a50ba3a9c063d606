"""CPU suite: the STEPPING form of the device decoder's role (dec::decode_role_steps, nlzm_amd/csrc/nlzm_decode.h), compiled for the host with
every GPU lane a fiber (tests/host_sim/decode_steps_sim.cpp): a decode that pauses in front of a frame header, saves its state and is resumed
by a later launch writes the bytes, reports the lengths and counts the counters of the one-shot role; input that arrives later pauses it
without a read outside [src, src + len); damaged streams end with the one-shot role's code.

Streams are the reference's (oracle_py.compress, as in tests/test_decode_sim.py).  As there, every buffer the role sees -- here the state
record too -- lies between two PROT_NONE pages with canaries beside it, the cut and damaged sources flush against the page behind them,
and the damaged streams run in a UBSan build of the stand-alone harness.  All runs (one process each) are started together when the first
test asks for one, the longest first: 417 s of CPU time, 60 s on eight cores with the three harnesses built (building them adds 14 s),
measured with nothing else running -- at the one-minute budget, not under it.  The simulator decodes ~60,000 rANS symbols a second; the cut
sweep of dense_150k_w17 is 386 cuts at about 0.65 s each, dealt to eight processes.  Its cuts (not chunk_plus1's, which all start at the
stream's first byte) start from the state saved one frame in front of the cut's last whole frame, so that every cut still decodes a
frame and then pauses in front of the one that is not whole: a use of the feature under test that keeps the sweep complete at a third of
the cost of 386 decodes from the first byte."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cases, oracle_py, simkit

HERE = os.path.dirname(os.path.abspath(__file__))
WORKERS = max(1, min(8, os.cpu_count() or 2))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "streams.json")))["cases"]}

FRAMES = {"chunk_plus1": 2, "cutnice_60k_w17": 5, "dense_150k_w17": 5, "runs_300k_w18": 5, "dups_600k_w20": 5, "text_200k_w15": 14, "dups_400k_w16": 27}
# (stream, build, misalignment of the destination)
STEPS = [("chunk_plus1", "product", 1), ("dense_150k_w17", "product", 7), ("text_200k_w15", "product", 15), ("dups_400k_w16", "tiny", 1)]
SIZE_ONLY = ["chunk_plus1", "cutnice_60k_w17"]
TARGET_STRIDE = 4099
MORE = [("chunk_plus1", 4, False), ("dense_150k_w17", 8, True)]      # (stream, processes the cuts are dealt to, far cuts start from a saved state)
MORE_STRIDE = 97
FLIPS, FLIP_PARTS = 100, 2
TARGET_PARTS = 4
BLOCKS_K = 5


def sha(b):
    return hashlib.sha256(b).hexdigest()


def case_of(name):
    return next(c for c in cases.CASES if c[0] == name)


def heads_of(stream):
    """the stream offsets of the frame headers, the terminator's last"""
    h, pos = [], 4
    while True:
        h.append(pos)
        if not int.from_bytes(stream[pos:pos + 4], "big"):
            return h
        pos += int.from_bytes(stream[pos + 4:pos + 8], "big") + int.from_bytes(stream[pos + 8:pos + 12], "big")


def cuts_of(stream):
    """every offset within 16 bytes of a frame header, every 97th elsewhere: the sweep no cut of which may be left out"""
    c = set(range(0, len(stream), MORE_STRIDE))
    for h in heads_of(stream):
        c.update(x for x in range(max(0, h - 16), h + 17) if x < len(stream))
    return c


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    SIM, SIM_TINY, SIM_SAN = simkit.build("decode_steps_sim", "decode_steps_sim_tiny", "decode_steps_sim_san", jobs=3)
    d = tmp_path_factory.mktemp("decode_steps_sim")
    streams, inputs = {}, {}
    for n in FRAMES:
        inputs[n] = cases.make_case(case_of(n)).tobytes()
        streams[n] = oracle_py.compress(np.frombuffer(inputs[n], dtype=np.uint8), case_of(n)[4])
        (d / f"{n}.nlzm").write_bytes(streams[n])
    bdata = corpus.mixed(700_000, corpus.SEED + 9)         # (tests/test_decode_sim.py's blocks_input())
    branges = [shard.block_range(bdata.size, BLOCKS_K, i) for i in range(BLOCKS_K)]
    (d / "blocks.nlzm").write_bytes(b"".join(oracle_py.compress(bdata[lo:hi], 18) for lo, hi in branges))
    jobs = []                                              # (key, command), the longest first
    for n, build, mis in sorted(STEPS, key=lambda s: -len(streams[s[0]]))[:1]:
        jobs.append((("steps", n), [SIM_TINY if build == "tiny" else SIM, "steps", d / f"{n}.nlzm", d / f"{n}.out", 1, mis]))
    for n, parts, near in sorted(MORE, key=lambda m: -len(streams[m[0]])):
        jobs += [(("more", n, s), [SIM, "more", d / f"{n}.nlzm", MORE_STRIDE, s, parts, int(near)]) for s in range(parts)]
    jobs += [(("mutants", s), [SIM_SAN, "mutants", d / "chunk_plus1.nlzm", 7, FLIPS, s, FLIP_PARTS]) for s in range(FLIP_PARTS)]
    jobs += [(("targets", s), [SIM, "targets", d / "dense_150k_w17.nlzm", TARGET_STRIDE, s, TARGET_PARTS]) for s in range(TARGET_PARTS)]
    for n, build, mis in sorted(STEPS, key=lambda s: -len(streams[s[0]]))[1:]:
        jobs.append((("steps", n), [SIM_TINY if build == "tiny" else SIM, "steps", d / f"{n}.nlzm", d / f"{n}.out", 1, mis]))
    jobs.append((("blocks",), [SIM, "blocks", d / "blocks.nlzm", d / "blocks.out"]))
    for n in SIZE_ONLY:
        jobs.append((("size", n), [SIM, "steps", d / f"{n}.nlzm", d / f"{n}.none", 1, 3, "size"]))
    started = simkit.Runs(WORKERS)
    for key, cmd in jobs:
        started.submit(key, cmd)
    yield {"runs": started, "dir": d, "streams": streams, "inputs": inputs, "blocks": (bdata.tobytes(), branges)}
    started.close()


def ok(runs, key):
    return runs["runs"].ok(key, "decode_steps_sim: OK").stdout


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_counts(runs, name):
    """the streams are the reference's, and their frames what the cases below count on"""
    assert sha(runs["streams"][name]) == GOLD[name]["stream_sha256"]
    assert len(heads_of(runs["streams"][name])) - 1 == FRAMES[name]


@pytest.mark.parametrize("name,build,mis", STEPS)
def test_one_frame_per_launch_to_the_end(runs, name, build, mis):
    """After launch k out_len is min(k * chunk_size, n) and the bytes so far are the input's (the harness compares them, and finds nothing
    written beyond them, after EVERY launch); at the end every counter -- ring_bytes and global_bytes among them -- is the one-shot role's on
    the same stream.  The destination is misaligned (1, 7, 15), so the ring's reload meets the head and tail bytes a flush meets."""
    out = ok(runs, ("steps", name))
    c = case_of(name)
    n, chunk = c[2], nlzm_amd.geometry(c[2], c[4])["chunk_size"]
    assert f"ring={512 if build == 'tiny' else 65536} " in out and f"frames={FRAMES[name]}\n" in out
    launches = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"^launch (\d+) rc=(-?\d+) why=(\d+) out_len=(\d+)$", out, re.M)]
    assert [l[0] for l in launches] == list(range(1, FRAMES[name] + 1))
    for k, rc, why, out_len in launches:
        assert out_len == min(k * chunk, n), k
        assert (rc, why) == ((0, 0) if k == FRAMES[name] else (1, 1)), k        # paused for "frames" until the terminator ends the last launch
    one, stepped = (next(l for l in out.splitlines() if l.startswith(tag)).split()[1:] for tag in ("oneshot ", "stepped "))
    assert one == stepped and f"out_len={n}" in one
    if build == "tiny":
        fields = dict(f.split("=") for f in stepped)
        assert int(fields["global_bytes"]) > int(fields["ring_bytes"]) > 0       # (nearly every match reaches beyond a 512-byte ring)
    assert sha((runs["dir"] / f"{name}.out").read_bytes()) == GOLD[name]["input_sha256"]


def test_targets(runs):
    """Targets 0, 1, every 4,099th byte, n - 1, n, n + 1 on dense_150k_w17: the decode stops at the first frame boundary at or above the
    target, or at the end; a second launch with the same target decodes not a symbol; going on gives the input."""
    n = case_of("dense_150k_w17")[2]
    sweep = {0, 1, n - 1, n, n + 1} | set(range(0, n + 1, TARGET_STRIDE))
    ran = ended = 0
    for s in range(TARGET_PARTS):
        m = re.search(r"targets=(\d+) ran=(\d+) ended=(\d+) boundaries=(\d+)", ok(runs, ("targets", s)))
        assert m and int(m.group(1)) == len(sweep) and int(m.group(4)) == FRAMES["dense_150k_w17"] + 1
        ran, ended = ran + int(m.group(2)), ended + int(m.group(3))
    chunk = nlzm_amd.geometry(n, 17)["chunk_size"]
    assert ran == len(sweep)
    assert ended == sum(1 for t in sweep if t > (FRAMES["dense_150k_w17"] - 1) * chunk)      # (beyond the last boundary the terminator ends the decode)


@pytest.mark.parametrize("name,parts,near", MORE)
def test_input_that_arrives_later(runs, name, parts, near):
    """kMore with len cut at every offset within 16 bytes of each frame header and at every 97th elsewhere, the source flush against the page
    behind it: the launch pauses "for input" after exactly the frames that lie wholly inside len, goes on to the end once len is raised, and
    the bytes are the input's; the same cuts without kMore are today's kErrFormat, detail 3 (1 below eight bytes, as today).  The number of
    cuts run is the sweep's, computed here from the stream."""
    stream = runs["streams"][name]
    want = len(cuts_of(stream))
    total = ran = 0
    for s in range(parts):
        out = ok(runs, ("more", name, s))
        m = re.search(r"more: bytes=(\d+) frames=(\d+) cuts=(\d+) ran=(\d+)", out)
        assert m and int(m.group(1)) == len(stream) and int(m.group(2)) == FRAMES[name]
        total, ran = int(m.group(3)), ran + int(m.group(4))
    assert total == ran == want


@pytest.mark.parametrize("name", SIZE_ONLY)
def test_size_only_stepping(runs, name):
    out = ok(runs, ("size", name))
    n = case_of(name)[2]
    stepped = next(l for l in out.splitlines() if l.startswith("stepped "))
    assert f"out_len={n} " in stepped and f"launches={FRAMES[name]}\n" in out


def test_damaged_streams_under_ubsan(runs):
    """the first 100 single-bit flips of tests/test_decode_sim.py's generator on chunk_plus1, one frame a launch: rc and detail are the one-shot
    role's, accepted / rejected the host decoder's, for every one"""
    ran = pauses = 0
    for s in range(FLIP_PARTS):
        m = re.search(r"mutants=(\d+) ran=(\d+) accepted=(\d+) pauses=(\d+)", ok(runs, ("mutants", s)))
        assert m and int(m.group(1)) == FLIPS
        ran, pauses = ran + int(m.group(2)), pauses + int(m.group(4))
    assert ran == FLIPS and pauses > 0


def test_five_blocks_with_targets(runs):
    """targets [0, 1, raw / 2, to the end, 0]: blocks 0 and 4 are not launched, the others stop at their frame boundaries; a second launch ends
    all five; no block writes into another's range (the harness finds every byte a block has not decoded yet untouched)"""
    data, ranges = runs["blocks"]
    out = ok(runs, ("blocks",))
    raws = [hi - lo for lo, hi in ranges]
    chunks = [nlzm_amd.geometry(r, 18)["chunk_size"] for r in raws]
    rounds = {int(m.group(1)): (int(m.group(2)), list(map(int, m.group(3).split(",")))) for m in re.finditer(r"round (\d) launched=(\d+) done=([\d,]+)", out)}
    first = lambda t, i: min(raws[i], -(-t // chunks[i]) * chunks[i])
    assert rounds[0] == (3, [0, first(1, 1), first(raws[2] // 2, 2), raws[3], 0])
    assert rounds[1] == (4, raws)
    assert (runs["dir"] / "blocks.out").read_bytes() == data
