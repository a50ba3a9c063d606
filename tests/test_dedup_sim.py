"""CPU suite: the equal-range finder's roles (nlzm_amd/csrc/nlzm_dedup.h), compiled for the host with every GPU lane a fiber
(tests/host_sim/dedup_sim.cpp, a UBSan build, a program of its own), against the numpy model (tests/dedup_model.py) and byte comparisons.

Every fingerprint is taken twice: behind a PROT_NONE page (at the asked alignment; alignment 0 starts right after the page) and with the range's
last byte flush against the PROT_NONE page behind, so a read outside the range that leaves the mapping ends the harness.  Every pair is judged
three times, each side in a region of its own between PROT_NONE pages: both at their alignments behind the front pages, then each side in turn
flush against the page behind it.  Every output array is followed by a guard word, and the launch's shape moves from case to case.  The case
list is dealt to eight harness processes."""
import os
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import dedup_model, simkit

SIM = os.path.join(simkit.SIMDIR, "dedup_sim_san")
SHARDS = 8
KINDS = ["random", "text", "zeros", "ones"]
sh = partial(simkit.sh, timeout=900)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    simkit.build("dedup_sim_san")
    assert "-fsanitize=undefined" in simkit.compiled_with("dedup_sim_san")
    assert "nlzm_amd/csrc/nlzm_dedup.h" in simkit.compiled_from("dedup_sim_san")
    d = tmp_path_factory.mktemp("dedup_sim")
    (d / "g.txt").write_text("G\n")
    (d / "none.bin").write_bytes(b"")
    r = sh([SIM, d / "none.bin", d / "g.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    S, Cn = (int(x) for x in r.stdout.split()[:2])
    assert S == dedup_model.SEGMENT
    part = 3 * S + 777 + 300
    parts = {
        "random": np.random.default_rng(corpus.SEED + 120).integers(0, 256, part, dtype=np.uint8),
        "text": corpus.syn_text(part),
        "zeros": np.zeros(part, dtype=np.uint8),
        "ones": np.full(part, 0xFF, dtype=np.uint8),
    }
    data = np.concatenate([parts[k][:part] for k in KINDS])
    (d / "data.bin").write_bytes(data.tobytes())
    return {"dir": d, "S": S, "C": Cn, "data": data, "part": part, "memo": {}, "runs": 0}


def shape(j, n):
    """one to four waves a workgroup, one to three workgroups striding over the segments, ranges, chunks and pairs"""
    return 64 * (1 + (j + n) % 4), 1 + (j + n // 3) % 3


def run_lines(sim, lines):
    """the case lines dealt to SHARDS processes; their output lines, in order"""
    d = sim["dir"]
    sim["runs"] += 1
    shards = [lines[i::SHARDS] for i in range(SHARDS)]
    for i, sc in enumerate(shards):
        (d / f"cases_{sim['runs']}_{i}.txt").write_text("".join(l + "\n" for l in sc))
    with ThreadPoolExecutor(SHARDS) as ex:
        rs = list(ex.map(lambda i: sh([SIM, d / "data.bin", d / f"cases_{sim['runs']}_{i}.txt"]), range(SHARDS)))
    got = [None] * len(lines)
    for i, r in enumerate(rs):
        assert r.returncode == 0 and "dedup_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]       # (-11: a read left the buffer)
        out = r.stdout.splitlines()[:-1]
        assert len(out) == len(shards[i])
        got[i::SHARDS] = out
    return got


def at_of(sim, kind, shift):
    return KINDS.index(kind) * sim["part"] + shift


def want_fp(sim, kind, shift, n):
    key = (kind, shift, n)
    if key not in sim["memo"]:
        at = at_of(sim, kind, shift)
        sim["memo"][key] = dedup_model.fingerprint(sim["data"][at: at + n])
    return sim["memo"][key]


def check_fingerprints(sim, cases):
    """cases: (kind, shift, n, align)"""
    lines = [f"F {at_of(sim, k, s)} {n} {a} {shape(j, n)[0]} {shape(j, n)[1]}" for j, (k, s, n, a) in enumerate(cases)]
    bad = []
    for c, l in zip(cases, run_lines(sim, lines)):
        got = [int(x, 16) for x in l.split()]
        w = want_fp(sim, c[0], c[1], c[2])
        if got != [w, w]:
            bad.append((c, hex(w), l))
    assert not bad, bad[:5]


def test_every_length_against_the_model(sim):
    """every n from 0 to 2,100 and S - 1, S, S + 1, 2S + 31, 3S + 777; random bytes, text, all zeros and all 0xFF"""
    S = sim["S"]
    cases = [(KINDS[n % 4], n % 251, n, 0) for n in range(0, 2101)]
    cases += [(k, 7, n, 0) for n in (S - 1, S, S + 1, 2 * S + 31, 3 * S + 777) for k in KINDS]
    check_fingerprints(sim, cases)


def test_every_alignment_against_the_model(sim):
    """every start alignment from 0 to 15 for some twenty lengths: the same bytes give the same value at all sixteen"""
    S = sim["S"]
    lengths = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 1024, 2049, S - 1, S, S + 1, 2 * S + 31, 3 * S + 777]
    check_fingerprints(sim, [(KINDS[i % 4], (7 * n) % 251, n, a) for i, n in enumerate(lengths) for a in range(16)])


def test_many_ranges_in_one_launch(sim):
    """a thousand ranges of one buffer in one launch -- empty, overlapping, repeated, unordered, some of several segments -- and one launch of ranges
    that tile the buffer: every fingerprint is the model's of that range's bytes"""
    S, data = sim["S"], sim["data"]
    rng = np.random.default_rng(corpus.SEED + 121)
    lists = []
    ranges = []
    for i in range(1000):
        ln = 0 if i % 97 == 0 else int(rng.integers(0, 300)) if i % 50 else int(rng.integers(S, 2 * S + 100))
        ranges.append((int(rng.integers(0, data.size - ln + 1)), ln))
    ranges[5] = ranges[3]
    lists.append(ranges)
    edges = [0, 1, 17, S, S + 5, 3 * S + 4, 3 * S + 4, 5 * S, int(data.size)]
    lists.append([(a, b - a) for a, b in zip(edges, edges[1:])][::-1])
    lists.append([(int(data.size), 0)])
    lines = [f"R {64 * (1 + j)} {1 + j} {len(r)} " + " ".join(f"{o} {l}" for o, l in r) for j, r in enumerate(lists)]
    for r, l in zip(lists, run_lines(sim, lines)):
        assert [int(x, 16) for x in l.split()] == dedup_model.fingerprints(data, r)


def check_pairs(sim, cases):
    """cases: (kind_a, shift_a, kind_b, shift_b, n, align_a, align_b, flip)"""
    data = sim["data"]
    lines, want = [], []
    for j, (ka, sa, kb, sb, n, aa, ab, flip) in enumerate(cases):
        a, b = at_of(sim, ka, sa), at_of(sim, kb, sb)
        lines.append(f"P {a} {b} {n} {aa} {ab} {flip} {shape(j, n)[0]} {shape(j, n)[1]}")
        want.append(int(flip < 0 and bool(np.array_equal(data[a: a + n], data[b: b + n]))))
    bad = [(c, w, l) for c, w, l in zip(cases, want, run_lines(sim, lines)) if [int(x) for x in l.split()] != [w] * 3]
    assert not bad, bad[:5]
    return want


def test_pairs_every_misalignment(sim):
    """all 256 pairs of misalignments (a, b), each with every length 0 .. 80, and with one chunk, two chunks or their neighbours: equal strings are
    equal; strings from two places of random bytes or text are not (but two runs of zeros are)"""
    Cn = sim["C"]
    cases = []
    for aa in range(16):
        for ab in range(16):
            i = 16 * aa + ab
            for n in range(81):
                cases.append((KINDS[(i + n) % 4], (i + n) % 251, KINDS[(i + n) % 4], (i + n) % 251, n, aa, ab, -1))
            cases.append((KINDS[i % 2], 3, KINDS[i % 2], 3 + (i % 5 == 0), (Cn, 2 * Cn, 81 + i, Cn + 1)[i % 4], aa, ab, -1))
            cases.append(("zeros", 1, "zeros", 9, 60 + i, aa, ab, -1))
    want = check_pairs(sim, cases)
    assert {c[4] for c in cases} >= set(range(81)) and 0 in want and want.count(1) > 1000


def test_pairs_a_single_flipped_byte_is_found(sim):
    """lengths 1 .. 80: every position; one and two chunks and their neighbours: the first byte, the last, either side of the first and the last
    16-byte boundary and of every chunk boundary; the misalignments rotate through all 256 pairs"""
    Cn = sim["C"]
    cases, i = [], 0
    for n in range(1, 81):
        for flip in range(n):
            cases.append((KINDS[i % 4], i % 251, KINDS[i % 4], i % 251, n, i % 16, (i // 16) % 16, flip))
            i += 1
    for n in (Cn - 1, Cn, Cn + 1, 2 * Cn, 2 * Cn + 31):
        spots = {0, 15, 16, n - 1, (n - 1) // 16 * 16 - 1, (n - 1) // 16 * 16, Cn - 17, Cn - 16, Cn - 2}
        spots |= {p for c in range(Cn, n, Cn) for p in (c - 1, c, c + 15, c + 16)}
        for flip in sorted(p for p in spots if 0 <= p < n):
            cases.append((KINDS[i % 4], 11, KINDS[i % 4], 11, n, (5 * i) % 16, (3 * i + 1) % 16, flip))
            i += 1
    assert not any(check_pairs(sim, cases))


def test_many_pairs_in_one_launch_and_overlapping_sides(sim):
    """pairs of offsets into one buffer in one launch: sides that overlap each other (runs of zeros and of 0xFF shifted by 1 .. 40 bytes are equal,
    text shifted is not), sides shared between pairs, empty pairs, pairs of several chunks"""
    Cn, data, part = sim["C"], sim["data"], sim["part"]
    z, o, t = 2 * part, 3 * part, part
    pairs = [(z, z + d, n) for d in (1, 7, 16, 40) for n in (0, 1, 33, Cn + 5, 2 * Cn + 31)]
    pairs += [(o + 3, o + 3 + d, 1000 + d) for d in (1, 15, 17)]
    pairs += [(t, t + d, n) for d in (1, 16) for n in (1, 50, Cn + 5)]
    pairs += [(t + 5, t + 5, 3 * Cn + 100), (z, o, 0), (z + 9, z + 9, 77), (z, o, 20), (z + part - 10, o, 20)]
    lines = [f"Q {64 * (1 + j)} {1 + 2 * j} {len(pairs)} " + " ".join(f"{a} {b} {n}" for a, b, n in pairs) for j in range(2)]
    want = [int(np.array_equal(data[a: a + n], data[b: b + n])) for a, b, n in pairs]
    assert 0 in want and want.count(1) > 20
    for l in run_lines(sim, lines):
        assert [int(x) for x in l.split()] == want


def test_the_segment_size_is_the_librarys(sim):
    import nlzm_amd
    nlzm_amd.build()
    assert nlzm_amd.counter("dedup_segment_bytes") == sim["S"]
