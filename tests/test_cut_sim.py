"""CPU suite: the cut-point roles (nlzm_amd/csrc/nlzm_cut.h), compiled for the host with every GPU lane a fiber
(tests/host_sim/cut_sim.cpp, a UBSan build, a program of its own), against the numpy model (tests/cut_model.py).

Every case runs twice: behind a PROT_NONE page (at the asked alignment; alignment 0 starts right after the page) and with its last byte
flush against the PROT_NONE page behind the buffer, so a read outside the input that leaves the mapping ends the harness; every output
buffer is followed by a guard word, and the selection runs again with a list one entry short.  The case list is dealt to eight harness
processes."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import cut_model, simkit
from tests.simkit import sh

SIM = os.path.join(simkit.SIMDIR, "cut_sim_san")
SHARDS = 8
AVG_BITS = [1, 4, 12]
MAX_LENS = [32, 48, 100, 1000]
KINDS = ["random", "text", "zeros", "ones"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    simkit.build("cut_sim_san")
    assert "-fsanitize=undefined" in simkit.compiled_with("cut_sim_san")
    assert "nlzm_amd/csrc/nlzm_cut.h" in simkit.compiled_from("cut_sim_san")
    d = tmp_path_factory.mktemp("cut_sim")
    (d / "g.txt").write_text("G\n")
    (d / "none.bin").write_bytes(b"")
    r = sh([SIM, d / "none.bin", d / "g.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    S = int(r.stdout.split()[0])
    part = 3 * S + 777 + 300
    parts = {
        "random": np.random.default_rng(corpus.SEED + 78).integers(0, 256, part, dtype=np.uint8),
        "text": corpus.syn_text(part),
        "zeros": np.zeros(part, dtype=np.uint8),
        "ones": np.full(part, 0xFF, dtype=np.uint8),
    }
    data = np.concatenate([parts[k][:part] for k in KINDS])
    (d / "data.bin").write_bytes(data.tobytes())
    return {"dir": d, "S": S, "data": data, "part": part, "memo": {}}


def run_cases(sim, cases):
    """cases: (kind, shift, n, align, avg_bits, min_len, max_len); returns [((cand, cuts), (cand, cuts))] in order"""
    d = sim["dir"]
    shards = [cases[i::SHARDS] for i in range(SHARDS)]
    tag = f"{len(cases)}_{abs(hash(tuple(cases[:3]))) % 10**8}"
    for i, sc in enumerate(shards):
        # (the launch's shape moves with the case: one to four waves per workgroup, one to three workgroups striding over the segments)
        (d / f"cases_{tag}_{i}.txt").write_text("".join(
            f"C {KINDS.index(k) * sim['part'] + s} {n} {a} {b} {lo} {hi} {64 * (1 + (j + n) % 4)} {1 + (j + a) % 3}\n" for j, (k, s, n, a, b, lo, hi) in enumerate(sc)))
    with ThreadPoolExecutor(SHARDS) as ex:
        rs = list(ex.map(lambda i: sh([SIM, d / "data.bin", d / f"cases_{tag}_{i}.txt"]), range(SHARDS)))
    got = [None] * len(cases)
    for i, r in enumerate(rs):
        assert r.returncode == 0 and "cut_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]       # (-11: a read left the buffer)
        lines = r.stdout.splitlines()[:-1]
        assert len(lines) == len(shards[i])
        out = []
        for l in lines:
            both = []
            for half in l.split(";"):
                v = [int(x) for x in half.split()]
                assert len(v) == 2 + v[1]
                both.append((v[0], v[2:]))
            out.append(tuple(both))
        got[i::SHARDS] = out
    return got


def expect(sim, case):
    k, s, n, a, b, lo, hi = case
    key = (k, s, n, b, lo, hi)
    if key not in sim["memo"]:
        at = KINDS.index(k) * sim["part"] + s
        x = sim["data"][at: at + n]
        # (no cut fits at n <= min_len: nothing is scanned, and the candidates are reported as none)
        sim["memo"][key] = (int(cut_model.candidates(x, b).size) if n > lo else 0, cut_model.cut_points(x, b, lo, hi))
    return sim["memo"][key]


def check(sim, cases):
    got = run_cases(sim, cases)
    bad = []
    for c, g in zip(cases, got):
        w = expect(sim, c)
        if g != (w, w):
            bad.append((c, w[0], w[1][:8], [(x[0], x[1][:8]) for x in g]))
    assert not bad, bad[:5]
    return got


def test_every_length_against_the_model(sim):
    """every n from 0 to 2,100 and S - 1, S, S + 1, 2S + 31, 3S + 777; avg_bits 1, 4 and 12, min_len 32, max_len small enough to force cuts;
    random bytes, text, all zeros and all 0xFF"""
    S = sim["S"]
    cases = [(KINDS[n % 4], n % 251, n, 0, AVG_BITS[n % 3], 32, MAX_LENS[(n // 12) % 4]) for n in range(0, 2101)]
    for n in (S - 1, S, S + 1, 2 * S + 31, 3 * S + 777):
        for k in KINDS:
            for b in AVG_BITS:
                cases.append((k, 7, n, 0, b, 32, 100 if b == 12 else 1000))
            cases.append((k, 7, n, 0, 12, 1024, 16384))       # (avg_bits 12 with its default lengths: cuts by candidates, whole segments skipped by their counts)
            cases.append((k, 7, n, 0, 12, 32, 1 << 31))       # (no forced cut: on equal bytes all positions are candidates, or none)
    got = check(sim, cases)
    assert any(len(g[0][1]) > 1000 for g in got) and any(g[0][0] == 0 and c[2] > S for c, g in zip(cases, got))


def test_every_alignment_against_the_model(sim):
    """every start alignment from 0 to 15 for some twenty lengths"""
    S = sim["S"]
    lengths = [33, 34, 47, 48, 49, 63, 64, 65, 95, 96, 97, 511, 512, 513, 543, 544, 545, 1024, 2049, S - 1, S, S + 1, 2 * S + 31, 3 * S + 777]
    cases = [(KINDS[(i + a) % 4], (7 * n + a) % 251, n, a, AVG_BITS[(i + a) % 3], 32, MAX_LENS[(i + a) % 4]) for i, n in enumerate(lengths) for a in range(16)]
    check(sim, cases)


def test_the_segment_size_is_the_librarys(sim):
    import nlzm_amd
    nlzm_amd.build()
    assert nlzm_amd.counter("cut_segment_bytes") == sim["S"]
