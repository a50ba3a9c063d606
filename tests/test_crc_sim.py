"""CPU suite: the device CRC32's roles (nlzm_amd/csrc/nlzm_crc.h), compiled for the host with every GPU lane a fiber
(tests/host_sim/crc_sim.cpp, a UBSan build), against zlib.crc32.

Every case is hashed twice: behind a PROT_NONE page (at the asked alignment; alignment 0 starts right after the page) and with its last
byte flush against the PROT_NONE page behind the buffer, so a read outside the range that leaves the mapping ends the harness.  The case
list is dealt to eight harness processes, each of which runs its share in one go and prints one line per case: 8 s on eight cores
from a clean tree (4 s of it the build), 30 s of CPU time in all."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import simkit
from tests.simkit import sh

SIM = os.path.join(simkit.SIMDIR, "crc_sim_san")
SHARDS = 8
SEEDS = [0, 0x9E3779B9]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    simkit.build("crc_sim_san")
    d = tmp_path_factory.mktemp("crc_sim")
    (d / "g.txt").write_text("G\n")
    (d / "none.bin").write_bytes(b"")
    r = sh([SIM, d / "none.bin", d / "g.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    G = int(r.stdout.split()[0])
    data = np.random.default_rng(corpus.SEED + 32).integers(0, 256, 3 * G + 777 + 300, dtype=np.uint8).tobytes()
    (d / "data.bin").write_bytes(data)
    return {"dir": d, "G": G, "data": data}


def lengths_of(G):
    return list(range(0, 2101)) + [G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 777]


def aligned_lengths_of(G):
    """some thirty lengths that get every start alignment"""
    return [0, 1, 2, 3, 14, 15, 16, 17, 18, 31, 32, 33, 47, 63, 64, 65, 1007, 1008, 1023, 1024, 1025, 1039, 1040, 2047, 2048, 2049,
            G - 1, G, G + 1, 2 * G - 1, 2 * G + 1, 3 * G + 777]


def run_cases(sim, cases):
    """cases: (start, n, align, seed); returns [(front, back)] in order"""
    d = sim["dir"]
    shards = [cases[i::SHARDS] for i in range(SHARDS)]
    tag = f"{len(cases)}_{abs(hash(tuple(cases[:3]))) % 10**8}"
    for i, sc in enumerate(shards):
        # (the launch's shape moves with the case: one to four waves per workgroup, one to three workgroups striding over the segments)
        (d / f"cases_{tag}_{i}.txt").write_text("".join(f"C {s} {n} {a} {seed} {64 * (1 + (j + n) % 4)} {1 + (j + a) % 3}\n" for j, (s, n, a, seed) in enumerate(sc)))
    with ThreadPoolExecutor(SHARDS) as ex:
        rs = list(ex.map(lambda i: sh([SIM, d / "data.bin", d / f"cases_{tag}_{i}.txt"]), range(SHARDS)))
    got = [None] * len(cases)
    for i, r in enumerate(rs):
        assert r.returncode == 0 and "crc_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]       # (-11: a read left the buffer)
        lines = r.stdout.splitlines()[:-1]
        assert len(lines) == len(shards[i])
        got[i::SHARDS] = [tuple(int(x, 16) for x in l.split()) for l in lines]
    return got


def expect(sim, cases):
    return [zlib.crc32(sim["data"][s:s + n], seed) for s, n, a, seed in cases]


def test_every_length_against_zlib(sim):
    """every length from 0 to 2,100, the segment size G - 1, G, G + 1, 2G - 1, 2G, 2G + 1 and 3G + 777, at alignment 0 behind the guard page and
    flush against the one behind, from two seeds"""
    cases = [(i % 251, n, 0, seed) for seed in SEEDS for i, n in enumerate(lengths_of(sim["G"]))]
    got, want = run_cases(sim, cases), expect(sim, cases)
    bad = [(c, hex(w), [hex(x) for x in g]) for c, g, w in zip(cases, got, want) if g != (w, w)]
    assert not bad, bad[:10]


def test_every_alignment_against_zlib(sim):
    """every start alignment from 0 to 15 for some thirty lengths: round 0, 16, 1,024 (a wave's step), 2,048 and the segment size"""
    cases = [((7 * n + a) % 251, n, a, seed) for seed in SEEDS for n in aligned_lengths_of(sim["G"]) for a in range(16)]
    got, want = run_cases(sim, cases), expect(sim, cases)
    bad = [(c, hex(w), [hex(x) for x in g]) for c, g, w in zip(cases, got, want) if g != (w, w)]
    assert not bad, bad[:10]


def test_forty_mixed_ranges_in_one_call(sim):
    """one call of 40 ranges of one buffer between two guard pages: empty ones, overlapping ones, one that is the whole buffer, one that ends
    at its last byte, several longer than a segment"""
    G, d = sim["G"], sim["dir"]
    page = os.sysconf("SC_PAGESIZE")
    B = (3 * G + 777) // page * page
    rng = np.random.default_rng(corpus.SEED + 33)
    ranges = [(0, B), (B, 0), (0, 0), (B - 1, 1), (5, 0), (1, G), (1, G), (G - 3, G + 6), (17, 2 * G + 1)]
    while len(ranges) < 40:
        off = int(rng.integers(0, B))
        ranges.append((off, int(rng.integers(0, min(B - off, 3000 if len(ranges) % 3 else B) + 1))))
    (d / "ranges.txt").write_text(f"R {B} {len(ranges)} " + " ".join(f"{o} {l}" for o, l in ranges) + "\n")
    r = sh([SIM, d / "data.bin", d / "ranges.txt"])
    assert r.returncode == 0 and "crc_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    got = [int(x, 16) for x in r.stdout.splitlines()[0].split()]
    assert got == [zlib.crc32(sim["data"][o:o + l]) for o, l in ranges]
    assert sum(1 for o, l in ranges if l == 0) >= 3 and sum(1 for o, l in ranges if l > G) >= 4
