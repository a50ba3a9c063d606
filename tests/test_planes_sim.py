"""CPU suite: the byte-plane role (nlzm_amd/csrc/nlzm_planes.h), forward and inverse, compiled for the host with every GPU lane a fiber
(tests/host_sim/planes_sim.cpp, a UBSan build, a program of its own), against the numpy model (tests/planes_model.py).

Every source lies in a mapping of its own between two PROT_NONE pages -- at the asked misalignment behind the page in front, or with its last byte
flush against the page behind --, so a read outside a range that leaves the mapping ends the harness; every destination lies between guard bytes
that have to stay as they were; LDS starts poisoned.  Up to eight ranges share a launch, and the case list is dealt to eight harness processes."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import pytest

from nlzm_amd import corpus
from tests import planes_model, simkit

SIM = os.path.join(simkit.SIMDIR, "planes_sim_san")
SHARDS = 8
ELEMS = planes_model.ELEMS
sh = partial(simkit.sh, timeout=900, env={"NLZM_SIM_POISON": "7"})


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    simkit.build("planes_sim_san")
    assert "-fsanitize=undefined" in simkit.compiled_with("planes_sim_san")
    assert "nlzm_amd/csrc/nlzm_planes.h" in simkit.compiled_from("planes_sim_san")
    d = tmp_path_factory.mktemp("planes_sim")
    (d / "g.txt").write_text("G\n")
    (d / "none.bin").write_bytes(b"")
    r = sh([SIM, d / "none.bin", d / "g.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    S = int(r.stdout.split()[0])
    assert S % 128 == 0
    # bytes that tell their positions apart: random ones, and a stretch of a counter so that a plane mixed up with its neighbour shows
    data = np.random.default_rng(corpus.SEED + 150).integers(0, 256, 2 * S + 300, dtype=np.uint8)
    data[1000:1512] = np.arange(512, dtype=np.uint32).astype(np.uint8)
    (d / "data.bin").write_bytes(data.tobytes())
    return {"dir": d, "S": S, "data": data, "n": 0}


def run_launches(sim, launches):
    """launches: [(inverse, [(mode, salign, start, n, e, dalign), ...])], eight ranges at most each; every range's result is held to the model"""
    d = sim["dir"]
    sim["n"] += 1
    shards = [launches[i::SHARDS] for i in range(SHARDS)]
    for i, sl in enumerate(shards):
        # (the launch's shape moves with the case: one to four waves per workgroup, one to three workgroups striding over the segments)
        (d / f"cases_{sim['n']}_{i}.txt").write_text("".join(
            f"L {inv} {64 * (1 + (j + len(rs)) % 4)} {1 + (j + rs[0][3]) % 3} {len(rs)}\n" + "".join(f"{m} {sa} {s} {n} {e} {da}\n" for m, sa, s, n, e, da in rs)
            for j, (inv, rs) in enumerate(sl)))
    with ThreadPoolExecutor(SHARDS) as ex:
        rs = list(ex.map(lambda i: sh([SIM, d / "data.bin", d / f"cases_{sim['n']}_{i}.txt"]), range(SHARDS)))
    bad, memo = [], {}
    for i, r in enumerate(rs):
        assert r.returncode == 0 and "planes_sim: OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]       # (-11: a read left a range)
        lines = r.stdout.splitlines()[:-1]
        assert len(lines) == len(shards[i])
        for (inv, ranges), line in zip(shards[i], lines):
            got = line.split()
            assert len(got) == len(ranges)
            for (m, sa, s, n, e, da), g in zip(ranges, got):
                key = (inv, s, n, e)
                if key not in memo:
                    memo[key] = f"{zlib.crc32(planes_model.apply(sim['data'][s: s + n], e, bool(inv))):08x}"
                if g != memo[key]:
                    bad.append((inv, m, sa, s, n, e, da, g, memo[key]))
    assert not bad, bad[:8]


def grouped(ranges, per=8):
    return [ranges[i: i + per] for i in range(0, len(ranges), per)]


@pytest.mark.parametrize("inverse", [0, 1])
def test_every_length_against_the_model(sim, inverse):
    """every e; every n from 0 to 2,100 and S - 1, S, S + 1, 2S + e + 3; sources behind the page in front and against the page behind in turn"""
    S = sim["S"]
    launches = []
    for e in ELEMS:
        rs = [("FB"[(n + e) % 2], n % 16, (3 * n + e) % 251, n, e, (7 * n + e) % 16) for n in range(0, 2101)]
        for n in (S - 1, S, S + 1, 2 * S + e + 3):
            rs += [("F", 0, 7, n, e, 0), ("B", 0, 11, n, e, 5), ("F", 9, 13, n, e, 11)]
        launches += [(inverse, g) for g in grouped(rs)]
    run_launches(sim, launches)


@pytest.mark.parametrize("inverse", [0, 1])
def test_every_source_misalignment(sim, inverse):
    """every source misalignment from 0 to 15, for every e and some twenty lengths, the ones round the segment size among them"""
    S = sim["S"]
    lengths = [1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1025, S - 1, S, S + 1]
    rs = [("F", sa, (5 * n + sa) % 251, n, e, (3 * sa + i + e) % 16) for e in ELEMS for i, n in enumerate(lengths + [2 * S + e + 3]) for sa in range(16)]
    run_launches(sim, [(inverse, g) for g in grouped(rs)])


@pytest.mark.parametrize("inverse", [0, 1])
def test_every_pair_of_misalignments_up_to_80_bytes(sim, inverse):
    """every e, every length from 0 to 80, every pair of source and destination misalignments"""
    rs = [("F", sa, (n + sa + da) % 251, n, e, da) for e in ELEMS for n in range(0, 81) for sa in range(16) for da in range(16)]
    run_launches(sim, [(inverse, g) for g in grouped(rs)])


@pytest.mark.parametrize("inverse", [0, 1])
def test_mixed_element_sizes_and_overlapping_sources_in_one_launch(sim, inverse):
    """eight ranges of one buffer in one launch: every e, sources that overlap and repeat, an empty range, a range of more than two segments"""
    S = sim["S"]
    rs = [("D", 0, 0, 5000, 4, 3), ("D", 0, 100, 9000, 2, 0), ("D", 0, 4999, 11, 8, 15), ("D", 0, 100, 9000, 8, 1), ("D", 0, 777, 0, 4, 9),
          ("D", 0, 3, 2 * S + 11, 8, 6), ("D", 0, 1000, 513, 1, 2), ("D", 0, 1001, 511, 2, 13)]
    run_launches(sim, [(inverse, rs), (inverse, rs[::-1]), (inverse, rs[2:5])])


def test_the_segment_size_is_the_librarys(sim):
    import nlzm_amd
    nlzm_amd.build()
    assert nlzm_amd.counter("planes_segment_bytes") == sim["S"]
