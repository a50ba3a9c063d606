"""CPU suite: the CRC32, equal-range and byte-plane roles at offsets on either side of 2^32 of one buffer, in the fiber simulator
(tests/host_sim/far_sim.cpp), against the sparse model (tests/far_model.py) -- the small-range cases of tests/test_gpu_far.py, for a machine without a
GPU.  The buffer is a mapping of 2^32 + 2^22 bytes made with MAP_NORESERVE; only the pages round the islands are touched (the fill is written
256 KiB to either side of every island, and every case stays inside those stretches).  Where the kernel refuses the mapping the harness leaves
with status 4 and these tests skip, saying so.  The ranges longer than 2^32 are the device's: the simulator would take hours."""
import os
import zlib

import numpy as np
import pytest

from tests import far_model, planes_model, simkit

SIM = os.path.join(simkit.SIMDIR, "far_sim_san")
SEED = 20261
LINE, N, S = far_model.LINE, far_model.N, far_model.S
MARGIN = 1 << 18
CRC_SEG, PLANES_SEG = 32768, 8192


@pytest.fixture(scope="module")
def far(tmp_path_factory):
    simkit.build("far_sim_san")
    model, where = far_model.far_with_copies(SEED)
    d = tmp_path_factory.mktemp("far")
    blob, head, zones = b"", [f"M {N}"], []
    for o, b in model.islands:
        a, e = max(0, o - MARGIN), min(N, o + b.size + MARGIN)
        if zones and a <= zones[-1][1]:
            zones[-1][1] = e
        else:
            zones.append([a, e])
    head += [f"Z {a} {e - a} {model.fill}" for a, e in zones]
    for o, b in model.islands:
        head.append(f"I {o} {b.size} {len(blob)}")
        blob += b.tobytes()
    (d / "islands.bin").write_bytes(blob)
    return {"model": model, "where": where, "dir": d, "head": head, "zones": zones}


def run(far, lines, inside):
    """the harness on the layout and `lines`; `inside`: the (offset, length) stretches of the source the lines read, which must lie where the fill was written"""
    for o, l in inside:
        assert any(a <= o and o + l <= e for a, e in far["zones"]), (o, l)
    cases = far["dir"] / "cases.txt"
    cases.write_text("\n".join(far["head"] + lines) + "\n")
    r = simkit.sh([SIM, far["dir"] / "islands.bin", cases], 600)
    if r.returncode == 4:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0 and r.stdout.endswith("far_sim: OK\n"), r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()[:-1]
    assert len(out) == len(lines)
    return [line.split() for line in out]


def test_crc32_ranges_round_the_lines(far):
    m = far["model"]
    seg = CRC_SEG
    ranges = [r for r in far_model.edge_ranges(LINE, N, seg) if r[1] < 1 << 20]
    assert len(ranges) > 300 and any(o < LINE < o + l for o, l in ranges) and any(o > LINE and l > seg for o, l in ranges) and any(o + l == N and l > seg for o, l in ranges)
    got = run(far, [f"C {len(ranges)} " + " ".join(f"{o} {l}" for o, l in ranges)], ranges)[0]
    for (o, l), g in zip(ranges, got):
        assert int(g, 16) == m.crc32(o, l), f"crc roles: offset {o} (2^32 {o - LINE:+d}), {l} bytes: got {g}, want {m.crc32(o, l):08x}"


def test_fingerprints_and_compares_of_copies_on_either_side_of_the_line(far):
    m, w = far["model"], far["where"]
    P = far_model.PIECE
    places = [w["across"]] + [o for pair in zip(w["below"], w["above"]) for o in pair]          # (all sixteen misalignments on either side)
    ranges = [(o, P) for o in places] + [(w["near"], P)] + [(o, S + 1) for o in places[::2]] + [(LINE + d, 100 + d) for d in range(-17, 18, 5)] + [(LINE - 5, 0)]
    got = run(far, [f"F {len(ranges)} " + " ".join(f"{o} {l}" for o, l in ranges)], ranges)[0]
    for (o, l), g in zip(ranges, got):
        assert int(g, 16) == m.fingerprint(o, l), f"fingerprint roles: offset {o} (2^32 {o - LINE:+d}), {l} bytes: got {g}, want {m.fingerprint(o, l):016x}"
    assert len(set(got[: len(places)])) == 1 and got[len(places)] != got[0]
    pairs = [(places[0], o, P) for o in places[1:]] + [(places[0], w["near"], P), (places[3], w["near"], P), (w["near"], places[6], P - 1), (places[2], places[7], 0),
                                                       (places[1] + 1, places[8] + 1, P - 1), (places[0], w["near"], P - 1)]
    got = run(far, [f"Q {len(pairs)} " + " ".join(f"{a} {b} {l}" for a, b, l in pairs)], [(a, l) for a, _, l in pairs] + [(b, l) for _, b, l in pairs])[0]
    for (a, b, l), g in zip(pairs, got):
        want = int(np.array_equal(m.read(a, l), m.read(b, l)))
        assert int(g) == want, f"pair roles: offsets {a} (2^32 {a - LINE:+d}) and {b} (2^32 {b - LINE:+d}), {l} bytes: got {g}, want {want}"
    assert [int(g) for g in got[len(places) - 1: len(places) + 2]] == [0, 0, 1]


@pytest.mark.parametrize("inverse", [0, 1])
def test_planes_small_ranges_on_either_side_of_the_line(far, inverse):
    m = far["model"]
    calls = far_model.planes_calls(LINE, PLANES_SEG)
    lines = [f"P {inverse} {len(c)} " + " ".join(f"{s} {d} {n} {e}" for s, d, n, e in c) for c in calls]
    got = run(far, lines, [(s, n) for c in calls for s, _, n, _ in c])
    for c, g in zip(calls, got):
        for (s, d, n, e), v in zip(c, g):
            want = zlib.crc32(planes_model.apply(m.read(s, n), e, bool(inverse)))
            assert int(v, 16) == want, (f"planes role (inverse {inverse}, e {e}): source {s} (2^32 {s - LINE:+d}), destination {d} (2^32 {d - LINE:+d}), {n} bytes: "
                                        f"CRC32 of the destination {v}, want {want:08x}")
