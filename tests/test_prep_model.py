"""CPU suite: tests/prep_model.py -- the model that tests/test_gpu_prep.py holds the pre-pass kernels to -- is held first, by something that
is not the model: RK256's closed form by the oracle's hash and the reference's roll, the pre-filter's marks by a brute-force truth without
any hashing (on the very input, launches and parameter sets the GPU test uses), the binning by its properties and a scalar loop, the
hot bins' threshold by hand-made totals; and the comparison helpers by altered words they must name."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_py
from tests import prep_model as pm


def test_rk_closed_form_and_oracle_roll_agree():
    for kind in ("rand", "ff"):
        d = pm.rk_input(kind, 5003)
        first = int(oracle_py.lib().nlzm_oracle_rk_hash256(d.ctypes.data))
        closed, rolled = pm.rk_closed(d), pm.rk_rolled(d, first)
        assert closed.size == 5003 - 255 and int(closed[0]) == first
        assert not pm.compare("rk model", kind, "closed form against the roll", closed, rolled)
    assert len(set(pm.rk_closed(pm.rk_input("rand", 5003)).tolist())) > 4000         # (not a constant)
    assert pm.rk_closed(np.zeros(255, np.uint8)).size == 0 and pm.rk_closed(np.zeros(256, np.uint8)).size == 1
    # the expected table of a probe call: nothing outside [pos0, min(pos1, n - 255)) is written
    d = pm.rk_input("rand", 1281)
    want = pm.rk_expected(d, 1023, 1023 + 40)
    assert (want[:3] == pm.rk_closed(d)[1023:1026]).all() and (want[3:] == pm.SENTINEL).all()


@pytest.fixture(scope="module")
def pf():
    d = pm.pf_input()
    return {"data": d, "models": {p[0]: pm.pf_model(d, pm.PF_LAUNCHES, p[4], p[1], p[3], p[2]) for p in pm.PF_PARAMS}}


def test_prefilter_launches_are_what_the_issue_asks():
    L = pm.PF_LAUNCHES
    assert len(L) == 4 and all(L[i][1] == L[i + 1][0] for i in range(3))
    assert any(a1 % 256 and a1 % 1024 for _, a1 in L[:-1]) and any(a1 - a0 == 1 for a0, a1 in L)
    assert pm.PF_N - 65 < L[-1][1] < pm.PF_N
    assert {(p[1], p[2], p[3]) for p in pm.PF_PARAMS} == {(12, 10, 0), (20, 16, 0), (20, 16, 1), (33, 16, 1)}
    d = pm.pf_input()
    runs = np.flatnonzero(np.diff(d.astype(np.int16)) != 0)
    assert np.diff(runs).max() >= 500 and (d[20_000:20_600] == 0xFF).all()


@pytest.mark.parametrize("name,t_bits,m_bits,bitmap,wmask", pm.PF_PARAMS, ids=[p[0] for p in pm.PF_PARAMS])
def test_prefilter_model_misses_no_true_mark(pf, name, t_bits, m_bits, bitmap, wmask):
    uncs, T, M = pf["models"][name]
    truth = pm.pf_truth(pf["data"], pm.PF_LAUNCHES, wmask, bitmap)
    for li, ((a0, a1), unc, must) in enumerate(zip(pm.PF_LAUNCHES, uncs, truth)):
        assert unc.size == a1 - a0 and unc[0] == 1 and set(unc.tolist()) <= {0, 1}
        if a1 - a0 > 1:
            assert must.size > 20, f"launch {li} has no true marks to miss"
        missed = must[unc[must] == 0]
        assert missed.size == 0, f"{name}: launch {li}: true marks missing at {(missed - 1 + a0)[:8].tolist()}"
        print(f"{name}: launch {li}: {int(unc.sum())} marks of {unc.size}, {must.size} of them true")
    assert (M == pm.NONE).all() and T


def test_prefilter_model_is_no_blanket(pf):
    """a model that marked everything would miss nothing either: with 2^20 slots most positions of random bytes stay unmarked, the window
    of 2^13 drops the far copies that the bitmap keeps, and the two slot functions place the same 65-grams differently"""
    d, L = pf["data"], pm.PF_LAUNCHES
    for name in ("t20_m16", "t20_m16_bitmap", "t33_m16_bitmap"):
        uncs = pf["models"][name][0]
        assert sum(int(u.sum()) for u in uncs) < 0.45 * sum(u.size for u in uncs), name
    far_w13 = pf["models"]["t12_m10_w13"][0][2][15_000 + 1 - L[2][0]: 15_000 + 200 - L[2][0]]         # the copy of 1,000 at 15,000: 14,000 back
    far_map = pf["models"]["t20_m16_bitmap"][0][2][15_000 + 1 - L[2][0]: 15_000 + 200 - L[2][0]]
    assert far_map.all() and not far_w13.all()
    T20, T33 = pf["models"]["t20_m16_bitmap"][1], pf["models"]["t33_m16_bitmap"][1]
    assert max(T20) < 1 << 15 and max(T33) < 1 << 28 and max(T33) > 1 << 24
    assert sum(bin(v).count("1") for v in T33.values()) >= sum(bin(v).count("1") for v in T20.values())
    # the table form holds 1 + the LATEST position: the run of 700 equal bytes leaves its last full 65-gram
    Tt = pf["models"]["t20_m16"][1]
    h, h2 = pm.pf_hashes(d)
    assert Tt[int(pm.pf_slot(h[12_100:12_101], h2[12_100:12_101], 20)[0])] >= 12_000 + 700 - 65 + 1


BIN_CASES = pm.bin_cases()


def test_bin_cases_are_what_the_issue_asks():
    heads = {c[8] for c in BIN_CASES}
    assert heads == {64, 1000, 8192, 30720, 36864, 36865, 61440} and {c[1] for c in BIN_CASES} == {"rand", "zeros", "alt", "text"}
    assert {c[5] for c in BIN_CASES if c[8] > 36864} == {15, 16}
    lasts = set()
    for _, _, n, cs, feed, _, c0, nc, _ in BIN_CASES:
        assert c0 > 0 and 3 <= nc <= 5 and feed > cs
        remain = n - (c0 + nc - 1) * cs
        lasts.add("lt4" if remain < 4 else "lt_chunk" if remain < cs else "lt_feed" if remain < feed else "full")
    assert {"lt4", "lt_chunk", "lt_feed"} <= lasts and {c[3] for c in BIN_CASES} == {3000, 14848}


@pytest.mark.parametrize("case", BIN_CASES, ids=[c[0] for c in BIN_CASES])
def test_bin_model_is_a_stable_partition(case):
    name, kind, n, cs, feed, shift, c0, nc, nheads = case
    d, unc = pm.bin_input(kind, n), pm.bin_unc(n, cs, c0, nc)
    off, pos, care = pm.bin_model(d, cs, feed, shift, c0, nc, nheads, unc, c0 * cs)
    for k in range(nc):
        start, n_ok = (c0 + k) * cs, pm.bin_n_ok(n, cs, feed, c0 + k)
        assert 0 <= n_ok <= cs and (start + n_ok + 3 <= n if n_ok else n - start < 4) and (n_ok in (0, cs) or start + n_ok + 3 == min(n, start + feed))
        a, w1 = pos[k, :n_ok, 0].astype(np.int64), pos[k, :n_ok, 1]
        assert (np.sort(a) == np.arange(start, start + n_ok)).all()                     # a permutation of the chunk's positions
        assert (pos[k, n_ok:] == pm.SENTINEL).all()
        assert off[k, 0] == 0 and off[k, nheads] == n_ok and (np.diff(off[k].astype(np.int64)) >= 0).all()
        b = (w1 & np.uint32(0x1FFFFFFF)) % np.uint32(nheads)
        j = np.arange(n_ok)
        assert (off[k, b] <= j).all() and (j < off[k, b + 1]).all()                      # every entry inside its bin's range
        same = b[1:] == b[:-1]
        assert (np.diff(a)[same] > 0).all() and (np.diff(b.astype(np.int64)) >= 0).all()   # ascending inside a bin, bins in order
    if kind == "zeros":
        assert (off[:, 1:] == off[:, 1:2]).all()           # one bin holds everything


def test_bin_model_words_against_a_scalar_loop():
    name, kind, n, cs, feed, shift, c0, nc, nheads = next(c for c in BIN_CASES if c[0] == "A,rand,nheads=1000")
    d, unc = pm.bin_input(kind, n), pm.bin_unc(n, cs, c0, nc)
    off, pos, care = pm.bin_model(d, cs, feed, shift, c0, nc, nheads, unc, c0 * cs)
    raw, a0 = d.tobytes(), c0 * cs
    seen = {31: set(), 30: set(), 29: set()}
    for k in range(nc):
        for a, w1, cw in zip(pos[k, :, 0].tolist(), pos[k, :, 1].tolist(), care[k, :, 1].tolist()):
            if a == pm.SENTINEL:
                continue
            hf = ((int.from_bytes(raw[a:a + 4], "little") * 987660757) & 0xFFFFFFFF) >> shift
            want = hf | (int(unc[a - a0]) << 31) | ((int(unc[a - a0 - 1]) if a > a0 else 0) << 30) | (int(unc[a - a0 + 1]) << 29)
            assert w1 == want, (a, hex(w1), hex(want))
            assert cw == (0xDFFFFFFF if a == min(n, (c0 + nc) * cs) - 1 else 0xFFFFFFFF)
            for bit in seen:
                seen[bit].add((w1 >> bit) & 1)
    assert all(v == {0, 1} for v in seen.values())
    first = int(np.flatnonzero(pos[0, :, 0] == a0)[0])
    assert not pos[0, first, 1] & 0x40000000                # the launch's first position has no position before it


def test_hot_threshold_rule_on_hand_made_totals():
    tot = np.array([1024, 2047, 1500, 10, 500, 1023, 0])
    off1 = pm.hot_offs(tot, 1, 1)
    # exactly hmax bins in the top bucket: they are the hot ones
    assert pm.hot_threshold(tot, 3, 0) == 1024 and pm.hot_model(off1, 7, 3, 0) == {0, 1, 2}
    # hmax + 1 bins in the top bucket: no power of two below 2048 leaves at most hmax, and none is hot
    assert pm.hot_threshold(tot, 2, 0) == 2048 and pm.hot_model(off1, 7, 2, 0) == set()
    # room for one more bucket
    assert pm.hot_threshold(tot, 4, 0) == 512 and pm.hot_model(off1, 7, 4, 0) == {0, 1, 2, 5}
    assert pm.hot_threshold(tot, 6, 0) == 1 and pm.hot_model(off1, 7, 6, 0) == {0, 1, 2, 3, 4, 5}          # (a bin without positions is never hot)
    # min_count inside the top bucket: the bins below it do not count against hmax, and the threshold is raised to it
    assert pm.hot_threshold(tot, 3, 1400) == 1400 and pm.hot_model(off1, 7, 3, 1400) == {1, 2}
    assert pm.hot_threshold(tot, 2, 1400) == 1400 and pm.hot_model(off1, 7, 2, 1400) == {1, 2}
    assert pm.hot_threshold(tot, 1, 1400) == 2048 and pm.hot_model(off1, 7, 1, 1400) == set()
    assert pm.hot_model(off1, 7, 3, 2048) == set() and pm.hot_model(pm.hot_offs(np.zeros(7, int), 1, 1), 7, 3, 0) == set()
    # the totals are summed over the chunks
    off5 = pm.hot_offs(tot, 5, 2)
    assert off5.shape == (5, 8) and (np.diff(off5.astype(np.int64), axis=1).sum(axis=0) == tot).all() and (off5[:-1, -1] > 0).any()
    assert pm.hot_model(off5, 7, 3, 0) == {0, 1, 2}
    # the generated cases: every kind, and the kinds do what their names say
    for nheads in (64, 1000, 30720):
        cases = pm.hot_cases(nheads, 5)
        assert len(cases) == 3 * (4 + 4 * 3)
        by = {c[0]: pm.hot_model(c[1], nheads, c[2], c[3]) for c in cases}
        for hmax in (1, 2, 480):
            k = min(hmax, nheads // 2)
            assert len(by[f"top_exact,nheads={nheads},nchunks=5,hmax={hmax},min_count=0"]) >= k
            if hmax < nheads // 2:
                assert len(by[f"top_exact,nheads={nheads},nchunks=5,hmax={hmax},min_count=0"]) == hmax
                assert by[f"top_plus1,nheads={nheads},nchunks=5,hmax={hmax},min_count=0"] == set()
                assert by[f"equal,nheads={nheads},nchunks=5,hmax={hmax},min_count=1500"] == set()
            assert by[f"equal,nheads={nheads},nchunks=5,hmax={hmax},min_count=1501"] == set()
        assert all(len(pm.hot_model(c[1], nheads, c[2], c[3])) <= c[2] for c in cases)
        assert any(0 < len(v) for kk, v in by.items() if kk.startswith("geometric"))
        assert by[f"equal,nheads={nheads},nchunks=5,hmax=480,min_count=0"] == (set(range(64)) if nheads == 64 else set())


def test_the_comparison_names_every_altered_word():
    """one altered word in each section of each kernel's answer: the comparison fails, once, and names kernel, case, section, index, got and want"""
    rng = np.random.default_rng(9)
    d = pm.pf_input()
    uncs, T, M = pm.pf_model(d, pm.PF_LAUNCHES, (1 << 20) - 1, 20, 0, 16)
    name, kind, n, cs, feed, shift, c0, nc, nheads = next(c for c in BIN_CASES if c[0] == "B,rand,nheads=1000")      # (its last position is binned)
    off, pos, care = pm.bin_model(pm.bin_input(kind, n), cs, feed, shift, c0, nc, nheads, pm.bin_unc(n, cs, c0, nc), c0 * cs)
    sections = [("rk_hash_kernel", "out", pm.rk_expected(pm.rk_input("rand", 1281), 1, 1026), None),
                ("prefilter_mark_kernel", "unc of launch 2", uncs[2], None),
                ("prefilter_insert_kernel", "T, index of the words that are not 0", np.array(sorted(T), dtype=np.uint64), None),
                ("prefilter_insert_kernel", "T, value", np.array([T[k] for k in sorted(T)], dtype=np.uint32), None),
                ("prefilter_insert_kernel", "M", M, None),
                ("bin_kernel", "off", off, None), ("bin_kernel", "pos", pos, care),
                ("gather_frames_kernel", "dst", rng.integers(0, 256, 500, dtype=np.uint8), None)]
    for kernel, section, want, cmask in sections:
        assert not pm.compare(kernel, "c", section, want.copy(), want, cmask)
        flat = want.ravel()
        for i in (0, flat.size - 1, int(rng.integers(0, flat.size))):
            got = flat.copy()
            got[i] ^= got.dtype.type(1 << int(rng.integers(0, 8)))
            msgs = pm.compare(kernel, "c", section, got.reshape(want.shape), want, cmask)
            w = 2 if got.dtype.itemsize == 1 else 8
            assert msgs == [f"{kernel}: case c, {section}[{i}]: got 0x{int(got[i]):0{w}X}, want 0x{int(flat[i]):0{w}X}"], msgs
    # bit 29 of the launch's last position is the one thing not compared; bit 29 of any other is
    last = np.flatnonzero(care.ravel() != 0xFFFFFFFF)
    assert last.size == 1
    got = pos.copy().ravel()
    got[last[0]] ^= np.uint32(0x20000000)
    assert not pm.compare("bin_kernel", "c", "pos", got, pos, care)
    got[last[0]] ^= np.uint32(0x40000000)
    assert len(pm.compare("bin_kernel", "c", "pos", got, pos, care)) == 1
    got = pos.copy().ravel()
    got[last[0] - 2] ^= np.uint32(0x20000000)
    assert len(pm.compare("bin_kernel", "c", "pos", got, pos, care)) == 1
    assert pm.compare("bin_kernel", "c", "off", off.ravel()[:-1], off)[0].endswith(f"{off.size - 1} elements, the model has {off.size}")
    # a stray store into the slack, a missing one in the body
    arr = np.concatenate([np.full(64, pm.SENTINEL, np.uint32), np.arange(10, dtype=np.uint32), np.full(64, pm.SENTINEL, np.uint32)])
    body, msgs = pm.strip_slack("rk_hash_kernel", "c", "out", arr, 64)
    assert not msgs and (body == np.arange(10)).all()
    arr[63] = 5; arr[-1] = 6
    msgs = pm.strip_slack("rk_hash_kernel", "c", "out", arr, 64)[1]
    assert len(msgs) == 2 and "out, slack in front[63]: got 0x00000005" in msgs[0] and "out, slack behind[63]: got 0x00000006" in msgs[1]
    # the hot bins: a wrong count, a bin too many, one missing, a wrong back pointer, a store behind the list
    want, hmax = {3, 9, 11}, 4
    lst = np.array([3, 11, 9, 3, pm.SENTINEL], dtype=np.uint32)
    hob = np.zeros(16, np.uint32)
    hob[[11, 9, 3]] = [1, 2, 3]
    assert not pm.hot_check("c", want, hmax, hob, lst, 3)
    assert any("counter hot_bins: grew by 2" in m for m in pm.hot_check("c", want, hmax, hob, lst, 2))
    bad = lst.copy(); bad[0] = 2
    assert any(m.startswith("hot_select_kernel: case c, hot_list[0]: got 2, want 3") for m in pm.hot_check("c", want, hmax, hob, bad, 3))
    bad = lst.copy(); bad[2] = 10
    msgs = pm.hot_check("c", want, hmax, hob, bad, 3)
    assert any("missing [9], not wanted [10]" in m for m in msgs)
    bad = hob.copy(); bad[9] = 3
    assert pm.hot_check("c", want, hmax, bad, lst, 3) == ["hot_select_kernel: case c, hot_of_bin[9]: got 0x00000003, want 0x00000002"]
    bad = lst.copy(); bad[4] = 7
    assert len(pm.hot_check("c", want, hmax, hob, bad, 3)) == 1
    assert pm.hot_check("c", set(), hmax, np.zeros(16, np.uint32), np.array([0] + [pm.SENTINEL] * 4, dtype=np.uint32), 0) == []
