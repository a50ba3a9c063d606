"""GPU suite (-m gpu): the compress path's pre-pass and gather kernels, each launched alone through the probe library (tests/prep_probe: no
kernel of its own, it calls the product's launch wrappers) and held to tests/prep_model.py, which tests/test_prep_model.py holds on the CPU:
rk_hash_kernel word for word, every unc byte of every pre-filter launch with the final T and M (and no true mark of the brute-force truth
missing), bin_kernel's offsets and both words of every entry on both of its paths, hot_select_kernel's list as a set with its back
pointers and counter, gather_frames_kernel's bytes.  Whole-stream parity cannot see these: a wrong mark, hot list or assumption bit costs
speed and no byte.  Every output array comes back with sentinel slack around it, and a mismatch names kernel, case, index, got and want.
Nothing here can wait for a workgroup; sizes that do not fit are refused by the probe before it launches."""
import ctypes as C
import os

import numpy as np
import pytest
import torch        # (before the libraries are loaded, as bench.py has it: all then share one HIP runtime)

import nlzm_amd
from tests import prep_model as pm

pytestmark = pytest.mark.gpu

PROBE_PATH = os.path.join(os.path.dirname(nlzm_amd.LIB_PATH), "libprep_probe.so")
U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def probe(gpu):
    assert os.path.exists(PROBE_PATH), f"{PROBE_PATH} is missing: build() makes it beside the library"
    lib = C.CDLL(PROBE_PATH)
    p, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.prep_probe_slack.restype = u64
    lib.prep_probe_rk_hash.argtypes = [p, u64, u64, u64, p, u64]
    lib.prep_probe_prefilter.argtypes = [p, u64, p, u32, u32, u32, u32, u32, p, u64, p, p, p, p, u64, p]
    lib.prep_probe_bin.argtypes = [p, u64, u32, u32, u32, u32, u32, u32, p, u64, u32, p, u64, p, u64]
    lib.prep_probe_hot_select.argtypes = [p, u32, u32, u32, u32, p, u64, p, u64, p, p]
    lib.prep_probe_gather.argtypes = [p, u64, p, p, u32, p, u64]
    lib.slack = int(lib.prep_probe_slack())
    assert lib.slack == 64
    return lib


# ---- rk_hash_kernel -----------------------------------------------------------------------------------------------------------------
def run_rk(lib, data, pos0, pos1, short=0):
    out = np.zeros(pos1 - pos0 + 2 * lib.slack - short, U32)
    rc = lib.prep_probe_rk_hash(data.ctypes.data, data.size, pos0, pos1, out.ctypes.data, out.size)
    return rc, out


def test_rk_hash_every_word_and_nothing_else(probe):
    """one window, the tile's edge at 1,279 / 1,280 / 1,281 bytes, the host's pos0 = a0 - 1024 and odd ones, 1 / 1,023 / 1,024 / 1,025 positions and
    counts that are no multiple of 1,024, pos1 at the last window and beyond it, sums that wrap (all 0xFF): every word is the model's, and
    nothing outside [pos0, min(pos1, n - 255)) is written"""
    msgs, cases = [], pm.rk_cases()
    for name, kind, n, pos0, pos1 in cases:
        data = pm.rk_input(kind, n)
        rc, out = run_rk(probe, data, pos0, pos1)
        assert rc == 0, (name, rc)
        body, m = pm.strip_slack("rk_hash_kernel", name, "out", out, probe.slack)
        msgs += m + pm.compare("rk_hash_kernel", name, "out", body, pm.rk_expected(data, pos0, pos1))
    print(f"rk_hash_kernel: {len(cases)} calls")
    assert not msgs, "\n".join(msgs[:40])


# ---- the pre-filter -----------------------------------------------------------------------------------------------------------------
def run_prefilter(lib, data, launches, wmask, t_bits, bitmap, m_bits, t_cap=1 << 17, unc_short=0):
    L = np.array(launches, dtype=U32)
    unc = np.zeros(sum(a1 - a0 + 2 * lib.slack for a0, a1 in launches) - unc_short, np.uint8)
    m_live, m_out = np.full(len(launches), 77, U32), np.zeros(1 << m_bits, U32)
    t_idx, t_val, t_count = np.zeros(t_cap, U64), np.zeros(t_cap, U32), C.c_uint64(0)
    rc = lib.prep_probe_prefilter(data.ctypes.data, data.size, L.ctypes.data, len(launches), wmask, t_bits, bitmap, m_bits, unc.ctypes.data, unc.size,
                                  m_live.ctypes.data, m_out.ctypes.data, t_idx.ctypes.data, t_val.ctypes.data, t_cap, C.byref(t_count))
    return rc, unc, m_live, m_out, t_idx, t_val, int(t_count.value)


@pytest.fixture(scope="module")
def pf_data():
    return pm.pf_input()


@pytest.mark.parametrize("name,t_bits,m_bits,bitmap,wmask", pm.PF_PARAMS, ids=[p[0] for p in pm.PF_PARAMS])
def test_prefilter_marks_tables_and_truth(probe, pf_data, name, t_bits, m_bits, bitmap, wmask):
    """four launches on one T and M (uneven boundaries, one of a single position, the last ending inside the input's last 65 bytes): every unc
    byte of every launch, M empty after every launch, the final T -- and then the marks against the truth that knows no hashing"""
    launches = pm.PF_LAUNCHES
    rc, unc, m_live, m_out, t_idx, t_val, t_count = run_prefilter(probe, pf_data, launches, wmask, t_bits, bitmap, m_bits)
    assert rc == 0, rc
    want_unc, want_T, want_M = pm.pf_model(pf_data, launches, wmask, t_bits, bitmap, m_bits)
    truth = pm.pf_truth(pf_data, launches, wmask, bitmap)
    msgs, at = [], 0
    for li, (a0, a1) in enumerate(launches):
        ln = a1 - a0 + 2 * probe.slack
        body, m = pm.strip_slack("prefilter_mark_kernel", name, f"unc of launch {li}", unc[at:at + ln], probe.slack)
        at += ln
        msgs += m + pm.compare("prefilter_hash_kernel / prefilter_mark_kernel", name, f"unc of launch {li} [{a0}, {a1})", body, want_unc[li])
        missed = truth[li][body[truth[li]] != 1]
        msgs += [f"prefilter_hash_kernel / prefilter_mark_kernel: case {name}, launch {li}: the true mark of position {int(i) - 1 + a0} is missing (unc[{int(i)}])"
                 for i in missed[:8]]
        print(f"{name}: launch {li}: {int((body == 1).sum())} marks of {body.size}, {truth[li].size} of them true")
        if int(m_live[li]):
            msgs.append(f"prefilter_insert_kernel: case {name}, launch {li}: {int(m_live[li])} entries of M are not kNone after the launch, want 0")
    msgs += pm.compare("prefilter_insert_kernel", name, "M", m_out, want_M)
    keys = sorted(want_T)
    assert t_count <= t_idx.size
    msgs += pm.compare("prefilter_insert_kernel", name, "T, index of the words that are not 0", t_idx[:t_count], np.array(keys, dtype=U64))
    if t_count == len(keys):
        msgs += pm.compare("prefilter_insert_kernel", name, "T, value of the words that are not 0", t_val[:t_count], np.array([want_T[k] for k in keys], dtype=U32))
    assert not msgs, "\n".join(msgs[:40])


# ---- bin_kernel ---------------------------------------------------------------------------------------------------------------------
def run_bin(lib, data, cs, feed, shift, c0, nc, nheads, unc, batch_a0, short=0):
    off = np.zeros(nc * (nheads + 1) + 2 * lib.slack - short, U32)
    pos = np.zeros(nc * cs * 2 + 2 * lib.slack, U32)
    rc = lib.prep_probe_bin(data.ctypes.data, data.size, cs, feed, shift, c0, nc, nheads, unc.ctypes.data, unc.size, batch_a0,
                            off.ctypes.data, off.size, pos.ctypes.data, pos.size)
    return rc, off, pos


BIN_CASES = pm.bin_cases()


@pytest.mark.parametrize("kind", ("rand", "zeros", "alt", "text"))
def test_bin_offsets_and_both_words_of_every_entry(probe, kind):
    """chunks that are no multiple of 1,024 (and the host's 14,848), feed > chunk_size, c0 > 0, a last chunk with fewer than four bytes, with less than
    a chunk and with less than a feed; 64 to 61,440 bins: the modulus, the product's 30,720, the last count with cursors in LDS and the path
    with cursors in HBM; every position in ONE bin (zeros: a wave's lanes rank among themselves, the sixteen waves queue); a random unc, so that
    bits 31, 30 and 29 all take both values (bit 30 of the launch's first position is 0; bit 29 of its last is not compared)"""
    msgs, ran = [], 0
    for name, k, n, cs, feed, shift, c0, nc, nheads in BIN_CASES:
        if k != kind:
            continue
        data, unc = pm.bin_input(kind, n), pm.bin_unc(n, cs, c0, nc)
        rc, off, pos = run_bin(probe, data, cs, feed, shift, c0, nc, nheads, unc, c0 * cs)
        assert rc == 0, (name, rc)
        want_off, want_pos, care = pm.bin_model(data, cs, feed, shift, c0, nc, nheads, unc, c0 * cs)
        off, m1 = pm.strip_slack("bin_kernel", name, "off", off, probe.slack)
        pos, m2 = pm.strip_slack("bin_kernel", name, "pos", pos, probe.slack)
        msgs += m1 + m2 + pm.compare("bin_kernel", name, "off[chunk][bin]", off, want_off)
        msgs += pm.compare("bin_kernel", name, "pos[chunk][entry][word]", pos, want_pos, care)
        ran += 1
    print(f"bin_kernel, {kind}: {ran} launches")
    assert ran >= 7 and not msgs, "\n".join(msgs[:40])


# ---- hot_select_kernel --------------------------------------------------------------------------------------------------------------
def run_hot(lib, off, nchunks, nheads, hmax, min_count, counter0=0, short=0):
    off = np.ascontiguousarray(off, dtype=U32)
    hob = np.zeros(nheads + 2 * lib.slack, U32)
    lst = np.zeros(1 + hmax + 2 * lib.slack - short, U32)
    counter, other = C.c_uint64(counter0), C.c_uint32(99)
    rc = lib.prep_probe_hot_select(off.ctypes.data, nchunks, nheads, hmax, min_count, hob.ctypes.data, hob.size, lst.ctypes.data, lst.size,
                                   C.byref(counter), C.byref(other))
    return rc, hob, lst, int(counter.value) - counter0, int(other.value)


@pytest.mark.parametrize("nheads,nchunks", [(64, 1), (64, 5), (1000, 1), (1000, 5), (30720, 1), (30720, 5)])
def test_hot_select_against_the_model(probe, nheads, nchunks):
    """totals all zero, all equal (one bucket holds more than hmax: none is hot), exactly hmax and hmax + 1 bins in the top bucket, a geometric
    spread; min_count 0, inside a bucket and above every total; hmax 1, 2 and 480.  The list is a set (its order is the hardware's)."""
    msgs, cases = [], pm.hot_cases(nheads, nchunks)
    for i, (name, off, hmax, mc) in enumerate(cases):
        c0 = (1 << 40) + i
        rc, hob, lst, grew, other = run_hot(probe, off, nchunks, nheads, hmax, mc, counter0=c0)
        assert rc == 0, (name, rc)
        hob, m1 = pm.strip_slack("hot_select_kernel", name, "hot_of_bin", hob, probe.slack)
        lst, m2 = pm.strip_slack("hot_select_kernel", name, "hot_list", lst, probe.slack)
        msgs += m1 + m2 + pm.hot_check(name, pm.hot_model(off, nheads, hmax, mc), hmax, hob, lst, grew)
        if other:
            msgs.append(f"hot_select_kernel: case {name}: {other} other words of the counters were written")
    print(f"hot_select_kernel, {nheads} bins in {nchunks} chunks: {len(cases)} launches")
    assert not msgs, "\n".join(msgs[:40])


# ---- gather_frames_kernel -----------------------------------------------------------------------------------------------------------
def run_gather(lib, frames, stride, dst_off, out_len, body):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    d, l = np.array(dst_off, dtype=U64), np.array(out_len, dtype=U32)
    dst = np.zeros(body + 2 * lib.slack, np.uint8)
    rc = lib.prep_probe_gather(frames.ctypes.data, stride, d.ctypes.data, l.ctypes.data, len(out_len), dst.ctypes.data, dst.size)
    return rc, dst


def test_gather_frames_bytes_gaps_and_slack(probe):
    """five frames of 0, 1, 255, 256 and 1,000 bytes to unaligned offsets with gaps between them, out of order: the bytes arrive, the gaps and the
    slack keep the sentinel"""
    lens, offs, stride, body = [0, 1, 255, 256, 1000], [5, 3, 1301, 1013, 11], 1003, 1600
    rng = np.random.default_rng(41)
    frames = rng.integers(0, 256, 5 * stride, dtype=np.uint8)
    rc, dst = run_gather(probe, frames, stride, offs, lens, body)
    assert rc == 0, rc
    want = np.full(body, pm.SENTINEL8, np.uint8)
    for f, (o, l) in enumerate(zip(offs, lens)):
        want[o:o + l] = frames[f * stride:f * stride + l]
    assert (want == pm.SENTINEL8).sum() >= body - sum(lens)
    got, msgs = pm.strip_slack("gather_frames_kernel", "five frames", "dst", dst, probe.slack)
    msgs += pm.compare("gather_frames_kernel", "five frames", "dst", got, want)
    assert not msgs, "\n".join(msgs)


# ---- what does not fit is refused, and nothing is launched ------------------------------------------------------------------------------
def test_sizes_that_do_not_fit_are_refused(probe):
    d = pm.rk_input("rand", 1281)
    assert run_rk(probe, d, 0, 100, short=1)[0] == -1 and run_rk(probe, d, 100, 100)[0] == -1
    pf = pm.pf_input()
    assert run_prefilter(probe, pf, ((0, 100), (100, 300)), 255, 12, 0, 10, unc_short=1)[0] == -1
    assert run_prefilter(probe, pf, ((0, 100), (50, 300)), 255, 12, 0, 10)[0] == -1             # launches that overlap
    assert run_prefilter(probe, pf, ((0, pf.size + 1),), 255, 12, 0, 10)[0] == -1               # a launch beyond the input
    assert run_prefilter(probe, pf, ((0, 100),), 255, 33, 0, 10)[0] == -1                       # 2^33 words
    assert run_prefilter(probe, pf, ((0, 100),), 255, 12, 0, 0)[0] == -1
    name, kind, n, cs, feed, shift, c0, nc, nheads = BIN_CASES[0]
    data, unc = pm.bin_input(kind, n), pm.bin_unc(n, cs, c0, nc)
    assert run_bin(probe, data, cs, feed, shift, c0, nc, nheads, unc, c0 * cs, short=1)[0] == -1
    assert run_bin(probe, data, cs, feed, shift, c0, nc + 1, nheads, np.zeros(2 * n, np.uint8), c0 * cs)[0] == -1     # a chunk that begins behind the input
    assert run_bin(probe, data, cs, feed, shift, c0, nc, nheads, unc[:-1], c0 * cs)[0] == -1                       # unc without the one behind
    assert run_bin(probe, data, cs, feed, shift, c0, nc, nheads, unc, c0 * cs + 1)[0] == -1
    assert run_bin(probe, data, cs, cs - 1, shift, c0, nc, nheads, unc, c0 * cs)[0] == -1
    off = pm.hot_offs(np.arange(64), 2, 1)
    assert run_hot(probe, off, 2, 64, 4, 0, short=1)[0] == -1 and run_hot(probe, off, 0, 64, 4, 0)[0] == -1
    fr = np.zeros(2 * 100, np.uint8)
    assert run_gather(probe, fr, 100, [0, 450], [100, 51], 500)[0] == -1                        # a frame that ends behind the body
    assert run_gather(probe, fr, 100, [0, 100], [100, 101], 500)[0] == -1                       # a frame longer than the stride
    assert run_gather(probe, fr, 100, [0, 450], [100, 50], 500)[0] == 0
