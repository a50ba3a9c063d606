"""The model the compress path's pre-pass and gather kernels are held to: RK256, the pre-filter's marks and tables, the
binning by BT4 head and the choice of hot bins, in plain numpy uint32 / uint64 arithmetic, written from the definitions in the comments of
nlzm_kernels.hip and the reference lines they cite (NLZM.cpp:739, :793-799, :1514-1518) -- not from the kernels' bodies.  It stands beside the hand-made
restatements in tests/host_sim/sim2.cpp (SimPrefilter, the rolled RK hash, SimWorkers' lazy bins), which are held by whole-stream parity only.

tests/test_prep_model.py holds the model on the CPU (two forms of RK256 against each other and the oracle, the marks against a brute-force
truth without hashing, the binning as a property); tests/test_gpu_prep.py then holds the device to the model, through tests/prep_probe.
The inputs and cases of both live here, so that what the CPU tests vouch for is what the GPU tests use.  TEST CODE ONLY."""
import numpy as np

from nlzm_amd import corpus

U32, U64 = np.uint32, np.uint64
NONE = 0xFFFFFFFF
SENTINEL = 0xA5A5A5A5           # what the probe fills every output word with (0xA5 in every byte)
SENTINEL8 = 0xA5

RK_ADDH = 0x2F0FD693            # NLZM.cpp:793
RK_REMH = 0x0E4EA401            # :796, ADDH^256
PF_LEN = 65
PF_MUL, PF_MUL2, PF_MUL64 = 0x9E3779B1, 0x85EBCA77, 0x9E3779B97F4A7C15
HASH4_MUL = 987660757           # :739


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison: one message per mismatch, naming kernel, case, section, index, got and want
# ---------------------------------------------------------------------------------------------------------------------------------
def compare(kernel, case, section, got, want, care=None, limit=8):
    """got against want, element for element (under the bit mask `care` where given)"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    if got.shape != want.shape:
        return [f"{kernel}: case {case}, {section}: {got.size} elements, the model has {want.size}"]
    diff = got.astype(U64) ^ want.astype(U64)
    if care is not None:
        diff &= np.asarray(care).ravel().astype(U64)
    bad = np.flatnonzero(diff)
    w = 2 if got.dtype.itemsize == 1 else 8
    return [f"{kernel}: case {case}, {section}[{int(i)}]: got 0x{int(got[i]):0{w}X}, want 0x{int(want[i]):0{w}X}" for i in bad[:limit]] + \
           ([f"{kernel}: case {case}, {section}: ... and {bad.size - limit} more"] if bad.size > limit else [])


def strip_slack(kernel, case, section, arr, slack):
    """-> (the body of slack + body + slack, messages for every slack element that is not the sentinel any more)"""
    arr = np.asarray(arr)
    sent = SENTINEL8 if arr.dtype.itemsize == 1 else SENTINEL
    front, body, back = arr[:slack], arr[slack:arr.size - slack], arr[arr.size - slack:]
    msgs = compare(kernel, case, section + ", slack in front", front, np.full(front.size, sent, arr.dtype))
    msgs += compare(kernel, case, section + ", slack behind", back, np.full(back.size, sent, arr.dtype))
    return body, msgs


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def make_input(n, seed, copies=(), run=None, ff=None, text=None):
    """seeded random bytes; text = (at, length): a slice of corpus.syn_text; run = (at, length, byte); ff = (at, length) of 0xFF;
    copies = (src, dst, length), planted last and in order"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    if text:
        d[text[0]:text[0] + text[1]] = corpus.syn_text(text[1] + 1000)[1000:]
    if run:
        d[run[0]:run[0] + run[1]] = run[2]
    if ff:
        d[ff[0]:ff[0] + ff[1]] = 0xFF
    for s, t, l in copies:
        d[t:t + l] = d[s:s + l].copy()
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# RK256: rkhash[a] = sum_{j<256} in[a+j] * ADDH^(256-j) mod 2^32, for every a with a + 256 <= n
# ---------------------------------------------------------------------------------------------------------------------------------
def _windows(data, k):
    return np.lib.stride_tricks.sliding_window_view(np.asarray(data, dtype=np.uint8), k)


def rk_closed(data):
    """the closed form, as a product of the windows with the powers (a byte times a power is below 2^40, 256 of them below 2^48)"""
    data = np.asarray(data, dtype=np.uint8)
    if data.size < 256:
        return np.zeros(0, U32)
    pw = np.array([pow(RK_ADDH, 256 - j, 1 << 32) for j in range(256)], dtype=U64)
    return (_windows(data, 256).astype(U64) @ pw & U64(0xFFFFFFFF)).astype(U32)


def rk_rolled(data, first):
    """`first` (the oracle's nlzm_oracle_rk_hash256 of the first window), then rolling_hash_add_remove (NLZM.cpp:799) from window to window"""
    data = np.asarray(data, dtype=np.uint8)
    m = data.size - 255
    out = np.zeros(max(m, 0), U32)
    if m <= 0:
        return out
    h = int(first)
    out[0] = h
    b = data.tolist()
    for a in range(1, m):
        h = ((b[a + 255] + h - b[a - 1] * RK_REMH) * RK_ADDH) & 0xFFFFFFFF
        out[a] = h
    return out


def rk_cases():
    """(name, input, n, pos0, pos1): the tile's edge (a block takes 1,024 positions and stages 1,280 bytes), one window, the host's
    pos0 = a0 - 1024 and odd ones, lengths around 1,024, pos1 at and beyond the last window"""
    out = []
    for n in (256, 257, 1279, 1280, 1281, 5003):
        for pos0 in (0, 1, 1023, 1024, 1025):
            ends = {pos0 + 1, pos0 + 1023, pos0 + 1024, pos0 + 1025, pos0 + 1500, n - 255, n - 254, n + 40}
            for pos1 in sorted(e for e in ends if e > pos0):
                out.append((f"n={n},pos0={pos0},pos1={pos1}", "rand", n, pos0, pos1))
    for n, pos0, pos1 in ((256, 0, 1), (1281, 0, 1026), (5003, 1, 5003 - 255), (5003, 1025, 3000)):
        out.append((f"ff,n={n},pos0={pos0},pos1={pos1}", "ff", n, pos0, pos1))
    return out


def rk_input(kind, n):
    if kind == "ff":
        return np.full(n, 0xFF, np.uint8)
    return make_input(5003, 11, copies=((10, 2000, 300),), run=(700, 520, 0x5A), ff=(3000, 300))[:n].copy()


def rk_expected(data, pos0, pos1):
    """the probe's body: word i belongs to position pos0 + i; nothing outside [pos0, min(pos1, n - 255)) is written"""
    want = np.full(pos1 - pos0, SENTINEL, U32)
    h = rk_closed(data)
    hi = min(pos1, data.size - 255)
    if hi > pos0:
        want[:hi - pos0] = h[pos0:hi]
    return want


# ---------------------------------------------------------------------------------------------------------------------------------
# pre-filter
# ---------------------------------------------------------------------------------------------------------------------------------
def pf_hashes(data):
    """for every a with a + 65 <= n: h, the RK-style hash of the 65 bytes, and h2, the second hash beside it"""
    w = _windows(data, PF_LEN)
    h, h2 = np.zeros(w.shape[0], U32), np.zeros(w.shape[0], U32)
    for j in range(PF_LEN):
        b = w[:, j].astype(U32)
        h = (h + b) * U32(RK_ADDH)
        h2 = (h2 ^ b) * U32(0x01000193) + U32(0x7F4A7C15)
    return h, h2


def pf_slot(h, h2, t_bits):
    """the slot of a 65-gram in T: from its 32-bit hash up to 2^32 slots, from both hashes as one 64-bit word beyond that"""
    if t_bits <= 32:
        return ((h * U32(PF_MUL)) >> U32(32 - t_bits)).astype(U64)
    return (((h2.astype(U64) << U64(32)) | h.astype(U64)) * U64(PF_MUL64)) >> U64(64 - t_bits)


def pf_mslot(h, m_bits):
    return (h * U32(PF_MUL2)) >> U32(32 - m_bits)


def pf_model(data, launches, wmask, t_bits, t_bitmap, m_bits):
    """-> (unc of every launch, T as {word index: value} of the words that are not 0, M after the last launch).
    T[slot] is 1 + the latest position of an EARLIER launch whose 65-gram hashes there (bitmap form: one bit, "some earlier position does", and
    no window test); M[slot2] the earliest position of THIS launch hashing there.  C(x) = T says "an earlier one inside the window" or M names
    a position in front of x; unc[0] = 1, unc[x + 1] = C(x); then the launch's positions enter T and M is empty again."""
    data = np.asarray(data, dtype=np.uint8)
    n = data.size
    h, h2 = pf_hashes(data)
    slot, mslot = pf_slot(h, h2, t_bits).tolist(), pf_mslot(h, m_bits)
    nok = h.size                                    # positions 0 .. nok-1 have 65 bytes
    T = {}
    M = np.full(1 << m_bits, NONE, U32)
    uncs = []
    for a0, a1 in launches:
        e = min(a1, nok)
        pos = np.arange(a0, max(e, a0), dtype=U32)
        C = np.zeros(a1 - a0, np.uint8)
        if pos.size:
            ms = mslot[a0:e]
            np.minimum.at(M, ms, pos)
            if t_bitmap:
                c1 = np.array([s in T for s in slot[a0:e]], dtype=bool)
            else:
                c1 = np.array([s in T and a - (T[s] - 1) <= wmask for a, s in zip(range(a0, e), slot[a0:e])], dtype=bool)
            C[:e - a0] = c1 | (M[ms] < pos)
        unc = np.zeros(a1 - a0, np.uint8)
        unc[0] = 1
        unc[1:] = C[:-1]
        uncs.append(unc)
        for a in range(a0, e):
            T[slot[a]] = 1 if t_bitmap else a + 1       # (ascending: the latest stays)
        M[:] = NONE
    if t_bitmap:
        words = {}
        for s in T:
            words[s >> 5] = words.get(s >> 5, 0) | (1 << (s & 31))
        T = words
    return uncs, T, M


def pf_truth(data, launches, wmask, t_bitmap):
    """brute force, no hashing: per launch the positions x (x + 1 still in the launch) that MUST be marked -- an earlier y with the same 65 bytes
    and, in table form, x - y <= wmask (the latest earlier one decides).  -> per launch, the indexes into unc (x + 1 - a0) that must be 1"""
    data = np.asarray(data, dtype=np.uint8)
    raw, n = data.tobytes(), data.size
    last, must = {}, np.zeros(n, bool)
    for x in range(n - PF_LEN + 1):
        g = raw[x:x + PF_LEN]
        y = last.get(g)
        if y is not None and (t_bitmap or x - y <= wmask):
            must[x] = True
        last[g] = x
    return [np.flatnonzero(must[a0:a1 - 1]) + 1 for a0, a1 in launches]


PF_N = 40_000
# four launches with uneven boundaries: 9,973 is no multiple of 256, the second launch is ONE position, the last ends inside the input's last 65 bytes
PF_LAUNCHES = ((0, 9_973), (9_973, 9_974), (9_974, 25_600), (25_600, PF_N - 30))
# (name, t_bits, m_bits, bitmap, wmask): heavy collisions and a window shorter than the input; the usual sizes in both forms; the 64-bit slot
PF_PARAMS = (("t12_m10_w13", 12, 10, 0, (1 << 13) - 1), ("t20_m16", 20, 16, 0, (1 << 20) - 1), ("t20_m16_bitmap", 20, 16, 1, (1 << 20) - 1),
             ("t33_m16_bitmap", 33, 16, 1, (1 << 28) - 1))


def pf_input():
    """random bytes with a slice of text, a run of 700 of one byte, 600 of 0xFF, and copies of 60 .. 400 bytes: near and far (beyond 2^13), inside a
    launch (M) and across launches (T), one over the single-position launch, one into the last 65 bytes, one of 60 bytes (too short to count)"""
    return make_input(PF_N, 7, text=(3_000, 6_000), run=(12_000, 700, 0x41), ff=(20_000, 600),
                      copies=((100, 1_500, 400), (200, 9_800, 130), (9_500, 9_960, 100), (1_000, 15_000, 300), (22_000, 26_000, 200),
                              (30_000, 30_070, 66), (5_000, 39_000, 400), (38_000, 39_800, 200), (600, 700, 60), (16_000, 16_100, 65)))


# ---------------------------------------------------------------------------------------------------------------------------------
# binning
# ---------------------------------------------------------------------------------------------------------------------------------
def hash4_of(data):
    """hash4 (NLZM.cpp:739) of the four bytes at every position that has four"""
    d = np.asarray(data, dtype=np.uint8).astype(U32)
    x = d[:-3] | (d[1:-2] << U32(8)) | (d[2:-1] << U32(16)) | (d[3:] << U32(24))
    return x * U32(HASH4_MUL)


def bin_n_ok(n, chunk_size, feed, ci):
    """positions of chunk ci that are binned: the chunk reads min(feed, what remains) bytes, owns the first chunk_size of them, and a position
    needs four bytes inside what the chunk reads (:1515)"""
    read = min(feed, n - ci * chunk_size)
    return max(0, min(chunk_size, read - 3))


def bin_model(data, chunk_size, feed, bt_shift, c0, nchunks, nheads, unc, batch_a0):
    """-> (off[nchunks][nheads + 1], pos[nchunks][chunk_size][2] with the sentinel where nothing is written, care: the bits of pos compared).
    Word 0 is the position, word 1 its head before the modulus with the marks of the position itself, the one before (never for the launch's
    first) and the one behind in bits 31, 30, 29; bit 29 of the launch's last position is an assumption and is not compared."""
    data = np.asarray(data, dtype=np.uint8)
    n = data.size
    h4 = hash4_of(data)
    unc = np.asarray(unc, dtype=np.uint8).astype(bool)
    off = np.zeros((nchunks, nheads + 1), U32)
    pos = np.full((nchunks, chunk_size, 2), SENTINEL, U32)
    care = np.full((nchunks, chunk_size, 2), 0xFFFFFFFF, U32)
    a_last = min(n, (c0 + nchunks) * chunk_size) - 1
    for k in range(nchunks):
        start = (c0 + k) * chunk_size
        n_ok = bin_n_ok(n, chunk_size, feed, c0 + k)
        a = np.arange(start, start + n_ok)
        hfull = h4[start:start + n_ok] >> U32(bt_shift)
        b = hfull % U32(nheads)
        order = np.argsort(b, kind="stable")
        off[k, 1:] = np.cumsum(np.bincount(b, minlength=nheads))
        i = a - batch_a0
        before = np.where(a > batch_a0, unc[np.maximum(i - 1, 0)], False)
        w1 = hfull | (unc[i].astype(U32) << U32(31)) | (before.astype(U32) << U32(30)) | (unc[i + 1].astype(U32) << U32(29))
        pos[k, :n_ok, 0] = a[order]
        pos[k, :n_ok, 1] = w1[order]
        care[k, :n_ok, 1][a[order] == a_last] = 0xDFFFFFFF
    return off, pos, care


def bin_input(kind, n):
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "alt":
        return np.resize(np.frombuffer(b"ABCDwxyz", dtype=np.uint8), n).copy()
    if kind == "text":
        return corpus.syn_text(n)
    return np.random.default_rng(23).integers(0, 256, n, dtype=np.uint8)


def bin_cases():
    """(name, input, n, chunk_size, feed, bt_shift, c0, nchunks, nheads).  Geometries: a chunk size that is no multiple of 1,024 with feed > chunk_size,
    c0 > 0 and a last chunk with (A) less than a chunk, (B) more than a chunk and less than a feed, (C) fewer than four bytes left; (D) the host's
    chunk of 14,848.  Bins: below 1,024, the product's 30,720, the last count whose cursors are in LDS (36,864), and the path with cursors in HBM."""
    geos = {"A": (5 * 3000 + 1234, 3000, 3500, 2, 4), "B": (3 * 3000 + 3200, 3000, 3500, 1, 3), "C": (3 * 3000 + 2, 3000, 3500, 1, 3),
            "D": (4 * 14848 - 5000, 14848, 16384, 1, 3)}
    shift = {61440: 15}
    out = []
    for kind in ("rand", "zeros", "alt", "text"):
        for nheads in (64, 1000, 8192, 30720, 36864, 36865, 61440):
            n, cs, feed, c0, nc = geos["A"]
            out.append((f"A,{kind},nheads={nheads}", kind, n, cs, feed, shift.get(nheads, 16), c0, nc, nheads))
    for g in "BCD":
        for kind in ("rand", "zeros"):
            for nheads in (1000, 30720, 61440):
                n, cs, feed, c0, nc = geos[g]
                out.append((f"{g},{kind},nheads={nheads}", kind, n, cs, feed, shift.get(nheads, 16), c0, nc, nheads))
    return out


def bin_unc(n, chunk_size, c0, nchunks):
    """a seeded random mask for the launch's positions and one behind them: bits 31, 30 and 29 all take both values"""
    cnt = min(n, (c0 + nchunks) * chunk_size) - c0 * chunk_size
    return np.random.default_rng(31 + cnt).integers(0, 2, cnt + 1, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# hot bins
# ---------------------------------------------------------------------------------------------------------------------------------
def hot_threshold(tot, hmax, min_count):
    """the smallest power of two that leaves at most hmax bins at or above it, among the bins with at least min_count positions (and one), raised
    to min_count where that is larger; None when no power of two does (then no bin is hot)"""
    tot = np.asarray(tot, dtype=np.int64)
    elig = tot[(tot >= max(min_count, 1))]
    for k in range(32):
        if np.count_nonzero(elig >= (1 << k)) <= hmax:
            return max(1 << k, min_count)
    return None


def hot_model(off, nheads, hmax, min_count):
    """off[nchunks][nheads + 1] -> the SET of hot bins"""
    off = np.asarray(off, dtype=np.int64).reshape(-1, nheads + 1)
    tot = np.diff(off, axis=1).sum(axis=0)
    thr = hot_threshold(tot, hmax, min_count)
    return set() if thr is None else set(np.flatnonzero(tot >= thr).tolist())


def hot_check(case, want, hmax, hot_of_bin, hot_list, grew):
    """the device's answer against the model's set: the list's order is the hardware's (an atomicAdd hands out the places), so the list is
    compared as a set, hot_of_bin[b] must be 1 + b's index in THAT list and 0 elsewhere, hot_list[0] the count and what the counter grew by;
    behind the list the sentinel stays"""
    k, name = "hot_select_kernel", f"case {case}"
    hot_of_bin, hot_list = np.asarray(hot_of_bin, dtype=U32), np.asarray(hot_list, dtype=U32)
    msgs = []
    cnt = int(hot_list[0])
    if cnt != len(want):
        msgs.append(f"{k}: {name}, hot_list[0]: got {cnt}, want {len(want)}")
    if grew != len(want):
        msgs.append(f"{k}: {name}, counter hot_bins: grew by {grew}, want {len(want)}")
    cnt = min(cnt, hmax)
    got = hot_list[1:1 + cnt].tolist()
    if set(got) != want or len(set(got)) != len(got):
        miss, extra = sorted(want - set(got)), sorted(set(got) - want)
        msgs.append(f"{k}: {name}, hot_list as a set: got {len(got)} entries, missing {miss[:6]}, not wanted {extra[:6]}, want {len(want)} bins")
    msgs += compare(k, case, "hot_list behind the list", hot_list[1 + cnt:], np.full(hot_list.size - 1 - cnt, SENTINEL, U32))
    hob = np.zeros(hot_of_bin.size, U32)
    ok = [(i, b) for i, b in enumerate(got) if b < hob.size]
    if ok:
        hob[[b for _, b in ok]] = [i + 1 for i, _ in ok]
    msgs += compare(k, case, "hot_of_bin", hot_of_bin, hob)
    return msgs


def hot_offs(tot, nchunks, seed):
    """an off[nchunks][nheads + 1] whose totals per bin are `tot`: every bin's count dealt to the chunks at random"""
    tot = np.asarray(tot, dtype=np.int64)
    rng = np.random.default_rng(seed)
    cnt = np.zeros((nchunks, tot.size), np.int64)
    left = tot.copy()
    for c in range(nchunks - 1):
        cnt[c] = rng.integers(0, left + 1)
        left -= cnt[c]
    cnt[nchunks - 1] = left
    off = np.zeros((nchunks, tot.size + 1), U32)
    off[:, 1:] = np.cumsum(cnt, axis=1)
    return off


def hot_totals(kind, nheads, hmax, seed):
    """totals per bin.  zero; equal: every bin 1,500 (more than hmax bins share the one bucket: none is hot, unless hmax holds them all);
    top_exact / top_plus1: min(hmax, nheads / 2) bins -- and one more -- in the bucket [1024, 2048), the others in lower buckets; geometric: counts
    from 3 up to 40,000 spread over the buckets"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(nheads, np.int64)
    if kind == "equal":
        return np.full(nheads, 1500, np.int64)
    if kind in ("top_exact", "top_plus1"):
        k = min(hmax, nheads // 2) + (kind == "top_plus1")
        tot = rng.integers(0, 1024, nheads)
        tot[rng.permutation(nheads)[:k]] = rng.integers(1024, 2048, k)
        if k >= 2:
            idx = np.flatnonzero(tot >= 1024)
            tot[idx[0]], tot[idx[1]] = 1024, 2047            # the bucket's two ends
        return tot.astype(np.int64)
    return np.minimum(40_000, (3 * 1.0 / np.maximum(rng.random(nheads), 1e-4) ** 1.3)).astype(np.int64)


def hot_cases(nheads, nchunks):
    """(name, off, hmax, min_count) for one size: every kind of totals with hmax 1, 2 and 480 and min_count 0, inside a bucket (1,500: strictly
    between 2^10 and 2^11, with totals on both sides of it; the equal totals get it just below, at and just above themselves) and above every total"""
    out = []
    for ki, kind in enumerate(("zero", "equal", "top_exact", "top_plus1", "geometric")):
        for hmax in (1, 2, 480):
            tot = hot_totals(kind, nheads, hmax, 100 * ki + hmax)
            off = hot_offs(tot, nchunks, 7 * ki + hmax)
            for mc in ((0, 1499, 1500, 1501) if kind == "equal" else (0, 1500, int(tot.max()) + 1)):
                out.append((f"{kind},nheads={nheads},nchunks={nchunks},hmax={hmax},min_count={mc}", off, hmax, mc))
    return out
