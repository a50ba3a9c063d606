"""GPU suite (-m gpu): the range kernels behind offset 2^32 of ONE buffer.  A tensor of 2^32 + 2^22 bytes is made on the device -- one fill byte and a
few islands of random bytes, tests/far_model.py's layout -- and nlzm_hip_crc32*_dev, nlzm_hip_planes_dev, nlzm_hip_equal_ranges_dev,
nlzm_hip_cut_points_dev and nlzm_hip_compress_ranges*_dev are held to the sparse model, to the oracle and, for the ranges longer than 2^32, to plain
torch on the device.  No array of that size ever exists on the host.  Every check is exact and names entry point, offset, length, got and want."""
import ctypes as C

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

from tests import far_model, oracle_py, planes_model

pytestmark = pytest.mark.gpu

E_CAPACITY = -4
HIST = 16
SEED = 20261
LINE, N, S = far_model.LINE, far_model.N, far_model.S
GUARD = 0xEE
PIECE = 1 << 28             # what one torch call compares or counts: no temporary is larger
# device memory the file needs at its peak (the long planes test): the far buffer, the second far tensor, a random source, torch's transposed
# reference -- four tensors of N bytes -- and a margin of 2 GiB for what is not counted here: the 128 bytes behind the buffer, torch's PIECE-sized
# temporaries, the cut bitmap (N / 8), the library's scratch and streams, the allocator's rounding
NEED = 4 * N + (2 << 30)
CUT = (11, 4096, 1 << 26)   # avg_bits, min_len, max_len


@pytest.fixture(scope="module")
def far(gpu):
    free, total = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip(f"the far buffers need {NEED} bytes of device memory, {free} are free (of {total})")
    model, where = far_model.far_with_copies(SEED)
    x = torch.full((N + 128,), model.fill, dtype=torch.uint8, device="cuda:0")       # (128 readable bytes behind n: nlzm_hip_compress_ranges_dev asks for them)
    for o, b in model.islands:
        x[o: o + b.size] = torch.from_numpy(b).to("cuda:0")
    y = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert x.data_ptr() % 256 == 0 and y.data_ptr() % 256 == 0
    yield {"model": model, "where": where, "x": x, "y": y, "lib": gpu.load_library()}
    del x, y
    torch.cuda.empty_cache()


def u64(v):
    return (C.c_uint64 * len(v))(*[int(a) for a in v])


# ---- CRC32 ------------------------------------------------------------------------------------------------------------------------------


def test_crc32_ranges_round_the_lines_and_over_all_bytes(gpu, far):
    """starts at 2^32 + d and 2^31 + d, d = -17 .. 17, lengths 0 / 1 / 15 / 16 / 17 / S - 1 / S / S + 1 / 70,001; ranges that end at the line, one
    behind it and at N; [0, N), [1, N - 1), [2^32 - 5, N) -- one call -- and nlzm_hip_crc32_dev over all N bytes with a seed"""
    lib, m, x = far["lib"], far["model"], far["x"]
    seg = gpu.counter("crc_segment_bytes")
    ranges = far_model.edge_ranges(LINE, N, seg)
    assert (0, N) in ranges and (1, N - 2) in ranges and (LINE - 5, N - LINE + 5) in ranges and 300 <= len(ranges) <= 1000
    assert all(((LINE if j else LINE >> 1) + d, ln) in ranges for j in (0, 1) for d in range(-17, 18) for ln in (0, 1, 15, 16, 17))
    assert all(any(o == mid + d and l == ln for o, l in ranges) for mid in (LINE, LINE >> 1) for d in (-17, 0, 17) for ln in (seg - 1, seg, seg + 1, 70_001)
               if (d + (0, 1, 15, 16, 17, seg - 1, seg, seg + 1, 70_001).index(ln)) % 3 == 0)
    k = len(ranges)
    crc = (C.c_uint32 * k)(*([0xDEAD] * k))
    rc = lib.nlzm_hip_crc32_ranges_dev(x.data_ptr(), N, k, u64([o for o, _ in ranges]), u64([l for _, l in ranges]), crc)
    assert rc == 0, lib.nlzm_hip_last_error()
    assert gpu.counter("crc_bytes") == sum(l for _, l in ranges)
    for (o, l), got in zip(ranges, crc):
        want = m.crc32(o, l)
        assert got == want, f"nlzm_hip_crc32_ranges_dev: offset {o} (2^32 {o - LINE:+d}), {l} bytes: got {got:#010x}, want {want:#010x}"
    one = C.c_uint32(0xDEAD)
    rc = lib.nlzm_hip_crc32_dev(x.data_ptr(), N, 0xC0FFEE, C.byref(one))
    assert rc == 0, lib.nlzm_hip_last_error()
    want = m.crc32(0, N, 0xC0FFEE)
    assert one.value == want and gpu.counter("crc_bytes") == N, f"nlzm_hip_crc32_dev: offset 0, {N} bytes, seed 0xC0FFEE: got {one.value:#010x}, want {want:#010x}"


# ---- byte planes ------------------------------------------------------------------------------------------------------------------------


def planes_dev(lib, src, src_len, dst, dst_len, ranges, inverse):
    """ranges: (src_off, dst_off, len, e)"""
    k = len(ranges)
    col = lambda j: u64([r[j] for r in ranges])
    el = (C.c_uint8 * k)(*[r[3] for r in ranges])
    return lib.nlzm_hip_planes_dev(src.data_ptr(), src_len, dst.data_ptr(), dst_len, k, col(0), col(1), col(2), el, int(inverse))


def count_not(t, byte):
    """how many bytes of t differ from `byte`, counted on the device"""
    return sum(int((t[i: i + PIECE] != byte).sum()) for i in range(0, t.numel(), PIECE))


def first_difference(a, b):
    """the first index at which two device tensors of one length differ, or None"""
    for i in range(0, a.numel(), PIECE):
        if not torch.equal(a[i: i + PIECE], b[i: i + PIECE]):
            return i + int((a[i: i + PIECE] != b[i: i + PIECE]).nonzero()[0])
    return None


@pytest.mark.parametrize("inverse", [False, True])
def test_planes_small_ranges_on_either_side_of_the_line(gpu, far, inverse):
    """e in 1, 2, 4, 8; lengths from a few hundred bytes to two segments and a ragged tail; the source below, across and above 2^32 and the
    destination below, across and above 2^32 -- all nine pairs -- at misalignments 0, 3 and 9.  One destination range can lie across the line
    at a time, so a call holds three ranges (one source region, the three destination regions); after every call the windows are compared
    on the host and the bytes of the whole destination that differ from the guard are counted on the device."""
    lib, m, x, y = far["lib"], far["model"], far["x"], far["y"]
    seg = gpu.counter("planes_segment_bytes")
    y.fill_(GUARD)
    calls = moved = 0
    for ranges in far_model.planes_calls(LINE, seg):
        e = ranges[0][3]
        torch.cuda.synchronize()           # (the guard was written on torch's stream; the library launches on its own)
        assert planes_dev(lib, x, N, y, N, ranges, inverse) == 0, lib.nlzm_hip_last_error()
        calls += 1
        not_guard = 0
        for s, d, n, _ in ranges:
            moved += n
            want = np.full(n + 128, GUARD, dtype=np.uint8)
            want[64: 64 + n] = np.frombuffer(planes_model.apply(m.read(s, n), e, inverse), dtype=np.uint8)
            got = y[d - 64: d + n + 64].cpu().numpy()
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (f"nlzm_hip_planes_dev (inverse {int(inverse)}, e {e}): source {s} (2^32 {s - LINE:+d}), destination {d} (2^32 {d - LINE:+d}), "
                                    f"{n} bytes: at byte {int(diff[0]) - 64} got {int(got[diff[0]]):#04x}, want {int(want[diff[0]]):#04x}")
            not_guard += int(np.count_nonzero(want != GUARD))
        assert gpu.counter("planes_bytes") == sum(r[2] for r in ranges)
        got = count_not(y, GUARD)
        assert got == not_guard, f"nlzm_hip_planes_dev (inverse {int(inverse)}, e {e}), ranges {ranges}: {got} bytes of the destination differ from the guard, want {not_guard}"
        for _, d, n, _ in ranges:
            y[d: d + n] = GUARD
    assert calls == 36 and moved > 36 * 3 * 333


def long_planes(gpu, far, e, inverse, s0, d0, n):
    """one range longer than 2^32 from a source of random bytes into the guarded tensor, against torch on the device"""
    lib, y = far["lib"], far["y"]
    g = torch.Generator(device="cuda:0").manual_seed(SEED + e)
    r = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    for i in range(0, N, PIECE):
        r[i: i + PIECE].random_(0, 256, generator=g)
    y.fill_(GUARD)
    torch.cuda.synchronize()
    assert n > LINE and n % e != 0 and s0 % 16 != 0 and d0 % 16 != 0 and s0 + n <= N and d0 + n <= N
    assert planes_dev(lib, r, N, y, N, [(s0, d0, n, e)], inverse) == 0, lib.nlzm_hip_last_error()
    assert gpu.counter("planes_bytes") == n
    mm = n // e
    src = r[s0: s0 + e * mm]
    want = (src.view(e, mm) if inverse else src.view(mm, e)).t().contiguous().view(-1)
    name = f"nlzm_hip_planes_dev (inverse {int(inverse)}, e {e}): source {s0}, destination {d0}, {n} bytes"
    at = first_difference(y[d0: d0 + e * mm], want)
    assert at is None, f"{name}: at byte {at} (plane {at // mm if not inverse else at % e}) got {int(y[d0 + at]):#04x}, want {int(want[at]):#04x}"
    del want
    assert torch.equal(y[d0 + e * mm: d0 + n], r[s0 + e * mm: s0 + n]), f"{name}: the tail of {n - e * mm} bytes"
    assert count_not(y[:d0], GUARD) == 0 and count_not(y[d0 + n:], GUARD) == 0, f"{name}: a byte outside the destination range has changed"


@pytest.mark.parametrize("inverse", [False, True])
def test_planes_one_range_longer_than_4_gib_e4(gpu, far, inverse):
    long_planes(gpu, far, 4, inverse, 5, 1027, LINE + 4099)          # (a tail of 3 bytes)


def test_planes_one_range_longer_than_4_gib_e8(gpu, far):
    long_planes(gpu, far, 8, False, 1027, 9, LINE + (1 << 21) + 5)


# ---- equal ranges -----------------------------------------------------------------------------------------------------------------------


def equal_ranges_dev(lib, t, n, ranges):
    k = len(ranges)
    first, fp = (C.c_uint32 * k)(*([0xDEAD] * k)), (C.c_uint64 * k)()
    rc = lib.nlzm_hip_equal_ranges_dev(t.data_ptr(), n, k, u64([o for o, _ in ranges]), u64([l for _, l in ranges]), first, fp)
    assert rc == 0, lib.nlzm_hip_last_error()
    return [int(v) for v in first], [int(v) for v in fp]


def test_equal_ranges_copies_on_either_side_of_the_line(gpu, far):
    """the piece across 2^32 and its copies below and above at all sixteen misalignments are one class, whole and as prefixes; the near-copy that
    differs in its last byte is a class of its own; first_of against the definition, every fingerprint against the sparse model"""
    lib, m, w = far["lib"], far["model"], far["where"]
    P = far_model.PIECE
    places = [w["across"]] + [o for pair in zip(w["below"], w["above"]) for o in pair]
    assert sorted(o % 16 for o in w["below"]) == sorted(o % 16 for o in w["above"]) == list(range(16)) and all(o + P <= LINE for o in w["below"]) and min(w["above"]) > LINE
    ranges = [(o, P) for o in places] + [(w["near"], P)] + [(o, S + 1) for o in places] + [(w["near"], S + 1), (w["near"] + 1, P - 1), (places[5] + 1, P - 1)]
    seen, want = {}, []
    for i, (o, l) in enumerate(ranges):
        want.append(seen.setdefault(m.read(o, l).tobytes(), i))
    assert want[: len(places) + 1] == [0] * len(places) + [len(places)] and want[-3] == len(places) + 1 and want[-2:] == [len(ranges) - 2, len(ranges) - 1]
    first, fps = equal_ranges_dev(lib, far["x"], N, ranges)
    for i, (o, l) in enumerate(ranges):
        assert first[i] == want[i], f"nlzm_hip_equal_ranges_dev: range {i}, offset {o} (2^32 {o - LINE:+d}), {l} bytes: first_of got {first[i]}, want {want[i]}"
        f = m.fingerprint(o, l)
        assert fps[i] == f, f"nlzm_hip_equal_ranges_dev: range {i}, offset {o} (2^32 {o - LINE:+d}), {l} bytes: fingerprint got {fps[i]:#018x}, want {f:#018x}"


def test_equal_ranges_longer_than_4_gib(gpu, far):
    """the second tensor made periodic (one chunk of 768 KiB again and again: 2^32 is no multiple of it, so bytes 2^32 apart differ): [0, L),
    [P, P + L) and [2P, 2P + L), L = 2^32 + 2^20, hold the same bytes -- but one byte behind the third range's 2^32nd is altered, outside the
    other two.  Also the fill-and-islands buffer's [0, N), whose fingerprint the sparse model has"""
    lib, y = far["lib"], far["y"]
    P = 3 << 18
    L = LINE + (1 << 20)
    chunk = np.random.default_rng(SEED + 50).integers(0, 256, P, dtype=np.uint8)
    c = torch.from_numpy(chunk).to("cuda:0")
    whole = N // P * P
    y[:whole].view(N // P, P)[:] = c
    y[whole:] = c[: N - whole]
    at = 2 * P + LINE + (1 << 19) + 5000           # index 2^32 + 2^19 + 5000 of the third range; the second ends at P + L
    assert P % S == 0 and LINE % P != 0 and P + L <= at < 2 * P + L <= N
    pm = far_model.Periodic(N, chunk, {at: int(chunk[at % P]) ^ 0x10})
    y[at] = pm.patches[at]
    torch.cuda.synchronize()
    ranges = [(0, L), (P, L), (2 * P, L), (3 * P, 777), (0, 777), (at - 776, 777)]
    first, fps = equal_ranges_dev(lib, y, N, ranges)
    want = [0, 0, 2, 3, 3, 5]
    for i, (o, l) in enumerate(ranges):
        assert first[i] == want[i], f"nlzm_hip_equal_ranges_dev (periodic buffer): range {i}, offset {o}, {l} bytes: first_of got {first[i]}, want {want[i]}"
        f = pm.fingerprint(o, l) if o % S == 0 else far_model.dedup_model.fingerprint(pm.read(o, l))
        assert fps[i] == f, f"nlzm_hip_equal_ranges_dev (periodic buffer): range {i}, offset {o}, {l} bytes: fingerprint got {fps[i]:#018x}, want {f:#018x}"
    assert fps[0] == fps[1] != fps[2] and gpu.counter("dedup_compared_bytes") >= L
    m = far["model"]
    ranges = [(0, N), (1, N - 2), (LINE - 5, N - LINE + 5), (0, N)]
    first, fps = equal_ranges_dev(lib, far["x"], N, ranges)
    assert first == [0, 1, 2, 0]
    for (o, l), got in zip(ranges, fps):
        assert got == m.fingerprint(o, l), f"nlzm_hip_equal_ranges_dev: offset {o}, {l} bytes: fingerprint got {got:#018x}, want {m.fingerprint(o, l):#018x}"


# ---- cut points -------------------------------------------------------------------------------------------------------------------------


def test_cut_points_over_all_bytes(gpu, far):
    """cuts on both sides of 2^32 decided by candidates in the islands, cuts forced at max_len across the fill, one cut within min_len of N;
    the list and "cut_candidates" against the sparse model; then cut_cap one short"""
    lib, m, x = far["lib"], far["model"], far["x"]
    avg_bits, lo, hi = CUT
    want, ncand = m.cut_points(avg_bits, lo, hi)
    cand = set((m.candidates(avg_bits) + 1).tolist())
    edges = [0] + want
    assert any(c in cand and c < LINE for c in want) and any(c in cand and c > LINE for c in want)
    assert any(b - a == hi and b not in cand for a, b in zip(edges, want)) and 0 < N - want[-1] < lo
    cap = len(want) + 16
    cuts, got = (C.c_uint64 * cap)(), C.c_uint32(0xDEAD)
    rc = lib.nlzm_hip_cut_points_dev(x.data_ptr(), N, avg_bits, lo, hi, cuts, cap, C.byref(got))
    assert rc == 0, lib.nlzm_hip_last_error()
    have = [int(cuts[i]) for i in range(min(got.value, cap))]
    bad = next((i for i, (a, b) in enumerate(zip(have, want)) if a != b), min(len(have), len(want)))
    assert have == want, (f"nlzm_hip_cut_points_dev: offset 0, {N} bytes, avg_bits {avg_bits}, min {lo}, max {hi}: {len(have)} cuts, want {len(want)}; "
                          f"cut {bad}: got {have[bad] if bad < len(have) else None}, want {want[bad] if bad < len(want) else None}")
    assert gpu.counter("cut_candidates") == ncand, f"nlzm_hip_cut_points_dev: cut_candidates got {gpu.counter('cut_candidates')}, want {ncand}"
    short = (C.c_uint64 * len(want))(*([7] * len(want)))
    rc = lib.nlzm_hip_cut_points_dev(x.data_ptr(), N, avg_bits, lo, hi, short, len(want) - 1, C.byref(got))
    assert rc == E_CAPACITY and got.value == len(want) and all(v == 7 for v in short), (rc, got.value)


# ---- compress ranges --------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ten(far):
    """ten ranges of 20 to 60 KB of island bytes: below, across and above 2^32, across 2^31, at the buffer's start, ending at N, one empty, one
    repeated, and the same 40,000 bytes at two far places (the piece across the line and a copy above it)"""
    m, w = far["model"], far["where"]
    ranges = [(LINE - 90_000, 30_000), (LINE - 20_001, 45_003), (LINE + 7, 60_000), ((LINE >> 1) - 10_000, 20_000), (N - 50_000, 50_000), (LINE + 3, 0),
              (LINE - 20_001, 45_003), (5, 25_000), (w["above"][3], 40_000), (w["across"], 40_000)]
    for o, l in ranges:
        assert l == 0 or (len(m.touching(o, l)) == 1 and m.touching(o, l)[0][0] <= o and o + l <= m.touching(o, l)[0][0] + m.touching(o, l)[0][1].size)
    raw = [m.read(o, l) for o, l in ranges]
    return {"ranges": ranges, "raw": raw, "memo": {}}


def oracle(ten, data: bytes):
    if data not in ten["memo"]:
        ten["memo"][data] = oracle_py.compress(data, HIST)
    return ten["memo"][data]


def compress_dev(far, ranges, elems=None):
    lib, x = far["lib"], far["x"]
    k = len(ranges)
    ln = u64([l for _, l in ranges])
    bound = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
    dst = torch.full((bound,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    blen, got = (C.c_uint64 * k)(), C.c_uint64(0)
    head = (x.data_ptr(), N, k, u64([o for o, _ in ranges]), ln)
    tail = (HIST, dst.data_ptr(), bound, blen, C.byref(got))
    if elems is None:
        rc = lib.nlzm_hip_compress_ranges_dev(*head, *tail)
    else:
        rc = lib.nlzm_hip_compress_ranges_typed_dev(*head, (C.c_uint8 * k)(*elems), *tail)
    assert rc == 0, lib.nlzm_hip_last_error()
    return [int(v) for v in blen], int(got.value), dst[: int(got.value)].cpu().numpy().tobytes()


def check_streams(name, ranges, blen, total, blob, want):
    assert total == sum(blen) == len(blob), (name, total, sum(blen))
    at = 0
    for i, ((o, l), w) in enumerate(zip(ranges, want)):
        got = blob[at: at + blen[i]]
        assert got == w, (f"{name}: range {i}, offset {o} (2^32 {o - LINE:+d}), {l} bytes: stream of {len(got)} bytes, want {len(w)}; "
                          f"first difference at byte {next((j for j, (a, b) in enumerate(zip(got, w)) if a != b), min(len(got), len(w)))}")
        at += blen[i]


def test_compress_ranges_far_offsets_against_the_oracle(gpu, far, ten):
    ranges = ten["ranges"]
    want = [oracle(ten, r.tobytes()) for r in ten["raw"]]
    plain = compress_dev(far, ranges)
    check_streams("nlzm_hip_compress_ranges_dev", ranges, *plain, want)
    gpu.set_option("dedup_ranges", 1)
    try:
        deduped = compress_dev(far, ranges)
        assert gpu.counter("dedup_distinct") == len(ranges) - 2 and gpu.counter("dedup_gather_us") > 0      # (the repeated range and the copy went through the gather launch)
    finally:
        gpu.set_option("dedup_ranges", 0)
    check_streams("nlzm_hip_compress_ranges_dev with dedup_ranges", ranges, *deduped, want)
    assert deduped == plain


def test_compress_ranges_typed_far_offsets_against_the_oracle(gpu, far, ten):
    ranges = ten["ranges"]
    elems = [(2, 4)[i % 2] for i in range(len(ranges))]
    want = [oracle(ten, planes_model.forward(r, e)) for r, e in zip(ten["raw"], elems)]
    got = compress_dev(far, ranges, elems)
    check_streams("nlzm_hip_compress_ranges_typed_dev", ranges, *got, want)
    assert gpu.counter("planes_bytes") == sum(l for _, l in ranges)
