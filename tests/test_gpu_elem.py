"""GPU suite (-m gpu): the element sizes of typed ranges chosen on the device (include/nlzm_hip_elem.h: nlzm_hip_plane_costs*, nlzm_hip_choose_elems*,
nlzm_hip_compress_ranges_auto*) against the model (tests/elem_model.py) and the oracle run on the model's planes at the model's choice, and the torch
binding.  Every check is exact.  Inputs are under 600 KB but for the one buffer beyond 4 GiB, which exists on the device alone; only streams a
compressor made are handed to the device."""
import ctypes as C

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus
from tests import elem_model, oracle_py, planes_model

pytestmark = pytest.mark.gpu

HIST = 17
LINE = 1 << 32
FAR_N = LINE + (1 << 22)
# device memory the far test needs: its one buffer, and a margin of 1 GiB for the library's scratch and the allocator's rounding
FAR_NEED = FAR_N + (1 << 30)


def model_of(data, ranges):
    memo = {}
    for o, n in ranges:
        if (o, n) not in memo:
            H = elem_model.hist(data[o:o + n])
            memo[(o, n)] = (elem_model.costs_of_hist(H), H)
    return [memo[r][0] for r in ranges], np.stack([memo[r][1] for r in ranges])


def test_plane_costs_against_the_model_in_one_call(gpu):
    """lengths 0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, S - 1, S, S + 1, 2S + 11 at offsets that move through 0 .. 15, every offset 0 .. 15 at lengths
    17, 4096 and S + 1, repeated and overlapping ranges; on mixed bytes, one repeated byte and a counter i mod 256: every counter and every cost"""
    S = gpu.counter("elem_segment_bytes")
    span = 2 * S + 11 + 16
    parts = [corpus.mixed(span, corpus.SEED + 330), np.full(span, 0xC3, dtype=np.uint8), np.arange(span, dtype=np.uint32).astype(np.uint8)]
    data = np.concatenate(parts)
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, S - 1, S, S + 1, 2 * S + 11]
    ranges = []
    for c in range(3):
        ranges += [(c * span + (3 * i + c) % 16, n) for i, n in enumerate(lengths)]
        ranges += [(c * span + o, n) for o in range(16) for n in (17, 4096, S + 1)]
    ranges += [ranges[5], ranges[12], (span - 100, 300), (span - 100, 300), (2 * span - 4096, S + 4096), (0, 3 * span)]      # repeats, and ranges across two contents
    costs, hist = gpu.plane_costs(data, ranges, hist=True)
    assert gpu.counter("elem_bytes") == sum(n for _, n in ranges)
    want_costs, want_hist = model_of(data, ranges)
    bad = [(r, [int(v) for v in np.argwhere(g != w)[0]]) for r, g, w in zip(ranges, hist, want_hist) if not np.array_equal(g, w)]
    assert not bad, bad[:4]
    bad = [(r, g, w) for r, g, w in zip(ranges, costs, want_costs) if g != w]
    assert not bad, bad[:4]
    assert gpu.plane_costs(data, ranges) == want_costs          # (without the histograms: the ranges of one segment never leave their wave)


def test_one_range_and_three_thousand(gpu):
    """k = 1, and k = 3,000 ranges of 0 .. 300 bytes: more waves than one pass of the grid's small units"""
    data = corpus.mixed(40_000, corpus.SEED + 331)
    rng = np.random.default_rng(corpus.SEED + 332)
    ranges = [(int(o), int(n)) for o, n in zip(rng.integers(0, 39_000, 3000), rng.integers(0, 301, 3000))]
    want, _ = model_of(data, ranges)
    assert gpu.plane_costs(data, ranges) == want
    assert gpu.plane_costs(data, ranges[7:8]) == want[7:8]
    assert gpu.plane_costs(data, [(0, 40_000)]) == [elem_model.costs(data)]
    assert gpu.choose_elems(data, ranges) == [1] * 3000          # (below 4,096 bytes)


@pytest.fixture(scope="module")
def six():
    """six ranges of 16 KiB to 128 KiB in one buffer, none aligned: bf16 and fp32 weights, Zipf int32 ids, a float64 walk, prose, random bytes"""
    rng = np.random.default_rng(corpus.SEED + 333)
    w = (rng.standard_normal(32768) * 0.02).astype("<f4")
    parts = [
        (w.view("<u4") >> 16).astype("<u2").tobytes(),                                  # 64 KiB
        w.tobytes(),                                                                    # 128 KiB
        np.minimum(rng.zipf(1.2, 16384), (1 << 31) - 1).astype("<i4").tobytes(),        # 64 KiB
        np.cumsum(rng.standard_normal(4096)).astype("<f8").tobytes(),                   # 32 KiB
        corpus.syn_text(40_000).tobytes(),
        rng.integers(0, 256, 16384, dtype=np.uint8).tobytes(),
    ]
    blob, ranges = b"", []
    for b in parts:
        blob += b"\x00" * 3
        ranges.append((len(blob), len(b)))
        blob += b
    data = np.frombuffer(blob, dtype=np.uint8)
    elems = [elem_model.choose_for(data[o:o + n]) for o, n in ranges]
    assert elems == [2, 4, 4, 8, 1, 1]              # (what the pricing table of DESIGN.md section 31 has for these kinds)
    return {"data": data, "ranges": ranges, "elems": elems}


def test_choose_elems_is_the_models(gpu, six):
    assert gpu.choose_elems(six["data"], six["ranges"]) == six["elems"]
    costs = gpu.plane_costs(six["data"], six["ranges"])
    assert [gpu.choose_elem(c, n) for c, (_, n) in zip(costs, six["ranges"])] == six["elems"]


def test_compress_auto_against_the_oracle(gpu, six):
    data, ranges, elems = six["data"], six["ranges"], six["elems"]
    want = [oracle_py.compress(planes_model.forward(data[o:o + n], e), HIST) for (o, n), e in zip(ranges, elems)]
    got, chosen = gpu.compress_auto(data, ranges, HIST)
    assert chosen == elems
    assert [len(s) for s in got] == [len(s) for s in want] and got == want
    assert gpu.counter("elem_us") > 0 and gpu.counter("planes_bytes") == sum(n for _, n in ranges)
    raw = [data[o:o + n].tobytes() for o, n in ranges]
    assert gpu.decompress_typed(b"".join(got), [len(s) for s in got], [n for _, n in ranges], chosen) == raw
    # a repeated range, with dedup: the same streams, one of them a copy
    more = ranges + [ranges[2]]
    again, chosen2 = gpu.compress_auto(data, more, HIST, dedup=True)
    assert chosen2 == elems + [elems[2]] and again == want + [want[2]]
    assert gpu.counter("dedup_distinct") == len(ranges) and gpu.counter("dedup_ranges") == 0
    assert gpu.decompress_typed(b"".join(again), [len(s) for s in again], [n for _, n in more], chosen2) == raw + [raw[2]]


def test_compress_tensors_auto(gpu):
    g = torch.Generator().manual_seed(corpus.SEED + 334)
    ids = torch.randint(0, 3000, (4096,), generator=g, dtype=torch.int32)
    records = ids.view(torch.uint8).clone()          # a uint8 tensor of packed int32 records, 16 KiB
    weights = (torch.randn(8192, generator=g) * 0.02).to(torch.bfloat16)
    tensors = [records, weights.to("cuda:0")]
    assert elem_model.choose_for(records.numpy()) == 4
    container, meta = gpu.compress_tensors(tensors, HIST, auto=True)
    assert [m[1:3] for m in meta] == [(16384, 4), (16384, 2)]
    blob = container.cpu().numpy().tobytes()
    assert blob[: meta[0][0]] == oracle_py.compress(planes_model.forward(records.numpy(), 4), HIST)
    back = gpu.decompress_tensors(container, meta)
    for t, r in zip(tensors, back):
        assert r.dtype == t.dtype and r.shape == t.shape and torch.equal(r.cpu().view(torch.uint8), t.cpu().contiguous().view(torch.uint8))
    plain, meta1 = gpu.compress_tensors(tensors, HIST)
    assert [m[1:3] for m in meta1] == [(16384, 1), (16384, 2)] and meta1[1] == meta[1]
    assert plain.numel() > container.numel()         # (the records are worth filtering)
    assert gpu.compress_tensors(tensors, HIST, auto=False)[1] == meta1


def test_a_range_behind_4_gib(gpu):
    """one buffer of 2^32 + 2^22 bytes on the device, zeros but for 140,000 bytes behind offset 2^32; ranges that start behind 2^32, one of them longer
    than a segment, and one that crosses the line: costs and counters exact against the model on their bytes"""
    free, total = torch.cuda.mem_get_info()
    if free < FAR_NEED:
        pytest.skip(f"the far buffer needs {FAR_NEED} bytes of device memory, {free} are free (of {total})")
    lib = gpu.load_library()
    S = gpu.counter("elem_segment_bytes")
    island = corpus.mixed(140_000, corpus.SEED + 335)
    at = LINE + 12_345
    x = torch.zeros(FAR_N, dtype=torch.uint8, device="cuda:0")
    x[at: at + island.size] = torch.from_numpy(island).to("cuda:0")
    x[LINE - 3000: LINE] = torch.from_numpy(island[:3000]).to("cuda:0")
    torch.cuda.synchronize()
    ranges = [(at + 3, 4099), (at + 17, S + 4000), (at, island.size), (LINE - 3000, 3000 + 12_345 + 5000), (FAR_N - 5000, 5000)]
    k = len(ranges)
    cost, hist = (C.c_uint64 * (4 * k))(), np.zeros((k, 8, 256), dtype=np.uint64)
    u64 = lambda v: (C.c_uint64 * k)(*v)
    rc = lib.nlzm_hip_plane_costs_dev(x.data_ptr(), FAR_N, k, u64([o for o, _ in ranges]), u64([n for _, n in ranges]), cost, hist.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, lib.nlzm_hip_last_error()
    del x
    torch.cuda.empty_cache()

    def read(o, n):
        out = np.zeros(n, dtype=np.uint8)
        for lo, b in ((at, island), (LINE - 3000, island[:3000])):
            a, z = max(o, lo), min(o + n, lo + b.size)
            if a < z:
                out[a - o: z - o] = b[a - lo: z - lo]
        return out

    for i, (o, n) in enumerate(ranges):
        H = elem_model.hist(read(o, n))
        assert np.array_equal(hist[i], H), f"nlzm_hip_plane_costs_dev: offset {o} (2^32 {o - LINE:+d}), {n} bytes: the counters differ"
        got, want = tuple(int(cost[4 * i + j]) for j in range(4)), elem_model.costs_of_hist(H)
        assert got == want, f"nlzm_hip_plane_costs_dev: offset {o} (2^32 {o - LINE:+d}), {n} bytes: got {got}, want {want}"


def test_counters(gpu, six):
    gpu.plane_costs(six["data"], six["ranges"])
    assert gpu.counter("elem_us") > 0 and gpu.counter("elem_bytes") == sum(n for _, n in six["ranges"])
    assert gpu.counter("elem_segment_bytes") % 16 == 0
    gpu.plane_costs(six["data"], [(0, 7)])           # (nothing to count: no launch)
    assert gpu.counter("elem_us") == 0 and gpu.counter("elem_bytes") == 7
