"""GPU suite (-m gpu): the byte-plane filter of typed ranges (nlzm_hip_planes*, nlzm_hip_compress_ranges_typed*, nlzm_hip_decompress_blocks_typed*)
against the numpy model (tests/planes_model.py) and the oracle run on the model's planes, the torch binding, and the command line's -elem:E.
Every check is exact.  Inputs are under 300 KB; only streams a compressor made are handed to the device."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus
from tests import oracle_py, planes_model
from tests.cli_tools import cli

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
HIST = 16
ELEMS = planes_model.ELEMS
GUARD = 0xEE


@pytest.fixture(scope="module")
def data():
    """150 KB that tell their positions apart: random bytes, and a stretch of a counter"""
    d = np.random.default_rng(corpus.SEED + 160).integers(0, 256, 150_000, dtype=np.uint8)
    d[1000:1512] = np.arange(512, dtype=np.uint32).astype(np.uint8)
    return d


def edge_cases(S):
    """(source offset, length, e) for every e: the lengths round an element, a 16-byte unit, sixteen elements and the segment; source misalignments 3 and 9"""
    out = []
    for e in ELEMS:
        for i, n in enumerate(sorted({0, 1, e - 1, e, e + 1, 15, 16, 17, 16 * e - 1, 16 * e, 16 * e + 1, S - 1, S, S + 1, 2 * S + e + 3})):
            out.append(((3, 9)[i % 2] + 16 * (i % 5), n, e))
            if n >= S - 1:
                out.append(((9, 3)[i % 2] + 16, n, e))
    return out


@pytest.mark.parametrize("inverse", [False, True])
def test_host_form_against_the_model(gpu, data, inverse):
    S = gpu.counter("planes_segment_bytes")
    cases = edge_cases(S)
    got = gpu.planes(data, [(o, n) for o, n, _ in cases], [e for _, _, e in cases], inverse)
    assert gpu.counter("planes_bytes") == sum(n for _, n, _ in cases)
    bad = [(o, n, e) for (o, n, e), g in zip(cases, got) if g != planes_model.apply(data[o:o + n], e, inverse)]
    assert not bad, bad
    # inverse(forward) is the identity, through the device both ways
    back = gpu.planes(b"".join(got), [(sum(n for _, n, _ in cases[:i]), cases[i][1]) for i in range(len(cases))], [e for _, _, e in cases], not inverse)
    assert back == [data[o:o + n].tobytes() for o, n, _ in cases]


def planes_dev(lib, src, dst, ranges, inverse):
    """ranges: (src_off, dst_off, len, e)"""
    k = len(ranges)
    u64 = lambda j: (C.c_uint64 * k)(*[r[j] for r in ranges])
    el = (C.c_uint8 * k)(*[r[3] for r in ranges])
    return lib.nlzm_hip_planes_dev(src.data_ptr(), int(src.numel()), dst.data_ptr(), int(dst.numel()), k, u64(0), u64(1), u64(2), el, int(inverse))


@pytest.mark.parametrize("inverse", [False, True])
def test_dev_form_against_the_model_between_guard_bytes(gpu, data, inverse):
    """the edge cases, and lengths 100 + j written to destinations at every misalignment j = 0 .. 15, all in one launch on torch tensors; every
    destination lies between guard bytes, which stay as they were"""
    lib = gpu.load_library()
    S = gpu.counter("planes_segment_bytes")
    cases = edge_cases(S) + [(5 + 7 * j, 100 + j, ELEMS[j % 4]) for j in range(16)] + [(11, 100 + j, ELEMS[(j + 1) % 4]) for j in range(16)]
    ranges, at = [], 64
    for i, (o, n, e) in enumerate(cases):
        mis = (i - len(edge_cases(S))) % 16 if i >= len(edge_cases(S)) else (5 * i + 1) % 16
        at = (at + 15) // 16 * 16 + mis            # (torch allocations are 16-byte aligned and more)
        ranges.append((o, at, n, e))
        at += n + 48
    src = torch.from_numpy(data).to("cuda:0")
    dst = torch.full((at + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    assert planes_dev(lib, src, dst, ranges, inverse) == 0, lib.nlzm_hip_last_error()
    out = dst.cpu().numpy()
    want = np.full(out.size, GUARD, dtype=np.uint8)
    for o, d, n, e in ranges:
        want[d:d + n] = np.frombuffer(planes_model.apply(data[o:o + n], e, inverse), dtype=np.uint8)
    diff = np.flatnonzero(out != want)
    assert diff.size == 0, (diff[:8].tolist(), [r for r in ranges if r[1] - 48 <= diff[0] < r[1] + r[2] + 48])
    assert gpu.counter("planes_bytes") == sum(r[2] for r in ranges)


def test_error_returns(gpu, data):
    """every argument error, on the device that is there: nothing is launched, nothing is written, and the next call works"""
    lib = gpu.load_library()
    src = torch.from_numpy(data[:4096].copy()).to("cuda:0")
    dst = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bad = [
        ([(0, 0, 100, 2), (0, 99, 10, 2)], b"overlaps range 1 "),
        ([(0, 0, 100, 3)], b"element size 3"),
        ([(4000, 0, 97, 2)], b"range 0 "),
        ([(0, 4000, 97, 2)], b"range 0 "),
    ]
    for ranges, text in bad:
        assert planes_dev(lib, src, dst, ranges, False) == E_ARG and text in lib.nlzm_hip_last_error(), ranges
    assert planes_dev(lib, src, src, [(0, 2048, 100, 2)], False) == E_ARG and b"no in-place form" in lib.nlzm_hip_last_error()
    assert planes_dev(lib, src, src[1024:], [(0, 0, 100, 2)], True) == E_ARG and b"no in-place form" in lib.nlzm_hip_last_error()
    assert bool((dst == GUARD).all())
    with pytest.raises(nlzm_amd.NlzmError):
        gpu.planes(bytes(100), [(0, 100)], [5])
    with pytest.raises(ValueError):
        gpu.planes(bytes(100), [], [])
    with pytest.raises(nlzm_amd.NlzmError):
        gpu.compress_typed(bytes(100), [(0, 50), (60, 41)], [2, 4], HIST)
    with pytest.raises(nlzm_amd.NlzmError):
        gpu.compress_typed(bytes(100), [(0, 50), (60, 40)], [2, 7], HIST)
    assert planes_dev(lib, src, dst, [(0, 16, 100, 4)], False) == 0
    assert dst[16:116].cpu().numpy().tobytes() == planes_model.forward(data[:100], 4)


@pytest.fixture(scope="module")
def ten(gpu):
    """250 KB of typed content and ten ranges with mixed e: bf16-like and fp32-like weights, int32 and int64 indices, text at e = 1, a duplicate of
    the int32 range (the same bytes elsewhere), an empty range, a ragged tail.  The oracle's streams of the model's planes are made once."""
    rng = np.random.default_rng(corpus.SEED + 161)
    w = (rng.standard_normal(20_000) * 0.02).astype("<f4")
    parts = [
        ((w.view("<u4") >> 16).astype("<u2").tobytes(), 2),
        (w[:9_000].tobytes(), 4),
        ((np.arange(4096) * 3 + 1000).astype("<i4").tobytes(), 4),
        ((np.arange(6_000) * 7).astype("<i8").tobytes(), 8),
        (corpus.syn_text(20_000).tobytes(), 1),
        ((np.arange(4096) * 3 + 1000).astype("<i4").tobytes(), 4),
        (rng.integers(0, 50, 30_001, dtype=np.uint8).tobytes(), 2),
        (rng.integers(0, 256, 1_003, dtype=np.uint8).tobytes(), 8),
    ]
    blob, ranges, elems = b"", [], []
    for b, e in parts:
        blob += b"\x00" * 3                          # (no range starts aligned)
        ranges.append((len(blob), len(b)))
        elems.append(e)
        blob += b
    ranges += [(len(blob), 0), (ranges[1][0] + 2, 10_000)]      # an empty range, and one that overlaps another at a different element size
    elems += [4, 2]
    data = np.frombuffer(blob, dtype=np.uint8)
    assert data.size < 300_000
    filtered = [planes_model.forward(data[o:o + l], e) for (o, l), e in zip(ranges, elems)]
    return {"data": data, "ranges": ranges, "elems": elems, "want": [oracle_py.compress(f, HIST) for f in filtered]}


def test_compress_ranges_typed_against_the_oracle(gpu, ten):
    got = gpu.compress_typed(ten["data"], ten["ranges"], ten["elems"], HIST)
    assert gpu.counter("planes_bytes") == sum(l for _, l in ten["ranges"]) and gpu.counter("planes_us") > 0
    assert [len(s) for s in got] == [len(s) for s in ten["want"]]
    assert got == ten["want"]
    distinct = gpu.counter("dedup_distinct")
    again = gpu.compress_typed(ten["data"], ten["ranges"], ten["elems"], HIST, dedup=True)
    assert again == got and gpu.counter("dedup_ranges") == 0
    assert gpu.counter("dedup_distinct") == len(ten["ranges"]) - 1          # (the second int32 range is the first one's copy)
    assert gpu.counter("dedup_distinct") < max(distinct, len(ten["ranges"]))
    # the filter is worth something on the index arrays: a quarter of the untyped stream at most
    plain = gpu.compress_ranges(ten["data"], ten["ranges"], HIST)
    assert 4 * len(got[2]) <= len(plain[2]) and 4 * len(got[3]) <= len(plain[3])
    # no element sizes, or all 1: the untyped call itself
    assert gpu.compress_typed(ten["data"], ten["ranges"], None, HIST) == plain
    assert gpu.compress_typed(ten["data"], ten["ranges"], [1] * len(ten["ranges"]), HIST) == plain


def test_decompress_blocks_typed_gives_the_ranges(gpu, ten):
    data, ranges, elems = ten["data"], ten["ranges"], ten["elems"]
    blob = b"".join(ten["want"])
    raw = [data[o:o + l].tobytes() for o, l in ranges]
    lens, raws = [len(s) for s in ten["want"]], [l for _, l in ranges]
    assert gpu.decompress_typed(blob, lens, raws, elems) == raw
    assert gpu.counter("planes_bytes") == sum(raws)
    assert gpu.decompress_typed(blob, None, None, elems) == raw           # (the hop over the frame headers, a size pass)
    # without the filter undone the blocks are the model's planes
    assert gpu.decompress_blocks(blob, len(ranges)) == [planes_model.forward(r, e) for r, e in zip(raw, elems)]
    # a destination one byte short
    lib = gpu.load_library()
    k = len(ranges)
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to("cuda:0")
    dst = torch.zeros(sum(raws), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    got = C.c_uint64(0)
    args = (src.data_ptr(), len(blob), k, (C.c_uint64 * k)(*lens), (C.c_uint64 * k)(*raws), (C.c_uint8 * k)(*elems), dst.data_ptr())
    assert lib.nlzm_hip_decompress_blocks_typed_dev(*args, sum(raws) - 1, None, C.byref(got)) == E_CAPACITY
    assert lib.nlzm_hip_decompress_blocks_typed_dev(*args, sum(raws), None, C.byref(got)) == 0 and got.value == sum(raws)
    assert dst.cpu().numpy().tobytes() == b"".join(raw)


def test_tensors_round_trip(gpu):
    g = torch.Generator().manual_seed(corpus.SEED + 162)
    a = (torch.randn(1000, generator=g) * 0.02).to(torch.bfloat16)
    b = torch.randn(777, generator=g).reshape(7, 111)
    c = torch.arange(33, dtype=torch.int64) * 1000 - 5
    d = torch.tensor([1, 2, 3, 250, 0], dtype=torch.uint8)
    tensors = [a, b.to("cuda:0"), c, d, a.clone()]        # (a tied copy last)
    container, meta = gpu.compress_tensors(tensors, HIST)
    assert container.dtype == torch.uint8 and container.is_cuda and container.numel() == sum(m[0] for m in meta)
    assert [m[1:3] for m in meta] == [(2000, 2), (3108, 4), (264, 8), (5, 1), (2000, 2)]
    blob = container.cpu().numpy().tobytes()
    at = 0
    for t, m in zip(tensors, meta):
        raw = t.cpu().contiguous().view(torch.uint8).numpy().tobytes()
        assert blob[at: at + m[0]] == oracle_py.compress(planes_model.forward(raw, m[2]), HIST)
        at += m[0]
    back = gpu.decompress_tensors(container, meta)
    for t, r in zip(tensors, back):
        assert r.is_cuda and r.dtype == t.dtype and r.shape == t.shape
        assert torch.equal(r.cpu().view(torch.uint8), t.cpu().contiguous().view(torch.uint8))
    tied, meta2 = gpu.compress_tensors(tensors, HIST, dedup=True)
    assert torch.equal(tied, container) and meta2 == meta and gpu.counter("dedup_distinct") == 4 and gpu.counter("dedup_ranges") == 0


def test_cli_elem(gpu, tmp_path):
    """-elem:4 -cdc:12 c, then d -gpu, t -gpu and host d: the output is the input and the CRC32s, which are the raw bytes', agree; every block holds
    whole elements and its stream is the oracle's of the model's planes; x refuses; -blocks:3 and -elem alone with -verify"""
    rng = np.random.default_rng(corpus.SEED + 163)
    ids = np.minimum(rng.zipf(1.3, 50_000), 1 << 20).astype("<i4")
    raw = ids.tobytes() + b"xyz"                     # (three bytes behind the last whole element)
    src, out = tmp_path / "in.bin", tmp_path / "c.nlzm"
    src.write_bytes(raw)
    r = cli("-window:16", "-elem:4", "-cdc:12", "c", src, out)
    assert r.returncode == 0 and "(cut by content)" in r.stdout and "Block index:" in r.stdout, r.stdout
    lens, raws, crcs, elems = nlzm_amd.read_index_typed(str(out) + ".idx")
    k = len(lens)
    assert open(str(out) + ".idx").read().startswith(f"NLZMIDX 3 {k} {len(raw)} ") and k > 10
    assert elems == [4] * k and sum(raws) == len(raw) and all(x % 4 == 0 and x > 0 for x in raws[:-1])
    starts = [sum(raws[:i]) for i in range(k)]
    assert crcs == [zlib.crc32(raw[o:o + l]) for o, l in zip(starts, raws)]
    blob = out.read_bytes()
    assert sum(lens) == len(blob)
    for i in (0, 1, k // 2, k - 1):
        at = sum(lens[:i])
        assert blob[at: at + lens[i]] == oracle_py.compress(planes_model.forward(raw[starts[i]: starts[i] + raws[i]], 4), 16), i
    for n, flags in enumerate((("-gpu",), ())):
        back = tmp_path / f"back{n}.bin"
        r = cli(*flags, "d", out, back)
        assert r.returncode == 0 and f"CRC32 ok ({k} blocks)" in r.stdout and back.read_bytes() == raw, r.stdout
    r = cli("-gpu", "t", out)
    assert r.returncode == 0 and f"CRC32 ok ({k} blocks)" in r.stdout, r.stdout
    part = tmp_path / "part.bin"
    r = cli("-range:0:10", "x", out, part)
    assert r.returncode == 255 and r.stdout.count("Error:") == 1 and "NLZMIDX 3" in r.stdout and not part.exists(), r.stdout
    # the typed container is smaller than the untyped one of the same cuts' kind
    plain = tmp_path / "p.nlzm"
    r = cli("-window:16", "-cdc:12", "c", src, plain)
    assert r.returncode == 0 and len(blob) < plain.stat().st_size, r.stdout
    # -blocks:3: ceil(n / 3) rounded up to whole elements; alone: one block; both with -verify
    out3, out1 = tmp_path / "b3.nlzm", tmp_path / "b1.nlzm"
    r = cli("-window:16", "-elem:8", "-blocks:3", "-verify", "c", src, out3)
    assert r.returncode == 0 and "Verified" in r.stdout, r.stdout
    per = -(-len(raw) // 3)
    per = -(-per // 8) * 8
    assert nlzm_amd.read_index_typed(str(out3) + ".idx")[1::2] == ([per, per, len(raw) - 2 * per], [8, 8, 8])
    r = cli("-window:16", "-elem:2", "-verify", "c", src, out1)
    assert r.returncode == 0 and "Verified" in r.stdout, r.stdout
    lens1, raws1, crcs1, elems1 = nlzm_amd.read_index_typed(str(out1) + ".idx")
    assert (raws1, crcs1, elems1) == ([len(raw)], [zlib.crc32(raw)], [2]) and out1.read_bytes() == oracle_py.compress(planes_model.forward(raw, 2), 16)
    for o in (out3, out1):
        r = cli("t", o)
        assert r.returncode == 0 and "CRC32 ok" in r.stdout, r.stdout
