"""GPU suite (-m gpu): the marshalling corners of the ctypes binding (nlzm_amd/__init__.py), one test per family of entry points -- empty inputs
(a NULL data pointer), no ranges at all, empty ranges beside a full one, a 1-byte input, the optional arrays left out.  Every call is a legal
one or is refused on the host.  What is expected comes from zlib, the oracle and the models under tests/, never from the library; every check is
exact.  Inputs are 40,000 bytes at window 15."""
import zlib

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

from nlzm_amd import corpus
from tests import cut_model, dedup_model, oracle_py, planes_model

pytestmark = pytest.mark.gpu

HIST = 15
N = 40_000


@pytest.fixture(scope="module")
def data():
    return corpus.syn_text(N)


@pytest.fixture(scope="module")
def shapes(data):
    """the two range lists every range call gets: (input, ranges, element sizes)"""
    return [(data, [(0, 0), (0, N), (0, 0)], [2, 4, 8]), (data[:1], [(0, 1)], [2])]


@pytest.fixture(scope="module")
def empty_stream():
    return oracle_py.compress(np.zeros(0, dtype=np.uint8), HIST)


def cut(src, ranges):
    return [src[o:o + l] for o, l in ranges]


def test_crc32_of_nothing_and_of_no_ranges(gpu, data):
    assert gpu.crc32(b"") == zlib.crc32(b"")
    assert gpu.crc32(b"", 0x1234ABCD) == zlib.crc32(b"", 0x1234ABCD)
    assert gpu.crc32_ranges(data, []) == []
    assert gpu.crc32_ranges(b"", []) == []
    assert gpu.crc32_ranges(data, [(0, 0)]) == [zlib.crc32(b"")]
    assert gpu.crc32_ranges(b"", [(0, 0)]) == [zlib.crc32(b"")]
    assert gpu.crc32_ranges(data, [(0, 0), (0, N), (0, 0)]) == [zlib.crc32(b""), zlib.crc32(data.tobytes()), zlib.crc32(b"")]


def test_compress_ranges_and_typed(gpu, shapes):
    """empty ranges round a full one, and one range that is all of a 1-byte input: the oracle's streams of the ranges, of the model's planes when
    typed; elems=None is the untyped call; the typed container comes back without block or raw lengths"""
    for src, ranges, elems in shapes:
        plain = [oracle_py.compress(p, HIST) for p in cut(src, ranges)]
        typed = [oracle_py.compress(np.frombuffer(planes_model.forward(p, e), dtype=np.uint8), HIST) for p, e in zip(cut(src, ranges), elems)]
        assert gpu.compress_ranges(src, ranges, HIST) == plain
        assert gpu.compress_ranges(src, ranges, HIST, dedup=True) == plain
        assert gpu.counter("dedup_ranges") == 0                  # (the option is as it stood)
        assert gpu.compress_typed(src, ranges, None, HIST) == plain
        assert gpu.compress_typed(src, ranges, elems, HIST) == typed
        assert gpu.compress_typed(src, ranges, elems, HIST, dedup=True) == typed
        assert gpu.counter("dedup_ranges") == 0
        want = [p.tobytes() for p in cut(src, ranges)]
        assert gpu.decompress_typed(b"".join(typed), None, None, elems) == want
        assert gpu.decompress_typed(b"".join(typed), [len(s) for s in typed], [l for _, l in ranges], elems) == want
        assert gpu.decompress_blocks(b"".join(plain), len(plain)) == want


def test_equal_ranges_and_planes(gpu, shapes):
    for src, ranges, elems in shapes:
        fp = []
        assert gpu.equal_ranges(src, ranges, fp) == dedup_model.first_of(src, ranges)
        assert fp == dedup_model.fingerprints(src, ranges)
        assert gpu.equal_ranges(src, ranges) == dedup_model.first_of(src, ranges)
        for inv in (False, True):
            assert gpu.planes(src, ranges, elems, inv) == [planes_model.apply(p, e, inv) for p, e in zip(cut(src, ranges), elems)]


def test_read_ranges_check_verify_and_decoder(gpu, data, empty_stream):
    blob = oracle_py.compress(data, HIST)
    assert gpu.read_ranges(blob, []) == []
    assert gpu.read_ranges(blob, [(0, 0)]) == [b""]
    assert gpu.read_ranges(blob, [(N, 0), (5, 7), (0, 0)]) == [b"", data[5:12].tobytes(), b""]
    assert gpu.read_ranges(blob, [], 1, [len(blob)], [N], [zlib.crc32(data.tobytes())]) == []
    # a one-block container of an empty input
    assert gpu.check(empty_stream, [zlib.crc32(b"")]) == 1
    assert gpu.check(empty_stream, [zlib.crc32(b"")], 1, [0]) == 1
    assert gpu.check(empty_stream, [zlib.crc32(b"") ^ 1], 1, [0]) == 0
    assert gpu.verify(empty_stream, b"") == 0
    assert gpu.decompress(empty_stream) == b""
    assert gpu.read_ranges(empty_stream, [(0, 0)]) == [b""]
    with gpu.Decoder(blob) as d:
        assert d.raw_lens == [N]
        assert d.read(0, 0) == b"" and d.read(N, 0) == b""
        assert d.done == [0] and not d.finished                 # (an empty read decodes nothing)
        with pytest.raises(ValueError):
            d.read(N, 1)
    with gpu.Decoder(empty_stream, 1, [len(empty_stream)], [0]) as d:
        assert d.read(0, 0) == b""


def test_cut_points_of_a_short_input(gpu, data):
    lo = cut_model.defaults(8)[0]
    for n in (0, 1, lo - 1, lo, lo + 1):
        assert gpu.cut_points(data[:n], 8) == cut_model.cut_points(data[:n], 8), n
    assert gpu.cut_points(data[:100], 8, 200, 300) == cut_model.cut_points(data[:100], 8, 200, 300) == []
    assert gpu.cut_ranges(0, []) == [(0, 0)]


def test_tensors_with_an_empty_one(gpu, empty_stream):
    tensors = [torch.empty(0), torch.arange(3, dtype=torch.int16)]
    container, meta = gpu.compress_tensors(tensors, HIST)
    second = oracle_py.compress(np.frombuffer(planes_model.forward(tensors[1].numpy().tobytes(), 2), dtype=np.uint8), HIST)
    assert bytes(container.cpu().numpy()) == empty_stream + second
    assert meta == [(len(empty_stream), 0, 4, torch.float32, (0,)), (len(second), 6, 2, torch.int16, (3,))]
    back = gpu.decompress_tensors(container, meta)
    assert [(t.dtype, tuple(t.shape), t.device.type) for t in back] == [(torch.float32, (0,), "cuda"), (torch.int16, (3,), "cuda")]
    assert back[1].cpu().tolist() == [0, 1, 2]
