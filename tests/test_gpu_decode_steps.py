"""GPU suite (-m gpu): decoding in steps -- nlzm_hip_decode_begin / _step / _extend_dev / _fetch / _finish / _abandon, nlzm_amd.Decoder and
`nlzm -gpu -steps:K d / t`.  A stream stops in front of a frame header and a later launch resumes it from the record the library keeps; the
bytes, the lengths and every counter are the one-shot decode's.  Only streams the device's compressor made are handed to the GPU (damaged and
cut streams are the simulator's business: tests/test_decode_steps_sim.py); errors in arguments are fine here."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cases

pytestmark = pytest.mark.gpu

E_ARG = -1
TOTALS = ("decode_syms", "decode_raw_ops", "decode_n_literal", "decode_n_dict", "decode_n_rep", "decode_ring_bytes", "decode_global_bytes", "decode_out_bytes")
ALL = (1 << 64) - 1
BLOCKS_K = 5


def case_of(name):
    return next(c for c in cases.CASES if c[0] == name)


def dev(arr):
    t = torch.zeros(max(1, arr.size), dtype=torch.uint8, device="cuda:0")
    if arr.size:
        t[:arr.size].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    torch.cuda.synchronize()
    return t


def arr_of(b):
    return np.frombuffer(b, dtype=np.uint8)


def chunk_of(n, wbits):
    return nlzm_amd.geometry(n, wbits)["chunk_size"]


def boundary(target, n, chunk):
    """the first frame boundary at or above `target` of a stream of n bytes (a frame's output ends at a multiple of the chunk size, or at n)"""
    return min(n, -(-target // chunk) * chunk)


@pytest.fixture(scope="module")
def made(gpu):
    """the small cases' streams, compressed on the device once, with the one-shot decode's totals beside them"""
    out = {}
    for name in ("text_200k_w15", "dups_600k_w20", "runs_300k_w18"):
        c = case_of(name)
        data = cases.make_case(c).copy()
        stream = gpu.compress(data, c[4])
        assert gpu.decompress(stream) == data.tobytes()
        out[name] = (data.tobytes(), stream, c[4], {k: gpu.counter(k) for k in TOTALS})
    return out


@pytest.fixture(scope="module")
def five(gpu):
    """five blocks of corpus.mixed(700_000) at window 18 (the input of tests/test_decode_sim.py's block set)"""
    data = corpus.mixed(700_000, corpus.SEED + 9)
    ranges = [shard.block_range(data.size, BLOCKS_K, i) for i in range(BLOCKS_K)]
    streams = gpu.compress_blocks(data, BLOCKS_K, 18)
    return data.tobytes(), ranges, streams


def test_one_frame_per_step(gpu, made):
    data, stream, wbits, one = made["text_200k_w15"]
    n, chunk = len(data), chunk_of(len(data), wbits)
    gpu.decompress(stream)
    one_cycles = gpu.counter("decode_cycles")
    with gpu.Decoder(stream) as d:
        cycles = 0
        for k in range(1, 15):
            done, finished = d.step(1)
            assert done == [min(k * chunk, n)] and finished == (k == 14), k
            assert gpu.counter("decode_steps") == k and gpu.counter("decode_out_bytes") == done[0]
            # the cycle counters run on through the state too: every launch adds its own, and the whole is never below its parts
            now = gpu.counter("decode_cycles")
            assert now > cycles and now >= gpu.counter("decode_window_cycles") + gpu.counter("decode_copy_cycles"), k
            assert gpu.counter("decode_max_stream_cycles") == now
            cycles = now
        assert 0.5 * one_cycles < cycles < 2 * one_cycles       # (fourteen launches' cycles are the one-shot decode's, give or take; not the last launch's alone)
        assert gpu.counter("decode_step_us") > 0
        got = d.read(0, n)
        assert gpu.counter("decode_steps") == 14          # (everything was decoded: the read launched nothing)
    assert got == data == gpu.decompress(stream)
    assert one == {k: gpu.counter(k) for k in TOTALS}      # (the decompress just above; and below: the stepped decode's totals)
    with gpu.Decoder(stream) as d:
        while not d.step(1)[1]:
            pass
        assert {k: gpu.counter(k) for k in TOTALS} == one


def test_ring_reload_keeps_the_split_of_match_bytes(gpu, made):
    """dups_600k_w20 has matches farther back than the ring: a resumed decode serves them from memory and the near ones from the ring it has
    reloaded, byte for byte as the one-shot decode does"""
    data, stream, wbits, one = made["dups_600k_w20"]
    assert one["decode_global_bytes"] == 224_252 and one["decode_ring_bytes"] > 100_000
    with gpu.Decoder(stream) as d:
        steps = 0
        while not d.step(2)[1]:
            steps += 1
        assert steps >= 2
        assert {k: gpu.counter(k) for k in TOTALS} == one
        assert d.read(0, len(data)) == data


def test_block_set_with_targets(gpu, five):
    data, ranges, streams = five
    lib = gpu.load_library()
    k = BLOCKS_K
    raws = [hi - lo for lo, hi in ranges]
    blob = b"".join(streams)
    d_src = dev(arr_of(blob))
    d_dst = torch.full((len(data),), 0xC3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    blen, raw = (C.c_uint64 * k)(*map(len, streams)), (C.c_uint64 * k)(*raws)
    assert lib.nlzm_hip_decode_begin_dev(d_src.data_ptr(), len(blob), k, blen, raw, d_dst.data_ptr(), len(data), 0) == 0, lib.nlzm_hip_last_error()
    targets = [0, 1, raws[2] // 2, ALL, 0]
    done, fin = (C.c_uint64 * k)(), C.c_int(1)
    assert lib.nlzm_hip_decode_step(0, (C.c_uint64 * k)(*targets), done, C.byref(fin), None) == 0, lib.nlzm_hip_last_error()
    chunks = [chunk_of(r, 18) for r in raws]
    assert list(done) == [0, boundary(1, raws[1], chunks[1]), boundary(raws[2] // 2, raws[2], chunks[2]), raws[3], 0] and fin.value == 0
    assert 0 < done[1] < raws[1] and raws[2] // 2 <= done[2] < raws[2]
    assert gpu.counter("decode_steps") == 1 and gpu.counter("decode_out_bytes") == sum(done)
    torch.cuda.synchronize()
    host = d_dst.cpu().numpy().tobytes()
    for (lo, hi), dn in zip(ranges, done):                 # what a block has decoded is the input's; the rest of its range is untouched
        assert host[lo:lo + dn] == data[lo:lo + dn] and host[lo + dn:hi] == b"\xC3" * (hi - lo - dn)
    assert lib.nlzm_hip_decode_step(0, None, done, C.byref(fin), None) == 0, lib.nlzm_hip_last_error()
    assert list(done) == raws and fin.value == 1
    raw_out, total = (C.c_uint64 * k)(), C.c_uint64(0)
    assert lib.nlzm_hip_decode_finish(raw_out, C.byref(total)) == 0, lib.nlzm_hip_last_error()
    assert list(raw_out) == raws and total.value == len(data)
    torch.cuda.synchronize()
    assert d_dst.cpu().numpy().tobytes() == data


def test_size_only_stepping(gpu, made):
    data, stream, wbits, one = made["runs_300k_w18"]
    lib = gpu.load_library()
    d_src = dev(arr_of(stream))
    assert lib.nlzm_hip_decode_begin_dev(d_src.data_ptr(), len(stream), 1, None, None, None, 0, 0) == 0, lib.nlzm_hip_last_error()
    done, fin, steps = (C.c_uint64 * 1)(), C.c_int(0), 0
    while not fin.value:
        assert lib.nlzm_hip_decode_step(2, None, done, C.byref(fin), None) == 0, lib.nlzm_hip_last_error()
        steps += 1
        assert steps < 50
    assert done[0] == len(data) and steps == 3             # (five frames, two a step)
    buf = (C.c_uint8 * 8)()
    assert lib.nlzm_hip_decode_fetch(0, 8, buf) == E_ARG    # nothing is stored
    total = C.c_uint64(0)
    assert lib.nlzm_hip_decode_finish(None, C.byref(total)) == 0 and total.value == len(data)


def test_input_that_arrives_later(gpu, made):
    data, stream, wbits, one = made["runs_300k_w18"]
    lib = gpu.load_library()
    n, chunk = len(data), chunk_of(len(data), wbits)
    heads, pos = [], 4                                     # the frame headers' offsets
    while int.from_bytes(stream[pos:pos + 4], "big"):
        heads.append(pos)
        pos += int.from_bytes(stream[pos + 4:pos + 8], "big") + int.from_bytes(stream[pos + 8:pos + 12], "big")
    assert len(heads) == 5
    cut = (heads[2] + heads[3]) // 2                       # inside the third frame
    d_src = dev(arr_of(stream))
    d_dst = torch.full((n,), 0xC3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.nlzm_hip_decode_begin_dev(d_src.data_ptr(), cut, 1, None, None, d_dst.data_ptr(), n, gpu.DECODE_MORE) == 0, lib.nlzm_hip_last_error()
    done, fin = (C.c_uint64 * 1)(), C.c_int(1)
    assert lib.nlzm_hip_decode_step(0, None, done, C.byref(fin), None) == 0, lib.nlzm_hip_last_error()
    assert done[0] == 2 * chunk and fin.value == 0
    total = C.c_uint64(0)
    assert lib.nlzm_hip_decode_finish(None, C.byref(total)) == E_ARG       # not at its end, and nobody said "that was all": still open
    assert lib.nlzm_hip_decode_extend_dev(cut - 1) == E_ARG
    # "that was all" (an extend without growth), a step that still wants input -- and then more comes after all: no longer "cut off"
    assert lib.nlzm_hip_decode_extend_dev(cut) == 0
    assert lib.nlzm_hip_decode_step(0, None, done, C.byref(fin), None) == 0 and done[0] == 2 * chunk and fin.value == 0
    assert lib.nlzm_hip_decode_extend_dev(len(stream) - 1) == 0
    assert lib.nlzm_hip_decode_finish(None, C.byref(total)) == E_ARG       # (not E_FORMAT, and the set stays open)
    assert lib.nlzm_hip_decode_extend_dev(len(stream)) == 0, lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_decode_step(0, None, done, C.byref(fin), None) == 0, lib.nlzm_hip_last_error()
    assert done[0] == n and fin.value == 1
    assert {k: gpu.counter(k) for k in TOTALS} == one
    assert lib.nlzm_hip_decode_finish(None, C.byref(total)) == 0 and total.value == n
    torch.cuda.synchronize()
    assert d_dst.cpu().numpy().tobytes() == data


def test_lifecycle(gpu, made):
    data, stream, wbits, one = made["text_200k_w15"]
    other = made["runs_300k_w18"]
    lib = gpu.load_library()
    n, chunk = len(data), chunk_of(len(data), wbits)
    src = arr_of(stream)
    raw = (C.c_uint64 * 1)(n)
    buf = np.zeros(n, dtype=np.uint8)
    done, fin, total = (C.c_uint64 * 1)(), C.c_int(0), C.c_uint64(0)
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == E_ARG           # no set is open
    assert lib.nlzm_hip_decode_begin(src.ctypes.data, src.size, 1, None, raw, 0) == 0, lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_decode_fetch(0, 10, buf.ctypes.data) == E_ARG                     # nothing decoded yet
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == 0 and done[0] == chunk
    assert lib.nlzm_hip_decode_step(1, None, done, None, None) == E_ARG
    assert lib.nlzm_hip_decode_fetch(chunk - 5, 10, buf.ctypes.data) == E_ARG             # five bytes of it are not decoded yet
    assert lib.nlzm_hip_decode_fetch(n - 5, 10, buf.ctypes.data) == E_ARG                 # runs over the end
    assert lib.nlzm_hip_decode_fetch(n + 1, 0, buf.ctypes.data) == E_ARG
    assert lib.nlzm_hip_decode_fetch(1, ALL, buf.ctypes.data) == E_ARG                    # (off + len wraps)
    assert lib.nlzm_hip_decode_fetch(3, chunk - 3, buf.ctypes.data) == 0 and buf[:chunk - 3].tobytes() == data[3:chunk]
    assert lib.nlzm_hip_decode_finish(None, C.byref(total)) == E_ARG                      # before the end: refused, the set stays open
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == 0 and done[0] == 2 * chunk
    lib.nlzm_hip_decode_abandon()                                                         # in the middle
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == E_ARG
    assert gpu.decompress(other[1]) == other[0]
    # begin twice: the second closes the first
    assert lib.nlzm_hip_decode_begin(src.ctypes.data, src.size, 1, None, raw, 0) == 0
    assert lib.nlzm_hip_decode_step(3, None, done, C.byref(fin), None) == 0 and done[0] == 3 * chunk
    assert lib.nlzm_hip_decode_begin(src.ctypes.data, src.size, 1, None, None, 0) == 0     # (sized by the library)
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == 0 and done[0] == chunk and gpu.counter("decode_steps") == 1
    # flags: only MORE, only on the _dev form, only for one stream; a failing begin leaves no set open
    assert lib.nlzm_hip_decode_begin(src.ctypes.data, src.size, 1, None, raw, gpu.DECODE_MORE) == E_ARG
    assert lib.nlzm_hip_decode_step(1, None, done, C.byref(fin), None) == E_ARG
    d_src = dev(src)
    for nb, flags in ((1, 2), (1, 4), (2, gpu.DECODE_MORE)):
        two = (C.c_uint64 * 2)(n, 0)
        assert lib.nlzm_hip_decode_begin_dev(d_src.data_ptr(), src.size, nb, None, two, None, 0, flags) == E_ARG, (nb, flags)
    assert lib.nlzm_hip_decode_begin_dev(d_src.data_ptr(), src.size, 2, None, None, None, 0, 0) == E_ARG       # two blocks need their lengths
    assert lib.nlzm_hip_decode_begin_dev(None, 8, 1, None, None, None, 0, 0) == E_ARG
    lib.nlzm_hip_decode_abandon()                                                         # nothing open: still fine
    assert gpu.counter("decode_state_bytes") >= 18 * 64 * 2


def test_decoder_read_walks_forward(gpu, five):
    data, ranges, streams = five
    blob, lens, raws = b"".join(streams), [len(s) for s in streams], [hi - lo for lo, hi in ranges]
    chunk = chunk_of(raws[2], 18)
    s2 = ranges[2][0]
    with gpu.Decoder(blob, BLOCKS_K, lens, raws) as d:
        assert d.read(s2 + 10, 1000) == data[s2 + 10:s2 + 1010]
        assert d.done == [0, 0, chunk, 0, 0] and gpu.counter("decode_steps") == 1
        first = gpu.counter("decode_syms")
        assert d.read(s2 + 20, 500) == data[s2 + 20:s2 + 520] and gpu.counter("decode_steps") == 1     # decoded already: no launch
        assert d.read(s2 + chunk + 5, 1000) == data[s2 + chunk + 5:s2 + chunk + 1005]
        assert d.done == [0, 0, 2 * chunk, 0, 0] and gpu.counter("decode_steps") == 2
        both = gpu.counter("decode_syms")
        # one read that spans two blocks: block 2 to its end, block 3 to its first boundary
        s3 = ranges[3][0]
        assert d.read(s3 - 100, 200) == data[s3 - 100:s3 + 100]
        assert d.done == [0, 0, raws[2], chunk_of(raws[3], 18), 0] and gpu.counter("decode_steps") == 3 and not d.finished
        done, finished = d.step()
        assert done == raws and finished and d.read(0, len(data)) == data
    # the second read did not start over: a decoder that goes to the second boundary in ONE launch decodes the same symbols in all
    with gpu.Decoder(blob, BLOCKS_K, lens, raws) as d:
        d.read(s2 + chunk + 5, 1000)
        assert d.done == [0, 0, 2 * chunk, 0, 0] and gpu.counter("decode_steps") == 1
        assert first < both == gpu.counter("decode_syms")
        with pytest.raises(ValueError):
            d.read(len(data) - 5, 10)


def test_cli_steps(gpu, tmp_path):
    data = corpus.mixed(1_500_000, corpus.SEED + 41)
    src, f = tmp_path / "in.bin", tmp_path / "four.nlzm"
    data.tofile(src)
    r = subprocess.run([nlzm_amd.CLI_PATH, "-window:20", "-blocks:4", "-crc", "c", str(src), str(f)], capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "four.nlzm.idx").read_text().startswith("NLZMIDX 2 4 "), r.stdout + r.stderr

    def lines(out):
        return [re.sub(r"[\d.]+ sec", "T sec", l) for l in out.splitlines()]

    a, b = tmp_path / "plain.out", tmp_path / "steps.out"
    plain = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "d", str(f), str(a)], capture_output=True, text=True)
    steps = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "-steps:4", "d", str(f), str(b)], capture_output=True, text=True)
    assert plain.returncode == 0 and steps.returncode == 0, plain.stdout + steps.stdout + steps.stderr
    assert a.read_bytes() == b.read_bytes() == data.tobytes()
    extra = [l for l in lines(steps.stdout) if l.startswith("Steps: ")]
    assert len(extra) == 1 and re.fullmatch(r"Steps: 4 frames, [1-9]\d* launches", extra[0]), steps.stdout
    assert [l for l in lines(steps.stdout) if not l.startswith("Steps: ")] == lines(plain.stdout)
    assert "CRC32 ok (4 blocks)" in steps.stdout
    plain = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "t", str(f)], capture_output=True, text=True)
    steps = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "-steps:4", "t", str(f)], capture_output=True, text=True)
    assert plain.returncode == 0 and steps.returncode == 0, plain.stdout + steps.stdout + steps.stderr
    assert [l for l in lines(steps.stdout) if not l.startswith("Steps: ")] == lines(plain.stdout) and "CRC32 ok (4 blocks)" in steps.stdout
    assert sum(l.startswith("Steps: 4 frames, ") for l in lines(steps.stdout)) == 1
    # the flag is for d -gpu and t -gpu
    for argv in (["-steps:4", "t", str(f)], ["-gpu", "-steps:4", "h", str(f)], ["-gpu", "-steps:0", "t", str(f)]):
        r = subprocess.run([nlzm_amd.CLI_PATH] + argv, capture_output=True, text=True)
        assert r.returncode != 0 and "Steps:" not in r.stdout, argv
