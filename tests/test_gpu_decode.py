"""GPU suite (-m gpu): the device decoder through the C ABI, the binding and the command line.  Only streams a compressor made are
handed to the GPU (damaged streams are the CPU suite's business: tests/test_decode_sim.py); errors in arguments are fine here.
The file decodes much and compresses little: the oracle makes the streams of item 1 on eight host threads while the GPU works."""
import ctypes as C
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cases, oracle_py

pytestmark = pytest.mark.gpu

E_CAPACITY = -4
ALL = cases.CASES + cases.BIG_CASES


@pytest.fixture(scope="module")
def streams():
    """every case's reference stream, made by the oracle on host threads (the slow direction: started once, collected per test)"""
    ex = ThreadPoolExecutor(8)
    inputs = {c[0]: cases.make_case(c).copy() for c in ALL}         # (made here: make_case keeps one input and is not for threads)
    futs = {c[0]: ex.submit(oracle_py.compress, inputs[c[0]], c[4]) for c in sorted(ALL, key=lambda c: -c[2])}
    yield futs
    ex.shutdown(wait=False, cancel_futures=True)


def dev(arr, pad=0):
    t = torch.zeros(max(1, arr.size + pad), dtype=torch.uint8, device="cuda:0")
    if arr.size:
        t[:arr.size].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    torch.cuda.synchronize()
    return t


def arr_of(b):
    return np.frombuffer(b, dtype=np.uint8)


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_reference_stream_decodes(gpu, streams, case):
    """decode_file replacement (NLZM.cpp:1912-2039) on the reference's stream: the input comes back, the size query gives its length"""
    stream = streams[case[0]].result()
    data = cases.make_case(case).tobytes()
    lib = gpu.load_library()
    n = C.c_uint64(12345)
    assert lib.nlzm_hip_decompress(stream, len(stream), None, 0, C.byref(n)) == 0, lib.nlzm_hip_last_error()
    assert n.value == case[2]
    assert gpu.decompress(stream) == data


def test_dst_cap_too_small(gpu, streams):
    case = next(c for c in cases.CASES if c[0] == "text_300k_w20")
    stream = streams[case[0]].result()
    size = case[2]
    d_src = dev(arr_of(stream))
    d_dst = torch.full((size,), 0xC3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lib = gpu.load_library()
    n = C.c_uint64(0)
    assert lib.nlzm_hip_decompress_dev(d_src.data_ptr(), len(stream), d_dst.data_ptr(), size - 1, C.byref(n)) == E_CAPACITY
    torch.cuda.synchronize()
    assert int(d_dst[size - 1]) == 0xC3
    assert lib.nlzm_hip_decompress_dev(d_src.data_ptr(), len(stream), d_dst.data_ptr(), size, C.byref(n)) == 0, lib.nlzm_hip_last_error()
    assert n.value == size and d_dst.cpu().numpy().tobytes() == cases.make_case(case).tobytes()
    # null arguments are refused, not followed
    assert lib.nlzm_hip_decompress_dev(None, 8, None, 0, C.byref(n)) == -1
    assert lib.nlzm_hip_verify_dev(d_src.data_ptr(), len(stream), 0, None, d_dst.data_ptr(), size, C.byref(n), C.byref(n)) == -1
    assert lib.nlzm_hip_verify_dev(d_src.data_ptr(), len(stream), 1, None, d_dst.data_ptr(), size, C.byref(n), None) == -1


def test_block_set_at_bench_geometry(gpu):
    """bench.py's block-mode geometry (32 x 17 MB, -window:28): compressed in block mode, decoded 32 workgroups at once with and without
    the lengths, compared on the device; verify says equal, and names the offset after one byte of the ORIGINAL's copy is flipped."""
    name, kind, size, seed_off, wbits, k = cases.BLOCK_SET
    data = cases.make_case(cases.BLOCK_SET[:5])
    lib = gpu.load_library()
    d_in = dev(data, 4096)
    cap = int(lib.nlzm_hip_compress_bound(size)) + k * (16 + 131072)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    blen, total = (C.c_uint64 * k)(), C.c_uint64(0)
    assert lib.nlzm_hip_compress_blocks_dev(d_in.data_ptr(), size, k, wbits, d_out.data_ptr(), cap, blen, C.byref(total)) == 0, lib.nlzm_hip_last_error()
    want_raw = [hi - lo for lo, hi in (shard.block_range(size, k, i) for i in range(k))]
    raw_in = (C.c_uint64 * k)(*want_raw)
    for lens, raws in ((blen, raw_in), (None, None)):
        d_back = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
        raw_out, n = (C.c_uint64 * k)(), C.c_uint64(0)
        torch.cuda.synchronize()
        rc = lib.nlzm_hip_decompress_blocks_dev(d_out.data_ptr(), total.value, k, lens, raws, d_back.data_ptr(), size, raw_out, C.byref(n))
        assert rc == 0, lib.nlzm_hip_last_error()
        torch.cuda.synchronize()
        assert n.value == size and list(raw_out) == want_raw
        assert bool(torch.equal(d_back, d_in[:size]))
        del d_back
    assert gpu.counter("decode_streams") == k and gpu.counter("decode_out_bytes") == size
    first, dlen = C.c_uint64(0), C.c_uint64(0)
    assert lib.nlzm_hip_verify_dev(d_out.data_ptr(), total.value, k, blen, d_in.data_ptr(), size, C.byref(first), C.byref(dlen)) == 0, lib.nlzm_hip_last_error()
    assert first.value == size and dlen.value == size
    assert gpu.counter("decode_passes") == 1            # (the partition is the compressor's: no size pass)
    at = 13 * 17_000_000 + 4_321
    d_in[at] ^= 0x10
    torch.cuda.synchronize()
    assert lib.nlzm_hip_verify_dev(d_out.data_ptr(), total.value, k, None, d_in.data_ptr(), size, C.byref(first), C.byref(dlen)) == 0, lib.nlzm_hip_last_error()
    assert first.value == at and dlen.value == size
    # a wrong length is a mismatch at the shorter length -- and when it is the ORIGINAL that is shorter, that offset is n itself, the value
    # that also means "equal": the decoded length is what must give it away
    short = at - 100
    assert lib.nlzm_hip_verify_dev(d_out.data_ptr(), total.value, k, blen, d_in.data_ptr(), short, C.byref(first), C.byref(dlen)) == 0, lib.nlzm_hip_last_error()
    assert first.value == short and dlen.value == size != short
    with pytest.raises(gpu.LengthMismatch):
        gpu.verify_verdict(first.value, dlen.value, short)


def test_block_sets_small(gpu):
    """64 blocks; fewer bytes than blocks (trailing blocks are empty streams), a last block shorter than the others, one block"""
    for n, k in ((2_000_000, 64), (5, 4), (3, 8), (300_001, 7), (70_000, 1)):
        data = corpus.syn_text(n, corpus.SEED + n)
        blob = b"".join(gpu.compress_blocks(data, k, 17))
        got = gpu.decompress_blocks(blob, k)
        assert [len(g) for g in got] == [hi - lo for lo, hi in (shard.block_range(n, k, i) for i in range(k))], (n, k)
        assert b"".join(got) == data.tobytes(), (n, k)
        assert gpu.verify(blob, data, k) == n
        if n > 100:
            bad = data.copy()
            bad[n // 2] ^= 1
            assert gpu.verify(blob, bad, k) == n // 2
            # the original longer than what the container holds: a mismatch where the decode ends; shorter: never "equal"
            assert gpu.verify(blob, np.concatenate([data, data[:9]]), k) == n
            with pytest.raises(gpu.LengthMismatch):
                gpu.verify(blob, data[:n - 7], k)
    with pytest.raises(gpu.LengthMismatch):                # (n = 0 against a stream that is not empty)
        gpu.verify(blob, data[:0], k)


def test_single_stream_no_golden_file_pins(gpu):
    """10 MB of the image's own source text where it is there, else of wiki-shaped markup: compressed and verified on the device, nothing but
    the verdict leaves it -- the reference-free necessary condition (the stream decodes to the input) at any size, on any bytes."""
    try:
        data = corpus.make("real_text", 10_000_000)
    except RuntimeError:
        data = corpus.make("xml_like", 10_000_000, corpus.SEED + 33)
    lib = gpu.load_library()
    d_in = dev(data, 4096)
    cap = int(lib.nlzm_hip_compress_bound(data.size))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    n, first, dlen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    torch.cuda.synchronize()
    assert lib.nlzm_hip_compress_dev(d_in.data_ptr(), data.size, 24, d_out.data_ptr(), cap, C.byref(n)) == 0, lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_verify_dev(d_out.data_ptr(), n.value, 1, None, d_in.data_ptr(), data.size, C.byref(first), C.byref(dlen)) == 0, lib.nlzm_hip_last_error()
    assert first.value == data.size and dlen.value == data.size


def test_cli_verify_and_gpu_decode(gpu, tmp_path):
    data = corpus.mixed(1_500_000, corpus.SEED + 41)
    src = tmp_path / "in.bin"
    data.tofile(src)
    one, five = tmp_path / "one.nlzm", tmp_path / "five.nlzm"
    r = subprocess.run([nlzm_amd.CLI_PATH, "-window:20", "-verify", "c", str(src), str(one)], capture_output=True, text=True)
    assert r.returncode == 0 and "Verified" in r.stdout, r.stdout + r.stderr
    assert one.read_bytes() == oracle_py.compress(data, 20)
    r = subprocess.run([nlzm_amd.CLI_PATH, "-window:20", "-blocks:5", "-verify", "c", str(src), str(five)], capture_output=True, text=True)
    assert r.returncode == 0 and "Verified" in r.stdout, r.stdout + r.stderr
    for f in (one, five):
        a, b = tmp_path / (f.name + ".gpu"), tmp_path / (f.name + ".host")
        r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "d", str(f), str(a)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([nlzm_amd.CLI_PATH, "d", str(f), str(b)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert a.read_bytes() == b.read_bytes() == data.tobytes()
        crc = [re.search(r"output CRC32 ([0-9A-F]+)", subprocess.run([nlzm_amd.CLI_PATH] + flag + ["t", str(f)], capture_output=True, text=True).stdout).group(1)
               for flag in ([], ["-gpu"])]
        assert crc[0] == crc[1] == f"{oracle_py.crc32(data):X}"
    # without its index the container is split by its frame headers, on the device path too
    # an index that passes every check of its own and asks for 2^60 bytes of output: wrong, not fatal -- the frame headers decide
    idx = tmp_path / "five.nlzm.idx"
    lines = idx.read_text().split("\n")
    head, rows = lines[0].split(), [l.split() for l in lines[1:] if l]
    huge = 1 << 60
    rows[0][2] = str(huge - sum(int(r[2]) for r in rows[1:]))
    idx.write_text("\n".join([" ".join(head[:3] + [str(huge), head[4]])] + [" ".join(r) for r in rows]) + "\n")
    h = tmp_path / "five.hugeidx"
    r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "d", str(five), str(h)], capture_output=True, text=True)
    assert r.returncode == 0 and "does not describe" in r.stdout and h.read_bytes() == data.tobytes(), r.stdout + r.stderr
    idx.unlink()
    c = tmp_path / "five.noidx"
    r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "d", str(five), str(c)], capture_output=True, text=True)
    assert r.returncode == 0 and "Blocks: 5" in r.stdout and c.read_bytes() == data.tobytes(), r.stdout


@pytest.mark.parametrize("name", ["text_300k_w20", "random_100k_w15"])
def test_counters_are_the_oracles(gpu, streams, name):
    case = next(c for c in cases.CASES if c[0] == name)
    _, ost = oracle_py.compress(cases.make_case(case), case[4], want_stats=True)
    assert gpu.decompress(streams[name].result()) == cases.make_case(case).tobytes()
    for key, okey in (("decode_syms", "rans_syms"), ("decode_raw_ops", "bit_ops"), ("decode_n_literal", "n_literal"), ("decode_n_dict", "n_dict"),
                      ("decode_n_rep", "n_rep")):
        assert gpu.counter(key) == ost[okey], key
    assert gpu.counter("decode_out_bytes") == case[2] and gpu.counter("decode_cycles") > 0
