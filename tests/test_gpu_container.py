"""GPU suite (-m gpu): containers of more blocks than one persistent launch holds -- compressed in sets one after another
(nlzm_hip_compress_blocks*, nlzm_container_plan.h) -- and the one-shot decoder's small-ring kernel (decode_small_kernel), which takes over
when a launch has more streams than the 64 KiB kernel holds at once.  Every compressed block is compared with the oracle's stream of its byte
range; only well-formed streams go to the device."""
import ctypes as C
import json
import os
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cases, oracle_py
from tests.test_decode_small_ring_sim import REACH, stream_input

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "decode_small_ring.json")))
BIG, SMALL = 65536, 16384


def oracle_blocks(data, nblocks, hist_bits):
    """the reference run on every block's byte range (host threads)"""
    ranges = [shard.block_range(data.size, nblocks, i) for i in range(nblocks)]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda r: oracle_py.compress(data[r[0]:r[1]], hist_bits), ranges))


def set_sizes(nblocks, set_blocks):
    nsets = -(-nblocks // set_blocks)
    return [nblocks // nsets + (1 if s < nblocks % nsets else 0) for s in range(nsets)]


@pytest.fixture(scope="module")
def mixed(gpu):
    data = corpus.mixed(600_000)
    return data, {k: oracle_blocks(data, k, 16) for k in (64, 65, 70, 130)}


@pytest.fixture()
def options(gpu):
    """the options this file touches, back at their defaults afterwards"""
    yield gpu
    gpu.set_option("container_set_blocks", 32)
    gpu.set_option("decode_ring", 0)


@pytest.mark.parametrize("nblocks,set_blocks,sizes", [(70, None, [24, 23, 23]), (130, 64, [44, 43, 43])])
def test_sets_by_default(options, mixed, nblocks, set_blocks, sizes):
    gpu = options
    data, want = mixed
    if set_blocks:
        gpu.set_option("container_set_blocks", set_blocks)
    assert set_sizes(nblocks, set_blocks or 32) == sizes
    got = gpu.compress_blocks(data, nblocks, 16)
    bad = [i for i in range(nblocks) if got[i] != want[nblocks][i]]
    assert not bad, f"blocks {bad[:10]} differ from the oracle's"
    assert gpu.counter("container_sets") == 3
    st = gpu.stats()
    assert st["in_bytes"] == data.size and st["out_bytes"] == sum(len(s) for s in got)
    assert gpu.counter("block_redo_streams") == 0 and gpu.counter("block_pool_bytes") > 0


def test_pool_is_the_largest_sets(options, mixed):
    """"block_pool_bytes" after a container is what its largest set took: the allocation grows to the set that needs most and is never shrunk.  That
    need not be the set with the most blocks -- 23 streams get a worker CU more each than 24 do (CUs / streams), and their buffers grow with it -- so
    the container's figure is held to the larger of its first set (24 blocks) and its second (23) compressed alone; the third is the second with a
    shorter last block.  (The allocation a call before left behind is dropped first each time: a kept one that fits is used again as it is.)"""
    gpu = options
    data, _ = mixed

    def pool_after(part, nblocks):
        gpu.set_option("keep_block_pool", 0)
        gpu.set_option("keep_block_pool", 1)
        assert gpu.counter("block_pool_bytes") == 0
        gpu.compress_blocks(part, nblocks, 16)
        return gpu.counter("block_pool_bytes")

    per = -(-data.size // 70)
    whole, first, second = pool_after(data, 70), pool_after(data[:24 * per], 24), pool_after(data[24 * per:47 * per], 23)
    assert gpu.counter("container_sets") == 1
    print(f"block_pool_bytes: container {whole}, first set alone {first}, second set alone {second}")
    assert whole == max(first, second) > 0
    # with the option off the sets still share one allocation, which goes when the call ends
    gpu.set_option("keep_block_pool", 0)
    try:
        got = gpu.compress_blocks(data, 70, 16)
        assert gpu.counter("container_sets") == 3 and gpu.counter("block_pool_bytes") == 0
        assert got == mixed[1][70]
    finally:
        gpu.set_option("keep_block_pool", 1)


def test_boundary(options, mixed):
    gpu = options
    data, want = mixed
    got = gpu.compress_blocks(data, 64, 16)                  # one launch holds them: today's path, ONE set whatever the option says
    assert got == want[64] and gpu.counter("container_sets") == 1
    gpu.set_option("container_set_blocks", 64)
    got = gpu.compress_blocks(data, 65, 16)
    assert set_sizes(65, 64) == [33, 32]
    assert got == want[65] and gpu.counter("container_sets") == 2
    assert gpu.stats()["in_bytes"] == data.size


@pytest.mark.parametrize("n,nblocks", [(100, 70), (100, 200), (0, 70)])
def test_ragged(options, n, nblocks):
    """fewer bytes than blocks: the trailing blocks are empty streams, and whole sets consist of them (n = 100, 200 blocks: one byte a block, 100
    empty ones -- sets of 29, 29, 29, 29, 28, 28, 28, the last three empty altogether and one half so)"""
    gpu = options
    data = corpus.syn_text(n) if n else np.zeros(0, dtype=np.uint8)
    got = gpu.compress_blocks(data, nblocks, 16)
    assert len(got) == nblocks
    empty = oracle_py.compress(data[:0], 16)
    for i in range(nblocks):
        lo, hi = shard.block_range(n, nblocks, i)
        assert got[i] == (oracle_py.compress(data[lo:hi], 16) if hi > lo else empty), i
    assert gpu.counter("container_sets") == len(set_sizes(nblocks, 32))
    assert gpu.stats()["in_bytes"] == n


def test_round_trip_at_width(options):
    """600 blocks of 2,000 bytes, made by the oracle on the CPU: one decode launch of 600 streams"""
    gpu = options
    k, n = 600, 1_200_000
    data = corpus.mixed(n, corpus.SEED + 3)
    streams = oracle_blocks(data, k, 16)
    blob = b"".join(streams)
    want_ring = SMALL if k > 2 * torch.cuda.get_device_properties(0).multi_processor_count else BIG
    out = gpu.decompress_blocks(blob, k)
    assert b"".join(out) == data.tobytes()
    assert gpu.counter("decode_ring_size") == want_ring and gpu.counter("decode_streams") == k
    assert gpu.verify(blob, data, k) == n
    assert gpu.counter("decode_ring_size") == want_ring
    crcs = [zlib.crc32(data[lo:hi].tobytes()) for lo, hi in (shard.block_range(n, k, i) for i in range(k))]
    assert gpu.check(blob, crcs, k, [2000] * k) == k
    assert gpu.counter("decode_ring_size") == want_ring
    # 64 streams and fewer are the kernel they have always been
    assert b"".join(gpu.decompress_blocks(b"".join(streams[:64]), 64)) == data[:128_000].tobytes()
    assert gpu.counter("decode_ring_size") == BIG


def decompress_dev(gpu, stream, n, misalign=0):
    """nlzm_hip_decompress_dev into a destination `misalign` bytes off a 256-byte boundary, canaries round it"""
    lib = gpu.load_library()
    d_src = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to("cuda:0")
    d = torch.full((256 + misalign + n + 256,), 0xC3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert d.data_ptr() % 256 == 0
    got = C.c_uint64(0)
    rc = lib.nlzm_hip_decompress_dev(d_src.data_ptr(), d_src.numel(), d.data_ptr() + 256 + misalign, n, C.byref(got))
    torch.cuda.synchronize()
    assert rc == 0, lib.nlzm_hip_last_error()
    h = d.cpu().numpy()
    assert (h[:256 + misalign] == 0xC3).all() and (h[256 + misalign + n:] == 0xC3).all()
    return h[256 + misalign: 256 + misalign + int(got.value)].tobytes()


@pytest.mark.parametrize("name", ["text_200k_w15", "dups_600k_w20", REACH[0]])
def test_forced_small_ring(options, name):
    gpu = options
    data, bits = stream_input(name)
    stream = oracle_py.compress(data, bits)
    gpu.set_option("decode_ring", BIG)
    big = gpu.decompress(stream)
    assert gpu.counter("decode_ring_size") == BIG
    big_bytes = gpu.counter("decode_ring_bytes"), gpu.counter("decode_global_bytes")
    gpu.set_option("decode_ring", SMALL)
    small = gpu.decompress(stream)
    assert gpu.counter("decode_ring_size") == SMALL
    assert small == big == data.tobytes()
    rec = GOLD["streams"][name]
    assert GOLD["ring"] == SMALL
    assert (gpu.counter("decode_ring_bytes"), gpu.counter("decode_global_bytes")) == (rec["ring_bytes"], rec["global_bytes"])
    assert sum(big_bytes) == rec["ring_bytes"] + rec["global_bytes"] and big_bytes[1] <= rec["global_bytes"]
    if name == "text_200k_w15":
        assert decompress_dev(gpu, stream, data.size, misalign=1) == data.tobytes()
        assert gpu.counter("decode_ring_size") == SMALL


def test_ranges_with_either_ring(options):
    """a container of seven blocks of 150,000 bytes of dense text: prefix mode runs on the kernel the option names"""
    gpu = options
    k, per = 7, 150_000
    data = corpus.dense_text(k * per, corpus.SEED + 16)
    streams = oracle_blocks(data, k, 17)
    blob, lens, raws = b"".join(streams), [len(s) for s in streams], [per] * k
    ranges = [(1000, 4096), (3 * per + 70_000, 30_000),                   # inside a block
              (per - 100, 300), (5 * per - 20_000, 40_000),               # across two
              (2 * per - 4096, 4096), (7 * per - 1, 1),                   # ending at a block's last byte
              (4 * per, 0), (0, 0),                                       # empty
              (6 * per, 17_000), (0, 16)]
    raw = data.tobytes()
    want = [raw[o:o + l] for o, l in ranges]
    for ring in (BIG, SMALL):
        gpu.set_option("decode_ring", ring)
        assert gpu.read_ranges(blob, ranges, k, lens, raws) == want, ring
        assert gpu.counter("decode_ring_size") == ring and gpu.counter("range_blocks_decoded") == 6       # (no range touches block 2)


def test_command_line(gpu, tmp_path):
    data = corpus.mixed(600_000)
    src, out = tmp_path / "in.bin", tmp_path / "out.nlzm"
    src.write_bytes(data.tobytes())

    def run(*args):
        r = subprocess.run([nlzm_amd.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    assert "Blocks: 70" in run("-window:16", "-blocks:70", "-crc", "c", src, out)
    idx = open(str(out) + ".idx").read().splitlines()
    assert idx[0].startswith("NLZMIDX 2 70 600000 ") and len(idx) == 1 + 70
    lens, raws, crcs = nlzm_amd.read_index(str(out) + ".idx")
    assert raws == [hi - lo for lo, hi in (shard.block_range(600_000, 70, i) for i in range(70))]
    assert crcs == [zlib.crc32(data[lo:hi].tobytes()) for lo, hi in (shard.block_range(600_000, 70, i) for i in range(70))]
    for flags in ((), ("-gpu",)):
        back = tmp_path / f"back{len(flags)}.bin"
        assert "CRC32 ok" in run(*flags, "d", out, back)
        assert back.read_bytes() == data.tobytes()
        assert "CRC32 ok" in run(*flags, "t", out)
    part = tmp_path / "part.bin"
    assert "CRC32 ok" in run("-range:8000:20000", "-range:599000:1000", "x", out, part)
    assert part.read_bytes() == data.tobytes()[8000:28000] + data.tobytes()[599000:600000]
