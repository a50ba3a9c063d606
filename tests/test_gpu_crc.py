"""GPU suite (-m gpu): the device CRC32 through the C ABI, the binding and the command line, against zlib.crc32; checking a block container
against CRCs without its original.  Only streams a compressor made are handed to the device, as in tests/test_gpu_decode.py."""
import ctypes as C
import re
import zlib

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus, shard
from tests.cli_tools import cli

pytestmark = pytest.mark.gpu

E_ARG = -1
STATUS_CRC = 256 - 4


def seeded(n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    t = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    return t


def crc_dev(lib, t, off, n, seed=0):
    out = C.c_uint32(0xDEADBEEF)
    assert lib.nlzm_hip_crc32_dev(t.data_ptr() + off, n, seed, C.byref(out)) == 0, lib.nlzm_hip_last_error()
    return out.value


def test_crc32_dev_against_zlib(gpu):
    """sizes round a chunk, a wave's step and a segment, ten million and a thousand million bytes; the device pointer moved off its alignment;
    seeds chain as zlib's do.  The bytes are made on the device and copied back for zlib."""
    lib = gpu.load_library()
    G = gpu.counter("crc_segment_bytes")
    big = 1_000_000_000
    t = seeded(big + 16, corpus.SEED + 50)
    host = t.cpu().numpy()
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, G - 1, G, G + 1, 10_000_019, big):
        assert crc_dev(lib, t, 0, n) == zlib.crc32(host[:n]), n
    assert gpu.counter("crc_bytes") == big and gpu.counter("crc_us") > 0
    for n in (17, G + 1, 10_000_019):
        for off in (1, 7, 13):
            assert crc_dev(lib, t, off, n) == zlib.crc32(host[off:off + n]), (n, off)
    for cut, n in ((0, 1000), (1, 1000), (3 * G + 5, 5 * G + 77), (10_000_019, 20_000_000)):
        a = crc_dev(lib, t, 0, cut)
        assert crc_dev(lib, t, cut, n - cut, a) == zlib.crc32(host[:n]), (cut, n)
    out = C.c_uint32(0)
    assert lib.nlzm_hip_crc32_dev(None, 8, 0, C.byref(out)) == E_ARG and lib.nlzm_hip_crc32_dev(t.data_ptr(), 8, 0, None) == E_ARG
    # the host-buffer form and the binding
    assert gpu.crc32(host[:300_001].tobytes()) == zlib.crc32(host[:300_001])
    assert gpu.crc32(b"") == 0 and gpu.crc32(b"abc", 5) == zlib.crc32(b"abc", 5)


def test_crc32_ranges_dev(gpu):
    lib = gpu.load_library()
    n, k = 64_000_000, 32
    t = seeded(n, corpus.SEED + 51)
    host = t.cpu().numpy()

    def ranges_dev(ranges, buf_len=n):
        m = len(ranges)
        off, ln, out = (C.c_uint64 * m)(*[o for o, _ in ranges]), (C.c_uint64 * m)(*[l for _, l in ranges]), (C.c_uint32 * m)()
        rc = lib.nlzm_hip_crc32_ranges_dev(t.data_ptr(), buf_len, m, off, ln, out)
        return rc, list(out)

    part = [shard.block_range(n, k, i) for i in range(k)]
    rc, got = ranges_dev([(lo, hi - lo) for lo, hi in part])
    assert rc == 0, lib.nlzm_hip_last_error()
    assert got == [zlib.crc32(host[lo:hi]) for lo, hi in part]
    whole = 0
    for c, (lo, hi) in zip(got, part):
        whole = gpu.crc32_combine(whole, c, hi - lo)
    assert whole == zlib.crc32(host) == crc_dev(lib, t, 0, n)
    # 50 odd ranges: empty ones, overlapping ones, one that ends at buf_len exactly
    rng = np.random.default_rng(corpus.SEED + 52)
    odd = [(n - 12_345, 12_345), (n, 0), (0, 0), (77, 1), (1_000_001, 3_000_003), (1_000_002, 3_000_003)]
    while len(odd) < 50:
        off = int(rng.integers(0, n))
        odd.append((off, int(rng.integers(0, min(n - off, 2_000_000 if len(odd) % 4 else 300) + 1))))
    rc, got = ranges_dev(odd)
    assert rc == 0, lib.nlzm_hip_last_error()
    assert got == [zlib.crc32(host[o:o + l]) for o, l in odd]
    assert gpu.crc32_ranges(host[:100_000].tobytes(), [(5, 70_000), (99_999, 1), (100_000, 0)]) == [zlib.crc32(host[5:70_005]), zlib.crc32(host[99_999:100_000]), 0]
    # refused, not followed: a range that runs over the buffer, a pair whose sum wraps, null arrays
    assert ranges_dev([(0, 10), (n - 5, 6)])[0] == E_ARG
    assert ranges_dev([(n + 1, 0)])[0] == E_ARG
    assert ranges_dev([((1 << 64) - 8, 16)])[0] == E_ARG and ranges_dev([(16, (1 << 64) - 8)])[0] == E_ARG
    assert lib.nlzm_hip_crc32_ranges_dev(t.data_ptr(), n, 1, None, None, None) == E_ARG


def test_feed_input_crc32(gpu):
    lib = gpu.load_library()
    data = np.random.default_rng(corpus.SEED + 53).integers(0, 64, 3_000_000, dtype=np.uint8)
    crc = C.c_uint32(0)
    assert lib.nlzm_hip_feed_input_crc32(C.byref(crc)) == E_ARG           # no feed
    buf, got = np.empty(1 << 20, dtype=np.uint8), C.c_uint64(0)

    def drain():
        while True:
            assert lib.nlzm_hip_feed_output(buf.ctypes.data, buf.size, C.byref(got)) == 0, lib.nlzm_hip_last_error()
            if not got.value:
                return

    assert lib.nlzm_hip_feed_begin(data.size, 20) == 0, lib.nlzm_hip_last_error()
    try:
        for lo in range(0, data.size, 1 << 20):
            assert lib.nlzm_hip_feed(data[lo:].ctypes.data, min(1 << 20, data.size - lo)) == 0, lib.nlzm_hip_last_error()
            drain()
        assert lib.nlzm_hip_feed_input_crc32(C.byref(crc)) == E_ARG       # fed, but not finished
        assert lib.nlzm_hip_feed_finish() == 0, lib.nlzm_hip_last_error()
        drain()
        assert lib.nlzm_hip_feed_input_crc32(None) == E_ARG
        assert lib.nlzm_hip_feed_input_crc32(C.byref(crc)) == 0, lib.nlzm_hip_last_error()
        assert crc.value == zlib.crc32(data)
    finally:
        lib.nlzm_hip_feed_end()
    assert lib.nlzm_hip_feed_input_crc32(C.byref(crc)) == E_ARG           # ended


def test_check_dev_on_a_block_container(gpu):
    lib = gpu.load_library()
    k = 6
    data = corpus.mixed(900_000, corpus.SEED + 54)
    raw = data.tobytes()
    ranges = [shard.block_range(data.size, k, i) for i in range(k)]
    streams = gpu.compress_blocks(data, k, 18)
    crcs = [zlib.crc32(raw[lo:hi]) for lo, hi in ranges]
    raws = [hi - lo for lo, hi in ranges]
    assert raws[2] == raws[3]

    def check(streams, crcs, with_raw):
        blob = np.frombuffer(b"".join(streams), dtype=np.uint8)
        d = torch.from_numpy(blob.copy()).to("cuda:0")
        torch.cuda.synchronize()
        blen, want, out = (C.c_uint64 * k)(*map(len, streams)), (C.c_uint32 * k)(*crcs), (C.c_uint32 * k)()
        rl = (C.c_uint64 * k)(*raws) if with_raw else None
        bad = C.c_uint32(99)
        assert lib.nlzm_hip_check_dev(d.data_ptr(), blob.size, k, blen, rl, want, C.byref(bad), out) == 0, lib.nlzm_hip_last_error()
        return bad.value, list(out)

    swapped = streams[:2] + [streams[3], streams[2]] + streams[4:]      # both streams intact: nothing malformed reaches the GPU
    for with_raw in (True, False):
        assert check(streams, crcs, with_raw) == (k, crcs)
        wrong = list(crcs)
        wrong[4] ^= 1
        assert check(streams, wrong, with_raw) == (4, crcs)
        bad, out = check(swapped, crcs, with_raw)
        assert bad == 2 and out == crcs[:2] + [crcs[3], crcs[2]] + crcs[4:]
    assert gpu.counter("crc_bytes") == data.size
    # the binding, host buffers: block lengths found by the frame headers
    assert gpu.check(b"".join(streams), crcs, k, raws) == k and gpu.check(b"".join(streams), crcs, k) == k
    assert gpu.check(b"".join(swapped), crcs, k) == 2
    assert gpu.check(streams[0], crcs[:1]) == 1 and gpu.check(streams[0], [crcs[0] ^ 2]) == 0
    # a length that is not the block's is a bad block too
    assert gpu.check(b"".join(streams), crcs, k, [raws[0] - 1, raws[1] + 1] + raws[2:]) == 0
    bad = C.c_uint32(0)
    assert lib.nlzm_hip_check_dev(None, 8, 1, None, None, (C.c_uint32 * 1)(), C.byref(bad), None) == E_ARG


def test_cli_crc(gpu, tmp_path):
    k = 6
    data = corpus.mixed(900_000, corpus.SEED + 55)
    raw = data.tobytes()
    src = tmp_path / "in.bin"
    data.tofile(src)

    plain, with_crc = tmp_path / "plain.nlzm", tmp_path / "crc.nlzm"
    r = cli("-window:18", f"-blocks:{k}", "c", src, plain)
    assert r.returncode == 0, r.stdout + r.stderr
    r = cli("-window:18", f"-blocks:{k}", "-crc", "c", src, with_crc)
    assert r.returncode == 0 and f"Done (input CRC32 {zlib.crc32(raw):X}," in r.stdout, r.stdout + r.stderr
    # without the flag: the same container and the index of version 1
    assert plain.read_bytes() == with_crc.read_bytes()
    idx1 = (tmp_path / "plain.nlzm.idx").read_text().splitlines()
    idx2 = (tmp_path / "crc.nlzm.idx").read_text().splitlines()
    assert idx1[0] == f"NLZMIDX 1 {k} {data.size} {plain.stat().st_size}" and all(len(l.split()) == 3 for l in idx1[1:]) and len(idx1) == k + 1
    ranges = [shard.block_range(data.size, k, i) for i in range(k)]
    assert idx2[0] == f"{idx1[0].replace('NLZMIDX 1', 'NLZMIDX 2')} {zlib.crc32(raw):08X}"
    assert idx2[1:] == [f"{l} {zlib.crc32(raw[lo:hi]):08X}" for l, (lo, hi) in zip(idx1[1:], ranges)]
    for flags in ([], ["-gpu"]):
        r = cli(*flags, "t", with_crc)
        assert r.returncode == 0 and f"CRC32 ok ({k} blocks)" in r.stdout and f"output CRC32 {zlib.crc32(raw):X}," in r.stdout, r.stdout + r.stderr
    out = tmp_path / "back.bin"
    r = cli("-gpu", "d", with_crc, out)
    assert r.returncode == 0 and f"CRC32 ok ({k} blocks)" in r.stdout and out.read_bytes() == raw, r.stdout + r.stderr
    # one CRC of the index edited: both paths say which block and exit with the status of their own
    lines = list(idx2)
    f = lines[4].split()
    f[3] = f"{int(f[3], 16) ^ 0x100:08X}"
    lines[4] = " ".join(f)
    (tmp_path / "crc.nlzm.idx").write_text("\n".join(lines) + "\n")
    for flags in ([], ["-gpu"]):
        r = cli(*flags, "t", with_crc)
        assert r.returncode == STATUS_CRC and "CRC32 MISMATCH in block 4 " in r.stdout, (flags, r.returncode, r.stdout + r.stderr)
    # one stream: the CRC comes from the feed's device buffer, the index has one block
    one = tmp_path / "one.nlzm"
    r = cli("-window:18", "-crc", "c", src, one)
    assert r.returncode == 0 and f"Done (input CRC32 {zlib.crc32(raw):X}," in r.stdout, r.stdout + r.stderr
    c = f"{zlib.crc32(raw):08X}"
    assert (tmp_path / "one.nlzm.idx").read_text().splitlines() == [f"NLZMIDX 2 1 {data.size} {one.stat().st_size} {c}", f"0 {one.stat().st_size} {data.size} {c}"]
    for flags in ([], ["-gpu"]):
        r = cli(*flags, "t", one)
        assert r.returncode == 0 and "CRC32 ok (1 blocks)" in r.stdout, r.stdout + r.stderr
    one2 = tmp_path / "one2.nlzm"
    r = cli("-window:18", "c", src, one2)
    assert r.returncode == 0 and one2.read_bytes() == one.read_bytes() and not (tmp_path / "one2.nlzm.idx").exists(), r.stdout
    # h -gpu prints what h prints
    a, b = cli("h", src), cli("-gpu", "h", src)
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and a.stdout.splitlines()[-1] == f"{zlib.crc32(raw):X}", a.stdout + b.stdout
