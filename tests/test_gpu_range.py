"""GPU suite (-m gpu): byte ranges out of a block container through the C ABI, the binding and the command line.  Only well-formed
streams go to the device (the oracle's, made on host threads); wrong ARGUMENTS are fine here, as in tests/test_gpu_decode.py.  One
container of seven blocks, 1.7 MB decoded, serves every test; the expected bytes are slices of the blocks' inputs."""
import ctypes as C
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from tests import cases, oracle_py

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_FORMAT = -1, -4, -7
BLOCKS = ["dups_600k_w20", "text_300k_w20", "empty", "one_byte", "random_100k_w15", "runs_300k_w18", "xml_400k_w19"]
K = len(BLOCKS)
CANARY = 0xC3


def case_of(name):
    return next(c for c in cases.CASES if c[0] == name)


class Box:
    """the container on the host and on the device, and what a call needs of it"""

    def __init__(self, gpu):
        inputs = [cases.make_case(case_of(n)).copy() for n in BLOCKS]      # (made here: make_case keeps one input and is not for threads)
        with ThreadPoolExecutor(8) as ex:
            self.streams = list(ex.map(lambda i: oracle_py.compress(inputs[i], case_of(BLOCKS[i])[4]), range(K)))
        self.blocks = [a.tobytes() for a in inputs]
        self.data = b"".join(self.blocks)
        self.raws = [len(b) for b in self.blocks]
        self.lens = [len(s) for s in self.streams]
        self.start = [sum(self.raws[:i]) for i in range(K + 1)]
        self.total = self.start[K]
        self.crcs = [zlib.crc32(b) for b in self.blocks]
        self.blob = b"".join(self.streams)
        self.gpu, self.lib = gpu, gpu.load_library()
        self.d_src = torch.from_numpy(np.frombuffer(self.blob, dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()

    def slices(self, ranges):
        return b"".join(self.data[o:o + l] for o, l in ranges)

    def read(self, ranges, lens="given", raws="given", crcs=None, cap_delta=0, src=None, nblocks=K, room=None):
        """one nlzm_hip_read_ranges_dev call into a destination misaligned by 5 bytes between canaries; -> (rc, bytes up to dst_len, dst_len,
        first_bad, canaries intact)"""
        k = len(ranges)
        want = sum(l for _, l in ranges) if room is None else room
        d = torch.full((64 + 5 + want + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        off, ln = (C.c_uint64 * max(1, k))(*[o for o, _ in ranges]), (C.c_uint64 * max(1, k))(*[l for _, l in ranges])
        blen = (C.c_uint64 * nblocks)(*(self.lens if lens == "given" else lens)) if lens is not None else None
        raw = (C.c_uint64 * nblocks)(*(self.raws if raws == "given" else raws)) if raws is not None else None
        crc = (C.c_uint32 * nblocks)(*crcs) if crcs is not None else None
        n, bad = C.c_uint64(12345), C.c_uint32(12345)
        s = self.d_src if src is None else src
        rc = self.lib.nlzm_hip_read_ranges_dev(s.data_ptr(), s.numel(), nblocks, blen, raw, crc, k, off, ln, d.data_ptr() + 64 + 5, max(0, want + cap_delta),
                                               C.byref(n), C.byref(bad))
        torch.cuda.synchronize()
        h = d.cpu().numpy()
        # after a success the canaries start behind *dst_len; after an error behind dst_cap (a block that goes straight into the destination may
        # have written what it decoded before the error showed) -- self.untouched says whether anything at all was written
        got = int(n.value) if rc == 0 else max(0, want + cap_delta)
        intact = bool((h[:69] == CANARY).all() and (h[69 + got:] == CANARY).all())
        self.untouched = bool((h == CANARY).all())
        return rc, h[69:69 + got].tobytes() if rc == 0 else b"", int(n.value), int(bad.value), intact

    def counters(self, *keys):
        return [self.gpu.counter(k) for k in keys]


@pytest.fixture(scope="module")
def box(gpu):
    return Box(gpu)


def test_forty_ranges_in_one_call(box):
    st, T = box.start, box.total
    rng = np.random.default_rng(4242)
    ranges = [(1000, 4096), (st[1] + 10, 299_000),                       # inside a block
              (st[1] - 100, 300), (st[5] - 7, 9),                        # across two blocks
              (st[1] + 299_990, 100_020 + 5),                            # across four: 1, (2), 3, 4, 5 -- and across the empty block
              (st[2] - 1, 3),                                            # block 1's last byte, the empty block, block 3, block 4's first
              (st[4], 500), (st[6], 1), (st[0], 16),                     # starting at a block's first byte
              (st[5] - 500, 500), (st[6] - 1, 1), (st[1] - 4096, 4096),  # ending at a block's last byte
              (0, 0), (T, 0), (st[3], 0), (12345, 0),                    # length 0
              (0, T),                                                    # the whole container
              (T - 1, 1),                                                # the last byte
              (5000, 3000), (6000, 3000), (5500, 100),                   # overlapping
              (st[6] + 77, 1234), (st[6] + 77, 1234), (1000, 4096),      # repeated
              (st[6] + 100_000, 50_000), (st[4] + 3, 1), (st[0] + 590_000, 10_000)]        # unordered
    while len(ranges) < 40:
        off = int(rng.integers(0, T))
        ranges.append((off, int(rng.integers(0, min(T - off, 70_000) + 1))))
    rc, got, n, bad, intact = box.read(ranges)
    assert rc == 0, box.lib.nlzm_hip_last_error()
    assert n == sum(l for _, l in ranges) and bad == K
    assert got == box.slices(ranges)
    assert intact
    decoded, direct, returned = box.counters("range_blocks_decoded", "range_blocks_direct", "range_returned_bytes")
    assert decoded == 6 and direct == 0 and returned == n               # every block but the empty one, each once; all have several users


def test_the_prefix_is_real(box):
    rc, got, n, _, intact = box.read([(1000, 4096)])
    assert rc == 0 and got == box.data[1000:5096] and intact, box.lib.nlzm_hip_last_error()
    assert box.counters("range_decoded_bytes", "range_blocks_decoded", "range_scratch_bytes", "range_pieces", "decode_out_bytes") == [5096, 1, 5096, 1, 5096]
    rc, got, n, _, intact = box.read([(550_000, 4096)])
    assert rc == 0 and got == box.data[550_000:554_096] and intact
    assert box.counters("range_decoded_bytes")[0] == 554_096
    assert box.gpu.counter("decode_global_bytes") > 0                   # (dups: matches farther back than the ring, cut or not)


def test_the_direct_path(box):
    st = box.start
    ranges = [(st[1], st[6] - st[1])]
    rc, got, n, _, intact = box.read(ranges)
    assert rc == 0 and got == box.slices(ranges) and intact, box.lib.nlzm_hip_last_error()
    assert box.counters("range_scratch_bytes", "range_pieces", "range_blocks_direct", "range_blocks_decoded") == [0, 0, 4, 4]      # (the empty block is none)
    # a range that starts in front of a block and ends inside it: that block goes direct as a prefix, the first one through the scratch buffer
    ranges = [(st[1] - 10, 10 + 300_000 + 0 + 1 + 500)]
    rc, got, n, _, intact = box.read(ranges)
    assert rc == 0 and got == box.slices(ranges) and intact
    assert box.counters("range_blocks_direct", "range_blocks_decoded", "range_scratch_bytes", "range_pieces") == [3, 4, 600_000, 1]
    assert box.counters("range_decoded_bytes")[0] == 600_000 + 300_000 + 1 + 500


def test_each_block_is_decoded_once(box):
    st = box.start
    rng = np.random.default_rng(77)
    ranges = []
    for _ in range(20):
        off = int(rng.integers(0, 350_000))
        ranges.append((st[6] + off, int(rng.integers(1, 20_000))))
    rc, got, n, _, intact = box.read(ranges)
    assert rc == 0 and got == box.slices(ranges) and intact, box.lib.nlzm_hip_last_error()
    assert box.counters("range_blocks_decoded", "range_decoded_bytes", "range_pieces", "decode_streams") == [1, max(o + l for o, l in ranges) - st[6], 20, 1]


def test_without_lengths_and_a_lone_stream(box):
    st = box.start
    ranges = [(st[1] - 50, 100), (st[4] + 9, 90_000), (st[6] + 399_000, 1000)]
    rc, got, n, _, intact = box.read(ranges, lens=None, raws=None)
    assert rc == 0 and got == box.slices(ranges) and intact, box.lib.nlzm_hip_last_error()
    assert box.gpu.counter("decode_passes") == 2                        # the size pass of all blocks, then the decode
    rc, got, n, _, intact = box.read(ranges)
    assert rc == 0 and got == box.slices(ranges) and box.gpu.counter("decode_passes") == 1
    # one stream is nblocks = 1
    lone = torch.from_numpy(np.frombuffer(box.streams[1], dtype=np.uint8).copy()).to("cuda:0")
    for lens, raws in ((None, None), ([box.lens[1]], [box.raws[1]])):
        rc, got, n, _, intact = box.read([(299_000, 1000), (5, 10)], lens=lens, raws=raws, src=lone, nblocks=1)
        assert rc == 0 and got == box.blocks[1][299_000:] + box.blocks[1][5:15] and intact, box.lib.nlzm_hip_last_error()


def test_arguments(box):
    st, T = box.start, box.total
    for bad in ([((1 << 64) - 1, 2)], [(T, 1)], [(T - 1, 2)], [(0, 10), (T + 1, 0)]):
        rc, _, _, _, intact = box.read(bad, room=16)
        assert rc == E_ARG and box.untouched, bad                        # nothing written, anywhere
    rc, _, _, _, intact = box.read([(1000, 4096), (st[4], 100)], cap_delta=-1)
    assert rc == E_CAPACITY and box.untouched                            # nothing written: not even the ranges that would have fitted
    rc, got, n, bad, intact = box.read([])
    assert rc == 0 and n == 0 and got == b"" and intact
    # a fully read block against a raw length that overstates / understates it, addressed as that table has it
    for delta, want in ((5, E_FORMAT), (-5, E_CAPACITY)):
        raws = list(box.raws)
        raws[4] += delta
        rc, _, _, _, intact = box.read([(st[4], raws[4])], raws=raws)
        assert rc == want and intact, (delta, rc)
    assert box.lib.nlzm_hip_read_ranges_dev(None, 8, 1, None, None, None, 0, None, None, None, 0, C.byref(C.c_uint64(0)), None) == E_ARG
    assert box.lib.nlzm_hip_read_ranges_dev(box.d_src.data_ptr(), box.d_src.numel(), 0, None, None, None, 0, None, None, None, 0, C.byref(C.c_uint64(0)), None) == E_ARG


def test_crcs(box):
    st = box.start
    ranges = [(st[1] - 100, 100 + 300_000), (st[4] + 10, 50), (st[5] + 5, 300_000 - 5), (st[6], 399_999)]
    # read in full: 0 (to its end), 1, 5; in part: 4, 6
    rc, got, n, bad, intact = box.read(ranges, crcs=box.crcs)
    assert rc == 0 and got == box.slices(ranges) and intact, box.lib.nlzm_hip_last_error()
    assert bad == K and box.gpu.counter("range_blocks_checked") == 3
    wrong = list(box.crcs)
    wrong[5] ^= 0x00000100
    rc, got, n, bad, intact = box.read(ranges, crcs=wrong)
    assert rc == 0 and bad == 5 and got == box.slices(ranges)
    wrong = list(box.crcs)
    wrong[6] ^= 0x00000100                                               # block 6 is read one byte short of its end: it cannot be checked
    rc, got, n, bad, intact = box.read(ranges, crcs=wrong)
    assert rc == 0 and bad == K and box.gpu.counter("range_blocks_checked") == 3


def test_binding_and_command_line(box, tmp_path):
    st, gpu = box.start, box.gpu
    ranges = [(st[1] - 3, 10), (0, 0), (st[6] + 1000, 4096), (st[4], 100_000), (st[5] - 2, 300_004)]
    want = [box.data[o:o + l] for o, l in ranges]
    assert gpu.read_ranges(box.blob, ranges, K) == want
    assert gpu.read_ranges(box.blob, ranges, K, box.lens, box.raws, box.crcs) == want
    assert gpu.read_range(box.blob, st[6] + 5, 77, K, box.lens, box.raws) == box.data[st[6] + 5:st[6] + 82]
    assert gpu.read_range(box.streams[1], 1234, 4321) == box.blocks[1][1234:5555]
    wrong = list(box.crcs)
    wrong[4] ^= 1
    with pytest.raises(gpu.CrcMismatch) as e:
        gpu.read_ranges(box.blob, ranges, K, box.lens, box.raws, wrong)
    assert e.value.block == 4
    f, out = tmp_path / "c.nlzm", tmp_path / "o.bin"
    f.write_bytes(box.blob)
    lines, off = [f"NLZMIDX 2 {K} {box.total} {len(box.blob)} {zlib.crc32(box.data):08X}"], 0
    for i in range(K):
        lines.append(f"{off} {box.lens[i]} {box.raws[i]} {box.crcs[i]:08X}")
        off += box.lens[i]
    (tmp_path / "c.nlzm.idx").write_text("\n".join(lines) + "\n")
    assert gpu.read_index(tmp_path / "c.nlzm.idx") == (box.lens, box.raws, box.crcs)
    r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu"] + [f"-range:{o}:{l}" for o, l in ranges] + ["x", str(f), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == b"".join(want)
    assert "CRC32 ok (3 of 5 blocks read in full)" in r.stdout, r.stdout    # blocks 0, 1, 4, 5, 6 read; 0, 4 and 5 to their ends


# ---- the split of the container on the device (split_kernel, dec::split_walk) against the host's walk -------------------------------------
# nlzm_hip_decompress_blocks_dev without lengths hops over the frame headers in device memory; nlzm_hip_decompress_blocks on host buffers
# splits with nlzm_host::split_streams.  Wrong ARGUMENTS over intact bytes: nothing here is a damaged stream.  Nothing can wait: the walk is
# one lane, and every step moves forward by at least 28 bytes or ends.

def split_both(box, nblocks, src_len):
    """the two entries on the same bytes and arguments -> [(rc, last error, decode passes, dst_len, raw lengths, the destination)] for dev, host"""
    lib, cap, out = box.lib, box.total, []
    host_src = np.frombuffer(box.blob, dtype=np.uint8)
    for dev in (True, False):
        raw, n = (C.c_uint64 * nblocks)(*([12345] * nblocks)), C.c_uint64(12345)
        if dev:
            d = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rc = lib.nlzm_hip_decompress_blocks_dev(box.d_src.data_ptr(), src_len, nblocks, None, None, d.data_ptr(), cap, raw, C.byref(n))
        else:
            h = np.full(cap + 64, CANARY, dtype=np.uint8)
            rc = lib.nlzm_hip_decompress_blocks(host_src.ctypes.data, src_len, nblocks, None, None, h.ctypes.data, cap, raw, C.byref(n))
        err = lib.nlzm_hip_last_error().decode() if rc else ""
        passes = box.gpu.counter("decode_passes")
        if dev:
            torch.cuda.synchronize()
            h = d.cpu().numpy()
        out.append((rc, err, passes, int(n.value), list(raw), h.tobytes()))
    return out


def test_split_on_the_device_is_the_hosts(box):
    """nblocks = K: the outputs are equal (and the inputs); fewer blocks: whatever the host entry does, code and bytes; more blocks than there
    are: both name block K + 1"""
    for nblocks in list(range(1, K + 1)) + [K + 1, K + 3]:
        dev, host = split_both(box, nblocks, len(box.blob))
        assert dev == host, (nblocks, dev[:5], host[:5])
        rc, err, passes, n, raw, dst = dev
        if nblocks <= K:
            want = b"".join(box.blocks[:nblocks])
            assert rc == 0 and n == len(want) and raw == box.raws[:nblocks] and dst[:n] == want and set(dst[n:]) == {CANARY}, nblocks
            assert passes == 2                                           # the size pass, then the decode
        else:
            assert rc == E_FORMAT and f"block {K + 1} of {nblocks} " in err and passes == 0, (nblocks, rc, err, passes)
            assert raw == [12345] * nblocks and n == 12345 and set(dst) == {CANARY}


def test_split_of_a_cut_container(box):
    """src_len cut inside three blocks -- the first (several frames), the empty one, the last -- at offsets round the header's and a frame header's
    fields, and at the block's last four bytes and last byte: both entries return the same code and name the same block, which is the first
    block that the bytes do not hold in full, and neither launches a decode"""
    cstart = [sum(box.lens[:i]) for i in range(K + 1)]
    seen = set()
    for j in (0, 2, K - 1):
        for c in (0, 1, 3, 4, 7, 8, 11, 12, 15, 16, 27, box.lens[j] - 4, box.lens[j] - 1):
            src_len = cstart[j] + c
            dev, host = split_both(box, K, src_len)
            assert dev == host, (j, c, dev[:5], host[:5])
            rc, err, passes, n, raw, dst = dev
            first_cut = next(i for i in range(K) if cstart[i + 1] > src_len)       # (c may reach past a short block: the empty one is 8 bytes)
            assert rc == E_FORMAT and f"block {first_cut + 1} of {K} " in err and passes == 0, (j, c, rc, err, passes)
            assert set(dst) == {CANARY}
            seen.add(first_cut)
    assert seen == {0, 2, 3, K - 1}
    assert box.lens[0] > 100_000 and box.lens[2] == 8
