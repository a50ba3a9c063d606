"""CPU suite: the device CRC32's entry points without a device, its arithmetic against zlib, its kernels' ISA, and the command line's
handling of an index that holds CRC32s (NLZMIDX 2) on the host path (`t -gpu` shares the index code and is run by tests/test_gpu_crc.py)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import oracle_py
from tests.cli_tools import cli, write_index

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
E_NODEVICE = -2
STATUS_CRC = 256 - 4                                  # the command line's -4


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_combine_against_zlib(lib):
    rng = np.random.default_rng(corpus.SEED + 40)
    data = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    whole = zlib.crc32(data)
    for _ in range(200):
        cut = int(rng.integers(0, len(data) + 1))
        assert nlzm_amd.crc32_combine(zlib.crc32(data[:cut]), zlib.crc32(data[cut:]), len(data) - cut) == whole
    assert nlzm_amd.crc32_combine(whole, 0, 0) == whole                     # len_b = 0: B is empty
    assert nlzm_amd.crc32_combine(0, whole, len(data)) == whole             # A is empty


def test_combine_with_a_length_beyond_32_bits(lib):
    """B = 2^32 + 12,345 zero bytes, fed to zlib in pieces"""
    a = b"the part in front"
    len_b = (1 << 32) + 12_345
    piece = bytes(1 << 26)
    crc_b, crc_ab, left = 0, zlib.crc32(a), len_b
    while left:
        m = min(left, len(piece))
        crc_b, crc_ab, left = zlib.crc32(piece[:m], crc_b), zlib.crc32(piece[:m], crc_ab), left - m
    assert nlzm_amd.crc32_combine(zlib.crc32(a), crc_b, len_b) == crc_ab


def test_crc_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 64)()
    out = C.c_uint32(0)
    one, zero = (C.c_uint64 * 1)(8), (C.c_uint64 * 1)(0)
    calls = {
        "nlzm_hip_crc32": lambda: lib.nlzm_hip_crc32(buf, 64, 0, C.byref(out)),
        "nlzm_hip_crc32_dev": lambda: lib.nlzm_hip_crc32_dev(buf, 64, 0, C.byref(out)),
        "nlzm_hip_crc32_ranges": lambda: lib.nlzm_hip_crc32_ranges(buf, 64, 1, zero, one, C.byref(out)),
        "nlzm_hip_crc32_ranges_dev": lambda: lib.nlzm_hip_crc32_ranges_dev(buf, 64, 1, zero, one, C.byref(out)),
        "nlzm_hip_check": lambda: lib.nlzm_hip_check(buf, 8, 1, one, None, C.byref(out), C.byref(out), None),
        "nlzm_hip_check_dev": lambda: lib.nlzm_hip_check_dev(buf, 8, 1, one, None, C.byref(out), C.byref(out), None),
    }
    for name, call in calls.items():
        assert call() == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
    assert lib.nlzm_hip_feed_input_crc32(C.byref(out)) != 0 and lib.nlzm_hip_last_error()
    for f in (lambda: nlzm_amd.crc32(b"abc"), lambda: nlzm_amd.crc32_ranges(b"abc", [(0, 3)]), lambda: nlzm_amd.check(bytes.fromhex("000a000e00000000"), [0])):
        with pytest.raises(nlzm_amd.NlzmError):
            f()


def test_crc_counters_are_known_names(lib):
    v = C.c_uint64(0)
    for key in ("crc_us", "crc_bytes", "crc_segment_bytes"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert v.value >= 1024 and v.value % 1024 == 0       # the segment size: whole steps of a wave, known without a device
    assert lib.nlzm_hip_get_counter(b"crc_no_such", C.byref(v)) != 0


def test_crc_kernels_have_no_scratch_flat_or_calls():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "asmcheck-crc"], capture_output=True, text=True)
    assert r.returncode == 0 and "asmcheck-crc: ok" in r.stdout, r.stdout + r.stderr


def test_library_has_the_crc_kernels(lib):
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    assert b"crc_segments_kernel" in blob and b"crc_combine_kernel" in blob


# ---- the command line, host only: streams from the oracle, the index written here, the CRCs zlib's ----

K = 5


@pytest.fixture(scope="module")
def container(lib):
    data = corpus.mixed(400_000, corpus.SEED + 41)
    ranges = [shard.block_range(data.size, K, i) for i in range(K)]
    streams = [oracle_py.compress(data[lo:hi], 17) for lo, hi in ranges]
    raw = data.tobytes()
    return {"data": raw, "ranges": ranges, "streams": streams, "crcs": [zlib.crc32(raw[lo:hi]) for lo, hi in ranges], "whole": zlib.crc32(raw)}


def test_cli_good_index_with_crcs(tmp_path, container):
    c = container
    f = tmp_path / "c.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    write_index(tmp_path / "c.nlzm.idx", c["streams"], [hi - lo for lo, hi in c["ranges"]], c["crcs"], c["whole"])
    r = cli("t", f)
    assert r.returncode == 0 and f"CRC32 ok ({K} blocks)" in r.stdout and f"Blocks: {K}" in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    assert f"Done (output CRC32 {c['whole']:X}," in r.stdout
    out = tmp_path / "o.bin"
    r = cli("d", f, out)
    assert r.returncode == 0 and f"CRC32 ok ({K} blocks)" in r.stdout, r.stdout
    assert out.read_bytes() == c["data"]


def test_cli_wrong_block_crc(tmp_path, container):
    c = container
    f = tmp_path / "c.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    crcs = list(c["crcs"])
    crcs[2] ^= 0x00010000                                  # block 3, counted from 1
    write_index(tmp_path / "c.nlzm.idx", c["streams"], [hi - lo for lo, hi in c["ranges"]], crcs, c["whole"])
    r = cli("t", f)
    assert r.returncode == STATUS_CRC, (r.returncode, r.stdout)
    assert f"CRC32 MISMATCH in block 3 (index says {crcs[2]:08X}, decoded {c['crcs'][2]:08X})" in r.stdout and "CRC32 ok" not in r.stdout, r.stdout
    out = tmp_path / "o.bin"
    r = cli("d", f, out)
    assert r.returncode == STATUS_CRC and "CRC32 MISMATCH in block 3 " in r.stdout, (r.returncode, r.stdout)
    assert out.read_bytes() == c["data"]                   # what decoded is what a user can recover: written all the same


def test_cli_wrong_whole_crc(tmp_path, container):
    c = container
    f = tmp_path / "c.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    write_index(tmp_path / "c.nlzm.idx", c["streams"], [hi - lo for lo, hi in c["ranges"]], c["crcs"], c["whole"] ^ 1)
    r = cli("t", f)
    assert r.returncode == STATUS_CRC, (r.returncode, r.stdout)
    assert f"CRC32 MISMATCH of the whole file (index says {c['whole'] ^ 1:08X}, blocks combine to {c['whole']:08X})" in r.stdout and "CRC32 ok" not in r.stdout, r.stdout


def test_cli_one_stream_with_an_index(tmp_path, lib):
    data = corpus.syn_text(120_000).tobytes()
    s = oracle_py.compress(np.frombuffer(data, dtype=np.uint8), 17)
    f = tmp_path / "s.nlzm"
    f.write_bytes(s)
    crc = zlib.crc32(data)
    write_index(tmp_path / "s.nlzm.idx", [s], [len(data)], [crc], crc)
    r = cli("t", f)
    assert r.returncode == 0 and "CRC32 ok (1 blocks)" in r.stdout, r.stdout
    write_index(tmp_path / "s.nlzm.idx", [s], [len(data)], [crc ^ 0x80], crc ^ 0x80)
    out = tmp_path / "o.bin"
    r = cli("d", f, out)
    assert r.returncode == STATUS_CRC and "CRC32 MISMATCH in block 1 " in r.stdout, (r.returncode, r.stdout)
    assert out.read_bytes() == data


def test_cli_index_with_crcs_that_does_not_fit(tmp_path, container):
    """the structural checks of version 1 hold for version 2: an index whose lengths do not add up is not believed, the frame headers decide,
    and nothing is said about CRCs"""
    c = container
    f = tmp_path / "c.nlzm"
    f.write_bytes(b"".join(c["streams"]))
    raws = [hi - lo for lo, hi in c["ranges"]]
    write_index(tmp_path / "c.nlzm.idx", c["streams"], [raws[0] - 5] + raws[1:], c["crcs"], c["whole"], n_in=sum(raws))
    r = cli("t", f)
    assert r.returncode == 0 and "does not fit" in r.stdout and f"Blocks: {K}" in r.stdout and "CRC32 ok" not in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    # raw lengths of another partition (same sum): believed at first, shown wrong by the decode, and again no CRC claim
    write_index(tmp_path / "c.nlzm.idx", c["streams"], [raws[0] - 5, raws[1] + 5] + raws[2:], c["crcs"], c["whole"])
    out = tmp_path / "o.bin"
    r = cli("d", f, out)
    assert r.returncode == 0 and "does not describe" in r.stdout and "CRC32 ok" not in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    assert out.read_bytes() == c["data"]
    # a version-1 index is read as before
    write_index(tmp_path / "c.nlzm.idx", c["streams"], raws, version=1)
    r = cli("t", f)
    assert r.returncode == 0 and "does not" not in r.stdout and "CRC32 ok" not in r.stdout and f"Blocks: {K}" in r.stdout, r.stdout
