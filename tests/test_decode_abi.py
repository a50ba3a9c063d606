"""CPU suite: the decoder's entry points without a device, its kernels' ISA, and the command line's handling of a block index
that does not describe the file (the host path; `d -gpu` shares the code and is run by tests/test_gpu_decode.py)."""
import ctypes as C
import os
import subprocess

import pytest

import nlzm_amd
from nlzm_amd import corpus, shard
from tests import cli_tools, oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NODEVICE = -2


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_decode_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 64)()
    n64, first = C.c_uint64(0), C.c_uint64(0)
    one = (C.c_uint64 * 1)(8)
    calls = {
        "nlzm_hip_decompress_dev": lambda: lib.nlzm_hip_decompress_dev(buf, 8, None, 0, C.byref(n64)),
        "nlzm_hip_decompress": lambda: lib.nlzm_hip_decompress(buf, 8, buf, 64, C.byref(n64)),
        "nlzm_hip_decompress_blocks_dev": lambda: lib.nlzm_hip_decompress_blocks_dev(buf, 8, 1, one, None, None, 0, None, C.byref(n64)),
        "nlzm_hip_decompress_blocks": lambda: lib.nlzm_hip_decompress_blocks(buf, 8, 1, one, None, buf, 64, None, C.byref(n64)),
        "nlzm_hip_verify_dev": lambda: lib.nlzm_hip_verify_dev(buf, 8, 1, None, buf, 0, C.byref(first), C.byref(n64)),
        "nlzm_hip_verify": lambda: lib.nlzm_hip_verify(buf, 8, 1, None, buf, 0, C.byref(first), C.byref(n64)),
    }
    for name, call in calls.items():
        assert call() == E_NODEVICE, name
        assert b"nlzm_hip_init" in lib.nlzm_hip_last_error(), name
    for f in (nlzm_amd.decompress, lambda s: nlzm_amd.decompress_blocks(s, 1), lambda s: nlzm_amd.verify(s, b"")):
        with pytest.raises(nlzm_amd.NlzmError):
            f(bytes.fromhex("000a000e00000000"))


def test_verify_verdict_never_reads_a_longer_decode_as_equal():
    """The library answers (first_mismatch, decoded_len); equal is BOTH == n.  A stream that decodes to the original and more behind it has
    first_mismatch == n as well -- the binding must not hand that back as len(data)."""
    n = 1000
    assert nlzm_amd.verify_verdict(n, n, n) == n                       # equal
    assert nlzm_amd.verify_verdict(17, n, n) == 17                     # a byte differs
    assert nlzm_amd.verify_verdict(990, 990, n) == 990                 # the decode is shorter: a mismatch where it ends
    for longer in (n + 1, 10 * n):
        with pytest.raises(nlzm_amd.LengthMismatch):
            nlzm_amd.verify_verdict(n, longer, n)
    with pytest.raises(nlzm_amd.LengthMismatch):
        nlzm_amd.verify_verdict(0, 8, 0)                                # nothing against something
    assert nlzm_amd.verify_verdict(0, 0, 0) == 0
    hdr = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    assert "#define NLZM_HIP_VERIFY_EQUAL(first_mismatch, decoded_len, n) ((first_mismatch) == (n) && (decoded_len) == (n))" in hdr
    cli = open(os.path.join(ROOT, "nlzm_amd", "csrc", "nlzm_cli.cpp")).read()
    assert "NLZM_HIP_VERIFY_EQUAL(first, decoded, (uint64_t)in.size())" in cli and "first != in.size()" not in cli


def test_decode_counters_are_known_names(lib):
    v = C.c_uint64(1)
    for key in ("decode_syms", "decode_raw_ops", "decode_n_literal", "decode_n_dict", "decode_n_rep", "decode_out_bytes", "decode_ring_bytes",
                "decode_global_bytes", "decode_cycles", "decode_window_cycles", "decode_copy_cycles", "decode_max_stream_cycles", "decode_streams",
                "decode_passes", "decode_ms", "decode_us"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0, key
    assert lib.nlzm_hip_get_counter(b"decode_no_such", C.byref(v)) != 0


def test_decode_kernels_have_no_scratch_flat_or_calls():
    """The symbol chain of a stream may not wait for memory: the model is in registers, the input in register windows.  Checked in the gfx950 ISA,
    as for the persistent kernel."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nlzm_amd", "csrc"), "asmcheck-decode"], capture_output=True, text=True)
    assert r.returncode == 0 and "asmcheck-decode: ok" in r.stdout, r.stdout + r.stderr


def test_library_has_the_decode_kernels(lib):
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    assert b"decode_kernel" in blob and b"split_kernel" in blob and b"compare_kernel" in blob


def test_cli_block_index_that_lies(tmp_path, lib):
    """An index whose fields pass the header checks and still do not describe the file: a length so large that offset + length wraps
    (it used to be read out of bounds), and raw lengths that are not what the blocks decode to (stale index).  Both fall back to the frame
    headers, with a note, and the output is the input."""
    data = corpus.mixed(300_000, corpus.SEED + 11)
    k = 3
    ranges = [shard.block_range(data.size, k, i) for i in range(k)]
    streams = [oracle_py.compress(data[lo:hi], 17) for lo, hi in ranges]
    blob = b"".join(streams)
    f, idx = tmp_path / "c.nlzm", tmp_path / "c.nlzm.idx"
    f.write_bytes(blob)

    def write_index(lens, raws):
        cli_tools.write_index(idx, lens, raws, version=1, n_in=data.size, n_out=len(blob))

    good_lens, good_raws = [len(s) for s in streams], [hi - lo for lo, hi in ranges]
    # block 2's length wraps offset + length round to a small number
    write_index([good_lens[0], (1 << 64) - good_lens[0] + 16, good_lens[2]], good_raws)
    out = tmp_path / "o1.bin"
    r = subprocess.run([nlzm_amd.CLI_PATH, "d", str(f), str(out)], capture_output=True, text=True)
    # (a block that claims more bytes than the file has left reads as "the file is cut inside it": block 1 comes out, nothing is read out of bounds)
    assert r.returncode not in (0, 255) and "cut off inside block 2" in r.stdout, r.stdout
    assert out.read_bytes() == data.tobytes()[:ranges[1][0]]
    # raw lengths of another partition: same sum, wrong per block
    write_index(good_lens, [good_raws[0] - 5, good_raws[1] + 5, good_raws[2]])
    out = tmp_path / "o2.bin"
    r = subprocess.run([nlzm_amd.CLI_PATH, "d", str(f), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "does not describe" in r.stdout and f"Blocks: {k}" in r.stdout, r.stdout
    assert out.read_bytes() == data.tobytes()
    # ... and a sum that is not the header's n_in does not fit at all
    write_index(good_lens, [good_raws[0] - 5, good_raws[1], good_raws[2]])
    r = subprocess.run([nlzm_amd.CLI_PATH, "t", str(f)], capture_output=True, text=True)
    assert r.returncode == 0 and "does not fit" in r.stdout and f"Blocks: {k}" in r.stdout, r.stdout
    # the right index still is taken
    write_index(good_lens, good_raws)
    r = subprocess.run([nlzm_amd.CLI_PATH, "t", str(f)], capture_output=True, text=True)
    assert r.returncode == 0 and "does not" not in r.stdout and f"Blocks: {k}" in r.stdout, r.stdout


def test_cli_gpu_flags_need_a_device(tmp_path, lib):
    """`d -gpu` asks for the device and says so when there is none; plain `d` on the same file does not."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    s = tmp_path / "s.nlzm"
    s.write_bytes(bytes.fromhex("000a000e00000000"))
    r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", "t", str(s)], capture_output=True, text=True)
    assert r.returncode != 0 and "Error:" in r.stdout
    r = subprocess.run([nlzm_amd.CLI_PATH, "t", str(s)], capture_output=True, text=True)
    assert r.returncode == 0 and "Done (output CRC32 0" in r.stdout
