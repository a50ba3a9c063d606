"""CPU suite: the options and counters of containers compressed in sets and of the small-ring decoder through the C ABI without a device,
what the header says of them, the command line's -blocks:k, and decode_small_kernel's ISA and resource figures."""
import ctypes as C
import os
import re
import subprocess

import pytest

import nlzm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlzm_amd", "csrc")
E_ARG, E_NODEVICE = -1, -2


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_options_accept_what_the_header_documents(lib):
    for v in (1, 7, 32, 64):
        assert lib.nlzm_hip_set_option(b"container_set_blocks", v) == 0, v
    for v in (0, -1, 65, 65536):
        assert lib.nlzm_hip_set_option(b"container_set_blocks", v) == E_ARG, v
        assert b"container_set_blocks" in lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_set_option(b"container_set_blocks", 32) == 0
    for v in (0, 65536, 16384):
        assert lib.nlzm_hip_set_option(b"decode_ring", v) == 0, v
    for v in (1, 512, 8192, 32768, 131072, -16384):
        assert lib.nlzm_hip_set_option(b"decode_ring", v) == E_ARG, v
        assert b"decode_ring" in lib.nlzm_hip_last_error()
    assert lib.nlzm_hip_set_option(b"decode_ring", 0) == 0


def test_counters_answer_without_a_device(lib):
    v = C.c_uint64(99)
    for key in (b"container_sets", b"decode_ring_size"):
        assert lib.nlzm_hip_get_counter(key, C.byref(v)) == 0 and v.value == 0, key


def test_header_documents_them_and_the_library_exports_what_it_declares(lib):
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    for word in ('"container_set_blocks"', '"decode_ring"', '"container_sets"', '"decode_ring_size"', "65536", "16384", "decode_small_kernel"):
        assert word in header, word
    declared = set(re.findall(r"^(?:int|void|uint64_t|uint32_t|const char \*)\s*\*?(nlzm_hip_\w+)\(", header, re.M))
    assert declared == set(nlzm_amd.ABI_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    assert b"decode_small_kernel" in blob and b"decode_kernel" in blob and b"decode_steps_kernel" in blob
    util = open(os.path.join(CSRC, "nlzm_host_util.h")).read()
    assert "void launch_decode_small(" in util


def test_wide_containers_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 4096)()
    lens, n = (C.c_uint64 * 1000)(), C.c_uint64(0)
    assert lib.nlzm_hip_compress_blocks(buf, 1000, 1000, 16, buf, 4096, lens, C.byref(n)) == E_NODEVICE
    assert lib.nlzm_hip_compress_blocks_dev(buf, 1000, 1000, 16, buf, 4096, lens, C.byref(n)) == E_NODEVICE
    assert b"nlzm_hip_init" in lib.nlzm_hip_last_error()
    with pytest.raises(ValueError):
        nlzm_amd.compress_blocks(bytes(100), 65537)
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.compress_blocks(bytes(100), 1000)


def test_cli_takes_wide_containers(lib, tmp_path):
    r = subprocess.run([nlzm_amd.CLI_PATH], capture_output=True, text=True)
    assert "1 to 65536" in r.stdout and "-blocks:k" in r.stdout
    src = tmp_path / "in"
    src.write_bytes(bytes(100))
    for flag, said in (("-blocks:1000", "Blocks: 1000"), ("-blocks:65536", "Blocks: 65536"), ("-blocks:70000", "Blocks: 65536"), ("-blocks:0", "Blocks: 1")):
        r = subprocess.run([nlzm_amd.CLI_PATH, flag, "h", str(src)], capture_output=True, text=True)
        assert said in r.stdout.splitlines(), (flag, r.stdout)
    r = subprocess.run([nlzm_amd.CLI_PATH, "-blocks:1000", "-gpus:2", "h", str(src)], capture_output=True, text=True)
    assert "Blocks: 64 (on each GPU: a launch holds no more)" in r.stdout       # the per-device limit stays


def test_small_kernel_has_no_scratch_flat_or_calls():
    r = subprocess.run(["make", "-C", CSRC, "asmcheck-decode"], capture_output=True, text=True)
    assert r.returncode == 0 and "asmcheck-decode: ok" in r.stdout, r.stdout + r.stderr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^asmcheck-decode:.*nlzm_decode_small\.hip", mk, re.M) and "for f in nlzm_decode.hip nlzm_decode_small.hip" in mk
    assert "nlzm_decode_small.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)


def test_small_kernel_resources(tmp_path):
    """-Rpass-analysis=kernel-resource-usage of nlzm_decode_small.hip with the product's flags: no scratch, the 16 KiB ring and nothing else in LDS,
    at most 128 VGPRs (four waves a SIMD have 128 each; above that the ring would no longer be what bounds the occupancy)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only",
                        "-o", str(tmp_path / "small.s"), "nlzm_decode_small.hip"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\w+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    keys = [k for k in res if re.search(r"\d+decode_small_kernelE", k)]
    assert len(keys) == 1 and len(res) == 1, list(res)         # (one kernel in the file, and it is this one)
    k = res[keys[0]]
    assert int(k["ScratchSize"]) == 0 and int(k["VGPRs Spill"]) == 0 and k["Dynamic Stack"] == "False", k
    assert int(k["LDS Size"]) == 16384, k
    assert int(k["VGPRs"]) <= 128, k
    assert int(k["Occupancy"]) >= 3, k
