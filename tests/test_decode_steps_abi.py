"""CPU suite: the stepping decoder's entry points without a device, its counters' names, both decode kernels' ISA and the one-shot kernel's
resource figures (building the stepping form beside it may not change what it is), and the command line's -steps flag where it does not belong
(`-gpu -steps:K d / t` themselves are run by tests/test_gpu_decode_steps.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import nlzm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlzm_amd", "csrc")
E_ARG, E_NODEVICE = -1, -2
ENTRIES = ("nlzm_hip_decode_begin_dev", "nlzm_hip_decode_begin", "nlzm_hip_decode_step", "nlzm_hip_decode_extend_dev", "nlzm_hip_decode_fetch",
           "nlzm_hip_decode_finish", "nlzm_hip_decode_abandon")


@pytest.fixture(scope="module")
def lib():
    nlzm_amd.build()
    return nlzm_amd.load_library()


def test_header_and_exports_agree(lib):
    header = open(os.path.join(ROOT, "include", "nlzm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(nlzm_hip_decode_\w+)\(", header, re.M))
    assert declared == set(ENTRIES)
    for name in ENTRIES:
        assert name in nlzm_amd.ABI_SYMBOLS and hasattr(lib, name), name
    assert "#define NLZM_HIP_DECODE_MORE 1u" in header and nlzm_amd.DECODE_MORE == 1
    util = open(os.path.join(CSRC, "nlzm_host_util.h")).read()
    assert "void launch_decode_steps(" in util
    blob = open(nlzm_amd.LIB_PATH, "rb").read()
    assert b"decode_steps_kernel" in blob and b"decode_kernel" in blob


def test_state_bytes_answers_without_a_device(lib):
    v = C.c_uint64(0)
    assert lib.nlzm_hip_get_counter(b"decode_state_bytes", C.byref(v)) == 0
    # 18 model registers of 64 lanes (entries fit 16 bits, kept as dwords at most), the offsets, rep[4], the running counters: a few KB
    assert 18 * 64 * 2 + 2 * 8 + 4 * 4 + 10 * 8 <= v.value <= 8192 and v.value % 16 == 0
    for key in ("decode_steps", "decode_step_us"):
        assert lib.nlzm_hip_get_counter(key.encode(), C.byref(v)) == 0 and v.value == 0, key
    assert lib.nlzm_hip_get_counter(b"decode_step_no_such", C.byref(v)) != 0


def test_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 64)()
    n, fin, ms = C.c_uint64(0), C.c_int(0), C.c_double(0)
    one = (C.c_uint64 * 1)(8)
    calls = {
        "begin_dev": lambda: lib.nlzm_hip_decode_begin_dev(buf, 8, 1, one, one, buf, 64, 0),
        "begin_dev, nothing": lambda: lib.nlzm_hip_decode_begin_dev(None, 0, 0, None, None, None, 0, 0),
        "begin": lambda: lib.nlzm_hip_decode_begin(buf, 8, 1, one, one, 0),
        "begin, nothing": lambda: lib.nlzm_hip_decode_begin(None, 0, 0, None, None, 0),
        "step": lambda: lib.nlzm_hip_decode_step(1, one, one, C.byref(fin), C.byref(ms)),
        "step, nothing": lambda: lib.nlzm_hip_decode_step(0, None, None, None, None),
        "extend_dev": lambda: lib.nlzm_hip_decode_extend_dev(8),
        "fetch": lambda: lib.nlzm_hip_decode_fetch(0, 8, buf),
        "fetch, nothing": lambda: lib.nlzm_hip_decode_fetch(0, 8, None),
        "finish": lambda: lib.nlzm_hip_decode_finish(one, C.byref(n)),
        "finish, nothing": lambda: lib.nlzm_hip_decode_finish(None, None),
    }
    for name, call in calls.items():
        assert call() in (E_NODEVICE, E_ARG), name
        assert lib.nlzm_hip_last_error(), name
    assert calls["begin"]() == E_NODEVICE and b"nlzm_hip_init" in lib.nlzm_hip_last_error()
    lib.nlzm_hip_decode_abandon()                          # always works
    with pytest.raises(nlzm_amd.NlzmError):
        nlzm_amd.Decoder(bytes.fromhex("000a000e00000000"))
    with pytest.raises(ValueError):
        nlzm_amd.Decoder(bytes.fromhex("000a000e00000000"), 2, [8])


def test_both_decode_kernels_have_no_scratch_flat_or_calls():
    r = subprocess.run(["make", "-C", CSRC, "asmcheck-decode"], capture_output=True, text=True)
    assert r.returncode == 0 and "asmcheck-decode: ok" in r.stdout, r.stdout + r.stderr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "asmcheck-decode: nlzm_decode.hip nlzm_decode.h" in mk          # (the file both kernels are in, whole)
    hip = open(os.path.join(CSRC, "nlzm_decode.hip")).read()
    assert "void decode_kernel(" in hip and "void decode_steps_kernel(" in hip


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """-Rpass-analysis=kernel-resource-usage of nlzm_decode.hip with the product's flags: {kernel: {figure: value}}"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    out = tmp_path_factory.mktemp("res") / "decode.s"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only",
                        "-o", str(out), "nlzm_decode.hip"], cwd=CSRC, capture_output=True, text=True)
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
    return res, out.read_text()


def kernel(res, name):
    keys = [k for k in res if re.search(rf"\d+{name}E", k)]
    assert len(keys) == 1, (name, list(res))
    return res[keys[0]]


def test_one_shot_kernel_keeps_its_figures(resources):
    """DESIGN.md section 18's record of decode_kernel: the stepping form is a second instantiation and may not cost the first one anything"""
    k = kernel(resources[0], "decode_kernel")
    assert (int(k["VGPRs"]), int(k["TotalSGPRs"]), int(k["ScratchSize"]), int(k["LDS Size"])) == (105, 106, 0, 65536), k
    assert int(k["SGPRs Spill"]) <= 54 and int(k["VGPRs Spill"]) == 0, k


def test_stepping_kernel_resources(resources):
    res, asm = resources
    k = kernel(res, "decode_steps_kernel")
    assert int(k["ScratchSize"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["LDS Size"]) == 65536 and k["Dynamic Stack"] == "False", k
    assert int(k["VGPRs"]) <= 256, k                       # (one wave per workgroup: occupancy is not what it is short of, but AGPR moves would be)
    # the model is saved and restored by register: 18 coalesced dword stores / loads a lane (the compiler may widen none of them: lanes interleave)
    body = asm[asm.index("decode_steps_kernel"):]
    assert not re.search(r"scratch_(load|store)|flat_(load|store|atomic)|s_swappc", asm)
    assert len(re.findall(r"global_store_dword ", body)) >= 18 and len(re.findall(r"global_load_dword ", body)) >= 18


def test_cli_steps_flag_where_it_does_not_belong(tmp_path, lib):
    s = tmp_path / "s.nlzm"
    s.write_bytes(bytes.fromhex("000a000e00000000"))
    for argv in (["-steps:4", "t", s], ["-steps:4", "d", s, tmp_path / "o"], ["-gpu", "-steps:4", "h", s], ["-steps:4", "c", s, tmp_path / "c"]):
        r = subprocess.run([nlzm_amd.CLI_PATH] + [str(a) for a in argv], capture_output=True, text=True)
        assert r.returncode == 255 and "-steps:K is for d -gpu and t -gpu" in r.stdout, (argv, r.stdout)
    assert not (tmp_path / "o").exists() and not (tmp_path / "c").exists()
    for bad in ("-steps:0", "-steps:", "-steps:-3", "-steps:x", "-steps:4x", "-steps: 4", "-steps:+4", "-steps:4294967296"):
        r = subprocess.run([nlzm_amd.CLI_PATH, "-gpu", bad, "t", str(s)], capture_output=True, text=True)
        assert r.returncode == 255 and "Unrecognized flag" in r.stdout, (bad, r.stdout)
    r = subprocess.run([nlzm_amd.CLI_PATH], capture_output=True, text=True)
    assert "-steps:K" in r.stdout
    r = subprocess.run([nlzm_amd.CLI_PATH, "t", str(s)], capture_output=True, text=True)       # without the flag nothing changes
    assert r.returncode == 0 and "Done (output CRC32 0" in r.stdout and "Steps:" not in r.stdout
