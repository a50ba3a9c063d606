"""GPU suite (-m gpu): content-defined cut points found on the device (nlzm_hip_cut_points*) against the numpy model (tests/cut_model.py).
Every check is exact.  Inputs are at most 100 KB; the kernels' bounds are held on the CPU (tests/test_cut_sim.py), nothing here is damaged."""
import ctypes as C

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from nlzm_amd import corpus
from tests import cut_model

pytestmark = pytest.mark.gpu

E_CAPACITY = -4
KINDS = ["text", "random", "zeros", "ones"]


@pytest.fixture(scope="module")
def inputs(gpu):
    """host bytes of every kind, and one device tensor that holds them all, each at a 256-byte boundary (so that a shift by 1 .. 15 is that misalignment)"""
    S = gpu.counter("cut_segment_bytes")
    part = 3 * S + 777 + 64
    room = (part + 255) // 256 * 256
    host = {
        "text": corpus.syn_text(part),
        "random": np.random.default_rng(corpus.SEED + 90).integers(0, 256, part, dtype=np.uint8),
        "zeros": np.zeros(part, dtype=np.uint8),
        "ones": np.full(part, 0xFF, dtype=np.uint8),
    }
    flat = np.zeros(room * len(KINDS), dtype=np.uint8)
    for i, k in enumerate(KINDS):
        flat[i * room: i * room + part] = host[k]
    dev = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 256 == 0
    return {"S": S, "host": host, "dev": dev, "room": room, "memo": {}}


def lengths_of(S):
    return [0, 1, 31, 32, 33, S - 1, S, S + 1, 2 * S + 31, 3 * S + 777]


def model(inputs, kind, shift, n, avg_bits, lo, hi):
    key = (kind, shift, n, avg_bits, lo, hi)
    if key not in inputs["memo"]:
        inputs["memo"][key] = cut_model.cut_points(inputs["host"][kind][shift: shift + n], avg_bits, lo, hi)
    return inputs["memo"][key]


def cuts_dev(lib, inputs, kind, shift, n, avg_bits, lo, hi, cap=None):
    want_cap = n // lo if cap is None else cap
    cuts, got = (C.c_uint64 * max(1, want_cap))(), C.c_uint32(0xDEAD)
    ptr = inputs["dev"].data_ptr() + KINDS.index(kind) * inputs["room"] + shift
    rc = lib.nlzm_hip_cut_points_dev(ptr, n, avg_bits, lo, hi, cuts, want_cap, C.byref(got))
    return rc, got.value, [int(cuts[i]) for i in range(min(got.value, want_cap))]


@pytest.mark.parametrize("avg_bits", [1, 4, 12])
def test_device_cuts_equal_the_models(gpu, inputs, avg_bits):
    """n in 0, 1, 31, 32, 33, S - 1, S, S + 1, 2S + 31, 3S + 777 on text, random bytes, zeros and 0xFF, with small lengths (min 32, max small enough
    to force cuts) and the default ones, through the _dev form"""
    lib = gpu.load_library()
    for kind in KINDS:
        for n in lengths_of(inputs["S"]):
            for lo, hi in ((32, 100), (32, 1 << 31), cut_model.defaults(avg_bits)):
                rc, k, got = cuts_dev(lib, inputs, kind, 0, n, avg_bits, lo, hi)
                assert rc == 0, lib.nlzm_hip_last_error()
                want = model(inputs, kind, 0, n, avg_bits, lo, hi)
                assert (k, got) == (len(want), want), (kind, n, lo, hi)
                if n > lo:
                    assert gpu.counter("cut_candidates") == cut_model.candidates(inputs["host"][kind][:n], avg_bits).size


def test_misaligned_source(gpu, inputs):
    """the source pointer 1 .. 15 bytes off a 256-byte boundary"""
    lib = gpu.load_library()
    S = inputs["S"]
    for shift in range(1, 16):
        for j, n in enumerate((33, 1000 + shift, S + 1, 2 * S + 31)):
            kind, avg_bits = KINDS[(shift + j) % 2], (1, 4, 12)[(shift + j) % 3]
            lo, hi = (32, 100) if j % 2 else cut_model.defaults(avg_bits)
            rc, k, got = cuts_dev(lib, inputs, kind, shift, n, avg_bits, lo, hi)
            assert rc == 0, lib.nlzm_hip_last_error()
            assert got == model(inputs, kind, shift, n, avg_bits, lo, hi), (shift, n)


def test_host_form_and_binding(gpu, inputs):
    lib = gpu.load_library()
    S = inputs["S"]
    for kind in KINDS:
        data = inputs["host"][kind][: 2 * S + 31]
        for avg_bits in (4, 12):
            assert gpu.cut_points(data, avg_bits) == cut_model.cut_points(data, avg_bits)
        assert gpu.cut_points(data.tobytes(), 12, 100, 2000) == cut_model.cut_points(data, 12, 100, 2000)
    assert gpu.cut_points(b"", 12) == [] and gpu.cut_points(b"x" * 33, 1, 32, 32) == cut_model.cut_points(b"x" * 33, 1, 32, 32)
    cuts = gpu.cut_points(inputs["host"]["text"][:50_000], 10)
    blocks = gpu.cut_ranges(50_000, cuts)
    assert blocks == cut_model.blocks(50_000, cuts) and len(blocks) > 10 and gpu.counter("cut_us") > 0
    # the host form through the C ABI, with a list exactly as long as needed
    data = inputs["host"]["random"][:S + 1]
    want = cut_model.cut_points(data, 4, 32, 100)
    buf, got = (C.c_uint64 * len(want))(), C.c_uint32(0)
    assert lib.nlzm_hip_cut_points(data.ctypes.data, data.size, 4, 32, 100, buf, len(want), C.byref(got)) == 0, lib.nlzm_hip_last_error()
    assert got.value == len(want) and list(buf) == want


def test_a_list_one_short(gpu, inputs):
    """cut_cap one short: NLZM_HIP_E_CAPACITY with the number needed, and the next call works"""
    lib = gpu.load_library()
    S = inputs["S"]
    for kind, avg_bits, lo, hi in (("text", 4, 32, 100), ("zeros", 12, 32, 64), ("random", 12, 1024, 16384)):
        n = 2 * S + 31
        want = model(inputs, kind, 0, n, avg_bits, lo, hi)
        assert len(want) >= 2
        rc, k, _ = cuts_dev(lib, inputs, kind, 0, n, avg_bits, lo, hi, cap=len(want) - 1)
        assert rc == E_CAPACITY and k == len(want) and b"cut_cap" in lib.nlzm_hip_last_error()
        rc, k, got = cuts_dev(lib, inputs, kind, 0, n, avg_bits, lo, hi, cap=len(want))
        assert rc == 0 and got == want
