"""GPU suite (-m gpu): the gfx950 half of nlzm_amd/csrc/xw.h -- DPP scans, wave_shr, ds_bpermute, the split 64-bit cross-lane reads, the
inline-asm 16-byte sc1 accesses, the LDS and agent-scope atomics -- primitive by primitive against the model (tests/xw_model.py), through
the probe role (tests/xw_probe/xw_probe.h) that tests/test_xw_sim.py runs in the simulator.  One launch of one workgroup of 256 and a
second launch that reads what the first wrote; the probe cannot wait for anything.  A mismatch names primitive, case, lane, got and want.

What the device returns where the contract defines nothing (a live lane's result that depends on a lane that has left the role) is
printed (pytest -rP shows it), not asserted: profiles/xw_probe_gpu.txt holds one run's.  2 s on an MI355X, most of it the model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch        # (before the library is loaded, as bench.py has it: both then share one HIP runtime)

import nlzm_amd
from tests import xw_model as xm

pytestmark = pytest.mark.gpu

PROBE_PATH = os.path.join(os.path.dirname(nlzm_amd.LIB_PATH), "libxw_probe.so")


@pytest.fixture(scope="module")
def probe(gpu):
    assert os.path.exists(PROBE_PATH), f"{PROBE_PATH} is missing: build() makes it beside the library"
    lib = C.CDLL(PROBE_PATH)
    lib.xw_probe_run.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32]
    T = xm.Table(strict=False)
    d_in = torch.from_numpy(T.input().view(np.int32)).to("cuda:0")
    d_g = torch.zeros(xm.G_WORDS, dtype=torch.int32, device="cuda:0")
    d_out0 = torch.from_numpy(np.full(T.out_words, xm.SENTINEL, dtype=np.uint32).view(np.int32)).to("cuda:0")
    d_out1 = torch.from_numpy(np.full(T.out2_words, xm.SENTINEL, dtype=np.uint32).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    # sizes that do not fit the table's header are refused before anything is launched
    assert lib.xw_probe_run(d_in.data_ptr(), d_in.numel(), d_out0.data_ptr(), d_out0.numel() - 1, d_g.data_ptr(), d_g.numel(), 0) == -1
    assert lib.xw_probe_run(d_in.data_ptr(), d_in.numel(), d_out0.data_ptr(), d_out0.numel(), d_g.data_ptr(), d_g.numel(), 0) == 0
    assert lib.xw_probe_run(d_in.data_ptr(), d_in.numel(), d_out1.data_ptr(), d_out1.numel(), d_g.data_ptr(), d_g.numel(), 1) == 0
    torch.cuda.synchronize()
    return {"T": T, "out0": d_out0.cpu().numpy().view(np.uint32), "out1": d_out1.cpu().numpy().view(np.uint32), "g": d_g.cpu().numpy().view(np.uint32)}


def test_every_primitive_against_the_model(probe):
    """row boundaries at lanes 15/16, 31/32, 47/48, values on both sides of 2^31, sums that wrap, shuffle sources of 64 and more, the high half
    deciding in lds_min64, the carry in the 64-bit adds, the store-overwrite-store sequence of st_agent128, and -- in the waves with exited
    lanes -- everything the contract defines there"""
    T = probe["T"]
    msgs = xm.compare(probe["out0"], *T.expected())
    assert not msgs, "\n".join(msgs)


def test_second_launch_reads_what_the_first_wrote(probe):
    T = probe["T"]
    msgs = xm.compare(probe["out1"], *T.expected2())
    assert not msgs, "\n".join(msgs)
    # ... and so does the host
    g = probe["g"]
    for t in (0, 63, 64, 255):
        a, b = T.g_final[t]
        assert [int(v) for v in g[4 * t:4 * t + 4]] == a and [int(v) for v in g[1024 + 4 * t:1024 + 4 * t + 4]] == b


def test_what_the_hardware_orders_holds_as_a_property(probe):
    msgs = xm.check_properties(probe["T"], probe["out0"], probe["out1"])
    assert not msgs, "\n".join(msgs)


def test_record_the_undefined_slots(probe):
    """recorded, not asserted: what a live lane gets whose source has left the role.  Asserted here is only that every such case ran (the
    device build runs them all) and that exited lanes wrote nothing."""
    T = probe["T"]
    lines = xm.undefined_slots(T, probe["out0"])
    print(f"xw probe on the device: {T.nc} cases of {len(xm.OPS)} cross-lane primitives, {T.ne} exit cases in 2 waves with exited lanes, "
          f"{T.out_words} + {T.out2_words} output words")
    print("undefined slots (a live lane whose result depends on an exited lane), recorded, not asserted:")
    for l in lines:
        print("  " + l)
    assert lines and not any(l.endswith("not run") for l in lines)
