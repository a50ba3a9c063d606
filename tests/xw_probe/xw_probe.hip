// xw_probe.hip -- the probe role (xw_probe.h) as a gfx950 kernel, and its launcher.  TEST CODE ONLY: built by nlzm_amd/csrc/Makefile
// into a shared object of its own (nlzm_amd/libxw_probe.so), never linked into the product's library.  tests/test_gpu_xw.py loads it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xw_probe.h"

namespace xwp {
__shared__ Lds g_probe_lds;
}
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&xwp::g_probe_lds); }
}

namespace xwp {

// one workgroup of four waves
__global__ __launch_bounds__(256) void probe_kernel(const uint32_t *in, uint32_t *out, uint32_t *g, uint32_t phase)
{
    probe_role(Args{ in, out, g, phase });
}

}  // namespace xwp

// One launch of the probe on device buffers, and a wait for it.  The buffers' sizes (in uint32 words) must be exactly what the table's
// header asks for: the role indexes by the header's counts alone.  Returns 0, -1 for sizes that do not fit, or the HIP error.
extern "C" int xw_probe_run(const void *d_in, uint64_t in_words, void *d_out, uint64_t out_words, void *d_g, uint64_t g_words, uint32_t phase)
{
    if (!d_in || !d_out || !d_g || phase > 1 || in_words < xwp::kHead) return -1;
    uint32_t head[xwp::kHead];
    hipError_t e = hipMemcpy(head, d_in, sizeof head, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    const uint32_t nc = head[1], ne = head[2];
    if (head[0] != xwp::kMagic || nc > 4096 || ne > 4096) return -1;
    if (in_words != xwp::in_words(nc, ne) || g_words != xwp::gWords) return -1;
    if (out_words != (phase ? xwp::out2_words() : xwp::out_words(nc, ne))) return -1;
    hipLaunchKernelGGL(xwp::probe_kernel, dim3(1), dim3(xwp::kThreads), 0, 0, (const uint32_t *)d_in, (uint32_t *)d_out, (uint32_t *)d_g, phase);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}
