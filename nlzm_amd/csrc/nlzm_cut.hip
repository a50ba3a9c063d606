// nlzm_cut.hip -- the cut-point kernels for gfx950: the scan role (nlzm_cut.h), one wave per workgroup -- a wave's stage and the table are
// 34 KiB of LDS, four workgroups to a CU -- taking segments in a grid-wide stride, and the select role, one wave in all.  The host side is
// nlzm_hip_cut.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_cut_host.h"
#include "nlzm_cut.h"
#include "nlzm_units.h"

namespace nlzm {
__shared__ cut::Lds g_cut_lds;
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_cut_lds); }
}
namespace nlzm {

constexpr uint32_t kCutThreads = 64;

__device__ __forceinline__ cut::Args global_args(cut::Args a)               // (pointers handed over in a struct: global ones, not flat)
{
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.bits = NLZM_GLOBAL(uint32_t, a.bits);
    a.count = NLZM_GLOBAL(uint32_t, a.count);
    a.cut = NLZM_GLOBAL(unsigned long long, a.cut);
    a.res = NLZM_GLOBAL(unsigned long long, a.res);
    return a;
}

__global__ __launch_bounds__(kCutThreads) void cut_scan_kernel(cut::Args args)
{
    const cut::Args a = global_args(args);
    cut::scan_role(a, kCutThreads, blockIdx.x, gridDim.x);      // (one wave a workgroup: the workgroup's index is the wave's)
}

__global__ __launch_bounds__(kCutThreads) void cut_select_kernel(cut::Args args)
{
    const cut::Args a = global_args(args);
    cut::select_role(a);
}

// both launches of one call: every segment's candidates -- a workgroup per segment, beyond max_blocks workgroups they stride -- then the selection
void launch_cut(const cut::Args &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.nsegs) return;
    hipLaunchKernelGGL(cut_scan_kernel, units::grid<kCutThreads>(a.nsegs, max_blocks), dim3(kCutThreads), 0, st, a);
    hipLaunchKernelGGL(cut_select_kernel, dim3(1), dim3(kCutThreads), 0, st, a);
}

}  // namespace nlzm
