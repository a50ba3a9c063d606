// nlzm_planes.hip -- the byte-plane kernels for gfx950: the planes role (nlzm_planes.h) in both directions, four waves per workgroup -- a wave's
// image is 8,320 bytes of LDS, a workgroup's 33,280 --, one wave per segment of a range, beyond max_blocks workgroups in a grid-wide stride.  The host
// side is nlzm_hip_planes.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_planes_host.h"
#include "nlzm_planes.h"

namespace nlzm {
__shared__ planes::Lds g_planes_lds[4];
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_planes_lds[0]); }
}
namespace nlzm {

constexpr uint32_t kPlanesThreads = 256;
static_assert(sizeof(g_planes_lds) == planes::lds_bytes(kPlanesThreads / 64), "one image per wave");

__device__ __forceinline__ planes::Args global_args(planes::Args a)       // (pointers handed over in a struct: global ones, not flat)
{
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.dst = NLZM_GLOBAL(uint8_t, a.dst);
    a.src_off = NLZM_GLOBAL(const unsigned long long, a.src_off);
    a.dst_off = NLZM_GLOBAL(const unsigned long long, a.dst_off);
    a.len = NLZM_GLOBAL(const unsigned long long, a.len);
    a.elem = NLZM_GLOBAL(const unsigned long long, a.elem);
    a.seg0 = NLZM_GLOBAL(const unsigned long long, a.seg0);
    return a;
}

__global__ __launch_bounds__(kPlanesThreads) void planes_forward_kernel(planes::Args args)
{
    const planes::Args a = global_args(args);
    planes::planes_role(a, false, units::wave<kPlanesThreads>(), units::waves<kPlanesThreads>());
}

__global__ __launch_bounds__(kPlanesThreads) void planes_inverse_kernel(planes::Args args)
{
    const planes::Args a = global_args(args);
    planes::planes_role(a, true, units::wave<kPlanesThreads>(), units::waves<kPlanesThreads>());
}

// ONE launch for all ranges of a call; no segment, no launch
void launch_planes(const planes::Args &a, bool inverse, uint32_t max_blocks, hipStream_t st)
{
    if (!a.nsegs) return;
    const dim3 grid = units::grid<kPlanesThreads>(a.nsegs, max_blocks);
    if (inverse) hipLaunchKernelGGL(planes_inverse_kernel, grid, dim3(kPlanesThreads), 0, st, a);
    else hipLaunchKernelGGL(planes_forward_kernel, grid, dim3(kPlanesThreads), 0, st, a);
}

}  // namespace nlzm
