// nlzm_crc.hip -- the CRC32 kernels for gfx950: the segment role (nlzm_crc.h), four waves per workgroup that share one set of tables in
// LDS and take segments in a grid-wide stride, and the combine role, one wave per range.  The host side is nlzm_hip_crc.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_crc.h"

namespace nlzm {
__shared__ crc::Lds g_crc_lds;
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_crc_lds); }
}
namespace nlzm {

constexpr uint32_t kCrcThreads = 256;
constexpr uint32_t kCombineThreads = 1024;

__device__ __forceinline__ crc::Args global_args(crc::Args a)               // (pointers handed over in a struct: global ones, not flat)
{
    a.buf = NLZM_GLOBAL(const uint8_t, a.buf);
    a.off = NLZM_GLOBAL(const unsigned long long, a.off);
    a.len = NLZM_GLOBAL(const unsigned long long, a.len);
    a.seg0 = NLZM_GLOBAL(const unsigned long long, a.seg0);
    a.part = NLZM_GLOBAL(uint32_t, a.part);
    a.out = NLZM_GLOBAL(uint32_t, a.out);
    return a;
}

__global__ __launch_bounds__(kCrcThreads) void crc_segments_kernel(crc::Args args)
{
    const crc::Args a = global_args(args);
    crc::segments_role(a, kCrcThreads, units::wave<kCrcThreads>(), units::waves<kCrcThreads>());
}

__global__ __launch_bounds__(kCombineThreads) void crc_combine_kernel(crc::Args args)
{
    const crc::Args a = global_args(args);
    crc::combine_role(a, blockIdx.x, kCombineThreads);
}

// both launches of one call: every range's segments -- a workgroup per four of them, which the dispatcher deals out as CUs come free; beyond
// max_blocks workgroups they stride -- then every range's combine
void launch_crc(const crc::Args &a, uint32_t max_blocks, hipStream_t st)
{
    if (a.nsegs) hipLaunchKernelGGL(crc_segments_kernel, units::grid<kCrcThreads>(a.nsegs, max_blocks), dim3(kCrcThreads), 0, st, a);
    hipLaunchKernelGGL(crc_combine_kernel, dim3(a.nranges), dim3(kCombineThreads), 0, st, a);
}

}  // namespace nlzm
