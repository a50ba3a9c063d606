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

#define NLZM_G(T, x) ((T *)(__attribute__((address_space(1))) T *)(unsigned long long)(x))      // (pointers handed over in a struct: global ones, not flat)

constexpr uint32_t kCrcThreads = 256;
constexpr uint32_t kCombineThreads = 1024;

__device__ __forceinline__ crc::Args global_args(crc::Args a)
{
    a.buf = NLZM_G(const uint8_t, a.buf);
    a.off = NLZM_G(const unsigned long long, a.off);
    a.len = NLZM_G(const unsigned long long, a.len);
    a.seg0 = NLZM_G(const unsigned long long, a.seg0);
    a.part = NLZM_G(uint32_t, a.part);
    a.out = NLZM_G(uint32_t, a.out);
    return a;
}

__global__ __launch_bounds__(kCrcThreads) void crc_segments_kernel(crc::Args args)
{
    const crc::Args a = global_args(args);
    constexpr uint32_t wpb = kCrcThreads / 64;
    crc::segments_role(a, kCrcThreads, (unsigned long long)blockIdx.x * wpb + xw::wave(), (unsigned long long)gridDim.x * wpb);
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
    if (a.nsegs) {
        const unsigned long long want = (a.nsegs + kCrcThreads / 64 - 1) / (kCrcThreads / 64);
        hipLaunchKernelGGL(crc_segments_kernel, dim3((uint32_t)(want < max_blocks ? want : max_blocks)), dim3(kCrcThreads), 0, st, a);
    }
    hipLaunchKernelGGL(crc_combine_kernel, dim3(a.nranges), dim3(kCombineThreads), 0, st, a);
}

}  // namespace nlzm
