// nlzm_range.hip -- the range reader's gather kernel for gfx950: the gather role (nlzm_range.h), four waves per workgroup, one wave per
// chunk of a piece, beyond max_blocks workgroups in a grid-wide stride.  The host side is nlzm_hip_range.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_range.h"

namespace nlzm {

constexpr uint32_t kGatherThreads = 256;

__global__ __launch_bounds__(kGatherThreads) void range_gather_kernel(range::Args args)
{
    range::Args a = args;
    a.pieces = NLZM_RANGE_G(const range::Piece, a.pieces);
    a.chunk0 = NLZM_RANGE_G(const unsigned long long, a.chunk0);
    constexpr uint32_t wpb = kGatherThreads / 64;
    range::gather_role(a, (unsigned long long)blockIdx.x * wpb + xw::wave(), (unsigned long long)gridDim.x * wpb);
}

// ONE launch for all pieces of a call; no chunk, no launch
void launch_gather(const range::Args &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.nchunks) return;
    const unsigned long long want = (a.nchunks + kGatherThreads / 64 - 1) / (kGatherThreads / 64);
    hipLaunchKernelGGL(range_gather_kernel, dim3((uint32_t)(want < max_blocks ? want : max_blocks)), dim3(kGatherThreads), 0, st, a);
}

}  // namespace nlzm
