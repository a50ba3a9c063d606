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
    a.pieces = NLZM_GLOBAL(const range::Piece, a.pieces);
    a.chunk0 = NLZM_GLOBAL(const unsigned long long, a.chunk0);
    range::gather_role(a, units::wave<kGatherThreads>(), units::waves<kGatherThreads>());
}

// ONE launch for all pieces of a call; no chunk, no launch
void launch_gather(const range::Args &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.nchunks) return;
    hipLaunchKernelGGL(range_gather_kernel, units::grid<kGatherThreads>(a.nchunks, max_blocks), dim3(kGatherThreads), 0, st, a);
}

}  // namespace nlzm
