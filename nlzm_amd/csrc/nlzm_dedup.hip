// nlzm_dedup.hip -- the equal-range finder's kernels for gfx950: the four roles of nlzm_dedup.h, four waves per workgroup, one wave per segment,
// range, chunk or pair, beyond max_blocks workgroups in a grid-wide stride.  The host side is nlzm_hip_dedup.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_dedup_host.h"
#include "nlzm_dedup.h"

namespace nlzm {

constexpr uint32_t kDedupThreads = 256;

__device__ __forceinline__ dedup::FpArgs global_args(dedup::FpArgs a)       // (pointers handed over in a struct: global ones, not flat)
{
    a.buf = NLZM_GLOBAL(const uint8_t, a.buf);
    a.off = NLZM_GLOBAL(const unsigned long long, a.off);
    a.len = NLZM_GLOBAL(const unsigned long long, a.len);
    a.seg0 = NLZM_GLOBAL(const unsigned long long, a.seg0);
    a.seg_h = NLZM_GLOBAL(unsigned long long, a.seg_h);
    a.fp = NLZM_GLOBAL(unsigned long long, a.fp);
    return a;
}
__device__ __forceinline__ dedup::PairArgs global_args(dedup::PairArgs a)
{
    a.buf = NLZM_GLOBAL(const uint8_t, a.buf);
    a.pairs = NLZM_GLOBAL(const dedup::Pair, a.pairs);
    a.chunk0 = NLZM_GLOBAL(const unsigned long long, a.chunk0);
    a.chunk_ne = NLZM_GLOBAL(uint32_t, a.chunk_ne);
    a.equal = NLZM_GLOBAL(uint32_t, a.equal);
    return a;
}

__global__ __launch_bounds__(kDedupThreads) void dedup_fingerprint_kernel(dedup::FpArgs args)
{
    const dedup::FpArgs a = global_args(args);
    dedup::fingerprint_role(a, units::wave<kDedupThreads>(), units::waves<kDedupThreads>());
}
__global__ __launch_bounds__(kDedupThreads) void dedup_combine_kernel(dedup::FpArgs args)
{
    const dedup::FpArgs a = global_args(args);
    dedup::combine_role(a, units::wave<kDedupThreads>(), units::waves<kDedupThreads>());
}
__global__ __launch_bounds__(kDedupThreads) void dedup_pair_kernel(dedup::PairArgs args)
{
    const dedup::PairArgs a = global_args(args);
    dedup::pair_role(a, units::wave<kDedupThreads>(), units::waves<kDedupThreads>());
}
__global__ __launch_bounds__(kDedupThreads) void dedup_verdict_kernel(dedup::PairArgs args)
{
    const dedup::PairArgs a = global_args(args);
    dedup::verdict_role(a, units::wave<kDedupThreads>(), units::waves<kDedupThreads>());
}

// the fingerprints of all ranges of a call: every segment's sum (no segment, no launch), then every range's fingerprint
void launch_fingerprints(const dedup::FpArgs &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.k) return;
    if (a.nsegs) hipLaunchKernelGGL(dedup_fingerprint_kernel, units::grid<kDedupThreads>(a.nsegs, max_blocks), dim3(kDedupThreads), 0, st, a);
    hipLaunchKernelGGL(dedup_combine_kernel, units::grid<kDedupThreads>(a.k, max_blocks), dim3(kDedupThreads), 0, st, a);
}

// the verdicts of all pairs of a round: every chunk's word (no chunk, no launch), then every pair's
void launch_pairs(const dedup::PairArgs &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.npairs) return;
    if (a.nchunks) hipLaunchKernelGGL(dedup_pair_kernel, units::grid<kDedupThreads>(a.nchunks, max_blocks), dim3(kDedupThreads), 0, st, a);
    hipLaunchKernelGGL(dedup_verdict_kernel, units::grid<kDedupThreads>(a.npairs, max_blocks), dim3(kDedupThreads), 0, st, a);
}

}  // namespace nlzm
