// nlzm_elem.hip -- the kernels of the element-size statistic for gfx950: the count role and the total role (nlzm_elem.h), four waves per workgroup -- a
// wave's counters are 8,192 bytes of LDS, a workgroup's 32,768 --, one wave per segment of a range and one wave per range of more than one segment,
// beyond max_blocks workgroups in a grid-wide stride.  The host side is nlzm_hip_elem.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_elem_host.h"
#include "nlzm_elem.h"

namespace nlzm {
__shared__ elem::Lds g_elem_lds[4];
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_elem_lds[0]); }
}
namespace nlzm {

constexpr uint32_t kElemThreads = 256;
static_assert(sizeof(g_elem_lds) == elem::lds_bytes(kElemThreads / 64), "one set of counters per wave");

__device__ __forceinline__ elem::Args global_args(elem::Args a)       // (pointers handed over in a struct: global ones, not flat)
{
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.off = NLZM_GLOBAL(const unsigned long long, a.off);
    a.len = NLZM_GLOBAL(const unsigned long long, a.len);
    a.slot = NLZM_GLOBAL(const unsigned long long, a.slot);
    a.seg0 = NLZM_GLOBAL(const unsigned long long, a.seg0);
    a.wide = NLZM_GLOBAL(const unsigned long long, a.wide);
    a.totals = NLZM_GLOBAL(unsigned long long, a.totals);
    a.cost = NLZM_GLOBAL(unsigned long long, a.cost);
    return a;
}

__global__ __launch_bounds__(kElemThreads) void elem_count_kernel(elem::Args args)
{
    const elem::Args a = global_args(args);
    elem::count_role(a, units::wave<kElemThreads>(), units::waves<kElemThreads>());
}

// (no LDS of its own use: the totals are read where they lie)
__global__ __launch_bounds__(kElemThreads) void elem_total_kernel(elem::Args args)
{
    const elem::Args a = global_args(args);
    elem::total_role(a, units::wave<kElemThreads>(), units::waves<kElemThreads>());
}

// the launches of a call, back to back on one stream: no segment, no launch; no range of more than one segment, no second launch
void launch_elem(const elem::Args &a, uint32_t max_blocks, hipStream_t st)
{
    if (!a.nsegs) return;
    hipLaunchKernelGGL(elem_count_kernel, units::grid<kElemThreads>(a.nsegs, max_blocks), dim3(kElemThreads), 0, st, a);
    if (a.nwide) hipLaunchKernelGGL(elem_total_kernel, units::grid<kElemThreads>(a.nwide, max_blocks), dim3(kElemThreads), 0, st, a);
}

}  // namespace nlzm
