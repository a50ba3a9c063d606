// nlzm_units.h -- the unit table of the range kernels, once.  k entries -- ranges, pieces, pairs -- are ONE launch: entry i is
// cut into units of `unit` bytes counted from its own first byte and owns units [t[i], t[i + 1]) of the launch, t[0] = 0; an entry that owns nothing
// repeats its successor's start.  One wave takes one unit, and beyond max_blocks workgroups the waves stride.  The gather role (nlzm_range.h), the
// CRC's segments (nlzm_crc.h), the equal-range finder (nlzm_dedup.h) and the byte planes (nlzm_planes.h) find a unit's owner here; the host plans
// (nlzm_read_plan.h, nlzm_planes_plan.h) and host files build the table here; the kernel files take their wave index and their grid from here.
//
// Three builds of this one text: device code and -DNLZM_SIM, against xw.h like the role headers; and plain g++ -std=c++17, where the host plans and
// tests/host_sim/units_sim.cpp (tests/test_units_sim.py) include it.  The host half uses the standard library only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(NLZM_SIM) || defined(__HIP__)
#include "xw.h"
#define NLZM_UNITS_FN XW_FN
#else
#define NLZM_UNITS_FN inline
#endif

// a pointer handed over in a struct or read from memory: a global one, not a flat one
#if defined(__HIP__) && !defined(NLZM_SIM)
#define NLZM_GLOBAL(T, x) ((T *)(__attribute__((address_space(1))) T *)(unsigned long long)(x))
#else
#define NLZM_GLOBAL(T, x) ((T *)(x))
#endif

namespace nlzm {
namespace units {

// the owner of unit u: the last r < n with table[r] <= u (n >= 1 and table[0] = 0 <= u).  Entries that own nothing repeat their successor's start,
// so "the last" is never one of them while u < table[n]: some entry behind them holds the unit.
NLZM_UNITS_FN uint32_t owner_of(const unsigned long long *table, uint32_t n, unsigned long long u)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t m = lo + (hi - lo) / 2; if (table[m] <= u) lo = m; else hi = m; }
    return lo;
}

// ceil(len / unit) with no len + unit - 1, which wraps
inline unsigned long long count(unsigned long long len, unsigned long long unit) { return len / unit + (len % unit ? 1 : 0); }

// the table of n entries, n + 1 words: table[i + 1] - table[i] = count(len_of(i), unit)
template <class Len>
std::vector<unsigned long long> prefix(uint32_t n, unsigned long long unit, Len len_of)
{
    std::vector<unsigned long long> t((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) t[i + 1] = t[i] + count(len_of(i), unit);
    return t;
}

// the grid of a launch: a workgroup per per_block units, max_blocks at most (beyond them the waves stride).  units + per_block does not wrap: the
// tables refuse long before.
inline uint32_t blocks_for(unsigned long long units, uint32_t per_block, uint32_t max_blocks)
{
    const unsigned long long want = (units + per_block - 1) / per_block;
    return (uint32_t)(want < max_blocks ? want : max_blocks);
}

#if defined(__HIP__) && !defined(NLZM_SIM)
// a kernel of kThreads threads a workgroup: its wave among all waves of the grid, their number, and the grid for `n` units, one wave each
template <uint32_t kThreads> XW_FN unsigned long long wave() { return (unsigned long long)blockIdx.x * (kThreads / 64) + xw::wave(); }
template <uint32_t kThreads> XW_FN unsigned long long waves() { return (unsigned long long)gridDim.x * (kThreads / 64); }
template <uint32_t kThreads> inline dim3 grid(unsigned long long n, uint32_t max_blocks) { return dim3(blocks_for(n, kThreads / 64, max_blocks)); }
#endif

}  // namespace units
}  // namespace nlzm
