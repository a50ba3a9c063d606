// nlzm_container_plan.h -- what the HOST decides when a block container has more blocks than one persistent launch holds, with no device in
// it: integers in, a table out.  nlzm_hip_blocks.cpp (nlzm_hip_blocks_begin, nlzm_hip_compress_blocks_dev), nlzm_hip_multi.cpp and the CPU harness
// tests/host_sim/container_plan_sim.cpp include this one text, so that what the test proves is what the library runs:
//   container::block_range   block i of the ceil(n / nblocks) partition (nlzm_amd/shard.py block_range, nlzm_hip_blocks_begin; a device's part of a multi-GPU call)
//   container::make_plan     the sets: which blocks in which set, each set's byte range, the bound of what the whole container may take
//   container::make_ranges_plan   the same for blocks that are ranges of the caller's choosing (nlzm_hip_compress_ranges*; the CPU harness
//                            tests/host_sim/ranges_plan_sim.cpp): the ranges checked against the input, the sets, each set's longest range, the bound
// The sets run one after another, each through the block-set code with the partition fixed to `per` bytes a block; a set's streams go straight
// behind those of the set before it.  Standard library only; compiles with plain g++ -std=c++17.
#pragma once

#include <stdint.h>

#include <vector>

#include "nlzm_read_plan.h"

namespace nlzm {
namespace container {

constexpr uint32_t kMaxBlocks = 65536;              // what every read-side entry point and the .idx reader accept
constexpr uint32_t kDefaultSetBlocks = 32;          // option "container_set_blocks": an MI355X does best with 32 to 40 streams at once

// block i of nblocks over n bytes, `per` = ceil(n / nblocks) bytes a block: [lo, lo + len), empty behind the input's end
inline uint64_t per_block(uint64_t n, uint64_t nblocks) { return nblocks ? n / nblocks + (n % nblocks ? 1 : 0) : n; }   // (no n + nblocks - 1: it can wrap)
inline void block_range(uint64_t n, uint64_t per, uint32_t i, uint64_t &lo, uint64_t &len)
{
    // (no i * per before it is known to fit: per > n / i says i * per > n, and the block starts at the input's end)
    lo = i && per > n / i ? n : (uint64_t)i * per;
    len = n - lo < per ? n - lo : per;
}

struct Set {
    uint32_t first = 0, count = 0;                  // blocks [first, first + count)
    uint64_t off = 0, len = 0;                      // their bytes: [off, off + len) of the input, the blocks' ranges back to back
};
struct Plan {
    uint32_t nblocks = 0;
    uint64_t per = 0;                               // bytes per block (the last non-empty one may hold fewer)
    std::vector<Set> sets;                          // in block order
    uint64_t out_bound = 0;                         // sum of bound(block's length) over all blocks: what the container can take at most
};

// nblocks <= capacity: ONE set, whatever set_blocks says (today's path).  Otherwise ceil(nblocks / set_blocks) sets, as equal as they can be:
// the first nblocks % nsets of them hold one block more than the others (65 blocks by 32: 22 + 22 + 21, not 32 + 32 + 1).
// bound(len): an upper bound of the stream of a block of len bytes (nlzm_hip_compress_bound).
template <class Bound>
inline int make_plan(Plan &P, uint64_t n, uint32_t nblocks, uint32_t set_blocks, uint32_t capacity, Bound bound, ErrText err)
{
    P = Plan{};
    if (!nblocks || nblocks > kMaxBlocks) return plan_error(err, NLZM_HIP_E_ARG, "nblocks out of range (1 .. %u)", kMaxBlocks);
    if (!capacity) return plan_error(err, NLZM_HIP_E_ARG, "the device holds no block set");
    if (!set_blocks || set_blocks > capacity) return plan_error(err, NLZM_HIP_E_ARG, "container_set_blocks %u out of range (1 .. %u)", set_blocks, capacity);
    P.nblocks = nblocks;
    P.per = per_block(n, nblocks);
    const uint32_t nsets = nblocks <= capacity ? 1u : nblocks / set_blocks + (nblocks % set_blocks ? 1u : 0u);
    const uint32_t base = nblocks / nsets, more = nblocks % nsets;
    P.sets.resize(nsets);
    uint32_t at = 0;
    for (uint32_t s = 0; s < nsets; s++) {
        Set &S = P.sets[s];
        S.first = at; S.count = base + (s < more ? 1u : 0u);
        uint64_t lo = 0, len = 0, hi_lo = 0, hi_len = 0;
        block_range(n, P.per, S.first, lo, len);
        block_range(n, P.per, S.first + S.count - 1, hi_lo, hi_len);
        S.off = lo; S.len = hi_lo + hi_len - lo;
        at += S.count;
    }
    for (uint32_t i = 0; i < nblocks; i++) {
        uint64_t lo = 0, len = 0;
        block_range(n, P.per, i, lo, len);
        const uint64_t b = bound(len);
        if (b > ~0ull - P.out_bound) return plan_error(err, NLZM_HIP_E_ARG, "the blocks' bounds do not sum in 64 bits");
        P.out_bound += b;
    }
    return 0;
}

// ---- ranges of the caller's choosing (nlzm_hip_compress_ranges*) ----
// Range i is [off[i], off[i] + len[i]) of n bytes: empty, overlapping, repeated, in any order.  The sets are consecutive ranges, split by the
// same rule as make_plan's (k <= capacity: ONE set); a set's streams share the decisions of its LONGEST range, as the equal split's share those of `per`.
struct RangeSet {
    uint32_t first = 0, count = 0;                  // ranges [first, first + count)
    uint64_t longest = 0;                           // the longest of them
};
struct RangesPlan {
    uint32_t k = 0;
    std::vector<RangeSet> sets;                     // in the caller's order
    uint64_t out_bound = 0;                         // sum of bound(len[i]): what the streams can take at most
    uint32_t bad_range = ~0u;                       // the range that runs over n, when that is the error
};

// the sum of bound(len[i]) over k ranges; false: k out of range, or the sum does not fit 64 bits
template <class Bound>
inline bool ranges_bound(uint32_t k, const uint64_t *len, Bound bound, uint64_t &sum)
{
    sum = 0;
    if (!k || k > kMaxBlocks || !len) return false;
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t b = bound(len[i]);
        if (b > ~0ull - sum) return false;
        sum += b;
    }
    return true;
}

template <class Bound>
inline int make_ranges_plan(RangesPlan &P, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t set_blocks, uint32_t capacity, Bound bound, ErrText err)
{
    P = RangesPlan{};
    if (!k || k > kMaxBlocks) return plan_error(err, NLZM_HIP_E_ARG, "%u ranges: 1 .. %u in one call", k, kMaxBlocks);
    if (!off || !len) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    if (!capacity) return plan_error(err, NLZM_HIP_E_ARG, "the device holds no block set");
    if (!set_blocks || set_blocks > capacity) return plan_error(err, NLZM_HIP_E_ARG, "container_set_blocks %u out of range (1 .. %u)", set_blocks, capacity);
    for (uint32_t i = 0; i < k; i++)
        if (off[i] > n || len[i] > n - off[i]) {    // (no off + len: it can wrap)
            P.bad_range = i;
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes of the input", i, (unsigned long long)off[i],
                              (unsigned long long)len[i], (unsigned long long)n);
        }
    if (!ranges_bound(k, len, bound, P.out_bound)) return plan_error(err, NLZM_HIP_E_ARG, "the ranges' bounds do not sum in 64 bits");
    P.k = k;
    const uint32_t nsets = k <= capacity ? 1u : k / set_blocks + (k % set_blocks ? 1u : 0u);
    const uint32_t base = k / nsets, more = k % nsets;
    P.sets.resize(nsets);
    uint32_t at = 0;
    for (uint32_t s = 0; s < nsets; s++) {
        RangeSet &S = P.sets[s];
        S.first = at; S.count = base + (s < more ? 1u : 0u);
        for (uint32_t i = S.first; i < S.first + S.count; i++) if (len[i] > S.longest) S.longest = len[i];
        at += S.count;
    }
    return 0;
}

}  // namespace container
}  // namespace nlzm
