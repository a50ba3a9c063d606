// nlzm_container_plan.h -- what the HOST decides when a block container has more blocks than one persistent launch holds, with no device in
// it: integers in, a table out.  nlzm_hip_blocks.cpp (nlzm_hip_blocks_begin, nlzm_hip_compress_blocks_dev), nlzm_hip_multi.cpp and the CPU harness
// tests/host_sim/container_plan_sim.cpp include this one text, so that what the test proves is what the library runs:
//   container::block_range   block i of the ceil(n / nblocks) partition (nlzm_amd/shard.py block_range, nlzm_hip_blocks_begin; a device's part of a multi-GPU call)
//   container::make_plan     the sets: which blocks in which set, each set's byte range, the bound of what the whole container may take
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

}  // namespace container
}  // namespace nlzm
