// nlzm_elem_plan.h -- what the HOST decides for the choice of a typed range's element size, with no device in it: integers in,
// integers and tables out.  nlzm_hip_elem.cpp and the CPU harnesses tests/host_sim/elem_plan_sim.cpp and elem_sim.cpp include this one text, so that
// what the tests prove is what the library runs.
//
//   elem::check_ranges   k (1 .. kMaxRanges), the arrays, every range against the n bytes of its buffer (check_in_buffer, nlzm_read_plan.h: no
//                        off + len) and against kMaxLen -- a range of 2^40 bytes or more is NLZM_HIP_E_ARG, because N L(N) has to fit 64 bits --;
//                        every text names its range
//   elem::Table          the launch's arguments (elem::Args, nlzm_elem.h), one array, one upload: off, len and slot of every range, seg0 (k + 1
//                        entries: range r owns segments [seg0[r], seg0[r + 1]) of `segment` bytes of its first 8 (len div 8) bytes), and the list of
//                        the ranges of more than one segment.  slot[r] is where the range's 2,048 totals lie, in units of 2,048 words: r itself when
//                        the caller wants the histograms, else the range's place among those of more than one segment, kNoSlot for the others
//   elem::Scratch        the call's device memory beyond its input, in bytes: the table, a 32-byte record a range, 16 KiB of totals a slot
//   elem::choose         the choice for one range from its four costs and its length; pure
// Standard library only; compiles with plain g++ -std=c++17.  An error leaves as an NLZM_HIP_E_* code and its text in the caller's buffer.
#pragma once

#include <stdint.h>

#include <vector>

#include "nlzm_read_plan.h"

namespace nlzm {
namespace elem {

constexpr uint32_t kMaxRanges = 65536;
constexpr uint64_t kMaxLen = 1ull << 40;            // a range is shorter
constexpr uint64_t kMinLen = 4096;                  // a range below this is left at e = 1
constexpr uint64_t kShare = 32;                     // a plane split has to save more than C_1 / kShare
constexpr uint32_t kBins = 8 * 256;                 // H[c][v] of a range
constexpr unsigned long long kNoSlot = ~0ull;

inline int check_ranges(uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, ErrText err)
{
    if (!k || k > kMaxRanges) return plan_error(err, NLZM_HIP_E_ARG, "%u ranges: 1 .. %u in one call", k, kMaxRanges);
    if (!off || !len) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    for (uint32_t i = 0; i < k; i++) {
        if (const int rc = check_in_buffer(i, off[i], len[i], n, err)) return rc;
        if (len[i] >= kMaxLen)
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes): the statistic takes ranges below 2^40 bytes", i, (unsigned long long)off[i],
                              (unsigned long long)len[i]);
    }
    return 0;
}

// costs: C_1, C_2, C_4, C_8 in 2^-16 bits (each below 2^60 for a range below 2^40 bytes: no sum here wraps)
inline uint32_t choose(const uint64_t *cost4, uint64_t len)
{
    if (len < kMinLen) return 1;
    uint32_t b = 0;
    for (uint32_t i = 1; i < 4; i++) if (cost4[i] < cost4[b]) b = i;        // (ties stay with the smaller e)
    if (b && cost4[b] + cost4[0] / kShare > cost4[0]) return 1;
    return 1u << b;
}

struct Table {
    std::vector<unsigned long long> words;          // off, len, slot: k entries each; seg0: k + 1; wide: nwide
    uint32_t k = 0, nwide = 0;
    unsigned long long nsegs = 0, bytes = 0, nslots = 0;
    // a's tables are this one at `base` (the host's copy, or one in device memory)
    template <class Args> void point(Args &a, const unsigned long long *base) const
    {
        a.off = base; a.len = base + k; a.slot = base + 2 * (size_t)k; a.seg0 = base + 3 * (size_t)k; a.wide = base + 4 * (size_t)k + 1;
        a.k = k; a.nwide = nwide; a.nsegs = nsegs;
    }
    // checked ranges (check_ranges); segment: a multiple of 16
    void make(uint32_t n, const uint64_t *off, const uint64_t *len, unsigned long long segment, bool want_hist)
    {
        k = n; nwide = 0; nsegs = 0; bytes = 0;
        words.assign(4 * (size_t)n + 1, 0);
        for (uint32_t i = 0; i < n; i++) {
            const unsigned long long segs = units::count(len[i] & ~7ull, segment);
            words[i] = off[i]; words[(size_t)n + i] = len[i]; words[3 * (size_t)n + i] = nsegs;
            words[2 * (size_t)n + i] = want_hist ? i : segs > 1 ? nwide : kNoSlot;
            if (segs > 1) { words.push_back(i); nwide++; }
            nsegs += segs;                          // (65,536 ranges below 2^40 bytes: below 2^56 bytes in all)
            bytes += len[i];
        }
        words[3 * (size_t)n + n] = nsegs;
        nslots = want_hist ? n : nwide;
    }
};

struct Scratch {
    uint64_t table = 0, cost = 0, totals = 0;
    uint64_t bytes() const { return table + cost + totals; }
    explicit Scratch(const Table &T) : table(T.words.size() * 8), cost((uint64_t)T.k * 32), totals(T.nslots * kBins * 8) {}
};

}  // namespace elem
}  // namespace nlzm
