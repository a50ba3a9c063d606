// nlzm_dedup_plan.h -- what the HOST makes of the ranges' fingerprints, with no device in it: first_of[i] = the smallest j <= i whose range holds
// the same bytes as range i (a range is equal to itself).  nlzm_hip_dedup.cpp and the CPU harness tests/host_sim/dedup_plan_sim.cpp include this
// one text, so that what the test proves is what the library runs.
//
//   dedup::check_ranges   k and every range against the buffer: a range with len > buf_len - off is NLZM_HIP_E_ARG, and the text names it
//   (the launches' tables -- segments of a range's fingerprint, chunks of a pair's compare -- are units::prefix, nlzm_units.h)
//   dedup::class_plan     the classes.  Two ranges with the same (off, len) are equal without a compare, and all empty ranges are equal to the first
//                         empty one: every range stands for the smallest index of its (off, len) -- of the empty ones -- and only those take part.
//                         They are grouped by (length, fingerprint's low hash_bits bits).  A round: in every group with two unresolved members or
//                         more the smallest unresolved index is the representative, and the pairs (representative, every other unresolved member)
//                         go to `compare`; members it finds equal are resolved to the representative, the others stay for the next round, the
//                         representative is resolved as its own first (so is a group's only unresolved member).  Rounds until no pair is left.
// The result is exact whatever the fingerprints are: equal bytes have equal lengths and fingerprints, so equal ranges share a group, and a member is
// resolved to a representative only by a compare.  A collision costs a round, never a wrong answer: a group of d distinct contents takes at most d
// rounds, and with fingerprints that tell all contents apart there is one.  Standard library only; compiles with plain g++ -std=c++17.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nlzm_read_plan.h"

namespace nlzm {
namespace dedup {

constexpr uint32_t kMaxRanges = 65536;

struct IndexPair { uint32_t rep, member; };         // ranges, by index: rep < member
struct Classes {
    std::vector<uint32_t> first_of;
    uint64_t distinct = 0;                          // ranges that are their own first
    uint64_t dup_bytes = 0;                         // bytes of the ranges that are another's copy
    uint64_t rounds = 0, pairs = 0, compared_bytes = 0;    // compared_bytes: the pairs' lengths (each side's)
};

inline int check_ranges(uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, ErrText err)
{
    if (!k || k > kMaxRanges) return plan_error(err, NLZM_HIP_E_ARG, "%u ranges: 1 .. %u in one call", k, kMaxRanges);
    if (!off || !len) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    for (uint32_t i = 0; i < k; i++) if (const int rc = check_in_buffer(i, off[i], len[i], buf_len, err)) return rc;
    return 0;
}

inline uint64_t mask_of(uint32_t hash_bits) { return hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1; }

// compare(pairs, equal): equal[p] = 1 when the ranges of pairs[p] hold the same bytes, else 0 (equal comes sized and zeroed); returns 0, or an
// error code that ends the plan.  The ranges are valid (check_ranges).
template <class Compare>
inline int class_plan(Classes &R, uint32_t k, const uint64_t *off, const uint64_t *len, const uint64_t *fp, uint32_t hash_bits, Compare compare)
{
    R = Classes{};
    R.first_of.assign(k, 0);
    const uint64_t mask = mask_of(hash_bits);
    // stands[i]: the smallest index with range i's (off, len); every empty range's is the first empty one
    std::vector<uint32_t> order(k), stands(k);
    for (uint32_t i = 0; i < k; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (len[x] != len[y]) return len[x] < len[y];
        if (len[x] && off[x] != off[y]) return off[x] < off[y];
        return x < y;
    });
    for (uint32_t at = 0; at < k;) {
        uint32_t end = at + 1;
        while (end < k && len[order[end]] == len[order[at]] && (!len[order[at]] || off[order[end]] == off[order[at]])) end++;
        for (uint32_t j = at; j < end; j++) stands[order[j]] = order[at];
        at = end;
    }
    // the groups of those that stand for themselves: by (length, masked fingerprint), members in index order
    std::vector<uint32_t> own;
    for (uint32_t i = 0; i < k; i++) if (stands[i] == i) own.push_back(i);
    std::sort(own.begin(), own.end(), [&](uint32_t x, uint32_t y) {
        if (len[x] != len[y]) return len[x] < len[y];
        if ((fp[x] & mask) != (fp[y] & mask)) return (fp[x] & mask) < (fp[y] & mask);
        return x < y;
    });
    std::vector<std::vector<uint32_t>> groups;      // the unresolved members of every group that still has two
    for (size_t at = 0; at < own.size();) {
        size_t end = at + 1;
        while (end < own.size() && len[own[end]] == len[own[at]] && (fp[own[end]] & mask) == (fp[own[at]] & mask)) end++;
        if (end - at == 1) R.first_of[own[at]] = own[at];
        else groups.emplace_back(own.begin() + at, own.begin() + end);
        at = end;
    }
    std::vector<IndexPair> pairs;
    std::vector<uint8_t> equal;
    while (!groups.empty()) {
        pairs.clear();
        for (const auto &g : groups)
            for (size_t j = 1; j < g.size(); j++) { pairs.push_back(IndexPair{ g[0], g[j] }); R.compared_bytes += len[g[0]]; }
        equal.assign(pairs.size(), 0);
        if (const int rc = compare(pairs, equal)) return rc;
        R.rounds++;
        R.pairs += pairs.size();
        size_t p = 0;
        std::vector<std::vector<uint32_t>> next;
        for (auto &g : groups) {
            R.first_of[g[0]] = g[0];
            std::vector<uint32_t> rest;
            for (size_t j = 1; j < g.size(); j++, p++) {
                if (equal[p]) R.first_of[g[j]] = g[0];
                else rest.push_back(g[j]);
            }
            if (rest.size() == 1) R.first_of[rest[0]] = rest[0];
            else if (rest.size() > 1) next.push_back(std::move(rest));
        }
        groups.swap(next);
    }
    for (uint32_t i = 0; i < k; i++) {
        if (stands[i] != i) R.first_of[i] = R.first_of[stands[i]];
        if (R.first_of[i] == i) R.distinct++;
        else R.dup_bytes += len[i];
    }
    return 0;
}

}  // namespace dedup
}  // namespace nlzm
