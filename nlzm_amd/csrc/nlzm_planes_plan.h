// nlzm_planes_plan.h -- what the HOST decides for the byte-plane filter, with no device in it: integers in, integers and tables out.  nlzm_hip_planes.cpp
// and the CPU harness tests/host_sim/planes_plan_sim.cpp include this one text, so that what the test proves is what the library runs.
//
//   planes::check_elems    k and every element size: 1, 2, 4 or 8, else NLZM_HIP_E_ARG, and the text names the range
//   planes::check_ranges   ... and every range against both buffers (len > src_len - src_off, len > dst_len - dst_off: NLZM_HIP_E_ARG, named), the
//                          destinations against each other -- sorted by dst_off, empty ones left out, a range that starts before the one in front of it
//                          ends overlaps it: NLZM_HIP_E_ARG, both named -- and the two buffers against each other (there is no in-place form)
//   planes::check_typed_ranges   k, the element sizes and every range of a typed call against its one buffer (check_in_buffer, nlzm_read_plan.h)
//   planes::Table          the launch's arguments (planes::Args, nlzm_planes.h): src_off, dst_off, len, elem of every range and seg0, k + 1 entries --
//                          range r owns segments [seg0[r], seg0[r + 1]) of `segment` bytes --, one array, one upload
//   planes::runs           the destinations as sorted runs of bytes that lie back to back: what a host-buffer call copies back
//   planes::Layout         the typed compress and decode calls' scratch: range i's filtered bytes lie at at[i] = len[0] + ... + len[i - 1], `total` bytes
//                          in all, and the allocation holds `pad` bytes more behind them (what the compress path reads behind its input)
// Standard library only; compiles with plain g++ -std=c++17.  An error leaves as an NLZM_HIP_E_* code and its text in the caller's buffer.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "nlzm_read_plan.h"

namespace nlzm {
namespace planes {

constexpr uint32_t kMaxRanges = 65536;
constexpr uint64_t kPad = 128;                      // readable bytes the compress path wants behind its input

inline bool elem_ok(uint64_t e) { return e == 1 || e == 2 || e == 4 || e == 8; }

inline int check_elems(uint32_t k, const uint8_t *elem, ErrText err)
{
    if (!k || k > kMaxRanges) return plan_error(err, NLZM_HIP_E_ARG, "%u ranges: 1 .. %u in one call", k, kMaxRanges);
    if (!elem) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    for (uint32_t i = 0; i < k; i++)
        if (!elem_ok(elem[i])) return plan_error(err, NLZM_HIP_E_ARG, "range %u: element size %u (1, 2, 4 or 8)", i, (unsigned)elem[i]);
    return 0;
}

// src_at / dst_at: the buffers' addresses as integers (device or host: they are only compared)
inline int check_ranges(uint64_t src_at, uint64_t src_len, uint64_t dst_at, uint64_t dst_len, uint32_t k, const uint64_t *src_off, const uint64_t *dst_off,
                        const uint64_t *len, const uint8_t *elem, ErrText err)
{
    if (const int rc = check_elems(k, elem, err)) return rc;
    if (!src_off || !dst_off || !len) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    for (uint32_t i = 0; i < k; i++) {
        if (src_off[i] > src_len || len[i] > src_len - src_off[i])      // (no off + len: it can wrap)
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes of the source", i, (unsigned long long)src_off[i],
                              (unsigned long long)len[i], (unsigned long long)src_len);
        if (dst_off[i] > dst_len || len[i] > dst_len - dst_off[i])
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes of the destination", i, (unsigned long long)dst_off[i],
                              (unsigned long long)len[i], (unsigned long long)dst_len);
    }
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < k; i++) if (len[i]) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return dst_off[x] != dst_off[y] ? dst_off[x] < dst_off[y] : x < y; });
    for (size_t j = 1; j < order.size(); j++) {
        const uint32_t a = order[j - 1], b = order[j];
        if (dst_off[b] - dst_off[a] < len[a])
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (destination offset %llu, %llu bytes) overlaps range %u (destination offset %llu)", a,
                              (unsigned long long)dst_off[a], (unsigned long long)len[a], b, (unsigned long long)dst_off[b]);
    }
    // the buffers: [src_at, src_at + src_len) and [dst_at, dst_at + dst_len) share no byte (an empty buffer shares none)
    if (src_len && dst_len) {
        const bool apart = src_at < dst_at ? dst_at - src_at >= src_len : src_at - dst_at >= dst_len;
        if (!apart) return plan_error(err, NLZM_HIP_E_ARG, "the source and the destination buffer overlap (there is no in-place form)");
    }
    return 0;
}

// the ranges of a typed call against the n bytes of their buffer, and the element sizes
inline int check_typed_ranges(uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem, ErrText err)
{
    if (const int rc = check_elems(k, elem, err)) return rc;
    if (!off || !len) return plan_error(err, NLZM_HIP_E_ARG, "null argument");
    for (uint32_t i = 0; i < k; i++) if (const int rc = check_in_buffer(i, off[i], len[i], n, err)) return rc;
    return 0;
}

// the destinations of checked ranges as runs (offset, bytes), ascending: ranges that lie back to back are one run
inline std::vector<std::pair<uint64_t, uint64_t>> runs(uint32_t k, const uint64_t *dst_off, const uint64_t *len)
{
    std::vector<std::pair<uint64_t, uint64_t>> r;
    for (uint32_t i = 0; i < k; i++) if (len[i]) r.emplace_back(dst_off[i], len[i]);
    std::sort(r.begin(), r.end());
    size_t n = 0;
    for (size_t j = 0; j < r.size(); j++) {
        if (n && r[n - 1].first + r[n - 1].second == r[j].first) r[n - 1].second += r[j].second;
        else r[n++] = r[j];
    }
    r.resize(n);
    return r;
}

struct Table {
    std::vector<unsigned long long> words;          // src_off, dst_off, len, elem: k entries each; seg0: k + 1
    uint32_t k = 0;
    unsigned long long nsegs = 0, bytes = 0;
    // a's tables are this one at `base` (the host's copy, or one in device memory)
    template <class Args> void point(Args &a, const unsigned long long *base) const
    {
        a.src_off = base; a.dst_off = base + k; a.len = base + 2 * (size_t)k; a.elem = base + 3 * (size_t)k; a.seg0 = base + 4 * (size_t)k;
        a.k = k; a.nsegs = nsegs;
    }
    // checked ranges (check_ranges)
    int make(uint32_t n, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, const uint8_t *elem, unsigned long long segment, ErrText err)
    {
        k = n; nsegs = 0; bytes = 0;
        words.assign(5 * (size_t)n + 1, 0);
        unsigned long long *w = words.data();
        for (uint32_t i = 0; i < n; i++) {
            w[i] = src_off[i]; w[(size_t)n + i] = dst_off[i]; w[2 * (size_t)n + i] = len[i]; w[3 * (size_t)n + i] = elem[i]; w[4 * (size_t)n + i] = nsegs;
            nsegs += units::count(len[i], segment);
            bytes += len[i];                        // (ranges inside a buffer whose destinations do not overlap: below 2^64)
            if (nsegs > (1ull << 40)) return plan_error(err, NLZM_HIP_E_ARG, "the ranges of one call may hold 2^40 segments of %llu bytes in all", segment);
        }
        w[4 * (size_t)n + n] = nsegs;
        return 0;
    }
};

struct Layout {
    std::vector<uint64_t> at;                       // k entries
    uint64_t total = 0, alloc = 0;
    int make(uint32_t k, const uint64_t *len, uint64_t pad, ErrText err)
    {
        at.assign(k, 0); total = 0;
        for (uint32_t i = 0; i < k; i++) {
            at[i] = total;
            if (len[i] > ~0ull - pad - total) return plan_error(err, NLZM_HIP_E_ARG, "the ranges' lengths do not sum in 64 bits");
            total += len[i];
        }
        alloc = total + pad;
        return 0;
    }
};

}  // namespace planes
}  // namespace nlzm
