// nlzm_read_plan.h -- what the HOST decides on the read path, with no device in it: integers in, integers and tables out.  The library's host
// files (nlzm_hip_range.cpp, nlzm_hip_crc.cpp, nlzm_hip_decode.cpp), the command line (nlzm_cli.cpp) and the simulator harnesses
// (tests/host_sim/range_sim.cpp, crc_sim.cpp) include this one text, so that what the tests prove is what the library runs:
//   equal_shares       the raw lengths of the blocks of a container made from n bytes (nlzm_hip_verify*)
//   range::make_plan   which bytes of which block a set of ranges needs, where each block is decoded to, which piece goes where
//   range::for_each_part   the walk both of its loops and the command line's slicing make: the non-empty blocks a range intersects
//   check_in_buffer    a range against the bytes of its buffer: the one text of that refusal
//   range::pack_pieces the gather launch's arguments: the non-empty pieces and their chunk prefix table (nlzm_units.h)
//   crc::SegTable      the CRC launch's arguments: off / len / seg0 of the ranges, checked against the buffer
// (the split of a host buffer into block streams by their frame headers sits beside stream_length: nlzm_host_decode.h, split_streams.)
// Standard library only; compiles with plain g++ -std=c++17.  An error leaves as an NLZM_HIP_E_* code and its text in the caller's buffer.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_units.h"

namespace nlzm {

struct ErrText { char *text; size_t cap; };
inline int plan_error(ErrText e, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (e.text && e.cap) vsnprintf(e.text, e.cap, fmt, ap);
    va_end(ap);
    return code;
}

// Range i, len bytes from off, against the buf_len bytes of its buffer (no off + len: it can wrap)
inline int check_in_buffer(uint32_t i, uint64_t off, uint64_t len, uint64_t buf_len, ErrText err)
{
    if (off <= buf_len && len <= buf_len - off) return 0;
    return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes of the buffer", i, (unsigned long long)off, (unsigned long long)len,
                      (unsigned long long)buf_len);
}

// The blocks of a container made from n bytes hold ceil(n / nblocks) bytes each, the last ones fewer
inline void equal_shares(uint64_t n, uint32_t nblocks, std::vector<uint64_t> &raw)
{
    raw.assign(nblocks, 0);
    const uint64_t per = (n + nblocks - 1) / nblocks;
    for (uint32_t i = 0; i < nblocks; i++) { const uint64_t lo = i * per < n ? i * per : n, hi = lo + per < n ? lo + per : n; raw[i] = hi - lo; }
}

namespace range {

constexpr uint64_t kNone = ~0ull;

// The plan of a call, from the blocks' raw lengths and the ranges alone (no device, no pointer):
//   start[b]   where block b's contents start in what the container holds (start[nblocks] = total)
//   need[b]    bytes of block b's contents from its first one up to the furthest any range wants (0: the block is not decoded)
//   place[b]   where they are decoded to: direct[b] -- an offset into the caller's destination, when exactly one range needs the block and
//              that range starts at or before the block's first byte --, else an offset into the scratch buffer
//   pieces     what the gather launch moves from the scratch buffer to the destination, in the ranges' order
struct PlanPiece { uint64_t scratch_off, dst_off, len; };
struct Plan {
    std::vector<uint64_t> start, need, place;
    std::vector<uint8_t> direct;
    std::vector<uint32_t> users;
    std::vector<PlanPiece> pieces;
    uint64_t total = 0, dst_len = 0, scratch = 0;
    uint32_t bad_range = ~0u;                       // the range that runs over the container, when that is the error
};

// f(b, from, to) for every non-empty block b that the range [off, off + len) intersects, in order: [from, to) is the intersection, in the
// container's offsets.  The range lies inside the container (make_plan checks it: off + len does not wrap).
template <class F>
inline void for_each_part(const std::vector<uint64_t> &start, uint32_t nblocks, uint64_t off, uint64_t len, F f)
{
    if (!len) return;
    const uint64_t hi = off + len;
    // the first block: the last b with start[b] <= off.  Blocks of raw length 0 share their start with the block behind them, so "the last"
    // is never one of them (off < total: some block behind holds the byte)
    uint32_t b = (uint32_t)(std::upper_bound(start.begin(), start.begin() + nblocks, off) - start.begin()) - 1;
    for (; b < nblocks && start[b] < hi; b++) {
        if (start[b + 1] == start[b]) continue;     // a block of raw length 0 is never needed
        f(b, off > start[b] ? off : start[b], hi < start[b + 1] ? hi : start[b + 1]);
    }
}

inline int make_plan(Plan &P, uint32_t nblocks, const uint64_t *raw, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint64_t dst_cap, ErrText err)
{
    P = Plan{};
    P.start.assign((size_t)nblocks + 1, 0);
    for (uint32_t b = 0; b < nblocks; b++) {
        if (raw[b] > ~0ull - P.start[b]) return plan_error(err, NLZM_HIP_E_ARG, "the blocks' raw lengths do not sum in 64 bits");
        P.start[b + 1] = P.start[b] + raw[b];
    }
    P.total = P.start[nblocks];
    P.need.assign(nblocks, 0); P.place.assign(nblocks, kNone); P.direct.assign(nblocks, 0); P.users.assign(nblocks, 0);
    for (uint32_t r = 0; r < nranges; r++) {
        if (off[r] > P.total || len[r] > P.total - off[r]) {     // (no off + len: it can wrap)
            P.bad_range = r;
            return plan_error(err, NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes the container holds", r, (unsigned long long)off[r],
                              (unsigned long long)len[r], (unsigned long long)P.total);
        }
        if (len[r] > ~0ull - P.dst_len) return plan_error(err, NLZM_HIP_E_ARG, "the ranges' lengths do not sum in 64 bits");
        P.dst_len += len[r];
    }
    if (P.dst_len > dst_cap) return plan_error(err, NLZM_HIP_E_CAPACITY, "the ranges hold %llu bytes, dst_cap %llu", (unsigned long long)P.dst_len, (unsigned long long)dst_cap);
    uint64_t at = 0;
    for (uint32_t r = 0; r < nranges; r++) {
        for_each_part(P.start, nblocks, off[r], len[r], [&](uint32_t b, uint64_t from, uint64_t to) {
            if (to - P.start[b] > P.need[b]) P.need[b] = to - P.start[b];
            if (!P.users[b]++ && from == P.start[b]) { P.direct[b] = 1; P.place[b] = at + (from - off[r]); }
            else P.direct[b] = 0;
        });
        at += len[r];
    }
    for (uint32_t b = 0; b < nblocks; b++)
        if (P.need[b] && !P.direct[b]) { P.place[b] = P.scratch; P.scratch += P.need[b]; }      // (sums of parts of the blocks: below total)
    at = 0;
    for (uint32_t r = 0; r < nranges; r++) {
        for_each_part(P.start, nblocks, off[r], len[r], [&](uint32_t b, uint64_t from, uint64_t to) {
            if (!P.direct[b]) P.pieces.push_back(PlanPiece{ P.place[b] + (from - P.start[b]), at + (from - off[r]), to - from });
        });
        at += len[r];
    }
    return 0;
}

// What a gather launch is handed (range::Args, nlzm_range.h): the pieces that are not empty, as Piece{ src, dst, len } with the offsets
// taken from `scratch` and `dst`, and chunk0 -- piece p owns chunks [chunk0[p], chunk0[p + 1]) of `chunk` bytes.  Returns the chunk count.
template <class Piece>
inline unsigned long long pack_pieces(const std::vector<PlanPiece> &pieces, const uint8_t *scratch, uint8_t *dst, unsigned long long chunk, std::vector<Piece> &out,
                                      std::vector<unsigned long long> &chunk0)
{
    out.clear(); chunk0.clear();
    unsigned long long nchunks = 0;
    for (const PlanPiece &p : pieces) {
        if (!p.len) continue;
        out.push_back(Piece{ scratch + p.scratch_off, dst + p.dst_off, p.len });
        chunk0.push_back(nchunks);
        nchunks += units::count(p.len, chunk);
    }
    chunk0.push_back(nchunks);
    return nchunks;
}

}  // namespace range

namespace crc {

// What a CRC launch is handed (crc::Args, nlzm_crc.h): one array of 3 (nranges + 1) words -- off, len and seg0 of every range and a
// terminating entry --, range r owning segments [seg0[r], seg0[r + 1]) of `segment` bytes.
struct SegTable {
    std::vector<unsigned long long> words;
    uint32_t nranges = 0;
    unsigned long long nsegs = 0, bytes = 0;
    // a's off / len / seg0 are this table at `base` (the host's copy, or one in device memory)
    template <class Args> void point(Args &a, const unsigned long long *base) const
    {
        a.off = base; a.len = a.off + nranges + 1; a.seg0 = a.len + nranges + 1;
        a.nranges = nranges; a.nsegs = nsegs;
    }

    int make(uint64_t buf_len, uint32_t n, const uint64_t *range_off, const uint64_t *range_len, unsigned long long segment, ErrText err)
    {
        nranges = n; nsegs = 0; bytes = 0;
        words.assign(3 * ((size_t)n + 1), 0);
        unsigned long long *h_off = words.data(), *h_len = h_off + n + 1, *h_seg0 = h_len + n + 1;
        for (uint32_t i = 0; i < n; i++) {
            if (const int rc = check_in_buffer(i, range_off[i], range_len[i], buf_len, err)) return rc;
            h_off[i] = range_off[i]; h_len[i] = range_len[i]; h_seg0[i] = nsegs;
            nsegs += units::count(range_len[i], segment);
            bytes += range_len[i];
            if (nsegs > (1ull << 31)) return plan_error(err, NLZM_HIP_E_ARG, "the ranges of one call may hold 2^31 segments of %llu bytes in all", segment);
        }
        h_seg0[n] = nsegs;
        return 0;
    }
};

}  // namespace crc
}  // namespace nlzm
