// nlzm_hip_range.cpp -- host side of the range reader: the nlzm_hip_read_ranges* entry points of include/nlzm_hip.h.  The plan is made
// here, on the host; the device runs ONE decode launch (nlzm_decode.hip, the role's prefix mode: nlzm_decode.h) for all blocks a call
// needs and ONE gather launch (nlzm_range.hip, nlzm_range.h) for all pieces that leave the scratch buffer.  Uses the decoder's and the
// CRC's host side (nlzm_hip_decode.cpp, nlzm_hip_crc.cpp) and nothing of the compress pipeline.
#include <stdint.h>
#include <string.h>

#include "nlzm_host_util.h"
#include "nlzm_decode.h"
#include "nlzm_range.h"
#include "nlzm_read_plan.h"

using namespace nlzm;
using range::Plan;

namespace {

// what nlzm_hip_get_counter("range_*") reports of the last call
struct Last {
    unsigned long long blocks_decoded = 0, blocks_direct = 0, blocks_checked = 0, decoded_bytes = 0, returned_bytes = 0, scratch_bytes = 0, pieces = 0;
    double decode_us = 0, gather_us = 0;
};
PerDevice<Last> g_last;

// the plan (nlzm_read_plan.h), its error the library's
int plan_of(Plan &P, uint32_t nblocks, const uint64_t *raw, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint64_t dst_cap)
{
    char why[512];
    const int rc = range::make_plan(P, nblocks, raw, nranges, off, len, dst_cap, ErrText{ why, sizeof why });
    return rc ? fail(rc, "%s", why) : 0;
}

// The plan carried out: stream_of[b] is block b's stream in device memory (needed blocks only), blen[b] its length.
int execute(hipStream_t st, const Plan &P, uint32_t nblocks, const std::vector<const uint8_t *> &stream_of, const uint64_t *blen, const uint64_t *raw,
            const uint32_t *crc, uint8_t *d_dst, uint32_t *first_bad)
{
    Last &L = g_last.here();
    DevBuf scratch;
    if (P.scratch) if (const int rc = scratch.alloc_for(P.scratch, "the blocks that are read in part")) return rc;
    std::vector<dec::StreamArgs> args;
    std::vector<uint32_t> block_of;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (!P.need[b]) continue;
        uint8_t *to = (P.direct[b] ? d_dst : scratch.as<uint8_t>()) + P.place[b];
        dec::StreamArgs a = decode_stream_args(stream_of[b], blen[b], to, P.need[b]);
        a.flags = P.need[b] < raw[b] ? dec::kPrefix : 0u;           // read in full: the decoder's own bound, and its verdict on a longer stream
        args.push_back(a);
        block_of.push_back(b);
        L.blocks_decoded++;
        L.blocks_direct += P.direct[b];
        L.decoded_bytes += P.need[b];
    }
    L.scratch_bytes = P.scratch;
    L.pieces = P.pieces.size();
    L.returned_bytes = P.dst_len;
    if (!args.empty()) {
        std::vector<dec::StreamResult> res;
        const double ms0 = decode_call_ms();
        const int rc = decode_run_streams(st, args, res);
        L.decode_us += 1000.0 * (decode_call_ms() - ms0);
        if (rc) return rc;
        for (size_t i = 0; i < args.size(); i++)
            if (res[i].out_len != args[i].cap)
                return fail(NLZM_HIP_E_FORMAT, "block %u decodes to %llu bytes, not the %llu it was said to hold", block_of[i] + 1, res[i].out_len, (unsigned long long)raw[block_of[i]]);
    }
    // the gather launch: every piece that lies in the scratch buffer, on the same stream behind the decode
    std::vector<range::Piece> hp;
    std::vector<unsigned long long> c0;
    range::pack_pieces(P.pieces, scratch.as<uint8_t>(), d_dst, range::kChunk, hp, c0);     // (c0: gather_on makes its own, from the same units::count)
    if (const int rc = gather_on(st, "gather", hp, &L.gather_us)) return rc;
    if (first_bad) *first_bad = nblocks;
    if (crc) {
        // the blocks this call decoded in full, hashed where they lie: in the destination (direct) or in the scratch buffer
        uint32_t bad = nblocks;
        for (int where = 0; where < 2; where++) {
            std::vector<uint64_t> o, l;
            std::vector<uint32_t> which;
            for (uint32_t b = 0; b < nblocks; b++)
                if (P.need[b] && P.need[b] == raw[b] && (P.direct[b] != 0) == (where == 0)) { o.push_back(P.place[b]); l.push_back(raw[b]); which.push_back(b); }
            if (which.empty()) continue;
            std::vector<uint32_t> got(which.size());
            const int rc = crc_ranges_on(st, where == 0 ? (const void *)d_dst : scratch.p, where == 0 ? P.dst_len : P.scratch, (uint32_t)which.size(), o.data(), l.data(), 0, got.data());
            if (rc) return rc;
            for (size_t i = 0; i < which.size(); i++) if (got[i] != crc[which[i]] && which[i] < bad) bad = which[i];
            L.blocks_checked += which.size();
        }
        if (first_bad) *first_bad = bad;
    }
    return 0;
}

// what both entry points begin with: the library's stream, the arguments checked, a fresh record, the outputs of a call that reads nothing
int enter(hipStream_t *st, const void *src, uint32_t nblocks, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint64_t *dst_len, const uint32_t *crc,
          uint32_t *first_bad)
{
    if (const int rc = host_stream(st)) return rc;
    if (!src || !dst_len || !nblocks || nblocks > 65536 || (nranges && (!off || !len)) || (crc && !first_bad))
        return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    decode_begin_call();
    crc_begin_call();
    g_last.here() = Last{};
    *dst_len = 0;
    if (first_bad) *first_bad = nblocks;
    return 0;
}

}  // namespace

namespace nlzm {

int gather_on(hipStream_t st, const char *what, const std::vector<range::Piece> &pieces, double *us)
{
    const size_t np = pieces.size();
    if (!np) return 0;
    if (np > 0xFFFFFFFFull) return fail(NLZM_HIP_E_ARG, "more than 2^32 pieces in one call");
    const std::vector<unsigned long long> c0 = units::prefix((uint32_t)np, range::kChunk, [&](uint32_t p) { return pieces[p].len; });
    DevBuf dp, dc;
    int rc = dp.alloc(np * sizeof(range::Piece));
    if (!rc) rc = dc.alloc((np + 1) * sizeof(unsigned long long));
    if (rc) return rc;
    const range::Args a{ dp.as<range::Piece>(), dc.as<unsigned long long>(), (uint32_t)np, c0[np] };
    float ms = 0;
    rc = timed_launch(st, what, &ms,
        [&] {
            const hipError_t e = hipMemcpyAsync(dp.p, pieces.data(), np * sizeof(range::Piece), hipMemcpyHostToDevice, st);
            return e != hipSuccess ? e : hipMemcpyAsync(dc.p, c0.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
        },
        [&] { launch_gather(a, kStrideBlocks, st); },
        [] { return hipSuccess; });
    if (rc) return rc;
    *us += 1000.0 * ms;
    return 0;
}

int range_counter(const char *key, uint64_t *value)
{
    const Last &L = g_last.here();
    static const struct { const char *name; unsigned long long Last::*m; } kInt[] = {
        { "range_blocks_decoded", &Last::blocks_decoded }, { "range_blocks_direct", &Last::blocks_direct }, { "range_blocks_checked", &Last::blocks_checked },
        { "range_decoded_bytes", &Last::decoded_bytes }, { "range_returned_bytes", &Last::returned_bytes }, { "range_scratch_bytes", &Last::scratch_bytes },
        { "range_pieces", &Last::pieces },
    };
    for (const auto &e : kInt) if (!strcmp(key, e.name)) { *value = L.*(e.m); return 0; }
    if (!strcmp(key, "range_us")) { *value = (uint64_t)(L.decode_us + L.gather_us + 0.5); return 0; }
    if (!strcmp(key, "range_decode_us")) { *value = (uint64_t)(L.decode_us + 0.5); return 0; }
    if (!strcmp(key, "range_gather_us")) { *value = (uint64_t)(L.gather_us + 0.5); return 0; }
    if (!strcmp(key, "range_chunk_bytes")) { *value = range::kChunk; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

}  // namespace nlzm

extern "C" {

int nlzm_hip_read_ranges_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len, const uint32_t *crc,
                             uint32_t nranges, const uint64_t *off, const uint64_t *len, void *d_dst, uint64_t dst_cap, uint64_t *dst_len, uint32_t *first_bad)
{
    hipStream_t st;
    if (const int rc = enter(&st, d_src, nblocks, nranges, off, len, dst_len, crc, first_bad)) return rc;
    if (!nranges) return 0;
    std::vector<uint64_t> boff, blen, raw;
    int rc = decode_split(st, d_src, src_len, nblocks, block_len, boff, blen);
    if (rc) return rc;
    if (raw_len) raw.assign(raw_len, raw_len + nblocks);
    else if ((rc = decode_sizes(st, (const uint8_t *)d_src, boff, blen, raw))) return rc;      // a size pass of all blocks
    Plan P;
    if ((rc = plan_of(P, nblocks, raw.data(), nranges, off, len, dst_cap))) return rc;
    if (P.dst_len && !d_dst) return fail(NLZM_HIP_E_ARG, "null argument");
    std::vector<const uint8_t *> stream_of(nblocks);
    for (uint32_t b = 0; b < nblocks; b++) stream_of[b] = (const uint8_t *)d_src + boff[b];
    rc = execute(st, P, nblocks, stream_of, blen.data(), raw.data(), crc, (uint8_t *)d_dst, first_bad);
    if (rc) return rc;
    *dst_len = P.dst_len;
    return 0;
}

int nlzm_hip_read_ranges(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len, const uint32_t *crc,
                         uint32_t nranges, const uint64_t *off, const uint64_t *len, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_len, uint32_t *first_bad)
{
    hipStream_t st;
    if (const int rc = enter(&st, src, nblocks, nranges, off, len, dst_len, crc, first_bad)) return rc;
    if (!nranges) return 0;
    // the blocks' boundaries on the host (the hop the command line makes), their raw lengths given or by a size pass of the whole container
    std::vector<uint64_t> boff, blen, raw;
    int rc = decode_split_host(src, src_len, nblocks, block_len, boff, blen);
    if (rc) return rc;
    DevBuf ds, dd;
    std::vector<const uint8_t *> stream_of(nblocks, nullptr);
    if (raw_len) raw.assign(raw_len, raw_len + nblocks);
    else {
        const uint64_t bytes = boff.back() + blen.back();
        if ((rc = ds.alloc(bytes))) return rc;
        HIPCHK(hipMemcpyAsync(ds.p, src, bytes, hipMemcpyHostToDevice, st));
        for (uint32_t b = 0; b < nblocks; b++) stream_of[b] = ds.as<uint8_t>() + boff[b];
        if ((rc = decode_sizes(st, ds.as<uint8_t>(), boff, blen, raw))) return rc;
    }
    Plan P;
    if ((rc = plan_of(P, nblocks, raw.data(), nranges, off, len, dst_cap))) return rc;
    if (P.dst_len && !dst) return fail(NLZM_HIP_E_ARG, "null argument");
    if (!ds.p) {                                    // only the needed blocks' streams are uploaded, packed back to back
        uint64_t bytes = 0;
        for (uint32_t b = 0; b < nblocks; b++) if (P.need[b]) bytes += blen[b];
        if ((rc = ds.alloc(bytes))) return rc;
        uint64_t to = 0;
        for (uint32_t b = 0; b < nblocks; b++) {
            if (!P.need[b]) continue;
            stream_of[b] = ds.as<uint8_t>() + to;
            HIPCHK(hipMemcpyAsync(ds.as<uint8_t>() + to, src + boff[b], blen[b], hipMemcpyHostToDevice, st));
            to += blen[b];
        }
    }
    if ((rc = dd.alloc(P.dst_len))) return rc;
    rc = execute(st, P, nblocks, stream_of, blen.data(), raw.data(), crc, dd.as<uint8_t>(), first_bad);
    if (rc) return rc;
    if (P.dst_len) HIPCHK(hipMemcpyAsync(dst, dd.p, P.dst_len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *dst_len = P.dst_len;
    return 0;
}

}  // extern "C"
