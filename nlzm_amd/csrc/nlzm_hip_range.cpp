// nlzm_hip_range.cpp -- host side of the range reader: the nlzm_hip_read_ranges* entry points of include/nlzm_hip.h.  The plan is made
// here, on the host; the device runs ONE decode launch (nlzm_decode.hip, the role's prefix mode: nlzm_decode.h) for all blocks a call
// needs and ONE gather launch (nlzm_range.hip, nlzm_range.h) for all pieces that leave the scratch buffer.  Uses the decoder's and the
// CRC's host side (nlzm_hip_decode.cpp, nlzm_hip_crc.cpp) and nothing of the compress pipeline.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_decode.h"
#include "nlzm_host_decode.h"
#include "nlzm_range.h"

namespace nlzm {
// nlzm_hip.cpp
int host_error(int code, const char *text);
int host_stream(hipStream_t *st);
// nlzm_hip_decode.cpp
void decode_begin_call();
double decode_call_ms();
unsigned long long decode_budget_for(uint64_t stream_len);
int decode_run_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res);
int decode_split(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len);
// nlzm_hip_crc.cpp
void crc_begin_call();
int crc_ranges_on(hipStream_t st, const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t seed, uint32_t *crc_out);
// nlzm_range.hip
void launch_gather(const range::Args &a, uint32_t max_blocks, hipStream_t st);
}  // namespace nlzm

using namespace nlzm;

namespace {

int fail(int code, const char *fmt, ...)
{
    char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return host_error(code, text);
}
#define HIPCHK(expr)                                                                                                        \
    do {                                                                                                                    \
        hipError_t e_ = (expr);                                                                                             \
        if (e_ != hipSuccess)                                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? NLZM_HIP_E_NOMEM : NLZM_HIP_E_NODEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, bytes ? bytes : 16)); return 0; }
    template <class T> T *as() const { return (T *)p; }
};
struct Events {
    hipEvent_t ev[2] = { nullptr, nullptr };
    ~Events() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    int create() { for (auto &e : ev) HIPCHK(hipEventCreate(&e)); return 0; }
};

// what nlzm_hip_get_counter("range_*") reports: the last call, one record per device, as the decoder's
struct Last {
    unsigned long long blocks_decoded = 0, blocks_direct = 0, blocks_checked = 0, decoded_bytes = 0, returned_bytes = 0, scratch_bytes = 0, pieces = 0;
    double decode_us = 0, gather_us = 0;
};
std::mutex g_last_mu;
std::map<int, Last> g_last_of;
Last &last_of_device()
{
    int device = -1;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> lk(g_last_mu);
    return g_last_of[device];
}

constexpr uint64_t kNone = ~0ull;

// The plan of a call, from the blocks' raw lengths and the ranges alone (no device, no pointer):
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
};

int make_plan(Plan &P, uint32_t nblocks, const uint64_t *raw, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint64_t dst_cap)
{
    P.start.assign((size_t)nblocks + 1, 0);
    for (uint32_t b = 0; b < nblocks; b++) {
        if (raw[b] > ~0ull - P.start[b]) return fail(NLZM_HIP_E_ARG, "the blocks' raw lengths do not sum in 64 bits");
        P.start[b + 1] = P.start[b] + raw[b];
    }
    P.total = P.start[nblocks];
    P.need.assign(nblocks, 0); P.place.assign(nblocks, kNone); P.direct.assign(nblocks, 0); P.users.assign(nblocks, 0);
    P.dst_len = 0;
    for (uint32_t r = 0; r < nranges; r++) {
        if (off[r] > P.total || len[r] > P.total - off[r])       // (no off + len: it can wrap)
            return fail(NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes the container holds", r, (unsigned long long)off[r],
                        (unsigned long long)len[r], (unsigned long long)P.total);
        if (len[r] > ~0ull - P.dst_len) return fail(NLZM_HIP_E_ARG, "the ranges' lengths do not sum in 64 bits");
        P.dst_len += len[r];
    }
    if (P.dst_len > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the ranges hold %llu bytes, dst_cap %llu", (unsigned long long)P.dst_len, (unsigned long long)dst_cap);
    // the first block of a non-empty range: the last b with start[b] <= off.  Blocks of raw length 0 share their start with the block behind
    // them, so "the last" is never one of them (off < total: some block behind holds the byte)
    auto first_block = [&](uint64_t o) { return (uint32_t)(std::upper_bound(P.start.begin(), P.start.begin() + nblocks, o) - P.start.begin()) - 1; };
    uint64_t at = 0;
    for (uint32_t r = 0; r < nranges; r++) {
        const uint64_t lo = off[r], hi = off[r] + len[r];           // (checked above: does not wrap)
        for (uint32_t b = len[r] ? first_block(lo) : nblocks; b < nblocks && P.start[b] < hi; b++) {
            if (P.start[b + 1] == P.start[b]) continue;              // a block of raw length 0 is never needed
            const uint64_t end = (hi < P.start[b + 1] ? hi : P.start[b + 1]) - P.start[b];
            if (end > P.need[b]) P.need[b] = end;
            if (!P.users[b]++ && lo <= P.start[b]) { P.direct[b] = 1; P.place[b] = at + (P.start[b] - lo); }
            else P.direct[b] = 0;
        }
        at += len[r];
    }
    P.scratch = 0;
    for (uint32_t b = 0; b < nblocks; b++)
        if (P.need[b] && !P.direct[b]) { P.place[b] = P.scratch; P.scratch += P.need[b]; }      // (sums of parts of the blocks: below total)
    at = 0;
    for (uint32_t r = 0; r < nranges; r++) {
        const uint64_t lo = off[r], hi = off[r] + len[r];
        for (uint32_t b = len[r] ? first_block(lo) : nblocks; b < nblocks && P.start[b] < hi; b++) {
            if (P.start[b + 1] == P.start[b] || P.direct[b]) continue;
            const uint64_t from = lo > P.start[b] ? lo : P.start[b], to = hi < P.start[b + 1] ? hi : P.start[b + 1];
            P.pieces.push_back(PlanPiece{ P.place[b] + (from - P.start[b]), at + (from - lo), to - from });
        }
        at += len[r];
    }
    return 0;
}

// The plan carried out: stream_of[b] is block b's stream in device memory (needed blocks only), blen[b] its length.
int execute(hipStream_t st, const Plan &P, uint32_t nblocks, const std::vector<const uint8_t *> &stream_of, const uint64_t *blen, const uint64_t *raw,
            const uint32_t *crc, uint8_t *d_dst, uint32_t *first_bad)
{
    Last &L = last_of_device();
    DevBuf scratch;
    if (P.scratch) {
        if (hipMalloc(&scratch.p, P.scratch) != hipSuccess) {
            (void)hipGetLastError(); scratch.p = nullptr;
            return fail(NLZM_HIP_E_NOMEM, "no %llu bytes of device memory for the blocks that are read in part", (unsigned long long)P.scratch);
        }
    }
    std::vector<dec::StreamArgs> args;
    std::vector<uint32_t> block_of;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (!P.need[b]) continue;
        uint8_t *to = (P.direct[b] ? d_dst : scratch.as<uint8_t>()) + P.place[b];
        dec::StreamArgs a{ stream_of[b], blen[b], to, P.need[b], decode_budget_for(blen[b]) };
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
    size_t np = 0;
    for (const PlanPiece &p : P.pieces) np += p.len != 0;
    if (np) {
        std::vector<range::Piece> hp(np);
        std::vector<unsigned long long> c0(np + 1);
        unsigned long long nchunks = 0;
        size_t k = 0;
        for (const PlanPiece &p : P.pieces) {
            if (!p.len) continue;
            hp[k] = range::Piece{ scratch.as<uint8_t>() + p.scratch_off, d_dst + p.dst_off, p.len };
            c0[k++] = nchunks;
            nchunks += (p.len + range::kChunk - 1) / range::kChunk;
        }
        c0[np] = nchunks;
        if (np > 0xFFFFFFFFull) return fail(NLZM_HIP_E_ARG, "more than 2^32 pieces in one call");
        DevBuf dp, dc;
        int rc = dp.alloc(np * sizeof(range::Piece));
        if (!rc) rc = dc.alloc((np + 1) * sizeof(unsigned long long));
        if (rc) return rc;
        Events E;
        if ((rc = E.create())) return rc;
        range::Args a{ dp.as<range::Piece>(), dc.as<unsigned long long>(), (uint32_t)np, nchunks };
        hipError_t e = hipMemcpyAsync(dp.p, hp.data(), np * sizeof(range::Piece), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dc.p, c0.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(E.ev[0], st);
        if (e == hipSuccess) { launch_gather(a, 1u << 20, st); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipEventRecord(E.ev[1], st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        else (void)hipStreamSynchronize(st);        // (nothing queued before the failure may outlive `hp` and `c0`)
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, E.ev[0], E.ev[1]);
        if (e != hipSuccess) return fail(NLZM_HIP_E_NODEVICE, "gather launch failed: %s", hipGetErrorString(e));
        L.gather_us += 1000.0 * ms;
    }
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

void begin_call()
{
    decode_begin_call();
    crc_begin_call();
    last_of_device() = Last{};
}

int check_args(const void *src, uint32_t nblocks, uint32_t nranges, const uint64_t *off, const uint64_t *len, const void *dst, const uint64_t *dst_len,
               const uint32_t *crc, const uint32_t *first_bad)
{
    if (!src || !dst_len || !nblocks || nblocks > 65536 || (nranges && (!off || !len)) || (crc && !first_bad))
        return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    (void)dst;
    return 0;
}

}  // namespace

namespace nlzm {
int range_counter(const char *key, uint64_t *value)
{
    const Last &L = last_of_device();
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
    if (const int rc = host_stream(&st)) return rc;
    if (const int rc = check_args(d_src, nblocks, nranges, off, len, d_dst, dst_len, crc, first_bad)) return rc;
    begin_call();
    *dst_len = 0;
    if (first_bad) *first_bad = nblocks;
    if (!nranges) return 0;
    std::vector<uint64_t> boff, blen, raw(nblocks);
    int rc = decode_split(st, d_src, src_len, nblocks, block_len, boff, blen);
    if (rc) return rc;
    if (raw_len) memcpy(raw.data(), raw_len, nblocks * sizeof(uint64_t));
    else {                                          // a size pass of all blocks
        std::vector<dec::StreamArgs> args(nblocks);
        for (uint32_t b = 0; b < nblocks; b++) args[b] = dec::StreamArgs{ (const uint8_t *)d_src + boff[b], blen[b], nullptr, ~0ull, decode_budget_for(blen[b]) };
        std::vector<dec::StreamResult> res;
        if ((rc = decode_run_streams(st, args, res))) return rc;
        for (uint32_t b = 0; b < nblocks; b++) raw[b] = res[b].out_len;
    }
    Plan P;
    if ((rc = make_plan(P, nblocks, raw.data(), nranges, off, len, dst_cap))) return rc;
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
    if (const int rc = host_stream(&st)) return rc;
    if (const int rc = check_args(src, nblocks, nranges, off, len, dst, dst_len, crc, first_bad)) return rc;
    begin_call();
    *dst_len = 0;
    if (first_bad) *first_bad = nblocks;
    if (!nranges) return 0;
    // the blocks' boundaries on the host (the hop the command line makes), their raw lengths given or by a size pass of the whole container
    std::vector<uint64_t> boff(nblocks), blen(nblocks), raw(nblocks);
    uint64_t at = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (block_len) {
            if (block_len[b] > src_len - at) return fail(NLZM_HIP_E_ARG, "block %u's length %llu runs over the %llu bytes given", b + 1, (unsigned long long)block_len[b], (unsigned long long)src_len);
            blen[b] = block_len[b];
        } else {
            const size_t l = nlzm_host::stream_length(nlzm_host::Span{ src + at, (size_t)(src_len - at) });
            if (!l) return fail(NLZM_HIP_E_FORMAT, "block %u of %u is not an NLZM stream, or is cut off (found by the frame headers)", b + 1, nblocks);
            blen[b] = l;
        }
        boff[b] = at; at += blen[b];
    }
    DevBuf ds, dd;
    int rc = 0;
    std::vector<const uint8_t *> stream_of(nblocks, nullptr);
    if (raw_len) memcpy(raw.data(), raw_len, nblocks * sizeof(uint64_t));
    else {
        if ((rc = ds.alloc(at))) return rc;
        HIPCHK(hipMemcpyAsync(ds.p, src, at, hipMemcpyHostToDevice, st));
        std::vector<dec::StreamArgs> args(nblocks);
        for (uint32_t b = 0; b < nblocks; b++) {
            stream_of[b] = ds.as<uint8_t>() + boff[b];
            args[b] = dec::StreamArgs{ stream_of[b], blen[b], nullptr, ~0ull, decode_budget_for(blen[b]) };
        }
        std::vector<dec::StreamResult> res;
        if ((rc = decode_run_streams(st, args, res))) return rc;
        for (uint32_t b = 0; b < nblocks; b++) raw[b] = res[b].out_len;
    }
    Plan P;
    if ((rc = make_plan(P, nblocks, raw.data(), nranges, off, len, dst_cap))) return rc;
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
