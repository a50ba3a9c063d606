// nlzm_hip_decode.cpp -- host side of the device decoder: the nlzm_hip_decompress* / nlzm_hip_verify_dev entry points of
// include/nlzm_hip.h.  Kernels: nlzm_decode.hip; the role they run: nlzm_decode.h.  Uses the library's device, stream and error text
// (nlzm_hip.cpp, through nlzm_host_util.h) and nothing else of the compress pipeline.
#include <stdint.h>
#include <string.h>

#include "nlzm_host_util.h"
#include "nlzm_decode.h"
#include "nlzm_host_decode.h"
#include "nlzm_read_plan.h"

using namespace nlzm;

namespace {

// what nlzm_hip_get_counter("decode_*") reports: the streams of the last storing pass (of the last size pass, if the call made no other)
struct Last {
    dec::StreamResult sum{};
    unsigned long long max_cycles = 0, max_stream = 0, streams = 0, passes = 0;
    double ms = 0;                                  // device time of all passes of the last call
    unsigned long long steps = 0;                   // launches of the open (or last) decode set
    double step_ms = 0;                             // device time of its last step
    unsigned long long ring = 0;                    // LDS ring of the kernel the last decode launch ran
};
PerDevice<Last> g_last;

// the blocks' offsets from their lengths as the caller gives them, which may not run over the src_len bytes there are
int given_split(uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    off.assign(nblocks, 0); len.assign(nblocks, 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        if (block_len[i] > src_len - at) return fail(NLZM_HIP_E_ARG, "block %u's length %llu runs over the %llu bytes given", i + 1, (unsigned long long)block_len[i], (unsigned long long)src_len);
        off[i] = at; len[i] = block_len[i]; at += block_len[i];
    }
    return 0;
}
int bad_block(uint32_t i, uint32_t nblocks) { return fail(NLZM_HIP_E_FORMAT, "block %u of %u is not an NLZM stream, or is cut off (found by the frame headers)", i, nblocks); }

}  // namespace

namespace nlzm {

void decode_begin_call() { Last &L = g_last.here(); L.ms = 0; L.passes = 0; }
double decode_call_ms() { return g_last.here().ms; }

// The budget is a minute and a second per megabyte of stream, in clock100() ticks: a lone wave decodes tens of megabytes of output a second,
// so this is an order of magnitude above any well-formed stream and still ends a decode that has gone wrong.
dec::StreamArgs decode_stream_args(const uint8_t *d_stream, uint64_t len, uint8_t *d_dst, uint64_t cap)
{
    return dec::StreamArgs{ d_stream, len, d_dst, cap, (60ull + len / 1000000ull) * 100000000ull };
}

// Which one-shot kernel a launch of k streams runs (option "decode_ring"): the 64 KiB ring fits a CU's LDS twice, so 2 x CUs streams are at work
// at once and each wave has its SIMD to itself; with more streams than that the small ring's workgroups -- several to a SIMD, which hides the
// lone wave's issue latency -- take over.  Up to 2 x CUs streams every launch is the kernel it has always been.
static bool small_ring_for(size_t k)
{
    int64_t opt = 0; int cus = 0;
    host_decode_setup(&opt, &cus);
    return opt ? opt != (int64_t)dec::kRing : k > 2 * (size_t)cus;
}

// one timed launch of the streams in `args`, by a one-shot kernel or by the stepping one; the call's device time and pass count go on
static int launch_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res, bool steps, float *ms)
{
    const size_t k = args.size();
    const bool small = !steps && small_ring_for(k);
    DevBuf da, dr;
    int rc = da.alloc(k * sizeof(dec::StreamArgs));
    if (!rc) rc = dr.alloc(k * sizeof(dec::StreamResult));
    if (rc) return rc;
    res.assign(k, dec::StreamResult{});
    rc = timed_launch(st, steps ? "decode step" : "decode", ms,
        [&] {
            const hipError_t e = hipMemcpyAsync(da.p, args.data(), k * sizeof(dec::StreamArgs), hipMemcpyHostToDevice, st);
            return e != hipSuccess ? e : hipMemsetAsync(dr.p, 0xFF, k * sizeof(dec::StreamResult), st);        // (a workgroup that never ran reports rc = -1)
        },
        [&] { if (steps) launch_decode_steps(da.p, dr.p, (uint32_t)k, st); else if (small) launch_decode_small(da.p, dr.p, (uint32_t)k, st); else launch_decode(da.p, dr.p, (uint32_t)k, st); },
        [&] { return hipMemcpyAsync(res.data(), dr.p, k * sizeof(dec::StreamResult), hipMemcpyDeviceToHost, st); });
    if (rc) return rc;
    Last &L = g_last.here();
    L.ms += *ms;
    L.passes++;
    L.ring = small ? decode_small_ring() : dec::kRing;
    return 0;
}

// one launch of the streams in `args` (a destination pointer, a bound and the flags per stream); res: what each reported
int decode_run_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res)
{
    const size_t k = args.size();
    float ms = 0;
    if (const int rc = launch_streams(st, args, res, false, &ms)) return rc;
    Last &L = g_last.here();
    L.sum = dec::StreamResult{};
    L.max_cycles = 0; L.max_stream = 0;
    L.streams = k;
    for (size_t i = 0; i < k; i++) {
        const dec::StreamResult &r = res[i];
        L.sum.syms += r.syms; L.sum.raw_ops += r.raw_ops; L.sum.n_literal += r.n_literal; L.sum.n_dict += r.n_dict; L.sum.n_rep += r.n_rep;
        L.sum.ring_bytes += r.ring_bytes; L.sum.global_bytes += r.global_bytes; L.sum.out_len += r.out_len;
        L.sum.cycles += r.cycles; L.sum.window_cycles += r.window_cycles; L.sum.copy_cycles += r.copy_cycles;
        if (r.cycles > L.max_cycles) { L.max_cycles = r.cycles; L.max_stream = i; }
    }
    for (size_t i = 0; i < k; i++) {
        const dec::StreamResult &r = res[i];
        if (r.rc == dec::kErrFormat)
            return fail(NLZM_HIP_E_FORMAT, "stream %zu of %zu is not a well-formed NLZM stream (check %u failed after %llu output bytes)", i + 1, k, r.detail, r.out_len);
        if (r.rc == dec::kErrCapacity)
            return fail(NLZM_HIP_E_CAPACITY, "stream %zu of %zu decodes to more than the %llu bytes there is room for", i + 1, k, (unsigned long long)args[i].cap);
        if (r.rc) return fail(NLZM_HIP_E_KERNEL, "decode kernel: stream %zu of %zu ended with code %d after %llu output bytes", i + 1, k, r.rc, r.out_len);
    }
    return 0;
}

// THE size pass: the streams [d_src + off[i], + len[i]) decoded with no destination; raw: how many bytes each holds
int decode_sizes(hipStream_t st, const uint8_t *d_src, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, std::vector<uint64_t> &raw)
{
    const size_t k = off.size();
    std::vector<dec::StreamArgs> args(k);
    for (size_t i = 0; i < k; i++) args[i] = decode_stream_args(d_src + off[i], len[i], nullptr, ~0ull);
    std::vector<dec::StreamResult> res;
    if (const int rc = decode_run_streams(st, args, res)) return rc;
    raw.resize(k);
    for (size_t i = 0; i < k; i++) raw[i] = res[i].out_len;
    return 0;
}

// the block streams' offsets and lengths: given, or found by hopping over their frame headers on the device ...
int decode_split(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    if (block_len) return given_split(src_len, nblocks, block_len, off, len);
    off.assign(nblocks, 0); len.assign(nblocks, 0);
    DevBuf dl, db;
    int rc = dl.alloc(nblocks * sizeof(uint64_t));
    if (!rc) rc = db.alloc(sizeof(uint32_t));
    if (rc) return rc;
    uint32_t bad = 0;
    launch_split(d_src, src_len, nblocks, dl.as<unsigned long long>(), db.as<uint32_t>(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(len.data(), dl.p, nblocks * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bad, db.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return bad_block(bad, nblocks);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nblocks; i++) { off[i] = at; at += len[i]; }
    return 0;
}
// ... and of a container in host memory: the same hop on the host (the one the command line makes)
int decode_split_host(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    if (block_len) return given_split(src_len, nblocks, block_len, off, len);
    const size_t found = nlzm_host::split_streams(nlzm_host::Span{ src, (size_t)src_len }, nblocks, len);
    if (found < nblocks) return bad_block((uint32_t)found + 1, nblocks);
    off.assign(nblocks, 0);
    for (uint32_t i = 1; i < nblocks; i++) off[i] = off[i - 1] + len[i - 1];
    return 0;
}

int decode_counter(const char *key, uint64_t *value)
{
    const Last &L = g_last.here();
    static const struct { const char *name; unsigned long long dec::StreamResult::*m; } kSum[] = {
        { "decode_syms", &dec::StreamResult::syms }, { "decode_raw_ops", &dec::StreamResult::raw_ops }, { "decode_n_literal", &dec::StreamResult::n_literal },
        { "decode_n_dict", &dec::StreamResult::n_dict }, { "decode_n_rep", &dec::StreamResult::n_rep }, { "decode_ring_bytes", &dec::StreamResult::ring_bytes },
        { "decode_global_bytes", &dec::StreamResult::global_bytes }, { "decode_out_bytes", &dec::StreamResult::out_len }, { "decode_cycles", &dec::StreamResult::cycles },
        { "decode_window_cycles", &dec::StreamResult::window_cycles }, { "decode_copy_cycles", &dec::StreamResult::copy_cycles },
    };
    for (const auto &e : kSum) if (!strcmp(key, e.name)) { *value = L.sum.*(e.m); return 0; }
    if (!strcmp(key, "decode_max_stream_cycles")) { *value = L.max_cycles; return 0; }
    if (!strcmp(key, "decode_slowest_stream")) { *value = L.max_stream; return 0; }
    if (!strcmp(key, "decode_streams")) { *value = L.streams; return 0; }
    if (!strcmp(key, "decode_passes")) { *value = L.passes; return 0; }
    if (!strcmp(key, "decode_ms")) { *value = (uint64_t)(L.ms + 0.5); return 0; }
    if (!strcmp(key, "decode_us")) { *value = (uint64_t)(L.ms * 1000.0 + 0.5); return 0; }
    if (!strcmp(key, "decode_steps")) { *value = L.steps; return 0; }
    if (!strcmp(key, "decode_step_us")) { *value = (uint64_t)(L.step_ms * 1000.0 + 0.5); return 0; }
    if (!strcmp(key, "decode_ring_size")) { *value = L.ring; return 0; }
    if (!strcmp(key, "decode_state_bytes")) { *value = dec::kStateBytes; return 0; }      // (needs no device)
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

}  // namespace nlzm

namespace {

// The blocks of a container in device memory, sized (raw_len_in == nullptr: a size pass) and, with a destination, decoded into it back to back
int blocks_dev(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in, void *d_dst,
               uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    std::vector<uint64_t> off, len, raw;
    int rc = decode_split(st, d_src, src_len, nblocks, block_len, off, len);
    if (rc) return rc;
    if (raw_len_in) raw.assign(raw_len_in, raw_len_in + nblocks);
    else if ((rc = decode_sizes(st, (const uint8_t *)d_src, off, len, raw))) return rc;
    uint64_t total = 0;
    for (uint32_t i = 0; i < nblocks; i++) total += raw[i];
    if (d_dst) {
        if (total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the blocks decode to %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
        std::vector<dec::StreamArgs> args(nblocks);
        uint64_t at = 0;
        for (uint32_t i = 0; i < nblocks; i++) { args[i] = decode_stream_args((const uint8_t *)d_src + off[i], len[i], (uint8_t *)d_dst + at, raw[i]); at += raw[i]; }
        std::vector<dec::StreamResult> res;
        if ((rc = decode_run_streams(st, args, res))) return rc;
        for (uint32_t i = 0; i < nblocks; i++)
            if (res[i].out_len != raw[i])
                return fail(NLZM_HIP_E_FORMAT, "block %u decodes to %llu bytes, not the %llu it was said to hold", i + 1, res[i].out_len, (unsigned long long)raw[i]);
    }
    if (raw_len_out) for (uint32_t i = 0; i < nblocks; i++) raw_len_out[i] = raw[i];
    if (dst_len) *dst_len = total;
    return 0;
}

// The blocks decoded into a buffer of the call's own, `dd`.  With lengths the caller claims (claimed != nullptr; dd holds their sum, `cap`):
// ONE pass, every block bounded by its length.  A container that does not fit them -- a block decodes to more (E_CAPACITY) or to less
// (E_FORMAT) -- or no claim at all: the blocks are sized, dd is made anew and they are decoded by what they hold.  raw / total: what decoded.
int decode_claimed_or_sized(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *claimed, uint64_t cap,
                            DevBuf &dd, std::vector<uint64_t> &raw, uint64_t *total)
{
    raw.resize(nblocks);
    int rc = NLZM_HIP_E_FORMAT;
    if (claimed) rc = blocks_dev(st, d_src, src_len, nblocks, block_len, claimed, dd.p, cap, raw.data(), total);
    if (rc != NLZM_HIP_E_CAPACITY && rc != NLZM_HIP_E_FORMAT) return rc;
    const double ms = decode_call_ms();             // (the call's device time so far is added once more below: counted as it always was)
    rc = blocks_dev(st, d_src, src_len, nblocks, block_len, nullptr, nullptr, 0, raw.data(), total);       // sizes
    if (rc) return rc;
    if (dd.p) { (void)hipFree(dd.p); dd.p = nullptr; }
    if ((rc = dd.alloc(*total))) return rc;
    rc = blocks_dev(st, d_src, src_len, nblocks, block_len, raw.data(), dd.p, *total, nullptr, total);
    g_last.here().ms += ms;
    return rc;
}

}  // namespace

extern "C" {

int nlzm_hip_decompress_dev(const void *d_stream, uint64_t stream_len, void *d_dst, uint64_t dst_cap, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!d_stream || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    decode_begin_call();
    const std::vector<dec::StreamArgs> args{ decode_stream_args((const uint8_t *)d_stream, stream_len, (uint8_t *)d_dst, d_dst ? dst_cap : ~0ull) };
    std::vector<dec::StreamResult> res;
    if (const int rc = decode_run_streams(st, args, res)) return rc;
    *dst_len = res[0].out_len;
    return 0;
}

int nlzm_hip_decompress(const uint8_t *stream, uint64_t stream_len, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_len)
{
    return nlzm_hip_decompress_blocks(stream, stream_len, 1, &stream_len, nullptr, dst, dst_cap, nullptr, dst_len);
}

int nlzm_hip_decompress_blocks_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in,
                                   void *d_dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!d_src || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    decode_begin_call();
    return blocks_dev(st, d_src, src_len, nblocks, block_len, raw_len_in, d_dst, dst_cap, raw_len_out, dst_len);
}

int nlzm_hip_decompress_blocks(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in,
                               uint8_t *dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!src || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    decode_begin_call();
    // host buffers: the container is split on the host (the same hop the command line makes), sized on the device, decoded into a
    // device buffer of exactly that size and copied back
    std::vector<uint64_t> boff, blen;
    int rc = decode_split_host(src, src_len, nblocks, block_len, boff, blen);
    if (rc) return rc;
    DevBuf ds, dd;
    if ((rc = ds.alloc(src_len))) return rc;
    HIPCHK(hipMemcpyAsync(ds.p, src, src_len, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> raw(nblocks);
    uint64_t total = 0;
    rc = blocks_dev(st, ds.p, src_len, nblocks, blen.data(), raw_len_in, nullptr, 0, raw.data(), &total);
    if (rc) return rc;
    if (dst) {
        if (total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the stream decodes to %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
        rc = dd.alloc(total);
        if (rc) return rc;
        rc = blocks_dev(st, ds.p, src_len, nblocks, blen.data(), raw.data(), dd.p, total, raw.data(), &total);
        if (rc) return rc;
        if (total) HIPCHK(hipMemcpyAsync(dst, dd.p, total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (raw_len_out) memcpy(raw_len_out, raw.data(), nblocks * sizeof(uint64_t));
    if (dst_len) *dst_len = total;
    return 0;
}

int nlzm_hip_verify_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const void *d_orig, uint64_t n,
                        uint64_t *first_mismatch, uint64_t *decoded_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!d_src || (!d_orig && n) || !first_mismatch || !decoded_len || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    decode_begin_call();
    // The blocks of a container made from n bytes hold ceil(n / nblocks) bytes each (the last ones fewer): decoded on that assumption in
    // ONE pass, every block bounded by its share.  A container that does not fit it (some other partition, a wrong length) is sized first.
    std::vector<uint64_t> shares, raw;
    equal_shares(n, nblocks, shares);
    DevBuf dd, df;
    int rc = dd.alloc(n);
    if (!rc) rc = df.alloc(sizeof(unsigned long long));
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = decode_claimed_or_sized(st, d_src, src_len, nblocks, block_len, shares.data(), n, dd, raw, &total))) return rc;
    const uint64_t m = total < n ? total : n;
    unsigned long long first = m;
    HIPCHK(hipMemcpyAsync(df.p, &first, sizeof first, hipMemcpyHostToDevice, st));
    if (m) { launch_compare(dd.p, d_orig, m, df.as<unsigned long long>(), st); HIPCHK(hipGetLastError()); }
    HIPCHK(hipMemcpyAsync(&first, df.p, sizeof first, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // a wrong length: a mismatch at the shorter length, unless the bytes differ before it.  When the stream decodes to MORE than n bytes whose
    // first n agree, that offset is n itself -- the value that also says "equal": the decoded length is what tells the two apart
    *first_mismatch = first;
    *decoded_len = total;
    return 0;
}

int nlzm_hip_verify(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint8_t *orig, uint64_t n,
                    uint64_t *first_mismatch, uint64_t *decoded_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!src || (!orig && n) || !first_mismatch || !decoded_len) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf ds, dorig;
    int rc = ds.alloc(src_len);
    if (!rc) rc = dorig.alloc(n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ds.p, src, src_len, hipMemcpyHostToDevice, st));
    if (n) HIPCHK(hipMemcpyAsync(dorig.p, orig, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return nlzm_hip_verify_dev(ds.p, src_len, nblocks, block_len, dorig.p, n, first_mismatch, decoded_len);
}

int nlzm_hip_check_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                       const uint32_t *crc, uint32_t *first_bad, uint32_t *crc_out)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!d_src || !crc || !first_bad || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    decode_begin_call();
    crc_begin_call();
    // With the lengths the caller holds: ONE decode pass, every block bounded by its length.  A block that decodes to more or to less shows in
    // that pass's error; the blocks are then sized and decoded by what they hold, as without lengths, and the comparison below names the block.
    std::vector<uint64_t> raw, off(nblocks);
    DevBuf dd;
    uint64_t total = 0;
    const uint64_t *claimed = raw_len;
    if (raw_len) {
        bool fits = true;
        for (uint32_t i = 0; i < nblocks; i++) { if (raw_len[i] > ~0ull - total) fits = false; else total += raw_len[i]; }
        if (!fits || hipMalloc(&dd.p, total ? total : 16) != hipSuccess) { (void)hipGetLastError(); dd.p = nullptr; claimed = nullptr; }     // (lengths no buffer can hold are wrong lengths)
    }
    int rc = decode_claimed_or_sized(st, d_src, src_len, nblocks, block_len, claimed, total, dd, raw, &total);
    if (rc) return rc;
    uint64_t at = 0;
    for (uint32_t i = 0; i < nblocks; i++) { off[i] = at; at += raw[i]; }
    std::vector<uint32_t> got(nblocks);
    rc = crc_ranges_on(st, dd.p, total, nblocks, off.data(), raw.data(), 0, got.data());
    if (rc) return rc;
    uint32_t bad = nblocks;
    for (uint32_t i = nblocks; i-- > 0;) if (got[i] != crc[i] || (raw_len && raw[i] != raw_len[i])) bad = i;
    *first_bad = bad;
    if (crc_out) memcpy(crc_out, got.data(), nblocks * sizeof(uint32_t));
    return 0;
}

int nlzm_hip_check(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                   const uint32_t *crc, uint32_t *first_bad, uint32_t *crc_out)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!src || !crc || !first_bad) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf ds;
    const int rc = ds.alloc(src_len);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ds.p, src, src_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return nlzm_hip_check_dev(ds.p, src_len, nblocks, block_len, raw_len, crc, first_bad, crc_out);
}

}  // extern "C"

// ---- decoding in steps: one open decode set per device state (the idiom of nlzm_hip_blocks_begin / _step / _finish / _abandon) ----------------
namespace {

struct StepSet {
    bool open = false, more = false, bounded = false, cut_off = false, extended_flat = false;
    const uint8_t *d_src = nullptr;
    uint8_t *d_dst = nullptr;                       // nullptr: size-only stepping
    void *own_src = nullptr, *own_dst = nullptr;    // the host form's: the uploaded container, the library's output buffer
    dec::StepState *states = nullptr;
    uint32_t nblocks = 0;
    std::vector<uint64_t> off, len, bound, at, done;        // per block: stream offset and length, bound on its output, its offset in the output, bytes decoded
    std::vector<uint8_t> fin, started;
    std::vector<dec::StreamResult> tot;             // every block's running totals (what its last launch reported)
    uint64_t total = 0;                             // bounded: the sum of the blocks' lengths
};
PerDevice<StepSet> g_steps;

void steps_close(StepSet &S)
{
    if (S.states) (void)hipFree(S.states);
    if (S.own_src) (void)hipFree(S.own_src);
    if (S.own_dst) (void)hipFree(S.own_dst);
    S = StepSet{};
}

// binds what begin found: the split, the bounds, one state record per block.  Decodes nothing.
int steps_open(StepSet &S, hipStream_t st, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, const uint64_t *raw_len, uint64_t dst_cap)
{
    const uint32_t k = S.nblocks;
    S.off = off; S.len = len;
    S.bound.assign(k, 0); S.at.assign(k, 0); S.done.assign(k, 0); S.fin.assign(k, 0); S.started.assign(k, 0); S.tot.assign(k, dec::StreamResult{});
    S.bounded = raw_len != nullptr;
    uint64_t total = 0;
    for (uint32_t i = 0; i < k; i++) {
        S.at[i] = total;
        S.bound[i] = raw_len ? raw_len[i] : (S.d_dst ? dst_cap : ~0ull);
        if (raw_len) { if (raw_len[i] > ~0ull - total) return fail(NLZM_HIP_E_ARG, "the blocks' lengths do not fit 64 bits"); total += raw_len[i]; }
    }
    S.total = total;
    if (S.d_dst && raw_len && total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the blocks decode to %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
    HIPCHK(hipMalloc((void **)&S.states, (size_t)k * sizeof(dec::StepState)));
    HIPCHK(hipMemsetAsync(S.states, 0, (size_t)k * sizeof(dec::StepState), st));
    HIPCHK(hipStreamSynchronize(st));
    Last &L = g_last.here();
    L.steps = 0; L.step_ms = 0;
    S.open = true;
    return 0;
}

}  // namespace

extern "C" {

int nlzm_hip_decode_begin_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len, void *d_dst, uint64_t dst_cap, uint32_t flags)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    steps_close(S);                                 // a second begin closes the set before it
    if (!d_src || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    if (flags & ~(uint32_t)NLZM_HIP_DECODE_MORE) return fail(NLZM_HIP_E_ARG, "unknown flags %u (a decode that is cut in the middle of an op, as a prefix read is, cannot be resumed)", flags);
    if ((flags & NLZM_HIP_DECODE_MORE) && nblocks != 1) return fail(NLZM_HIP_E_ARG, "NLZM_HIP_DECODE_MORE is for one stream");
    if (!raw_len && nblocks != 1) return fail(NLZM_HIP_E_ARG, "raw_len may be NULL for one stream only");
    decode_begin_call();
    std::vector<uint64_t> off, len;
    if (flags & NLZM_HIP_DECODE_MORE) { off.assign(1, 0); len.assign(1, src_len); }       // (what has arrived so far: nothing to hop over yet)
    else if (const int rc = decode_split(st, d_src, src_len, nblocks, block_len, off, len)) return rc;
    S.d_src = (const uint8_t *)d_src; S.d_dst = (uint8_t *)d_dst; S.nblocks = nblocks; S.more = (flags & NLZM_HIP_DECODE_MORE) != 0;
    const int rc = steps_open(S, st, off, len, raw_len, dst_cap);
    if (rc) steps_close(S);
    return rc;
}

int nlzm_hip_decode_begin(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len, uint32_t flags)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    steps_close(S);
    if (!src || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    if (flags) return fail(NLZM_HIP_E_ARG, "flags %u: NLZM_HIP_DECODE_MORE is for nlzm_hip_decode_begin_dev (a decode cut in the middle of an op cannot be resumed)", flags);
    decode_begin_call();
    std::vector<uint64_t> off, len, raw;
    int rc = decode_split_host(src, src_len, nblocks, block_len, off, len);
    if (rc) return rc;
    HIPCHK(hipMalloc(&S.own_src, src_len ? src_len : 16));
    rc = [&]() -> int {
        HIPCHK(hipMemcpyAsync(S.own_src, src, src_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        if (raw_len) raw.assign(raw_len, raw_len + nblocks);
        else if (const int r = decode_sizes(st, (const uint8_t *)S.own_src, off, len, raw)) return r;      // the existing size pass
        uint64_t total = 0;
        for (uint32_t i = 0; i < nblocks; i++) { if (raw[i] > ~0ull - total) return fail(NLZM_HIP_E_ARG, "the blocks' lengths do not fit 64 bits"); total += raw[i]; }
        HIPCHK(hipMalloc(&S.own_dst, total ? total : 16));
        S.d_src = (const uint8_t *)S.own_src; S.d_dst = (uint8_t *)S.own_dst; S.nblocks = nblocks; S.more = false;
        return steps_open(S, st, off, len, raw.data(), total);
    }();
    if (rc) steps_close(S);
    return rc;
}

int nlzm_hip_decode_step(uint32_t max_frames, const uint64_t *target, uint64_t *done, int *finished, double *device_ms)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    if (!S.open) return fail(NLZM_HIP_E_ARG, "no decode set is open");
    if (!finished) return fail(NLZM_HIP_E_ARG, "null argument");
    decode_begin_call();
    Last &L = g_last.here();
    L.step_ms = 0;
    const uint32_t k = S.nblocks;
    std::vector<dec::StreamArgs> args;
    std::vector<uint32_t> who;
    for (uint32_t i = 0; i < k; i++) {
        if (S.fin[i] || (target && S.done[i] >= target[i])) continue;       // finished, or at its target already: not launched
        dec::StreamArgs a = decode_stream_args(S.d_src + S.off[i], S.len[i], S.d_dst ? S.d_dst + S.at[i] : nullptr, S.bound[i]);
        a.flags = (S.started[i] ? dec::kResume : 0u) | (S.more ? dec::kMore : 0u);
        a.state = S.states + i; a.max_frames = max_frames; a.target = target ? target[i] : ~0ull;
        args.push_back(a); who.push_back(i);
    }
    if (!args.empty()) {
        std::vector<dec::StreamResult> res;
        float ms = 0;
        int rc = launch_streams(st, args, res, true, &ms);
        for (size_t j = 0; !rc && j < who.size(); j++) {
            const uint32_t i = who[j];
            const dec::StreamResult &r = res[j];
            S.tot[i] = r; S.done[i] = r.out_len; S.started[i] = 1;
            if (r.rc == dec::kErrFormat) rc = fail(NLZM_HIP_E_FORMAT, "block %u of %u is not a well-formed NLZM stream (check %u failed after %llu output bytes)", i + 1, k, r.detail, r.out_len);
            else if (r.rc == dec::kErrCapacity) rc = fail(NLZM_HIP_E_CAPACITY, "block %u of %u decodes to more than the %llu bytes there is room for", i + 1, k, (unsigned long long)S.bound[i]);
            else if (r.rc != dec::kOk && r.rc != dec::kPaused) rc = fail(NLZM_HIP_E_KERNEL, "decode step kernel: block %u of %u ended with code %d after %llu output bytes", i + 1, k, r.rc, r.out_len);
            else if (r.rc == dec::kOk) {
                S.fin[i] = 1;
                if (S.bounded && r.out_len > S.bound[i]) rc = fail(NLZM_HIP_E_CAPACITY, "block %u decodes to %llu bytes, more than the %llu it was said to hold", i + 1, r.out_len, (unsigned long long)S.bound[i]);
                else if (S.bounded && r.out_len != S.bound[i]) rc = fail(NLZM_HIP_E_FORMAT, "block %u decodes to %llu bytes, not the %llu it was said to hold", i + 1, r.out_len, (unsigned long long)S.bound[i]);
            } else if (S.more && r.why == dec::kWhyInput && S.extended_flat) S.cut_off = true;      // the caller said "no more" and the stream still wants some
        }
        if (rc) { steps_close(S); return rc; }      // a failing step closes the set (block mode's rule)
        L.steps++;
        L.step_ms = ms;
    }
    // the set's totals so far
    L.sum = dec::StreamResult{};
    L.max_cycles = 0; L.max_stream = 0; L.streams = k;
    bool all = true;
    for (uint32_t i = 0; i < k; i++) {
        const dec::StreamResult &r = S.tot[i];
        L.sum.syms += r.syms; L.sum.raw_ops += r.raw_ops; L.sum.n_literal += r.n_literal; L.sum.n_dict += r.n_dict; L.sum.n_rep += r.n_rep;
        L.sum.ring_bytes += r.ring_bytes; L.sum.global_bytes += r.global_bytes; L.sum.out_len += S.done[i];
        L.sum.cycles += r.cycles; L.sum.window_cycles += r.window_cycles; L.sum.copy_cycles += r.copy_cycles;
        if (r.cycles > L.max_cycles) { L.max_cycles = r.cycles; L.max_stream = i; }
        if (done) done[i] = S.done[i];
        all = all && S.fin[i];
    }
    *finished = all ? 1 : 0;
    if (device_ms) *device_ms = L.step_ms;
    return 0;
}

int nlzm_hip_decode_extend_dev(uint64_t src_len_now)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    if (!S.open || !S.more) return fail(NLZM_HIP_E_ARG, "no decode set with NLZM_HIP_DECODE_MORE is open");
    if (src_len_now < S.len[0]) return fail(NLZM_HIP_E_ARG, "the stream cannot shrink (%llu bytes were there, now %llu)", (unsigned long long)S.len[0], (unsigned long long)src_len_now);
    S.extended_flat = src_len_now == S.len[0];      // an extend without growth: the caller's "that was all"
    if (!S.extended_flat) S.cut_off = false;        // (more has come after all: a step that paused for want of it no longer says "cut off")
    S.len[0] = src_len_now;
    return 0;
}

int nlzm_hip_decode_fetch(uint64_t off, uint64_t len, uint8_t *dst)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    if (!S.open) return fail(NLZM_HIP_E_ARG, "no decode set is open");
    if (!S.d_dst) return fail(NLZM_HIP_E_ARG, "the open decode set only sizes: it stores nothing");
    if (!dst && len) return fail(NLZM_HIP_E_ARG, "null argument");
    const uint64_t total = S.bounded ? S.total : S.done[0];
    if (off > total || len > total - off) return fail(NLZM_HIP_E_ARG, "the range (offset %llu, %llu bytes) runs over the %llu bytes there are", (unsigned long long)off, (unsigned long long)len, (unsigned long long)total);
    if (!len) return 0;
    for (uint32_t i = 0; i < S.nblocks; i++) {      // every block the range intersects must have decoded up to where the range ends in it
        const uint64_t lo = S.at[i], hi = S.bounded ? lo + S.bound[i] : total;
        if (hi <= off || lo >= off + len) continue;
        const uint64_t need = (off + len < hi ? off + len : hi) - lo;
        if (S.done[i] < need) return fail(NLZM_HIP_E_ARG, "block %u has decoded %llu bytes, the range needs %llu of it", i + 1, (unsigned long long)S.done[i], (unsigned long long)need);
    }
    HIPCHK(hipMemcpyAsync(dst, S.d_dst + off, len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int nlzm_hip_decode_finish(uint64_t *raw_len_out, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    StepSet &S = g_steps.here();
    if (!S.open) return fail(NLZM_HIP_E_ARG, "no decode set is open");
    bool all = true;
    for (uint32_t i = 0; i < S.nblocks; i++) all = all && S.fin[i];
    if (!all) {
        if (S.cut_off) { steps_close(S); return fail(NLZM_HIP_E_FORMAT, "the stream is cut off: it pauses for input that the caller says will not come"); }
        return fail(NLZM_HIP_E_ARG, "the decode set has not reached its end (the set stays open)");
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < S.nblocks; i++) { if (raw_len_out) raw_len_out[i] = S.done[i]; total += S.done[i]; }
    if (dst_len) *dst_len = total;
    steps_close(S);
    return 0;
}

void nlzm_hip_decode_abandon(void) { steps_close(g_steps.here()); }

}  // extern "C"
