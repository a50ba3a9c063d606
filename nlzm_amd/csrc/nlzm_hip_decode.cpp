// nlzm_hip_decode.cpp -- host side of the device decoder: the nlzm_hip_decompress* / nlzm_hip_verify_dev entry points of
// include/nlzm_hip.h.  Kernels: nlzm_decode.hip; the role they run: nlzm_decode.h.  Uses the library's device, stream and error text
// (nlzm_hip.cpp) and nothing else of the compress pipeline.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_decode.h"
#include "nlzm_host_decode.h"

namespace nlzm {
// nlzm_hip.cpp
int host_error(int code, const char *text);
int host_stream(hipStream_t *st);
// nlzm_decode.hip
void launch_decode(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st);
void launch_split(const void *d_src, unsigned long long len, uint32_t nblocks, unsigned long long *d_block_len, uint32_t *d_bad, hipStream_t st);
void launch_compare(const void *d_a, const void *d_b, unsigned long long n, unsigned long long *d_first, hipStream_t st);
// nlzm_hip_crc.cpp
void crc_begin_call();
int crc_ranges_on(hipStream_t st, const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t seed, uint32_t *crc_out);
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

// what nlzm_hip_get_counter("decode_*") reports: the streams of the last storing pass (of the last size pass, if the call made no other).
// One record per device, like the rest of the library's state; the map is guarded, a record is its device's (calls are not re-entrant per device).
struct Last {
    dec::StreamResult sum{};
    unsigned long long max_cycles = 0, max_stream = 0, streams = 0, passes = 0;
    double ms = 0;                                  // device time of all passes of the last call
};
std::mutex g_last_mu;
std::map<int, Last> g_last_of;
Last &last_of_device()
{
    int device = -1;
    (void)hipGetDevice(&device);                    // (no device: one record under -1, which only ever holds zeros)
    std::lock_guard<std::mutex> lk(g_last_mu);
    return g_last_of[device];
}
#define g_last (last_of_device())

struct Events {
    hipEvent_t ev[2] = { nullptr, nullptr };
    ~Events() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    int create() { for (auto &e : ev) HIPCHK(hipEventCreate(&e)); return 0; }
};

// A minute and a second per megabyte of stream, in clock100() ticks: a lone wave decodes tens of megabytes of output a second,
// so this is an order of magnitude above any well-formed stream and still ends a decode that has gone wrong.
unsigned long long budget_for(uint64_t stream_len) { return (60ull + stream_len / 1000000ull) * 100000000ull; }

// one launch of the streams in `args` (a destination pointer, a bound and the flags per stream); res: what each reported
int run_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res)
{
    const size_t k = args.size();
    DevBuf da, dr;
    int rc = da.alloc(k * sizeof(dec::StreamArgs));
    if (!rc) rc = dr.alloc(k * sizeof(dec::StreamResult));
    if (rc) return rc;
    Events E;
    if ((rc = E.create())) return rc;
    hipEvent_t *ev = E.ev;
    res.assign(k, dec::StreamResult{});
    hipError_t e = hipMemcpyAsync(da.p, args.data(), k * sizeof(dec::StreamArgs), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(dr.p, 0xFF, k * sizeof(dec::StreamResult), st);      // (a workgroup that never ran reports rc = -1)
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess) { launch_decode(da.p, dr.p, (uint32_t)k, st); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), dr.p, k * sizeof(dec::StreamResult), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);           // (nothing queued before the failure may outlive `args` and `res`)
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (e != hipSuccess) return fail(NLZM_HIP_E_NODEVICE, "decode launch failed: %s", hipGetErrorString(e));
    Last &L = last_of_device();
    L.ms += ms;
    L.passes++;
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

// stream i = [d_src + off[i], + len[i]) -> d_dst + dst_off[i], at most cap[i] bytes (d_dst == nullptr: sizes only)
int run_pass(hipStream_t st, const uint8_t *d_src, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, uint8_t *d_dst,
             const std::vector<uint64_t> &dst_off, const std::vector<uint64_t> &cap, std::vector<dec::StreamResult> &res)
{
    const size_t k = off.size();
    std::vector<dec::StreamArgs> args(k);
    for (size_t i = 0; i < k; i++)
        args[i] = dec::StreamArgs{ d_src + off[i], len[i], d_dst ? d_dst + dst_off[i] : nullptr, d_dst ? cap[i] : ~0ull, budget_for(len[i]) };
    return run_streams(st, args, res);
}

void begin_call() { g_last.ms = 0; g_last.passes = 0; }

// the block streams' offsets and lengths: given, or found by hopping over their frame headers on the device
int split(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    off.assign(nblocks, 0); len.assign(nblocks, 0);
    if (block_len) {
        uint64_t at = 0;
        for (uint32_t i = 0; i < nblocks; i++) {
            if (block_len[i] > src_len - at) return fail(NLZM_HIP_E_ARG, "block %u's length %llu runs over the %llu bytes given", i + 1, (unsigned long long)block_len[i], (unsigned long long)src_len);
            off[i] = at; len[i] = block_len[i]; at += block_len[i];
        }
        return 0;
    }
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
    if (bad) return fail(NLZM_HIP_E_FORMAT, "block %u of %u is not an NLZM stream, or is cut off (found by the frame headers)", bad, nblocks);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nblocks; i++) { off[i] = at; at += len[i]; }
    return 0;
}

int blocks_dev(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in, void *d_dst,
               uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    std::vector<uint64_t> off, len, raw(nblocks), dst_off(nblocks);
    int rc = split(st, d_src, src_len, nblocks, block_len, off, len);
    if (rc) return rc;
    std::vector<dec::StreamResult> res;
    if (raw_len_in) for (uint32_t i = 0; i < nblocks; i++) raw[i] = raw_len_in[i];
    else {
        rc = run_pass(st, (const uint8_t *)d_src, off, len, nullptr, dst_off, raw, res);
        if (rc) return rc;
        for (uint32_t i = 0; i < nblocks; i++) raw[i] = res[i].out_len;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < nblocks; i++) { dst_off[i] = total; total += raw[i]; }
    if (d_dst) {
        if (total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the blocks decode to %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
        rc = run_pass(st, (const uint8_t *)d_src, off, len, (uint8_t *)d_dst, dst_off, raw, res);
        if (rc) return rc;
        for (uint32_t i = 0; i < nblocks; i++)
            if (res[i].out_len != raw[i])
                return fail(NLZM_HIP_E_FORMAT, "block %u decodes to %llu bytes, not the %llu it was said to hold", i + 1, res[i].out_len, (unsigned long long)raw[i]);
    }
    if (raw_len_out) for (uint32_t i = 0; i < nblocks; i++) raw_len_out[i] = raw[i];
    if (dst_len) *dst_len = total;
    return 0;
}

}  // namespace

namespace nlzm {
// what the range reader (nlzm_hip_range.cpp) shares with the entries here
void decode_begin_call() { begin_call(); }
double decode_call_ms() { return g_last.ms; }
unsigned long long decode_budget_for(uint64_t stream_len) { return budget_for(stream_len); }
int decode_run_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res) { return run_streams(st, args, res); }
int decode_split(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    return split(st, d_src, src_len, nblocks, block_len, off, len);
}
int decode_counter(const char *key, uint64_t *value)
{
    static const struct { const char *name; unsigned long long dec::StreamResult::*m; } kSum[] = {
        { "decode_syms", &dec::StreamResult::syms }, { "decode_raw_ops", &dec::StreamResult::raw_ops }, { "decode_n_literal", &dec::StreamResult::n_literal },
        { "decode_n_dict", &dec::StreamResult::n_dict }, { "decode_n_rep", &dec::StreamResult::n_rep }, { "decode_ring_bytes", &dec::StreamResult::ring_bytes },
        { "decode_global_bytes", &dec::StreamResult::global_bytes }, { "decode_out_bytes", &dec::StreamResult::out_len }, { "decode_cycles", &dec::StreamResult::cycles },
        { "decode_window_cycles", &dec::StreamResult::window_cycles }, { "decode_copy_cycles", &dec::StreamResult::copy_cycles },
    };
    for (const auto &e : kSum) if (!strcmp(key, e.name)) { *value = g_last.sum.*(e.m); return 0; }
    if (!strcmp(key, "decode_max_stream_cycles")) { *value = g_last.max_cycles; return 0; }
    if (!strcmp(key, "decode_slowest_stream")) { *value = g_last.max_stream; return 0; }
    if (!strcmp(key, "decode_streams")) { *value = g_last.streams; return 0; }
    if (!strcmp(key, "decode_passes")) { *value = g_last.passes; return 0; }
    if (!strcmp(key, "decode_ms")) { *value = (uint64_t)(g_last.ms + 0.5); return 0; }
    if (!strcmp(key, "decode_us")) { *value = (uint64_t)(g_last.ms * 1000.0 + 0.5); return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}
}  // namespace nlzm

extern "C" {

int nlzm_hip_decompress_dev(const void *d_stream, uint64_t stream_len, void *d_dst, uint64_t dst_cap, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!d_stream || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    begin_call();
    const std::vector<uint64_t> off{ 0 }, len{ stream_len }, cap{ dst_cap };
    std::vector<dec::StreamResult> res;
    const int rc = run_pass(st, (const uint8_t *)d_stream, off, len, (uint8_t *)d_dst, off, cap, res);
    if (rc) return rc;
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
    begin_call();
    return blocks_dev(st, d_src, src_len, nblocks, block_len, raw_len_in, d_dst, dst_cap, raw_len_out, dst_len);
}

int nlzm_hip_decompress_blocks(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in,
                               uint8_t *dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!src || !nblocks || nblocks > 65536) return fail(NLZM_HIP_E_ARG, "null argument, or nblocks outside 1 .. 65536");
    begin_call();
    // host buffers: the container is split on the host (the same hop the command line makes), sized on the device, decoded into a
    // device buffer of exactly that size and copied back
    std::vector<uint64_t> blen(nblocks);
    if (block_len) memcpy(blen.data(), block_len, nblocks * sizeof(uint64_t));
    else {
        uint64_t at = 0;
        for (uint32_t i = 0; i < nblocks; i++) {
            const size_t l = nlzm_host::stream_length(nlzm_host::Span{ src + at, (size_t)(src_len - at) });
            if (!l) return fail(NLZM_HIP_E_FORMAT, "block %u of %u is not an NLZM stream, or is cut off (found by the frame headers)", i + 1, nblocks);
            blen[i] = l; at += l;
        }
    }
    DevBuf ds, dd;
    int rc = ds.alloc(src_len);
    if (rc) return rc;
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
    begin_call();
    // The blocks of a container made from n bytes hold ceil(n / nblocks) bytes each (the last ones fewer): decoded on that assumption in
    // ONE pass, every block bounded by its share.  A container that does not fit it (some other partition, a wrong length) is sized first.
    std::vector<uint64_t> raw(nblocks);
    const uint64_t per = (n + nblocks - 1) / nblocks;
    for (uint32_t i = 0; i < nblocks; i++) { const uint64_t lo = i * per < n ? i * per : n, hi = lo + per < n ? lo + per : n; raw[i] = hi - lo; }
    DevBuf dd, df;
    int rc = dd.alloc(n);
    if (!rc) rc = df.alloc(sizeof(unsigned long long));
    if (rc) return rc;
    uint64_t total = 0;
    rc = blocks_dev(st, d_src, src_len, nblocks, block_len, raw.data(), dd.p, n, nullptr, &total);
    if (rc == NLZM_HIP_E_CAPACITY || rc == NLZM_HIP_E_FORMAT) {
        const double ms = g_last.ms;
        rc = blocks_dev(st, d_src, src_len, nblocks, block_len, nullptr, nullptr, 0, raw.data(), &total);       // sizes
        if (rc) return rc;
        (void)hipFree(dd.p); dd.p = nullptr;
        rc = dd.alloc(total);
        if (rc) return rc;
        rc = blocks_dev(st, d_src, src_len, nblocks, block_len, raw.data(), dd.p, total, nullptr, &total);
        g_last.ms += ms;
    }
    if (rc) return rc;
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
    begin_call();
    crc_begin_call();
    // With the lengths the caller holds: ONE decode pass, every block bounded by its length.  A block that decodes to more or to less shows in
    // that pass's error; the blocks are then sized and decoded by what they hold, as without lengths, and the comparison below names the block.
    std::vector<uint64_t> raw(nblocks), off(nblocks);
    DevBuf dd;
    uint64_t total = 0;
    int rc = NLZM_HIP_E_FORMAT;
    if (raw_len) {
        bool fits = true;
        for (uint32_t i = 0; i < nblocks; i++) { if (raw_len[i] > ~0ull - total) fits = false; else total += raw_len[i]; }
        if (fits && hipMalloc(&dd.p, total ? total : 16) == hipSuccess)
            rc = blocks_dev(st, d_src, src_len, nblocks, block_len, raw_len, dd.p, total, raw.data(), &total);
        else { (void)hipGetLastError(); dd.p = nullptr; }         // (lengths no buffer can hold are wrong lengths)
        if (rc && rc != NLZM_HIP_E_CAPACITY && rc != NLZM_HIP_E_FORMAT) return rc;
    }
    if (rc) {
        const double ms = g_last.ms;
        rc = blocks_dev(st, d_src, src_len, nblocks, block_len, nullptr, nullptr, 0, raw.data(), &total);       // sizes
        if (rc) return rc;
        if (dd.p) { (void)hipFree(dd.p); dd.p = nullptr; }
        rc = dd.alloc(total);
        if (rc) return rc;
        rc = blocks_dev(st, d_src, src_len, nblocks, block_len, raw.data(), dd.p, total, nullptr, &total);
        g_last.ms += ms;
        if (rc) return rc;
    }
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
