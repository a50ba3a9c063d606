// nlzm_hip_crc.cpp -- host side of the device CRC32: the nlzm_hip_crc32* entry points of include/nlzm_hip.h.  Kernels: nlzm_crc.hip; the
// roles they run and the arithmetic: nlzm_crc.h.  Uses the library's device, stream and error text (nlzm_hip.cpp) as the decoder's host
// side does, and nothing else of the compress pipeline.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_crc.h"

namespace nlzm {
// nlzm_hip.cpp
int host_error(int code, const char *text);
int host_stream(hipStream_t *st);
// nlzm_crc.hip
void launch_crc(const crc::Args &a, uint32_t max_blocks, hipStream_t st);
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

// what nlzm_hip_get_counter("crc_*") reports: one record per device, as the decoder's
struct Last { double us = 0; unsigned long long bytes = 0; };
std::mutex g_last_mu;
std::map<int, Last> g_last_of;
Last &last_of_device()
{
    int device = -1;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> lk(g_last_mu);
    return g_last_of[device];
}

constexpr uint32_t kMaxRanges = 1u << 20;

}  // namespace

namespace nlzm {

int crc_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "crc_segment_bytes")) { *value = crc::kSegment; return 0; }       // (no device needed)
    if (!strcmp(key, "crc_us")) { *value = (uint64_t)(last_of_device().us + 0.5); return 0; }
    if (!strcmp(key, "crc_bytes")) { *value = last_of_device().bytes; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

void crc_begin_call() { Last &L = last_of_device(); L.us = 0; L.bytes = 0; }

// The CRC32 (from `seed`) of nranges ranges of the buffer at d_buf, on stream st; off / len / crc_out are host arrays.  Returns when the
// CRCs are in crc_out.  Also what nlzm_hip_check* (nlzm_hip_decode.cpp) and nlzm_hip_feed_input_crc32 (nlzm_hip.cpp) call.
int crc_ranges_on(hipStream_t st, const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t seed,
                  uint32_t *crc_out)
{
    if (!nranges) return 0;
    if (nranges > kMaxRanges) return fail(NLZM_HIP_E_ARG, "%u ranges, at most %u in one call", nranges, kMaxRanges);
    std::vector<unsigned long long> h(3 * ((size_t)nranges + 1));
    unsigned long long *h_off = h.data(), *h_len = h_off + nranges + 1, *h_seg0 = h_len + nranges + 1;
    unsigned long long nsegs = 0, bytes = 0;
    for (uint32_t i = 0; i < nranges; i++) {
        if (off[i] > buf_len || len[i] > buf_len - off[i])      // (no off + len: it can wrap)
            return fail(NLZM_HIP_E_ARG, "range %u (offset %llu, %llu bytes) runs over the %llu bytes of the buffer", i, (unsigned long long)off[i],
                        (unsigned long long)len[i], (unsigned long long)buf_len);
        h_off[i] = off[i]; h_len[i] = len[i]; h_seg0[i] = nsegs;
        nsegs += len[i] / crc::kSegment + (len[i] % crc::kSegment ? 1 : 0);
        bytes += len[i];
        if (nsegs > (1ull << 31)) return fail(NLZM_HIP_E_ARG, "the ranges of one call may hold 2^31 segments of %llu bytes in all", crc::kSegment);
    }
    h_off[nranges] = h_len[nranges] = 0; h_seg0[nranges] = nsegs;
    if (!d_buf && bytes) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf dh, dp, dout;
    int rc = dh.alloc(h.size() * sizeof(unsigned long long));
    if (!rc) rc = dp.alloc(nsegs * sizeof(uint32_t));
    if (!rc) rc = dout.alloc(nranges * sizeof(uint32_t));
    if (rc) return rc;
    Events E;
    if ((rc = E.create())) return rc;
    crc::Args a{};
    a.buf = (const uint8_t *)d_buf;
    a.off = dh.as<unsigned long long>(); a.len = a.off + nranges + 1; a.seg0 = a.len + nranges + 1;
    a.part = dp.as<uint32_t>(); a.out = dout.as<uint32_t>();
    a.nranges = nranges; a.seed = seed; a.nsegs = nsegs;
    hipError_t e = hipMemcpyAsync(dh.p, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(E.ev[0], st);
    if (e == hipSuccess) { launch_crc(a, 1u << 22, st); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(E.ev[1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(crc_out, dout.p, nranges * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);           // (nothing queued before the failure may outlive `h` and `crc_out`)
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, E.ev[0], E.ev[1]);
    if (e != hipSuccess) return fail(NLZM_HIP_E_NODEVICE, "CRC launch failed: %s", hipGetErrorString(e));
    Last &L = last_of_device();
    L.us += 1000.0 * ms;
    L.bytes += bytes;
    return 0;
}

}  // namespace nlzm

extern "C" {

uint32_t nlzm_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc::combine(crc_a, crc_b, len_b); }

int nlzm_hip_crc32_ranges_dev(const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t *crc)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (nranges && (!off || !len || !crc)) return fail(NLZM_HIP_E_ARG, "null argument");
    crc_begin_call();
    return crc_ranges_on(st, d_buf, buf_len, nranges, off, len, 0, crc);
}

int nlzm_hip_crc32_dev(const void *d_buf, uint64_t n, uint32_t seed, uint32_t *crc)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!crc || (!d_buf && n)) return fail(NLZM_HIP_E_ARG, "null argument");
    crc_begin_call();
    const uint64_t off = 0;
    return crc_ranges_on(st, d_buf, n, 1, &off, &n, seed, crc);
}

int nlzm_hip_crc32_ranges(const uint8_t *buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t *crc)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if ((!buf && buf_len) || (nranges && (!off || !len || !crc))) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf d;
    if (const int rc = d.alloc(buf_len)) return rc;
    if (buf_len) HIPCHK(hipMemcpyAsync(d.p, buf, buf_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return nlzm_hip_crc32_ranges_dev(d.p, buf_len, nranges, off, len, crc);
}

int nlzm_hip_crc32(const uint8_t *buf, uint64_t n, uint32_t seed, uint32_t *crc)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!crc || (!buf && n)) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf d;
    if (const int rc = d.alloc(n)) return rc;
    if (n) HIPCHK(hipMemcpyAsync(d.p, buf, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return nlzm_hip_crc32_dev(d.p, n, seed, crc);
}

}  // extern "C"
