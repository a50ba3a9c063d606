// nlzm_hip_crc.cpp -- host side of the device CRC32: the nlzm_hip_crc32* entry points of include/nlzm_hip.h.  Kernels: nlzm_crc.hip; the
// roles they run and the arithmetic: nlzm_crc.h.  Uses the library's device, stream and error text (nlzm_hip.cpp) as the decoder's host
// side does, and nothing else of the compress pipeline.
#include <stdint.h>
#include <string.h>

#include "nlzm_host_util.h"
#include "nlzm_crc.h"
#include "nlzm_read_plan.h"

using namespace nlzm;

namespace {

// what nlzm_hip_get_counter("crc_*") reports of the last call
struct Last { double us = 0; unsigned long long bytes = 0; };
PerDevice<Last> g_last;

constexpr uint32_t kMaxRanges = 1u << 20;

}  // namespace

namespace nlzm {

int crc_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "crc_segment_bytes")) { *value = crc::kSegment; return 0; }       // (no device needed)
    if (!strcmp(key, "crc_us")) { *value = (uint64_t)(g_last.here().us + 0.5); return 0; }
    if (!strcmp(key, "crc_bytes")) { *value = g_last.here().bytes; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

void crc_begin_call() { Last &L = g_last.here(); L.us = 0; L.bytes = 0; }

// The CRC32 (from `seed`) of nranges ranges of the buffer at d_buf, on stream st; off / len / crc_out are host arrays.  Returns when the
// CRCs are in crc_out.  Also what nlzm_hip_check* (nlzm_hip_decode.cpp) and nlzm_hip_feed_input_crc32 (nlzm_hip_feed.cpp) call.
int crc_ranges_on(hipStream_t st, const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t seed,
                  uint32_t *crc_out)
{
    if (!nranges) return 0;
    if (nranges > kMaxRanges) return fail(NLZM_HIP_E_ARG, "%u ranges, at most %u in one call", nranges, kMaxRanges);
    crc::SegTable T;
    char why[512];
    if (const int rc = T.make(buf_len, nranges, off, len, crc::kSegment, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (!d_buf && T.bytes) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf dh, dp, dout;
    int rc = dh.alloc(T.words.size() * sizeof(unsigned long long));
    if (!rc) rc = dp.alloc(T.nsegs * sizeof(uint32_t));
    if (!rc) rc = dout.alloc(nranges * sizeof(uint32_t));
    if (rc) return rc;
    crc::Args a{};
    a.buf = (const uint8_t *)d_buf;
    T.point(a, dh.as<unsigned long long>());
    a.part = dp.as<uint32_t>(); a.out = dout.as<uint32_t>();
    a.seed = seed;
    float ms = 0;
    rc = timed_launch(st, "CRC", &ms,
        [&] { return hipMemcpyAsync(dh.p, T.words.data(), T.words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st); },
        [&] { launch_crc(a, kStrideBlocksWide, st); },
        [&] { return hipMemcpyAsync(crc_out, dout.p, nranges * sizeof(uint32_t), hipMemcpyDeviceToHost, st); });
    if (rc) return rc;
    Last &L = g_last.here();
    L.us += 1000.0 * ms;
    L.bytes += T.bytes;
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
    if (const int rc = upload(d, buf, buf_len, st)) return rc;
    return nlzm_hip_crc32_ranges_dev(d.p, buf_len, nranges, off, len, crc);
}

int nlzm_hip_crc32(const uint8_t *buf, uint64_t n, uint32_t seed, uint32_t *crc)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    if (!crc || (!buf && n)) return fail(NLZM_HIP_E_ARG, "null argument");
    DevBuf d;
    if (const int rc = upload(d, buf, n, st)) return rc;
    return nlzm_hip_crc32_dev(d.p, n, seed, crc);
}

}  // extern "C"
