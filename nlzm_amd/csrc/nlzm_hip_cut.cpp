// nlzm_hip_cut.cpp -- host side of the content-defined cut points: the nlzm_hip_cut_points* entry points of include/nlzm_hip.h.  Kernels:
// nlzm_cut.hip; the roles they run and the rule: nlzm_cut.h.  Uses the library's device, stream and error text (nlzm_hip.cpp) as the CRC's
// host side does, and nothing else of the compress pipeline.
#include <stdint.h>
#include <string.h>

#include "nlzm_host_util.h"
#include "nlzm_cut_host.h"
#include "nlzm_cut.h"
#include "nlzm_units.h"

using namespace nlzm;

namespace {

// what nlzm_hip_get_counter("cut_*") reports of the last call
struct Last { double us = 0; unsigned long long candidates = 0; };
PerDevice<Last> g_last;

// the arguments that need no device
int check_args(uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len, const uint64_t *cut, uint32_t cut_cap, const uint32_t *ncuts)
{
    if (!ncuts || (!cut && cut_cap)) return fail(NLZM_HIP_E_ARG, "null argument");
    if (avg_bits < 1 || avg_bits > 30) return fail(NLZM_HIP_E_ARG, "avg_bits %u out of range (1 .. 30)", avg_bits);
    if (min_len < 32 || min_len > max_len || max_len > (1ull << 31))
        return fail(NLZM_HIP_E_ARG, "min_len %llu, max_len %llu: 32 <= min_len <= max_len <= 2^31", (unsigned long long)min_len, (unsigned long long)max_len);
    if (n / min_len > 0xFFFFFFFFull) return fail(NLZM_HIP_E_ARG, "%llu bytes may take more than 2^32 - 1 cuts at min_len %llu", (unsigned long long)n, (unsigned long long)min_len);
    return 0;
}

// the cuts of the n bytes at d_src, on stream st.  Device memory: the bitmap (n / 8 bytes), a word per segment, the list (what the caller's
// has room for, n / min_len entries at most) and two result words.
int cut_points_on(hipStream_t st, const void *d_src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len, uint64_t *cut, uint32_t cut_cap, uint32_t *ncuts)
{
    Last &L = g_last.here();
    L.us = 0; L.candidates = 0;
    *ncuts = 0;
    if (n <= min_len) return 0;                     // (no cut fits: one block, n = 0 included; nothing is read)
    if (!d_src) return fail(NLZM_HIP_E_ARG, "null argument");
    cut::Args a{};
    a.src = (const uint8_t *)d_src;
    a.n = n;
    a.nsegs = units::count(n, cut::kSegment);
    a.min_len = min_len; a.max_len = max_len;
    a.shift = 32 - avg_bits;
    a.cut_cap = n / min_len < cut_cap ? n / min_len : cut_cap;
    DevBuf bits, count, list;
    int rc = bits.alloc((size_t)((n + 31) / 32) * sizeof(uint32_t));
    if (!rc) rc = count.alloc((size_t)a.nsegs * sizeof(uint32_t));
    if (!rc) rc = list.alloc((size_t)(a.cut_cap + 2) * sizeof(unsigned long long));
    if (rc) return rc;
    a.bits = bits.as<uint32_t>(); a.count = count.as<uint32_t>();
    a.res = list.as<unsigned long long>(); a.cut = a.res + 2;
    unsigned long long res[2] = { 0, 0 };
    float ms = 0;
    rc = timed_launch(st, "cut", &ms,
        [&] { return hipSuccess; },
        [&] { launch_cut(a, kStrideBlocksWide, st); },
        [&] { return hipMemcpyAsync(res, a.res, sizeof res, hipMemcpyDeviceToHost, st); });
    if (rc) return rc;
    L.us = 1000.0 * ms;
    L.candidates = res[1];
    *ncuts = (uint32_t)res[0];
    if (res[0] > cut_cap) return fail(NLZM_HIP_E_CAPACITY, "the input takes %llu cuts, cut_cap %u", res[0], cut_cap);
    if (res[0]) HIPCHK(hipMemcpy(cut, a.cut, (size_t)res[0] * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

namespace nlzm {

int cut_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "cut_segment_bytes")) { *value = cut::kSegment; return 0; }       // (no device needed)
    if (!strcmp(key, "cut_us")) { *value = (uint64_t)(g_last.here().us + 0.5); return 0; }
    if (!strcmp(key, "cut_candidates")) { *value = g_last.here().candidates; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

}  // namespace nlzm

extern "C" {

int nlzm_hip_cut_points_dev(const void *d_src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len, uint64_t *cut, uint32_t cut_cap, uint32_t *ncuts)
{
    if (const int rc = check_args(n, avg_bits, min_len, max_len, cut, cut_cap, ncuts)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    return cut_points_on(st, d_src, n, avg_bits, min_len, max_len, cut, cut_cap, ncuts);
}

int nlzm_hip_cut_points(const uint8_t *src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len, uint64_t *cut, uint32_t cut_cap, uint32_t *ncuts)
{
    if (const int rc = check_args(n, avg_bits, min_len, max_len, cut, cut_cap, ncuts)) return rc;
    if (!src && n) return fail(NLZM_HIP_E_ARG, "null argument");
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    DevBuf d;
    if (const int rc = upload(d, src, n, st)) return rc;
    return cut_points_on(st, d.p, n, avg_bits, min_len, max_len, cut, cut_cap, ncuts);
}

}  // extern "C"
