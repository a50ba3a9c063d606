// nlzm_hip_elem.cpp -- host side of the choice of a typed range's element size: the entry points of include/nlzm_hip_elem.h.  Kernels: nlzm_elem.hip;
// the roles they run and the rule: nlzm_elem.h; the argument checks, the launch's table, the scratch layout and the choice: nlzm_elem_plan.h.  Uses the
// library's device, stream and error text (nlzm_hip.cpp) as the byte planes' host side does; the _auto calls run nlzm_hip_compress_ranges_typed_dev on
// the sizes chosen, and nothing else of the compress side.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nlzm_hip_elem.h"
#include "nlzm_host_util.h"
#include "nlzm_elem_host.h"
#include "nlzm_elem.h"
#include "nlzm_elem_plan.h"

using namespace nlzm;

static_assert(elem::kBins == elem::kCounters && elem::kNoSlot == elem::kNone, "the plan's table is the roles'");
static_assert(elem::kSegment % 16 == 0 && elem::kSegment < (1ull << 32), "units of sixteen bytes, counters of 32 bits");

namespace {

// what nlzm_hip_get_counter("elem_*") reports of the last call
struct Last { double us = 0; unsigned long long bytes = 0; };
PerDevice<Last> g_last;

int check_args(const void *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, const void *out)
{
    char why[512] = "";
    if (const int rc = elem::check_ranges(buf_len, k, off, len, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if ((!buf && buf_len) || !out) return fail(NLZM_HIP_E_ARG, "null argument");
    return 0;
}

// the costs of k checked ranges, and their histograms where hist is not NULL: the table uploaded, the totals zeroed, the launches timed, the
// records copied back.  Nothing stays allocated.
int costs_on(hipStream_t st, const void *d_buf, uint32_t k, const uint64_t *off, const uint64_t *len, uint64_t *cost, uint64_t *hist)
{
    g_last.here() = Last{};
    elem::Table T;
    T.make(k, off, len, elem::kSegment, hist != nullptr);
    const elem::Scratch need(T);
    memset(cost, 0, (size_t)k * 32);
    if (hist) memset(hist, 0, (size_t)k * elem::kBins * 8);
    g_last.here().bytes = T.bytes;
    if (!T.nsegs) return 0;                         // (no range holds eight bytes: every cost is 0, and nothing is launched)
    DevBuf dt, dc, dh;
    if (const int rc = dt.alloc_for(need.table, "the ranges' table")) return rc;
    if (const int rc = dc.alloc_for(need.cost, "the ranges' costs")) return rc;
    if (const int rc = dh.alloc_for(need.totals, "the ranges' byte counts")) return rc;
    elem::Args a{};
    a.src = (const uint8_t *)d_buf; a.totals = dh.as<unsigned long long>(); a.cost = dc.as<unsigned long long>();
    T.point(a, dt.as<unsigned long long>());
    float ms = 0;
    const int rc = timed_launch(st, "elem", &ms,
        [&] {
            hipError_t e = hipMemcpyAsync(dt.p, T.words.data(), need.table, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemsetAsync(dc.p, 0, need.cost, st);
            if (e == hipSuccess && need.totals) e = hipMemsetAsync(dh.p, 0, need.totals, st);
            return e;
        },
        [&] { launch_elem(a, kStrideBlocks, st); },
        [&] {
            hipError_t e = hipMemcpyAsync(cost, dc.p, need.cost, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && hist) e = hipMemcpyAsync(hist, dh.p, need.totals, hipMemcpyDeviceToHost, st);
            return e;
        });
    if (rc) return rc;
    g_last.here().us = 1000.0 * ms;
    return 0;
}

int choose_on(hipStream_t st, const void *d_buf, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem_out)
{
    std::vector<uint64_t> cost((size_t)k * 4);
    if (const int rc = costs_on(st, d_buf, k, off, len, cost.data(), nullptr)) return rc;
    for (uint32_t i = 0; i < k; i++) elem_out[i] = (uint8_t)elem::choose(&cost[4 * (size_t)i], len[i]);
    return 0;
}

}  // namespace

namespace nlzm {

int elem_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "elem_segment_bytes")) { *value = elem::kSegment; return 0; }          // (no device needed)
    if (!strcmp(key, "elem_us")) { *value = (uint64_t)(g_last.here().us + 0.5); return 0; }
    if (!strcmp(key, "elem_bytes")) { *value = g_last.here().bytes; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

}  // namespace nlzm

extern "C" {

uint32_t nlzm_hip_choose_elem(const uint64_t *cost4, uint64_t len) { return cost4 ? elem::choose(cost4, len) : 1; }

int nlzm_hip_plane_costs_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint64_t *cost, uint64_t *hist)
{
    if (const int rc = check_args(d_buf, buf_len, k, off, len, cost)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    return costs_on(st, d_buf, k, off, len, cost, hist);
}

int nlzm_hip_plane_costs(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint64_t *cost, uint64_t *hist)
{
    if (const int rc = check_args(buf, buf_len, k, off, len, cost)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    DevBuf d;
    if (const int rc = upload(d, buf, buf_len, st)) return rc;
    return costs_on(st, d.p, k, off, len, cost, hist);
}

int nlzm_hip_choose_elems_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem)
{
    if (const int rc = check_args(d_buf, buf_len, k, off, len, elem)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    return choose_on(st, d_buf, k, off, len, elem);
}

int nlzm_hip_choose_elems(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem)
{
    if (const int rc = check_args(buf, buf_len, k, off, len, elem)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    DevBuf d;
    if (const int rc = upload(d, buf, buf_len, st)) return rc;
    return choose_on(st, d.p, k, off, len, elem);
}

int nlzm_hip_compress_ranges_auto_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem_out,
                                      uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (const int rc = check_args(d_src, n, k, off, len, elem_out)) return rc;
    if (!d_dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    const uint64_t bound = nlzm_hip_compress_ranges_bound(k, len);
    if (dst_cap < bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)bound);
    if (const int rc = choose_on(st, d_src, k, off, len, elem_out)) return rc;
    return nlzm_hip_compress_ranges_typed_dev(d_src, n, k, off, len, elem_out, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
}

int nlzm_hip_compress_ranges_auto(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem_out,
                                  uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (const int rc = check_args(src, n, k, off, len, elem_out)) return rc;
    if (!dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    const uint64_t bound = nlzm_hip_compress_ranges_bound(k, len);
    if (dst_cap < bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)bound);
    // the input with what the compress path reads behind it (ranges left at e = 1 are compressed where they lie), the streams in a buffer of the call's
    constexpr uint64_t kBehind = 512;
    if (n > ~0ull - kBehind) return fail(NLZM_HIP_E_NOMEM, "no %llu bytes of device memory for the input", (unsigned long long)n);
    DevBuf in, out;
    if (const int rc = in.alloc_for(n + kBehind, "the input")) return rc;
    if (const int rc = out.alloc_for(bound, "the ranges' streams")) return rc;
    HIPCHK(hipMemsetAsync(in.as<uint8_t>() + n, 0, kBehind, st));
    if (n) HIPCHK(hipMemcpyAsync(in.p, src, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t got = 0;
    if (const int rc = nlzm_hip_compress_ranges_auto_dev(in.p, n, k, off, len, elem_out, hist_bits_req, out.p, bound, block_len, &got)) return rc;
    if (got) HIPCHK(hipMemcpy(dst, out.p, got, hipMemcpyDeviceToHost));
    *dst_len = got;
    return 0;
}

}  // extern "C"
