// nlzm_hip_planes.cpp -- host side of the byte-plane filter of typed ranges: the nlzm_hip_planes*, nlzm_hip_compress_ranges_typed* and
// nlzm_hip_decompress_blocks_typed* entry points of include/nlzm_hip.h.  Kernels: nlzm_planes.hip; the roles they run and the rule: nlzm_planes.h; the
// argument checks, the launch's table and the scratch layout: nlzm_planes_plan.h.  Uses the library's device, stream and error text (nlzm_hip.cpp) as
// the cut points' host side does; the typed calls run the untyped entry points (nlzm_hip_compress_ranges_dev, nlzm_hip_decompress_blocks_dev) on a
// scratch allocation, and nothing else of either pipeline.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "nlzm_host_util.h"
#include "nlzm_planes_host.h"
#include "nlzm_planes.h"
#include "nlzm_planes_plan.h"

using namespace nlzm;

namespace {

// what nlzm_hip_get_counter("planes_*") reports of the last call
struct Last { double us = 0; unsigned long long bytes = 0; };
PerDevice<Last> g_last;

int check_args(const void *src, uint64_t src_len, const void *dst, uint64_t dst_len, uint32_t k, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len,
               const uint8_t *elem)
{
    char why[512] = "";
    if (const int rc = planes::check_ranges((uint64_t)(uintptr_t)src, src_len, (uint64_t)(uintptr_t)dst, dst_len, k, src_off, dst_off, len, elem, ErrText{ why, sizeof why }))
        return fail(rc, "%s", why);
    if ((!src && src_len) || (!dst && dst_len)) return fail(NLZM_HIP_E_ARG, "null argument");
    return 0;
}

bool all_bytes(uint32_t k, const uint8_t *elem)
{
    if (!elem || !k || k > planes::kMaxRanges) return true;        // (no sizes, or a count the untyped call refuses)
    for (uint32_t i = 0; i < k; i++) if (elem[i] != 1) return false;
    return true;
}

// k checked ranges in ONE launch on stream st: the table uploaded, the kernel timed; its time and bytes are ADDED to the call's counters
int planes_on(hipStream_t st, const void *d_src, void *d_dst, uint32_t k, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, const uint8_t *elem, bool inverse)
{
    planes::Table T;
    char why[256] = "";
    if (const int rc = T.make(k, src_off, dst_off, len, elem, planes::kSegment, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (!T.nsegs) return 0;
    DevBuf dt;
    if (const int rc = dt.alloc(T.words.size() * sizeof(unsigned long long))) return rc;
    planes::Args a{};
    a.src = (const uint8_t *)d_src; a.dst = (uint8_t *)d_dst;
    T.point(a, dt.as<unsigned long long>());
    float ms = 0;
    const int rc = timed_launch(st, "planes", &ms,
        [&] { return hipMemcpyAsync(dt.p, T.words.data(), T.words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st); },
        [&] { launch_planes(a, inverse, kStrideBlocks, st); },
        [] { return hipSuccess; });
    if (rc) return rc;
    Last &L = g_last.here();
    L.us += 1000.0 * ms;
    L.bytes += T.bytes;
    return 0;
}

void begin_call() { g_last.here() = Last{}; }

// the ranges of a typed call against their buffer, the element sizes, and the scratch layout: what needs no device
int check_typed(uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem, planes::Layout &lay)
{
    char why[512] = "";
    if (const int rc = planes::check_typed_ranges(n, k, off, len, elem, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (const int rc = lay.make(k, len, planes::kPad, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    return 0;
}

}  // namespace

namespace nlzm {

int planes_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "planes_segment_bytes")) { *value = planes::kSegment; return 0; }      // (no device needed)
    if (!strcmp(key, "planes_us")) { *value = (uint64_t)(g_last.here().us + 0.5); return 0; }
    if (!strcmp(key, "planes_bytes")) { *value = g_last.here().bytes; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

}  // namespace nlzm

extern "C" {

int nlzm_hip_planes_dev(const void *d_src, uint64_t src_len, void *d_dst, uint64_t dst_len, uint32_t k, const uint64_t *src_off, const uint64_t *dst_off,
                        const uint64_t *len, const uint8_t *elem, int inverse)
{
    if (const int rc = check_args(d_src, src_len, d_dst, dst_len, k, src_off, dst_off, len, elem)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    begin_call();
    return planes_on(st, d_src, d_dst, k, src_off, dst_off, len, elem, inverse != 0);
}

int nlzm_hip_planes(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_len, uint32_t k, const uint64_t *src_off, const uint64_t *dst_off,
                    const uint64_t *len, const uint8_t *elem, int inverse)
{
    if (const int rc = check_args(src, src_len, dst, dst_len, k, src_off, dst_off, len, elem)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    begin_call();
    DevBuf ds, dd;
    if (const int rc = dd.alloc(dst_len)) return rc;
    if (const int rc = upload(ds, src, src_len, st)) return rc;
    if (const int rc = planes_on(st, ds.p, dd.p, k, src_off, dst_off, len, elem, inverse != 0)) return rc;
    // only what the ranges wrote comes back: the bytes between them are the caller's
    for (const auto &r : planes::runs(k, dst_off, len)) HIPCHK(hipMemcpyAsync(dst + r.first, dd.as<uint8_t>() + r.first, r.second, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int nlzm_hip_compress_ranges_typed_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem,
                                       uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (all_bytes(k, elem)) return nlzm_hip_compress_ranges_dev(d_src, n, k, off, len, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
    if (!d_dst || !dst_len || (!d_src && n)) return fail(NLZM_HIP_E_ARG, "null argument");
    planes::Layout lay;
    if (const int rc = check_typed(n, k, off, len, elem, lay)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    const uint64_t bound = nlzm_hip_compress_ranges_bound(k, len);
    if (dst_cap < bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)bound);
    begin_call();
    DevBuf scratch;
    if (const int rc = scratch.alloc_for(lay.alloc, "the ranges' byte planes")) return rc;
    HIPCHK(hipMemsetAsync(scratch.as<uint8_t>() + lay.total, 0, planes::kPad, st));
    if (const int rc = planes_on(st, d_src, scratch.p, k, off, lay.at.data(), len, elem, false)) return rc;
    return nlzm_hip_compress_ranges_dev(scratch.p, lay.total, k, lay.at.data(), len, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
}

int nlzm_hip_compress_ranges_typed(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem,
                                   uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (all_bytes(k, elem)) return nlzm_hip_compress_ranges(src, n, k, off, len, hist_bits_req, dst, dst_cap, block_len, dst_len);
    if ((!src && n) || !dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    planes::Layout lay;
    if (const int rc = check_typed(n, k, off, len, elem, lay)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    const uint64_t bound = nlzm_hip_compress_ranges_bound(k, len);
    if (dst_cap < bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)bound);
    DevBuf in, out;
    if (const int rc = out.alloc_for(bound, "the ranges' streams")) return rc;
    if (const int rc = upload(in, src, n, st)) return rc;
    uint64_t got = 0;
    if (const int rc = nlzm_hip_compress_ranges_typed_dev(in.p, n, k, off, len, elem, hist_bits_req, out.p, bound, block_len, &got)) return rc;
    if (got) HIPCHK(hipMemcpy(dst, out.p, got, hipMemcpyDeviceToHost));
    *dst_len = got;
    return 0;
}

int nlzm_hip_decompress_blocks_typed_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                                         const uint8_t *elem, void *d_dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    if (!d_dst || all_bytes(nblocks, elem))         // (a size pass, or nothing to undo: the untyped call itself)
        return nlzm_hip_decompress_blocks_dev(d_src, src_len, nblocks, block_len, raw_len, d_dst, dst_cap, raw_len_out, dst_len);
    char why[256] = "";
    if (const int rc = planes::check_elems(nblocks, elem, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    std::vector<uint64_t> raw(nblocks);
    uint64_t total = 0;
    if (raw_len) memcpy(raw.data(), raw_len, (size_t)nblocks * sizeof(uint64_t));
    else if (const int rc = nlzm_hip_decompress_blocks_dev(d_src, src_len, nblocks, block_len, nullptr, nullptr, 0, raw.data(), &total)) return rc;
    planes::Layout lay;
    if (const int rc = lay.make(nblocks, raw.data(), 0, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (lay.total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the blocks decode to %llu bytes, dst_cap %llu", (unsigned long long)lay.total, (unsigned long long)dst_cap);
    DevBuf scratch;
    if (const int rc = scratch.alloc_for(lay.total, "the blocks' byte planes")) return rc;
    if (const int rc = nlzm_hip_decompress_blocks_dev(d_src, src_len, nblocks, block_len, raw.data(), scratch.p, lay.total, nullptr, &total)) return rc;
    begin_call();
    if (const int rc = planes_on(st, scratch.p, d_dst, nblocks, lay.at.data(), lay.at.data(), raw.data(), elem, true)) return rc;
    if (raw_len_out) memcpy(raw_len_out, raw.data(), (size_t)nblocks * sizeof(uint64_t));
    if (dst_len) *dst_len = total;
    return 0;
}

int nlzm_hip_decompress_blocks_typed(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                                     const uint8_t *elem, uint8_t *dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len)
{
    if (!dst || all_bytes(nblocks, elem))
        return nlzm_hip_decompress_blocks(src, src_len, nblocks, block_len, raw_len, dst, dst_cap, raw_len_out, dst_len);
    char why[256] = "";
    if (const int rc = planes::check_elems(nblocks, elem, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (!src) return fail(NLZM_HIP_E_ARG, "null argument");
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    // the container is split on the host (the hop the untyped call makes), uploaded, sized where no lengths came, and decoded into a buffer of the call's
    std::vector<uint64_t> boff, blen, raw(nblocks);
    if (const int rc = decode_split_host(src, src_len, nblocks, block_len, boff, blen)) return rc;
    DevBuf ds, dd;
    if (const int rc = upload(ds, src, src_len, st)) return rc;
    uint64_t total = 0;
    if (raw_len) memcpy(raw.data(), raw_len, (size_t)nblocks * sizeof(uint64_t));
    else if (const int rc = nlzm_hip_decompress_blocks_dev(ds.p, src_len, nblocks, blen.data(), nullptr, nullptr, 0, raw.data(), &total)) return rc;
    planes::Layout lay;
    if (const int rc = lay.make(nblocks, raw.data(), 0, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (lay.total > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "the blocks decode to %llu bytes, dst_cap %llu", (unsigned long long)lay.total, (unsigned long long)dst_cap);
    if (const int rc = dd.alloc_for(lay.total, "the decoded blocks")) return rc;
    if (const int rc = nlzm_hip_decompress_blocks_typed_dev(ds.p, src_len, nblocks, blen.data(), raw.data(), elem, dd.p, lay.total, nullptr, &total)) return rc;
    if (total) HIPCHK(hipMemcpy(dst, dd.p, total, hipMemcpyDeviceToHost));
    if (raw_len_out) memcpy(raw_len_out, raw.data(), (size_t)nblocks * sizeof(uint64_t));
    if (dst_len) *dst_len = total;
    return 0;
}

}  // extern "C"
