// nlzm_hip_dedup.cpp -- host side of the equal-range finder: the nlzm_hip_equal_ranges* entry points of include/nlzm_hip.h, and what the compress
// path calls when "dedup_ranges" is set.  Kernels: nlzm_dedup.hip; the roles they run and the fingerprint's rule: nlzm_dedup.h; the classes, made
// here on the host from the fingerprints and the pair role's verdicts: nlzm_dedup_plan.h.  Uses the library's device, stream and error text
// (nlzm_hip.cpp) as the cut points' host side does, the range reader's gather launch (nlzm_range.hip), and nothing else of the compress pipeline.
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "nlzm_host_util.h"
#include "nlzm_dedup_host.h"
#include "nlzm_dedup.h"
#include "nlzm_dedup_plan.h"
#include "nlzm_range.h"

using namespace nlzm;

namespace {

// what nlzm_hip_get_counter("dedup_*") reports of the last call
struct Last {
    unsigned long long distinct = 0, dup_bytes = 0, rounds = 0, pairs = 0, compared_bytes = 0;
    double us = 0, gather_us = 0;
};
PerDevice<Last> g_last;

// the two options: the process's, like the library's error text (a multi-device call compresses no ranges)
std::atomic<int64_t> g_dedup_ranges{ 0 }, g_hash_bits{ 64 };

// the arguments that need no device
int check_args(uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, const uint32_t *first_of)
{
    char why[512] = "";
    if (const int rc = dedup::check_ranges(buf_len, k, off, len, ErrText{ why, sizeof why })) return fail(rc, "%s", why);
    if (!first_of) return fail(NLZM_HIP_E_ARG, "null argument");
    return 0;
}

// one round's pairs on the device: equal[p] for every pair
int compare_pairs(hipStream_t st, const void *d_buf, const uint64_t *off, const uint64_t *len, const std::vector<dedup::IndexPair> &pairs, std::vector<uint8_t> &equal, double *us)
{
    const size_t np = pairs.size();
    if (!np) return 0;
    std::vector<dedup::Pair> hp(np);
    for (size_t p = 0; p < np; p++) hp[p] = dedup::Pair{ off[pairs[p].rep], off[pairs[p].member], len[pairs[p].rep] };
    const std::vector<unsigned long long> c0 = units::prefix((uint32_t)np, dedup::kChunk, [&](uint32_t p) { return hp[p].len; });
    DevBuf dp, dc, dn, de;
    int rc = dp.alloc(np * sizeof(dedup::Pair));
    if (!rc) rc = dc.alloc((np + 1) * sizeof(unsigned long long));
    if (!rc) rc = dn.alloc((size_t)c0[np] * sizeof(uint32_t));
    if (!rc) rc = de.alloc(np * sizeof(uint32_t));
    if (rc) return rc;
    const dedup::PairArgs a{ (const uint8_t *)d_buf, dp.as<dedup::Pair>(), dc.as<unsigned long long>(), dn.as<uint32_t>(), de.as<uint32_t>(), (uint32_t)np, c0[np] };
    std::vector<uint32_t> got(np, 0);
    float ms = 0;
    rc = timed_launch(st, "dedup pairs", &ms,
        [&] {
            const hipError_t e = hipMemcpyAsync(dp.p, hp.data(), np * sizeof(dedup::Pair), hipMemcpyHostToDevice, st);
            return e != hipSuccess ? e : hipMemcpyAsync(dc.p, c0.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
        },
        [&] { launch_pairs(a, kStrideBlocks, st); },
        [&] { return hipMemcpyAsync(got.data(), de.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st); });
    if (rc) return rc;
    *us += 1000.0 * ms;
    for (size_t p = 0; p < np; p++) equal[p] = got[p] != 0;
    return 0;
}

// first_of and the fingerprints (may be nullptr) of k checked ranges of the bytes at d_buf, on stream st.  Device memory: three words a range and one
// a segment for the fingerprints; per round a pair's record, two words a pair and one a chunk.
int equal_ranges_on(hipStream_t st, const void *d_buf, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t *first_of, uint64_t *fingerprint)
{
    Last &L = g_last.here();
    L = Last{};
    uint64_t total = 0;
    for (uint32_t i = 0; i < k; i++) total += len[i];
    if (total && !d_buf) return fail(NLZM_HIP_E_ARG, "null argument");
    const std::vector<unsigned long long> seg0 = units::prefix(k, dedup::kSegment, [&](uint32_t i) { return len[i]; });
    std::vector<unsigned long long> table(3 * (size_t)k + 1);      // off, len, seg0: one upload
    for (uint32_t i = 0; i < k; i++) { table[i] = off[i]; table[(size_t)k + i] = len[i]; }
    memcpy(table.data() + 2 * (size_t)k, seg0.data(), ((size_t)k + 1) * sizeof(unsigned long long));
    DevBuf dt, ds, df;
    int rc = dt.alloc(table.size() * sizeof(unsigned long long));
    if (!rc) rc = ds.alloc((size_t)seg0[k] * sizeof(unsigned long long));
    if (!rc) rc = df.alloc((size_t)k * sizeof(unsigned long long));
    if (rc) return rc;
    const unsigned long long *t = dt.as<unsigned long long>();
    const dedup::FpArgs a{ (const uint8_t *)d_buf, t, t + k, t + 2 * (size_t)k, ds.as<unsigned long long>(), df.as<unsigned long long>(), k, seg0[k] };
    std::vector<uint64_t> fp(k, 0);
    float ms = 0;
    rc = timed_launch(st, "dedup fingerprints", &ms,
        [&] { return hipMemcpyAsync(dt.p, table.data(), table.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st); },
        [&] { launch_fingerprints(a, kStrideBlocks, st); },
        [&] { return hipMemcpyAsync(fp.data(), df.p, (size_t)k * sizeof(uint64_t), hipMemcpyDeviceToHost, st); });
    if (rc) return rc;
    L.us += 1000.0 * ms;
    if (fingerprint) memcpy(fingerprint, fp.data(), (size_t)k * sizeof(uint64_t));
    dedup::Classes R;
    rc = dedup::class_plan(R, k, off, len, fp.data(), (uint32_t)g_hash_bits.load(),
        [&](const std::vector<dedup::IndexPair> &pairs, std::vector<uint8_t> &equal) { return compare_pairs(st, d_buf, off, len, pairs, equal, &L.us); });
    if (rc) return rc;
    memcpy(first_of, R.first_of.data(), (size_t)k * sizeof(uint32_t));
    L.distinct = R.distinct; L.dup_bytes = R.dup_bytes; L.rounds = R.rounds; L.pairs = R.pairs; L.compared_bytes = R.compared_bytes;
    return 0;
}

}  // namespace

namespace nlzm {

int dedup_counter(const char *key, uint64_t *value)
{
    if (!strcmp(key, "dedup_segment_bytes")) { *value = dedup::kSegment; return 0; }        // (no device needed)
    if (!strcmp(key, "dedup_ranges")) { *value = (uint64_t)g_dedup_ranges.load(); return 0; }      // (the option as it stands, for a caller that sets and restores it)
    const Last &L = g_last.here();
    static const struct { const char *name; unsigned long long Last::*m; } kInt[] = {
        { "dedup_distinct", &Last::distinct }, { "dedup_dup_bytes", &Last::dup_bytes }, { "dedup_rounds", &Last::rounds }, { "dedup_pairs", &Last::pairs },
        { "dedup_compared_bytes", &Last::compared_bytes },
    };
    for (const auto &e : kInt) if (!strcmp(key, e.name)) { *value = L.*(e.m); return 0; }
    if (!strcmp(key, "dedup_us")) { *value = (uint64_t)(L.us + 0.5); return 0; }
    if (!strcmp(key, "dedup_gather_us")) { *value = (uint64_t)(L.gather_us + 0.5); return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

int dedup_set_option(const char *key, int64_t value)
{
    if (!strcmp(key, "dedup_ranges")) {
        if (value < 0 || value > 1) return fail(NLZM_HIP_E_ARG, "%s out of range", key);
        g_dedup_ranges = value;
        return 0;
    }
    if (!strcmp(key, "test_dedup_hash_bits")) {
        if (value < 0 || value > 64) return fail(NLZM_HIP_E_ARG, "%s out of range", key);
        g_hash_bits = value;
        return 0;
    }
    return 1;
}

bool dedup_ranges_option() { return g_dedup_ranges.load() != 0; }

int dedup_first_of(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t *first_of)
{
    if (const int rc = check_args(buf_len, k, off, len, first_of)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    return equal_ranges_on(st, d_buf, k, off, len, first_of, nullptr);
}

int dedup_place(const uint8_t *d_from, uint8_t *d_to, uint32_t k, const uint64_t *from, const uint64_t *to, const uint64_t *len)
{
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    std::vector<range::Piece> hp;
    for (uint32_t i = 0; i < k; i++) if (len[i]) hp.push_back(range::Piece{ d_from + from[i], d_to + to[i], len[i] });
    return gather_on(st, "dedup gather", hp, &g_last.here().gather_us);
}

}  // namespace nlzm

extern "C" {

int nlzm_hip_equal_ranges_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t *first_of, uint64_t *fingerprint)
{
    if (const int rc = check_args(buf_len, k, off, len, first_of)) return rc;
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    return equal_ranges_on(st, d_buf, k, off, len, first_of, fingerprint);
}

int nlzm_hip_equal_ranges(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t *first_of, uint64_t *fingerprint)
{
    if (const int rc = check_args(buf_len, k, off, len, first_of)) return rc;
    if (!buf && buf_len) return fail(NLZM_HIP_E_ARG, "null argument");
    hipStream_t st;
    if (const int rc = host_stream(&st)) return rc;
    DevBuf d;
    if (const int rc = upload(d, buf, buf_len, st)) return rc;
    return equal_ranges_on(st, d.p, k, off, len, first_of, fingerprint);
}

}  // extern "C"
