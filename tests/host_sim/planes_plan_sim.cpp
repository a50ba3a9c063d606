// planes_plan_sim.cpp -- the host plan of the byte-plane filter (nlzm_amd/csrc/nlzm_planes_plan.h) in a program of its own, under AddressSanitizer
// and UBSan.  TEST HARNESS ONLY (tests/test_planes_plan.py).
//
//   planes_plan_sim sweep
//       random range lists: planes::check_ranges against brute force (a bitmap of the destination), the table against its definition, the runs
//       against the bitmap, the layout against a running sum; k = 1 and k = 65,536; lengths that do not sum in 64 bits.
//   planes_plan_sim check <src_at> <src_len> <dst_at> <dst_len> <segment> <ranges>
//       <ranges>: a line `src_off dst_off len elem` per range.  Prints "error <code> <text>", or "ok nsegs <n> bytes <b> runs <r>" and the seg0 table.
#include "../../nlzm_amd/csrc/nlzm_planes_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

using namespace nlzm;

namespace {

[[noreturn]] void die(const char *what) { fprintf(stderr, "planes_plan_sim: %s\n", what); exit(3); }

int sweep()
{
    std::mt19937_64 rng(20261020);
    unsigned long long cases = 0, refused = 0;
    char why[512];
    for (int round = 0; round < 4000; round++) {
        const uint64_t src_len = rng() % 300, dst_len = 1 + rng() % 300, segment = 16 * (1 + rng() % 4);
        const uint32_t k = 1 + (uint32_t)(rng() % 9);
        std::vector<uint64_t> so(k), d0(k), ln(k);
        std::vector<uint8_t> el(k);
        for (uint32_t i = 0; i < k; i++) {
            ln[i] = rng() % 5 ? rng() % 40 : 0;
            so[i] = rng() % (src_len + 2); d0[i] = rng() % (dst_len + 2);
            el[i] = (uint8_t)(rng() % 13 ? 1u << (rng() % 4) : rng() % 11);
        }
        // brute force, in the order the plan reports: elements, then each range against its buffers, then the destinations, then the buffers
        const uint64_t src_at = 4096, dst_at = round % 7 == 3 ? 4096 + rng() % 300 : 8192;
        bool bad = false;
        for (uint32_t i = 0; i < k; i++) if (el[i] != 1 && el[i] != 2 && el[i] != 4 && el[i] != 8) bad = true;
        for (uint32_t i = 0; i < k && !bad; i++) if (so[i] + ln[i] > src_len || d0[i] + ln[i] > dst_len) bad = true;
        if (!bad) {
            std::vector<uint8_t> map(dst_len, 0);
            for (uint32_t i = 0; i < k; i++) for (uint64_t b = 0; b < ln[i]; b++) { if (map[d0[i] + b]) bad = true; map[d0[i] + b] = 1; }
            if (!bad && src_len && dst_len && src_at < dst_at + dst_len && dst_at < src_at + src_len) bad = true;
            if (!bad) {
                // the runs are the bitmap's
                const auto r = planes::runs(k, d0.data(), ln.data());
                std::vector<uint8_t> seen(dst_len, 0);
                for (size_t j = 0; j < r.size(); j++) {
                    if (!r[j].second || (j && r[j - 1].first + r[j - 1].second >= r[j].first)) die("runs: empty, unsorted or touching");
                    for (uint64_t b = 0; b < r[j].second; b++) seen[r[j].first + b] = 1;
                }
                if (seen != map) die("runs: not the destinations");
            }
        }
        why[0] = 0;
        const int rc = planes::check_ranges(src_at, src_len, dst_at, dst_len, k, so.data(), d0.data(), ln.data(), el.data(), ErrText{ why, sizeof why });
        if ((rc != 0) != bad) die("check_ranges disagrees with brute force");
        if (rc && (rc != NLZM_HIP_E_ARG || !why[0])) die("an error without its code or text");
        cases++;
        if (rc) { refused++; continue; }
        planes::Table T;
        if (T.make(k, so.data(), d0.data(), ln.data(), el.data(), segment, ErrText{ why, sizeof why })) die("table refused");
        struct { const unsigned long long *src_off, *dst_off, *len, *elem, *seg0; uint32_t k; unsigned long long nsegs; } a{};
        T.point(a, T.words.data());
        unsigned long long segs = 0, bytes = 0;
        if (T.words.size() != 5 * (size_t)k + 1 || a.k != k) die("table size");
        for (uint32_t i = 0; i < k; i++) {
            if (a.src_off[i] != so[i] || a.dst_off[i] != d0[i] || a.len[i] != ln[i] || a.elem[i] != el[i] || a.seg0[i] != segs) die("table entry");
            segs += (ln[i] + segment - 1) / segment; bytes += ln[i];
        }
        if (a.seg0[k] != segs || a.nsegs != segs || T.bytes != bytes) die("table totals");
        planes::Layout L;
        if (L.make(k, ln.data(), 128, ErrText{ why, sizeof why }) || L.total != bytes || L.alloc != bytes + 128) die("layout");
        uint64_t at = 0;
        for (uint32_t i = 0; i < k; i++) { if (L.at[i] != at) die("layout entry"); at += ln[i]; }
    }
    if (refused < 100 || cases - refused < 100) die("the sweep is one-sided");
    {   // the edges of k, a null table, sums that wrap
        std::vector<uint64_t> z(65537, 0), d(65537, 0), l(65537, 1);
        std::vector<uint8_t> e(65537, 2);
        for (uint32_t i = 0; i < 65537; i++) d[i] = i;
        const ErrText err{ why, sizeof why };
        if (planes::check_ranges(0, 8, 4096, 65537, 0, z.data(), d.data(), l.data(), e.data(), err) != NLZM_HIP_E_ARG) die("k = 0");
        if (planes::check_ranges(0, 8, 4096, 65537, 65537, z.data(), d.data(), l.data(), e.data(), err) != NLZM_HIP_E_ARG) die("k = 65537");
        if (planes::check_ranges(0, 8, 4096, 65537, 65536, z.data(), d.data(), l.data(), e.data(), err) != 0) die("k = 65536");
        if (planes::check_ranges(0, 8, 4096, 65537, 1, z.data(), d.data(), l.data(), e.data(), err) != 0) die("k = 1");
        if (planes::check_ranges(0, 8, 4096, 65537, 1, nullptr, d.data(), l.data(), e.data(), err) != NLZM_HIP_E_ARG) die("null src_off");
        if (planes::check_ranges(0, 8, 4096, 65537, 1, z.data(), d.data(), l.data(), nullptr, err) != NLZM_HIP_E_ARG) die("null elem");
        const uint64_t huge[2] = { ~0ull - 100, 200 }, wrap_off[2] = { ~0ull, 0 }, two[2] = { 2, 2 };
        const uint8_t e2[2] = { 4, 4 };
        planes::Layout L;
        if (L.make(2, huge, 128, err) != NLZM_HIP_E_ARG || L.make(2, huge, 0, err) != NLZM_HIP_E_ARG) die("a sum that wraps");
        if (planes::check_ranges(0, 100, 4096, 100, 2, wrap_off, z.data(), two, e2, err) != NLZM_HIP_E_ARG || !strstr(why, "range 0 ")) die("an offset that wraps");
        // the typed calls' check: one buffer, the ranges may overlap
        const uint64_t in_off[2] = { 98, 0 }, over_off[2] = { 0, 99 };
        if (planes::check_typed_ranges(100, 2, in_off, two, e2, err) != 0) die("typed ranges inside their buffer");
        if (planes::check_typed_ranges(100, 2, over_off, two, e2, err) != NLZM_HIP_E_ARG || !strstr(why, "range 1 (offset 99, 2 bytes) runs over the 100 bytes of the buffer")) die("a typed range over its buffer's end");
        if (planes::check_typed_ranges(100, 2, wrap_off, two, e2, err) != NLZM_HIP_E_ARG || !strstr(why, "range 0 ")) die("a typed offset that wraps");
        if (planes::check_typed_ranges(100, 2, in_off, two, nullptr, err) != NLZM_HIP_E_ARG || planes::check_typed_ranges(100, 2, nullptr, two, e2, err) != NLZM_HIP_E_ARG) die("typed: null");
    }
    printf("sweep: cases=%llu refused=%llu\n", cases, refused);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        if (sweep()) return 3;
        printf("planes_plan_sim: OK\n");
        return 0;
    }
    if (argc != 8 || strcmp(argv[1], "check")) { fprintf(stderr, "usage: see the head of planes_plan_sim.cpp\n"); return 2; }
    const uint64_t src_at = strtoull(argv[2], nullptr, 10), src_len = strtoull(argv[3], nullptr, 10), dst_at = strtoull(argv[4], nullptr, 10), dst_len = strtoull(argv[5], nullptr, 10);
    const uint64_t segment = strtoull(argv[6], nullptr, 10);
    FILE *f = fopen(argv[7], "r");
    if (!f) return 2;
    std::vector<uint64_t> so, d0, ln;
    std::vector<uint8_t> el;
    unsigned long long a, b, c, e;
    while (fscanf(f, "%llu %llu %llu %llu", &a, &b, &c, &e) == 4) { so.push_back(a); d0.push_back(b); ln.push_back(c); el.push_back((uint8_t)e); }
    fclose(f);
    char why[512] = "";
    const uint32_t k = (uint32_t)so.size();
    int rc = planes::check_ranges(src_at, src_len, dst_at, dst_len, k, so.data(), d0.data(), ln.data(), el.data(), ErrText{ why, sizeof why });
    planes::Table T;
    if (!rc) rc = T.make(k, so.data(), d0.data(), ln.data(), el.data(), segment, ErrText{ why, sizeof why });
    if (rc) printf("error %d %s\n", rc, why);
    else {
        printf("ok nsegs %llu bytes %llu runs %zu\n", T.nsegs, T.bytes, planes::runs(k, d0.data(), ln.data()).size());
        for (uint32_t i = 0; i <= k; i++) printf("%llu%s", T.words[4 * (size_t)k + i], i < k ? " " : "\n");
    }
    printf("planes_plan_sim: OK\n");
    return 0;
}
