// far_plan_sim.cpp -- the host tables of the range entry points for lengths nobody can allocate: crc::SegTable (nlzm_read_plan.h), planes::check_ranges,
// planes::Table and planes::Layout (nlzm_planes_plan.h), container::make_ranges_plan (nlzm_container_plan.h), dedup::check_ranges (nlzm_dedup_plan.h)
// and units::prefix (nlzm_units.h) -- the headers the library includes -- in a program of its own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY
// (tests/test_far_plan.py, which holds the expected values: Python's integers).
//
//   far_plan_sim <cases>     every case: "T <buf_len> <crc_segment> <planes_segment> <dedup_segment> <k> <off> <len> ... (k pairs)".  Four lines a case:
//       crc    <nsegs> <bytes> <seg0[0]> .. <seg0[k]>                              or   crc    error <code> <text>
//       planes <nsegs> <bytes> <total> <alloc> <seg0[0]> .. <seg0[k]>              or   planes error <code> <text>
//              (range i's element size is 1 << (i % 4); its destination is planes::Layout's at[i] in a buffer of `total` bytes elsewhere)
//       ranges <nsets> <out_bound> <first> <count> <longest> ... (per set)         or   ranges error <code> <bad_range> <text>
//              (set_blocks 32, capacity 64, bound(len) = 16 + 131072 + (len / 14848 + 1) * 16384)
//       dedup  <t[0]> .. <t[k]>                                                    or   dedup  error <code> <text>
#include "../../nlzm_amd/csrc/nlzm_container_plan.h"
#include "../../nlzm_amd/csrc/nlzm_dedup_plan.h"
#include "../../nlzm_amd/csrc/nlzm_planes_plan.h"
#include "../../nlzm_amd/csrc/nlzm_read_plan.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

using namespace nlzm;

namespace {

uint64_t bound(uint64_t n) { return 16 + 131072 + (n / 14848 + 1) * 16384; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: see the head of far_plan_sim.cpp\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        uint64_t buf_len, crc_seg, planes_seg, dedup_seg;
        uint32_t k;
        if (kind[0] != 'T' || fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu32, &buf_len, &crc_seg, &planes_seg, &dedup_seg, &k) != 5 || !k || k > 65536) return 2;
        std::vector<uint64_t> off(k), len(k);
        for (uint32_t i = 0; i < k; i++) if (fscanf(f, "%" SCNu64 " %" SCNu64, &off[i], &len[i]) != 2) return 2;
        char text[512] = "";
        const ErrText err{ text, sizeof text };

        crc::SegTable C;
        if (const int rc = C.make(buf_len, k, off.data(), len.data(), crc_seg, err)) printf("crc error %d %s\n", rc, text);
        else {
            if (C.words.size() != 3 * ((size_t)k + 1)) return 3;
            printf("crc %llu %llu", C.nsegs, C.bytes);
            for (uint32_t i = 0; i <= k; i++) {
                if (i < k && (C.words[i] != off[i] || C.words[(size_t)k + 1 + i] != len[i])) return 3;
                printf(" %llu", C.words[2 * ((size_t)k + 1) + i]);
            }
            printf("\n");
        }

        std::vector<uint8_t> elem(k);
        for (uint32_t i = 0; i < k; i++) elem[i] = (uint8_t)(1u << (i % 4));
        planes::Layout lay;
        planes::Table T;
        int rc = lay.make(k, len.data(), planes::kPad, err);
        // (the two buffers as addresses: the source at 0, the destination right behind it)
        if (!rc) rc = planes::check_ranges(0, buf_len, buf_len, lay.total, k, off.data(), lay.at.data(), len.data(), elem.data(), err);
        if (!rc) rc = T.make(k, off.data(), lay.at.data(), len.data(), elem.data(), planes_seg, err);
        if (rc) printf("planes error %d %s\n", rc, text);
        else {
            printf("planes %llu %llu %" PRIu64 " %" PRIu64, T.nsegs, T.bytes, lay.total, lay.alloc);
            for (uint32_t i = 0; i <= k; i++) printf(" %llu", T.words[4 * (size_t)k + i]);
            printf("\n");
            for (uint32_t i = 0; i < k; i++) if (T.words[i] != off[i] || T.words[(size_t)k + i] != lay.at[i] || T.words[2 * (size_t)k + i] != len[i] || T.words[3 * (size_t)k + i] != elem[i]) return 3;
        }

        container::RangesPlan P;
        if (const int rc2 = container::make_ranges_plan(P, buf_len, k, off.data(), len.data(), 32, 64, bound, err)) printf("ranges error %d %u %s\n", rc2, P.bad_range, text);
        else {
            printf("ranges %zu %" PRIu64, P.sets.size(), P.out_bound);
            for (const auto &s : P.sets) printf(" %u %u %" PRIu64, s.first, s.count, s.longest);
            printf("\n");
        }

        if (const int rc3 = dedup::check_ranges(buf_len, k, off.data(), len.data(), err)) printf("dedup error %d %s\n", rc3, text);
        else {
            printf("dedup");
            for (unsigned long long v : units::prefix(k, dedup_seg, [&](uint32_t i) { return len[i]; })) printf(" %llu", v);
            printf("\n");
        }
    }
    fclose(f);
    printf("far_plan_sim: OK\n");
    return 0;
}
