// elem_plan_sim.cpp -- the host plan of the element-size statistic (nlzm_amd/csrc/nlzm_elem_plan.h) in a program of its own, under AddressSanitizer
// and UBSan.  TEST HARNESS ONLY (tests/test_elem_plan.py).
//
//   elem_plan_sim sweep
//       random range lists: elem::check_ranges against brute force, the table and the scratch against their definitions; elem::choose against a
//       restatement in 128-bit integers over random and near-tie costs; k = 1 and k = 65,536; offsets that wrap; lengths round 2^40.
//   elem_plan_sim check <buf_len> <segment> <hist> <ranges>
//       <ranges>: a line `off len` per range.  Prints "error <code> <text>", or "ok nsegs <n> nwide <w> slots <s> scratch <bytes>", the seg0 table, the
//       slots ("-" for none) and the ranges of more than one segment.
//   elem_plan_sim choose <C_1> <C_2> <C_4> <C_8> <len>     prints the choice
#include "../../nlzm_amd/csrc/nlzm_elem_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

using namespace nlzm;

namespace {

[[noreturn]] void die(const char *what) { fprintf(stderr, "elem_plan_sim: %s\n", what); exit(3); }

// the rule as the issue words it, in integers that cannot wrap
uint32_t choose_brute(const uint64_t *c, uint64_t len)
{
    if (len < 4096) return 1;
    const uint32_t es[4] = { 1, 2, 4, 8 };
    uint32_t best = 0;
    for (uint32_t i = 0; i < 4; i++) {
        bool smaller_or_tie_with_smaller_e = true;
        for (uint32_t j = 0; j < 4; j++) if (c[j] < c[i] || (c[j] == c[i] && j < i)) smaller_or_tie_with_smaller_e = false;
        if (smaller_or_tie_with_smaller_e) best = i;
    }
    if (es[best] != 1 && (unsigned __int128)c[best] + c[0] / 32 > (unsigned __int128)c[0]) return 1;
    return es[best];
}

int sweep()
{
    std::mt19937_64 rng(20261021);
    unsigned long long cases = 0, refused = 0, chosen[9] = { 0 };
    char why[512];
    for (int round = 0; round < 4000; round++) {
        const uint64_t n = rng() % 3000, segment = 16 * (1 + rng() % 8);
        const uint32_t k = 1 + (uint32_t)(rng() % 9);
        const bool hist = rng() % 2;
        std::vector<uint64_t> off(k), len(k);
        for (uint32_t i = 0; i < k; i++) { len[i] = rng() % 5 ? rng() % 600 : 0; off[i] = rng() % (n + 2); }
        bool bad = false;
        for (uint32_t i = 0; i < k; i++) if (off[i] + len[i] > n) bad = true;
        why[0] = 0;
        const int rc = elem::check_ranges(n, k, off.data(), len.data(), ErrText{ why, sizeof why });
        if ((rc != 0) != bad) die("check_ranges disagrees with brute force");
        if (rc && (rc != NLZM_HIP_E_ARG || !strstr(why, "range "))) die("an error without its code or its range");
        cases++;
        if (rc) { refused++; continue; }
        elem::Table T;
        T.make(k, off.data(), len.data(), segment, hist);
        struct { const unsigned long long *off, *len, *slot, *seg0, *wide; uint32_t k, nwide; unsigned long long nsegs; } a{};
        T.point(a, T.words.data());
        unsigned long long segs = 0, bytes = 0;
        uint32_t wide = 0;
        for (uint32_t i = 0; i < k; i++) {
            const unsigned long long mine = (len[i] / 8 * 8 + segment - 1) / segment;
            if (a.off[i] != off[i] || a.len[i] != len[i] || a.seg0[i] != segs) die("table entry");
            if (a.slot[i] != (hist ? i : mine > 1 ? wide : elem::kNoSlot)) die("table slot");
            if (mine > 1) { if (wide >= a.nwide || a.wide[wide] != i) die("table wide"); wide++; }
            segs += mine; bytes += len[i];
        }
        if (a.k != k || a.nwide != wide || a.seg0[k] != segs || a.nsegs != segs || T.bytes != bytes || T.nslots != (hist ? k : wide)) die("table totals");
        if (T.words.size() != 4 * (size_t)k + 1 + wide) die("table size");
        const elem::Scratch S(T);
        if (S.table != 8 * T.words.size() || S.cost != 32ull * k || S.totals != T.nslots * 16384 || S.bytes() != S.table + S.cost + S.totals) die("scratch");
    }
    if (refused < 100 || cases - refused < 100) die("the sweep is one-sided");
    // the choice: random costs of every magnitude, ties, and costs within a few units of the 1/32 boundary
    for (int round = 0; round < 200000; round++) {
        uint64_t c[4];
        const unsigned shift = rng() % 60;
        for (auto &v : c) v = (rng() >> 4) >> shift;
        if (round % 3 == 0) c[1 + rng() % 3] = c[rng() % 4];
        if (round % 5 == 0) { const uint32_t i = 1 + rng() % 3; c[i] = c[0] - c[0] / 32 + rng() % 5 - 2; if (c[i] > c[0]) c[i] = c[0]; }
        const uint64_t len = round % 7 ? 4096 + rng() % 100000 : rng() % 4097;
        const uint32_t got = elem::choose(c, len);
        if (got != choose_brute(c, len)) die("choose disagrees with brute force");
        chosen[got]++;
    }
    for (uint32_t e : { 1u, 2u, 4u, 8u }) if (chosen[e] < 1000) die("the choices are one-sided");
    {   // the edges of k, nulls, an offset that wraps, lengths round 2^40
        std::vector<uint64_t> z(65537, 0), l(65537, 1);
        const ErrText err{ why, sizeof why };
        if (elem::check_ranges(8, 0, z.data(), l.data(), err) != NLZM_HIP_E_ARG) die("k = 0");
        if (elem::check_ranges(8, 65537, z.data(), l.data(), err) != NLZM_HIP_E_ARG) die("k = 65537");
        if (elem::check_ranges(8, 65536, z.data(), l.data(), err) != 0) die("k = 65536");
        if (elem::check_ranges(8, 1, z.data(), l.data(), err) != 0) die("k = 1");
        if (elem::check_ranges(8, 1, nullptr, l.data(), err) != NLZM_HIP_E_ARG || elem::check_ranges(8, 1, z.data(), nullptr, err) != NLZM_HIP_E_ARG) die("null");
        const uint64_t wrap_off[2] = { 0, ~0ull }, two[2] = { 2, 2 };
        if (elem::check_ranges(100, 2, wrap_off, two, err) != NLZM_HIP_E_ARG || !strstr(why, "range 1 ")) die("an offset that wraps");
        const uint64_t o2[2] = { 0, 5 }, just[2] = { 1, (1ull << 40) - 1 }, over[2] = { 1, 1ull << 40 };
        if (elem::check_ranges(1ull << 41, 2, o2, just, err) != 0) die("a range of 2^40 - 1 bytes");
        if (elem::check_ranges(1ull << 41, 2, o2, over, err) != NLZM_HIP_E_ARG || !strstr(why, "range 1 ") || !strstr(why, "2^40")) die("a range of 2^40 bytes");
        elem::Table T;
        T.make(2, o2, just, 65536, false);
        if (T.nsegs != 1 + ((1ull << 40) - 8) / 65536 || T.nwide != 1 || T.words[2 * 2 + 0] != elem::kNoSlot || T.words[2 * 2 + 1] != 0) die("the table of a long range");
    }
    printf("sweep: cases=%llu refused=%llu\n", cases, refused);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        if (sweep()) return 3;
        printf("elem_plan_sim: OK\n");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "choose")) {
        uint64_t c[4];
        for (int i = 0; i < 4; i++) c[i] = strtoull(argv[2 + i], nullptr, 10);
        printf("%u\nelem_plan_sim: OK\n", elem::choose(c, strtoull(argv[6], nullptr, 10)));
        return 0;
    }
    if (argc != 6 || strcmp(argv[1], "check")) { fprintf(stderr, "usage: see the head of elem_plan_sim.cpp\n"); return 2; }
    const uint64_t n = strtoull(argv[2], nullptr, 10), segment = strtoull(argv[3], nullptr, 10);
    const bool hist = atoi(argv[4]) != 0;
    FILE *f = fopen(argv[5], "r");
    if (!f) return 2;
    std::vector<uint64_t> off, len;
    unsigned long long a, b;
    while (fscanf(f, "%llu %llu", &a, &b) == 2) { off.push_back(a); len.push_back(b); }
    fclose(f);
    char why[512] = "";
    const uint32_t k = (uint32_t)off.size();
    const int rc = elem::check_ranges(n, k, off.data(), len.data(), ErrText{ why, sizeof why });
    if (rc) printf("error %d %s\n", rc, why);
    else {
        elem::Table T;
        T.make(k, off.data(), len.data(), segment, hist);
        printf("ok nsegs %llu nwide %u slots %llu scratch %llu\n", T.nsegs, T.nwide, T.nslots, (unsigned long long)elem::Scratch(T).bytes());
        for (uint32_t i = 0; i <= k; i++) printf("%llu%s", T.words[3 * (size_t)k + i], i < k ? " " : "\n");
        for (uint32_t i = 0; i < k; i++) { if (T.words[2 * (size_t)k + i] == elem::kNoSlot) printf("-"); else printf("%llu", T.words[2 * (size_t)k + i]); printf("%s", i + 1 < k ? " " : "\n"); }
        for (uint32_t i = 0; i < T.nwide; i++) printf("%llu%s", T.words[4 * (size_t)k + 1 + i], i + 1 < T.nwide ? " " : "");
        printf("\n");
    }
    printf("elem_plan_sim: OK\n");
    return 0;
}
