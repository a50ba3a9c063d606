// ranges_plan_sim.cpp -- the plan of a call on ranges of the caller's choosing (nlzm_amd/csrc/nlzm_container_plan.h, make_ranges_plan) on its own: no
// device, no library.  TEST HARNESS ONLY (tests/test_ranges_plan.py; built by the Makefile with -fsanitize=address,undefined).
//
//   ranges_plan_sim sweep                                    the fixed cases, checked here; one summary line
//   ranges_plan_sim plan <n> <set_blocks> <capacity> <file>  one plan from the "off len" lines of <file>, printed:
//                                                            "sets S out_bound B" and a line "set first count longest" per set, or "error code text"
//   ranges_plan_sim equal <n> <nblocks> <set_blocks> <capacity>   the equal partition's ranges through make_ranges_plan, held to make_plan's sets
#include "../../nlzm_amd/csrc/nlzm_container_plan.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace nlzm;

namespace {

// the library's bound (nlzm_hip_compress_bound; the plan takes it as a parameter so that this file links nothing)
uint64_t bound(uint64_t n) { return 16 + 131072 + (n / 14848 + 1) * 16384; }

#define FAIL(...) do { printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

// what every plan that was made must hold
int check(const container::RangesPlan &P, uint64_t n, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, uint32_t set_blocks, uint32_t capacity)
{
    const uint32_t k = (uint32_t)off.size();
    if (P.k != k) FAIL("k %u", P.k);
    const size_t nsets = P.sets.size();
    if (k <= capacity ? nsets != 1 : nsets != (k + set_blocks - 1) / set_blocks) FAIL("%zu sets for %u ranges by %u at a capacity of %u", nsets, k, set_blocks, capacity);
    uint32_t at = 0, lo_count = ~0u, hi_count = 0;
    uint64_t sum = 0;
    for (size_t s = 0; s < nsets; s++) {
        const container::RangeSet &S = P.sets[s];
        if (S.first != at || !S.count || S.count > capacity || (nsets > 1 && S.count > set_blocks)) FAIL("set %zu: first %u count %u", s, S.first, S.count);
        uint64_t longest = 0;
        for (uint32_t i = S.first; i < S.first + S.count; i++) {
            if (off[i] > n || len[i] > n - off[i]) FAIL("range %u was accepted", i);
            longest = len[i] > longest ? len[i] : longest;
            sum += bound(len[i]);
        }
        if (S.longest != longest) FAIL("set %zu: longest %" PRIu64 ", its ranges say %" PRIu64, s, S.longest, longest);
        lo_count = S.count < lo_count ? S.count : lo_count; hi_count = S.count > hi_count ? S.count : hi_count;
        if (s && S.count > P.sets[s - 1].count) FAIL("a larger set behind a smaller one");
        at += S.count;
    }
    if (at != k || hi_count - lo_count > 1) FAIL("%u ranges in the sets, sizes %u .. %u", at, lo_count, hi_count);
    if (P.out_bound != sum) FAIL("out_bound %" PRIu64 ", the ranges' bounds sum to %" PRIu64, P.out_bound, sum);
    return 0;
}

int make_and_check(uint64_t n, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, uint32_t set_blocks, uint32_t capacity, container::RangesPlan &P)
{
    char text[512] = "";
    const int rc = container::make_ranges_plan(P, n, (uint32_t)off.size(), off.data(), len.data(), set_blocks, capacity, bound, ErrText{ text, sizeof text });
    if (rc) FAIL("rc %d (%s)", rc, text);
    return check(P, n, off, len, set_blocks, capacity);
}

int cmd_sweep()
{
    container::RangesPlan P;
    char text[512] = "";
    const ErrText err{ text, sizeof text };
    unsigned ran = 0;
    // k <= capacity: one set, whatever set_blocks says
    for (uint32_t k : { 1u, 9u, 63u, 64u }) for (uint32_t sb : { 1u, 7u, 32u, 64u }) {
        std::vector<uint64_t> off(k), len(k);
        for (uint32_t i = 0; i < k; i++) { off[i] = (i * 7919u) % 1000; len[i] = (i * 104729u) % (1000 - off[i] + 1); }
        if (make_and_check(1000, off, len, sb, 64, P) || P.sets.size() != 1 || P.sets[0].count != k) FAIL("%u ranges are one set", k);
        ran++;
    }
    // 65 ranges by 32: 22 + 22 + 21; 65,536 ranges by 32: 2,048 sets of 32; in any order, overlapping, repeated, empty
    {
        std::vector<uint64_t> off(65), len(65);
        for (uint32_t i = 0; i < 65; i++) { off[i] = (64 - i) * 10; len[i] = i % 3 ? 25 : 0; }
        len[40] = 300; len[41] = 300; off[41] = off[40];
        if (make_and_check(1000, off, len, 32, 64, P) || P.sets.size() != 3 || P.sets[0].count != 22 || P.sets[1].count != 22 || P.sets[2].count != 21) FAIL("65 by 32");
        if (P.sets[0].longest != 25 || P.sets[1].longest != 300 || P.sets[2].longest != 25) FAIL("65 by 32: the longest ranges");
        if (make_and_check(1000, off, len, 64, 64, P) || P.sets.size() != 2 || P.sets[0].count != 33 || P.sets[1].count != 32) FAIL("65 by 64");
        if (make_and_check(1000, off, len, 7, 16, P) || P.sets.size() != 10) FAIL("65 by 7");
        ran += 3;
    }
    {
        std::vector<uint64_t> off(65536), len(65536);
        for (uint32_t i = 0; i < 65536; i++) { off[i] = i; len[i] = (i * 31u) % 97; }
        if (make_and_check(65536 + 96, off, len, 32, 64, P) || P.sets.size() != 2048) FAIL("65,536 by 32");
        for (const container::RangeSet &S : P.sets) if (S.count != 32) FAIL("65,536 by 32: a set of %u", S.count);
        ran++;
    }
    // empty ranges only, at the start, inside and at the very end of the input, and of an empty input
    for (uint64_t n : { (uint64_t)0, (uint64_t)1000 }) for (uint32_t k : { 1u, 64u, 70u }) {
        std::vector<uint64_t> off(k), len(k, 0);
        for (uint32_t i = 0; i < k; i++) off[i] = n ? (i % 3 == 0 ? 0 : i % 3 == 1 ? n : i) : 0;
        if (make_and_check(n, off, len, 32, 64, P)) return 1;
        for (const container::RangeSet &S : P.sets) if (S.longest) FAIL("empty ranges have a longest one");
        if (P.out_bound != (uint64_t)k * bound(0)) FAIL("the bound of %u empty streams", k);
        ran++;
    }
    // a range that runs over n: refused and named, also where off + len wraps
    {
        const uint64_t n = 1000;
        const struct { uint64_t off, len; } bad[] = { { 0, 1001 }, { 1000, 1 }, { 1001, 0 }, { 500, 501 }, { ~0ull, 2 }, { 2, ~0ull }, { ~0ull - 5, 10 } };
        for (const auto &b : bad) for (uint32_t where : { 0u, 3u, 69u }) {
            std::vector<uint64_t> off(70, 10), len(70, 10);
            off[where] = b.off; len[where] = b.len;
            text[0] = 0;
            const int rc = container::make_ranges_plan(P, n, 70, off.data(), len.data(), 32, 64, bound, err);
            char want[32];
            snprintf(want, sizeof want, "range %u ", where);
            if (rc != NLZM_HIP_E_ARG || P.bad_range != where || !strstr(text, want) || !P.sets.empty()) FAIL("range %u = (%" PRIu64 ", %" PRIu64 ") over n: rc %d, text '%s'", where, b.off, b.len, rc, text);
            ran++;
        }
        std::vector<uint64_t> off{ 0, 1000, 999, 0 }, len{ 1000, 0, 1, 0 };      // (the edges that are inside)
        if (make_and_check(n, off, len, 32, 64, P)) return 1;
    }
    // a bound sum that would wrap: two ranges of 2^63 bytes and more
    {
        std::vector<uint64_t> off{ 0, 0, 0 }, len{ 1ull << 63, 1ull << 63, 1ull << 63 };       // (each one's own bound still fits)
        if (container::make_ranges_plan(P, ~0ull, 3, off.data(), len.data(), 32, 64, bound, err) != NLZM_HIP_E_ARG || !strstr(text, "sum")) FAIL("bounds that do not sum in 64 bits were summed");
        uint64_t sum = 1;
        if (container::ranges_bound(3, len.data(), bound, sum) || container::ranges_bound(0, len.data(), bound, sum) || container::ranges_bound(65537, len.data(), bound, sum)) FAIL("ranges_bound");
        std::vector<uint64_t> one{ 1ull << 62 };
        if (!container::ranges_bound(1, one.data(), bound, sum) || sum != bound(1ull << 62)) FAIL("ranges_bound of one range");
        ran++;
    }
    // what the plan refuses
    {
        std::vector<uint64_t> off(70, 0), len(70, 1);
        if (container::make_ranges_plan(P, 100, 0, off.data(), len.data(), 32, 64, bound, err) != NLZM_HIP_E_ARG || container::make_ranges_plan(P, 100, 65537, off.data(), len.data(), 32, 64, bound, err) != NLZM_HIP_E_ARG ||
            container::make_ranges_plan(P, 100, 70, off.data(), len.data(), 0, 64, bound, err) != NLZM_HIP_E_ARG || container::make_ranges_plan(P, 100, 70, off.data(), len.data(), 32, 0, bound, err) != NLZM_HIP_E_ARG ||
            container::make_ranges_plan(P, 100, 70, off.data(), len.data(), 65, 64, bound, err) != NLZM_HIP_E_ARG || container::make_ranges_plan(P, 100, 70, nullptr, len.data(), 32, 64, bound, err) != NLZM_HIP_E_ARG ||
            container::make_ranges_plan(P, 100, 70, off.data(), nullptr, 32, 64, bound, err) != NLZM_HIP_E_ARG)
            FAIL("a plan that must be refused was made");
        ran++;
    }
    printf("sweep: cases=%u\n", ran);
    printf("ranges_plan_sim: OK\n");
    return 0;
}

int cmd_plan(char **argv)
{
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const uint32_t set_blocks = (uint32_t)strtoul(argv[3], nullptr, 10), capacity = (uint32_t)strtoul(argv[4], nullptr, 10);
    std::vector<uint64_t> off, len;
    FILE *f = fopen(argv[5], "r");
    if (!f) return 2;
    unsigned long long o, l;
    while (fscanf(f, "%llu %llu", &o, &l) == 2) { off.push_back(o); len.push_back(l); }
    fclose(f);
    container::RangesPlan P;
    char text[512] = "";
    const int rc = container::make_ranges_plan(P, n, (uint32_t)off.size(), off.data(), len.data(), set_blocks, capacity, bound, ErrText{ text, sizeof text });
    if (rc) { printf("error %d %s\n", rc, text); printf("ranges_plan_sim: OK\n"); return 0; }
    if (check(P, n, off, len, set_blocks, capacity)) return 1;
    printf("sets %zu out_bound %" PRIu64 "\n", P.sets.size(), P.out_bound);
    for (const container::RangeSet &S : P.sets) printf("set %u %u %" PRIu64 "\n", S.first, S.count, S.longest);
    printf("ranges_plan_sim: OK\n");
    return 0;
}

// the equal partition's ranges give the sets make_plan gives: the same blocks in the same sets, the same bound, and `per` as every full set's longest range
int cmd_equal(char **argv)
{
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const uint32_t nblocks = (uint32_t)strtoul(argv[3], nullptr, 10), set_blocks = (uint32_t)strtoul(argv[4], nullptr, 10), capacity = (uint32_t)strtoul(argv[5], nullptr, 10);
    container::Plan E;
    char text[512] = "";
    if (container::make_plan(E, n, nblocks, set_blocks, capacity, bound, ErrText{ text, sizeof text })) FAIL("make_plan: %s", text);
    std::vector<uint64_t> off(nblocks), len(nblocks);
    for (uint32_t i = 0; i < nblocks; i++) container::block_range(n, E.per, i, off[i], len[i]);
    container::RangesPlan P;
    if (make_and_check(n, off, len, set_blocks, capacity, P)) return 1;
    if (P.sets.size() != E.sets.size() || P.out_bound != E.out_bound) FAIL("%zu sets and a bound of %" PRIu64 ", make_plan has %zu and %" PRIu64, P.sets.size(), P.out_bound, E.sets.size(), E.out_bound);
    for (size_t s = 0; s < P.sets.size(); s++) {
        if (P.sets[s].first != E.sets[s].first || P.sets[s].count != E.sets[s].count) FAIL("set %zu differs", s);
        if (P.sets[s].longest != (E.sets[s].len < E.per ? E.sets[s].len : E.per)) FAIL("set %zu: longest %" PRIu64, s, P.sets[s].longest);
    }
    printf("equal: sets=%zu\n", P.sets.size());
    printf("ranges_plan_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return cmd_sweep();
    if (argc == 6 && !strcmp(argv[1], "plan")) return cmd_plan(argv);
    if (argc == 6 && !strcmp(argv[1], "equal")) return cmd_equal(argv);
    fprintf(stderr, "usage: see the head of ranges_plan_sim.cpp\n");
    return 2;
}
