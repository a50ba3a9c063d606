// container_plan_sim.cpp -- the plan of a container compressed in sets (nlzm_amd/csrc/nlzm_container_plan.h) on its own: no device, no library.
// TEST HARNESS ONLY (tests/test_container_plan.py; built by the Makefile with -fsanitize=address,undefined).
//
//   container_plan_sim sweep                                 every combination of the issue's table, checked here (see check()); one line each
//   container_plan_sim plan <n> <nblocks> <set_blocks> <capacity>    one plan, printed: the test holds the block ranges to shard.block_range
#include "../../nlzm_amd/csrc/nlzm_container_plan.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace nlzm;

namespace {

// the library's bound (nlzm_hip_compress_bound; the plan takes it as a parameter so that this file links nothing)
uint64_t bound(uint64_t n) { return 16 + 131072 + (n / 14848 + 1) * 16384; }

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL n=%" PRIu64 " nblocks=%u set_blocks=%u capacity=%u: ", n, nblocks, set_blocks, capacity); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int check(uint64_t n, uint32_t nblocks, uint32_t set_blocks, uint32_t capacity)
{
    container::Plan P;
    char text[256] = "";
    const int rc = container::make_plan(P, n, nblocks, set_blocks, capacity, bound, ErrText{ text, sizeof text });
    if (set_blocks > capacity) { CHECK(rc == NLZM_HIP_E_ARG && text[0], "set_blocks above the capacity was accepted"); return 0; }
    CHECK(rc == 0, "rc %d (%s)", rc, text);
    const uint64_t per = nblocks ? (n / nblocks + (n % nblocks ? 1 : 0)) : 0;
    CHECK(P.per == per && P.nblocks == nblocks, "per %" PRIu64, P.per);
    const size_t nsets = P.sets.size();
    if (nblocks <= capacity) CHECK(nsets == 1, "%zu sets for blocks that fit one launch", nsets);
    else CHECK(nsets == (nblocks + set_blocks - 1) / set_blocks, "%zu sets", nsets);
    // every block in exactly one set, in order; sizes at most the capacity (above it: at most set_blocks) and within one of each other
    uint32_t at = 0, lo_count = ~0u, hi_count = 0;
    uint64_t byte_at = 0, out_bound = 0;
    for (size_t s = 0; s < nsets; s++) {
        const container::Set &S = P.sets[s];
        CHECK(S.first == at && S.count >= 1, "set %zu starts at block %u, expected %u", s, S.first, at);
        CHECK(S.count <= capacity && (nsets == 1 || S.count <= set_blocks), "set %zu holds %u blocks", s, S.count);
        lo_count = S.count < lo_count ? S.count : lo_count; hi_count = S.count > hi_count ? S.count : hi_count;
        // the set's bytes: its blocks' ranges back to back, which tile [0, n) set after set
        CHECK(S.off == byte_at, "set %zu starts at byte %" PRIu64 ", expected %" PRIu64, s, S.off, byte_at);
        CHECK(S.len <= n - S.off, "set %zu: off + len runs over n", s);               // (no off + len that could wrap)
        uint64_t in_set = 0;
        for (uint32_t i = S.first; i < S.first + S.count; i++) {
            uint64_t lo = 0, len = 0;
            container::block_range(n, P.per, i, lo, len);
            // nlzm_amd/shard.py block_range: lo = min(n, i * per), hi = min(n, lo + per), in arithmetic that cannot wrap
            const unsigned __int128 want_lo128 = (unsigned __int128)i * per;
            const uint64_t want_lo = want_lo128 < n ? (uint64_t)want_lo128 : n, want_len = n - want_lo < per ? n - want_lo : per;
            CHECK(lo == want_lo && len == want_len, "block %u is [%" PRIu64 ", +%" PRIu64 ")", i, lo, len);
            CHECK(lo == S.off + in_set, "block %u does not follow the block before it", i);
            CHECK(len <= n - lo, "block %u: off + len runs over n", i);
            // the set's own partition (nlzm_hip_blocks_begin with the partition fixed to `per`, on the set's bytes) gives the same block
            const uint64_t k = i - S.first;
            const unsigned __int128 rel128 = (unsigned __int128)k * per;
            const uint64_t rel_lo = rel128 < S.len ? (uint64_t)rel128 : S.len, rel_len = S.len - rel_lo < per ? S.len - rel_lo : per;
            CHECK(S.off + rel_lo == lo && rel_len == len, "block %u: the set's own cut differs", i);
            in_set += len;
            out_bound += bound(len);
        }
        CHECK(in_set == S.len, "set %zu: its blocks hold %" PRIu64 " bytes, the set says %" PRIu64, s, in_set, S.len);
        byte_at += S.len;
        at += S.count;
    }
    CHECK(at == nblocks, "%u blocks in the sets", at);
    CHECK(byte_at == n, "the sets hold %" PRIu64 " bytes", byte_at);
    CHECK(hi_count - lo_count <= 1, "set sizes %u .. %u", lo_count, hi_count);
    for (size_t s = 1; s < nsets; s++) CHECK(P.sets[s].count <= P.sets[s - 1].count, "a larger set behind a smaller one");
    CHECK(P.out_bound == out_bound, "out_bound %" PRIu64 ", the blocks' bounds sum to %" PRIu64, P.out_bound, out_bound);
    return 0;
}

int cmd_sweep()
{
    const uint32_t nbs[] = { 1, 32, 64, 65, 66, 127, 128, 129, 1000, 65536 }, sbs[] = { 1, 7, 32, 64 }, caps[] = { 16, 64 };
    unsigned ran = 0, refused = 0;
    container::Plan P0;
    for (uint32_t nblocks : nbs) for (uint32_t set_blocks : sbs) for (uint32_t capacity : caps) {
        const uint64_t ns[] = { 0, 1, (uint64_t)nblocks - 1, nblocks, 1000001, 1ull << 63, (1ull << 63) - 65535 };      // (the last two: the largest whose bounds still sum in 64 bits)
        for (uint64_t n : ns) {
            if (check(n, nblocks, set_blocks, capacity)) return 1;
            ran++; refused += set_blocks > capacity;
        }
    }
    // block_range where i * per passes 2^64: the block starts at the input's end, as the 128-bit product says
    for (uint32_t nblocks : nbs) for (uint64_t n : { ~0ull, ~0ull - 1, ~0ull - 65535 }) {
        const uint64_t per = container::per_block(n, nblocks);
        for (uint32_t i : { 0u, 1u, nblocks / 2, nblocks - 2, nblocks - 1 }) {
            if (i >= nblocks) continue;
            uint64_t lo = 0, len = 0;
            container::block_range(n, per, i, lo, len);
            const unsigned __int128 p128 = (unsigned __int128)i * per;
            const uint64_t want_lo = p128 < n ? (uint64_t)p128 : n;
            if (lo != want_lo || len != (n - want_lo < per ? n - want_lo : per) || len > n - lo) { printf("FAIL: block_range(n=%" PRIu64 ", nblocks=%u, i=%u)\n", n, nblocks, i); return 1; }
        }
    }
    // The partition where the library once wrote it out by hand, lo = min(n, i * per) and hi = min(n, (i + 1) * per) in 64 bits (inputs below 2^32):
    // nlzm_hip_blocks_begin with `per` fixed by the caller -- a set of a container or a device's share, so per is larger than ceil(n / nblocks),
    // and a set lying wholly behind the input's end has n = 0 with per > 0: empty blocks at 0 -- and the multi-GPU call's part i of m blocks a
    // device, [min(n, i * m * per), min(n, (i + 1) * m * per)), which is block i of m * per bytes a block.
    for (uint64_t n : { (uint64_t)0, (uint64_t)1, (uint64_t)999, (uint64_t)1000, (uint64_t)1000001, (uint64_t)0xFFFEFFFFu }) for (uint32_t nblocks : { 1u, 2u, 7u, 32u, 64u }) {
        const uint64_t ceil_per = container::per_block(n, nblocks);
        for (uint64_t per : { ceil_per, ceil_per + 1, 2 * ceil_per + 3, n + 1, (uint64_t)0xFFFF0000u }) for (uint32_t m : { 1u, 3u, 64u }) for (uint32_t i = 0; i < nblocks; i++) {
            const uint64_t step = per * m;          // (m = 1: a block of the set; m > 1: a device's part)
            const uint64_t want_lo = (uint64_t)i * step < n ? (uint64_t)i * step : n, want_hi = (uint64_t)(i + 1) * step < n ? (uint64_t)(i + 1) * step : n;
            uint64_t lo = 0, len = 0;
            container::block_range(n, step, i, lo, len);
            if (lo != want_lo || len != want_hi - want_lo) { printf("FAIL: block_range(n=%" PRIu64 ", per=%" PRIu64 ", i=%u) with the partition fixed\n", n, step, i); return 1; }
        }
    }
    if (container::make_plan(P0, ~0ull, 32, 32, 64, bound, ErrText{ nullptr, 0 }) != NLZM_HIP_E_ARG) { printf("FAIL: bounds that do not sum in 64 bits were summed\n"); return 1; }
    // what the plan refuses
    container::Plan P;
    char text[256] = "";
    const ErrText err{ text, sizeof text };
    if (container::make_plan(P, 100, 0, 32, 64, bound, err) != NLZM_HIP_E_ARG || container::make_plan(P, 100, 65537, 32, 64, bound, err) != NLZM_HIP_E_ARG ||
        container::make_plan(P, 100, 70, 0, 64, bound, err) != NLZM_HIP_E_ARG || container::make_plan(P, 100, 70, 32, 0, bound, err) != NLZM_HIP_E_ARG) {
        printf("FAIL: a plan that must be refused was made\n");
        return 1;
    }
    // the issue's own examples
    if (container::make_plan(P, 1000, 65, 32, 64, bound, err) || P.sets.size() != 3 || P.sets[0].count != 22 || P.sets[1].count != 22 || P.sets[2].count != 21) { printf("FAIL: 65 by 32\n"); return 1; }
    if (container::make_plan(P, 1000, 130, 64, 64, bound, err) || P.sets.size() != 3 || P.sets[0].count != 44 || P.sets[1].count != 43 || P.sets[2].count != 43) { printf("FAIL: 130 by 64\n"); return 1; }
    if (container::make_plan(P, 1000, 65, 64, 64, bound, err) || P.sets.size() != 2 || P.sets[0].count != 33 || P.sets[1].count != 32) { printf("FAIL: 65 by 64\n"); return 1; }
    if (container::make_plan(P, 1000, 64, 7, 64, bound, err) || P.sets.size() != 1 || P.sets[0].count != 64) { printf("FAIL: 64 blocks are one set\n"); return 1; }
    printf("sweep: combinations=%u refused=%u\n", ran, refused);
    printf("container_plan_sim: OK\n");
    return 0;
}

int cmd_plan(char **argv)
{
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const uint32_t nblocks = (uint32_t)strtoul(argv[3], nullptr, 10), set_blocks = (uint32_t)strtoul(argv[4], nullptr, 10), capacity = (uint32_t)strtoul(argv[5], nullptr, 10);
    container::Plan P;
    char text[256] = "";
    const int rc = container::make_plan(P, n, nblocks, set_blocks, capacity, bound, ErrText{ text, sizeof text });
    if (rc) { printf("error %d %s\n", rc, text); return 0; }
    printf("per %" PRIu64 " sets %zu out_bound %" PRIu64 "\n", P.per, P.sets.size(), P.out_bound);
    for (const container::Set &S : P.sets) {
        printf("set %u %u %" PRIu64 " %" PRIu64 "\n", S.first, S.count, S.off, S.len);
        for (uint32_t i = S.first; i < S.first + S.count; i++) {
            uint64_t lo = 0, len = 0;
            container::block_range(n, P.per, i, lo, len);
            printf("block %u %" PRIu64 " %" PRIu64 "\n", i, lo, lo + len);
        }
    }
    printf("container_plan_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return cmd_sweep();
    if (argc == 6 && !strcmp(argv[1], "plan")) return cmd_plan(argv);
    fprintf(stderr, "usage: see the head of container_plan_sim.cpp\n");
    return 2;
}
