// dedup_plan_sim.cpp -- the class plan of the equal-range finder (nlzm_amd/csrc/nlzm_dedup_plan.h, the header nlzm_hip_dedup.cpp includes) in a
// program of its own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_dedup_plan.py).
//
//   dedup_plan_sim sweep
//       random range lists over buffers of a two-letter alphabet (equal ranges abound), k = 1 and k = 65,536, the identical-(off, len) and the empty
//       shortcut, a range over the buffer named; the fingerprints -- a hash of the bytes made here -- masked to 0, 2 and 64 bits.  Every result is
//       held to brute force, and every round to the plan's rules (below).  Prints "sweep: cases=N".
//   dedup_plan_sim plan <hash_bits> <data> <ranges>
//       <ranges>: lines "off len".  Prints "first_of i0 i1 ...", then "distinct D dup_bytes B rounds R pairs P compared_bytes C", or
//       "error <code> <text>".
// What `compare` holds every round to: a pair's two ranges have the same length and masked fingerprint, no length 0, not the same (off, len), and
// rep < member; an index is a member at most once a round; a representative, or a member that was found equal, never shows up again -- so every
// element is resolved exactly once.  Afterwards: the rounds are at most the largest number of distinct contents in a group.
#include "../../nlzm_amd/csrc/nlzm_dedup_plan.h"
#include "sim_kit.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <string>
#include <vector>

using namespace nlzm;
using simkit::slurp;

namespace {

void die(const char *what) { fprintf(stderr, "dedup_plan_sim: %s\n", what); exit(3); }

uint64_t content_hash(const uint8_t *p, uint64_t n)         // (any function of the bytes and the length will do here)
{
    uint64_t h = 0xCBF29CE484222325ull ^ n;
    for (uint64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    return h ^ (h >> 29);
}

struct Run { dedup::Classes R; int rc = 0; };

Run run_checked(const std::vector<uint8_t> &buf, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, uint32_t hash_bits)
{
    const uint32_t k = (uint32_t)off.size();
    const uint64_t mask = dedup::mask_of(hash_bits);
    std::vector<uint64_t> fp(k);
    for (uint32_t i = 0; i < k; i++) fp[i] = content_hash(buf.data() + off[i], len[i]);
    std::vector<uint8_t> closed(k, 0);              // 1: was a representative, or was found equal
    std::vector<uint32_t> seen_in(k, 0);
    uint32_t round = 0;
    Run out;
    out.rc = dedup::class_plan(out.R, k, off.data(), len.data(), fp.data(), hash_bits, [&](const std::vector<dedup::IndexPair> &pairs, std::vector<uint8_t> &equal) {
        round++;
        if (pairs.empty() || equal.size() != pairs.size()) die("an empty round, or verdicts of another size");
        std::vector<uint32_t> reps;
        for (size_t p = 0; p < pairs.size(); p++) {
            const uint32_t a = pairs[p].rep, b = pairs[p].member;
            if (a >= b || b >= k) die("a pair's indices");
            if (len[a] != len[b] || !len[a] || ((fp[a] ^ fp[b]) & mask) || off[a] == off[b]) die("a pair that needs no compare, or of two groups");
            if (closed[a] || closed[b]) die("a resolved element is compared again");
            if (seen_in[b] == round) die("an element is a member twice in a round");
            seen_in[b] = round;
            equal[p] = !memcmp(buf.data() + off[a], buf.data() + off[b], len[a]);
            reps.push_back(a);
        }
        for (size_t p = 0; p < pairs.size(); p++) {
            if (seen_in[pairs[p].rep] == round) die("a representative is a member in its round");
            if (equal[p]) closed[pairs[p].member] = 1;
        }
        for (uint32_t a : reps) closed[a] = 1;
        return 0;
    });
    if (out.rc) return out;
    // brute force: the smallest j <= i with the same bytes
    const dedup::Classes &R = out.R;
    if (R.first_of.size() != k) die("first_of's size");
    std::map<std::string, uint32_t> first;
    uint64_t distinct = 0, dup_bytes = 0;
    std::map<std::pair<uint64_t, uint64_t>, std::map<std::string, int>> groups;
    for (uint32_t i = 0; i < k; i++) {
        const std::string s((const char *)buf.data() + off[i], (size_t)len[i]);
        const uint32_t want = first.emplace(s, i).first->second;
        if (R.first_of[i] != want) { fprintf(stderr, "dedup_plan_sim: first_of[%u] = %u, brute force says %u (hash_bits %u)\n", i, R.first_of[i], want, hash_bits); exit(3); }
        if (want == i) distinct++; else dup_bytes += len[i];
        groups[{ len[i], fp[i] & mask }][s]++;
    }
    size_t most = 0;
    for (const auto &g : groups) if (g.second.size() > most) most = g.second.size();
    if (R.distinct != distinct || R.dup_bytes != dup_bytes || R.rounds != round) die("the plan's counts");
    if (R.rounds > most) die("more rounds than a group has distinct contents");
    if (hash_bits == 64 && R.rounds > 1) die("a second round with fingerprints that tell all contents apart");
    return out;
}

int sweep()
{
    std::mt19937_64 rng(20260101);
    unsigned long cases = 0;
    for (int t = 0; t < 600; t++) {
        const uint32_t n = (uint32_t)(rng() % 80), k = 1 + (uint32_t)(rng() % (t % 10 ? 40 : 400));
        std::vector<uint8_t> buf(n + 1);
        for (auto &b : buf) b = "ab"[rng() & 1];
        std::vector<uint64_t> off(k), len(k);
        for (uint32_t i = 0; i < k; i++) { off[i] = rng() % (n + 1); len[i] = rng() % (std::min<uint64_t>(7, n - off[i]) + 1); }
        const Run full = run_checked(buf, off, len, 64);
        for (uint32_t bits : { 0u, 2u }) {
            const Run r = run_checked(buf, off, len, bits);
            if (r.R.first_of != full.R.first_of) die("first_of depends on the mask");
            cases++;
        }
        cases++;
    }
    {   // k = 1; the shortcuts: identical (off, len) and empties take no compare
        std::vector<uint8_t> buf(64, 'x');
        const Run one = run_checked(buf, { 5 }, { 9 }, 0);
        if (one.R.first_of != std::vector<uint32_t>{ 0 } || one.R.rounds || one.R.pairs) die("k = 1");
        const Run same = run_checked(buf, { 3, 60, 3, 0, 3, 64 }, { 7, 0, 7, 0, 7, 0 }, 0);
        if (same.R.first_of != std::vector<uint32_t>{ 0, 1, 0, 1, 0, 1 } || same.R.rounds || same.R.pairs || same.R.distinct != 2 || same.R.dup_bytes != 14) die("the shortcuts");
        const Run shifted = run_checked(buf, { 3, 4, 3 }, { 7, 7, 7 }, 64);
        if (shifted.R.first_of != std::vector<uint32_t>{ 0, 0, 0 } || shifted.R.rounds != 1 || shifted.R.pairs != 1 || shifted.R.compared_bytes != 7) die("one pair");
        cases += 3;
    }
    {   // k = 65,536: all equal at other offsets (one round of 65,535 pairs); four contents under one fingerprint (four rounds at most); all alike by (off, len)
        const uint32_t k = 65536;
        std::vector<uint8_t> zeros(k + 8, 0), four(k + 8);
        for (size_t i = 0; i < four.size(); i++) four[i] = (uint8_t)((i / 3) & 3);
        std::vector<uint64_t> off(k), len(k, 8), same_off(k, 17);
        for (uint32_t i = 0; i < k; i++) off[i] = i;
        const Run a = run_checked(zeros, off, len, 64);
        if (a.R.distinct != 1 || a.R.rounds != 1 || a.R.pairs != k - 1 || a.R.dup_bytes != 8ull * (k - 1)) die("65,536 equal ranges");
        const Run b = run_checked(four, off, std::vector<uint64_t>(k, 1), 0);
        if (b.R.distinct != 4 || b.R.rounds > 4 || b.R.rounds < 2) die("65,536 ranges of four contents");
        const Run c = run_checked(four, same_off, len, 2);
        if (c.R.distinct != 1 || c.R.rounds || c.R.pairs) die("65,536 times one range");
        cases += 3;
    }
    {   // the arguments: k out of range, a range over the buffer (also where off + len wraps) named
        char text[256];
        const uint64_t off[3] = { 0, 90, ~0ull }, len[3] = { 10, 11, 2 };
        if (dedup::check_ranges(100, 0, off, len, ErrText{ text, sizeof text }) != NLZM_HIP_E_ARG || dedup::check_ranges(100, 65537, off, len, ErrText{ text, sizeof text }) != NLZM_HIP_E_ARG) die("k out of range");
        if (dedup::check_ranges(100, 1, off, len, ErrText{ text, sizeof text }) || dedup::check_ranges(100, 1, nullptr, len, ErrText{ text, sizeof text }) != NLZM_HIP_E_ARG) die("check_ranges");
        if (dedup::check_ranges(100, 2, off, len, ErrText{ text, sizeof text }) != NLZM_HIP_E_ARG || !strstr(text, "range 1 ") || !strstr(text, "runs over")) die("a range over the buffer");
        const uint64_t off2[3] = { 0, 90, ~0ull }, len2[3] = { 10, 10, 2 };
        if (dedup::check_ranges(100, 3, off2, len2, ErrText{ text, sizeof text }) != NLZM_HIP_E_ARG || !strstr(text, "range 2 ")) die("a range that wraps");
        cases += 4;
    }
    printf("sweep: cases=%lu\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        const int rc = sweep();
        if (!rc) printf("dedup_plan_sim: OK\n");
        return rc;
    }
    if (argc == 5 && !strcmp(argv[1], "plan")) {
        const uint32_t bits = (uint32_t)atoi(argv[2]);
        std::vector<uint8_t> buf = slurp(argv[3]);
        const uint64_t n = buf.size();
        buf.push_back(0);
        std::vector<uint64_t> off, len;
        FILE *f = fopen(argv[4], "r");
        if (!f) return 2;
        unsigned long long o, l;
        while (fscanf(f, "%llu %llu", &o, &l) == 2) { off.push_back(o); len.push_back(l); }
        fclose(f);
        char text[512] = "";
        if (const int rc = dedup::check_ranges(n, (uint32_t)off.size(), off.data(), len.data(), ErrText{ text, sizeof text })) {
            printf("error %d %s\ndedup_plan_sim: OK\n", rc, text);
            return 0;
        }
        const Run r = run_checked(buf, off, len, bits);
        printf("first_of");
        for (uint32_t v : r.R.first_of) printf(" %u", v);
        printf("\ndistinct %llu dup_bytes %llu rounds %llu pairs %llu compared_bytes %llu\n", (unsigned long long)r.R.distinct, (unsigned long long)r.R.dup_bytes,
               (unsigned long long)r.R.rounds, (unsigned long long)r.R.pairs, (unsigned long long)r.R.compared_bytes);
        printf("dedup_plan_sim: OK\n");
        return 0;
    }
    fprintf(stderr, "usage: see the head of dedup_plan_sim.cpp\n");
    return 2;
}
