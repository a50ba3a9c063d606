// dedup_sim.cpp -- the equal-range finder's roles (nlzm_amd/csrc/nlzm_dedup.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_dedup_sim.py, which holds the expected values: tests/dedup_model.py's fingerprints, and byte comparisons).
//
//   dedup_sim <data> <cases>     one line of output per line of <cases>; <threads> lanes a workgroup, <blocks> workgroups for every launch of the case:
//       G   prints the segment and the chunk size.
//       F <start> <n> <align> <threads> <blocks>
//           the fingerprint of the n bytes of <data> from <start>, twice: at <align> bytes behind a PROT_NONE page ("front"; alignment 0 starts right
//           after it) and with the last byte flush against the PROT_NONE page behind ("back").  Prints both, in hex.
//       R <threads> <blocks> <count> <off> <len> ...
//           the fingerprints of <count> ranges of <data> in ONE launch; <data> lies flush against the PROT_NONE page behind.  Prints them, in hex.
//       P <a_start> <b_start> <n> <align_a> <align_b> <flip> <threads> <blocks>
//           are the n bytes of <data> from <a_start> and those from <b_start> -- with byte <flip> of the second string inverted, -1: none -- equal?
//           Each string in a region of its own between PROT_NONE pages, three placements: both behind their front pages at their alignments; the
//           first flush against the page behind it; the second flush against the page behind it.  Prints the three verdicts.
//       Q <threads> <blocks> <count> <a> <b> <len> ...
//           the verdicts of <count> pairs of offsets into <data> in ONE launch (the sides may overlap); <data> flush against the page behind.
//
// A read outside a string that leaves the mapping ends the harness with SIGSEGV: this is host code, which is where faults belong.  Every output array
// is followed by a word that has to stay as it was, and every word of it has to be written.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_dedup.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "dedup_sim";

namespace {

enum Role { kFingerprint, kCombine, kPair, kVerdict };
struct Launch { Role role; dedup::FpArgs f; dedup::PairArgs p; uint32_t threads; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    const unsigned long long wpb = P->threads / 64, w = (unsigned long long)xw::block_index() * wpb + xw::wave(), nw = (unsigned long long)xw::sim().nblocks * wpb;
    switch (P->role) {
    case kFingerprint: dedup::fingerprint_role(P->f, w, nw); break;
    case kCombine: dedup::combine_role(P->f, w, nw); break;
    case kPair: dedup::pair_role(P->p, w, nw); break;
    case kVerdict: dedup::verdict_role(P->p, w, nw); break;
    }
}
void launch(Launch &L, Role role, uint32_t blocks)
{
    L.role = role;
    std::vector<unsigned long long> lds(blocks, 64);
    xw::launch(blocks, L.threads, lds.data(), entry, &L);
}

constexpr uint32_t kCanary32 = 0xC0FFEE11u, kUnwritten32 = 0xDEADBEEFu;
constexpr unsigned long long kCanary64 = 0xC0FFEE1122334455ull, kUnwritten64 = 0xDEADBEEFDEADBEEFull;

void die(const char *what) { fprintf(stderr, "dedup_sim: %s\n", what); exit(3); }

// the fingerprints of the ranges of the bytes at buf, as the library's host side launches them
std::vector<unsigned long long> fingerprints(const uint8_t *buf, const std::vector<unsigned long long> &off, const std::vector<unsigned long long> &len, uint32_t threads, uint32_t blocks)
{
    const size_t k = off.size();
    const std::vector<unsigned long long> seg0 = units::prefix((uint32_t)k, dedup::kSegment, [&](uint32_t i) { return len[i]; });      // (the library's: nlzm_units.h)
    std::vector<unsigned long long> seg_h(seg0[k] + 1, kUnwritten64), fp(k + 1, kUnwritten64);
    seg_h[seg0[k]] = kCanary64; fp[k] = kCanary64;
    Launch L{ kFingerprint, dedup::FpArgs{ buf, off.data(), len.data(), seg0.data(), seg_h.data(), fp.data(), (uint32_t)k, seg0[k] }, dedup::PairArgs{}, threads };
    if (seg0[k]) launch(L, kFingerprint, blocks);
    launch(L, kCombine, blocks);
    if (seg_h[seg0[k]] != kCanary64 || fp[k] != kCanary64) die("a write behind a buffer's end");
    for (unsigned long long s = 0; s < seg0[k]; s++) if (seg_h[s] == kUnwritten64) die("a segment's word was not written");
    for (size_t i = 0; i < k; i++) if (fp[i] == kUnwritten64) die("a range's fingerprint was not written");
    fp.pop_back();
    return fp;
}

// the verdicts of the pairs of offsets from buf
std::vector<uint32_t> verdicts(const uint8_t *buf, const std::vector<dedup::Pair> &pairs, uint32_t threads, uint32_t blocks)
{
    const size_t np = pairs.size();
    const std::vector<unsigned long long> c0 = units::prefix((uint32_t)np, dedup::kChunk, [&](uint32_t p) { return pairs[p].len; });
    std::vector<uint32_t> ne(c0[np] + 1, kUnwritten32), eq(np + 1, kUnwritten32);
    ne[c0[np]] = kCanary32; eq[np] = kCanary32;
    Launch L{ kPair, dedup::FpArgs{}, dedup::PairArgs{ buf, pairs.data(), c0.data(), ne.data(), eq.data(), (uint32_t)np, c0[np] }, threads };
    if (c0[np]) launch(L, kPair, blocks);
    launch(L, kVerdict, blocks);
    if (ne[c0[np]] != kCanary32 || eq[np] != kCanary32) die("a write behind a buffer's end");
    for (unsigned long long c = 0; c < c0[np]; c++) if (ne[c] > 1) die("a chunk's word was not written");
    for (size_t p = 0; p < np; p++) if (eq[p] > 1) die("a pair's verdict was not written");
    eq.pop_back();
    return eq;
}

bool shape_ok(unsigned threads, unsigned blocks) { return threads && threads % 64 == 0 && threads <= 1024 && blocks; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of dedup_sim.cpp\n"); return 2; }
    const std::vector<uint8_t> data = slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    Regions map;                                    // ONE mapping, region A and region B: the two strings of a pair are offsets from one base
    map.make(2, data.size() + 16);
    const struct { uint8_t *base, *a_lo, *a_hi, *b_lo, *b_hi; size_t room; } g{ map.base, map.lo(0), map.hi(0), map.lo(1), map.hi(1), map.room };
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        unsigned threads, blocks;
        if (kind[0] == 'G') { printf("%llu %llu\n", dedup::kSegment, dedup::kChunk); continue; }
        if (kind[0] == 'F') {
            unsigned long long start, n, align;
            if (fscanf(f, "%llu %llu %llu %u %u", &start, &n, &align, &threads, &blocks) != 5 || start + n > data.size() || align + n > g.room || !shape_ok(threads, blocks)) return 2;
            memset(g.a_lo, 0xA5, g.room);
            uint8_t *front = g.a_lo + align;
            if (n) memcpy(front, data.data() + start, n);
            const unsigned long long f0 = fingerprints(g.base, { (unsigned long long)(front - g.base) }, { n }, threads, blocks)[0];
            memset(g.a_lo, 0x5A, g.room);
            uint8_t *back = g.a_hi - n;
            if (n) memcpy(back, data.data() + start, n);
            const unsigned long long f1 = fingerprints(g.base, { (unsigned long long)(back - g.base) }, { n }, threads, blocks)[0];
            printf("%016llx %016llx\n", f0, f1);
        } else if (kind[0] == 'R' || kind[0] == 'Q') {
            unsigned count;
            if (fscanf(f, "%u %u %u", &threads, &blocks, &count) != 3 || !shape_ok(threads, blocks) || !count || count > 65536) return 2;
            memset(g.a_lo, 0xA5, g.room);
            uint8_t *at = g.a_hi - data.size();
            if (!data.empty()) memcpy(at, data.data(), data.size());
            if (kind[0] == 'R') {
                std::vector<unsigned long long> off(count), len(count);
                for (unsigned i = 0; i < count; i++) if (fscanf(f, "%llu %llu", &off[i], &len[i]) != 2 || off[i] > data.size() || len[i] > data.size() - off[i]) return 2;
                for (unsigned long long v : fingerprints(at, off, len, threads, blocks)) printf("%016llx ", v);
            } else {
                std::vector<dedup::Pair> pairs(count);
                for (auto &p : pairs) if (fscanf(f, "%llu %llu %llu", &p.a, &p.b, &p.len) != 3 || p.a > data.size() || p.b > data.size() || p.len > data.size() - p.a || p.len > data.size() - p.b) return 2;
                for (uint32_t v : verdicts(at, pairs, threads, blocks)) printf("%u ", v);
            }
            printf("\n");
        } else if (kind[0] == 'P') {
            unsigned long long a_start, b_start, n, align_a, align_b;
            long long flip;
            if (fscanf(f, "%llu %llu %llu %llu %llu %lld %u %u", &a_start, &b_start, &n, &align_a, &align_b, &flip, &threads, &blocks) != 8 || a_start + n > data.size() ||
                b_start + n > data.size() || align_a + n > g.room || align_b + n > g.room || flip >= (long long)n || !shape_ok(threads, blocks)) return 2;
            for (int place = 0; place < 3; place++) {
                memset(g.a_lo, 0xA5, g.room);
                memset(g.b_lo, 0x5A, g.room);
                uint8_t *a = place == 1 ? g.a_hi - n : g.a_lo + align_a, *b = place == 2 ? g.b_hi - n : g.b_lo + align_b;
                if (n) { memcpy(a, data.data() + a_start, n); memcpy(b, data.data() + b_start, n); }
                if (flip >= 0) b[flip] ^= 0xFF;
                printf("%u ", verdicts(g.base, { dedup::Pair{ (unsigned long long)(a - g.base), (unsigned long long)(b - g.base), n } }, threads, blocks)[0]);
            }
            printf("\n");
        } else return 2;
    }
    fclose(f);
    printf("dedup_sim: OK\n");
    return 0;
}
