// cut_sim.cpp -- the cut-point roles (nlzm_amd/csrc/nlzm_cut.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_cut_sim.py, which holds the expected values: tests/cut_model.py's).
//
//   cut_sim <data> <cases>       one line of output per line of <cases>:
//       C <start> <n> <align> <avg_bits> <min_len> <max_len> <threads> <blocks>
//           the n bytes of <data> from <start>, scanned by <blocks> workgroups of <threads> lanes and selected by one wave, twice: at <align>
//           bytes behind a PROT_NONE page ("front"; alignment 0 starts right after it) and with the last byte flush against the PROT_NONE page
//           behind ("back").  Prints, for each of the two, the number of candidates, the number of cuts and the cuts: "cand k c0 c1 ... ; cand k c0 ...".
//       G   prints the segment size.
//
// A read outside the input that leaves the mapping ends the harness with SIGSEGV: this is host code, which is where faults belong.  The
// bitmap, the counts and the list are followed by a word each that has to stay as it was; the selection runs a second time with a list one
// entry short, which must report the same number of cuts and leave the entry behind the list alone.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_cut.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "cut_sim";

namespace {

struct Launch { cut::Args a; uint32_t threads; bool select; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    if (P->select) cut::select_role(P->a);
    else cut::scan_role(P->a, P->threads, (unsigned long long)xw::block_index() * (P->threads / 64) + xw::wave(), (unsigned long long)xw::sim().nblocks * (P->threads / 64));
}

constexpr uint32_t kCanary32 = 0xC0FFEE11u;
constexpr unsigned long long kCanary64 = 0xC0FFEE1122334455ull;

struct Result { unsigned long long cand = 0; std::vector<unsigned long long> cuts; };

Result run(const uint8_t *src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len, uint32_t threads, uint32_t blocks)
{
    Result R;
    if (n <= min_len) return R;                     // (what the library's host side does: no launch)
    const unsigned long long nsegs = n / cut::kSegment + (n % cut::kSegment ? 1 : 0), nwords = (n + 31) / 32, cap = n / min_len;
    std::vector<uint32_t> bits(nwords + 1, 0xDEADBEEFu), count(nsegs + 1, 0xDEADBEEFu);
    std::vector<unsigned long long> list(cap + 1, kCanary64), res(3, kCanary64);
    bits[nwords] = kCanary32; count[nsegs] = kCanary32;
    Launch P{ cut::Args{}, threads, false };
    P.a.src = src; P.a.n = n; P.a.nsegs = nsegs; P.a.bits = bits.data(); P.a.count = count.data(); P.a.cut = list.data(); P.a.res = res.data();
    P.a.cut_cap = cap; P.a.min_len = min_len; P.a.max_len = max_len; P.a.shift = 32 - avg_bits;
    std::vector<unsigned long long> lds(blocks, cut::lds_bytes(threads / 64));
    xw::launch(blocks, threads, lds.data(), entry, &P);
    P.select = true;
    const unsigned long long small = 64;
    xw::launch(1, 64, &small, entry, &P);
    if (bits[nwords] != kCanary32 || count[nsegs] != kCanary32 || list[cap] != kCanary64 || res[2] != kCanary64) { fprintf(stderr, "cut_sim: a write behind a buffer's end\n"); exit(3); }
    for (uint32_t c : std::vector<uint32_t>(count.begin(), count.end() - 1)) if (c == 0xDEADBEEFu) { fprintf(stderr, "cut_sim: a segment's count was not written\n"); exit(3); }
    for (unsigned long long w = 0; w < nwords; w++) if (bits[w] == 0xDEADBEEFu) { fprintf(stderr, "cut_sim: bitmap word %llu was not written\n", w); exit(3); }   // (a word of candidates that happens to read so would be reported too: the cases are fixed, and none does)
    if (res[0] > cap) { fprintf(stderr, "cut_sim: %llu cuts, at most %llu fit\n", res[0], cap); exit(3); }
    R.cand = res[1];
    R.cuts.assign(list.begin(), list.begin() + res[0]);
    if (res[0]) {                                   // a list one entry short: the same count, nothing written behind it
        std::vector<unsigned long long> shorter(res[0], kCanary64), res2(3, kCanary64);
        P.a.cut = shorter.data(); P.a.cut_cap = res[0] - 1; P.a.res = res2.data();
        xw::launch(1, 64, &small, entry, &P);
        if (res2[0] != res[0] || res2[1] != res[1] || shorter[res[0] - 1] != kCanary64 || res2[2] != kCanary64) { fprintf(stderr, "cut_sim: the short list\n"); exit(3); }
        for (unsigned long long i = 0; i + 1 < res[0]; i++) if (shorter[i] != list[i]) { fprintf(stderr, "cut_sim: the short list differs\n"); exit(3); }
    }
    return R;
}

void print(const Result &R, const char *end)
{
    printf("%llu %zu", R.cand, R.cuts.size());
    for (unsigned long long c : R.cuts) printf(" %llu", c);
    printf("%s", end);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of cut_sim.cpp\n"); return 2; }
    const std::vector<uint8_t> data = slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    Guarded g;
    g.make(data.size() + 16);
    const size_t room = (size_t)(g.hi - g.lo);
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'G') { printf("%llu\n", cut::kSegment); continue; }
        if (kind[0] != 'C') return 2;
        unsigned long long start, n, align, min_len, max_len;
        unsigned avg_bits, threads, blocks;
        if (fscanf(f, "%llu %llu %llu %u %llu %llu %u %u", &start, &n, &align, &avg_bits, &min_len, &max_len, &threads, &blocks) != 8 || start + n > data.size() || align + n > room ||
            avg_bits < 1 || avg_bits > 30 || min_len < 32 || min_len > max_len || !threads || threads % 64 || !blocks) return 2;
        memset(g.lo, 0xA5, room);
        uint8_t *front = g.lo + align;
        if (n) memcpy(front, data.data() + start, n);
        print(run(front, n, avg_bits, min_len, max_len, threads, blocks), " ; ");
        memset(g.lo, 0x5A, room);
        uint8_t *back = g.hi - n;
        if (n) memcpy(back, data.data() + start, n);
        print(run(back, n, avg_bits, min_len, max_len, threads, blocks), "\n");
    }
    fclose(f);
    printf("cut_sim: OK\n");
    return 0;
}
