// elem_sim.cpp -- the count role and the total role of the element-size statistic (nlzm_amd/csrc/nlzm_elem.h) run on the CPU, every lane a fiber
// (xw_sim.cpp).  TEST HARNESS ONLY (tests/test_elem_sim.py, which holds the expected values: tests/elem_model.py's).
//
//   elem_sim <data> <cases>    one line of output per range of every launch of <cases>:
//       L <threads> <blocks> <k> <hist>      a launch of k ranges, followed by k lines
//       <mode> <salign> <start> <n>
//           the n bytes of <data> from <start>.  Range i's source lies in slot i (k: 8 at most), a mapping of its own between two PROT_NONE pages: mode F
//           at <salign> bytes behind the page in front (0 starts right after it), mode B with its last byte flush against the page behind.  Mode D
//           (k: 1,024 at most): the source is slot 0 itself, which holds <data> from its first byte on, at offset <start> -- ranges of that mode may
//           overlap and repeat (no range of another mode may come first in such a launch).  <hist> 1: the totals of every range are kept, as the
//           library keeps them for a caller that wants the histograms; 0: of the ranges of more than one segment only.
//           Prints C_1 C_2 C_4 C_8 and the CRC32 of the range's 2,048 totals as little-endian 64-bit words ("-" where none were kept).
//       G   prints the segment size.
//
// A read outside a source that leaves its mapping ends the harness with SIGSEGV: this is host code, which is where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_elem.h"
#include "../../nlzm_amd/csrc/nlzm_elem_plan.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;

const char simkit::kProgram[] = "elem_sim";

static_assert(elem::kBins == elem::kCounters && elem::kNoSlot == elem::kNone, "the plan's table is the roles'");

namespace {

struct Launch { elem::Args a; uint32_t threads; bool total; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    const unsigned long long w = (unsigned long long)xw::block_index() * (P->threads / 64) + xw::wave(), nw = (unsigned long long)xw::sim().nblocks * (P->threads / 64);
    if (P->total) elem::total_role(P->a, w, nw);
    else elem::count_role(P->a, w, nw);
}

constexpr uint32_t kSlots = 8, kMany = 1024;

uint32_t crc32_of(const uint8_t *p, size_t n)
{
    static uint32_t table[256];
    if (!table[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); table[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of elem_sim.cpp\n"); return 2; }
    const std::vector<uint8_t> data = simkit::slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    simkit::Regions slots;
    slots.make(kSlots, 3 * (size_t)elem::kSegment + 64);
    uint8_t *const map = slots.base;
    const size_t pg = simkit::page(), room = slots.room, stride = slots.stride;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'G') { printf("%llu\n", elem::kSegment); continue; }
        if (kind[0] != 'L') return 2;
        unsigned threads, blocks, k, hist;
        if (fscanf(f, "%u %u %u %u", &threads, &blocks, &k, &hist) != 4 || !threads || threads % 64 || !blocks || !k || k > kMany) return 2;
        std::vector<uint64_t> off(k), len(k);
        for (uint32_t s = 0; s < kSlots; s++) memset(map + s * stride + pg, 0xA5, room);
        bool whole = false;
        for (uint32_t i = 0; i < k; i++) {
            char mode[4];
            unsigned long long salign, start, n;
            if (fscanf(f, "%3s %llu %llu %llu", mode, &salign, &start, &n) != 4 || start + n > data.size() || n + salign > room - 64 || salign > 15) return 2;
            uint8_t *at = nullptr;
            if (mode[0] == 'D') {
                if (!whole) { if (i || data.size() > room) return 2; memcpy(map + pg, data.data(), data.size()); whole = true; }
                at = map + pg + start;
            } else {
                if (whole || i >= kSlots) return 2;
                uint8_t *lo = map + i * stride + pg, *hi = lo + room;
                at = mode[0] == 'B' ? hi - n : lo + salign;
                if (n) memcpy(at, data.data() + start, n);
            }
            off[i] = (uint64_t)(at - map); len[i] = n;
        }
        char why[512] = "";
        if (elem::check_ranges(kSlots * stride + pg, k, off.data(), len.data(), ErrText{ why, sizeof why })) { fprintf(stderr, "elem_sim: %s\n", why); return 2; }
        elem::Table T;
        T.make(k, off.data(), len.data(), elem::kSegment, hist != 0);
        const elem::Scratch need(T);
        // the totals and the costs between canaries: what the library zeroes is zero, nothing else is written
        simkit::Canaried totals, cost;
        totals.make(need.totals, 0, 0);
        cost.make(need.cost, 0, 0);
        Launch P{ elem::Args{}, threads, false };
        P.a.src = map; P.a.totals = (unsigned long long *)totals.p(); P.a.cost = (unsigned long long *)cost.p();
        T.point(P.a, T.words.data());
        if (T.nsegs) {                              // (what the library's host side does: no segment, no launch; no wide range, no second launch)
            std::vector<unsigned long long> lds(blocks, elem::lds_bytes(threads / 64));
            xw::launch(blocks, threads, lds.data(), entry, &P);
            if (T.nwide) { P.total = true; xw::launch(blocks, threads, lds.data(), entry, &P); }
        }
        if (!totals.intact() || !cost.intact()) { fprintf(stderr, "elem_sim: a write outside the totals or the costs\n"); return 3; }
        for (uint32_t i = 0; i < k; i++) {
            const unsigned long long *c = P.a.cost + 4 * (size_t)i, slot = P.a.slot[i];
            printf("%llu %llu %llu %llu ", c[0], c[1], c[2], c[3]);
            if (slot == elem::kNoSlot) printf("-\n");
            else printf("%08x\n", crc32_of((const uint8_t *)(P.a.totals + slot * elem::kBins), elem::kBins * 8));
        }
    }
    fclose(f);
    printf("elem_sim: OK\n");
    return 0;
}
