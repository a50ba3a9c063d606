// planes_sim.cpp -- the byte-plane role (nlzm_amd/csrc/nlzm_planes.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_planes_sim.py, which holds the expected values: tests/planes_model.py's).
//
//   planes_sim <data> <cases>    one line of output per launch of <cases>:
//       L <inverse> <threads> <blocks> <k>      a launch of k ranges (1 .. 8), followed by k lines
//       <mode> <salign> <start> <n> <e> <dalign>
//           the n bytes of <data> from <start>, at element size e.  Range i's source lies in slot i, a mapping of its own between two PROT_NONE
//           pages: mode F at <salign> bytes behind the page in front (0 starts right after it), mode B with its last byte flush against the page
//           behind.  Mode D: the source is slot 0 itself, which holds <data> from its first byte on, at offset <start> -- ranges of that mode may
//           overlap (no range of another mode may come first in such a launch).  The destination is 64 + <dalign> bytes into a stretch of its own
//           of one buffer that is 64-byte aligned; every byte of that buffer outside the destinations has to stay as it was.
//           Prints the CRC32 of every range's destination.
//       G   prints the segment size.
//
// A read outside a source that leaves its mapping ends the harness with SIGSEGV: this is host code, which is where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_planes.h"
#include "../../nlzm_amd/csrc/nlzm_planes_plan.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;

const char simkit::kProgram[] = "planes_sim";

namespace {

struct Launch { planes::Args a; bool inverse; uint32_t threads; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    planes::planes_role(P->a, P->inverse, (unsigned long long)xw::block_index() * (P->threads / 64) + xw::wave(), (unsigned long long)xw::sim().nblocks * (P->threads / 64));
}

constexpr uint32_t kSlots = 8;
constexpr uint8_t kCanary = 0xEE;

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
    if (argc != 3) { fprintf(stderr, "usage: see the head of planes_sim.cpp\n"); return 2; }
    const std::vector<uint8_t> data = simkit::slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    // the slots: ONE mapping, [PROT_NONE page][room][PROT_NONE page][room] ... [PROT_NONE page], so that every source is an offset from its first byte
    simkit::Regions slots;
    slots.make(kSlots, 3 * (size_t)planes::kSegment + 64);
    uint8_t *const map = slots.base;
    const size_t pg = simkit::page(), room = slots.room, stride = slots.stride;
    const size_t dstride = room + 256;
    uint8_t *dst = nullptr;
    if (posix_memalign((void **)&dst, 64, kSlots * dstride)) return 2;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'G') { printf("%llu\n", planes::kSegment); continue; }
        if (kind[0] != 'L') return 2;
        unsigned inverse, threads, blocks, k;
        if (fscanf(f, "%u %u %u %u", &inverse, &threads, &blocks, &k) != 4 || !threads || threads % 64 || !blocks || !k || k > kSlots) return 2;
        std::vector<uint64_t> src_off(k), dst_off(k), len(k);
        std::vector<uint8_t> elem(k);
        memset(dst, kCanary, kSlots * dstride);
        for (uint32_t s = 0; s < kSlots; s++) memset(map + s * stride + pg, 0xA5, room);
        bool whole = false;
        for (uint32_t i = 0; i < k; i++) {
            char mode[4];
            unsigned long long salign, start, n, e, dalign;
            if (fscanf(f, "%3s %llu %llu %llu %llu %llu", mode, &salign, &start, &n, &e, &dalign) != 6 || start + n > data.size() || n + salign > room - 64 || salign > 15 || dalign > 15) return 2;
            uint8_t *lo = map + i * stride + pg, *hi = lo + room, *at = nullptr;
            if (mode[0] == 'D') {
                if (!whole) { if (i || data.size() > room) return 2; memcpy(map + pg, data.data(), data.size()); whole = true; }
                at = map + pg + start;
            } else {
                if (whole && !i) return 2;
                at = mode[0] == 'B' ? hi - n : lo + salign;
                if (n) memcpy(at, data.data() + start, n);
            }
            src_off[i] = (uint64_t)(at - map); dst_off[i] = i * dstride + 64 + dalign; len[i] = n; elem[i] = (uint8_t)e;
        }
        char why[512] = "";
        if (planes::check_ranges((uint64_t)(uintptr_t)map, kSlots * stride + pg, (uint64_t)(uintptr_t)dst, kSlots * dstride, k, src_off.data(), dst_off.data(), len.data(), elem.data(),
                                 ErrText{ why, sizeof why })) { fprintf(stderr, "planes_sim: %s\n", why); return 2; }
        planes::Table T;
        if (T.make(k, src_off.data(), dst_off.data(), len.data(), elem.data(), planes::kSegment, ErrText{ why, sizeof why })) { fprintf(stderr, "planes_sim: %s\n", why); return 2; }
        Launch P{ planes::Args{}, inverse != 0, threads };
        P.a.src = map; P.a.dst = dst;
        T.point(P.a, T.words.data());
        if (T.nsegs) {                              // (what the library's host side does: no segment, no launch)
            std::vector<unsigned long long> lds(blocks, planes::lds_bytes(threads / 64));
            xw::launch(blocks, threads, lds.data(), entry, &P);
        }
        // nothing outside the destinations was written
        std::vector<uint8_t> mine(kSlots * dstride, 0);
        for (uint32_t i = 0; i < k; i++) memset(mine.data() + dst_off[i], 1, len[i]);
        for (size_t b = 0; b < mine.size(); b++) if (!mine[b] && dst[b] != kCanary) { fprintf(stderr, "planes_sim: a write outside the destinations, at byte %zu\n", b); return 3; }
        for (uint32_t i = 0; i < k; i++) printf("%08x%s", crc32_of(dst + dst_off[i], len[i]), i + 1 < k ? " " : "\n");
    }
    fclose(f);
    free(dst);
    printf("planes_sim: OK\n");
    return 0;
}
