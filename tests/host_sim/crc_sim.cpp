// crc_sim.cpp -- the CRC32 roles (nlzm_amd/csrc/nlzm_crc.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_crc_sim.py, which holds the expected values: zlib's).
//
//   crc_sim <data> <cases>       one line of output per line of <cases>:
//       C <start> <n> <align> <seed> <threads> <blocks>
//           the n bytes of <data> from <start>, hashed from <seed> by <blocks> workgroups of <threads> lanes, twice: at <align> bytes behind
//           a PROT_NONE page ("front"; alignment 0 starts right after it) and with the last byte flush against the PROT_NONE page behind
//           ("back"; the start's alignment is then what the length leaves).  Prints both CRCs.
//       R <bytes> <k> <off> <len> ... (k pairs)
//           the first <bytes> bytes of <data> (a multiple of the page size: guard pages on both sides), k ranges in one call.  Prints k CRCs.
//       G   prints the segment size.
//
// A read outside a range that leaves the mapping ends the harness with SIGSEGV: this is host code, which is where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_crc.h"
#include "../../nlzm_amd/csrc/nlzm_read_plan.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "crc_sim";

namespace {

struct Launch { crc::Args a; uint32_t threads; bool combine; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    if (P->combine) crc::combine_role(P->a, xw::block_index(), P->threads);
    else crc::segments_role(P->a, P->threads, (unsigned long long)xw::block_index() * (P->threads / 64) + xw::wave(), (unsigned long long)xw::sim().nblocks * (P->threads / 64));
}

// the CRCs of k ranges of the buf_len bytes at buf, from the table the library's host side hands its launch (nlzm_read_plan.h: crc::SegTable)
std::vector<uint32_t> run(const uint8_t *buf, uint64_t buf_len, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, uint32_t seed, uint32_t threads,
                          uint32_t blocks)
{
    const uint32_t k = (uint32_t)off.size();
    crc::SegTable T;
    char why[512];
    if (T.make(buf_len, k, off.data(), len.data(), crc::kSegment, ErrText{ why, sizeof why })) { fprintf(stderr, "crc_sim: %s\n", why); exit(2); }
    const unsigned long long nsegs = T.nsegs;
    std::vector<uint32_t> part(nsegs + 1, 0xDEADBEEFu), out(k, 0xDEADBEEFu);
    Launch P{ crc::Args{}, threads, false };
    P.a.buf = buf; P.a.part = part.data(); P.a.out = out.data(); P.a.seed = seed;
    T.point(P.a, T.words.data());
    if (nsegs) {
        std::vector<unsigned long long> lds(blocks, sizeof(crc::Lds));
        xw::launch(blocks, threads, lds.data(), entry, &P);
    }
    P.combine = true;
    std::vector<unsigned long long> small(k, sizeof(crc::CombineLds));
    xw::launch(k, threads, small.data(), entry, &P);
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of crc_sim.cpp\n"); return 2; }
    const std::vector<uint8_t> data = slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    Guarded g;
    g.make(data.size() + 16);
    const size_t room = (size_t)(g.hi - g.lo);
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'G') { printf("%llu\n", crc::kSegment); continue; }
        if (kind[0] == 'C') {
            unsigned long long start, n, align;
            unsigned seed, threads, blocks;
            if (fscanf(f, "%llu %llu %llu %u %u %u", &start, &n, &align, &seed, &threads, &blocks) != 6 || start + n > data.size() || align + n > room) return 2;
            memset(g.lo, 0xA5, room);
            uint8_t *front = g.lo + align;
            if (n) memcpy(front, data.data() + start, n);
            const uint32_t c0 = run(front, n, { 0 }, { n }, seed, threads, blocks)[0];
            memset(g.lo, 0x5A, room);
            uint8_t *back = g.hi - n;
            if (n) memcpy(back, data.data() + start, n);
            const uint32_t c1 = run(back, n, { 0 }, { n }, seed, threads, blocks)[0];
            printf("%08X %08X\n", c0, c1);
        } else if (kind[0] == 'R') {
            unsigned long long bytes;
            unsigned k;
            if (fscanf(f, "%llu %u", &bytes, &k) != 2 || bytes > data.size() || bytes > room) return 2;
            std::vector<uint64_t> off(k), len(k);
            for (unsigned i = 0; i < k; i++) {
                unsigned long long o, l;
                if (fscanf(f, "%llu %llu", &o, &l) != 2 || o > bytes || l > bytes - o) return 2;
                off[i] = o; len[i] = l;
            }
            Guarded r;
            r.make(bytes);
            if ((size_t)(r.hi - r.lo) != bytes) return 2;
            memcpy(r.lo, data.data(), bytes);
            const std::vector<uint32_t> c = run(r.lo, bytes, off, len, 0, 128, 3);
            for (unsigned i = 0; i < k; i++) printf("%08X%s", c[i], i + 1 < k ? " " : "\n");
        } else return 2;
    }
    fclose(f);
    printf("crc_sim: OK\n");
    return 0;
}
