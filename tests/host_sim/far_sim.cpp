// far_sim.cpp -- the CRC32, equal-range and byte-plane roles (nlzm_amd/csrc/nlzm_crc.h, nlzm_dedup.h, nlzm_planes.h) at offsets on either side of 2^32
// of ONE buffer, run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY (tests/test_far_sim.py, which holds the expected values:
// tests/far_model.py's).  The buffer is a mapping of <n> bytes made with MAP_NORESERVE, of which only the pages round the islands are ever touched; a
// second one is the byte planes' destination.  Where the kernel refuses such a mapping the harness says so and leaves with status 4.
//
//   far_sim <islands> <cases>    <cases>, one command a line; every command but M, Z and I prints one line:
//       M <n>                                    map the two buffers (once, first)
//       Z <off> <len> <byte>                     fill a stretch of the source
//       I <off> <len> <at>                       the <len> bytes of the file <islands> from <at> on, to offset <off> of the source
//       C <k> <off> <len> ...                    the CRC32s of k ranges, one launch of the segments role and one of the combine role, from the table the
//                                                library's host side makes (crc::SegTable)
//       F <k> <off> <len> ...                    the fingerprints of k ranges, one launch of each role, from units::prefix's table
//       Q <k> <a> <b> <len> ...                  the verdicts of k pairs of offsets
//       P <inverse> <k> <src_off> <dst_off> <len> <e> ...
//                                                one launch of the planes role into the destination buffer; prints the CRC32 of every destination, checks
//                                                that the pages they lie in hold nothing else, and clears them again
//   Every launch: 128 lanes a workgroup, 3 workgroups.  Output arrays carry a guard word behind them.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_crc.h"
#include "../../nlzm_amd/csrc/nlzm_dedup.h"
#include "../../nlzm_amd/csrc/nlzm_planes.h"
#include "../../nlzm_amd/csrc/nlzm_dedup_plan.h"
#include "../../nlzm_amd/csrc/nlzm_planes_plan.h"
#include "../../nlzm_amd/csrc/nlzm_read_plan.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

using namespace nlzm;
using simkit::slurp;

namespace {

constexpr uint32_t kThreads = 128, kBlocks = 3;
constexpr unsigned long long kCanary64 = 0xC0FFEE1122334455ull;
constexpr uint32_t kCanary32 = 0xC0FFEE11u;

void die(const char *what) { fprintf(stderr, "far_sim: %s\n", what); exit(3); }

enum Role { kCrcSegments, kCrcCombine, kFingerprint, kFpCombine, kPair, kVerdict, kPlanes };
struct Launch { Role role; crc::Args c; dedup::FpArgs f; dedup::PairArgs p; planes::Args pl; bool inverse; };
void entry(void *arg)
{
    const Launch *P = (const Launch *)arg;
    const unsigned long long wpb = kThreads / 64, w = (unsigned long long)xw::block_index() * wpb + xw::wave(), nw = (unsigned long long)xw::sim().nblocks * wpb;
    switch (P->role) {
    case kCrcSegments: crc::segments_role(P->c, kThreads, w, nw); break;
    case kCrcCombine: crc::combine_role(P->c, xw::block_index(), kThreads); break;
    case kFingerprint: dedup::fingerprint_role(P->f, w, nw); break;
    case kFpCombine: dedup::combine_role(P->f, w, nw); break;
    case kPair: dedup::pair_role(P->p, w, nw); break;
    case kVerdict: dedup::verdict_role(P->p, w, nw); break;
    case kPlanes: planes::planes_role(P->pl, P->inverse, w, nw); break;
    }
}
void launch(Launch &L, Role role, uint32_t blocks, unsigned long long lds_bytes)
{
    L.role = role;
    std::vector<unsigned long long> lds(blocks, lds_bytes);
    xw::launch(blocks, kThreads, lds.data(), entry, &L);
}

uint32_t crc32_of(const uint8_t *p, size_t n)
{
    static uint32_t table[256];
    if (!table[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); table[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint8_t *far_map(unsigned long long n)
{
    void *m = mmap(nullptr, (size_t)n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) { printf("far_sim: the kernel refuses a mapping of %llu bytes (MAP_NORESERVE)\n", n); exit(4); }
    return (uint8_t *)m;
}

bool read_ranges(FILE *f, unsigned long long n, unsigned k, std::vector<uint64_t> &off, std::vector<uint64_t> &len)
{
    off.resize(k); len.resize(k);
    for (unsigned i = 0; i < k; i++) {
        unsigned long long o, l;
        if (fscanf(f, "%llu %llu", &o, &l) != 2 || o > n || l > n - o) return false;
        off[i] = o; len[i] = l;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of far_sim.cpp\n"); return 2; }
    if (sizeof(size_t) < 8) { printf("far_sim: no 64-bit address space\n"); return 4; }
    const std::vector<uint8_t> data = slurp(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
    unsigned long long n = 0;
    uint8_t *src = nullptr, *dst = nullptr;
    char kind[8];
    char why[512] = "";
    while (fscanf(f, "%7s", kind) == 1) {
        unsigned k;
        if (kind[0] == 'M') {
            if (src || fscanf(f, "%llu", &n) != 1 || !n) return 2;
            src = far_map(n); dst = far_map(n);
            continue;
        }
        if (!src) return 2;
        if (kind[0] == 'Z') {
            unsigned long long o, l;
            unsigned b;
            if (fscanf(f, "%llu %llu %u", &o, &l, &b) != 3 || o > n || l > n - o || b > 255) return 2;
            memset(src + o, (int)b, (size_t)l);
        } else if (kind[0] == 'I') {
            unsigned long long o, l, at;
            if (fscanf(f, "%llu %llu %llu", &o, &l, &at) != 3 || o > n || l > n - o || at > data.size() || l > data.size() - at) return 2;
            memcpy(src + o, data.data() + at, (size_t)l);
        } else if (kind[0] == 'C') {
            std::vector<uint64_t> off, len;
            if (fscanf(f, "%u", &k) != 1 || !k || !read_ranges(f, n, k, off, len)) return 2;
            crc::SegTable T;
            if (T.make(n, k, off.data(), len.data(), crc::kSegment, ErrText{ why, sizeof why })) { fprintf(stderr, "far_sim: %s\n", why); return 2; }
            std::vector<uint32_t> part(T.nsegs + 1, 0xDEADBEEFu), out(k + 1, 0xDEADBEEFu);
            part[T.nsegs] = kCanary32; out[k] = kCanary32;
            Launch L{};
            L.c.buf = src; L.c.part = part.data(); L.c.out = out.data(); L.c.seed = 0;
            T.point(L.c, T.words.data());
            if (T.nsegs) launch(L, kCrcSegments, kBlocks, sizeof(crc::Lds));
            launch(L, kCrcCombine, k, sizeof(crc::CombineLds));
            if (part[T.nsegs] != kCanary32 || out[k] != kCanary32) die("a write behind a buffer's end");
            for (unsigned i = 0; i < k; i++) printf("%08x%s", out[i], i + 1 < k ? " " : "\n");
        } else if (kind[0] == 'F') {
            std::vector<uint64_t> off, len;
            if (fscanf(f, "%u", &k) != 1 || !k || !read_ranges(f, n, k, off, len)) return 2;
            if (dedup::check_ranges(n, k, off.data(), len.data(), ErrText{ why, sizeof why })) { fprintf(stderr, "far_sim: %s\n", why); return 2; }
            std::vector<unsigned long long> o(off.begin(), off.end()), l(len.begin(), len.end());
            const std::vector<unsigned long long> seg0 = units::prefix(k, dedup::kSegment, [&](uint32_t i) { return l[i]; });
            std::vector<unsigned long long> seg_h(seg0[k] + 1, 0xDEADBEEFDEADBEEFull), fp(k + 1, 0xDEADBEEFDEADBEEFull);
            seg_h[seg0[k]] = kCanary64; fp[k] = kCanary64;
            Launch L{};
            L.f = dedup::FpArgs{ src, o.data(), l.data(), seg0.data(), seg_h.data(), fp.data(), (uint32_t)k, seg0[k] };
            if (seg0[k]) launch(L, kFingerprint, kBlocks, 64);
            launch(L, kFpCombine, kBlocks, 64);
            if (seg_h[seg0[k]] != kCanary64 || fp[k] != kCanary64) die("a write behind a buffer's end");
            for (unsigned i = 0; i < k; i++) printf("%016llx%s", fp[i], i + 1 < k ? " " : "\n");
        } else if (kind[0] == 'Q') {
            if (fscanf(f, "%u", &k) != 1 || !k || k > 65536) return 2;
            std::vector<dedup::Pair> pairs(k);
            for (auto &p : pairs) if (fscanf(f, "%llu %llu %llu", &p.a, &p.b, &p.len) != 3 || p.a > n || p.b > n || p.len > n - p.a || p.len > n - p.b) return 2;
            const std::vector<unsigned long long> c0 = units::prefix(k, dedup::kChunk, [&](uint32_t p) { return pairs[p].len; });
            std::vector<uint32_t> ne(c0[k] + 1, 0xDEADBEEFu), eq(k + 1, 0xDEADBEEFu);
            ne[c0[k]] = kCanary32; eq[k] = kCanary32;
            Launch L{};
            L.p = dedup::PairArgs{ src, pairs.data(), c0.data(), ne.data(), eq.data(), (uint32_t)k, c0[k] };
            if (c0[k]) launch(L, kPair, kBlocks, 64);
            launch(L, kVerdict, kBlocks, 64);
            if (ne[c0[k]] != kCanary32 || eq[k] != kCanary32) die("a write behind a buffer's end");
            for (unsigned i = 0; i < k; i++) { if (eq[i] > 1) die("a pair's verdict was not written"); printf("%u%s", eq[i], i + 1 < k ? " " : "\n"); }
        } else if (kind[0] == 'P') {
            unsigned inverse;
            if (fscanf(f, "%u %u", &inverse, &k) != 2 || !k || k > 64) return 2;
            std::vector<uint64_t> src_off(k), dst_off(k), len(k);
            std::vector<uint8_t> elem(k);
            for (unsigned i = 0; i < k; i++) {
                unsigned long long s, d, l, e;
                if (fscanf(f, "%llu %llu %llu %llu", &s, &d, &l, &e) != 4) return 2;
                src_off[i] = s; dst_off[i] = d; len[i] = l; elem[i] = (uint8_t)e;
            }
            if (planes::check_ranges((uint64_t)(uintptr_t)src, n, (uint64_t)(uintptr_t)dst, n, k, src_off.data(), dst_off.data(), len.data(), elem.data(), ErrText{ why, sizeof why })) {
                fprintf(stderr, "far_sim: %s\n", why);
                return 2;
            }
            planes::Table T;
            if (T.make(k, src_off.data(), dst_off.data(), len.data(), elem.data(), planes::kSegment, ErrText{ why, sizeof why })) { fprintf(stderr, "far_sim: %s\n", why); return 2; }
            Launch L{};
            L.inverse = inverse != 0;
            L.pl.src = src; L.pl.dst = dst;
            T.point(L.pl, T.words.data());
            if (T.nsegs) launch(L, kPlanes, kBlocks, planes::lds_bytes(kThreads / 64));
            for (unsigned i = 0; i < k; i++) printf("%08x%s", crc32_of(dst + dst_off[i], (size_t)len[i]), i + 1 < k ? " " : "\n");
            // the destinations cleared, every page they lie in -- and the page on either side -- holds zeros again, as all the others do
            for (unsigned i = 0; i < k; i++) memset(dst + dst_off[i], 0, (size_t)len[i]);
            for (unsigned i = 0; i < k; i++) {
                const unsigned long long lo = dst_off[i] / pg * pg, hi = (dst_off[i] + len[i] + pg - 1) / pg * pg;
                for (unsigned long long b = lo >= pg ? lo - pg : 0; b < (hi + pg <= n ? hi + pg : n); b++)
                    if (dst[b]) { fprintf(stderr, "far_sim: a write outside the destinations, at byte %llu\n", b); return 3; }
            }
        } else return 2;
    }
    fclose(f);
    printf("far_sim: OK\n");
    return 0;
}
