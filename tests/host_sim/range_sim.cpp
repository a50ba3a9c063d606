// range_sim.cpp -- what the range reader adds to the device code, run on the CPU with every lane a fiber (xw_sim.cpp): the decoder role's
// prefix mode (nlzm_amd/csrc/nlzm_decode.h, dec::kPrefix) beside the host decoder, and the gather role (nlzm_amd/csrc/nlzm_range.h) beside
// memcpy.  TEST HARNESS ONLY (tests/test_range_sim.py).
//
//   range_sim prefix <stream> <caps>     one decode per line "<flags> <cap>" of <caps>, the destination misaligned by cap % 16 between two
//                                        canary regions that start right at dst + cap.  flags 1 (kPrefix): rc 0, out_len = min(cap, raw), the
//                                        bytes the host decoder's first out_len, the ring / memory byte counters what the host decoder's parse
//                                        says a decode cut at cap serves from each side.  flags 0 and cap < raw: kErrCapacity.
//                                        Prints per line "cap out_len global_bytes cut_global" (cut_global: memory-served bytes of the op that
//                                        was cut) and the sums.
//   range_sim gather <cases>             lines of <cases>:
//       S <lo> <hi> <shard> <nshards>    every source misalignment 0 .. 15 x destination misalignment 0 .. 15 x length lo .. hi (the lengths
//                                        dealt to shards), each four times: both sides behind the front guard page at their misalignment, the
//                                        source / the destination / both flush against the PROT_NONE page behind
//       M <seed> <k>                     one launch of k pieces of mixed sizes, empty ones among them, sources anywhere in a buffer between
//                                        guard pages, destinations back to back up to the guard page behind
//       G                                prints the chunk size
//
// Every comparison is made here; a read or write that leaves a mapping ends the harness with SIGSEGV: host code, where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_decode.h"
#include "../../nlzm_amd/csrc/nlzm_host_decode.h"
#include "../../nlzm_amd/csrc/nlzm_range.h"

#include <malloc.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

using namespace nlzm;

namespace {

constexpr size_t kCanary = 4096;
constexpr uint8_t kPoison = 0xA5;

// a buffer of n bytes at a chosen misalignment between two canaries (as decode_sim.cpp's)
struct Canaried {
    std::vector<uint8_t> mem;
    size_t off = 0, n = 0;
    void make(size_t bytes, size_t misalign, uint8_t fill)
    {
        n = bytes;
        mem.assign(2 * kCanary + bytes + 64, kPoison);
        off = kCanary + ((64 - ((uintptr_t)mem.data() + kCanary) % 64) % 64) + misalign;
        memset(mem.data() + off, fill, bytes);
    }
    uint8_t *p() { return mem.data() + off; }
    bool intact() const
    {
        for (size_t i = 0; i < off; i++) if (mem[i] != kPoison) return false;
        for (size_t i = off + n; i < mem.size(); i++) if (mem[i] != kPoison) return false;
        return true;
    }
};

// `bytes` usable bytes (rounded up to pages) between two PROT_NONE pages (as crc_sim.cpp's)
struct Guarded {
    uint8_t *lo = nullptr, *hi = nullptr;
    void make(size_t bytes)
    {
        const size_t pg = (size_t)sysconf(_SC_PAGESIZE), n = (bytes + pg - 1) / pg * pg;
        uint8_t *m = (uint8_t *)mmap(nullptr, n + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED || mprotect(m, pg, PROT_NONE) || mprotect(m + pg + n, pg, PROT_NONE)) { fprintf(stderr, "range_sim: no guarded buffer\n"); exit(2); }
        lo = m + pg; hi = m + pg + n;
    }
};

std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    b.resize((size_t)sz);
    if (sz && fread(b.data(), 1, (size_t)sz, f) != (size_t)sz) { fprintf(stderr, "short read\n"); exit(2); }
    fclose(f);
    return b;
}

uint32_t rng_state = 1;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// ---- prefix mode ------------------------------------------------------------------------------------------------------------------
struct DecPack { dec::StreamArgs a; dec::StreamResult r; };
void dec_entry(void *arg) { DecPack *P = (DecPack *)arg; dec::decode_role(P->a, &P->r); }

int cmd_prefix(char **argv)
{
    const std::vector<uint8_t> stream = slurp(argv[2]);
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    nlzm_host::MatchLog log;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb, nullptr, &log)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    const unsigned long long raw = want.size();
    printf("ring=%u raw=%llu\n", dec::kRing, raw);
    Canaried src;
    src.make(stream.size(), 1, 0);
    memcpy(src.p(), stream.data(), stream.size());
    FILE *f = fopen(argv[3], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    unsigned flags;
    unsigned long long cap, runs = 0, sum_global = 0, sum_cut = 0;
    while (fscanf(f, "%u %llu", &flags, &cap) == 2) {
        Canaried dst;
        dst.make((size_t)cap, (size_t)(cap % 16), 0x5C);
        DecPack P;
        P.a = dec::StreamArgs{ src.p(), stream.size(), dst.p(), cap, ~0ull };
        P.a.flags = flags;
        P.r = dec::StreamResult{};
        const unsigned long long lds = sizeof(dec::Lds);
        xw::launch(1, 64, &lds, dec_entry, &P);
        const dec::StreamResult &r = P.r;
        if (!src.intact() || !dst.intact()) { printf("FAIL cap %llu: a byte outside [dst, dst + cap) or round the stream changed\n", cap); return 1; }
        if (!(flags & dec::kPrefix)) {
            if (cap < raw ? r.rc != dec::kErrCapacity : (r.rc != 0 || r.out_len != raw)) { printf("FAIL cap %llu without the flag: rc %d out_len %llu\n", cap, r.rc, r.out_len); return 1; }
            continue;
        }
        const unsigned long long stop = cap < raw ? cap : raw;
        if (r.rc != 0 || r.out_len != stop) { printf("FAIL cap %llu: rc %d out_len %llu, expected 0 and %llu\n", cap, r.rc, r.out_len, stop); return 1; }
        if (stop && memcmp(dst.p(), want.data(), (size_t)stop)) { printf("FAIL cap %llu: bytes differ from the host decoder's\n", cap); return 1; }
        // what the parse says each side serves when the decode is cut at `stop` (nlzm_decode.h, copy): a match that starts below stop counts
        // with the bytes of it that lie below stop
        unsigned long long want_ring = 0, want_global = 0, cut_global = 0;
        for (size_t i = 0; i < log.dv.size() && log.at[i] < stop; i++) {
            const bool cut = log.at[i] + log.lv[i] > stop;
            const uint32_t lv = cut ? (uint32_t)(stop - log.at[i]) : log.lv[i];
            const bool in_ring = log.dv[i] + (log.dv[i] < lv ? lv : 0u) <= dec::kRing;
            (in_ring ? want_ring : want_global) += lv;
            if (cut && !in_ring) cut_global += lv;
        }
        if (r.ring_bytes != want_ring || r.global_bytes != want_global) {
            printf("FAIL cap %llu: ring / memory byte counters %llu / %llu, the parse says %llu / %llu\n", cap, r.ring_bytes, r.global_bytes, want_ring, want_global);
            return 1;
        }
        printf("%llu %llu %llu %llu\n", cap, r.out_len, r.global_bytes, cut_global);
        runs++; sum_global += r.global_bytes; sum_cut += cut_global;
    }
    fclose(f);
    printf("runs=%llu sum_global=%llu sum_cut_global=%llu\n", runs, sum_global, sum_cut);
    printf("range_sim: OK\n");
    return 0;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------
struct GatherPack { range::Args a; uint32_t threads; };
void gather_entry(void *arg)
{
    const GatherPack *P = (const GatherPack *)arg;
    const uint32_t wpb = P->threads / 64;
    range::gather_role(P->a, (unsigned long long)xw::block_index() * wpb + xw::wave(), (unsigned long long)xw::sim().nblocks * wpb);
}
// one launch of the pieces, as the library's host side sets it up (nlzm_hip_range.cpp: empty pieces are left out)
void run_gather(const std::vector<range::Piece> &pieces, uint32_t threads, uint32_t blocks)
{
    std::vector<range::Piece> p;
    std::vector<unsigned long long> c0;
    unsigned long long nchunks = 0;
    for (const range::Piece &q : pieces) {
        if (!q.len) continue;
        p.push_back(q); c0.push_back(nchunks);
        nchunks += (q.len + range::kChunk - 1) / range::kChunk;
    }
    c0.push_back(nchunks);
    if (!nchunks) return;                           // zero pieces: no launch
    GatherPack P{ range::Args{ p.data(), c0.data(), (uint32_t)p.size(), nchunks }, threads };
    std::vector<unsigned long long> lds(blocks, 0);
    xw::launch(blocks, threads, lds.data(), gather_entry, &P);
}

Guarded g_src, g_dst;
std::vector<uint8_t> g_data;

// one piece: the bytes must arrive, and the 64 bytes on either side of the destination (as far as they are mapped) must stay
bool one_piece(uint8_t *s, uint8_t *d, size_t n, unsigned shape)
{
    memcpy(s, g_data.data(), n);
    uint8_t *wlo = d - g_dst.lo > 64 ? d - 64 : g_dst.lo, *whi = g_dst.hi - (d + n) > 64 ? d + n + 64 : g_dst.hi;
    memset(wlo, kPoison, (size_t)(whi - wlo));
    run_gather({ range::Piece{ s, d, n } }, 64 * (1 + shape % 4), 1 + shape % 3);
    for (uint8_t *q = wlo; q < d; q++) if (*q != kPoison) return false;
    for (uint8_t *q = d + n; q < whi; q++) if (*q != kPoison) return false;
    return !n || !memcmp(d, g_data.data(), n);
}

int cmd_gather(char **argv)
{
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    const size_t room = 6 * range::kChunk + 4096;
    g_src.make(room); g_dst.make(room);
    g_data.resize(room);
    for (auto &b : g_data) b = (uint8_t)(rnd() >> 3);
    char kind[8];
    unsigned long long cases = 0;
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'G') { printf("%llu\n", range::kChunk); continue; }
        if (kind[0] == 'S') {
            unsigned long long lo, hi, shard, nshards;
            if (fscanf(f, "%llu %llu %llu %llu", &lo, &hi, &shard, &nshards) != 4 || hi + 16 > room) return 2;
            for (unsigned long long n = lo + shard; n <= hi; n += nshards)
                for (unsigned sa = 0; sa < 16; sa++)
                    for (unsigned da = 0; da < 16; da++) {
                        const unsigned shape = (unsigned)(n + sa + 3 * da);
                        uint8_t *sf = g_src.lo + sa, *df = g_dst.lo + da, *sb = g_src.hi - n, *db = g_dst.hi - n;
                        const bool ok = one_piece(sf, df, n, shape) && one_piece(sb, df, n, shape + 1) && one_piece(sf, db, n, shape + 2) && one_piece(sb, db, n, shape + 3);
                        if (!ok) { printf("FAIL: length %llu, source misaligned by %u, destination by %u\n", n, sa, da); return 1; }
                        cases += 4;
                    }
        } else if (kind[0] == 'M') {
            unsigned seed, k;
            if (fscanf(f, "%u %u", &seed, &k) != 2) return 2;
            rng_state = seed;
            memcpy(g_src.lo, g_data.data(), room);
            memset(g_dst.lo, kPoison, room);
            std::vector<size_t> len(k), so(k);
            size_t total = 0;
            for (unsigned i = 0; i < k; i++) {
                const unsigned c = rnd() % 10;
                len[i] = c < 2 ? 0 : c < 7 ? rnd() % 100 : c < 9 || i % 16 != 3 ? rnd() % 600 : (size_t)range::kChunk - 20 + rnd() % 40;
                if (i == 7) len[i] = 2 * range::kChunk + 5;
                if (total + len[i] > room) len[i] = 0;
                so[i] = rnd() % (room - len[i] + 1);
                total += len[i];
            }
            if (k) { so[0] = 0; so[k - 1] = room - len[k - 1]; }          // (the buffer's first byte, and its last)
            std::vector<range::Piece> pieces(k);
            size_t at = room - total;                                      // the destinations end at the guard page
            std::vector<uint8_t> expect(room, kPoison);
            unsigned empty = 0, big = 0;
            for (unsigned i = 0; i < k; i++) {
                pieces[i] = range::Piece{ g_src.lo + so[i], g_dst.lo + at, len[i] };
                memcpy(expect.data() + at, g_data.data() + so[i], len[i]);
                at += len[i];
                empty += !len[i]; big += len[i] > range::kChunk;
            }
            run_gather(pieces, 128, 3);
            if (memcmp(g_dst.lo, expect.data(), room)) { printf("FAIL: %u pieces in one launch\n", k); return 1; }
            printf("pieces=%u empty=%u longer_than_a_chunk=%u bytes=%zu\n", k, empty, big, total);
            cases++;
        } else return 2;
    }
    fclose(f);
    printf("cases=%llu\n", cases);
    printf("range_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    // (thousands of small launches: the fibers' stacks come from the heap and stay there, instead of a mapping made and dropped per fiber)
    mallopt(M_MMAP_THRESHOLD, 4 << 20);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    if (argc == 4 && !strcmp(argv[1], "prefix")) return cmd_prefix(argv);
    if (argc == 3 && !strcmp(argv[1], "gather")) return cmd_gather(argv);
    fprintf(stderr, "usage: see the head of range_sim.cpp\n");
    return 2;
}
