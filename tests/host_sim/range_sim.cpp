// range_sim.cpp -- what the range reader adds to the device code, run on the CPU with every lane a fiber (xw_sim.cpp): the decoder role's
// prefix mode (nlzm_amd/csrc/nlzm_decode.h, dec::kPrefix) beside the host decoder, and the gather role (nlzm_amd/csrc/nlzm_range.h) beside
// memcpy; and the plan the host makes of a call (nlzm_amd/csrc/nlzm_read_plan.h), carried out with memcpy.  TEST HARNESS ONLY
// (tests/test_range_sim.py).
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
//   range_sim plan                       a container of six blocks of raw lengths 5, 0, 7, 3, 0, 4: the plan of every single range inside its 19
//                                        bytes and of every ordered pair of them, held against what the definitions say (need, direct, scratch,
//                                        pieces) and carried out -- the needed blocks "decoded" by memcpy to where the plan places them, the
//                                        packed pieces moved by memcpy, destination and scratch buffer between canaries; the plan's errors;
//                                        and a handful of the plans with the real gather role moving the packed pieces
//
// Every comparison is made here; a read or write that leaves a mapping ends the harness with SIGSEGV: host code, where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_decode.h"
#include "../../nlzm_amd/csrc/nlzm_host_decode.h"
#include "../../nlzm_amd/csrc/nlzm_range.h"
#include "../../nlzm_amd/csrc/nlzm_read_plan.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <malloc.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "range_sim";

namespace {

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
// one launch of the pieces (offsets from `src` and `dst`), packed as the library's host side packs them (nlzm_read_plan.h: empty ones are left out)
void run_gather(const std::vector<range::PlanPiece> &pieces, const uint8_t *src, uint8_t *dst, uint32_t threads, uint32_t blocks)
{
    std::vector<range::Piece> p;
    std::vector<unsigned long long> c0;
    const unsigned long long nchunks = range::pack_pieces(pieces, src, dst, range::kChunk, p, c0);
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
    run_gather({ range::PlanPiece{ (uint64_t)(s - g_src.lo), (uint64_t)(d - g_dst.lo), n } }, g_src.lo, g_dst.lo, 64 * (1 + shape % 4), 1 + shape % 3);
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
            std::vector<range::PlanPiece> pieces(k);
            size_t at = room - total;                                      // the destinations end at the guard page
            std::vector<uint8_t> expect(room, kPoison);
            unsigned empty = 0, big = 0;
            for (unsigned i = 0; i < k; i++) {
                pieces[i] = range::PlanPiece{ so[i], at, len[i] };
                memcpy(expect.data() + at, g_data.data() + so[i], len[i]);
                at += len[i];
                empty += !len[i]; big += len[i] > range::kChunk;
            }
            run_gather(pieces, g_src.lo, g_dst.lo, 128, 3);
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

// ---- the plan -------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kBlocks = 6;
const uint64_t kRaw[kBlocks] = { 5, 0, 7, 3, 0, 4 };      // empty blocks in the middle and beside a boundary
constexpr uint64_t kTotal = 19;
uint8_t content_byte(uint64_t i) { return (uint8_t)(37 * i + 11); }

// One set of ranges: the plan against the definitions, written out here block by block without the plan's own walk, then carried out.
// with_role: the packed pieces are moved by the gather role in the fiber simulator instead of memcpy.
bool plan_case(const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, bool with_role)
{
    const uint32_t nr = (uint32_t)off.size();
    uint64_t start[kBlocks + 1] = { 0 }, sum = 0;
    for (uint32_t b = 0; b < kBlocks; b++) start[b + 1] = start[b] + kRaw[b];
    for (uint32_t r = 0; r < nr; r++) sum += len[r];
    range::Plan P;
    char why[512] = "";
    const int rc = range::make_plan(P, kBlocks, kRaw, nr, off.data(), len.data(), sum, ErrText{ why, sizeof why });
    auto bad = [&](const char *what) {
        printf("FAIL: %s; ranges", what);
        for (uint32_t r = 0; r < nr; r++) printf(" (%llu, %llu)", (unsigned long long)off[r], (unsigned long long)len[r]);
        printf("\n");
        return false;
    };
    if (rc || P.total != kTotal || P.dst_len != sum) return bad("make_plan fails, or its totals are wrong");
    // need[b]: the furthest byte any range wants of b; 0 for blocks no range touches or of raw length 0.  direct: exactly one range uses
    // the block and starts at or before its first byte.  scratch: the sum of need[b] over the needed blocks that are not direct.
    uint64_t scratch = 0;
    for (uint32_t b = 0; b < kBlocks; b++) {
        uint64_t need = 0;
        uint32_t users = 0, first_user = 0;
        for (uint32_t r = 0; r < nr; r++) {
            const uint64_t lo = off[r], hi = off[r] + len[r];
            if (!len[r] || !kRaw[b] || hi <= start[b] || lo >= start[b + 1]) continue;
            const uint64_t want = (hi < start[b + 1] ? hi : start[b + 1]) - start[b];
            if (want > need) need = want;
            if (!users++) first_user = r;
        }
        const bool direct = users == 1 && off[first_user] <= start[b];
        if (P.need[b] != need) return bad("need[b] is not the furthest byte a range wants of the block");
        if ((P.direct[b] != 0) != direct) return bad("a block is direct that should not be, or the other way round");
        if (need && !direct) scratch += need;
    }
    if (P.scratch != scratch) return bad("scratch is not the sum of need[b] over the needed blocks that are not direct");
    // the pieces: one per range and non-direct block it intersects, in the ranges' order -- so none of a direct block
    std::vector<range::PlanPiece> want;
    uint64_t at = 0;
    for (uint32_t r = 0; r < nr; r++) {
        const uint64_t lo = off[r], hi = off[r] + len[r];
        for (uint32_t b = 0; b < kBlocks; b++) {
            if (!len[r] || !kRaw[b] || hi <= start[b] || lo >= start[b + 1] || P.direct[b]) continue;
            const uint64_t from = lo > start[b] ? lo : start[b], to = hi < start[b + 1] ? hi : start[b + 1];
            want.push_back(range::PlanPiece{ P.place[b] + (from - start[b]), at + (from - lo), to - from });
        }
        at += len[r];
    }
    if (want.size() != P.pieces.size()) return bad("the pieces are not one per range and non-direct block it intersects");
    for (size_t i = 0; i < want.size(); i++)
        if (want[i].scratch_off != P.pieces[i].scratch_off || want[i].dst_off != P.pieces[i].dst_off || want[i].len != P.pieces[i].len) return bad("a piece is not where the definitions put it");
    // carried out: "decode" the first need[b] bytes of every needed block to place[b], then move the packed pieces
    Canaried dst, scr;
    dst.make((size_t)sum, 3, 0x5C);
    scr.make((size_t)P.scratch, 5, 0xC5);
    for (uint32_t b = 0; b < kBlocks; b++) {
        if (!P.need[b]) continue;
        if (P.place[b] + P.need[b] > (P.direct[b] ? sum : P.scratch)) return bad("a block is placed outside its buffer");
        uint8_t *to = (P.direct[b] ? dst.p() : scr.p()) + P.place[b];
        for (uint64_t i = 0; i < P.need[b]; i++) to[i] = content_byte(start[b] + i);
    }
    if (with_role) run_gather(P.pieces, scr.p(), dst.p(), 128, 2);
    else {
        std::vector<range::Piece> hp;
        std::vector<unsigned long long> c0;
        const unsigned long long nchunks = range::pack_pieces(P.pieces, scr.p(), dst.p(), range::kChunk, hp, c0);
        if (c0.size() != hp.size() + 1 || c0.back() != nchunks) return bad("the chunk table has not one entry per packed piece and the total behind them");
        for (size_t i = 0; i < hp.size(); i++) {
            if (!hp[i].len || c0[i + 1] - c0[i] != (hp[i].len + range::kChunk - 1) / range::kChunk) return bad("a packed piece is empty, or its chunks do not cover it");
            memcpy(hp[i].dst, hp[i].src, (size_t)hp[i].len);
        }
    }
    at = 0;
    for (uint32_t r = 0; r < nr; r++)
        for (uint64_t i = 0; i < len[r]; i++, at++)
            if (dst.p()[at] != content_byte(off[r] + i)) return bad("the destination is not the ranges' bytes back to back");
    if (!dst.intact() || !scr.intact()) return bad("a byte outside the destination or the scratch buffer changed");
    return true;
}

int cmd_plan()
{
    std::vector<uint64_t> so, sl;                   // every range inside the container, the empty ones and off == total among them
    for (uint64_t o = 0; o <= kTotal; o++) for (uint64_t l = 0; o + l <= kTotal; l++) { so.push_back(o); sl.push_back(l); }
    unsigned long long plans = 0, role_plans = 0, errors = 0;
    for (size_t i = 0; i < so.size(); i++, plans++) if (!plan_case({ so[i] }, { sl[i] }, false)) return 1;
    for (size_t i = 0; i < so.size(); i++)
        for (size_t j = 0; j < so.size(); j++, plans++) if (!plan_case({ so[i], so[j] }, { sl[i], sl[j] }, false)) return 1;
    // the shared packing meets the role
    const std::vector<std::vector<uint64_t>> role[] = { { { 3, 0 }, { 10, 19 } }, { { 0 }, { 19 } }, { { 4 }, { 9 } }, { { 6, 5 }, { 1, 7 } }, { { 11, 2 }, { 8, 12 } },
                                                        { { 0, 5, 12 }, { 5, 7, 7 } }, { { 18, 0, 7 }, { 1, 0, 6 } } };
    for (const auto &c : role) { if (!plan_case(c[0], c[1], true)) return 1; role_plans++; }
    // the errors
    range::Plan P;
    char why[512];
    const ErrText err{ why, sizeof why };
    const uint64_t o1 = ~0ull, l1 = 2, o2 = kTotal + 1, l2 = 0, o3 = 2, l3 = 9, wrap[2] = { ~0ull, 2 };
    const struct { const char *what; uint32_t nblocks; const uint64_t *raw, *off, *len; uint64_t cap; int want; } kErr[] = {
        { "off = 2^64 - 1, len = 2", kBlocks, kRaw, &o1, &l1, ~0ull, NLZM_HIP_E_ARG },
        { "off = total + 1, len = 0", kBlocks, kRaw, &o2, &l2, ~0ull, NLZM_HIP_E_ARG },
        { "raw lengths that wrap 64 bits", 2, wrap, &o3, &l3, ~0ull, NLZM_HIP_E_ARG },
        { "dst_cap one below the sum", kBlocks, kRaw, &o3, &l3, l3 - 1, NLZM_HIP_E_CAPACITY },
    };
    for (const auto &e : kErr) {
        why[0] = 0;
        const int rc = range::make_plan(P, e.nblocks, e.raw, 1, e.off, e.len, e.cap, err);
        if (rc != e.want || !why[0]) { printf("FAIL: %s: code %d (%s), expected %d and a message\n", e.what, rc, why, e.want); return 1; }
        errors++;
    }
    if (range::make_plan(P, kBlocks, kRaw, 1, &o3, &l3, l3, err)) { printf("FAIL: dst_cap equal to the sum is refused\n"); return 1; }
    printf("plans=%llu role_plans=%llu errors=%llu\n", plans, role_plans, errors);
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
    if (argc == 2 && !strcmp(argv[1], "plan")) return cmd_plan();
    fprintf(stderr, "usage: see the head of range_sim.cpp\n");
    return 2;
}
