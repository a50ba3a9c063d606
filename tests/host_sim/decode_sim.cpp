// decode_sim.cpp -- the decoder role (nlzm_amd/csrc/nlzm_decode.h) run on the CPU, every lane a fiber (xw_sim.cpp), beside the
// host decoder (nlzm_amd/csrc/nlzm_host_decode.h), which is the specification.  TEST HARNESS ONLY (tests/test_decode_sim.py).
//
//   decode_sim decode  <stream> <out> [size]        one stream; `size`: nothing is stored, only the length found
//   decode_sim blocks  <container> <out> <given>    k streams back to back as k workgroups of one launch; given = 1: block and raw
//                                                   lengths from the host decoder, 0: split by frame hopping + a size-only launch first
//   decode_sim mutants <stream> <seed> <flips> <shard> <nshards>    damaged copies of the stream: role and host decoder must agree
//   decode_sim split   <container>                  dec::split_walk (the body of the device's split kernel) against nlzm_host::split_streams:
//                                                   the container cut at every length, and with edited frame headers, for 1 .. 7 blocks
//
// Every buffer the role sees lies inside a mapping of its own between two PROT_NONE pages, and what is left of the mapping around it is
// a canary that is checked after every launch.  decode / blocks: at an address that is deliberately not aligned, canaries on both
// sides.  mutants / split: the role's promise that reads stay inside [src, src + len) and writes inside [dst, dst + cap) is tested by
// the pages themselves -- every damaged stream is run once with source and destination flush against the page BEHIND them and once
// starting right behind the page IN FRONT (the canary is then on the side where no page can sit).  A read or write outside is a SIGSEGV of
// the harness: this is host code, which is where faults belong.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_decode.h"
#include "../../nlzm_amd/csrc/nlzm_host_decode.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "decode_sim";

namespace {

struct LaunchPack { std::vector<dec::StreamArgs> a; std::vector<dec::StreamResult> r; };
void entry(void *arg)
{
    LaunchPack *P = (LaunchPack *)arg;
    const uint32_t b = xw::block_index();
    dec::decode_role(P->a[b], &P->r[b]);
}
void run(LaunchPack &P)
{
    P.r.assign(P.a.size(), dec::StreamResult{});
    std::vector<unsigned long long> lds(P.a.size(), sizeof(dec::Lds));
    xw::launch((uint32_t)P.a.size(), 64, lds.data(), entry, &P);
}

void print_result(const dec::StreamResult &r)
{
    printf("rc=%d detail=%u out_len=%llu syms=%llu raw_ops=%llu n_literal=%llu n_dict=%llu n_rep=%llu ring_bytes=%llu global_bytes=%llu\n", r.rc, r.detail,
           r.out_len, r.syms, r.raw_ops, r.n_literal, r.n_dict, r.n_rep, r.ring_bytes, r.global_bytes);
}

int cmd_decode(int argc, char **argv)
{
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const bool size_only = argc > 4 && !strcmp(argv[4], "size");
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    nlzm_host::Counts hc;
    nlzm_host::MatchLog log;
    const int hrc = nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb, &hc, &log);
    printf("ring=%u reach=%u flush=%u\n", dec::kRing, dec::kRing, dec::kFlush);
    printf("host rc=%d out_len=%zu syms=%llu raw_ops=%llu n_literal=%llu n_dict=%llu n_rep=%llu\n", hrc, want.size(), (unsigned long long)hc.syms,
           (unsigned long long)hc.raw_ops, (unsigned long long)hc.n_literal, (unsigned long long)hc.n_dict, (unsigned long long)hc.n_rep);
    {   // (distance, length) histogram of the matches longer than 64
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> h;
        for (size_t i = 0; i < log.dv.size(); i++) if (log.lv[i] > 64) h[{ log.dv[i], log.lv[i] }]++;
        size_t shown = 0;
        for (const auto &e : h) { if (shown++ >= 4000) break; printf("longmatch %u %u %u\n", e.first.first, e.first.second, e.second); }
    }
    Guarded src, dst;
    src.make(stream.size(), 1, 0);
    memcpy(src.p(), stream.data(), stream.size());
    dst.make(want.size(), 3, 0x5C);                 // (size only: must stay 0x5C)
    LaunchPack P;
    P.a.push_back(dec::StreamArgs{ src.p(), stream.size(), size_only ? nullptr : dst.p(), size_only ? ~0ull : want.size(), ~0ull });
    run(P);
    print_result(P.r[0]);
    if (!src.intact() || !dst.intact()) { printf("FAIL: canary damaged\n"); return 1; }
    const dec::StreamResult &r = P.r[0];
    if ((r.rc != 0) != (hrc != 0)) { printf("FAIL: role rc %d, host decoder rc %d\n", r.rc, hrc); return 1; }
    if (!hrc) {
        if (r.out_len != want.size()) { printf("FAIL: length\n"); return 1; }
        if (r.syms != hc.syms || r.raw_ops != hc.raw_ops || r.n_literal != hc.n_literal || r.n_dict != hc.n_dict || r.n_rep != hc.n_rep) { printf("FAIL: counters\n"); return 1; }
        unsigned long long want_ring = 0, want_global = 0;      // what the parse says each side serves (nlzm_decode.h, copy)
        for (size_t i = 0; i < log.dv.size(); i++)
            (log.dv[i] + (log.dv[i] < log.lv[i] ? log.lv[i] : 0u) <= dec::kRing ? want_ring : want_global) += log.lv[i];
        if (!size_only && (r.ring_bytes != want_ring || r.global_bytes != want_global)) { printf("FAIL: ring / memory byte counters\n"); return 1; }
        if (size_only) {
            for (size_t i = 0; i < want.size(); i++) if (dst.p()[i] != 0x5C) { printf("FAIL: size-only mode wrote\n"); return 1; }
        } else if (want.size() && memcmp(dst.p(), want.data(), want.size())) { printf("FAIL: bytes differ from the host decoder's\n"); return 1; }
    }
    if (!size_only) spill(argv[3], dst.p(), hrc ? 0 : want.size());
    printf("decode_sim: OK\n");
    return 0;
}

int cmd_blocks(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> blob = slurp(argv[2]);
    const bool given = atoi(argv[4]) != 0;
    Guarded src;
    src.make(blob.size(), 2, 0);
    memcpy(src.p(), blob.data(), blob.size());
    std::vector<size_t> off, len, raw;
    for (size_t pos = 0; pos < blob.size();) {      // the container's split: what the library's hop over the frame headers does
        const size_t l = nlzm_host::stream_length(nlzm_host::Span{ blob.data() + pos, blob.size() - pos });
        if (!l) { printf("FAIL: container does not split\n"); return 1; }
        off.push_back(pos); len.push_back(l); pos += l;
    }
    const size_t k = off.size();
    std::vector<uint8_t> want;
    for (size_t i = 0; i < k; i++) {
        std::vector<uint8_t> o; uint32_t hb, fb;
        if (nlzm_host::decode_stream(nlzm_host::Span{ blob.data() + off[i], len[i] }, o, &hb, &fb)) { printf("FAIL: host decoder rejects block %zu\n", i); return 1; }
        raw.push_back(o.size());
        want.insert(want.end(), o.begin(), o.end());
    }
    std::vector<size_t> got_raw = raw;
    if (!given) {                                   // raw lengths unknown: a size-only launch of all blocks first
        LaunchPack Z;
        for (size_t i = 0; i < k; i++) Z.a.push_back(dec::StreamArgs{ src.p() + off[i], len[i], nullptr, ~0ull, ~0ull });
        run(Z);
        for (size_t i = 0; i < k; i++) { if (Z.r[i].rc) { printf("FAIL: size pass rc %d\n", Z.r[i].rc); return 1; } got_raw[i] = (size_t)Z.r[i].out_len; }
    }
    size_t total = 0;
    for (size_t i = 0; i < k; i++) total += got_raw[i];
    Guarded dst;
    dst.make(total, 5, 0x5C);
    LaunchPack P;
    size_t at = 0;
    for (size_t i = 0; i < k; i++) { P.a.push_back(dec::StreamArgs{ src.p() + off[i], len[i], dst.p() + at, got_raw[i], ~0ull }); at += got_raw[i]; }
    run(P);
    printf("blocks=%zu raw_len_out=", k);
    for (size_t i = 0; i < k; i++) printf("%s%llu", i ? "," : "", P.r[i].out_len);
    printf("\n");
    for (size_t i = 0; i < k; i++) if (P.r[i].rc || P.r[i].out_len != raw[i]) { printf("FAIL: block %zu rc %d\n", i, P.r[i].rc); return 1; }
    if (!src.intact() || !dst.intact()) { printf("FAIL: canary damaged\n"); return 1; }
    if (total != want.size() || memcmp(dst.p(), want.data(), total)) { printf("FAIL: bytes differ\n"); return 1; }
    spill(argv[3], dst.p(), total);
    printf("decode_sim: OK\n");
    return 0;
}

// one damaged stream through both decoders, with source and destination against the page behind them and behind the page in front; returns 0
// when role and host decoder agree both times
int one_mutant(const std::vector<uint8_t> &s, const char *what, size_t idx, long long cap_delta, unsigned *accepted)
{
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    const int hrc = nlzm_host::decode_stream(nlzm_host::Span{ s.data(), s.size() }, want, &hb, &fb);
    const size_t cap = (size_t)((long long)want.size() + cap_delta);
    for (Place place : { kBack, kFront }) {
        const char *where = place == kBack ? "against the page behind" : "behind the page in front";
        Guarded src, dst;
        src.make(s.size(), 0, 0, place);
        if (s.size()) memcpy(src.p(), s.data(), s.size());
        dst.make(cap, 0, 0x5C, place);
        LaunchPack P;
        P.a.push_back(dec::StreamArgs{ src.p(), s.size(), dst.p(), cap, ~0ull });
        run(P);
        const dec::StreamResult &r = P.r[0];
        if (!src.intact() || !dst.intact()) { printf("FAIL %s %zu (%s): canary damaged\n", what, idx, where); return 1; }
        if (cap_delta < 0) {
            if (hrc || r.rc != dec::kErrCapacity) { printf("FAIL %s %zu (%s): dst_cap one short gives rc %d\n", what, idx, where, r.rc); return 1; }
            continue;
        }
        if ((r.rc != 0) != (hrc != 0)) { printf("FAIL %s %zu (%s): role rc %d (detail %u), host decoder rc %d\n", what, idx, where, r.rc, r.detail, hrc); return 1; }
        if (!hrc && (r.out_len != want.size() || (want.size() && memcmp(dst.p(), want.data(), want.size())))) { printf("FAIL %s %zu (%s): accepted, bytes differ\n", what, idx, where); return 1; }
    }
    if (!hrc && cap_delta >= 0) (*accepted)++;
    return 0;
}

uint32_t rng_state;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
void put_be32(std::vector<uint8_t> &s, size_t at, uint32_t v) { s[at] = (uint8_t)(v >> 24); s[at + 1] = (uint8_t)(v >> 16); s[at + 2] = (uint8_t)(v >> 8); s[at + 3] = (uint8_t)v; }

int cmd_mutants(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> s0 = slurp(argv[2]);
    rng_state = (uint32_t)strtoul(argv[3], nullptr, 10);
    const size_t flips = (size_t)atoi(argv[4]), shard = (size_t)atoi(argv[5]), nshards = (size_t)atoi(argv[6]);
    // the list is made whole in every shard (same seed), each runs its share
    struct Mut { std::string what; std::vector<uint8_t> s; long long cap_delta; };
    std::vector<Mut> muts;
    const uint32_t nb0 = s0.size() >= 16 ? nlzm_host::be32(&s0[8]) : 12;
    const size_t head = s0.size() < 64 ? s0.size() : (size_t)(4 + nb0 + 16 < s0.size() ? 4 + nb0 + 16 : s0.size());      // header, first frame's header ... states
    for (size_t i = 0; i < flips; i++) {
        Mut m{ "flip", s0, 0 };
        size_t at;
        if (i % 2 == 0) { at = rnd() % (head < 32 ? head : 32); if (i % 4 == 0 && head > 32) at = 4 + nb0 + rnd() % 16; }   // frame header / states
        else at = rnd() % s0.size();
        if (at >= s0.size()) at = s0.size() - 1;
        m.s[at] ^= (uint8_t)(1u << (rnd() % 8));
        muts.push_back(m);
    }
    for (size_t c = 1; c <= 16 && c <= s0.size(); c++) { Mut m{ "cut", s0, 0 }; m.s.resize(s0.size() - c); muts.push_back(m); }
    for (int v : { 9, 29 }) { Mut m{ "hist_bits", s0, 0 }; m.s[0] = 0; m.s[1] = (uint8_t)v; muts.push_back(m); }
    for (int v : { 11, 21 }) { Mut m{ "frame_bits", s0, 0 }; m.s[2] = 0; m.s[3] = (uint8_t)v; muts.push_back(m); }
    if (s0.size() >= 16) {
        const uint32_t ops = nlzm_host::be32(&s0[4]);
        { Mut m{ "nb", s0, 0 }; put_be32(m.s, 8, 11); muts.push_back(m); }
        { Mut m{ "nr", s0, 0 }; put_be32(m.s, 12, 15); muts.push_back(m); }
        for (uint32_t v : { ops + 1, ops - 1, 0xFFFFFFFFu }) { Mut m{ "num_ops", s0, 0 }; put_be32(m.s, 4, v); muts.push_back(m); }
    }
    muts.push_back(Mut{ "cap", s0, -1 });
    unsigned accepted = 0, ran = 0;
    for (size_t i = shard; i < muts.size(); i += nshards) {
        if (one_mutant(muts[i].s, muts[i].what.c_str(), i, muts[i].cap_delta, &accepted)) return 1;
        ran++;
    }
    printf("mutants=%zu ran=%u accepted=%u\n", muts.size(), ran, accepted);
    printf("decode_sim: OK\n");
    return 0;
}

// dec::split_walk on the `len` bytes at p (which lie flush against a PROT_NONE page) against the host's split of the same span
int one_split(const uint8_t *p, size_t len, uint32_t nblocks, const char *what, size_t idx)
{
    std::vector<uint64_t> hl;
    const size_t found = nlzm_host::split_streams(nlzm_host::Span{ p, len }, nblocks, hl);
    unsigned long long got[8];
    for (auto &g : got) g = 0xA5A5A5A5A5A5A5A5ull;
    uint32_t bad = 0xA5A5A5A5u;
    dec::split_walk(p, len, nblocks, got, &bad);
    const uint32_t want_bad = found < nblocks ? (uint32_t)found + 1 : 0;
    bool ok = bad == want_bad && got[nblocks] == 0xA5A5A5A5A5A5A5A5ull;
    for (uint32_t i = 0; i < nblocks; i++) ok = ok && got[i] == (i < found ? hl[i] : 0);
    if (!ok) {
        printf("FAIL split %s %zu, %u blocks: bad %u (host: %u), lengths", what, idx, nblocks, bad, want_bad);
        for (uint32_t i = 0; i < nblocks; i++) printf(" %llu/%llu", got[i], (unsigned long long)(i < found ? hl[i] : 0));
        printf("\n");
        return 1;
    }
    return 0;
}

int cmd_split(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> blob = slurp(argv[2]);
    std::vector<uint64_t> lens;
    const size_t k = nlzm_host::split_streams(nlzm_host::Span{ blob.data(), blob.size() }, 64, lens);
    if (k != 5) { printf("FAIL: the container holds %zu streams, not five\n", k); return 1; }
    Guarded g;
    g.make(blob.size(), 0, 0, kBack);
    uint8_t *hi = g.p() + blob.size();
    size_t cuts = 0, edits = 0, rejected = 0;
    // cut at every length, the cut's last byte against the page
    for (size_t len = 0; len <= blob.size(); len++) {
        if (len) memcpy(hi - len, blob.data(), len);
        for (uint32_t nb = 1; nb <= 7; nb++) if (one_split(hi - len, len, nb, "cut", len)) return 1;
        cuts++;
    }
    // edited frame headers: the first frame of the third stream (one frame) and of the fifth (several), and the fifth's second frame
    std::vector<size_t> heads;
    size_t at = 0;
    for (size_t i = 0; i < k; i++) {
        if (i == 2 || i == 4) heads.push_back(at + 4);
        if (i == 4) { const size_t second = at + 4 + nlzm_host::be32(&blob[at + 8]) + nlzm_host::be32(&blob[at + 12]); if (second + 12 <= at + lens[i] && nlzm_host::be32(&blob[second])) heads.push_back(second); }
        at += lens[i];
    }
    if (heads.size() != 3) { printf("FAIL: the fifth stream has one frame only\n"); return 1; }
    for (size_t h : heads) {
        const uint32_t nb0 = nlzm_host::be32(&blob[h + 4]), nr0 = nlzm_host::be32(&blob[h + 8]);
        const uint32_t over = (uint32_t)(blob.size() - h - nb0) + 1;         // nb + nr runs one byte over the end
        const struct { const char *what; uint32_t nb, nr; } E[] = { { "nb=0", 0, nr0 }, { "nb=11", 11, nr0 }, { "nb=0xFFFFFFFF", 0xFFFFFFFFu, nr0 }, { "nr=15", nb0, 15 },
            { "nb+nr over the end", nb0, over }, { "nb+nr to the end exactly", nb0, over - 1 }, { "nb=nr=0xFFFFFFFF", 0xFFFFFFFFu, 0xFFFFFFFFu }, { "num_ops=0", nb0, nr0 } };
        for (const auto &e : E) {
            std::vector<uint8_t> m = blob;
            put_be32(m, h + 4, e.nb); put_be32(m, h + 8, e.nr);
            if (!strcmp(e.what, "num_ops=0")) put_be32(m, h, 0);
            memcpy(hi - m.size(), m.data(), m.size());
            std::vector<uint64_t> hl;
            if (nlzm_host::split_streams(nlzm_host::Span{ m.data(), m.size() }, 5, hl) < 5) rejected++;
            for (uint32_t nb = 1; nb <= 7; nb++) if (one_split(hi - m.size(), m.size(), nb, e.what, h)) return 1;
            edits++;
        }
    }
    if (!g.intact()) { printf("FAIL: canary damaged\n"); return 1; }
    printf("split: streams=%zu bytes=%zu cuts=%zu edits=%zu rejected=%zu\n", k, blob.size(), cuts, edits, rejected);
    printf("decode_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "split")) return cmd_split(argc, argv);
    if (argc >= 4 && !strcmp(argv[1], "decode")) return cmd_decode(argc, argv);
    if (argc == 5 && !strcmp(argv[1], "blocks")) return cmd_blocks(argc, argv);
    if (argc == 7 && !strcmp(argv[1], "mutants")) return cmd_mutants(argc, argv);
    fprintf(stderr, "usage: see the head of decode_sim.cpp\n");
    return 2;
}
