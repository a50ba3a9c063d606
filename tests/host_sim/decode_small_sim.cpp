// decode_small_sim.cpp -- the decoder role at the ring of decode_small_kernel (nlzm_amd/csrc/nlzm_decode_small.hip: 16 KiB), run on the CPU,
// every lane a fiber, beside the host decoder.  TEST HARNESS ONLY (tests/test_decode_small_ring_sim.py; built by the Makefile with
// -DNLZM_DEC_RING=16384).  The buffers, the launch and the result line are decode_sim.cpp's, which this file takes in whole (its main renamed).
//
//   decode_small_sim decode  <stream> <out> <misalign>      one stream, the destination `misalign` bytes off a 16-byte boundary, between
//                                                           PROT_NONE pages: bytes and counters against the host decoder, both byte counters
//                                                           against its parse, and mid_bytes = match bytes from 16 KiB + 1 .. 64 KiB back
//   decode_small_sim prefix  <stream> <cuts> <shard> <nshards>   prefix mode at `cuts` offsets spread over the stream's output, the destination's
//                                                           last byte flush against a PROT_NONE page
//   decode_small_sim mutants <stream> <seed> <flips> <count>     the first `count` damaged streams of decode_sim's list: rc AND detail are the
//                                                           host decoder's
#define main decode_sim_main
#include "decode_sim.cpp"
#undef main

namespace {

int small_decode(char **argv)
{
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const size_t mis = (size_t)atoi(argv[4]);
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    nlzm_host::Counts hc;
    nlzm_host::MatchLog log;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb, &hc, &log)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    printf("ring=%u flush=%u misalign=%zu\n", dec::kRing, dec::kFlush, mis);
    Guarded src, dst;
    src.make(stream.size(), 1, 0);
    memcpy(src.p(), stream.data(), stream.size());
    dst.make(want.size(), mis, 0x5C);
    if (((uintptr_t)dst.p() & 15u) != (mis & 15u)) { printf("FAIL: the destination is not misaligned by %zu\n", mis); return 1; }
    LaunchPack P;
    P.a.push_back(dec::StreamArgs{ src.p(), stream.size(), dst.p(), want.size(), ~0ull });
    run(P);
    print_result(P.r[0]);
    const dec::StreamResult &r = P.r[0];
    if (!src.intact() || !dst.intact()) { printf("FAIL: canary damaged\n"); return 1; }
    if (r.rc || r.out_len != want.size()) { printf("FAIL: rc / length\n"); return 1; }
    if (r.syms != hc.syms || r.raw_ops != hc.raw_ops || r.n_literal != hc.n_literal || r.n_dict != hc.n_dict || r.n_rep != hc.n_rep) { printf("FAIL: counters\n"); return 1; }
    unsigned long long want_ring = 0, want_global = 0, mid = 0;     // what the parse says each side serves (nlzm_decode.h, copy)
    for (size_t i = 0; i < log.dv.size(); i++) {
        const unsigned long long reach = log.dv[i] + (log.dv[i] < log.lv[i] ? log.lv[i] : 0u);
        (reach <= dec::kRing ? want_ring : want_global) += log.lv[i];
        if (reach > 16384 && reach <= 65536) mid += log.lv[i];
    }
    printf("mid_bytes=%llu\n", mid);
    if (r.ring_bytes != want_ring || r.global_bytes != want_global) { printf("FAIL: ring / memory byte counters\n"); return 1; }
    if (want.size() && memcmp(dst.p(), want.data(), want.size())) { printf("FAIL: bytes differ from the host decoder's\n"); return 1; }
    spill(argv[3], dst.p(), want.size());
    printf("decode_sim: OK\n");
    return 0;
}

int small_prefix(char **argv)
{
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const size_t cuts = (size_t)atoi(argv[3]), shard = (size_t)atoi(argv[4]), nshards = (size_t)atoi(argv[5]);
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    size_t ran = 0;
    for (size_t c = shard; c < cuts; c += nshards) {
        // spread over the output, never a multiple of 16 twice running, the first at 1 and the last at the stream's end
        const size_t cut = c + 1 == cuts ? want.size() : c == 0 ? 1 : want.size() * c / (cuts - 1) + (c % 5);
        Guarded src, dst;
        src.make(stream.size(), 1, 0);
        memcpy(src.p(), stream.data(), stream.size());
        dst.make(cut, 0, 0x5C, kBack);
        LaunchPack P;
        dec::StreamArgs a{ src.p(), stream.size(), dst.p(), cut, ~0ull };
        a.flags = dec::kPrefix;
        P.a.push_back(a);
        run(P);
        const dec::StreamResult &r = P.r[0];
        if (!src.intact() || !dst.intact()) { printf("FAIL: canary damaged at cut %zu\n", cut); return 1; }
        if (r.rc || r.out_len != cut || memcmp(dst.p(), want.data(), cut)) { printf("FAIL: prefix of %zu bytes: rc %d, out_len %llu\n", cut, r.rc, r.out_len); return 1; }
        printf("cut %zu ok\n", cut);
        ran++;
    }
    printf("prefix: cuts=%zu ran=%zu\n", cuts, ran);
    printf("decode_sim: OK\n");
    return 0;
}

// The list is cmd_mutants' of decode_sim.cpp, made the same way from the same seed (the flips, the cuts, the header edits); of it the first
// `count`.  A stream both decoders reject must be rejected for the SAME reason: the role's detail is the host decoder's code, negated.
int small_mutants(char **argv)
{
    const std::vector<uint8_t> s0 = slurp(argv[2]);
    rng_state = (uint32_t)strtoul(argv[3], nullptr, 10);
    const size_t flips = (size_t)atoi(argv[4]), count = (size_t)atoi(argv[5]);
    std::vector<std::vector<uint8_t>> muts;
    const uint32_t nb0 = s0.size() >= 16 ? nlzm_host::be32(&s0[8]) : 12;
    const size_t head = s0.size() < 64 ? s0.size() : (size_t)(4 + nb0 + 16 < s0.size() ? 4 + nb0 + 16 : s0.size());
    for (size_t i = 0; i < flips; i++) {
        std::vector<uint8_t> m = s0;
        size_t at;
        if (i % 2 == 0) { at = rnd() % (head < 32 ? head : 32); if (i % 4 == 0 && head > 32) at = 4 + nb0 + rnd() % 16; }
        else at = rnd() % s0.size();
        if (at >= s0.size()) at = s0.size() - 1;
        m[at] ^= (uint8_t)(1u << (rnd() % 8));
        muts.push_back(m);
    }
    for (size_t c = 1; c <= 16 && c <= s0.size(); c++) { std::vector<uint8_t> m = s0; m.resize(s0.size() - c); muts.push_back(m); }
    unsigned ran = 0, accepted = 0, rejected = 0;
    for (size_t i = 0; i < muts.size() && i < count; i++) {
        const std::vector<uint8_t> &s = muts[i];
        std::vector<uint8_t> want;
        uint32_t hb = 0, fb = 0;
        const int hrc = nlzm_host::decode_stream(nlzm_host::Span{ s.data(), s.size() }, want, &hb, &fb);
        Guarded src, dst;
        src.make(s.size(), 0, 0, kBack);
        if (s.size()) memcpy(src.p(), s.data(), s.size());
        dst.make(want.size(), 0, 0x5C, kBack);
        LaunchPack P;
        P.a.push_back(dec::StreamArgs{ src.p(), s.size(), dst.p(), want.size(), ~0ull });
        run(P);
        const dec::StreamResult &r = P.r[0];
        if (!src.intact() || !dst.intact()) { printf("FAIL mutant %zu: canary damaged\n", i); return 1; }
        if (hrc) {
            if (r.rc != dec::kErrFormat || (int)r.detail != -hrc) { printf("FAIL mutant %zu: role rc %d detail %u, host decoder rc %d\n", i, r.rc, r.detail, hrc); return 1; }
            rejected++;
        } else {
            if (r.rc || r.out_len != want.size() || (want.size() && memcmp(dst.p(), want.data(), want.size()))) { printf("FAIL mutant %zu: accepted by the host decoder, role rc %d\n", i, r.rc); return 1; }
            accepted++;
        }
        ran++;
    }
    printf("mutants=%zu ran=%u accepted=%u rejected=%u\n", muts.size(), ran, accepted, rejected);
    printf("decode_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "decode")) return small_decode(argv);
    if (argc == 6 && !strcmp(argv[1], "prefix")) return small_prefix(argv);
    if (argc == 6 && !strcmp(argv[1], "mutants")) return small_mutants(argv);
    fprintf(stderr, "usage: see the head of decode_small_sim.cpp\n");
    return 2;
}
