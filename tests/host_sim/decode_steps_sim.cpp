// decode_steps_sim.cpp -- the STEPPING form of the decoder role (dec::decode_role_steps, nlzm_amd/csrc/nlzm_decode.h) run on the CPU, every
// lane a fiber (xw_sim.cpp), beside the one-shot role and the host decoder.  TEST HARNESS ONLY (tests/test_decode_steps_sim.py).
//
//   decode_steps_sim steps   <stream> <out> <frames> <misalign> [size]   `frames` frames a launch to the end; every launch's bytes so far and, at the
//                                                                        end, every counter against the one-shot role's.  size: nothing is stored
//   decode_steps_sim targets <stream> <stride> <shard> <nshards>         a target sweep: 0, 1, every stride-th byte, n - 1, n, n + 1
//   decode_steps_sim more    <stream> <stride> <shard> <nshards> <near>  kMore: len cut within 16 bytes of every frame header and at every stride-th
//                                                                        offset elsewhere, raised afterwards; the same cuts without the flag.
//                                                                        near = 0: every cut decoded from the stream's first byte; 1: from the saved
//                                                                        state one frame in front of the last frame that lies inside the cut
//   decode_steps_sim mutants <stream> <seed> <flips> <shard> <nshards>   the first `flips` single-bit flips of decode_sim's generator, stepped one
//                                                                        frame at a time: rc and detail are the one-shot role's, rc the host decoder's
//   decode_steps_sim blocks  <container> <out>                           k streams back to back stepped with per-block targets
//
// As in decode_sim.cpp every buffer the role sees -- source, destination AND the state record -- lies in a mapping of its own between two
// PROT_NONE pages with canaries in what the pages enclose beside it; the sources of `more` and `mutants` lie flush against the page behind them.
#define NLZM_SIM 1
#include "../../nlzm_amd/csrc/nlzm_decode.h"
#include "../../nlzm_amd/csrc/nlzm_host_decode.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

using namespace nlzm;
using namespace simkit;

const char simkit::kProgram[] = "decode_steps_sim";

namespace {

struct LaunchPack { std::vector<dec::StreamArgs> a; std::vector<dec::StreamResult> r; bool steps = true; };
void entry(void *arg)
{
    LaunchPack *P = (LaunchPack *)arg;
    const uint32_t b = xw::block_index();
    if (P->steps) dec::decode_role_steps(P->a[b], &P->r[b]);
    else dec::decode_role(P->a[b], &P->r[b]);
}
void run(LaunchPack &P)
{
    P.r.assign(P.a.size(), dec::StreamResult{});
    std::vector<unsigned long long> lds(P.a.size(), sizeof(dec::Lds));
    xw::launch((uint32_t)P.a.size(), 64, lds.data(), entry, &P);
}
dec::StreamResult one_shot(const uint8_t *src, size_t len, uint8_t *dst, unsigned long long cap)
{
    LaunchPack P;
    P.steps = false;
    P.a.push_back(dec::StreamArgs{ src, len, dst, cap, ~0ull });
    run(P);
    return P.r[0];
}
// the state record of one stream, between canaries (16-byte aligned, as the library's allocation is)
struct State {
    Guarded g;
    State() { g.make(dec::kStateBytes, 16, 0); }
    dec::StepState *p() { return (dec::StepState *)g.p(); }
};
// one launch of the stepping form on one stream
dec::StreamResult step(const uint8_t *src, size_t len, uint8_t *dst, unsigned long long cap, State &T, bool resume, bool more, uint32_t max_frames, unsigned long long target)
{
    LaunchPack P;
    dec::StreamArgs a{ src, len, dst, cap, ~0ull };
    a.flags = (resume ? dec::kResume : 0u) | (more ? dec::kMore : 0u);
    a.state = T.p(); a.max_frames = max_frames; a.target = target;
    P.a.push_back(a);
    run(P);
    return P.r[0];
}

void print_result(const char *tag, const dec::StreamResult &r)
{
    printf("%s rc=%d detail=%u why=%u out_len=%llu syms=%llu raw_ops=%llu n_literal=%llu n_dict=%llu n_rep=%llu ring_bytes=%llu global_bytes=%llu\n", tag, r.rc, r.detail,
           r.why, r.out_len, r.syms, r.raw_ops, r.n_literal, r.n_dict, r.n_rep, r.ring_bytes, r.global_bytes);
}
bool same_counts(const dec::StreamResult &a, const dec::StreamResult &b)
{
    return a.out_len == b.out_len && a.syms == b.syms && a.raw_ops == b.raw_ops && a.n_literal == b.n_literal && a.n_dict == b.n_dict && a.n_rep == b.n_rep &&
           a.ring_bytes == b.ring_bytes && a.global_bytes == b.global_bytes;
}

// a well-formed stream's frame headers: head[k] the stream offset of frame k's header (the last entry: the terminator's), and, by stepping
// the host decoder's output, nothing else -- the output boundaries come from the role itself, one frame a launch (cmd_steps checks them)
std::vector<size_t> frame_heads(const std::vector<uint8_t> &s)
{
    std::vector<size_t> h;
    size_t pos = 4;
    for (;;) {
        h.push_back(pos);
        if (pos + 4 > s.size() || !nlzm_host::be32(&s[pos])) break;
        pos += (size_t)nlzm_host::be32(&s[pos + 4]) + nlzm_host::be32(&s[pos + 8]);
    }
    return h;
}

int cmd_steps(int argc, char **argv)
{
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const uint32_t per = (uint32_t)atoi(argv[4]);
    const size_t misalign = (size_t)atoi(argv[5]);
    const bool size_only = argc > 6 && !strcmp(argv[6], "size");
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    printf("ring=%u state_bytes=%u frames=%zu\n", dec::kRing, dec::kStateBytes, frame_heads(stream).size() - 1);
    Guarded src, dst, ref;
    src.make(stream.size(), 1, 0);
    memcpy(src.p(), stream.data(), stream.size());
    dst.make(want.size(), misalign, 0x5C);
    ref.make(want.size(), misalign, 0x5C);
    const dec::StreamResult one = one_shot(src.p(), stream.size(), size_only ? nullptr : ref.p(), size_only ? ~0ull : want.size());
    print_result("oneshot", one);
    if (one.rc) { printf("FAIL: the one-shot role rejects the stream\n"); return 1; }
    State T;
    dec::StreamResult r{};
    unsigned launches = 0;
    unsigned long long cycles_before = 0, window_before = 0, copy_before = 0;
    for (bool resume = false;; resume = true) {
        r = step(src.p(), stream.size(), size_only ? nullptr : dst.p(), size_only ? ~0ull : want.size(), T, resume, false, per, ~0ull);
        launches++;
        printf("launch %u rc=%d why=%u out_len=%llu\n", launches, r.rc, r.why, r.out_len);
        if (!src.intact() || !dst.intact() || !T.g.intact()) { printf("FAIL: canary damaged\n"); return 1; }
        if (r.rc != dec::kPaused && r.rc != dec::kOk) { printf("FAIL: launch %u rc %d detail %u\n", launches, r.rc, r.detail); return 1; }
        // the cycle counters run on through the state like the others: never below the launch before, and the whole never below its parts
        if (r.cycles < cycles_before || r.cycles < r.window_cycles + r.copy_cycles || r.window_cycles < window_before || r.copy_cycles < copy_before) {
            printf("FAIL: launch %u cycles %llu (before: %llu), window %llu (%llu), copy %llu (%llu)\n", launches, r.cycles, cycles_before, r.window_cycles, window_before, r.copy_cycles, copy_before); return 1;
        }
        // (one wave alone never waits, so the simulator's clock -- scheduler sweeps -- stands still: the harness adds 1,000 cycles to the saved
        //  record after every pause, and the launch that resumes from it must report them on top of its own)
        if (r.cycles < 1000ull * (launches - 1)) { printf("FAIL: launch %u reports %llu cycles: the state's %llu are not in it\n", launches, r.cycles, 1000ull * (launches - 1)); return 1; }
        cycles_before = r.cycles; window_before = r.window_cycles; copy_before = r.copy_cycles;
        if (r.rc == dec::kPaused) { if (T.p()->cycles != r.cycles) { printf("FAIL: the saved cycles are not the reported ones\n"); return 1; } T.p()->cycles += 1000; cycles_before += 1000; }
        if (r.out_len > want.size()) { printf("FAIL: length\n"); return 1; }
        if (size_only) { for (size_t i = 0; i < want.size(); i++) if (dst.p()[i] != 0x5C) { printf("FAIL: size-only mode wrote\n"); return 1; } }
        else {
            if (r.out_len && memcmp(dst.p(), want.data(), r.out_len)) { printf("FAIL: bytes after launch %u differ\n", launches); return 1; }
            for (size_t i = r.out_len; i < want.size(); i++) if (dst.p()[i] != 0x5C) { printf("FAIL: launch %u wrote beyond what it reports\n", launches); return 1; }
        }
        if (r.rc == dec::kOk) break;
        if (r.why != dec::kWhyFrames) { printf("FAIL: paused for reason %u\n", r.why); return 1; }
        if (launches > 100000) { printf("FAIL: no end\n"); return 1; }
    }
    print_result("stepped", r);
    printf("cycles stepped=%llu oneshot=%llu\n", r.cycles, one.cycles);
    if (!same_counts(r, one)) { printf("FAIL: the stepped decode's counters are not the one-shot's\n"); return 1; }
    if (T.p()->valid == dec::kStateValid) { printf("FAIL: a finished decode left a state to resume from\n"); return 1; }
    if (!size_only) spill(argv[3], dst.p(), want.size());
    printf("launches=%u\n", launches);
    printf("decode_steps_sim: OK\n");
    return 0;
}

// the output boundaries of a well-formed stream: bound[k] = bytes decoded in front of frame k's header (one frame a launch, size only)
std::vector<unsigned long long> boundaries(const uint8_t *src, size_t len)
{
    std::vector<unsigned long long> b{ 0 };
    State T;
    for (bool resume = false;; resume = true) {
        const dec::StreamResult r = step(src, len, nullptr, ~0ull, T, resume, false, 1, ~0ull);
        if (r.rc == dec::kOk) { if (r.out_len != b.back()) b.push_back(r.out_len); break; }
        if (r.rc != dec::kPaused) { printf("FAIL: boundaries rc %d\n", r.rc); exit(1); }
        b.push_back(r.out_len);
    }
    return b;
}

int cmd_targets(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const size_t stride = (size_t)atoi(argv[3]), shard = (size_t)atoi(argv[4]), nshards = (size_t)atoi(argv[5]);
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    const size_t n = want.size();
    Guarded src, dst;
    src.make(stream.size(), 3, 0);
    memcpy(src.p(), stream.data(), stream.size());
    const std::vector<unsigned long long> bound = boundaries(src.p(), stream.size());      // bound.back() == n, with the last frame's end
    std::set<unsigned long long> targets{ 0, 1, n - 1, n, n + 1 };
    for (size_t t = 0; t <= n; t += stride) targets.insert(t);
    unsigned ran = 0, ended = 0;
    size_t idx = 0;
    for (unsigned long long t : targets) {
        if (idx++ % nshards != shard) continue;
        dst.make(n, 7, 0x5C);
        State T;
        dec::StreamResult r = step(src.p(), stream.size(), dst.p(), n, T, false, false, 0, t);
        // the first frame boundary at or above the target; the last boundary is the stream's end, where the terminator ends the decode
        size_t k = 0;
        while (k + 1 < bound.size() && bound[k] < t) k++;
        const bool at_end = k + 1 == bound.size();
        if (at_end ? r.rc != dec::kOk : (r.rc != dec::kPaused || r.why != dec::kWhyTarget)) { printf("FAIL target %llu: rc %d why %u\n", t, r.rc, r.why); return 1; }
        if (r.out_len != bound[k]) { printf("FAIL target %llu: stopped at %llu, not at %llu\n", t, r.out_len, bound[k]); return 1; }
        if (r.out_len && memcmp(dst.p(), want.data(), r.out_len)) { printf("FAIL target %llu: bytes\n", t); return 1; }
        if (!at_end) {
            // a second launch with the same target does not run the stream: not a symbol, not a byte
            const dec::StreamResult r2 = step(src.p(), stream.size(), dst.p(), n, T, true, false, 0, t);
            if (r2.rc != dec::kPaused || r2.why != dec::kWhyTarget || !same_counts(r2, r)) { printf("FAIL target %llu: the second launch ran the stream\n", t); return 1; }
            r = step(src.p(), stream.size(), dst.p(), n, T, true, false, 0, ~0ull);
            if (r.rc != dec::kOk) { printf("FAIL target %llu: going on, rc %d\n", t, r.rc); return 1; }
        } else ended++;
        if (r.out_len != n || memcmp(dst.p(), want.data(), n)) { printf("FAIL target %llu: the whole decode's bytes\n", t); return 1; }
        if (!src.intact() || !dst.intact() || !T.g.intact()) { printf("FAIL: canary damaged\n"); return 1; }
        ran++;
    }
    printf("targets=%zu ran=%u ended=%u boundaries=%zu\n", targets.size(), ran, ended, bound.size());
    printf("decode_steps_sim: OK\n");
    return 0;
}

int cmd_more(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> stream = slurp(argv[2]);
    const size_t stride = (size_t)atoi(argv[3]), shard = (size_t)atoi(argv[4]), nshards = (size_t)atoi(argv[5]);
    const bool near = atoi(argv[6]) != 0;
    std::vector<uint8_t> want;
    uint32_t hb = 0, fb = 0;
    if (nlzm_host::decode_stream(nlzm_host::Span{ stream.data(), stream.size() }, want, &hb, &fb)) { printf("FAIL: the host decoder rejects the stream\n"); return 1; }
    const size_t n = want.size(), L = stream.size();
    const std::vector<size_t> head = frame_heads(stream);
    const size_t nframes = head.size() - 1;
    std::set<size_t> cuts;
    for (size_t h : head) for (size_t c = h > 16 ? h - 16 : 0; c <= h + 16 && c < L; c++) cuts.insert(c);
    for (size_t c = 0; c < L; c += stride) cuts.insert(c);
    Guarded whole;
    whole.make(L, 0, 0, kBack);
    memcpy(whole.p(), stream.data(), L);
    // near: the state at rest in front of every frame header, saved by a decode of one frame a launch (saved[k]: k frames done), which gives
    // the output boundaries too
    std::vector<std::vector<uint8_t>> saved;
    std::vector<unsigned long long> bound;
    if (near) {
        Guarded d0;
        d0.make(n, 15, 0x5C);
        State T;
        bound.push_back(0);
        saved.push_back(std::vector<uint8_t>());    // (0 frames done: a decode from the first byte)
        for (bool resume = false;; resume = true) {
            const dec::StreamResult r = step(whole.p(), L, d0.p(), n, T, resume, false, 1, ~0ull);
            if (r.rc != dec::kPaused && r.rc != dec::kOk) { printf("FAIL: the whole stream, rc %d\n", r.rc); return 1; }
            if (r.out_len != bound.back()) bound.push_back(r.out_len);
            if (r.rc == dec::kOk) break;
            saved.push_back(std::vector<uint8_t>(T.g.p(), T.g.p() + dec::kStateBytes));
        }
    } else bound = boundaries(whole.p(), L);
    if (bound.back() != n || bound.size() != nframes + 1) { printf("FAIL: boundaries\n"); return 1; }
    unsigned ran = 0;
    size_t idx = 0;
    for (size_t c : cuts) {
        if (idx++ % nshards != shard) continue;
        // frames that lie wholly inside the first c bytes (frame k ends where frame k + 1's header begins)
        size_t inside = 0;
        while (inside < nframes && head[inside + 1] <= c) inside++;
        Guarded src, dst;
        src.make(c, 0, 0, kBack);                   // the cut's last byte flush against the page behind it
        if (c) memcpy(src.p(), stream.data(), c);
        dst.make(n, 15, 0x5C);
        State T;
        const size_t from = near && inside > 1 && inside - 1 < saved.size() ? inside - 1 : 0;     // frames done where this cut's decode starts
        if (from) { memcpy(T.g.p(), saved[from].data(), dec::kStateBytes); memcpy(dst.p(), want.data(), bound[from]); }
        dec::StreamResult r = step(src.p(), c, dst.p(), n, T, from != 0, true, 0, ~0ull);
        if (r.rc != dec::kPaused || r.why != dec::kWhyInput) { printf("FAIL cut %zu: rc %d why %u detail %u\n", c, r.rc, r.why, r.detail); return 1; }
        if (T.p()->frames != inside || r.out_len != (inside < bound.size() ? bound[inside] : n)) { printf("FAIL cut %zu: paused after %llu frames / %llu bytes, %zu frames lie inside\n", c, T.p()->frames, r.out_len, inside); return 1; }
        if (!src.intact() || !dst.intact() || !T.g.intact()) { printf("FAIL cut %zu: canary damaged\n", c); return 1; }
        std::vector<uint8_t> at_rest(T.g.p(), T.g.p() + dec::kStateBytes);
        // the input has arrived: on to the end (the whole stream lies against its own page)
        r = step(whole.p(), L, dst.p(), n, T, true, true, 0, ~0ull);
        if (r.rc != dec::kOk || r.out_len != n || memcmp(dst.p(), want.data(), n)) { printf("FAIL cut %zu: going on, rc %d, %llu bytes\n", c, r.rc, r.out_len); return 1; }
        if (!whole.intact() || !dst.intact() || !T.g.intact()) { printf("FAIL cut %zu: canary damaged\n", c); return 1; }
        // the same cut without kMore: today's error -- near: from the state the cut's decode came to rest in; else from the first byte, both forms
        State T2;
        const bool again = near && c >= 8;
        if (again) memcpy(T2.g.p(), at_rest.data(), dec::kStateBytes);
        const dec::StreamResult e1 = step(src.p(), c, dst.p(), n, T2, again, false, 0, ~0ull), e0 = again ? e1 : one_shot(src.p(), c, dst.p(), n);
        const uint32_t detail = c < 8 ? 1u : 3u;
        if (e1.rc != dec::kErrFormat || e1.detail != detail || e0.rc != dec::kErrFormat || e0.detail != detail) {
            printf("FAIL cut %zu without kMore: rc %d detail %u (one-shot: rc %d detail %u)\n", c, e1.rc, e1.detail, e0.rc, e0.detail); return 1;
        }
        if (!src.intact() || !dst.intact() || !T2.g.intact()) { printf("FAIL cut %zu: canary damaged\n", c); return 1; }
        ran++;
    }
    printf("more: bytes=%zu frames=%zu cuts=%zu ran=%u\n", L, nframes, cuts.size(), ran);
    printf("decode_steps_sim: OK\n");
    return 0;
}

uint32_t rng_state;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int cmd_mutants(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> s0 = slurp(argv[2]);
    rng_state = (uint32_t)strtoul(argv[3], nullptr, 10);
    const size_t flips = (size_t)atoi(argv[4]), shard = (size_t)atoi(argv[5]), nshards = (size_t)atoi(argv[6]);
    size_t ran = 0;
    // decode_sim's generator (cmd_mutants there), flip for flip
    const uint32_t nb0 = s0.size() >= 16 ? nlzm_host::be32(&s0[8]) : 12;
    const size_t head = s0.size() < 64 ? s0.size() : (size_t)(4 + nb0 + 16 < s0.size() ? 4 + nb0 + 16 : s0.size());
    unsigned accepted = 0, paused = 0;
    for (size_t i = 0; i < flips; i++) {
        std::vector<uint8_t> s = s0;
        size_t at;
        if (i % 2 == 0) { at = rnd() % (head < 32 ? head : 32); if (i % 4 == 0 && head > 32) at = 4 + nb0 + rnd() % 16; }
        else at = rnd() % s0.size();
        if (at >= s0.size()) at = s0.size() - 1;
        s[at] ^= (uint8_t)(1u << (rnd() % 8));
        if (i % nshards != shard) continue;         // (the list is made whole in every shard, each runs its share)
        ran++;
        std::vector<uint8_t> want;
        uint32_t hb = 0, fb = 0;
        const int hrc = nlzm_host::decode_stream(nlzm_host::Span{ s.data(), s.size() }, want, &hb, &fb);
        const size_t cap = want.size();
        Guarded src, dst, ref;
        src.make(s.size(), 0, 0, kBack);
        memcpy(src.p(), s.data(), s.size());
        dst.make(cap, 0, 0x5C, kBack);
        ref.make(cap, 0, 0x5C, kBack);
        const dec::StreamResult one = one_shot(src.p(), s.size(), ref.p(), cap);
        State T;
        dec::StreamResult r{};
        for (bool resume = false;; resume = true) {
            r = step(src.p(), s.size(), dst.p(), cap, T, resume, false, 1, ~0ull);
            if (!src.intact() || !dst.intact() || !T.g.intact()) { printf("FAIL flip %zu: canary damaged\n", i); return 1; }
            if (r.rc != dec::kPaused) break;
            paused++;
        }
        if (r.rc != one.rc || r.detail != one.detail || (r.rc != 0) != (hrc != 0)) { printf("FAIL flip %zu: stepped rc %d detail %u, one-shot rc %d detail %u, host decoder rc %d\n", i, r.rc, r.detail, one.rc, one.detail, hrc); return 1; }
        if (!hrc) {
            if (r.out_len != want.size() || (want.size() && memcmp(dst.p(), want.data(), want.size()))) { printf("FAIL flip %zu: accepted, bytes differ\n", i); return 1; }
            accepted++;
        }
    }
    printf("mutants=%zu ran=%zu accepted=%u pauses=%u\n", flips, ran, accepted, paused);
    printf("decode_steps_sim: OK\n");
    return 0;
}

int cmd_blocks(int argc, char **argv)
{
    (void)argc;
    const std::vector<uint8_t> blob = slurp(argv[2]);
    Guarded src;
    src.make(blob.size(), 2, 0);
    memcpy(src.p(), blob.data(), blob.size());
    std::vector<size_t> off, len, raw, at;
    std::vector<uint8_t> want;
    for (size_t pos = 0; pos < blob.size();) {
        const size_t l = nlzm_host::stream_length(nlzm_host::Span{ blob.data() + pos, blob.size() - pos });
        if (!l) { printf("FAIL: container does not split\n"); return 1; }
        std::vector<uint8_t> o; uint32_t hb, fb;
        if (nlzm_host::decode_stream(nlzm_host::Span{ blob.data() + pos, l }, o, &hb, &fb)) { printf("FAIL: host decoder rejects a block\n"); return 1; }
        off.push_back(pos); len.push_back(l); raw.push_back(o.size()); at.push_back(want.size()); pos += l;
        want.insert(want.end(), o.begin(), o.end());
    }
    const size_t k = off.size();
    if (k != 5) { printf("FAIL: the container holds %zu streams, not five\n", k); return 1; }
    Guarded dst;
    dst.make(want.size(), 5, 0x5C);
    std::vector<State> T(k);
    // round 1: targets 0 (not launched, as the library has it), 1, half, the end, 0; round 2: every block to its end
    const unsigned long long target[5] = { 0, 1, raw[2] / 2, ~0ull, 0 };
    std::vector<unsigned long long> done(k, 0);
    std::vector<int> fin(k, 0), started(k, 0);
    for (int round = 0; round < 2; round++) {
        LaunchPack P;
        std::vector<size_t> who;
        for (size_t i = 0; i < k; i++) {
            const unsigned long long t = round ? ~0ull : target[i];
            if (fin[i] || done[i] >= t) continue;
            dec::StreamArgs a{ src.p() + off[i], len[i], dst.p() + at[i], raw[i], ~0ull };
            a.flags = started[i] ? dec::kResume : 0u; a.state = T[i].p(); a.target = t;
            P.a.push_back(a); who.push_back(i);
        }
        run(P);
        for (size_t j = 0; j < who.size(); j++) {
            const size_t i = who[j];
            const dec::StreamResult &r = P.r[j];
            if (r.rc != dec::kOk && !(r.rc == dec::kPaused && r.why == dec::kWhyTarget)) { printf("FAIL: block %zu rc %d why %u\n", i, r.rc, r.why); return 1; }
            started[i] = 1; done[i] = r.out_len; fin[i] = r.rc == dec::kOk;
            if (!T[i].g.intact()) { printf("FAIL: canary damaged\n"); return 1; }
        }
        printf("round %d launched=%zu done=", round, who.size());
        for (size_t i = 0; i < k; i++) printf("%s%llu", i ? "," : "", done[i]);
        printf("\n");
        if (!src.intact() || !dst.intact()) { printf("FAIL: canary damaged\n"); return 1; }
        // no block writes into another's range: what a block has not decoded yet is still the fill, what it has is the input's
        for (size_t i = 0; i < k; i++) {
            if (done[i] > raw[i] || (done[i] && memcmp(dst.p() + at[i], want.data() + at[i], done[i]))) { printf("FAIL: block %zu bytes\n", i); return 1; }
            for (size_t b = done[i]; b < raw[i]; b++) if (dst.p()[at[i] + b] != 0x5C) { printf("FAIL: block %zu's range written beyond what it decoded\n", i); return 1; }
        }
    }
    for (size_t i = 0; i < k; i++) if (!fin[i] || done[i] != raw[i]) { printf("FAIL: block %zu not finished\n", i); return 1; }
    spill(argv[3], dst.p(), want.size());
    printf("decode_steps_sim: OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 6 && !strcmp(argv[1], "steps")) return cmd_steps(argc, argv);
    if (argc == 6 && !strcmp(argv[1], "targets")) return cmd_targets(argc, argv);
    if (argc == 7 && !strcmp(argv[1], "more")) return cmd_more(argc, argv);
    if (argc == 7 && !strcmp(argv[1], "mutants")) return cmd_mutants(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "blocks")) return cmd_blocks(argc, argv);
    fprintf(stderr, "usage: see the head of decode_steps_sim.cpp\n");
    return 2;
}
