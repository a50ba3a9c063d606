// xw_probe.h -- a probe role for nlzm_amd/csrc/xw.h: every primitive of the execution layer applied to inputs from a table, every lane's
// result written to a table.  TEST CODE ONLY.  The SAME text is the gfx950 kernel (xw_probe.hip) and the fiber simulation
// (tests/host_sim/xw_probe_sim.cpp); tests/xw_model.py makes the input table and says, from the definitions in xw.h's comments, what
// the output table must hold (tests/test_xw_sim.py, tests/test_gpu_xw.py).
//
// The probe never waits: no spin, no hand-off between workgroups.  Everything is decided within a thread, within a wave, within the
// one workgroup after block_sync, or across two launches (phase 0 writes the words in `g`, phase 1 reads them).  One workgroup of 256.
//
// Every index below is a function of the two counts in the table's header, the lane and the thread; the launcher and the harness check
// the three buffers' sizes against those counts before the role runs.
#pragma once

#include "../../nlzm_amd/csrc/xw.h"

namespace xwp {

enum : uint32_t { kMagic = 0x78775031u, kThreads = 256 };
enum : uint32_t { opBallot = 1, opAny, opReadlane, opReadlane64, opReadfirst, opReadfirst64, opShfl, opShfl64, opShflUp, opShflUp64, opScanMax,
                  opScanAdd, opScanMinI32, opLaneBelow, opCount };

// ---- the input table (uint32 words) --------------------------------------------------------------------------------------------------
// header: magic, ncases, nexit, strict; then ncases + nexit records; then four words per thread
constexpr uint32_t kHead = 16;
constexpr uint32_t kRec = 4 + 3 * 64;               // op, a (d or l), fill, flags; lo[64]; hi[64]; src[64]
constexpr uint32_t in_thread(uint32_t nc, uint32_t ne) { return kHead + (nc + ne) * kRec; }     // x, min64 lo, min64 hi, y
constexpr uint32_t in_words(uint32_t nc, uint32_t ne) { return in_thread(nc, ne) + 4 * kThreads; }

// ---- the output table of phase 0 -----------------------------------------------------------------------------------------------------
constexpr uint32_t oId = 0;                                                     // lane, wave, thread per thread
constexpr uint32_t oCase = oId + 3 * kThreads;                                  // per case and lane: lo, hi
constexpr uint32_t o_lds(uint32_t nc) { return oCase + nc * 128; }
enum : uint32_t { lInc = 0, lIncFinal = 256, lAdd = 260, lOr = 264, lMax = 268, lAdd64 = 272, lMin64 = 276, lRtWave = 284, lRtBlock = 540, lWords = 796 };
constexpr uint32_t o_agent(uint32_t nc) { return o_lds(nc) + lWords; }          // 16 per thread: A[4] B[4] ld32 ld64[2] cas hit, miss, contended
constexpr uint32_t o_misc(uint32_t nc) { return o_agent(nc) + 16 * kThreads; }  // 4 per thread: opaque, tick ok, clock ok, 0xC0FFEE
constexpr uint32_t o_exit(uint32_t nc) { return o_misc(nc) + 4 * kThreads; }    // per pattern (2), exit case and lane: lo, hi
constexpr uint32_t out_words(uint32_t nc, uint32_t ne) { return o_exit(nc) + 2 * ne * 128; }
// ... and of phase 1: 32 per thread
constexpr uint32_t out2_words() { return 32 * kThreads; }

// ---- the words shared between the launches ------------------------------------------------------------------------------------------
enum : uint32_t { gA = 0, gB = 1024, g32 = 2048, g64 = 2304, gOr = 2816, gAdd64 = 2820, gCas = 2824, gCont = 3080, gWords = 3088 };

enum : uint32_t { kSentinel = 0xDEADBEEFu };        // what the host fills the output tables with

struct Args { const uint32_t *in; uint32_t *out; uint32_t *g; uint32_t phase; };
struct Lds {
    unsigned long long add64[2], min64[4];
    uint32_t inc, add[4], orw[4], mx[4], rt[kThreads];
};

// one cross-lane primitive on one record; o: 128 words
XW_FN void run_case(const uint32_t *rec, uint32_t *o)
{
    const uint32_t op = rec[0], a = rec[1], fill = rec[2], l = xw::lane();
    const uint32_t lo = rec[4 + l], hi = rec[68 + l], src = rec[132 + l];
    const unsigned long long v = ((unsigned long long)hi << 32) | lo;
    unsigned long long r = 0;
    switch (op) {
    case opBallot: r = xw::ballot(lo != 0); break;
    case opAny: r = xw::any(lo != 0) ? 1 : 0; break;
    case opReadlane: r = xw::readlane(lo, a); break;
    case opReadlane64: r = xw::readlane64(v, a); break;
    case opReadfirst: r = xw::readfirst(lo); break;
    case opReadfirst64: r = xw::readfirst64(v); break;
    case opShfl: r = xw::shfl(lo, src); break;
    case opShfl64: r = xw::shfl64(v, src); break;
    case opShflUp: r = xw::shfl_up(lo, a); break;
    case opShflUp64: r = xw::shfl_up64(v, a); break;
    case opScanMax: r = xw::scan_max(lo); break;
    case opScanAdd: r = xw::scan_add(lo); break;
    case opScanMinI32: r = (uint32_t)xw::scan_min_i32((int32_t)lo); break;
    case opLaneBelow: r = xw::lane_below(lo, fill); break;
    default: r = 0xBAD0BAD0BAD0BAD0ull; break;
    }
    o[2 * l] = (uint32_t)r;
    o[2 * l + 1] = (uint32_t)(r >> 32);
}

XW_FN void phase0(const Args &A)
{
    const uint32_t *in = A.in;
    uint32_t *out = A.out, *g = A.g;
    const uint32_t nc = in[1], ne = in[2], strict = in[3];
    const uint32_t t = xw::thread(), l = xw::lane(), w = xw::wave();
    const unsigned long long t0 = xw::tick(), c0 = xw::clock100();
    out[oId + 3 * t] = l; out[oId + 3 * t + 1] = w; out[oId + 3 * t + 2] = t;

    // the cross-lane primitives, all lanes live: the waves share the cases out
    for (uint32_t c = w; c < nc; c += kThreads / 64) run_case(in + kHead + c * kRec, out + oCase + c * 128);

    // (each once, in uniform flow, between checked operations: nothing is disturbed)
    xw::pause(); xw::pause_long(); xw::acquire_agent(); xw::after_poll();

    // LDS
    const uint32_t *ti = in + in_thread(nc, ne) + 4 * t;
    const uint32_t x = ti[0], mlo = ti[1], mhi = ti[2], y = ti[3];
    Lds *L = xw::lds<Lds>();
    uint32_t *ol = out + o_lds(nc);
    if (t == 0) {
        L->inc = 0;
        for (int k = 0; k < 4; k++) { L->add[k] = 0; L->orw[k] = 0; L->mx[k] = 0; L->min64[k] = ~0ull; }
        L->add64[0] = 0; L->add64[1] = 0;
    }
    xw::block_sync();
    ol[lInc + t] = xw::lds_inc(&L->inc);
    xw::lds_add(&L->add[t & 3], x);
    xw::lds_or(&L->orw[t & 3], y);
    xw::lds_max(&L->mx[t & 3], x);
    xw::lds_add64(&L->add64[t & 1], 0xFFFFFFFFull);
    xw::lds_min64(&L->min64[t & 3], ((unsigned long long)mhi << 32) | mlo);
    xw::lds_st(&L->rt[t], x ^ 0x5A5A5A5Au);
    xw::wave_sync();
    ol[lRtWave + t] = xw::lds_ld(&L->rt[(t & ~63u) | ((t + 1) & 63u)]);      // the lane above, of this wave
    xw::block_sync();
    ol[lRtBlock + t] = xw::lds_ld(&L->rt[(t + 64) & 255u]);                  // the same lane of the next wave
    if (t < 4) {
        ol[lAdd + t] = xw::lds_ld(&L->add[t]); ol[lOr + t] = xw::lds_ld(&L->orw[t]); ol[lMax + t] = xw::lds_ld(&L->mx[t]);
        ol[lMin64 + 2 * t] = (uint32_t)L->min64[t]; ol[lMin64 + 2 * t + 1] = (uint32_t)(L->min64[t] >> 32);
    }
    if (t < 2) { ol[lAdd64 + 2 * t] = (uint32_t)L->add64[t]; ol[lAdd64 + 2 * t + 1] = (uint32_t)(L->add64[t] >> 32); }
    if (t == 0) ol[lIncFinal] = xw::lds_ld(&L->inc);

    // agent-scope words: every thread its own slots.  The four variables are overwritten right behind the first 16-byte store and stored
    // again: the sequence st_agent128's s_nop is there for.
    uint32_t *oa = out + o_agent(nc) + 16 * t;
    uint32_t a = x, b = x ^ 0x11111111u, c = ~x, d = x + 0x01010101u;
    xw::st_agent128(g + gA + 4 * t, a, b, c, d);
    a = ~a; b += 0x9E3779B9u; c ^= 0xFFFF0000u; d = d * 5u + 1u;
    xw::st_agent128(g + gB + 4 * t, a, b, c, d);
    xw::st_agent(g + g32 + t, y);
    xw::st_agent64((unsigned long long *)(g + g64) + t, ((unsigned long long)~y << 32) | y);
    xw::drain();
    const xw::u32x4 ra = xw::ld_agent128(g + gA + 4 * t), rb = xw::ld_agent128(g + gB + 4 * t);
    oa[0] = ra.x; oa[1] = ra.y; oa[2] = ra.z; oa[3] = ra.w;
    oa[4] = rb.x; oa[5] = rb.y; oa[6] = rb.z; oa[7] = rb.w;
    oa[8] = xw::ld_agent(g + g32 + t);
    const unsigned long long r64 = xw::ld_agent64((const unsigned long long *)(g + g64) + t);
    oa[9] = (uint32_t)r64; oa[10] = (uint32_t)(r64 >> 32);
    xw::atomic_or_agent(g + gOr + (t & 3), y);
    xw::atomic_add64_agent((unsigned long long *)(g + gAdd64) + (t & 1), 0xFFFFFFFFull);
    oa[11] = xw::cas_agent(g + gCas + t, 0u, 1000u + t);        // the word is 0: a hit
    oa[12] = xw::cas_agent(g + gCas + t, 0u, 5u);               // ... and is not any more: a miss
    oa[13] = xw::cas_agent(g + gCont, 0u, t + 1);               // all threads on one word: one wins

    uint32_t *om = out + o_misc(nc) + 4 * t;
    om[0] = xw::opaque(x);
    om[1] = xw::tick() >= t0 ? 1u : 0u;
    om[2] = xw::clock100() >= c0 ? 1u : 0u;
    om[3] = 0xC0FFEEu;

    // exited lanes: in wave 1 lanes 40 .. 63 leave, in wave 2 every third lane (0, 3, ...) does; the others run the exit cases.  A case
    // whose flags say that a live lane would read an exited one is left out when the table asks for it (the simulator refuses such a read).
    if (w != 1 && w != 2) return;
    const uint32_t pat = w - 1;
    if (pat == 0 ? l >= 40 : l % 3 == 0) return;
    for (uint32_t c = 0; c < ne; c++) {
        const uint32_t *rec = in + kHead + (nc + c) * kRec;
        if (strict && ((rec[3] >> pat) & 1u)) continue;
        run_case(rec, out + o_exit(nc) + (pat * ne + c) * 128);
    }
}

// the second launch: what the first one left in `g`, by plain loads and by the agent-scope ones
XW_FN void phase1(const Args &A)
{
    const uint32_t t = xw::thread();
    const uint32_t *g = A.g;
    uint32_t *o = A.out + 32 * t;
    for (uint32_t k = 0; k < 4; k++) { o[k] = g[gA + 4 * t + k]; o[4 + k] = g[gB + 4 * t + k]; }
    const xw::u32x4 ra = xw::ld_agent128(g + gA + 4 * t), rb = xw::ld_agent128(g + gB + 4 * t);
    o[8] = ra.x; o[9] = ra.y; o[10] = ra.z; o[11] = ra.w;
    o[12] = rb.x; o[13] = rb.y; o[14] = rb.z; o[15] = rb.w;
    o[16] = xw::ld_agent(g + g32 + t);
    o[17] = g[g32 + t];
    const unsigned long long r64 = xw::ld_agent64((const unsigned long long *)(g + g64) + t), p64 = ((const unsigned long long *)(g + g64))[t];
    o[18] = (uint32_t)r64; o[19] = (uint32_t)(r64 >> 32);
    o[20] = (uint32_t)p64; o[21] = (uint32_t)(p64 >> 32);
    o[22] = xw::ld_agent(g + gCas + t);
    o[23] = xw::ld_agent(g + gOr + (t & 3));
    const unsigned long long s64 = xw::ld_agent64((const unsigned long long *)(g + gAdd64) + (t & 1));
    o[24] = (uint32_t)s64; o[25] = (uint32_t)(s64 >> 32);
    o[26] = xw::ld_agent(g + gCont);
    for (uint32_t k = 27; k < 32; k++) o[k] = 0;
}

XW_FN void probe_role(const Args &A)
{
    if (A.phase == 0) phase0(A); else phase1(A);
}

}  // namespace xwp
