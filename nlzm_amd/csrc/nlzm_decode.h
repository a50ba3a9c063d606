// nlzm_decode.h -- the decoder role: one NLZM stream decoded by one wave, written against xw.h like the roles of nlzm_v2.h,
// so that the same source is the gfx950 kernel (nlzm_decode.hip) and the fiber simulation (tests/host_sim/decode_sim.cpp).
//
// The bytes are specified by the host decoder, nlzm_host_decode.h (decode_file, NLZM.cpp:1912-2039): this role accepts exactly
// the streams that one accepts and writes exactly its bytes; the mutant test of tests/test_decode_sim.py holds it to that.
//
// What the 64 lanes are for (the host decoder does all of it one value at a time):
//  * the model, 72 CDFs of at most 16 entries, lives in 18 VGPRs: a register holds four CDFs, lane 16 g + i holds entry i of the
//    register's CDF g.  A symbol is found by ONE compare of all lanes and a population count, start / freq come by readlane, and
//    all entries adapt in one VALU pass.  No symbol touches LDS or memory for its model (priced in DESIGN.md section 16).
//    A register is chosen by selects with a wave-uniform condition, never by an indexed access (that would put the model in scratch).
//  * the two forward byte streams of a frame (rANS words, raw bits) are windows of 64 dwords, one per lane, read by readlane; the
//    next window is requested when the current one is opened, a whole window before it is needed.
//  * matches are copied by the wave, 64 bytes per step; literals go to the output ring as they are decoded.
//  * the stream's most recent kRing output bytes stay in an LDS ring that is flushed to memory in aligned 16-byte stores; matches
//    within the ring's reach are served from LDS, farther ones from memory.
//
// Termination on ANY input (the role never spins and never reads or writes outside its buffers):
//  * every op decodes at least one rANS symbol.  A symbol either reads two bytes of the frame -- a frame has at most nb + nr of them, then
//    `bad` ends it -- or leaves its state x >= 2^16 unread, and then x has strictly decreased: x' = freq * (x >> 14) + (x & 16383) - start
//    <= x - (16384 - freq) * (x >> 14), with x >> 14 >= 4 and freq < 16384.  freq < 16384 because no CDF can give one symbol everything:
//    adaptation moves entry i towards i (below the symbol) or towards 16384 + i + 127 - ns and stops 127 short of it (above), so
//    i <= c[i] <= 16384 - (ns - i), and a symbol's share is at most 16384 - (ns - 1).  So a state survives at most ~16384 * ln(2^16)
//    symbols without reading, and a frame ends after a number of symbols bounded by its size.
//  * frames: each consumes nb + nr >= 28 bytes of the stream or ends the decode.
//  * on top of the argument a clock100() budget, checked every 256 ops, ends a decode that takes absurdly long (kErrKernel).
#pragma once

#include "xw.h"

// The role can be built twice into one library: NLZM_DEC_NS names the namespace this inclusion's copy lives in, NLZM_DEC_RING its ring
// (nlzm_decode_small.hip: nlzm::dec_small at 16 KiB beside nlzm::dec at 64 KiB).  StreamArgs and StreamResult are the same bytes in every copy.
#ifndef NLZM_DEC_NS
#define NLZM_DEC_NS dec
#endif

namespace nlzm {
namespace NLZM_DEC_NS {

#ifndef NLZM_DEC_RING
#define NLZM_DEC_RING 65536
#endif
constexpr uint32_t kRing = NLZM_DEC_RING;           // bytes of the output ring (a test build shrinks it: tests/host_sim/Makefile)
constexpr uint32_t kMaxMatch = 7 + 255 + 5;         // lv <= 7 + 15 * 16 + 15, match_min <= 5
constexpr uint32_t kFlush = kRing - 288 < 8192 ? kRing - 288 : 8192;    // unflushed bytes from which the ring is flushed after an op
static_assert((kRing & (kRing - 1)) == 0 && kRing >= 512, "the ring is a power of two, and an op's kMaxMatch bytes + what is unflushed must fit");
static_assert(kFlush + kMaxMatch + 16 <= kRing, "an op may not overwrite bytes of the ring that are not in memory yet");

enum : int { kOk = 0, kErrCapacity = -4, kErrKernel = -5, kErrFormat = -7 };    // NLZM_HIP_E_CAPACITY, _KERNEL, _FORMAT
enum : int { kPaused = 1 };                         // the stepping form only: stopped in front of a frame header, the state saved (no error)

// ---- a decode at rest in front of a frame header (the stepping form, decode_role_steps) ---------------------------------------
// What crosses a frame header: where the header lies, how much is decoded, the model and rep[4]; the rANS states and the bit word are a
// frame's own, and the ring is a copy of output bytes that are in memory.  The record lies in device memory that the host library owns;
// the role that pauses writes it, the role that resumes reads it.  The model: register r of lane l at model[r][l], one coalesced store a
// register (entries fit 16 bits; kept as the dwords they are in the registers).
constexpr uint32_t kModelRegs = 18;
constexpr uint32_t kStateValid = 0x4E535431u;       // "NST1"
struct StepState {
    uint32_t model[kModelRegs][64];
    unsigned long long pos, n;                      // stream offset of the next frame header (0: the stream's own header is still to be read), output bytes so far
    unsigned long long syms, raw_ops, n_literal, n_dict, n_rep, ring_bytes, global_bytes, cycles, window_cycles, copy_cycles;     // the running counters
    unsigned long long frames;                      // frames done
    uint32_t rep[4];
    uint32_t valid, pad_;                           // kStateValid while the decode is at rest; anything else: nothing to resume from
};
constexpr uint32_t kStateBytes = (uint32_t)sizeof(StepState);

// one per stream (= per workgroup), in memory
struct StreamArgs {
    const uint8_t *src; unsigned long long len;     // reads stay inside [src, src + len)
    uint8_t *dst; unsigned long long cap;           // writes stay inside [dst, dst + cap); dst == nullptr: size only, nothing is stored
    unsigned long long budget;                      // clock100() ticks the decode may take
    uint32_t flags = 0;                             // kPrefix; the stepping form: kResume, kMore
    // the stepping form (decode_role_steps) only; the one-shot role does not look at them
    StepState *state = nullptr;                     // where a pause saves the decode and kResume finds it
    uint32_t max_frames = 0;                        // pause after this many frames of this launch (0: no limit)
    unsigned long long target = ~0ull;              // pause at the first frame boundary with out_len >= target
};
// kPrefix: reaching `cap` ends the decode SUCCESSFULLY (rc = kOk, out_len = cap): the literal that would land at dst + cap is not
// written (not even decoded: the decode stops behind the op that brings n to cap), a match that runs over it is copied up to it
// exactly, the ring is flushed in full.  What the stream holds behind the op that reaches `cap` is not looked at -- no later op, no
// frame end, no frame header, no terminator; cap = 0 reads the stream's four header bytes and nothing else: a prefix read vouches for
// NOTHING behind the bytes it returns (a stream damaged there decodes as if it were whole).  The counters (syms, n_literal, ...)
// count the ops up to and including the one that reached `cap`.  A stream that ends before `cap` reports its true, shorter out_len.
// Without the flag a `cap` below the stream's length stays kErrCapacity.
//
// The stepping form.  In front of every frame header -- where prefix mode makes its test, and nowhere else -- the decode PAUSES when
// max_frames frames were decoded in this launch, when n >= target, or, with kMore only, when the header or the frame's nb + nr bytes do
// not lie wholly inside [src, src + len): the stream's tail has not arrived (without kMore that stays kErrFormat, detail 3; with or
// without it no read leaves [src, src + len)).  The terminator ends the decode (kOk) whatever the limits say.  A pause flushes the ring in
// full, saves *state and reports rc = kPaused, out_len = n, why = the reason; kResume starts from *state instead of from the stream's four
// header bytes.  The counters run on through the state: after the last step they are the one-shot decode's.  kPrefix does not combine
// with a state (a decode cut in the middle of an op cannot be resumed): the host refuses it.
enum : uint32_t { kPrefix = 1u, kResume = 2u, kMore = 4u };
enum : uint32_t { kWhyNone = 0, kWhyFrames = 1, kWhyTarget = 2, kWhyInput = 3 };
struct StreamResult {
    int rc; uint32_t detail;                        // detail: the host decoder's code for a format error (-1 .. -7, negated)
    unsigned long long out_len;                     // bytes decoded (an error: up to where it was noticed)
    unsigned long long syms, raw_ops, n_literal, n_dict, n_rep;     // the oracle's rans_syms, bit_ops, n_literal, n_dict, n_rep
    unsigned long long ring_bytes, global_bytes;    // match bytes served from the LDS ring / from memory
    unsigned long long cycles, window_cycles, copy_cycles;         // wave cycles: in all, waiting for input windows, copying and flushing
    uint32_t why;                                   // written by the stepping form only: kWhy* of a pause, kWhyNone otherwise
};
static_assert(sizeof(StreamArgs) == 72 && sizeof(StreamResult) == 104, "one layout for every copy of the role: the host fills and reads them as nlzm::dec's");

// c += d for a counter: kept in VGPRs (every lane the same value) -- the role's wave-uniform state fills the scalar registers as it is
XW_FN void vadd(unsigned long long &c, unsigned long long d)
{
    const uint32_t lo = xw::opaque((uint32_t)c), hi = xw::opaque((uint32_t)(c >> 32));
    c = (((unsigned long long)hi << 32) | lo) + d;
}

struct alignas(16) V16 { uint32_t x, y, z, w; };
struct Lds { alignas(16) uint8_t ring[kRing]; };

// ---- a forward byte stream of the frame as a window of 64 dwords ------------------------------------------------------------
// Offsets are "v" offsets: stream offset + (address of src & 3), so that a multiple of four is an aligned dword in memory.
struct Win { uint32_t cur, nxt; unsigned long long vb; };          // the window covers v in [vb, vb + 256), nxt the 256 behind it

struct Src { const uint8_t *base; unsigned long long a, vend; };   // base = src - a (aligned), stream bytes are v in [a, vend)

XW_FN uint32_t win_load(const Src &S, unsigned long long vb)
{
    const unsigned long long v = vb + 4ull * xw::lane();
    if (v >= S.a && v + 4 <= S.vend) return *(const uint32_t *)(S.base + v);    // whole dword inside the stream: one aligned load
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; k++) if (v + k >= S.a && v + k < S.vend) w |= (uint32_t)S.base[v + k] << (8 * k);     // the stream's ends: byte by byte, nothing outside it
    return w;
}
XW_FN void win_open(const Src &S, Win &W, unsigned long long pos)
{
    W.vb = (pos + S.a) & ~3ull;
    W.cur = win_load(S, W.vb);
    W.nxt = win_load(S, W.vb + 256);
}
// the stream's byte at offset pos (the caller has checked pos against the frame's end; beyond the stream it reads 0)
XW_FN uint32_t win_byte(const Src &S, Win &W, unsigned long long pos, unsigned long long &wait_cycles)
{
    unsigned long long o = pos + S.a - W.vb;
    while (o >= 256) {                              // (reads are consecutive: once, except after a frame's states)
        const unsigned long long t0 = xw::tick();
        W.cur = xw::opaque(W.nxt);                  // the load that was issued a window ago is waited for here ...
        vadd(wait_cycles, xw::tick() - t0);
        W.vb += 256;
        W.nxt = win_load(S, W.vb + 256);            // ... and the one a window ahead issued
        o -= 256;
    }
    return (xw::readlane(W.cur, (uint32_t)(o >> 2)) >> (8 * ((uint32_t)o & 3))) & 255u;
}

// ---- the model in registers ----------------------------------------------------------------------------------------------------
struct Model {
    uint32_t misc;          // groups: cmd (4 symbols), lit_hi (16), len_direct (8), len_ext_hi (16)
    uint32_t shi;           // slot_hi[c] in group c (8 symbols each)
    uint32_t llo[4];        // lit_lo[h]: register h >> 2, group h & 3
    uint32_t elo[4];        // len_ext_lo[h] likewise
    uint32_t slo[8];        // slot_lo[c][s]: k = 8 c + s, register k >> 2, group k & 3
    uint32_t rep[4];
};
XW_FN uint32_t cdf_init(uint32_t ns) { const uint32_t i = xw::lane() & 15u; return i < ns ? i * (16384u / ns) : 16384u; }   // entries from ns up: never below f
XW_FN void model_init(Model &m)
{
    const uint32_t g = xw::lane() >> 4;
    m.misc = g == 0 ? cdf_init(4) : g == 2 ? cdf_init(8) : cdf_init(16);
    m.shi = cdf_init(8);
    for (int j = 0; j < 4; j++) { m.llo[j] = cdf_init(16); m.elo[j] = cdf_init(16); }
    for (int j = 0; j < 8; j++) m.slo[j] = cdf_init(8);
    for (uint32_t j = 0; j < 4; j++) m.rep[j] = j + 1;
}
// every model register with its index in StepState::model: constant indices after unrolling, never an indexed access to the registers
template <class F> XW_FN void model_each(Model &m, F f)
{
    f(0u, m.misc); f(1u, m.shi);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) { f(2u + j, m.llo[j]); f(6u + j, m.elo[j]); }
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) f(10u + j, m.slo[j]);
}

// ---- a frame ---------------------------------------------------------------------------------------------------------------------
struct Frame {
    Win wr, wb;                                     // rANS bytes, raw-bit bytes
    unsigned long long rp, bp, end;                 // stream offsets: next rANS byte, next raw-bit byte, the frame's end
    uint32_t s0, s1, s2, s3;                        // the four states, s0 the next symbol's (rotated instead of indexed)
    uint32_t word, word_bits, num_ops;              // (uint32 and wrapping, as the host decoder's)
    bool bad;
};
struct Count { unsigned long long syms, raw_ops, window_cycles; };

XW_FN uint32_t popc16(uint32_t v) { return (uint32_t)__builtin_popcount(v & 0xFFFFu); }

// ReadCDF (NLZM.cpp:666-712) on the CDF in group g of register r[q]; ns symbols.
// The symbol: the host decoder bisects for the last entry with f >= c[y] (:388-433); here every lane compares its entry and the
// symbol is the count of entries that are <= f, minus one (c[0] = 0 always counts).  The two agree because a CDF stays monotone:
// an adaptation step maps c -> c + ((mix - c) >> 7), which never decreases when c grows (c + 1 moves the shifted term by at most
// one) nor when mix grows, and mix_i <= mix_(i+1); so c[i] <= c[i+1] is kept, "f >= c[i]" holds on a prefix of the entries, and
// the bisection's answer is that prefix's last index.  Entries from ns up hold 16384 > f and never count.
template <int N> XW_FN uint32_t sym(const Src &S, Frame &F, Count &C, uint32_t (&r)[N], uint32_t q, uint32_t g, uint32_t ns)
{
    F.num_ops--;
    vadd(C.syms, 1);
    uint32_t v = r[0];
#pragma unroll
    for (int j = 1; j < N; j++) v = q == (uint32_t)j ? xw::opaque(r[j]) : v;     // (opaque: a choice by selects, not one indexed access -- that would be scratch)
    const uint32_t rs = F.s0, f = rs & 16383u;
    const unsigned long long le = xw::ballot(f >= v);
    const uint32_t y = popc16((uint32_t)(le >> (16 * g))) - 1;
    const uint32_t start = xw::readlane(v, 16 * g + y);
    uint32_t next = xw::readlane(v, 16 * g + (y < 15 ? y + 1 : 15));
    if (y == 15) next = 16384;
    const uint32_t freq = next - start;
    uint32_t x = freq * (rs >> 14) + f - start;                                    // :457-459
    if (x < 65536u) {                                                              // :481-488
        if (F.rp + 2 > F.end) { F.bad = true; return 0; }
        const uint32_t b0 = win_byte(S, F.wr, F.rp, C.window_cycles), b1 = win_byte(S, F.wr, F.rp + 1, C.window_cycles);
        x = (x << 16) + (b0 << 8) + b1;
        F.rp += 2;
    }
    F.s0 = F.s1; F.s1 = F.s2; F.s2 = F.s3; F.s3 = x;
    // adaptation of all entries at once (:284-298, :348-382)
    const uint32_t i = xw::lane() & 15u;
    const int mix = i <= y ? (int)i : (int)(16384 + i + 127 - ns);
    const uint32_t nv = v + (uint32_t)((mix - (int)v) >> 7);
    v = ((xw::lane() >> 4) == g && i < ns) ? nv : v;
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = xw::opaque(q == (uint32_t)j ? v : r[j]);
    return y;
}
XW_FN uint32_t sym1(const Src &S, Frame &F, Count &C, uint32_t &r, uint32_t g, uint32_t ns)
{
    uint32_t t[1] = { r };
    const uint32_t y = sym<1>(S, F, C, t, 0, g, ns);
    r = t[0];
    return y;
}
XW_FN uint32_t raw(const Src &S, Frame &F, Count &C, uint32_t nb)                 // ReadBits, :714-731
{
    F.num_ops--;
    vadd(C.raw_ops, 1);
    while (F.word_bits < 24) {
        if (F.bp >= F.end) { F.bad = true; return 0; }
        F.word |= win_byte(S, F.wb, F.bp, C.window_cycles) << (24 - F.word_bits);
        F.bp++;
        F.word_bits += 8;
    }
    const uint32_t y = F.word >> (32 - nb);
    F.word <<= nb; F.word_bits -= nb;
    return y;
}
XW_FN uint32_t dec_len(const Src &S, Frame &F, Count &C, Model &m)                // model_decode_lv, :1369-1383
{
    uint32_t lv = sym1(S, F, C, m.misc, 2, 8);
    if (lv == 7) {
        const uint32_t hi = sym1(S, F, C, m.misc, 3, 16);
        const uint32_t lo = sym<4>(S, F, C, m.elo, hi >> 2, hi & 3, 16);
        lv += (hi << 4) + lo;
    }
    return lv;
}
XW_FN uint32_t match_min(uint32_t d) { return 2u + (d >= 256u) + (d >= 4096u) + (d >= (1u << 20)); }     // :813-821

// ---- the output: LDS ring in front of memory ---------------------------------------------------------------------------------
// Position p of the output lies at ring[(p + a) & (kRing - 1)], a = address of dst & 15, so that 16 aligned bytes of the ring are
// 16 aligned bytes of memory.  Positions below `fl` are in memory.
//
// VISIBILITY (the one property the simulator cannot check): a match that is served from memory loads bytes that this same wave
// stored in an earlier flush.  Every flush ends with xw::drain() -- s_waitcnt vmcnt(0) -- before anything else runs: the stores
// have been acknowledged by the L2 when a later load of the same wave is issued, and the CU's vector L1 is write-through (a store
// does not leave a stale line behind for the CU's own later loads).  One wave, program order, a completed store: no fence or
// cache maintenance is needed, and no other wave or workgroup ever reads a stream's output while it is being decoded.  The bytes a
// resumed decode preloads (and its saved state) were stored by an EARLIER launch: a kernel boundary makes them visible.
struct Out {
    uint8_t *base;                                  // dst - a
    unsigned long long a, cap, n, fl;               // n: bytes decoded
    bool store;
    unsigned long long ring_bytes, global_bytes;
};
XW_FN void flush(Out &O, bool all)
{
    uint8_t *ring = xw::lds<Lds>()->ring;
    const unsigned long long vlo = O.fl + O.a;
    const unsigned long long vhi = all ? O.n + O.a : (O.n + O.a) & ~15ull;
    if (vhi <= vlo) return;
    const uint32_t l = xw::lane();
    unsigned long long up = (vlo + 15) & ~15ull;
    if (up > vhi) up = vhi;
    if (vlo + l < up) O.base[vlo + l] = ring[(vlo + l) & (kRing - 1)];             // up to 15 bytes in front of the first aligned 16
    const unsigned long long bend = vhi & ~15ull;
    for (unsigned long long u = up + 16ull * l; u + 16 <= bend; u += 1024)
        *(V16 *)(O.base + u) = *(const V16 *)(ring + (u & (kRing - 1)));
    const unsigned long long t = bend > up ? bend : up;
    if (t + l < vhi) O.base[t + l] = ring[(t + l) & (kRing - 1)];                  // (all: up to 15 bytes behind the last one)
    O.fl = vhi - O.a;
    xw::drain();
    xw::wave_sync();
}
// flush's mirror image for a resumed decode: the last min(kRing, n) output bytes, which an earlier launch stored, from memory into the ring
// (same alignment relation: 16 aligned bytes of memory are 16 aligned bytes of the ring).  Afterwards the ring holds what it would hold
// had the decode never stopped, so copy() serves the same matches from it.  Reads stay inside [dst, dst + n).
XW_FN void preload(Out &O)
{
    uint8_t *ring = xw::lds<Lds>()->ring;
    const unsigned long long vhi = O.n + O.a, vlo = vhi - (O.n < kRing ? O.n : (unsigned long long)kRing);
    if (vhi <= vlo) return;
    const uint32_t l = xw::lane();
    unsigned long long up = (vlo + 15) & ~15ull;
    if (up > vhi) up = vhi;
    if (vlo + l < up) ring[(vlo + l) & (kRing - 1)] = O.base[vlo + l];
    const unsigned long long bend = vhi & ~15ull;
    for (unsigned long long u = up + 16ull * l; u + 16 <= bend; u += 1024)
        *(V16 *)(ring + (u & (kRing - 1))) = *(const V16 *)(O.base + u);
    const unsigned long long t = bend > up ? bend : up;
    if (t + l < vhi) ring[(t + l) & (kRing - 1)] = O.base[t + l];
    xw::wave_sync();
}
// lv bytes from dv back (dv <= n and n + lv <= cap checked by the caller)
XW_FN void copy(Out &O, uint32_t dv, uint32_t lv)
{
    if (!O.store) { O.n += lv; return; }
    uint8_t *ring = xw::lds<Lds>()->ring;
    const unsigned long long from = O.n - dv;
    const bool periodic = dv < lv;                  // the source runs into the match itself: byte i is byte i % dv (the host's byte loop defines it)
    // from the ring when no step of the copy overwrites a ring byte a later step reads: steps read before they write, and step k
    // writes what lies kRing behind n + 64 k, which a plain copy has read by then exactly when dv <= kRing
    const bool in_ring = dv + (periodic ? lv : 0u) <= kRing;
    if (!in_ring) {
        const unsigned long long need = from + (periodic ? dv : lv);
        if (need > O.fl) flush(O, true);            // (only a ring far smaller than the product's gets here)
    }
    vadd(O.ring_bytes, in_ring ? lv : 0u);          // (both, unconditionally: "one or the other" becomes an indexed access, i.e. scratch)
    vadd(O.global_bytes, in_ring ? 0u : lv);
    const uint32_t l = xw::lane();
    // (two loops, not one with a chosen pointer: a load through "LDS or memory" would be a flat one)
    if (in_ring) {
        for (uint32_t k = 0; k < lv; k += 64) {
            const uint32_t i = k + l;
            uint32_t b = 0;
            if (i < lv) b = ring[(from + (periodic ? i % dv : i) + O.a) & (kRing - 1)];
            xw::wave_sync();
            if (i < lv) ring[(O.n + i + O.a) & (kRing - 1)] = (uint8_t)b;
            xw::wave_sync();
        }
    } else {
        for (uint32_t k = 0; k < lv; k += 64) {
            const uint32_t i = k + l;
            if (i < lv) ring[(O.n + i + O.a) & (kRing - 1)] = O.base[from + (periodic ? i % dv : i) + O.a];
        }
        xw::wave_sync();
    }
    O.n += lv;
}

// ---- the role ----------------------------------------------------------------------------------------------------------------------
XW_FN uint32_t ld_u8(const Src &S, unsigned long long pos) { return xw::readfirst((uint32_t)S.base[pos + S.a]); }
XW_FN uint32_t ld_be32(const Src &S, unsigned long long pos)
{
    return (ld_u8(S, pos) << 24) | (ld_u8(S, pos + 1) << 16) | (ld_u8(S, pos + 2) << 8) | ld_u8(S, pos + 3);
}

// (not XW_FN: the role is left to the optimiser's inliner, which takes it into its one caller AFTER the instantiation has been simplified.
//  decode_kernel, -Rpass-analysis=kernel-resource-usage: 105 VGPRs, 106 SGPRs, scratch 0, LDS 65,536 either way; spilled SGPRs 49 this way,
//  57 with the template forced in early, 54 as the plain forced-inline function it was before it became a template.  A compiler that
//  decides otherwise shows at once: `make asmcheck-decode` holds "no calls" for both kernels, and
//  tests/test_decode_steps_abi.py::test_one_shot_kernel_keeps_its_figures holds the figures above with the spills at 54 or fewer.)
#ifdef NLZM_SIM
#define NLZM_DEC_ROLE_FN inline
#else
#define NLZM_DEC_ROLE_FN __device__ inline
#endif
template <bool kSteps> NLZM_DEC_ROLE_FN void decode_role_t(const StreamArgs &A, StreamResult *res)
{
    const unsigned long long t_begin = xw::tick(), c_begin = xw::clock100();
    Src S;
    S.a = (unsigned long long)A.src & 3ull; S.base = A.src - S.a; S.vend = S.a + A.len;
    Out O;
    O.a = (unsigned long long)A.dst & 15ull; O.base = A.dst - O.a; O.cap = A.cap; O.n = 0; O.fl = 0; O.store = A.dst != nullptr;
    O.ring_bytes = 0; O.global_bytes = 0;
    Count C{ 0, 0, 0 };
    unsigned long long n_literal = 0, n_dict = 0, n_rep = 0, copy_cycles = 0;
    const unsigned long long len = A.len;
    const bool prefix = !kSteps && (A.flags & kPrefix) && O.store;
    const bool more = kSteps && (A.flags & kMore);
    unsigned long long frames = 0, cycles0 = 0;
    uint32_t why = kWhyNone, frames_here = 0;
    int rc = kOk;
    uint32_t detail = 0;
#define DEC_FAIL(code, why) { rc = (code); detail = (why); break; }
#define DEC_PAUSE(reason) { why = (reason); break; }
    do {
        Model m;
        unsigned long long pos = 0;
        if constexpr (kSteps) if (A.flags & kResume) {
            const StepState *T = A.state;
            if (xw::readfirst(T->valid) != kStateValid) DEC_FAIL(kErrKernel, 1)
            pos = xw::readfirst64(T->pos); O.n = xw::readfirst64(T->n); O.fl = O.n; frames = xw::readfirst64(T->frames);
            if (O.store && O.n > O.cap) DEC_FAIL(kErrCapacity, 0)
            const uint32_t l = xw::lane();
            model_each(m, [&](uint32_t r, uint32_t &v) { v = T->model[r][l]; });
            m.rep[0] = xw::readfirst(T->rep[0]); m.rep[1] = xw::readfirst(T->rep[1]); m.rep[2] = xw::readfirst(T->rep[2]); m.rep[3] = xw::readfirst(T->rep[3]);
            C.syms = T->syms; C.raw_ops = T->raw_ops; C.window_cycles = T->window_cycles;
            n_literal = T->n_literal; n_dict = T->n_dict; n_rep = T->n_rep; copy_cycles = T->copy_cycles; cycles0 = T->cycles;
            O.ring_bytes = T->ring_bytes; O.global_bytes = T->global_bytes;
            if (O.store) preload(O);
        }
        bool head = true;                                   // the stream's four header bytes are still to be read
        if constexpr (kSteps) {
            head = pos == 0;                                // (a resumed decode: only when it paused before they had arrived)
            if (head && len < 8 && more) { model_init(m); why = kWhyInput; head = false; }     // (saved below like every pause; the resume starts over)
        }
        if (head) {
            if (len < 8) DEC_FAIL(kErrFormat, 1)
            const uint32_t hb = (ld_u8(S, 0) << 8) + ld_u8(S, 1), fb = (ld_u8(S, 2) << 8) + ld_u8(S, 3);
            if (hb < 10 || hb > 28 || fb < 12 || fb > 20) DEC_FAIL(kErrFormat, 2)
            model_init(m);
            pos = 4;
        }
        uint32_t ops_seen = 0;
        for (;;) {
            if constexpr (kSteps) { if (why) break; }
            if (prefix && O.n >= O.cap) break;              // the prefix is whole: not a byte of what follows is looked at, no frame header either
            // THE pause test of the stepping form: a limit that is reached (it gives way to the terminator only), then input that is not there yet
            uint32_t lim = kWhyNone;
            if constexpr (kSteps) lim = A.max_frames && frames_here >= A.max_frames ? kWhyFrames : O.n >= A.target ? kWhyTarget : kWhyNone;
            if (pos + 4 > len) { if constexpr (kSteps) { if (lim) DEC_PAUSE(lim) if (more) DEC_PAUSE(kWhyInput) } DEC_FAIL(kErrFormat, 3) }
            Frame F;
            F.num_ops = ld_be32(S, pos);
            if (!F.num_ops) break;
            if constexpr (kSteps) { if (lim) DEC_PAUSE(lim) }
            if (pos + 12 > len) { if constexpr (kSteps) { if (more) DEC_PAUSE(kWhyInput) } DEC_FAIL(kErrFormat, 3) }
            const uint32_t nb = ld_be32(S, pos + 4), nr = ld_be32(S, pos + 8);
            if constexpr (kSteps) { if (more && nb >= 12 && nr >= 16 && pos + (unsigned long long)nb + nr > len) DEC_PAUSE(kWhyInput) }
            if (nb < 12 || nr < 16 || pos + (unsigned long long)nb + nr > len) DEC_FAIL(kErrFormat, 3)
            F.bp = pos + 12; F.rp = pos + nb; F.end = pos + nb + nr;
            F.word = 0; F.word_bits = 0; F.bad = false;
            win_open(S, F.wb, F.bp);
            win_open(S, F.wr, F.rp);
            {
                uint32_t st[4];
                for (int k = 0; k < 4; k++) {
                    uint32_t w = 0;
                    for (int j = 0; j < 4; j++) w |= win_byte(S, F.wr, F.rp + 4 * k + j, C.window_cycles) << (8 * j);
                    st[k] = w;
                }
                F.s0 = st[0]; F.s1 = st[1]; F.s2 = st[2]; F.s3 = st[3];
                F.rp += 16;
            }
            while (F.num_ops > 0 && !F.bad) {
                if ((++ops_seen & 255u) == 0 && xw::clock100() - c_begin > A.budget) DEC_FAIL(kErrKernel, 0)
                const uint32_t cmd = sym1(S, F, C, m.misc, 0, 4);
                if (cmd == 0) {
                    const uint32_t hi = sym1(S, F, C, m.misc, 1, 16);
                    const uint32_t lo = sym<4>(S, F, C, m.llo, hi >> 2, hi & 3, 16);
                    vadd(n_literal, 1);
                    if (O.store) {
                        if (F.bad) break;                           // (the host decoder's byte is garbage then, and the stream rejected)
                        if (O.n >= O.cap) DEC_FAIL(kErrCapacity, 0)        // (prefix mode never gets here with n == cap: it has stopped)
                        if (xw::lane() == 0) xw::lds<Lds>()->ring[(O.n + O.a) & (kRing - 1)] = (uint8_t)((hi << 4) + lo);
                    }
                    O.n++;
                } else {
                    uint32_t lv, dv;
                    if (cmd == 1) {
                        lv = dec_len(S, F, C, m);
                        const uint32_t lc = lv < 3 ? lv : 3;
                        const uint32_t shi = sym1(S, F, C, m.shi, lc, 8);
                        const uint32_t k = 8 * lc + shi;
                        const uint32_t slo = sym<8>(S, F, C, m.slo, k >> 2, k & 3, 8);
                        dv = (shi << 3) + slo;
                        if (dv >= 4) {                                                    // :1395-1413
                            uint32_t ab = (dv >> 1) - 1;
                            dv = (2 + (dv & 1)) << ab;
                            if (ab < 4) dv += raw(S, F, C, ab);
                            else { ab -= 4; if (ab > 0) dv += raw(S, F, C, ab) << 4; dv += raw(S, F, C, 4); }
                        }
                        dv += 1;
                        vadd(n_dict, 1);
                    } else if (cmd == 2) {
                        const uint32_t ri = raw(S, F, C, 2);
                        lv = dec_len(S, F, C, m);
                        dv = ri == 0 ? m.rep[0] : ri == 1 ? m.rep[1] : ri == 2 ? m.rep[2] : m.rep[3];
                        vadd(n_rep, 1);
                    } else DEC_FAIL(kErrFormat, 5)
                    lv += match_min(dv);
                    if (!(m.rep[0] == dv || m.rep[1] == dv || m.rep[2] == dv || m.rep[3] == dv)) {
                        m.rep[3] = m.rep[2]; m.rep[2] = m.rep[1]; m.rep[1] = m.rep[0]; m.rep[0] = dv;
                    }
                    if (F.bad) break;                               // (what was decoded after the frame ran out is garbage; the stream is rejected below)
                    if (dv > O.n) DEC_FAIL(kErrFormat, 6)
                    const unsigned long long t0 = xw::tick();
                    if (O.store && O.n + lv > O.cap) {
                        if (!prefix) DEC_FAIL(kErrCapacity, 0)                     // (nothing of the match written)
                        // the cut match: its first cap - n bytes, by the same copy -- bytes i < lv' of a periodic match are those of the whole one
                        copy(O, dv, (uint32_t)(O.cap - O.n));
                        vadd(copy_cycles, xw::tick() - t0);
                        break;
                    }
                    copy(O, dv, lv);
                    vadd(copy_cycles, xw::tick() - t0);
                }
                if (O.store && O.n - O.fl >= kFlush) {
                    const unsigned long long t0 = xw::tick();
                    flush(O, false);
                    vadd(copy_cycles, xw::tick() - t0);
                }
                if (prefix && O.n >= O.cap) break;          // ... and no further op (the frame loop's test ends the decode)
            }
            if (rc) break;
            if (F.bad) DEC_FAIL(kErrFormat, 7)
            pos += (unsigned long long)nb + nr;
            if constexpr (kSteps) { frames++; frames_here++; }
        }
        if (!rc && O.store) flush(O, true);
        if constexpr (kSteps) if (!rc && why) {             // at rest in front of the header at `pos`: everything decoded is in memory
            StepState *T = A.state;
            const uint32_t l = xw::lane();
            model_each(m, [&](uint32_t r, uint32_t &v) { T->model[r][l] = v; });
            if (l == 0) {
                T->pos = pos; T->n = O.n; T->frames = frames;
                T->syms = C.syms; T->raw_ops = C.raw_ops; T->n_literal = n_literal; T->n_dict = n_dict; T->n_rep = n_rep;
                T->ring_bytes = O.ring_bytes; T->global_bytes = O.global_bytes;
                T->cycles = cycles0 + (xw::tick() - t_begin); T->window_cycles = C.window_cycles; T->copy_cycles = copy_cycles;
                T->rep[0] = m.rep[0]; T->rep[1] = m.rep[1]; T->rep[2] = m.rep[2]; T->rep[3] = m.rep[3];
            }
            rc = kPaused;
        }
    } while (0);
#undef DEC_FAIL
#undef DEC_PAUSE
    if constexpr (kSteps) if (xw::lane() == 0) {
        A.state->valid = rc == kPaused ? kStateValid : 0u;  // (a decode that has ended, either way, leaves nothing to resume from)
        res->why = rc == kPaused ? why : kWhyNone;
    }
    if (xw::lane() == 0) {
        res->rc = rc; res->detail = detail; res->out_len = O.n;
        res->syms = C.syms; res->raw_ops = C.raw_ops; res->n_literal = n_literal; res->n_dict = n_dict; res->n_rep = n_rep;
        res->ring_bytes = O.ring_bytes; res->global_bytes = O.global_bytes;
        res->cycles = cycles0 + (xw::tick() - t_begin); res->window_cycles = C.window_cycles; res->copy_cycles = copy_cycles;
    }
}
// the one-shot decode, and the stepping form: the same role with the pause test, the saved state and the ring reload compiled in
XW_FN void decode_role(const StreamArgs &A, StreamResult *res) { decode_role_t<false>(A, res); }
XW_FN void decode_role_steps(const StreamArgs &A, StreamResult *res) { decode_role_t<true>(A, res); }

// ---- the split of a container -------------------------------------------------------------------------------------------------------
// stream_length (nlzm_host_decode.h) for nblocks streams back to back: ONE lane follows the sizes the frame headers carry (no cross-lane
// operation: the caller picks the lane).  block_len[i] = 0 and *bad = 1 + i when stream i is malformed or cut off; *bad = 0 and every
// length when all nblocks are there.  Reads stay inside [src, src + len); every step moves forward by at least 28 bytes or ends.
// tests/host_sim/decode_sim.cpp (split) holds it to nlzm_host::split_streams, flush against a page that may not be read.
XW_FN void split_walk(const uint8_t *__restrict__ src, unsigned long long len, uint32_t nblocks, unsigned long long *__restrict__ block_len,
                      uint32_t *__restrict__ bad)
{
    auto be32 = [&](unsigned long long p) { return ((uint32_t)src[p] << 24) | ((uint32_t)src[p + 1] << 16) | ((uint32_t)src[p + 2] << 8) | src[p + 3]; };
    unsigned long long at = 0;
    *bad = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        unsigned long long pos = at + 4, end = 0;
        if (len - at < 8 || at > len) { *bad = 1 + i; }
        else for (;;) {
            if (pos + 4 > len) { *bad = 1 + i; break; }
            if (!be32(pos)) { end = pos + 4; break; }
            if (pos + 12 > len) { *bad = 1 + i; break; }
            const uint32_t nb = be32(pos + 4), nr = be32(pos + 8);
            if (nb < 12 || nr < 16 || pos + (unsigned long long)nb + nr > len) { *bad = 1 + i; break; }
            pos += (unsigned long long)nb + nr;
        }
        if (!end) { for (; i < nblocks; i++) block_len[i] = 0; return; }
        block_len[i] = end - at;
        at = end;
    }
}

}  // namespace NLZM_DEC_NS
}  // namespace nlzm
