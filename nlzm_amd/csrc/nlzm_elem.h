// nlzm_elem.h -- the statistic that chooses a typed range's element size, for bytes that lie in device memory; written against
// xw.h like the byte planes' role (nlzm_planes.h): the same source runs on gfx950 (nlzm_elem.hip) and in the fiber simulator
// (tests/host_sim/elem_sim.cpp).  tests/elem_model.py restates the rule.
//
// The rule.  For a range x of n bytes, M = n div 8: H[c][v] is the number of i < 8 M with i mod 8 = c and x[i] = v, i counted from the range's own
// first byte (no address and no alignment enters; the n mod 8 bytes behind are in no histogram).  The planes of element size e are
// P(e, j)[v] = the sum over c = j (mod e) of H[c][v], j < e: fifteen histograms for e in {1, 2, 4, 8}.  log2_fix(n) = L(n) is the binary logarithm in
// 2^-16 bits; cost(h) = N L(N) - sum h[v] L(h[v]) + floor(K L(N) / 2) modulo 2^64 for a histogram of total N with K non-zero bins; C_e is the sum of
// cost(P(e, j)) over j < e.  A range gives (C_1, C_2, C_4, C_8); elem::choose (nlzm_elem_plan.h) picks from them on the host.
//
// k ranges are ONE launch of the count role.  The first 8 M bytes of a range are cut into segments of kSegment bytes, one wave per segment; range r owns
// segments [seg0[r], seg0[r + 1]) (nlzm_units.h), and waves stride over the segments.  A wave counts its segment into 8 x 256 counters of 32 bits in
// LDS: the bytes are loaded in 16-byte units at whatever address the segment starts (range::load16u), byte b of a unit belongs to class b mod 8 because
// units start at multiples of 16 of the range, and the eight bytes that 8 M may leave behind the last unit are counted one lane each.
//   * Lane l takes the bytes of its unit in the order l, l + 1, ... (mod 16): on bytes that count up, lanes that all took byte b at once would meet
//     on two of the 32 banks.
//   * Where every live lane of the wave holds the SAME sixteen bytes -- zeros, one repeated byte, any pattern whose period divides 16 -- sixteen lanes
//     add the number of live lanes once, instead of 64 lanes adding 1 to one counter sixteen times in a row.
// A range of ONE segment is finished by the wave that counted it: the fifteen costs from its counters, the range's 32-byte record written.  A range of
// more segments has a slot of 2,048 totals of 64 bits in device memory (zeroed by the host), every wave adds its non-zero counters to them with 64-bit
// atomic adds -- integer sums do not depend on the order --, and the total role, a second launch of one wave per such range, forms the costs from the
// totals.  No read leaves the first 8 M bytes of a range; nothing is asked of its address.
#pragma once

#include "xw.h"
#include "nlzm_range.h"
#include "nlzm_units.h"

namespace nlzm {
namespace elem {

constexpr unsigned long long kSegment = 65536;      // bytes of a range that one wave counts; a multiple of 16, and below 2^32 (the counters are 32 bits)
constexpr uint32_t kCounters = 8 * 256;             // H[c][v] at c * 256 + v
constexpr unsigned long long kNone = ~0ull;         // a range without a slot of totals

// what the host hands the launches: the tables of one upload (nlzm_elem_plan.h, elem::Table)
struct Args {
    const uint8_t *src;
    const unsigned long long *off, *len, *slot;     // k entries each
    const unsigned long long *seg0;                 // k + 1 entries
    const unsigned long long *wide;                 // nwide entries: the ranges of more than one segment
    unsigned long long *totals;                     // slots of kCounters words
    unsigned long long *cost;                       // four words a range
    uint32_t k, nwide;
    unsigned long long nsegs;
};

// the workgroup's LDS: one set of counters per wave
struct alignas(16) Lds { uint32_t count[kCounters]; };
constexpr unsigned long long lds_bytes(uint32_t waves) { return (unsigned long long)waves * sizeof(Lds); }

using range::V16;
using range::load16u;

// L(n): 2^16 log2 n rounded down by the steps the rule names, n below 2^63
XW_FN uint32_t log2_fix(unsigned long long n)
{
    if (n < 2) return 0;
    const uint32_t k = 63u - (uint32_t)__builtin_clzll(n);
    unsigned long long x = k <= 31 ? n << (31 - k) : n >> (k - 31);
    uint32_t r = k << 16;
    for (int i = 15; i >= 0; i--) {
        x = (x * x) >> 31;                          // (x below 2^32: the square fits)
        if (x >> 32) { x >>= 1; r += 1u << i; }
    }
    return r;
}

// the sum of v over the 64 lanes, in every lane (all 64 are live)
XW_FN unsigned long long wave_sum(unsigned long long v)
{
    for (uint32_t d = 1; d < 64; d <<= 1) v += xw::shfl64(v, xw::lane() ^ d);
    return v;
}

// (C_1, C_2, C_4, C_8) of the histograms get(c, v) to out[0 .. 3]: lanes over bins, one plane after the other.  Called by the whole wave.
template <class Get> XW_FN void costs_to(Get get, unsigned long long *out)
{
    const uint32_t l = xw::lane();
#pragma unroll 1
    for (uint32_t ei = 0; ei < 4; ei++) {
        const uint32_t e = 1u << ei;
        unsigned long long c_e = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < e; j++) {
            unsigned long long n = 0, s = 0, used = 0;
            for (uint32_t v = l; v < 256; v += 64) {
                unsigned long long h = 0;
                for (uint32_t c = j; c < 8; c += e) h += get(c, v);
                n += h; s += h * log2_fix(h); used += h != 0;
            }
            n = wave_sum(n); s = wave_sum(s); used = wave_sum(used);
            const unsigned long long ln = log2_fix(n);
            c_e += n * ln - s + used * ln / 2;
        }
        if (l == 0) out[ei] = c_e;
    }
}

// byte b (0 .. 15, the lane's own) of a unit that is the two words lo, hi: shifts, no indexed access
XW_FN uint32_t byte_of(unsigned long long lo, unsigned long long hi, uint32_t b)
{
    return (uint32_t)(((b & 8u) ? hi : lo) >> (8u * (b & 7u))) & 255u;
}

// one unit a lane (`on`: this lane holds one; lane 0 always does) into the wave's counters.  Wave-uniform control flow.
XW_FN void count_units(const V16 v, bool on, uint32_t live, uint32_t *cnt)
{
    const uint32_t l = xw::lane();
    const unsigned long long lo = v.x | (unsigned long long)v.y << 32, hi = v.z | (unsigned long long)v.w << 32;
    const unsigned long long flo = xw::readfirst64(lo), fhi = xw::readfirst64(hi);
    if (!xw::any(on && (lo != flo || hi != fhi))) {
        if (l < 16) xw::lds_add(&cnt[(l & 7u) * 256u + byte_of(flo, fhi, l)], live);
    } else if (on) {
#pragma unroll
        for (uint32_t s = 0; s < 16; s++) {
            const uint32_t b = (s + l) & 15u;
            xw::lds_add(&cnt[(b & 7u) * 256u + byte_of(lo, hi, b)], 1u);
        }
    }
}

// `body` bytes at p, a multiple of 8 and kSegment at most, into the wave's counters (which are zero).  Wave-uniform arguments.
XW_FN void count_segment(const uint8_t *p, uint32_t body, uint32_t *cnt)
{
    const uint32_t l = xw::lane(), U = body >> 4;
    uint32_t base = 0;
    for (; base + 256 <= U; base += 256) {          // (four loads in flight per lane)
        const V16 a = load16u(p + 16u * (base + l)), b = load16u(p + 16u * (base + 64 + l)), c = load16u(p + 16u * (base + 128 + l)), d = load16u(p + 16u * (base + 192 + l));
        count_units(a, true, 64, cnt);
        count_units(b, true, 64, cnt);
        count_units(c, true, 64, cnt);
        count_units(d, true, 64, cnt);
    }
    for (; base < U; base += 64) {
        const bool on = base + l < U;               // (a lane without a unit loads lane 0's again and counts nothing)
        count_units(load16u(p + 16u * (on ? base + l : base)), on, U - base < 64 ? U - base : 64, cnt);
    }
    if ((body & 15u) && l < 8) xw::lds_add(&cnt[l * 256u + p[16u * U + l]], 1u);
}

// wave `w` of `nwaves`: segments w, w + nwaves, ... of all ranges.  Called by every wave of the workgroup.
XW_FN void count_role(const Args &a, unsigned long long w, unsigned long long nwaves)
{
    uint32_t *cnt = xw::lds<Lds>()[xw::wave()].count;
    const uint32_t l = xw::lane();
    for (unsigned long long g = w; g < a.nsegs; g += nwaves) {
        const uint32_t lo = units::owner_of(a.seg0, a.k, g);               // the range whose segments hold g
        const unsigned long long whole = a.len[lo] & ~7ull, at = (g - a.seg0[lo]) * kSegment, left = whole - at;
        const unsigned long long slot = a.slot[lo];
        for (uint32_t i = l; i < kCounters / 4; i += 64) *(V16 *)(cnt + 4 * i) = V16{ 0, 0, 0, 0 };
        xw::wave_sync();
        count_segment(a.src + a.off[lo] + at, (uint32_t)(left < kSegment ? left : kSegment), cnt);
        xw::wave_sync();
        if (a.seg0[lo + 1] - a.seg0[lo] == 1) {     // the range is this segment: its record, and its totals where they are wanted
            costs_to([cnt](uint32_t c, uint32_t v) { return (unsigned long long)cnt[c * 256u + v]; }, a.cost + 4ull * lo);
            if (slot != kNone) for (uint32_t i = l; i < kCounters; i += 64) a.totals[slot * kCounters + i] = cnt[i];
        } else {
            for (uint32_t i = l; i < kCounters; i += 64) {
                const uint32_t c = cnt[i];
                if (c) xw::atomic_add64_agent(&a.totals[slot * kCounters + i], c);
            }
        }
        xw::wave_sync();                            // (the counters are zeroed again for the wave's next segment)
    }
}

// wave `w` of `nwaves`: the ranges of more than one segment w, w + nwaves, ..., from their totals
XW_FN void total_role(const Args &a, unsigned long long w, unsigned long long nwaves)
{
    for (unsigned long long g = w; g < a.nwide; g += nwaves) {
        const unsigned long long r = a.wide[g];
        const unsigned long long *t = a.totals + a.slot[r] * kCounters;
        costs_to([t](uint32_t c, uint32_t v) { return t[c * 256u + v]; }, a.cost + 4ull * r);
    }
}

}  // namespace elem
}  // namespace nlzm
