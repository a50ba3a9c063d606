// nlzm_dedup.h -- which ranges of a buffer in device memory hold the same bytes: the device roles of nlzm_hip_equal_ranges* (nlzm_hip_dedup.cpp),
// written against xw.h like the CRC's roles (nlzm_crc.h), the gather role (nlzm_range.h) and the cut points' (nlzm_cut.h): the same source is the
// gfx950 kernels (nlzm_dedup.hip) and the fiber simulation (tests/host_sim/dedup_sim.cpp).  tests/dedup_model.py restates the rule; what the host
// makes of the fingerprints -- the classes, exactly -- is nlzm_dedup_plan.h.
//
// The rule.  A range of n bytes is cut into segments of kSegment bytes counted from its own first byte: segment g holds the m = min(kSegment,
// n - g kSegment) bytes from g kSegment on, an empty range has none.  A segment's bytes, followed by zeros up to a multiple of 16, are the 32-bit
// little-endian words w[0 .. 4U), U = ceil(m / 16).  With K(j) = mix32(j + 1) (mix32: x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B;
// x ^= x >> 16, all modulo 2^32) -- a key for every word position of a segment, none used twice --
//     h(g) = sum over u = 0 .. U - 1 of  ((w[4u] + K(4u)) mod 2^32) * ((w[4u + 1] + K(4u + 1)) mod 2^32)
//                                      + ((w[4u + 2] + K(4u + 2)) mod 2^32) * ((w[4u + 3] + K(4u + 3)) mod 2^32),      modulo 2^64
// (32 x 32 -> 64-bit products: the NH form).  With splitmix64 (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
// x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31) the range's fingerprint is
//     F = splitmix64( (sum over g of splitmix64(h(g) + (g + 1) * 0x9E3779B97F4A7C15)) mod 2^64  XOR  splitmix64(n) ).
// It is a function of the range's bytes and its length: no address, no alignment, no wave enters it, and every sum is modulo 2^64, so no order does.
//
//   fingerprint role   One wave per segment of any range, in one launch for all ranges: segment s of the launch belongs to the last range r with
//                      seg0[r] <= s.  Lane l takes the 16-byte units l, l + 64, ... of the segment, four loads in flight, read as sixteen bytes at
//                      whatever address the range starts (unaligned global loads, as range::load16u); the tail under 16 bytes is read byte by byte
//                      by one lane.  The lanes' sums are added across the wave and h goes to seg_h[s]: one word, one writer.
//   combine role       One wave per range adds its segments' words, lane l segments l, l + 64, ..., and writes F.
//   pair role          A list of pairs {a, b, len} of offsets into the buffer: are the two byte strings equal?  A pair is cut into chunks of kChunk
//                      bytes, one wave each, prefix table chunk0 as range::Args has it.  Both sides are read in unaligned 16-byte units, the tail byte
//                      by byte; a ballot of "some byte of mine differs" decides the chunk, and chunk_ne[c] is 1 or 0: one word, one writer.
//   verdict role       One wave per pair: a ballot over its chunks' words, equal[p] = 1 or 0 (a pair of no bytes is equal).
// No atomics.  No load reaches outside [off, off + len) of its range, or outside either string of its pair; the sides of a pair may overlap each
// other and other pairs.
#pragma once

#include "xw.h"
#include "nlzm_units.h"

namespace nlzm {
namespace dedup {

constexpr unsigned long long kSegment = 32768;      // bytes of a range per fingerprint wave; a multiple of 16
constexpr unsigned long long kChunk = 32768;        // bytes of a pair per comparing wave; a multiple of 16
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

struct Pair { unsigned long long a, b, len; };      // offsets into the buffer

// what the host hands the fingerprint and combine launches: range r owns segments [seg0[r], seg0[r + 1])
struct FpArgs {
    const uint8_t *buf;
    const unsigned long long *off, *len;            // k entries each
    const unsigned long long *seg0;                 // k + 1 entries
    unsigned long long *seg_h;                      // nsegs words
    unsigned long long *fp;                         // k words
    uint32_t k;
    unsigned long long nsegs;
};
// ... and the pair and verdict launches: pair p owns chunks [chunk0[p], chunk0[p + 1])
struct PairArgs {
    const uint8_t *buf;
    const Pair *pairs;
    const unsigned long long *chunk0;               // npairs + 1 entries
    uint32_t *chunk_ne;                             // nchunks words
    uint32_t *equal;                                // npairs words
    uint32_t npairs;
    unsigned long long nchunks;
};

XW_FN uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    return x ^ (x >> 16);
}
XW_FN unsigned long long splitmix64(unsigned long long x)
{
    x += kGolden;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct V16 { uint32_t x, y, z, w; };
XW_FN V16 load16u(const uint8_t *p)                 // any address
{
    V16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
// unit u of a segment: its four words under their keys
XW_FN unsigned long long nh_unit(const V16 &v, uint32_t u)
{
    const uint32_t j = 4u * u + 1u;
    return (unsigned long long)(v.x + mix32(j)) * (v.y + mix32(j + 1)) + (unsigned long long)(v.z + mix32(j + 2)) * (v.w + mix32(j + 3));
}
XW_FN unsigned long long wave_add64(unsigned long long v)
{
    const uint32_t l = xw::lane();
    for (uint32_t d = 1; d < 64; d <<= 1) v += xw::shfl64(v, l ^ d);
    return v;
}

// h of the m bytes at p (1 <= m <= kSegment) by one wave (wave-uniform arguments); every lane returns it
XW_FN unsigned long long segment_h(const uint8_t *p, uint32_t m)
{
    const uint32_t l = xw::lane();
    const uint32_t full = m >> 4, tail = m & 15u;
    unsigned long long sum = 0;
    uint32_t u = l;
    for (; u + 192 < full; u += 256) {              // (four loads in flight per lane)
        const V16 a = load16u(p + 16u * u), b = load16u(p + 16u * (u + 64)), c = load16u(p + 16u * (u + 128)), e = load16u(p + 16u * (u + 192));
        sum += nh_unit(a, u) + nh_unit(b, u + 64) + nh_unit(c, u + 128) + nh_unit(e, u + 192);
    }
    for (; u < full; u += 64) sum += nh_unit(load16u(p + 16u * u), u);
    if (tail && l == 0) {                           // the last unit, zeros behind the segment's end: byte by byte
        const uint8_t *q = p + 16u * full;
        V16 t{ 0, 0, 0, 0 };
#pragma unroll
        for (uint32_t b = 0; b < 15; b++) {
            if (b >= tail) continue;
            const uint32_t v = (uint32_t)q[b] << (8u * (b & 3u));
            if (b < 4) t.x |= v; else if (b < 8) t.y |= v; else if (b < 12) t.z |= v; else t.w |= v;
        }
        sum += nh_unit(t, full);
    }
    return wave_add64(sum);
}

// wave `w` of `nwaves`: segments w, w + nwaves, ... of all ranges
XW_FN void fingerprint_role(const FpArgs &a, unsigned long long w, unsigned long long nwaves)
{
    for (unsigned long long s = w; s < a.nsegs; s += nwaves) {
        const uint32_t r = units::owner_of(a.seg0, a.k, s);
        const unsigned long long at = (s - a.seg0[r]) * kSegment, left = a.len[r] - at;
        const unsigned long long h = segment_h(a.buf + a.off[r] + at, (uint32_t)(left < kSegment ? left : kSegment));
        if (xw::lane() == 0) a.seg_h[s] = h;
    }
}

// wave `w` of `nwaves`: ranges w, w + nwaves, ...
XW_FN void combine_role(const FpArgs &a, unsigned long long w, unsigned long long nwaves)
{
    const uint32_t l = xw::lane();
    for (unsigned long long r = w; r < a.k; r += nwaves) {
        const unsigned long long s0 = a.seg0[r], ns = a.seg0[r + 1] - s0;
        unsigned long long sum = 0;
        for (unsigned long long g = l; g < ns; g += 64) sum += splitmix64(a.seg_h[s0 + g] + (g + 1) * kGolden);
        sum = wave_add64(sum);
        if (l == 0) a.fp[r] = splitmix64(sum ^ splitmix64(a.len[r]));
    }
}

// do the n bytes at x and at y (1 <= n <= kChunk) differ?  One wave, wave-uniform arguments; every lane returns the answer.
XW_FN bool chunk_differs(const uint8_t *x, const uint8_t *y, uint32_t n)
{
    const uint32_t l = xw::lane();
    const uint32_t full = n >> 4, tail = n & 15u;
    uint32_t d = 0;
    uint32_t u = l;
    for (; u + 192 < full; u += 256) {              // (eight loads in flight per lane)
        const V16 a0 = load16u(x + 16u * u), a1 = load16u(x + 16u * (u + 64)), a2 = load16u(x + 16u * (u + 128)), a3 = load16u(x + 16u * (u + 192));
        const V16 b0 = load16u(y + 16u * u), b1 = load16u(y + 16u * (u + 64)), b2 = load16u(y + 16u * (u + 128)), b3 = load16u(y + 16u * (u + 192));
        d |= (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w);
        d |= (a2.x ^ b2.x) | (a2.y ^ b2.y) | (a2.z ^ b2.z) | (a2.w ^ b2.w) | (a3.x ^ b3.x) | (a3.y ^ b3.y) | (a3.z ^ b3.z) | (a3.w ^ b3.w);
    }
    for (; u < full; u += 64) {
        const V16 a0 = load16u(x + 16u * u), b0 = load16u(y + 16u * u);
        d |= (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w);
    }
    if (l < tail) d |= (uint32_t)(x[16u * full + l] ^ y[16u * full + l]);
    return xw::ballot(d != 0) != 0;
}

// wave `w` of `nwaves`: chunks w, w + nwaves, ... of all pairs
XW_FN void pair_role(const PairArgs &a, unsigned long long w, unsigned long long nwaves)
{
    for (unsigned long long c = w; c < a.nchunks; c += nwaves) {
        const uint32_t p = units::owner_of(a.chunk0, a.npairs, c);
        const Pair P = a.pairs[p];
        const unsigned long long at = (c - a.chunk0[p]) * kChunk, left = P.len - at;
        const bool ne = chunk_differs(a.buf + P.a + at, a.buf + P.b + at, (uint32_t)(left < kChunk ? left : kChunk));
        if (xw::lane() == 0) a.chunk_ne[c] = ne ? 1u : 0u;
    }
}

// wave `w` of `nwaves`: pairs w, w + nwaves, ...
XW_FN void verdict_role(const PairArgs &a, unsigned long long w, unsigned long long nwaves)
{
    const uint32_t l = xw::lane();
    for (unsigned long long p = w; p < a.npairs; p += nwaves) {
        const unsigned long long c0 = a.chunk0[p], nc = a.chunk0[p + 1] - c0;
        uint32_t ne = 0;
        for (unsigned long long c = l; c < nc; c += 64) ne |= a.chunk_ne[c0 + c];
        const bool any = xw::ballot(ne != 0) != 0;
        if (l == 0) a.equal[p] = any ? 0u : 1u;
    }
}

}  // namespace dedup
}  // namespace nlzm
