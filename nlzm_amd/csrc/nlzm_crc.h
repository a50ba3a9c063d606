// nlzm_crc.h -- CRC32 of bytes that lie in device memory, written against xw.h like the decoder role (nlzm_decode.h): the same source
// runs on gfx950 (nlzm_crc.hip) and in the fiber simulator (tests/host_sim/crc_sim.cpp).
//
// The CRC is the reference's crc32_calc (NLZM.cpp:126-199): reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF -- zlib's.
//
// A 32-bit state is a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0 (zlib's convention).  Feeding k zero bytes to a state
// multiplies it by x^(8k); feeding a byte b to state s gives T0[(s ^ b) & 0xFF] ^ (s >> 8), which is linear in (s, b).  So the bytes of a
// range may be hashed in any grouping, each group from state 0, and put together by multiplying with powers of x:
//
//   segment role   A range is cut into segments of kSegment bytes, one wave per segment.  The wave hashes the segment's unaligned head (up
//                  to 15 bytes) byte by byte, then the aligned middle as 16-byte chunks: lane l owns chunks l, l + 64, l + 128, ... -- one
//                  coalesced 1,024-byte load per wave and step -- and advances its own state over "my 16 bytes and the 1,008 bytes of the
//                  other lanes, taken as zeros" with sixteen table lookups (the tables hold T0[b] * x^(8 (1023 - i)), 16 KiB of LDS, built by the workgroup).  After
//                  its last chunk a lane's state stands 1,024 bytes behind that chunk's start; one multiplication by x^(8 (16 d - 1008))
//                  (d: chunks between the lane's last one and the middle's end; the negative exponents taken modulo the order of x, which
//                  divides 2^32 - 1 as P is irreducible) moves it to the middle's end, and the wave xors its 64 states together.  The tail
//                  (under 16 bytes) goes byte by byte.  Only the lane that owns the range's first byte starts from ~seed, all others from 0.
//   combine role   One workgroup per range: every lane takes a run of consecutive segments, folds them by Horner's rule (state * x^(8 kSegment)
//                  ^ next), moves the result to the range's end with a power of x by square-and-multiply (the exponent is a 64-bit number of
//                  segments), and the workgroup xors.  No atomics: the result does not depend on which wave ran when.
//
// Reads stay inside [buf + off, buf + off + len) of every range; nothing is asked of the bytes around it.
#pragma once

#include "xw.h"
#include "nlzm_units.h"

#ifndef NLZM_SIM
#define CRC_HD __host__ __device__ inline      // (arithmetic the host side uses too: nlzm_hip_crc32_combine)
#else
#define CRC_HD inline
#endif

namespace nlzm {
namespace crc {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr unsigned long long kSegment = 32768;      // G: bytes per segment (one wave); a multiple of 1,024
constexpr uint32_t kStep = 1024;                    // bytes a wave takes per step: 64 lanes x 16
constexpr uint32_t kOne = 0x80000000u;              // x^0
constexpr uint32_t kX8 = 0x00800000u;               // x^8

// what the host hands a launch: range r is [buf + off[r], + len[r]) and owns segments [seg0[r], seg0[r + 1]) of `part`
struct Args {
    const uint8_t *buf;
    const unsigned long long *off, *len, *seg0;     // seg0: nranges + 1 entries
    uint32_t *part;                                 // one state per segment
    uint32_t *out;                                  // one CRC per range
    uint32_t nranges;
    uint32_t seed;                                  // of every range (zlib.crc32(b, seed))
    unsigned long long nsegs;
};

struct Lds {
    uint32_t step[16][256];                         // step[i][b] = T0[b] * x^(8 (1023 - i))
    uint32_t byte[256];                             // T0
};
struct CombineLds { uint32_t wave[16]; };           // (the combine role's: one word per wave of its workgroup)

// a * b mod P (zlib's multmodp, without its early exit: no branch on data)
CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = kOne; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
    }
    return p;
}
// base^e mod P
CRC_HD constexpr uint32_t powmod(uint32_t base, unsigned long long e)
{
    uint32_t r = kOne;
    for (; e; e >>= 1) {
        if (e & 1ull) r = mulmod(r, base);
        base = mulmod(base, base);
    }
    return r;
}
// x^(8 n): what n zero bytes multiply a state by
CRC_HD constexpr uint32_t x8n(unsigned long long n) { return powmod(kX8, n); }
// s * x^8: one zero byte
CRC_HD constexpr uint32_t zero_byte(uint32_t s)
{
    for (int k = 0; k < 8; k++) s = (s >> 1) ^ ((s & 1u) ? kPoly : 0u);
    return s;
}
constexpr uint32_t kX1008 = x8n(1008);              // x^(8 * 1008)
constexpr uint32_t kXSegment = x8n(kSegment);
// back[d] = x^(8 (16 d - 1008)), d = 0 .. 63: x^-k = x^(2^32 - 1 - k), as the order of x divides 2^32 - 1.  A constant of the program.
struct BackTable { uint32_t v[64]; };
CRC_HD constexpr BackTable make_back()
{
    BackTable t{};
    uint32_t p = powmod(0x40000000u, 0xFFFFFFFFull - 8ull * 1008);
    const uint32_t x128 = x8n(16);
    for (int d = 0; d < 64; d++) { t.v[d] = p; p = mulmod(p, x128); }
    return t;
}
#ifndef NLZM_SIM
__device__ __constant__ const BackTable kBack = make_back();
#else
static const BackTable kBack = make_back();
#endif

// crc_b = CRC32 of B, len_b = |B|: CRC32 of A || B from crc_a = CRC32 of A (zlib's crc32_combine).  Host and device.
CRC_HD constexpr uint32_t combine(uint32_t crc_a, uint32_t crc_b, unsigned long long len_b) { return mulmod(x8n(len_b), crc_a) ^ crc_b; }

// the tables, by all `nthreads` lanes of the workgroup (a multiple of 64); a block_sync follows
XW_FN void build_tables(Lds *L, uint32_t nthreads)
{
    for (uint32_t b = xw::thread(); b < 256; b += nthreads) {
        const uint32_t t0 = zero_byte(b);           // (byte b into state 0: T0[b])
        L->byte[b] = t0;
        uint32_t v = mulmod(t0, kX1008);
#pragma unroll
        for (int i = 15; i >= 0; i--) { L->step[i][b] = v; v = zero_byte(v); }
    }
    xw::block_sync();
}

struct u4 { uint32_t x, y, z, w; };
XW_FN u4 load16(const uint8_t *p)                   // p: 16-byte aligned
{
#ifndef NLZM_SIM
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    const v4 v = *(const v4 *)p;
    return u4{ v.x, v.y, v.z, v.w };
#else
    u4 v;
    memcpy(&v, p, 16);
    return v;
#endif
}

XW_FN uint32_t feed_byte(const Lds *L, uint32_t s, uint32_t b) { return L->byte[(s ^ b) & 0xFF] ^ (s >> 8); }

// a lane's state over its next chunk and the 1,008 bytes behind it
XW_FN uint32_t feed_chunk(const Lds *L, uint32_t s, u4 c)
{
    c.x ^= s;
    uint32_t r;
    r  = L->step[0][c.x & 0xFF] ^ L->step[1][(c.x >> 8) & 0xFF] ^ L->step[2][(c.x >> 16) & 0xFF] ^ L->step[3][c.x >> 24];
    r ^= L->step[4][c.y & 0xFF] ^ L->step[5][(c.y >> 8) & 0xFF] ^ L->step[6][(c.y >> 16) & 0xFF] ^ L->step[7][c.y >> 24];
    r ^= L->step[8][c.z & 0xFF] ^ L->step[9][(c.z >> 8) & 0xFF] ^ L->step[10][(c.z >> 16) & 0xFF] ^ L->step[11][c.z >> 24];
    r ^= L->step[12][c.w & 0xFF] ^ L->step[13][(c.w >> 8) & 0xFF] ^ L->step[14][(c.w >> 16) & 0xFF] ^ L->step[15][c.w >> 24];
    return r;
}

XW_FN uint32_t wave_xor(uint32_t v)
{
    const uint32_t l = xw::lane();
    for (uint32_t d = 1; d < 64; d <<= 1) v ^= xw::shfl(v, l ^ d);
    return v;
}

// the state after the n bytes at p, from state `s` (wave-uniform arguments; every lane returns the result)
XW_FN uint32_t segment_state(const Lds *L, const uint8_t *p, unsigned long long n, uint32_t s)
{
    const uint32_t l = xw::lane();
    unsigned long long head = (16u - (uint32_t)((unsigned long long)p & 15u)) & 15u;
    if (head > n) head = n;
    for (unsigned long long i = 0; i < head; i++) s = feed_byte(L, s, p[i]);
    const uint8_t *mid = p + head;
    const unsigned long long C = (n - head) >> 4;   // chunks of the middle
    if (C) {
        uint32_t mine = l ? 0u : s;
        const unsigned long long full = C >> 6;     // steps every lane takes part in
        const uint32_t rem = (uint32_t)(C & 63u);
        const uint8_t *q = mid + 16u * l;
        unsigned long long j = 0;
        for (; j + 4 <= full; j += 4, q += 4 * kStep) {     // (four loads in flight per lane)
            const u4 c0 = load16(q), c1 = load16(q + kStep), c2 = load16(q + 2 * kStep), c3 = load16(q + 3 * kStep);
            mine = feed_chunk(L, mine, c0);
            mine = feed_chunk(L, mine, c1);
            mine = feed_chunk(L, mine, c2);
            mine = feed_chunk(L, mine, c3);
        }
        for (; j < full; j++, q += kStep) mine = feed_chunk(L, mine, load16(q));
        if (l < rem) mine = feed_chunk(L, mine, load16(q));
        // the lane's last chunk is chunk `last`; lanes without one hold 0
        if (l < rem || full) {
            const unsigned long long last = l < rem ? (full << 6) + l : ((full - 1) << 6) + l;
            mine = mulmod(mine, kBack.v[(uint32_t)(C - 1 - last)]);
        }
        s = wave_xor(mine);
    }
    const uint8_t *tail = mid + (C << 4);
    const uint32_t nt = (uint32_t)((n - head) & 15u);
    for (uint32_t i = 0; i < nt; i++) s = feed_byte(L, s, tail[i]);
    return s;
}

// wave `w` of `nwaves`: segments w, w + nwaves, ... of all ranges.  Called by every wave of the workgroup (the tables are built first).
XW_FN void segments_role(const Args &a, uint32_t nthreads, unsigned long long w, unsigned long long nwaves)
{
    Lds *L = xw::lds<Lds>();
    build_tables(L, nthreads);
    for (unsigned long long g = w; g < a.nsegs; g += nwaves) {
        const uint32_t lo = units::owner_of(a.seg0, a.nranges, g);         // the range whose segments hold g
        const unsigned long long j = g - a.seg0[lo], at = j * kSegment, left = a.len[lo] - at;
        const uint32_t s = segment_state(L, a.buf + a.off[lo] + at, left < kSegment ? left : kSegment, j ? 0u : ~a.seed);
        if (xw::lane() == 0) a.part[g] = s;
    }
}

// the workgroup's `nthreads` lanes (a multiple of 64, at most 1,024): the CRC of range r from its segments' states
XW_FN void combine_role(const Args &a, uint32_t r, uint32_t nthreads)
{
    CombineLds *L = xw::lds<CombineLds>();
    const uint32_t t = xw::thread();
    const unsigned long long s0 = a.seg0[r], k = a.seg0[r + 1] - s0, n = a.len[r];
    if (!k) { if (t == 0) a.out[r] = a.seed; return; }          // an empty range
    const unsigned long long per = (k + nthreads - 1) / nthreads, lo = per * t < k ? per * t : k, hi = lo + per < k ? lo + per : k;
    const uint32_t xlast = x8n(n - (k - 1) * kSegment);          // (every segment but the range's last is whole)
    uint32_t acc = 0;
    for (unsigned long long j = lo; j < hi; j++) acc = mulmod(acc, j == k - 1 ? xlast : kXSegment) ^ a.part[s0 + j];
    // acc stands at the end of segment hi - 1: k - hi segments lie behind it, the last of them the range's last
    if (lo < hi && hi < k) acc = mulmod(mulmod(acc, powmod(kXSegment, k - hi - 1)), xlast);
    acc = wave_xor(acc);
    if (xw::lane() == 0) L->wave[xw::wave()] = acc;
    xw::block_sync();
    if (t == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < nthreads / 64; w++) all ^= L->wave[w];
        a.out[r] = ~all;
    }
}

}  // namespace crc
}  // namespace nlzm
