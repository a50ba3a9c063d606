// nlzm_cut.h -- content-defined cut points of bytes that lie in device memory, written against xw.h like the CRC's roles (nlzm_crc.h): the
// same source runs on gfx950 (nlzm_cut.hip) and in the fiber simulator (tests/host_sim/cut_sim.cpp).  tests/cut_model.py restates the rule.
//
// The rule.  G[b] = upper 32 bits of splitmix64(b).  h(p) = sum over j = 0 .. 31 of G[x[p - j]] << j, modulo 2^32, for p >= 31: the gear hash
// h = (h << 1) + G[byte], which has forgotten a byte after 32 steps.  Position p is a candidate when the top avg_bits bits of h(p) are zero; its
// boundary is p + 1.  Selection: s = 0; while n - s > min_len: e = the first candidate boundary in [s + min_len, min(s + max_len, n)], or that
// upper end when there is none; stop if e >= n; record the cut e; s = e.
//
//   scan role     One wave per segment of kSegment bytes.  The wave stages the segment and the 31 bytes in front of it into LDS -- coalesced
//                 16-byte loads, the unaligned head and tail byte by byte -- at an index that keeps the loads' alignment, padded by one word per
//                 512 bytes so that the 64 lanes' byte reads fall into 64 banks.  Lane l then rolls the hash over the run [512 l, 512 l + 512) of
//                 the segment, 31 bytes of warm-up first: one table lookup (LDS) per byte.  Its candidates are bits of a bitmap (bit p & 31 of
//                 word p >> 5), sixteen words a lane, and the wave writes the segment's candidate count, one word.
//   select role   The greedy rule is serial: ONE wave walks it.  From s + min_len it finishes the current segment in the bitmap, 64 words a
//                 step, skips whole segments by their counts, 64 a step, and finds the first set bit of the first segment that has one.  The cuts go to
//                 a list, as far as the list has room; the number of cuts and of candidates to two result words.
// No atomics: every word has one writer.  Reads stay inside [src, src + n).
#pragma once

#include "xw.h"

namespace nlzm {
namespace cut {

constexpr unsigned long long kSegment = 32768;      // bytes per segment (one wave); a multiple of 64 * 32
constexpr uint32_t kRun = (uint32_t)(kSegment / 64);    // bytes a lane rolls over
constexpr uint32_t kWarm = 31;                      // bytes in front of a position that its hash still knows
constexpr unsigned long long kNone = ~0ull;
// the staged bytes: byte k of [segment start - front, segment end) lies at index 32 + (address & 15) + k, index j in word (j >> 2) + (j >> 9)
constexpr uint32_t kStageTop = 32 + 15 + kWarm + (uint32_t)kSegment;
constexpr uint32_t kStageWords = (kStageTop >> 2) + (kStageTop >> 9) + 2;

constexpr unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct GearTable { uint32_t v[256]; };
constexpr GearTable make_gear()
{
    GearTable t{};
    for (uint32_t b = 0; b < 256; b++) t.v[b] = (uint32_t)(splitmix64(b) >> 32);
    return t;
}
#ifndef NLZM_SIM
__device__ __constant__ const GearTable kGear = make_gear();
#else
static const GearTable kGear = make_gear();
#endif

// what the host hands both launches
struct Args {
    const uint8_t *src;
    unsigned long long n, nsegs;
    uint32_t *bits;                                 // the bitmap: (n + 31) / 32 words
    uint32_t *count;                                // candidates per segment: nsegs words
    unsigned long long *cut;                        // the list: cut_cap entries
    unsigned long long *res;                        // res[0]: cuts the rule makes (may exceed cut_cap), res[1]: candidates
    unsigned long long cut_cap, min_len, max_len;
    uint32_t shift;                                 // 32 - avg_bits
};

// the workgroup's LDS: the table, then one stage per wave of the workgroup (the device launches one wave a workgroup)
struct Lds {
    uint32_t gear[256];
    uint32_t stage[kStageWords];
};
constexpr unsigned long long lds_bytes(uint32_t waves) { return sizeof(Lds) + (unsigned long long)(waves - 1) * kStageWords * 4; }

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

XW_FN uint32_t stage_at(uint32_t j) { return j + ((j >> 9) << 2); }        // byte address of index j in the stage
XW_FN uint32_t wave_add(uint32_t v)
{
    const uint32_t l = xw::lane();
    for (uint32_t d = 1; d < 64; d <<= 1) v += xw::shfl(v, l ^ d);
    return v;
}
XW_FN unsigned long long wave_add64(unsigned long long v)
{
    const uint32_t l = xw::lane();
    for (uint32_t d = 1; d < 64; d <<= 1) v += xw::shfl64(v, l ^ d);
    return v;
}

// segment g of the input: staged, hashed, its bitmap words and its count written.  Wave-uniform arguments; `stage` is this wave's.
XW_FN void scan_segment(const Args &a, const Lds *L, uint32_t *stage, unsigned long long g)
{
    const uint32_t l = xw::lane();
    const unsigned long long at = g * kSegment, left = a.n - at;
    const uint32_t seglen = (uint32_t)(left < kSegment ? left : kSegment), front = g ? kWarm : 0u;
    const uint8_t *q = a.src + at - front;          // the first byte staged
    const uint32_t total = front + seglen, base = 32u + (uint32_t)((unsigned long long)q & 15u);
    uint8_t *stage8 = (uint8_t *)stage;
    uint32_t head = (16u - (base & 15u)) & 15u;
    if (head > total) head = total;
    if (l < head) stage8[stage_at(base + l)] = q[l];
    const uint32_t chunks = (total - head) >> 4, tail = (total - head) & 15u;
    {
        const uint8_t *mid = q + head;
        const uint32_t j0 = base + head;            // a multiple of 16: a chunk lies in four consecutive words of the stage
        uint32_t c = l;
        for (; c + 192 < chunks; c += 256) {        // (four loads in flight per lane)
            const u4 v0 = load16(mid + 16u * c), v1 = load16(mid + 16u * (c + 64)), v2 = load16(mid + 16u * (c + 128)), v3 = load16(mid + 16u * (c + 192));
            uint32_t *w0 = stage + (stage_at(j0 + 16u * c) >> 2), *w1 = stage + (stage_at(j0 + 16u * (c + 64)) >> 2);
            uint32_t *w2 = stage + (stage_at(j0 + 16u * (c + 128)) >> 2), *w3 = stage + (stage_at(j0 + 16u * (c + 192)) >> 2);
            w0[0] = v0.x; w0[1] = v0.y; w0[2] = v0.z; w0[3] = v0.w;
            w1[0] = v1.x; w1[1] = v1.y; w1[2] = v1.z; w1[3] = v1.w;
            w2[0] = v2.x; w2[1] = v2.y; w2[2] = v2.z; w2[3] = v2.w;
            w3[0] = v3.x; w3[1] = v3.y; w3[2] = v3.z; w3[3] = v3.w;
        }
        for (; c < chunks; c += 64) {
            const u4 v = load16(mid + 16u * c);
            uint32_t *w = stage + (stage_at(j0 + 16u * c) >> 2);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        if (l < tail) stage8[stage_at(j0 + 16u * chunks + l)] = mid[16u * chunks + l];
    }
    xw::wave_sync();
    // lane l: positions [r0, r0 + len) of the segment.  The warm-up of the input's very first run reads indices nothing was staged at: what
    // they hold has left the hash after 32 bytes, and the positions below 31 are no candidates
    const uint32_t r0 = l * kRun;
    const uint32_t len = seglen > r0 ? (seglen - r0 < kRun ? seglen - r0 : kRun) : 0u;
    uint32_t cnt = 0;
    if (len) {
        uint32_t j = base + front + r0 - kWarm, h = 0;
        for (uint32_t k = 0; k < kWarm; k++, j++) h = (h << 1) + L->gear[stage8[stage_at(j)]];
        uint32_t *out = a.bits + (at >> 5) + (r0 >> 5);
        for (uint32_t t = 0; t < len; t += 32) {
            uint32_t word = 0;
            if (len - t >= 32) {
#pragma unroll 8
                for (uint32_t k = 0; k < 32; k++, j++) {
                    h = (h << 1) + L->gear[stage8[stage_at(j)]];
                    word |= (uint32_t)((h >> a.shift) == 0) << k;
                }
            } else {
                for (uint32_t k = 0; k < len - t; k++, j++) {
                    h = (h << 1) + L->gear[stage8[stage_at(j)]];
                    word |= (uint32_t)((h >> a.shift) == 0) << k;
                }
            }
            if (!g && !l && !t) word &= 0x80000000u;        // (positions 0 .. 30 of the input have no hash)
            out[t >> 5] = word;
            cnt += (uint32_t)__builtin_popcount(word);
        }
    }
    xw::wave_sync();                                // (the stage is written again for the wave's next segment)
    cnt = wave_add(cnt);
    if (l == 0) a.count[g] = cnt;
}

// wave `w` of `nwaves`: segments w, w + nwaves, ...  Called by every wave of the workgroup (the table is copied first).
XW_FN void scan_role(const Args &a, uint32_t nthreads, unsigned long long w, unsigned long long nwaves)
{
    Lds *L = xw::lds<Lds>();
    for (uint32_t b = xw::thread(); b < 256; b += nthreads) L->gear[b] = kGear.v[b];
    xw::block_sync();
    uint32_t *stage = L->stage + (size_t)xw::wave() * kStageWords;
    for (unsigned long long g = w; g < a.nsegs; g += nwaves) scan_segment(a, L, stage, g);
}

// the first candidate position in [lo, hi] (lo <= hi < n), kNone when there is none.  One wave; every lane returns the result.
XW_FN unsigned long long first_candidate(const Args &a, unsigned long long lo, unsigned long long hi)
{
    const uint32_t l = xw::lane();
    unsigned long long pos = lo;
    for (;;) {
        const unsigned long long seg = pos / kSegment, seg_last = (seg + 1) * kSegment - 1, last = hi < seg_last ? hi : seg_last;
        const unsigned long long w_lo = pos >> 5, w_hi = last >> 5;
        for (unsigned long long w = w_lo; w <= w_hi; w += 64) {
            const unsigned long long wi = w + l;
            uint32_t v = wi <= w_hi ? a.bits[wi] : 0u;
            if (wi == w_lo) v &= ~0u << (uint32_t)(pos & 31u);
            if (wi == w_hi) v &= ~0u >> (31u - (uint32_t)(last & 31u));
            const unsigned long long m = xw::ballot(v != 0);
            if (m) {
                const uint32_t f = (uint32_t)__builtin_ctzll(m);
                return ((w + f) << 5) + (uint32_t)__builtin_ctz(xw::readlane(v, f));
            }
        }
        if (last == hi) return kNone;
        // the segments behind it that hold no candidate, up to the one that holds hi
        unsigned long long g = seg + 1;
        const unsigned long long g_hi = hi / kSegment;
        for (;;) {
            const unsigned long long gi = g + l;
            const uint32_t c = gi <= g_hi ? a.count[gi] : 0u;
            const unsigned long long m = xw::ballot(c != 0);
            if (m) { g += (uint32_t)__builtin_ctzll(m); break; }
            if (g_hi - g < 64) return kNone;
            g += 64;
        }
        pos = g * kSegment;
    }
}

// the selection, by ONE wave
XW_FN void select_role(const Args &a)
{
    const uint32_t l = xw::lane();
    unsigned long long cand = 0;
    for (unsigned long long g = l; g < a.nsegs; g += 64) cand += a.count[g];
    cand = wave_add64(cand);
    unsigned long long s = 0, ncuts = 0;
    while (a.n - s > a.min_len) {
        const unsigned long long lo = s + a.min_len, hi = a.n - s > a.max_len ? s + a.max_len : a.n;
        const unsigned long long p = first_candidate(a, lo - 1, hi - 1);
        const unsigned long long e = p == kNone ? hi : p + 1;
        if (e >= a.n) break;
        if (l == 0 && ncuts < a.cut_cap) a.cut[ncuts] = e;
        ncuts++;
        s = e;
    }
    if (l == 0) { a.res[0] = ncuts; a.res[1] = cand; }
}

}  // namespace cut
}  // namespace nlzm
