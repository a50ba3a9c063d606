// nlzm_planes.h -- the byte-plane filter of typed ranges, both directions, for bytes that lie in device memory; written against xw.h like the gather
// role (nlzm_range.h) and the cut points' (nlzm_cut.h): the same source runs on gfx950 (nlzm_planes.hip) and in the fiber simulator
// (tests/host_sim/planes_sim.cpp).  tests/planes_model.py restates the rule.
//
// The rule.  For a range x of n bytes and an element size e in {1, 2, 4, 8}, m = n div e: planes_e(x) = y with y[j m + i] = x[i e + j] for 0 <= j < e,
// 0 <= i < m, and y[e m + t] = x[e m + t] for the n - e m tail bytes.  e = 1 is the identity.  Elements are counted from the range's own first byte: no
// address and no alignment enters the rule.
//
// k ranges are ONE launch.  A range is cut into segments of kSegment bytes of its interleaved side, one wave per segment; range r owns segments
// [seg0[r], seg0[r + 1]) (empty ranges own none), and waves stride over the segments.  A segment holds kSegment / e whole elements (the last one of a
// range fewer, and the range's tail bytes, which the wave copies as they are), so it is e plane runs of kSegment / e bytes on the plane side.
//
// The wave keeps an image of the segment's planes in LDS: row j, of kSegment / e + 16 bytes, holds plane j's run SHIFTED by the low four bits of
// that run's address on the plane side, so that sixteen aligned bytes of LDS are sixteen aligned bytes of the plane (the decoder ring's trick:
// flush / preload in nlzm_decode.h).
//   forward   the interleaved bytes are loaded once, in 16-byte units at whatever address the segment starts (range::load16u; under sixteen bytes at
//             the end byte by byte), and every byte of a unit is shifted out of its word and put at its place in its row; then every row's run is
//             stored: up to 15 bytes to the plane's first 16-byte boundary byte by byte, the middle in aligned 16-byte units read whole from LDS,
//             the rest byte by byte.
//   inverse   every plane's run is loaded the same way -- head, aligned 16-byte units written whole into its row, rest --, then every 16-byte unit
//             of the interleaved side is put together from the rows, byte by byte with shifts, and stored as the gather role stores a chunk: head,
//             16-byte units aligned on the destination, rest.
// No read leaves [src_off, src_off + len) of a range and no write [dst_off, dst_off + len); every byte is read once and written once; no atomics, no
// scratch; no alignment is asked of either side, or of one side relative to the other.  Source ranges of one launch may overlap; destinations must not.
#pragma once

#include "xw.h"
#include "nlzm_range.h"
#include "nlzm_units.h"

namespace nlzm {
namespace planes {

constexpr unsigned long long kSegment = 8192;       // bytes of a range's interleaved side that one wave handles; a multiple of 128 (sixteen elements of 8)
constexpr uint32_t kImage = (uint32_t)kSegment + 128;      // a wave's LDS image: e rows of kSegment / e + 16 bytes, e = 8 at most

// what the host hands a launch: five tables of one upload (nlzm_planes_plan.h, planes::Table).  The offsets are those of the INTERLEAVED side in
// `src` (forward) or `dst` (inverse) and of the plane side in the other.
struct Args {
    const uint8_t *src;
    uint8_t *dst;
    const unsigned long long *src_off, *dst_off, *len, *elem;      // k entries each
    const unsigned long long *seg0;                 // k + 1 entries
    uint32_t k;
    unsigned long long nsegs;
};

// the workgroup's LDS: one image per wave
struct alignas(16) Lds { uint8_t image[kImage]; };
constexpr unsigned long long lds_bytes(uint32_t waves) { return (unsigned long long)waves * kImage; }

using range::V16;
using range::load16u;
// sixteen bytes at a 16-byte aligned address, of global memory or of the image: ONE access (a vector of four words, which the compiler keeps whole)
#ifndef NLZM_SIM
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
XW_FN V16 get16(const uint8_t *p) { const v4u v = *(const v4u *)p; return V16{ v.x, v.y, v.z, v.w }; }
XW_FN void put16(uint8_t *p, const V16 &v) { *(v4u *)p = v4u{ v.x, v.y, v.z, v.w }; }
#else
XW_FN V16 get16(const uint8_t *p) { V16 v; memcpy(&v, p, 16); return v; }
XW_FN void put16(uint8_t *p, const V16 &v) { memcpy(p, &v, 16); }
#endif

// where byte `o` of a segment's interleaved side lies in the image: plane o mod E, element o div E; row j is shifted by (b0 + j m16) & 15, the low bits
// of q0 + j m, where plane 0's run of the segment starts at q0 on the plane side and m16 = m & 15
template <uint32_t E> XW_FN uint32_t image_at(uint32_t o, uint32_t b0, uint32_t m16)
{
    const uint32_t j = o % E;
    return j * ((uint32_t)kSegment / E + 16u) + ((b0 + j * m16) & 15u) + o / E;
}

// the sixteen bytes o, o + 1, ... of the interleaved side into their rows
template <uint32_t E> XW_FN void scatter16(uint8_t *image, uint32_t o, const V16 &v, uint32_t b0, uint32_t m16)
{
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) image[image_at<E>(o + b, b0, m16)] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
}
// ... and out of them
template <uint32_t E> XW_FN V16 collect16(const uint8_t *image, uint32_t o, uint32_t b0, uint32_t m16)
{
    uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) w[b >> 2] |= (uint32_t)image[image_at<E>(o + b, b0, m16)] << (8u * (b & 3u));
    return V16{ w[0], w[1], w[2], w[3] };
}

// `body` interleaved bytes at p (whole elements: a multiple of E, kSegment at most) to their planes: plane j's run is body / E bytes at q0 + j m.
// Wave-uniform arguments; `image` is this wave's.
template <uint32_t E> XW_FN void forward_segment(const uint8_t *p, uint8_t *q0, unsigned long long m, uint32_t body, uint8_t *image)
{
    const uint32_t l = xw::lane(), cnt = body / E, b0 = (uint32_t)((unsigned long long)q0 & 15u), m16 = (uint32_t)(m & 15u);
    const uint32_t U = body >> 4, rem = body & 15u;
    uint32_t u = l;
    for (; u + 192 < U; u += 256) {                 // (four loads in flight per lane)
        const V16 a = load16u(p + 16u * u), b = load16u(p + 16u * (u + 64)), c = load16u(p + 16u * (u + 128)), d = load16u(p + 16u * (u + 192));
        scatter16<E>(image, 16u * u, a, b0, m16);
        scatter16<E>(image, 16u * (u + 64), b, b0, m16);
        scatter16<E>(image, 16u * (u + 128), c, b0, m16);
        scatter16<E>(image, 16u * (u + 192), d, b0, m16);
    }
    for (; u < U; u += 64) scatter16<E>(image, 16u * u, load16u(p + 16u * u), b0, m16);
    if (l < rem) image[image_at<E>(16u * U + l, b0, m16)] = p[16u * U + l];
    xw::wave_sync();
    for (uint32_t j = 0; j < E; j++) {
        uint8_t *q = q0 + j * m;
        const uint32_t sh = (b0 + j * m16) & 15u;
        const uint8_t *row = image + j * ((uint32_t)kSegment / E + 16u) + sh;
        uint32_t head = (16u - sh) & 15u;
        if (head > cnt) head = cnt;
        if (l < head) q[l] = row[l];
        const uint32_t C = (cnt - head) >> 4;       // units of the middle: aligned in the plane, and in the image
        for (uint32_t v = l; v < C; v += 64) put16(q + head + 16u * v, get16(row + head + 16u * v));
        const uint32_t t = head + (C << 4);
        if (t + l < cnt) q[t + l] = row[t + l];
    }
    xw::wave_sync();                                // (the image is written again for the wave's next segment)
}

// the inverse: plane j's run of body / E bytes at p0 + j m, the interleaved bytes to q
template <uint32_t E> XW_FN void inverse_segment(const uint8_t *p0, uint8_t *q, unsigned long long m, uint32_t body, uint8_t *image)
{
    const uint32_t l = xw::lane(), cnt = body / E, b0 = (uint32_t)((unsigned long long)p0 & 15u), m16 = (uint32_t)(m & 15u);
    for (uint32_t j = 0; j < E; j++) {
        const uint8_t *p = p0 + j * m;
        const uint32_t sh = (b0 + j * m16) & 15u;
        uint8_t *row = image + j * ((uint32_t)kSegment / E + 16u) + sh;
        uint32_t head = (16u - sh) & 15u;
        if (head > cnt) head = cnt;
        if (l < head) row[l] = p[l];
        const uint32_t C = (cnt - head) >> 4;
        const uint8_t *mp = p + head;
        uint8_t *mr = row + head;
        uint32_t v = l;
        for (; v + 192 < C; v += 256) {             // (four loads in flight per lane)
            const V16 a = get16(mp + 16u * v), b = get16(mp + 16u * (v + 64)), c = get16(mp + 16u * (v + 128)), d = get16(mp + 16u * (v + 192));
            put16(mr + 16u * v, a);
            put16(mr + 16u * (v + 64), b);
            put16(mr + 16u * (v + 128), c);
            put16(mr + 16u * (v + 192), d);
        }
        for (; v < C; v += 64) put16(mr + 16u * v, get16(mp + 16u * v));
        const uint32_t t = head + (C << 4);
        if (t + l < cnt) row[t + l] = p[t + l];
    }
    xw::wave_sync();
    // the interleaved side as the gather role stores a chunk: head, 16-byte units aligned on the destination, rest
    uint32_t head = (16u - (uint32_t)((unsigned long long)q & 15u)) & 15u;
    if (head > body) head = body;
    if (l < head) q[l] = image[image_at<E>(l, b0, m16)];
    const uint32_t U = (body - head) >> 4;
    for (uint32_t u = l; u < U; u += 64) put16(q + head + 16u * u, collect16<E>(image, head + 16u * u, b0, m16));
    const uint32_t t = head + (U << 4);
    if (t + l < body) q[t + l] = image[image_at<E>(t + l, b0, m16)];
    xw::wave_sync();
}

// wave `w` of `nwaves`: segments w, w + nwaves, ... of all ranges.  Called by every wave of the workgroup.
XW_FN void planes_role(const Args &a, bool inverse, unsigned long long w, unsigned long long nwaves)
{
    uint8_t *image = xw::lds<Lds>()->image + (size_t)xw::wave() * kImage;
    const uint32_t l = xw::lane();
    for (unsigned long long g = w; g < a.nsegs; g += nwaves) {
        const uint32_t lo = units::owner_of(a.seg0, a.k, g);               // the range whose segments hold g
        const unsigned long long n = a.len[lo], e = a.elem[lo], m = n / e, whole = m * e, at = (g - a.seg0[lo]) * kSegment;
        const unsigned long long left = whole > at ? whole - at : 0;
        const uint32_t body = (uint32_t)(left < kSegment ? left : kSegment);
        const uint8_t *s = a.src + a.src_off[lo];
        uint8_t *d = a.dst + a.dst_off[lo];
        if (body) {
            const unsigned long long i0 = at / e;   // the segment's first element
            if (!inverse) {
                if (e == 1) forward_segment<1>(s + at, d + i0, m, body, image);
                else if (e == 2) forward_segment<2>(s + at, d + i0, m, body, image);
                else if (e == 4) forward_segment<4>(s + at, d + i0, m, body, image);
                else forward_segment<8>(s + at, d + i0, m, body, image);
            } else {
                if (e == 1) inverse_segment<1>(s + i0, d + at, m, body, image);
                else if (e == 2) inverse_segment<2>(s + i0, d + at, m, body, image);
                else if (e == 4) inverse_segment<4>(s + i0, d + at, m, body, image);
                else inverse_segment<8>(s + i0, d + at, m, body, image);
            }
        }
        // the range's tail bytes, fewer than e, lie in its last segment and stay where they are
        if (at + kSegment >= n && whole + l < n) d[whole + l] = s[whole + l];
    }
}

}  // namespace planes
}  // namespace nlzm
