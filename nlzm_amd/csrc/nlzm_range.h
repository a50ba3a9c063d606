// nlzm_range.h -- the gather role of the range reader (nlzm_hip_read_ranges*, nlzm_hip_range.cpp): a list of pieces {src, dst, len} in
// device memory, every piece copied.  Written against xw.h like the decoder role (nlzm_decode.h) and the CRC roles (nlzm_crc.h): the same
// source is the gfx950 kernel (nlzm_range.hip) and the fiber simulation (tests/host_sim/range_sim.cpp).
//
// A piece is cut into chunks of kChunk bytes, one wave per chunk, so that one large piece spreads over the device and thousands of small
// ones are one launch.  A chunk's wave copies
//   * the head, up to 15 bytes in front of the destination's first 16-byte boundary, byte by byte, lane l byte l;
//   * the middle in 16-byte stores that are ALIGNED ON THE DESTINATION SIDE, lane l units l, l + 64, ... (a wave's step is 1,024
//     consecutive bytes), four units of a lane in flight.  The source side of a unit is read as sixteen bytes at whatever address the
//     two phases leave: an unaligned load, which global memory serves at any byte address (the compiler is told the alignment is 1 and
//     chooses the width; DESIGN.md section 18 records what it chose).  No load reaches outside the piece, because a unit's source bytes
//     are exactly the sixteen bytes it stores;
//   * the tail, under 16 bytes, byte by byte.
// Reads stay inside [src, src + len), writes inside [dst, dst + len) of every piece; no alignment is asked of either side, and none of
// one side relative to the other.  Pieces of one launch may read overlapping sources; their destinations must not overlap.
#pragma once

#include "xw.h"
#include "nlzm_units.h"

namespace nlzm {
namespace range {

constexpr unsigned long long kChunk = 32768;        // bytes of a piece that one wave copies; a multiple of 1,024

struct Piece { const uint8_t *src; uint8_t *dst; unsigned long long len; };
// what the host hands a launch: piece p owns chunks [chunk0[p], chunk0[p + 1])
struct Args {
    const Piece *pieces;
    const unsigned long long *chunk0;               // npieces + 1 entries
    uint32_t npieces;
    unsigned long long nchunks;
};

struct alignas(16) V16 { uint32_t x, y, z, w; };
XW_FN V16 load16u(const uint8_t *p)                 // any address
{
    V16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
XW_FN void store16(uint8_t *p, const V16 &v) { *(V16 *)p = v; }      // p: 16-byte aligned

// n bytes from s to d by one wave (wave-uniform arguments)
XW_FN void copy_chunk(const uint8_t *s, uint8_t *d, unsigned long long n)
{
    const uint32_t l = xw::lane();
    unsigned long long head = (16u - (uint32_t)((unsigned long long)d & 15u)) & 15u;
    if (head > n) head = n;
    if (l < head) d[l] = s[l];
    const unsigned long long C = (n - head) >> 4;   // units of the middle
    const uint8_t *ms = s + head;
    uint8_t *md = d + head;
    unsigned long long u = l;
    for (; u + 192 < C; u += 256) {                 // (four loads in flight per lane)
        const V16 a = load16u(ms + 16 * u), b = load16u(ms + 16 * (u + 64)), c = load16u(ms + 16 * (u + 128)), e = load16u(ms + 16 * (u + 192));
        store16(md + 16 * u, a);
        store16(md + 16 * (u + 64), b);
        store16(md + 16 * (u + 128), c);
        store16(md + 16 * (u + 192), e);
    }
    for (; u < C; u += 64) store16(md + 16 * u, load16u(ms + 16 * u));
    const unsigned long long tail = head + (C << 4);
    if (tail + l < n) d[tail + l] = s[tail + l];
}

// wave `w` of `nwaves`: chunks w, w + nwaves, ... of all pieces
XW_FN void gather_role(const Args &a, unsigned long long w, unsigned long long nwaves)
{
    for (unsigned long long g = w; g < a.nchunks; g += nwaves) {
        const uint32_t lo = units::owner_of(a.chunk0, a.npieces, g);       // the piece whose chunks hold g
        const Piece p = a.pieces[lo];
        const unsigned long long at = (g - a.chunk0[lo]) * kChunk, left = p.len - at;
        copy_chunk(NLZM_GLOBAL(const uint8_t, p.src) + at, NLZM_GLOBAL(uint8_t, p.dst) + at, left < kChunk ? left : kChunk);
    }
}

}  // namespace range
}  // namespace nlzm
