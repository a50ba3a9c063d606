// nlzm_index.h -- the sidecar index of a block container ([output].idx), with no device and no library call in it: THE
// definition of the format.  The command line (nlzm_cli.cpp) and the CPU harness tests/host_sim/index_sim.cpp include this one text.
// Numbers separated by white space, in three versions:
//   NLZMIDX 1 k n_in n_out          then k entries  off len raw            (c -blocks:k)
//   NLZMIDX 2 k n_in n_out WHOLE    then k entries  off len raw CRC        (c -crc: the CRC32 of the block's bytes; WHOLE, the whole input's)
//   NLZMIDX 3 k n_in n_out WHOLE    then k entries  off len raw CRC elem   (c -elem:E: the block's bytes are byte planes at element size elem, the CRC32s the RAW bytes')
// off, len: where the block's stream lies in the container; raw: the input bytes it holds; n_in, n_out: the sums of raw and of len.
// parse() reads the text and judges nothing; structural() holds an index against itself, for a reader that does not look at the container (x);
// fits_file() holds it against the container's bytes (d, t); write() makes the text.  What a reader takes beyond that it says in an Accept.
#pragma once

#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace nlzm {
namespace index {

// the field layout, once for the parser and the writer (scanf reads a number as printf writes it: PRIu64 is SCNu64 here)
#define NLZM_INDEX_HEAD  "NLZMIDX %u %u %" PRIu64 " %" PRIu64
#define NLZM_INDEX_ENTRY "%" PRIu64 " %" PRIu64 " %" PRIu64

struct Index {
    bool present = false;                           // the file could be opened
    unsigned version = 0;                           // set as soon as the header word and a number behind it are read, whatever follows
    bool header = false;                            // all the header's fields of that version were there (versions 1 to 3)
    uint32_t k = 0;                                 // the blocks the header announces
    uint64_t n_in = 0, n_out = 0;
    uint32_t whole = 0;
    std::vector<uint64_t> off, len, raw;            // the entries that could be read, in order: k of them, or fewer where the text stops being one
    std::vector<uint32_t> crc;                      // (version 1: 0)
    std::vector<uint8_t> elem;                      // (versions 1 and 2: 1)
    bool trailing = false;                          // all k entries were read and a field follows them
    bool has_crc() const { return version >= 2; }
    bool typed() const { return version == 3; }
};

// scanf's reading of a number, as the index has been read since version 1: white space, a sign and a 0x in front of a CRC are taken, a number too
// large saturates.  An entry whose element size is none of 1, 2, 4, 8 is no entry: the entries end in front of it.
inline void parse(FILE *f, Index &ix)
{
    ix = Index{};
    ix.present = true;
    const int got = fscanf(f, NLZM_INDEX_HEAD, &ix.version, &ix.k, &ix.n_in, &ix.n_out);
    ix.header = got == 4 && ix.version >= 1 && ix.version <= 3 && (ix.version == 1 || fscanf(f, "%x", &ix.whole) == 1);
    for (uint32_t i = 0; ix.header && i < ix.k; i++) {
        uint64_t off = 0, len = 0, raw = 0;
        unsigned crc = 0, elem = 1;
        if (fscanf(f, NLZM_INDEX_ENTRY, &off, &len, &raw) != 3 || (ix.version >= 2 && fscanf(f, "%x", &crc) != 1)) return;
        if (ix.version == 3 && (fscanf(f, "%u", &elem) != 1 || (elem != 1 && elem != 2 && elem != 4 && elem != 8))) return;
        ix.off.push_back(off); ix.len.push_back(len); ix.raw.push_back(raw); ix.crc.push_back(crc); ix.elem.push_back((uint8_t)elem);
    }
    char extra[2];
    ix.trailing = ix.header && fscanf(f, "%1s", extra) == 1;
}
inline void parse(const char *path, Index &ix)
{
    ix = Index{};
    if (FILE *f = fopen(path, "rb")) { parse(f, ix); fclose(f); }
}

// what a reader takes: the newest version it knows, the most blocks, and whether fields behind the last entry are let pass
struct Accept { unsigned max_version; uint32_t max_blocks; bool trailing_ok; };
inline bool acceptable(const Index &ix, const Accept &a)
{
    return ix.header && ix.version <= a.max_version && ix.k >= 1 && ix.k <= a.max_blocks && (!ix.trailing || a.trailing_ok);
}

// The index against itself: every entry there, offsets back to back, no sum that wraps, lengths summing to n_out and raw lengths to n_in.
inline bool structural(const Index &ix, const Accept &a)
{
    if (!acceptable(ix, a) || ix.off.size() != ix.k) return false;
    uint64_t expect = 0, raw_sum = 0;
    for (uint32_t i = 0; i < ix.k; i++) {
        if (ix.off[i] != expect || ix.len[i] < 8 || ix.len[i] > ix.n_out - expect || ix.raw[i] > ix.n_in - raw_sum) return false;
        expect += ix.len[i]; raw_sum += ix.raw[i];
    }
    return expect == ix.n_out && raw_sum == ix.n_in;
}

// The index against the container's `size` bytes: every block's stream starts with a stream header and ends with a terminator (NLZM.cpp:1915-1921,
// :646-648), and the sums are the file's.  A file that ends inside a block is a container cut off there: the blocks in front of it are whole and
// counted, the entries behind it are not looked at, cut_tail says how many bytes of the cut block are present.  Returns the blocks to decode, 0
// when the index does not fit.
inline size_t fits_file(const Index &ix, const Accept &a, const uint8_t *file, size_t size, size_t &cut_tail)
{
    cut_tail = 0;
    if (!acceptable(ix, a) || ix.n_out < size) return 0;
    uint64_t expect = 0, raw_sum = 0;
    for (size_t n = 0; n < ix.k; n++) {
        if (n >= ix.off.size()) return 0;
        const uint64_t off = ix.off[n], len = ix.len[n];
        if (off != expect || len < 8 || off > size || ix.raw[n] > ix.n_in - raw_sum) return 0;
        if (len > size - off) { cut_tail = n ? size - (size_t)expect : 0; return n; }       // (no off + len, which can wrap; no block in front of the cut: no fit)
        const uint8_t *s = file + off;
        if (s[0] != 0 || s[1] < 10 || s[1] > 28 || s[len - 4] || s[len - 3] || s[len - 2] || s[len - 1]) return 0;
        expect = off + len; raw_sum += ix.raw[n];
    }
    return expect == size && ix.n_out == size && raw_sum == ix.n_in ? ix.k : 0;
}

inline void write(FILE *f, const Index &ix)
{
    fprintf(f, NLZM_INDEX_HEAD, ix.version, (unsigned)ix.off.size(), ix.n_in, ix.n_out);
    if (ix.has_crc()) fprintf(f, " %08X", ix.whole);
    for (size_t i = 0; i < ix.off.size(); i++) {
        fprintf(f, "\n" NLZM_INDEX_ENTRY, ix.off[i], ix.len[i], ix.raw[i]);
        if (ix.has_crc()) fprintf(f, " %08X", ix.crc[i]);
        if (ix.typed()) fprintf(f, " %u", (unsigned)ix.elem[i]);
    }
    fprintf(f, "\n");
}

}  // namespace index
}  // namespace nlzm
