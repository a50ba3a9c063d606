// index_sim.cpp -- the sidecar index's parser, validators and writer (nlzm_amd/csrc/nlzm_index.h) on their own: no device, no library.
// TEST HARNESS ONLY (tests/test_index_sim.py; built by the Makefile with -fsanitize=address,undefined).
//
//   index_sim roundtrip             the writer's text for every version word for word, and writer -> parser -> the same index, for 1, 5 and 300 blocks
//   index_sim judge <idx> <size>    the index text in <idx> through the parser, then through BOTH validators, each with what x takes of an index and
//                                   with what d / t take.  fits_file gets a container of <size> bytes made here: zeros, and a stream header wherever an
//                                   entry says a block starts (exactly <size> bytes on the heap: a read behind them is the sanitizer's to report).
//                                   Prints "parsed ..." and a line "x: ..." and "d: ..." with structural=0|1 fits_file=<blocks> cut_tail=<bytes>
#include "../../nlzm_amd/csrc/nlzm_index.h"

#include <stdlib.h>
#include <string.h>

#include <string>

using namespace nlzm::index;

namespace {

#define FAIL(...) do { printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

// the two readers of the command line (nlzm_cli.cpp: kExtractTakes, kDecodeTakes)
const Accept kX{ 2, 65536, false }, kD{ 3, 4096, true };

std::string text_of(const Index &ix)
{
    FILE *f = tmpfile();
    write(f, ix);
    const long n = ftell(f);
    std::string s((size_t)n, '\0');
    rewind(f);
    if (fread(&s[0], 1, (size_t)n, f) != (size_t)n) s.clear();
    fclose(f);
    return s;
}
Index parsed(const std::string &text)
{
    FILE *f = tmpfile();
    fwrite(text.data(), 1, text.size(), f);
    rewind(f);
    Index ix;
    parse(f, ix);
    fclose(f);
    return ix;
}
Index make(unsigned version, uint32_t k)
{
    Index ix;
    ix.version = version;
    uint64_t seed = 88172645463325252ull + k;
    for (uint32_t i = 0; i < k; i++) {
        seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
        ix.off.push_back(ix.n_out); ix.len.push_back(8 + seed % 100000); ix.raw.push_back((seed >> 20) % 300000);
        ix.crc.push_back(version >= 2 ? (uint32_t)(seed >> 32) : 0); ix.elem.push_back(version == 3 ? (uint8_t)(1u << (seed % 4)) : 1);
        ix.n_out += ix.len.back(); ix.n_in += ix.raw.back();
    }
    ix.whole = version >= 2 ? 0xC0FFEE00u + k : 0;
    return ix;
}

int roundtrip()
{
    // the three layouts, and the index of one stream that `c -crc` writes
    Index a;
    a.n_in = 30; a.n_out = 20; a.whole = 0xABCD;
    a.off = { 0, 12 }; a.len = { 12, 8 }; a.raw = { 10, 20 }; a.crc = { 1, 2 }; a.elem = { 2, 8 };
    const char *want[4] = { "", "NLZMIDX 1 2 30 20\n0 12 10\n12 8 20\n", "NLZMIDX 2 2 30 20 0000ABCD\n0 12 10 00000001\n12 8 20 00000002\n",
                            "NLZMIDX 3 2 30 20 0000ABCD\n0 12 10 00000001 2\n12 8 20 00000002 8\n" };
    for (unsigned v = 1; v <= 3; v++) {
        a.version = v;
        if (text_of(a) != want[v]) FAIL("version %u is written as\n%s", v, text_of(a).c_str());
    }
    Index one;
    one.version = 2; one.n_in = 5; one.n_out = 9; one.whole = 0xFF;
    one.off = { 0 }; one.len = { 9 }; one.raw = { 5 }; one.crc = { 0xFF };
    if (text_of(one) != "NLZMIDX 2 1 5 9 000000FF\n0 9 5 000000FF\n") FAIL("one stream is written as\n%s", text_of(one).c_str());
    int cases = 0;
    for (unsigned v = 1; v <= 3; v++)
        for (uint32_t k : { 1u, 5u, 300u }) {
            const Index w = make(v, k), r = parsed(text_of(w));
            if (!r.header || r.version != v || r.k != k || r.n_in != w.n_in || r.n_out != w.n_out || r.whole != w.whole || r.trailing) FAIL("version %u, %u blocks: the header", v, k);
            if (r.off != w.off || r.len != w.len || r.raw != w.raw || r.crc != w.crc || r.elem != w.elem) FAIL("version %u, %u blocks: the entries", v, k);
            if (!structural(r, kD) || structural(r, kX) != (v <= 2)) FAIL("version %u, %u blocks: structural", v, k);
            cases++;
        }
    printf("roundtrip: cases=%d\n", cases);
    return 0;
}

int judge(const char *path, size_t size)
{
    Index ix;
    parse(path, ix);
    if (!ix.present) FAIL("%s cannot be opened", path);
    printf("parsed version=%u header=%d k=%u entries=%zu trailing=%d\n", ix.version, (int)ix.header, ix.k, ix.off.size(), (int)ix.trailing);
    uint8_t *file = (uint8_t *)calloc(size ? size : 1, 1);
    for (size_t i = 0; i < ix.off.size(); i++) if (ix.off[i] < size && size - ix.off[i] >= 2) file[ix.off[i] + 1] = 17;
    const Accept *takes[2] = { &kX, &kD };
    for (int t = 0; t < 2; t++) {
        size_t cut_tail = 0;
        const size_t n = fits_file(ix, *takes[t], file, size, cut_tail);
        printf("%s: structural=%d fits_file=%zu cut_tail=%zu\n", t ? "d" : "x", (int)structural(ix, *takes[t]), n, cut_tail);
    }
    free(file);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    int rc = 2;
    if (argc == 2 && !strcmp(argv[1], "roundtrip")) rc = roundtrip();
    else if (argc == 4 && !strcmp(argv[1], "judge")) rc = judge(argv[2], (size_t)strtoull(argv[3], nullptr, 10));
    else printf("usage: index_sim roundtrip | judge <idx> <size>\n");
    if (!rc) printf("index_sim: OK\n");
    return rc;
}
