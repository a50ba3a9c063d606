// xw_probe_sim.cpp -- the xw.h probe role (tests/xw_probe/xw_probe.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_xw_sim.py; tests/xw_model.py makes the input table and holds the expected output).
//
//   xw_probe_sim <in.bin> <out0.bin> <out1.bin>
//       the input table (uint32 words); phase 0 and phase 1 are launched one after the other as one workgroup of 256 lanes, over the same
//       zeroed `g` words, and each phase's output table is written out.  Every buffer lies flush against a PROT_NONE page behind it, so
//       an index past a table's end is a SIGSEGV of the harness.
#define NLZM_SIM 1
#include "../xw_probe/xw_probe.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

namespace {

// `words` uint32 words whose last one lies flush against a PROT_NONE page
uint32_t *guarded(size_t words)
{
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), bytes = words * 4, n = (bytes + pg - 1) / pg * pg;
    uint8_t *m = (uint8_t *)mmap(nullptr, n + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED || mprotect(m, pg, PROT_NONE) || mprotect(m + pg + n, pg, PROT_NONE)) { fprintf(stderr, "xw_probe_sim: no guarded buffer\n"); exit(2); }
    return (uint32_t *)(m + pg + n - bytes);
}

void entry(void *arg) { xwp::probe_role(*(const xwp::Args *)arg); }

void spill(const char *path, const uint32_t *p, size_t words)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 4, words, f) != words) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: see the head of xw_probe_sim.cpp\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    if (sz < (long)(4 * xwp::kHead) || sz % 4) { fprintf(stderr, "xw_probe_sim: not a table\n"); return 2; }
    const size_t in_words = (size_t)sz / 4;
    uint32_t *in = guarded(in_words);
    if (fread(in, 4, in_words, f) != in_words) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    const uint32_t nc = in[1], ne = in[2];
    if (in[0] != xwp::kMagic || nc > 4096 || ne > 4096 || in_words != xwp::in_words(nc, ne)) { fprintf(stderr, "xw_probe_sim: the table's size does not fit its header\n"); return 2; }
    const size_t n0 = xwp::out_words(nc, ne), n1 = xwp::out2_words();
    uint32_t *out0 = guarded(n0), *out1 = guarded(n1), *g = guarded(xwp::gWords);
    for (size_t i = 0; i < n0; i++) out0[i] = xwp::kSentinel;
    for (size_t i = 0; i < n1; i++) out1[i] = xwp::kSentinel;
    memset(g, 0, 4 * xwp::gWords);
    const unsigned long long lds = sizeof(xwp::Lds);
    for (uint32_t phase = 0; phase < 2; phase++) {
        xwp::Args A{ in, phase ? out1 : out0, g, phase };
        xw::launch(1, xwp::kThreads, &lds, entry, &A);
    }
    spill(argv[2], out0, n0);
    spill(argv[3], out1, n1);
    printf("xw_probe_sim: OK\n");
    return 0;
}
