// xw_probe_sim.cpp -- the xw.h probe role (tests/xw_probe/xw_probe.h) run on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY
// (tests/test_xw_sim.py; tests/xw_model.py makes the input table and holds the expected output).
//
//   xw_probe_sim <in.bin> <out0.bin> <out1.bin>
//       the input table (uint32 words); phase 0 and phase 1 are launched one after the other as one workgroup of 256 lanes, over the same
//       zeroed `g` words, and each phase's output table is written out.  Every buffer lies flush against a PROT_NONE page behind it, so
//       an index past a table's end is a SIGSEGV of the harness.
#define NLZM_SIM 1
#include "../xw_probe/xw_probe.h"
#include "sim_kit.h"
#include "xw_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace simkit;

const char simkit::kProgram[] = "xw_probe_sim";

namespace {

// `words` uint32 words whose last one lies flush against a PROT_NONE page
uint32_t *guarded(Guarded &g, size_t words)
{
    g.make(words * 4);
    return (uint32_t *)(g.hi - words * 4);
}

void entry(void *arg) { xwp::probe_role(*(const xwp::Args *)arg); }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: see the head of xw_probe_sim.cpp\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    if (sz < (long)(4 * xwp::kHead) || sz % 4) { fprintf(stderr, "xw_probe_sim: not a table\n"); return 2; }
    const size_t in_words = (size_t)sz / 4;
    Guarded maps[4];
    uint32_t *in = guarded(maps[0], in_words);
    if (fread(in, 4, in_words, f) != in_words) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    const uint32_t nc = in[1], ne = in[2];
    if (in[0] != xwp::kMagic || nc > 4096 || ne > 4096 || in_words != xwp::in_words(nc, ne)) { fprintf(stderr, "xw_probe_sim: the table's size does not fit its header\n"); return 2; }
    const size_t n0 = xwp::out_words(nc, ne), n1 = xwp::out2_words();
    uint32_t *out0 = guarded(maps[1], n0), *out1 = guarded(maps[2], n1), *g = guarded(maps[3], xwp::gWords);
    for (size_t i = 0; i < n0; i++) out0[i] = xwp::kSentinel;
    for (size_t i = 0; i < n1; i++) out1[i] = xwp::kSentinel;
    memset(g, 0, 4 * xwp::gWords);
    const unsigned long long lds = sizeof(xwp::Lds);
    for (uint32_t phase = 0; phase < 2; phase++) {
        xwp::Args A{ in, phase ? out1 : out0, g, phase };
        xw::launch(1, xwp::kThreads, &lds, entry, &A);
    }
    spill(argv[2], out0, 4 * n0);
    spill(argv[3], out1, 4 * n1);
    printf("xw_probe_sim: OK\n");
    return 0;
}
