// units_sim.cpp -- the unit table of the range kernels (nlzm_amd/csrc/nlzm_units.h: count, prefix, owner_of, blocks_for) in a program of its own, under
// AddressSanitizer and UBSan: the header the role headers, the host plans and the kernel files include, built here with plain g++.  TEST HARNESS ONLY
// (tests/test_units_sim.py, which holds the expected values: Python's integers and bisect).
//
//   units_sim <cases>     one line of output per line of <cases>:
//       C <len> <unit>                              units::count
//       P <unit> <n> <len> ... (n)                  units::prefix: the n + 1 words
//       O <n> <t[0]> .. <t[n]> <q> <u> ... (q)      units::owner_of(t, n, u) for every u (the table lies in an allocation of exactly n + 1 words)
//       B <units> <per_block> <max_blocks>          units::blocks_for
#include "../../nlzm_amd/csrc/nlzm_units.h"

#include <inttypes.h>
#include <stdio.h>

#include <vector>

using namespace nlzm;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: see the head of units_sim.cpp\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'C') {
            unsigned long long len, unit;
            if (fscanf(f, "%llu %llu", &len, &unit) != 2 || !unit) return 2;
            printf("%llu\n", units::count(len, unit));
        } else if (kind[0] == 'P') {
            unsigned long long unit;
            uint32_t n;
            if (fscanf(f, "%llu %" SCNu32, &unit, &n) != 2 || !unit) return 2;
            std::vector<unsigned long long> len(n);
            for (auto &l : len) if (fscanf(f, "%llu", &l) != 1) return 2;
            const std::vector<unsigned long long> t = units::prefix(n, unit, [&](uint32_t i) { return len[i]; });
            if (t.size() != (size_t)n + 1) return 3;
            for (size_t i = 0; i < t.size(); i++) printf("%llu%s", t[i], i + 1 < t.size() ? " " : "\n");
        } else if (kind[0] == 'O') {
            uint32_t n, q;
            if (fscanf(f, "%" SCNu32, &n) != 1 || !n) return 2;
            std::vector<unsigned long long> t((size_t)n + 1);
            for (auto &v : t) if (fscanf(f, "%llu", &v) != 1) return 2;
            if (fscanf(f, "%" SCNu32, &q) != 1) return 2;
            for (uint32_t i = 0; i < q; i++) {
                unsigned long long u;
                if (fscanf(f, "%llu", &u) != 1) return 2;
                printf("%" PRIu32 "%s", units::owner_of(t.data(), n, u), i + 1 < q ? " " : "");
            }
            printf("\n");
        } else if (kind[0] == 'B') {
            unsigned long long n;
            uint32_t per_block, max_blocks;
            if (fscanf(f, "%llu %" SCNu32 " %" SCNu32, &n, &per_block, &max_blocks) != 3 || !per_block) return 2;
            printf("%" PRIu32 "\n", units::blocks_for(n, per_block, max_blocks));
        } else return 2;
    }
    fclose(f);
    printf("units_sim: OK\n");
    return 0;
}
