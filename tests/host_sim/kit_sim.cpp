// kit_sim.cpp -- the guarded buffer every out-of-bounds claim of the CPU suite rests on (sim_kit.h), held to its own promises.  TEST HARNESS
// ONLY (tests/test_simkit.py; no fibers, so under AddressSanitizer and UBSan).
//
//   kit_sim          a buffer in each of the three places: its address, its fill, intact(), and intact() turning false after one byte
//                    written just outside it, inside the canary
//   kit_sim behind   reads the first byte of the PROT_NONE page behind a kBack buffer: the program must end with SIGSEGV
#include "sim_kit.h"

using namespace simkit;

const char simkit::kProgram[] = "kit_sim";

int main(int argc, char **argv)
{
    const size_t n = 1000, mis = 7;
    for (Place place : { kMid, kFront, kBack }) {
        Guarded g;
        g.make(n, mis, 0x5C, place);
        uint8_t *want = place == kMid ? g.lo + kCanary + mis : place == kFront ? g.lo : g.hi - n;
        if (g.p() != want || (uintptr_t)g.lo % page() || (size_t)(g.hi - g.lo) != pages_for(n + 2 * kCanary + 64)) { printf("FAIL: place %d: the buffer's address\n", place); return 1; }
        if (g.p()[0] != 0x5C || g.p()[n - 1] != 0x5C || !g.intact()) { printf("FAIL: place %d: fill, or a fresh buffer is not intact\n", place); return 1; }
        uint8_t *outside = place == kBack ? g.p() - 1 : g.p() + n;      // (behind a kBack buffer there is no canary: the page is)
        *outside ^= 0xFF;
        if (g.intact()) { printf("FAIL: place %d: a byte outside the buffer changed and intact() says nothing\n", place); return 1; }
        if (argc == 2 && !strcmp(argv[1], "behind") && place == kBack) return *(volatile uint8_t *)g.hi;
    }
    printf("kit_sim: OK\n");
    return 0;
}
