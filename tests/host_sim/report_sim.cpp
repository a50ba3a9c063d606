// tests/host_sim/report_sim.cpp -- the compress pipeline's reports (nlzm_amd/csrc/nlzm_report.h, the text the library compiles) run on
// synthetic structs in which every slot holds a value of its own, so that a swapped pair of indices anywhere changes the text; what it
// prints is compared byte for byte with tests/golden/report_*.txt (tests/test_report.py).  TEST HARNESS ONLY; no fibers here.
//
//   report_sim all | fine | gates | cold | acct | counters | error
#define NLZM_SIM 1
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define NLZM_HD inline
#define NLZM_HDN
#include "../../nlzm_amd/csrc/nlzm_core.h"
#include "../../nlzm_amd/csrc/nlzm_report.h"

using namespace nlzm;

// every word of the struct a value of its own: word i holds base + step * i
template <class T, class W>
static void fill_words(T &t, W base, W step)
{
    std::vector<W> w(sizeof(T) / sizeof(W));
    for (size_t i = 0; i < w.size(); i++) w[i] = (W)(base + step * (W)i);
    memset(&t, 0, sizeof t);
    memcpy(&t, w.data(), w.size() * sizeof(W));
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    static Persist P;
    static WorkerCounters wc;
    static v2::Hx h;
    memset(&P, 0, sizeof P);
    for (uint32_t i = 0; i < kPfSlots; i++) P.prof[i] = 1000003ull * (i + 1);
    P.cnt.positions = 999983;
    fill_words(wc, 3000017ull, 30011ull);
    for (int k = 0; k < 8; k++) if (k != 0 && k != 3 && k != 7) memset(wc.hot_class[k], 0, sizeof wc.hot_class[k]);   // (the empty classes are passed over)
    fill_words(h, 1009u, 7u);

    if (!strcmp(what, "all") || !strcmp(what, "cold")) {
        stage_report(stdout, P);
        worker_report(stdout, wc, !strcmp(what, "all"));
    } else if (!strcmp(what, "fine")) {            // small divisors: no two slots round to the same figure
        P.cnt.positions = 997; P.prof[kPfParserPasses] = 1009; P.prof[kPfParserBlocks] = 1013; P.prof[kPfTableBlocks] = 1000003ull * 200; P.prof[kPfFinderLateBlocks] = 1019;
        for (auto &c : wc.hot_class) if (c[kHcWaves]) { c[kHcSteps] = 1021; c[kHcCalls] = 1031; c[kHcTestSteps] = 1033; }
        stage_report(stdout, P);
        worker_report(stdout, wc, true);
    } else if (!strcmp(what, "gates")) {           // every conditional section absent
        P.prof[kPfFinderSec] = P.prof[kPfTableGather] = P.prof[kPfParserWaveWork] = P.prof[kPfHelpJobs] = P.prof[kPfHelperJobs] = 0;
        stage_report(stdout, P);
        wc.call_tests = 0;
        for (auto &c : wc.hot_class) c[kHcSec] = c[kHcSec + 2] = 0;
        worker_report(stdout, wc, true);
        wc.hot_steps = 0;
        worker_report(stdout, wc, true);
    } else if (!strcmp(what, "acct")) {
        double a[8];
        acct_figures(P, a);
        for (int k = 0; k < 8; k++) printf("  %-26s %8.0f\n", kAcctRows[k].label, a[k]);
    } else if (!strcmp(what, "counters")) {
        static const char *const names[] = {
            "finder_blocks", "table_blocks", "parser_blocks", "parser_passes", "finder_wait_cycles", "finder_total_cycles", "table_wait_cycles", "table_total_cycles",
            "parser_wait_cycles", "parser_total_cycles", "parser_emit_cycles", "parser_setup_cycles", "parser_pass_cycles", "finder_bt_wait_cycles", "table_slow_blocks",
            "rk_cut_short_grown", "rk_cut_short_ties", "rk_cut_short_ties_won", "table_shape_changes", "table_wide_launches", "finder_seg_own", "finder_seg_waited",
            "helper_jobs", "helper_taken", "helper_taken_nodes", "helper_wait_cycles", "helper_jobs_done", "helper_blocks", "helper_passes",
            "worker_call_cycles", "worker_call_tests", "worker_calls", "hot_bin_calls", "positions", "no_such_counter" };
        for (const char *k : names) {
            uint64_t v = 0;
            if (compress_counter(k, P.prof, wc, P.cnt.positions, &v)) printf("%s %llu\n", k, (unsigned long long)v);
            else printf("%s: unknown\n", k);
        }
    } else if (!strcmp(what, "error")) {
        char buf[2048];
        stage_error_text(buf, sizeof buf, h, wc);
        printf("%s\n", buf);
    } else {
        fprintf(stderr, "usage: report_sim all | fine | gates | cold | acct | counters | error\n");
        return 2;
    }
    return 0;
}
