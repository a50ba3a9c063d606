// nlzm_report.h -- what the compress pipeline says about itself, with no device in it: pure functions of the structs the device fills
// (Persist::prof, WorkerCounters, v2::Hx; the slots' names are beside the structs, nlzm_core.h and nlzm_v2.h).  The library
// (nlzm_hip.cpp, nlzm_hip_blocks.cpp) and a CPU harness (tests/host_sim/report_sim.cpp, held to tests/golden/report_*.txt) include this one text:
//   stage_report        the stages' accounting of a stream (option "stage_report")
//   worker_report       ... and the worker lanes'
//   kAcctRows, acct_figures   the eight cycles-per-position figures a block set's min / median / max table is made of, with their labels
//   compress_counter    nlzm_hip_get_counter's names of the compress side
//   stage_error_text    where every stage was when a launch failed: the stage part of the error message
// Standard library only; compiles with plain g++ -std=c++17 (under NLZM_SIM, as the simulation includes nlzm_v2.h).
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "nlzm_v2.h"

namespace nlzm {

// per-stage accounting of the three-stage pipeline (Persist::prof, filled by nlzm_v2.h)
inline void stage_report(FILE *f, const Persist &P)
{
    static_assert(kPfTableFrontN == 5 && kPfFinderSecN == 8 && kPfParserWaveN == 4 && kPfParserLoaderSecN == 5 && kPfParserSecN == 7, "the lines below name every slot of these runs");
    const unsigned long long *p = P.prof;
    const double n = (double)(P.cnt.positions ? P.cnt.positions : 1);
    fprintf(f, "cycles/position  finder: total %.0f wait %.0f (%.0f of it for worker results) | table: total %.0f wait %.0f | parser: total %.0f wait %.0f (block set-up %.0f, passes %.0f, emit %.0f)\n",
            p[kPfFinderTotal] / n, p[kPfFinderWait] / n, p[kPfFinderWaitBt] / n, p[kPfTableTotal] / n, p[kPfTableWait] / n, p[kPfParserTotal] / n, p[kPfParserWait] / n,
            p[kPfParserSetup] / n, p[kPfParserPass] / n, p[kPfParserEmit] / n);
    fprintf(f, "finder: %llu blocks (%.1f positions each); cut by: nice %llu, new top entry %llu, RK candidate %llu, RK catch-up %llu, same worker bin %llu, other %llu\n",
            p[kPfFinderBlocks], n / (double)(p[kPfFinderBlocks] ? p[kPfFinderBlocks] : 1), p[kPfFinderCutNice], p[kPfFinderCutTop], p[kPfFinderCutRkCand], p[kPfFinderCutRkCatchUp],
            p[kPfFinderCutBin], p[kPfFinderCutOther]);
    fprintf(f, "table: %llu blocks, %llu on the slow path; parser: %llu blocks (%.1f nodes each), %.2f passes per block (%.0f cycles per pass), mask fills %llu, probe rounds %llu, re-sampled %llu\n",
            p[kPfTableBlocks], p[kPfTableSlowBlocks], p[kPfParserBlocks], n / (double)(p[kPfParserBlocks] ? p[kPfParserBlocks] : 1),
            (double)p[kPfParserPasses] / (double)(p[kPfParserBlocks] ? p[kPfParserBlocks] : 1), (double)p[kPfParserPass] / (double)(p[kPfParserPasses] ? p[kPfParserPasses] : 1),
            p[kPfParserMaskFills], p[kPfParserProbeRounds], p[kPfParserResampled]);
    fprintf(f, "table: %llu launches with %u-entry fronts on %u waves (the others: %u on %u), the shape changed %llu times\n", p[kPfTableWideLaunches], v2::kFrCapWide, v2::kTWWide, v2::kFrCap,
            v2::kTW, p[kPfTableShapeChanges]);
    {
        const double tb = (double)(p[kPfTableBlocks] ? p[kPfTableBlocks] : 1);
        fprintf(f, "table: blocks in which some position's front had more than 8 / 12 / 16 / 20 / 24 / the launch's capacity of entries at some step of the scan: %.2f / %.2f / %.2f / %.3f / %.3f / %.3f %%\n",
                100.0 * p[kPfTableFront + 0] / tb, 100.0 * p[kPfTableFront + 1] / tb, 100.0 * p[kPfTableFront + 2] / tb, 100.0 * p[kPfTableFront + 3] / tb, 100.0 * p[kPfTableFront + 4] / tb,
                100.0 * p[kPfTableSlowBlocks] / tb);
    }
    fprintf(f, "finder: RK256 entries cut short by the uint16 length parameter that became the growing top entry: %llu; that ended exactly where another entry ends: %llu (%llu of them the nearer one)\n",
            p[kPfRkShortTop], p[kPfRkShortTie], p[kPfRkShortWon]);
    fprintf(f, "finder: starts of nice regions whose segment the stage knew itself, ahead of the parser's word: %llu; that it had to wait for: %llu\n", p[kPfFinderSegOwn], p[kPfFinderSegWait]);
    fprintf(f, "finder: worker results not there at the first look: %llu of positions whose call is the finder's decision (unc), %llu of others\n", p[kPfFinderLateUnc], p[kPfFinderLateOther]);
    fprintf(f, "finder: blocks that had to wait for a worker result: %llu (%.0f cycles each); late results of hot bins' waves %llu, late results at lane 0 (the position the block before was cut at) %llu\n",
            p[kPfFinderLateBlocks], (double)p[kPfFinderWaitBt] / (double)(p[kPfFinderLateBlocks] ? p[kPfFinderLateBlocks] : 1), p[kPfFinderLateHot], p[kPfFinderLateFirst]);
    fprintf(f, "parser: waited for its record loader %llu times, the table stage %.0f positions ahead on average then\n", p[kPfParserNeed], (double)p[kPfParserAhead] / (double)(p[kPfParserNeed] ? p[kPfParserNeed] : 1));
    if (p[kPfHelpJobs] || p[kPfHelperJobs])
        fprintf(f, "helper parser: %llu jobs posted, %llu taken over (%llu nodes = %.1f %% of the positions), the parser stage waited %.0f cycles per position for it; "
                   "helper: %llu jobs seen, %llu done, %llu blocks (%.2f passes each), waited %.0f cycles per position for records\n",
                p[kPfHelpJobs], p[kPfHelpTaken], p[kPfHelpTakenNodes], 100.0 * p[kPfHelpTakenNodes] / n, p[kPfHelpWait] / n, p[kPfHelperJobs], p[kPfHelperDone], p[kPfHelperBlocks],
                (double)p[kPfHelperPasses] / (double)(p[kPfHelperBlocks] ? p[kPfHelperBlocks] : 1), p[kPfHelperWait] / n);
    if (p[kPfFinderSec]) {
        fprintf(f, "finder sections (cycles/position, profile build): predict %.0f, own loads %.0f, HT rows %.0f, candidates + jobs %.0f, record + RK256 %.0f, "
                   "BT4 results (wait included) %.0f, verify %.0f, commit %.0f\n", p[kPfFinderSec + 0] / n, p[kPfFinderSec + 1] / n, p[kPfFinderSec + 2] / n, p[kPfFinderSec + 3] / n,
                p[kPfFinderSec + 4] / n, p[kPfFinderSec + 5] / n, p[kPfFinderSec + 6] / n, p[kPfFinderSec + 7] / n);
    }
    if (p[kPfTableGather])
        fprintf(f, "table stage sections (cycles/position summed over the waves, profile build): gather %.0f, scan %.0f, waiting for the carry %.0f, carry merge (the part in block order) %.0f, records %.0f\n",
                p[kPfTableGather] / n, p[kPfTableScan] / n, p[kPfTableCarryWait] / n, p[kPfTableMerge] / n, p[kPfTableRecords] / n);
    if (p[kPfParserWaveWork]) {
        const double np = (double)(p[kPfParserPasses] ? p[kPfParserPasses] : 1);
        const unsigned long long *work = p + kPfParserWaveWork, *bar = p + kPfParserWaveBar;
        fprintf(f, "parser, cycles per pass (profile build): relax waves %.0f %.0f %.0f, probe wave %.0f (of it: sets that changed %.0f, mask fills %.0f), update %.0f, "
                   "barrier waits per wave %.0f %.0f %.0f %.0f; block end %.0f cycles/position\n",
                work[0] / np, work[1] / np, work[2] / np, work[3] / np, p[kPfParserDirty] / np, p[kPfParserFill] / np, p[kPfParserUpdate] / np,
                bar[0] / np, bar[1] / np, bar[2] / np, bar[3] / np, p[kPfParserBlockEnd] / n);
        fprintf(f, "parser, cycles per pass by wave 0..7 (profile build): work");
        for (uint32_t w = 0; w < kPfParserAllN; w++) fprintf(f, " %.0f", p[kPfParserAllWork + w] / np);
        fprintf(f, " | barrier wait");
        for (uint32_t w = 0; w < kPfParserAllN; w++) fprintf(f, " %.0f", p[kPfParserAllBar + w] / np);
        fprintf(f, " | update");
        for (uint32_t w = 0; w < kPfParserAllN; w++) fprintf(f, " %.0f", p[kPfParserAllUpdate + w] / np);
        fprintf(f, "\n");
        const double nbk = (double)(p[kPfParserBlocks] ? p[kPfParserBlocks] : 1);
        const unsigned long long *q = p + kPfParserLoaderSec, *s = p + kPfParserSec;
        fprintf(f, "parser loader wave, cycles per block set-up: block size + barrier %.0f, re-list %.0f, own edges %.0f, all edges %.0f, literal scan + clear + barrier %.0f\n",
                q[0] / nbk, q[1] / nbk, q[2] / nbk, q[3] / nbk, q[4] / nbk);
        fprintf(f, "parser wave 0, cycles per pass: relax %.0f, probe %.0f, clear %.0f | update: keys + cost scan %.0f, membership %.0f, winner sets %.0f, rest %.0f\n",
                s[0] / np, s[1] / np, s[2] / np, s[3] / np, s[4] / np, s[5] / np, s[6] / np);
    }
}
// ... and of the worker lanes
inline void worker_report(FILE *f, const WorkerCounters &wc, bool hot)
{
    static_assert(kHcSecN == 7, "the section line names every one");
    fprintf(f, "worker lanes: %llu calls made with their fate open (at and behind a position not decided yet), %llu decisions that took calls back, %llu calls made again for it\n",
            wc.dry_runs, wc.spec_calls, wc.spec_good);
    if (hot)
        fprintf(f, "hot bins (a wave each): %llu over all launches, %llu of %llu calls made by their waves\n", wc.hot_bins, wc.hot_calls, wc.bt_calls);
    if (hot && wc.hot_steps) {
        fprintf(f, "hot bins' waves: %llu steps (%.1f per call); the next call could not start in %.1f %% of them (a call without its stores on its way) + %.1f %% (an assumed \"skip\" behind a \"call\" still open); lanes: %llu turns spent waiting for a decision\n",
                wc.hot_steps, (double)wc.hot_steps / (wc.hot_calls ? wc.hot_calls : 1), 100.0 * wc.hot_blocked_dry / wc.hot_steps, 100.0 * wc.hot_blocked_risky / wc.hot_steps, wc.flag_waits);
        // (what a step was spent on is counted by the profile build only: the counting was a tenth of the step)
        fprintf(f, "hot bins' waves by the bin's positions in the launch (class: waves | calls, tests/call, entries skipped | steps, cycles/step; the profile build adds | %% of the steps: some lane tests "
                   "(tests per such step; lane-steps repeated for a held slot per step), taking back, every lane holds a call, next call may not start, no entry | idle steps with an undecided position open)\n");
        for (int k = 0; k < 8; k++) {
            const unsigned long long *h = wc.hot_class[k], *sec = h + kHcSec;
            if (!h[kHcWaves]) continue;
            const double st = (double)(h[kHcSteps] ? h[kHcSteps] : 1);
            fprintf(f, "  %s %7u: %5llu | %10llu calls, %5.1f, %10llu | %12llu steps, %5.0f", k ? ">=" : "< ", k ? 8192u << k : 16384u, h[kHcWaves], h[kHcCalls],
                    (double)h[kHcTests] / (h[kHcCalls] ? h[kHcCalls] : 1), h[kHcSkipped], h[kHcSteps], (double)h[kHcCycles] / st);
            if (sec[0] + sec[2]) {
                fprintf(f, " | %4.1f (%.2f; %.2f), %4.1f, %4.1f, %4.1f, %4.1f | %4.1f\n", 100.0 * h[kHcTestSteps] / st, (double)h[kHcLaneTests] / (h[kHcTestSteps] ? h[kHcTestSteps] : 1),
                        (double)h[kHcRepeats] / st, 100.0 * h[kHcTakingBack] / st, 100.0 * h[kHcAllHold] / st, 100.0 * h[kHcMayNotStart] / st, 100.0 * h[kHcNoEntry] / st, 100.0 * h[kHcIdleUndecided] / st);
                fprintf(f, "              cycles of a step by section: end of the step before + windows %.0f, oldest undecided + recovery %.0f, entries passed + start %.0f, loads until they are back %.0f, "
                           "call start / test %.0f, call end + result %.0f, accounting + watchdogs %.0f\n", sec[6] / st, sec[0] / st, sec[1] / st, sec[2] / st, sec[3] / st, sec[4] / st, sec[5] / st);
            } else fprintf(f, "\n");
        }
    }
    if (wc.call_tests)
        fprintf(f, "worker lanes: %.0f cycles per BT4 test, %.1f tests per timed call (lane clocks, divergence included)\n",
                (double)wc.call_cycles / wc.call_tests, (double)wc.call_tests / (wc.bt_calls ? wc.bt_calls : 1));
}

// which stage limits a stream: cycles per position, the rows of a block set's min / median / max table
constexpr struct { const char *label; uint32_t slot; } kAcctRows[8] = {
    { "finder total", kPfFinderTotal }, { "finder waiting", kPfFinderWait }, { "  of it for BT4 results", kPfFinderWaitBt }, { "table stage total", kPfTableTotal },
    { "table stage waiting", kPfTableWait }, { "parser total", kPfParserTotal }, { "parser waiting (records)", kPfParserWait }, { "parser passes", kPfParserPass },
};
inline void acct_figures(const Persist &P, double out[8])
{
    const double n = (double)(P.cnt.positions ? P.cnt.positions : 1);
    for (int k = 0; k < 8; k++) out[k] = P.prof[kAcctRows[k].slot] / n;
}

// nlzm_hip_get_counter, the compress side: false when the name is none of its
inline bool compress_counter(const char *key, const unsigned long long *prof, const WorkerCounters &wc, unsigned long long positions, uint64_t *value)
{
    static const struct { const char *name; uint32_t slot; } kProf[] = {
        { "finder_blocks", kPfFinderBlocks }, { "table_blocks", kPfTableBlocks }, { "parser_blocks", kPfParserBlocks }, { "parser_passes", kPfParserPasses },
        { "finder_wait_cycles", kPfFinderWait }, { "finder_total_cycles", kPfFinderTotal }, { "table_wait_cycles", kPfTableWait }, { "table_total_cycles", kPfTableTotal },
        { "parser_wait_cycles", kPfParserWait }, { "parser_total_cycles", kPfParserTotal }, { "parser_emit_cycles", kPfParserEmit }, { "parser_setup_cycles", kPfParserSetup },
        { "parser_pass_cycles", kPfParserPass }, { "finder_bt_wait_cycles", kPfFinderWaitBt }, { "table_slow_blocks", kPfTableSlowBlocks }, { "rk_cut_short_grown", kPfRkShortTop },
        { "rk_cut_short_ties", kPfRkShortTie }, { "rk_cut_short_ties_won", kPfRkShortWon }, { "table_shape_changes", kPfTableShapeChanges }, { "table_wide_launches", kPfTableWideLaunches },
        { "finder_seg_own", kPfFinderSegOwn }, { "finder_seg_waited", kPfFinderSegWait }, { "helper_jobs", kPfHelpJobs }, { "helper_taken", kPfHelpTaken },
        { "helper_taken_nodes", kPfHelpTakenNodes }, { "helper_wait_cycles", kPfHelpWait }, { "helper_jobs_done", kPfHelperDone }, { "helper_blocks", kPfHelperBlocks },
        { "helper_passes", kPfHelperPasses },
    };
    for (const auto &e : kProf) if (!strcmp(key, e.name)) { *value = prof[e.slot]; return true; }
    if (!strcmp(key, "worker_call_cycles")) { *value = wc.call_cycles; return true; }
    if (!strcmp(key, "worker_call_tests")) { *value = wc.call_tests; return true; }
    if (!strcmp(key, "worker_calls")) { *value = wc.bt_calls; return true; }
    if (!strcmp(key, "hot_bin_calls")) { *value = wc.hot_calls; return true; }
    if (!strcmp(key, "positions")) { *value = positions; return true; }
    return false;
}

// the first error any stage raised, and where every stage was when it left (nlzm_v2.h: raise(), Hx::dbg)
inline void stage_error_text(char *buf, size_t cap, const v2::Hx &h, const WorkerCounters &wc)
{
    const uint32_t *fi = h.dbg[v2::kDbgFinder], *tb = h.dbg[v2::kDbgTable], *pa = h.dbg[v2::kDbgParser];
    snprintf(buf, cap,
             "raised by stage %u at wait site %u, position %u, saw %u %u | "
             "progress: finder %u, table in %u out %u, parser %u, segment %u covered to %u | "
             "finder: block at %u reach %u top entry %u d %u end %u prev_nice %u seg_s %u rk_len %u t_pos_seen %u err %u base %u | "
             "table: cursor %u turn %u carry_seq %u f_seen %u p_seen %u carry_n %u | "
             "parser: chunk %u segment %u block node %u max_parse %u staged to %u t_out_seen %u err %u | "
             "worker lanes left waiting %llu, first of them at position %u",
             h.err_info[0], h.err_info[1], h.err_info[2], h.err_info[3], h.err_info[4],
             h.f_pos, h.t_pos, h.t_out, h.p_pos, (uint32_t)(h.p_seg >> 32), (uint32_t)h.p_seg,
             fi[v2::kDfBlock], fi[v2::kDfReach], fi[v2::kDfTopActive], fi[v2::kDfTopDist], fi[v2::kDfTopEnd], fi[v2::kDfPrevNice], fi[v2::kDfSegStart], fi[v2::kDfRkLen],
             fi[v2::kDfTPosSeen], fi[v2::kDfErr], fi[v2::kDfBase],
             tb[v2::kDtCursor], tb[v2::kDtTurn], tb[v2::kDtCarrySeq], tb[v2::kDtFSeen], tb[v2::kDtPSeen], tb[v2::kDtCarryN],
             pa[v2::kDpChunk], pa[v2::kDpSegment], pa[v2::kDpBlockNode], pa[v2::kDpMaxParse], pa[v2::kDpStaged], pa[v2::kDpTOutSeen], pa[v2::kDpErr],
             wc.stuck_lanes, wc.stuck_lanes ? (uint32_t)~(uint32_t)wc.stuck_pos_inv : 0u);
}

}  // namespace nlzm
