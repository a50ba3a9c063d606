// nlzm_hip_blocks.cpp -- independent blocks: the block set (nlzm_hip_blocks_*), whose streams share one persistent
// launch a round, and the one-shot forms over it -- one set, or a container's sets one after another (nlzm_container_plan.h).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "nlzm_host_state.h"
#include "nlzm_container_plan.h"
#include "nlzm_dedup_host.h"
#include "nlzm_launch.h"
#include "nlzm_report.h"

using namespace nlzm;
using namespace nlzm::host;

namespace {

// a stream of a block set: the device of the set's context, a HIP stream and the events of both launch sets of its own
int block_ctx_init(Ctx &c, const Ctx &of)
{
    c.device = of.device; c.cu_count = of.cu_count;
    HIPCHK(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    for (auto &set : c.ev) for (auto &ev : set) HIPCHK(hipEventCreate(&ev));
    c.inited = true;
    return 0;
}
void block_ctx_destroy(Ctx &c)
{
    free_stream_buffers(c);
    for (auto &set : c.ev) for (auto &ev : set) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    release_launch_stream(c);           // (a stream that was made again as a single stream has one)
    if (c.st) { (void)hipStreamDestroy(c.st); c.st = nullptr; }
    c.inited = false;
}

// The options stream `index` of a block set is opened with, from the set's: what nlzm_hip_blocks_begin has fitted to the device (worker CUs per
// stream, chunks per launch, the pre-filter table's size at most) and the block_* options in the place of the single stream's.  The pass that
// measures what a stream takes and the pass that opens it both come here.
Options block_stream_options(const Options &S, int64_t worker_blocks, int64_t batch, int64_t tbits_max, uint32_t index)
{
    Options o = S;
    o.report = 0;
    o.worker_blocks = worker_blocks; o.batch = batch; o.tbits_max = tbits_max;
    o.worker_threads = S.block_threads;         // (block mode: a stream has few worker CUs)
    o.hot_waves = S.block_hot_waves;
    o.helper = S.block_helper;
    o.test_fail_launch = (int64_t)index == S.test_fail_stream ? S.test_fail_launch : -1;
    return o;
}

}  // namespace

// Streams one persistent launch of this device holds, as nlzm_hip_blocks_begin fits them: three stage CUs (and the helper parsers' where
// "block_parser_helper" is on) and one worker CU a stream, 64 at most -- 64 on an MI355X.  0 without a device.
uint32_t host::blocks_capacity(const DevState &D)
{
    if (!D.ctx.inited) return 0;
    const int64_t roles_live = (int64_t)pipeline2_role_blocks() - (D.opt.block_helper ? 0 : (int64_t)v2::kHelpers);
    const int64_t cap = D.ctx.cu_count / (roles_live + 1);
    return (uint32_t)(cap < 0 ? 0 : cap > 64 ? 64 : cap);
}

// "keep_block_pool" keeps a closed set's one allocation (most of the device's memory for the bench's set) for the next set; anything
// else that then cannot allocate -- a single stream, a feed, find_matches -- takes it back here instead of failing with NOMEM.
bool host::idle_block_pool_dropped()
{
    DevState &D = cur();
    if (!D.jobs.empty() || !D.blocks_pool) return false;
    (void)hipFree(D.blocks_pool);
    D.blocks_pool = nullptr; D.blocks_pool_size = 0;
    return true;
}

void host::blocks_close(DevState &D, bool drop_pool)
{
    // (a round may still be queued or on the device -- an abandoned set, a failed step: every device wait is bounded)
    for (auto &st : D.group_st) (void)hipStreamSynchronize(st);
    for (auto &j : D.jobs) if (j.c.st) (void)hipStreamSynchronize(j.c.st);
    (void)hipGetLastError();
    D.rounds = DevState::Rounds{};
    for (auto &j : D.jobs) { j.d_out = nullptr; if (j.c.inited) block_ctx_destroy(j.c); }
    D.jobs.clear();
    if (D.blocks_pool && (drop_pool || !D.opt.keep_pool)) { (void)hipFree(D.blocks_pool); D.blocks_pool = nullptr; D.blocks_pool_size = 0; }
    for (auto &st : D.group_st) (void)hipStreamDestroy(st);
    for (auto &ev : D.group_ev) for (auto &e : ev) (void)hipEventDestroy(e);
    D.group_st.clear(); D.group_ev.clear();
    if (D.pack_host) (void)hipHostFree(D.pack_host);
    if (D.pack_dev) (void)hipFree(D.pack_dev);
    D.pack_host = D.pack_dev = nullptr;
}

namespace {

// run f(block) for every open block, `conc` at a time, each on a host thread of its own
template <class F>
void for_blocks(DevState &D, uint32_t conc, F f)
{
    const int device = D.ctx.device;
    std::mutex mu;
    uint32_t next_block = 0;
    auto worker = [&]() {
        t_dev = &D;
        (void)hipSetDevice(device);
        for (;;) {
            uint32_t i;
            { std::lock_guard<std::mutex> lk(mu); if (next_block >= D.jobs.size()) return; i = next_block++; }
            f(i, D.jobs[i]);
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < conc; t++) th.emplace_back(worker);
    for (auto &t : th) t.join();
}
}  // namespace

extern "C" {

int nlzm_hip_blocks_begin(const void *d_src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    const Options &O = D.opt;
    uint64_t per_fixed = D.blocks_per;              // (a multi-device call fixes the partition; cleared here)
    D.blocks_per = 0;
    const uint64_t *range_off = D.blocks_off, *range_len = D.blocks_len;       // (nlzm_hip_compress_ranges*: the blocks are the caller's ranges of the n bytes; cleared here)
    D.blocks_off = D.blocks_len = nullptr;
    if (range_len) {        // the set's shared decisions are those of the equal split of nblocks x its longest range
        per_fixed = 0;
        for (uint32_t i = 0; i < nblocks && i < 64; i++) if (range_len[i] > per_fixed) per_fixed = range_len[i];
    }
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!nblocks || nblocks > 64) return fail(NLZM_HIP_E_ARG, "nblocks out of range");
    blocks_close(D);
    // every block is in flight at once: one master CU + its worker CUs per stream, all resident together
    // (a spare CU per stream while there is room for it; every workgroup of the launch has a CU of its own either way:
    //  at most CUs / 4 streams -- three stage CUs and one worker CU each -- which is 64 on an MI355X)
    // (the helper parser's workgroup leaves at once where the streams run without one: it takes no CU then)
    const int64_t roles_live = (int64_t)pipeline2_role_blocks() - (O.block_helper ? 0 : (int64_t)v2::kHelpers);
    int64_t wb = C.cu_count / (int64_t)nblocks - roles_live;
    if (wb > 1 && nblocks > 1) wb--;
    if (wb > O.worker_blocks) wb = O.worker_blocks;
    if (wb < 1) return fail(NLZM_HIP_E_ARG, "%u streams do not fit %d CUs (at most %d)", nblocks, C.cu_count,
                               C.cu_count / (int)(roles_live + 1));
    D.blocks_wb = wb; D.blocks_n = n; D.blocks_src = (const uint8_t *)d_src; D.blocks_hist = hist_bits_req;
    // Every stream holds its own tables and hand-off arrays: the pre-filter table (4 << t_bits bytes) and the per-launch
    // arrays (about 2.2 KB per position of a launch) are sized so that all streams fit the free memory.
    int64_t tbits_max = 32, batch = O.block_batch;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        free_b += D.blocks_pool_size;               // (the allocation kept from the set before is this set's to use)
        const double per_stream = 0.85 * (double)free_b / nblocks;
        Geom g0;
        make_geom(per_fixed || range_len ? per_fixed : container::per_block(n, nblocks), hist_bits_req, g0);
        const double fixed = 8.0 * ((double)g0.wmask + 1) * 2 + 5e7;     // BT4 tree (widened), the rest
        double left = per_stream - fixed;
        if (left < 2e8) return fail(NLZM_HIP_E_NOMEM, "%u streams of %llu bytes at -window:%u do not fit %.1f GB of free memory", nblocks,
                                       (unsigned long long)g0.n, g0.wbits, free_b / 1e9);
        const bool bitmap = prefilter_is_bitmap(g0);
        while (tbits_max > 16 && (double)prefilter_bytes((uint32_t)tbits_max, bitmap) > 0.4 * left) tbits_max--;
        left -= (double)prefilter_bytes(prefilter_tbits(g0, O.tbits_per, tbits_max), bitmap);
        const int64_t fit = (int64_t)(left / launch_bytes_per_chunk(g0));
        if (fit < 1) return fail(NLZM_HIP_E_NOMEM, "%u streams do not fit the device memory", nblocks);
        if (batch > fit) batch = fit;
    }
    const uint64_t per = per_fixed ? per_fixed : container::per_block(n, nblocks);     // block i = [i*per, min(n, (i+1)*per))
    D.jobs.resize(nblocks);
    for (uint32_t i = 0; i < nblocks; i++) {
        if (range_len) { D.jobs[i].lo = range_off[i]; D.jobs[i].n = range_len[i]; }       // (checked against n by the plan: nlzm_container_plan.h)
        else container::block_range(n, per, i, D.jobs[i].lo, D.jobs[i].n);
        D.jobs[i].bound = nlzm_hip_compress_bound(D.jobs[i].n);
    }
    const auto stream_options = [&](uint32_t i) { return block_stream_options(O, wb, batch, tbits_max, i); };
    {   // ONE allocation for the whole block set: what a stream takes is added up first (the same code path, nothing touched on
        // the device), then every stream gets its slice -- some thirty-five hipMalloc calls per stream otherwise
        std::vector<size_t> need(nblocks);
        for (uint32_t i = 0; i < nblocks; i++) {
            Ctx m;                                  // (a scratch context: options as the streams will have them)
            m.inited = true; m.device = C.device; m.cu_count = C.cu_count;
            Pool mp; mp.measuring = true;
            m.pool = &mp;
            const int rc = stream_begin(m, stream_options(i), D.blocks_src + D.jobs[i].lo, D.jobs[i].n, hist_bits_req, (void *)(uintptr_t)16, D.jobs[i].bound);
            if (rc) { blocks_close(D); return rc; }
            need[i] = ((mp.used + 255) & ~(size_t)255) + ((D.jobs[i].bound + 255) & ~(size_t)255) + 4096;
        }
        size_t total = 0;
        for (size_t v : need) total += v;
        if (D.blocks_pool && D.blocks_pool_size < total) { (void)hipFree(D.blocks_pool); D.blocks_pool = nullptr; D.blocks_pool_size = 0; }
        if (!D.blocks_pool) {
            if (hipMalloc(&D.blocks_pool, total) != hipSuccess) { D.blocks_pool = nullptr; blocks_close(D); return fail(NLZM_HIP_E_NOMEM, "block set: %zu bytes for %u streams", total, nblocks); }
            D.blocks_pool_size = total;
        }
        size_t at = 0;
        for (uint32_t i = 0; i < nblocks; i++) {
            D.jobs[i].pool.base = D.blocks_pool + at; D.jobs[i].pool.size = need[i]; D.jobs[i].pool.used = 0; D.jobs[i].pool.measuring = false;
            at += need[i];
        }
    }
    for_blocks(D, nblocks, [&](uint32_t i, BlockJob &j) {
        j.rc = block_ctx_init(j.c, C);
        j.c.pool = &j.pool;
        if (!j.rc) j.rc = dev_alloc(j.c, &j.d_out, j.bound);
        if (!j.rc) j.rc = stream_begin(j.c, stream_options(i), D.blocks_src + j.lo, j.n, hist_bits_req, j.d_out, j.bound);
    });
    for (auto &j : D.jobs) if (j.rc) { const int rc = j.rc; blocks_close(D); return rc; }
    const int rc = [&]() -> int {
        HIPCHK(hipHostMalloc(&D.pack_host, 2 * stream2_pack_size(), hipHostMallocDefault));      // (one per launch set)
        HIPCHK(hipMalloc(&D.pack_dev, 2 * stream2_pack_size()));
        {   // the HIP stream of the shared launches: of higher priority than the streams' own, i.e. on a hardware queue apart
            int lo_p = 0, hi_p = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
            hipStream_t st;
            HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi_p));
            D.group_st.push_back(st);
        }
        for (uint32_t qi = 0; qi < 2; qi++) {
            std::array<hipEvent_t, 3> ev;
            for (auto &e : ev) HIPCHK(hipEventCreate(&e));
            D.group_ev.push_back(ev);
        }
        return 0;
    }();
    if (rc) blocks_close(D);        // (nothing of a block set that failed to open stays allocated)
    return rc;
}

static int blocks_step_impl(DevState &D, uint32_t max_chunks_per_block, uint64_t *in_done_total, int *finished, double *device_ms)
{
    Ctx &C = D.ctx;
    const size_t nj = D.jobs.size();
    hipEvent_t e0 = C.ev[0][kEvCallBegin], e1 = C.ev[0][kEvCallEnd];
    HIPCHK(hipEventRecord(e0, C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    // Rounds: every unfinished stream advances by one launch's worth, and the streams of a round share ONE persistent launch.
    // The rounds overlap: while launch r is on the device (on the 224 CUs its workgroups hold), the pre-pass kernels of round
    // r + 1 run on the CUs that are left, launch r + 1 is queued behind launch r, and the host waits for launch r only to code
    // and gather its frames -- which then runs beside launch r + 1.  (Measured before, 32 streams: 115-140 ms of pre-pass
    // and frame coding between two launches of 580 ms.)  A round's launch is bracketed by round_open_kernel (progress words)
    // and round_close_kernel (what the host checks, copied aside): both on the launch's HIP stream, which has a hardware queue
    // of its own (a stream of higher priority), so that nothing of the other streams queues behind a persistent launch.
    // A call that has collected its share leaves the next round QUEUED (sized like its own rounds) for the next call to collect:
    // the device does not idle between the calls of a caller that steps through the set.
    if (nj > stream2_pack_capacity()) return fail(NLZM_HIP_E_ARG, "too many streams for one launch");
    DevState::Rounds &R = D.rounds;
    hipStream_t gs = D.group_st[0];
    for (auto &p : R.plan) if (p.size() != nj) p.assign(nj, StepPlan{});
    const uint32_t kAll = 0xFFFFFFFFu;
    std::vector<uint32_t> quota(nj, max_chunks_per_block ? max_chunks_per_block : kAll);       // chunks this call still collects, per stream
    auto queue_round = [&](uint32_t q, bool in_call) -> int {      // pre-passes of the round's streams, then its launch
        std::vector<uint32_t> &act = R.act[q];
        act.clear();
        std::vector<uint32_t> todo(nj, 0);
        for (size_t i = 0; i < nj; i++) {
            const Ctx &c = D.jobs[i].c;
            const uint32_t rem = c.g.nchunks - c.pre_chunk;
            const uint32_t want = in_call ? quota[i] : (max_chunks_per_block ? max_chunks_per_block : kAll);
            todo[i] = rem < want ? rem : want;
            if (todo[i]) act.push_back((uint32_t)i);
        }
        if (act.empty()) return 0;
        for (uint32_t i : act) { const int rc = step_pre(D.jobs[i].c, todo[i], R.plan[q][i]); if (rc) return rc; }
        uint8_t *ph = (uint8_t *)D.pack_host + (size_t)q * stream2_pack_size(), *pd = (uint8_t *)D.pack_dev + (size_t)q * stream2_pack_size();
        for (uint32_t k = 0; k < act.size(); k++) {
            Ctx &c = D.jobs[act[k]].c;
            const StepPlan &P = R.plan[q][act[k]];
            HIPCHK(hipStreamWaitEvent(gs, c.ev[P.set][kEvPrepEnd], 0));          // its pre-pass is done
            fill_stream2_args(ph, k, c.g, P.G, P.V, P.c0, P.c1, c.set[P.set].snap);
        }
        HIPCHK(hipMemcpyAsync(pd, ph, stream2_pack_size(), hipMemcpyHostToDevice, gs));
        launch_round_open(pd, (uint32_t)act.size(), gs);
        HIPCHK(hipEventRecord(D.group_ev[q][0], gs));
        launch_pipeline2_multi(pd, (uint32_t)act.size(), (uint32_t)D.blocks_wb, gs);
        HIPCHK(hipEventRecord(D.group_ev[q][1], gs));
        launch_round_close(pd, (uint32_t)act.size(), gs);
        HIPCHK(hipEventRecord(D.group_ev[q][2], gs));
        return 0;
    };
    if (!R.have) {
        const int rc = queue_round(R.q, true);
        if (rc) return rc;
        R.have = !R.act[R.q].empty();
    }
    while (R.have) {
        const uint32_t q = R.q;
        bool more = false;              // does this call collect another round after this one?
        for (uint32_t i : R.act[q]) { const uint32_t nb = R.plan[q][i].nb; if (quota[i] != kAll) quota[i] -= nb < quota[i] ? nb : quota[i]; }
        for (size_t i = 0; i < nj; i++) more |= quota[i] && D.jobs[i].c.pre_chunk < D.jobs[i].c.g.nchunks;
        { const int rc = queue_round(q ^ 1, more); if (rc) return rc; }
        {   // (every stream of the round is looked at, so that the first failure is reported with its own diagnostics)
            int first_rc = 0;
            char first_msg[kErrText] = "";
            std::vector<int> rcs(nj, 0);
            auto note = [&](uint32_t i, int rc) {
                if (rc && !rcs[i]) rcs[i] = rc;
                if (rc && !first_rc) {
                    first_rc = rc;
                    error_prefixed(first_msg, nullptr, "block %u: ", i);
                }
            };
            // (a stream marked `redo` -- a launch of it used its pair-list arena up -- is out of the set's rounds: what is still queued of it runs on
            //  a state that is valid but not the reference's, and nothing of it is looked at; nlzm_hip_blocks_finish makes the stream again)
            for (uint32_t i : R.act[q]) {
                if (D.jobs[i].redo) continue;
                const hipError_t e = hipStreamWaitEvent(D.jobs[i].c.st, D.group_ev[q][2], 0);
                note(i, e == hipSuccess ? step_post_issue(D.jobs[i].c, R.plan[q][i]) : fail(NLZM_HIP_E_NODEVICE, "hipStreamWaitEvent failed: %s", hipGetErrorString(e)));
            }
            for (uint32_t i : R.act[q]) if (!rcs[i] && !D.jobs[i].redo) {
                Ctx &c = D.jobs[i].c;
                const int rc = step_post_check(c, R.plan[q][i]);
                if (rc && c.arena_out) { D.jobs[i].redo = true; c.next_chunk = c.pre_chunk = c.g.nchunks; continue; }
                note(i, rc);
            }
            for (uint32_t i : R.act[q]) if (!rcs[i] && !D.jobs[i].redo) note(i, step_post_done(D.jobs[i].c, R.plan[q][i], 0.0f));
            if (first_rc) { error_replace(first_msg); return first_rc; }
        }
        {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, D.group_ev[q][0], D.group_ev[q][1]));
            for (uint32_t i : R.act[q]) { Ctx &c = D.jobs[i].c; c.tm.match_parse_ms += ms; c.tm.total_ms += ms; }
        }
        R.q = q ^ 1;
        R.have = !R.act[q ^ 1].empty();
        if (!more) break;               // (what is queued now is the next call's first round)
    }
    HIPCHK(hipEventRecord(e1, C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (device_ms) *device_ms = ms;
    uint64_t tot = 0; int all = 1;
    for (size_t i = 0; i < nj; i++) {
        const Ctx &c = D.jobs[i].c;
        const unsigned long long d = (unsigned long long)c.next_chunk * c.g.chunk_size;
        tot += d < c.g.n ? d : c.g.n;
        all &= c.next_chunk >= c.g.nchunks;
    }
    if (in_done_total) *in_done_total = tot;
    if (finished) *finished = all;
    return 0;
}

int nlzm_hip_blocks_step(uint32_t max_chunks_per_block, uint64_t *in_done_total, int *finished, double *device_ms)
{
    DevState &D = cur();
    if (D.jobs.empty()) return fail(NLZM_HIP_E_ARG, "no open block set");
    const int rc = blocks_step_impl(D, max_chunks_per_block, in_done_total, finished, device_ms);
    if (rc) {
        // A failed round ends the block set: blocks_close waits for whatever is still queued (every device wait is bounded), then frees
        // every stream's buffers -- the caller's source buffer is not read after this returns.
        // (Nothing under blocks_close writes the error text: it waits, destroys and frees, and looks at no status.)
        blocks_close(D);
    }
    return rc;
}

int nlzm_hip_blocks_finish(void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (D.jobs.empty()) return fail(NLZM_HIP_E_ARG, "no open block set");
    if (!d_dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    for_blocks(D, (uint32_t)D.jobs.size(), [&](uint32_t, BlockJob &j) { j.rc = stream_finish(j.c, &j.len, false); });
    // A stream whose launch ran out of extension blocks for its BT4 pair lists (a block set reserves 32 pairs per position and an arena for the
    // positions that have more: an input with such positions all over it compresses as a single stream, which reserves all 256, but not here)
    // is made again now, from its first byte, as a single stream with buffers of its own, into its place in the set: the bytes are the same
    // either way (the reference run on the block), only the time differs.
    D.redo_streams = 0;
    Options single = D.opt;                 // (what a single stream of this device state is opened with; the fault a test asks for was the set's)
    single.test_fail_launch = -1;
    for (auto &j : D.jobs) {
        if (!j.redo) continue;
        D.redo_streams++;
        Ctx &c = j.c;
        (void)hipStreamSynchronize(c.st);
        for (auto &st : D.group_st) (void)hipStreamSynchronize(st);
        c.pool = nullptr;
        j.rc = stream_begin(c, single, D.blocks_src + j.lo, j.n, D.blocks_hist, j.d_out, j.bound);
        if (!j.rc) j.rc = stream_step(c, 0, nullptr, nullptr, nullptr);
        if (!j.rc) j.rc = stream_finish(c, &j.len, false);
        if (D.opt.report) fprintf(stderr, "block set: the stream of block %zu was made again as a single stream (its pair-list arena of %u blocks per launch had run out)%s\n",
                                  (size_t)(&j - &D.jobs[0]), c.cfg.ext_cap, j.rc ? ": FAILED" : "");
    }
    if (D.opt.report) {
        // which stage limits a stream under load: smallest / median / largest over the streams, cycles per position
        fprintf(stderr, "block set of %zu streams, %lld worker CUs each -- per stream, cycles per position (min / median / max over the streams):\n", D.jobs.size(), (long long)D.blocks_wb);
        for (int k = 0; k < 8; k++) {
            std::vector<double> v;
            for (auto &j : D.jobs) if (!j.rc) v.push_back(j.c.acct[k]);
            if (v.empty()) continue;
            std::sort(v.begin(), v.end());
            fprintf(stderr, "  %-26s %8.0f %8.0f %8.0f\n", kAcctRows[k].label, v.front(), v[v.size() / 2], v.back());
        }
    }
    int rc = 0;
    uint64_t pos = 0;
    memset(&C.stats, 0, sizeof C.stats);
    for (size_t i = 0; i < D.jobs.size() && !rc; i++) {
        BlockJob &j = D.jobs[i];
        if (j.rc) { rc = j.rc; break; }
        if (pos + j.len > dst_cap) { rc = fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu too small", (unsigned long long)dst_cap); break; }
        if (hipMemcpyAsync((uint8_t *)d_dst + pos, j.d_out, j.len, hipMemcpyDeviceToDevice, C.st) != hipSuccess)
            rc = fail(NLZM_HIP_E_NODEVICE, "gathering block %zu failed", i);
        if (block_len) block_len[i] = j.len;
        pos += j.len;
        add_stats(C.stats, j.c.stats);              // counters of the whole job
    }
    (void)hipStreamSynchronize(C.st);
    blocks_close(D);
    if (!rc) *dst_len = pos;
    return rc;
}

void nlzm_hip_blocks_abandon(void) { blocks_close(cur()); }

// Room that the streams of nblocks blocks of n bytes can take at most.  Up to 64 blocks (one set wherever a device holds them) the margin per
// stream the entry points have always asked for; above that the sum of the blocks' own bounds, which is what a container compressed in sets is
// guaranteed to fit (every set is bounded by its blocks' bounds).  No device needed.  0: nblocks out of range, or a sum beyond 64 bits.
uint64_t nlzm_hip_compress_blocks_bound(uint64_t n, uint32_t nblocks)
{
    if (!nblocks || nblocks > container::kMaxBlocks) return 0;
    if (nblocks <= 64) return nlzm_hip_compress_bound(n) + (uint64_t)nblocks * (16 + 131072);
    container::Plan P;
    if (container::make_plan(P, n, nblocks, 1, 1, nlzm_hip_compress_bound, ErrText{ nullptr, 0 })) return 0;
    return P.out_bound;
}

// one block set from begin to finish: what the one-shot form has always been (the set's partition is the caller's, or D.blocks_per's)
static int compress_block_set(const void *d_src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req, void *d_dst,
                              uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    const auto t0 = std::chrono::steady_clock::now();
    int rc = nlzm_hip_blocks_begin(d_src, n, nblocks, hist_bits_req);
    if (rc) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    double dev_ms = 0;
    rc = nlzm_hip_blocks_step(0, nullptr, nullptr, &dev_ms);
    if (rc) return rc;              // (the failed step has closed the set)
    const auto t2 = std::chrono::steady_clock::now();
    rc = nlzm_hip_blocks_finish(d_dst, dst_cap, block_len, dst_len);
    if (cur().opt.report) {
        const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "block set of %u: begin (tables, pre-filter) %.0f ms, steps %.0f ms (device %.0f ms), finish (gather) %.0f ms\n", nblocks,
                ms(t0, t1), ms(t1, t2), dev_ms, ms(t2, std::chrono::steady_clock::now()));
    }
    return rc;
}

// The sets of a container (nlzm_container_plan.h), one after another through compress_block_set with the partition fixed: set s compresses the
// bytes of its blocks and writes their streams straight behind those of the set before it.  The block set's one allocation stays for the next
// set ("keep_block_pool").  A set that fails has closed itself: the call ends with its error and nothing open.
static int compress_container(DevState &D, const container::Plan &P, const void *d_src, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap,
                              uint64_t *block_len, uint64_t *dst_len)
{
    nlzm_hip_stats total{};
    uint64_t pos = 0, redo = 0;
    // the sets share the one allocation whatever "keep_block_pool" says (46 GB freed and taken again 32 times otherwise): with the option off it
    // goes when the call ends, as it does after any set then, and "block_pool_bytes" reads 0
    const int64_t keep_pool = D.opt.keep_pool;
    D.opt.keep_pool = 1;
    struct Restore { DevState &D; int64_t keep; ~Restore() { D.opt.keep_pool = keep; if (!keep && D.jobs.empty()) blocks_close(D, true); } } restore{ D, keep_pool };
    for (const container::Set &S : P.sets) {
        uint64_t len = 0;
        D.blocks_per = P.per;                       // (read and cleared by nlzm_hip_blocks_begin; a set wholly behind the input's end: empty streams)
        const int rc = compress_block_set((const uint8_t *)d_src + S.off, S.len, S.count, hist_bits_req, (uint8_t *)d_dst + pos, dst_cap - pos,
                                          block_len ? block_len + S.first : nullptr, &len);
        D.blocks_per = 0;
        if (rc) return rc;
        pos += len;
        redo += D.redo_streams;
        D.container_sets++;
        add_stats(total, D.ctx.stats);              // counters of the whole container
    }
    D.ctx.stats = total;
    D.redo_streams = redo;
    *dst_len = pos;
    return 0;
}

int nlzm_hip_compress_blocks_dev(const void *d_src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req, void *d_dst,
                                 uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    const uint32_t cap = blocks_capacity(D);
    D.container_sets = 0;
    // one set: no device yet (the set's own error), a partition the caller has fixed (a multi-device call: its limit per device stays), or blocks that fit one launch
    if (!cap || D.blocks_per || nblocks <= cap) {
        const int rc = compress_block_set(d_src, n, nblocks, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
        if (!rc) D.container_sets = 1;
        return rc;
    }
    if (!d_dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    container::Plan P;
    char text[256] = "";
    const uint32_t set_blocks = (uint32_t)(D.opt.container_set_blocks < (int64_t)cap ? D.opt.container_set_blocks : (int64_t)cap);
    if (const int rc = container::make_plan(P, n, nblocks, set_blocks, cap, nlzm_hip_compress_bound, ErrText{ text, sizeof text })) return fail(rc, "%s", text);
    return compress_container(D, P, d_src, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
}

// The sets of a call on ranges (nlzm_container_plan.h, make_ranges_plan), one after another through compress_block_set with the set's ranges as its
// blocks: every set reads the caller's whole buffer and writes its streams straight behind those of the set before it.  The one allocation is shared
// as compress_container shares it; a set that fails has closed itself.
static int compress_range_sets(DevState &D, const container::RangesPlan &P, const void *d_src, uint64_t n, const uint64_t *off, const uint64_t *len,
                               uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    nlzm_hip_stats total{};
    uint64_t pos = 0, redo = 0;
    const int64_t keep_pool = D.opt.keep_pool;
    if (P.sets.size() > 1) D.opt.keep_pool = 1;
    struct Restore { DevState &D; int64_t keep; ~Restore() { D.opt.keep_pool = keep; if (!keep && D.jobs.empty()) blocks_close(D, true); } } restore{ D, keep_pool };
    for (const container::RangeSet &S : P.sets) {
        uint64_t out = 0;
        D.blocks_off = off + S.first; D.blocks_len = len + S.first;     // (read and cleared by nlzm_hip_blocks_begin)
        const int rc = compress_block_set(d_src, n, S.count, hist_bits_req, (uint8_t *)d_dst + pos, dst_cap - pos, block_len ? block_len + S.first : nullptr, &out);
        D.blocks_off = D.blocks_len = nullptr;
        if (rc) return rc;
        pos += out;
        redo += D.redo_streams;
        D.container_sets++;
        add_stats(total, D.ctx.stats);
    }
    D.ctx.stats = total;
    D.redo_streams = redo;
    *dst_len = pos;
    return 0;
}

uint64_t nlzm_hip_compress_ranges_bound(uint32_t k, const uint64_t *len)
{
    uint64_t sum = 0;
    return container::ranges_bound(k, len, nlzm_hip_compress_bound, sum) ? sum : 0;
}

// what both forms check before anything is allocated: the plan of the call (with the device's capacity where there is a device, else with one
// that only serves the checks), so that a bad argument is NLZM_HIP_E_ARG with or without a device
static int ranges_plan(DevState &D, container::RangesPlan &P, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len)
{
    const uint32_t cap = blocks_capacity(D);
    const uint32_t set_blocks = cap ? (uint32_t)(D.opt.container_set_blocks < (int64_t)cap ? D.opt.container_set_blocks : (int64_t)cap) : 1;
    char text[512] = "";
    if (const int rc = container::make_ranges_plan(P, n, k, off, len, set_blocks, cap ? cap : 1, nlzm_hip_compress_bound, ErrText{ text, sizeof text })) return fail(rc, "%s", text);
    return 0;
}

// Option "dedup_ranges": the ranges whose bytes an earlier range of the call holds are not compressed again (stream i is a function of range i's bytes and
// hist_bits_req alone: equal bytes, equal streams).  first_of from the device (nlzm_hip_dedup.cpp); the distinct ranges, in order of first occurrence,
// through the same plan and sets into a scratch allocation sized by their bound; ONE gather launch puts stream first_of[i] at stream i's place.
// *done = 0: every range is distinct, and the caller runs what it runs without the option.
static int compress_ranges_dedup(DevState &D, const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t hist_bits_req, void *d_dst,
                                 uint64_t *block_len, uint64_t *dst_len, bool *done)
{
    *done = false;
    std::vector<uint32_t> first_of(k), slot(k, 0);
    if (const int rc = dedup_first_of(d_src, n, k, off, len, first_of.data())) return rc;
    std::vector<uint64_t> doff, dlen;
    for (uint32_t i = 0; i < k; i++) if (first_of[i] == i) { slot[i] = (uint32_t)doff.size(); doff.push_back(off[i]); dlen.push_back(len[i]); }
    const uint32_t kd = (uint32_t)doff.size();
    if (kd == k) return 0;
    container::RangesPlan P;
    if (const int rc = ranges_plan(D, P, n, kd, doff.data(), dlen.data())) return rc;
    DevBuf scratch;
    if (hipMalloc(&scratch.p, P.out_bound) != hipSuccess) {
        (void)hipGetLastError(); scratch.p = nullptr;
        return fail(NLZM_HIP_E_NOMEM, "no %llu bytes of device memory for the streams of the %u distinct ranges", (unsigned long long)P.out_bound, kd);
    }
    std::vector<uint64_t> dblen(kd), dpos(kd), from(k), to(k), blen(k);
    uint64_t got = 0, pos = 0;
    if (const int rc = compress_range_sets(D, P, d_src, n, doff.data(), dlen.data(), hist_bits_req, scratch.p, P.out_bound, dblen.data(), &got)) return rc;
    for (uint32_t j = 0; j < kd; j++) { dpos[j] = pos; pos += dblen[j]; }
    pos = 0;
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t j = slot[first_of[i]];
        from[i] = dpos[j]; to[i] = pos; blen[i] = dblen[j];
        pos += blen[i];
    }
    if (const int rc = dedup_place(scratch.as<uint8_t>(), (uint8_t *)d_dst, k, from.data(), to.data(), blen.data())) return rc;
    if (block_len) memcpy(block_len, blen.data(), (size_t)k * sizeof(uint64_t));
    *dst_len = pos;
    *done = true;
    return 0;
}

int nlzm_hip_compress_ranges_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t hist_bits_req, void *d_dst,
                                 uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    D.container_sets = 0;
    if (!d_dst || !dst_len || (!d_src && n)) return fail(NLZM_HIP_E_ARG, "null argument");
    container::RangesPlan P;
    if (const int rc = ranges_plan(D, P, n, k, off, len)) return rc;
    if (!D.ctx.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (dst_cap < P.out_bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)P.out_bound);
    if (dedup_ranges_option()) {
        bool done = false;
        const int rc = compress_ranges_dedup(D, d_src, n, k, off, len, hist_bits_req, d_dst, block_len, dst_len, &done);
        if (rc || done) return rc;
    }
    return compress_range_sets(D, P, d_src, n, off, len, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
}

int nlzm_hip_compress_ranges(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t hist_bits_req, uint8_t *dst,
                             uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    if ((!src && n) || !dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    container::RangesPlan P;
    if (const int rc = ranges_plan(D, P, n, k, off, len)) return rc;
    if (!D.ctx.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (dst_cap < P.out_bound) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu, the ranges' streams may take %llu (nlzm_hip_compress_ranges_bound)", (unsigned long long)dst_cap, (unsigned long long)P.out_bound);
    DevBuf in, out;                                 // (neither size is 0: 512 bytes behind the input, a bound of a stream's margin at least)
    if (const int rc = in.alloc(n + 512)) return rc;
    if (hipMalloc(&out.p, P.out_bound) != hipSuccess) return fail(NLZM_HIP_E_NOMEM, "output buffer");
    uint8_t *d_in = in.as<uint8_t>(), *d_out = out.as<uint8_t>();
    if (hipMemset(d_in + n, 0, 512) != hipSuccess || (n && hipMemcpy(d_in, src, n, hipMemcpyHostToDevice) != hipSuccess))
        return fail(NLZM_HIP_E_NODEVICE, "copying the input to the device failed");
    uint64_t got = 0;
    int rc = nlzm_hip_compress_ranges_dev(d_in, n, k, off, len, hist_bits_req, d_out, P.out_bound, block_len, &got);
    if (!rc && got && hipMemcpy(dst, d_out, got, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(NLZM_HIP_E_NODEVICE, "copy back failed");
    if (!rc) *dst_len = got;
    return rc;
}

int nlzm_hip_compress_blocks(const uint8_t *src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req, uint8_t *dst,
                             uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if ((!src && n) || !dst || !dst_len || !nblocks) return fail(NLZM_HIP_E_ARG, "null argument");
    if (nblocks > container::kMaxBlocks) return fail(NLZM_HIP_E_ARG, "nblocks out of range (1 .. %u)", container::kMaxBlocks);
    DevBuf in, out;                                 // (neither size is 0: 512 bytes behind the input, a bound of a margin per stream at least)
    const uint64_t bound = nlzm_hip_compress_blocks_bound(n, nblocks);
    if (const int rc = in.alloc(n + 512)) return rc;
    if (hipMalloc(&out.p, bound) != hipSuccess) return fail(NLZM_HIP_E_NOMEM, "output buffer");
    uint8_t *d_in = in.as<uint8_t>(), *d_out = out.as<uint8_t>();
    if (hipMemset(d_in + n, 0, 512) != hipSuccess || (n && hipMemcpy(d_in, src, n, hipMemcpyHostToDevice) != hipSuccess))
        return fail(NLZM_HIP_E_NODEVICE, "copying the input to the device failed");
    uint64_t len = 0;
    int rc = nlzm_hip_compress_blocks_dev(d_in, n, nblocks, hist_bits_req, d_out, bound, block_len, &len);
    if (!rc && len > dst_cap) rc = fail(NLZM_HIP_E_CAPACITY, "streams are %llu bytes, dst_cap %llu", (unsigned long long)len, (unsigned long long)dst_cap);
    if (!rc && hipMemcpy(dst, d_out, len, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(NLZM_HIP_E_NODEVICE, "copy back failed");
    if (!rc) *dst_len = len;
    return rc;
}

}  // extern "C"
