// nlzm_hip.cpp -- host pipeline behind the C ABI of include/nlzm_hip.h.
//
// Replaces encode_file (NLZM.cpp:1711-1910): the whole input lives in HBM as one
// flat buffer; chunks (= frames, NLZM.cpp:1724) are processed in batches by the
// persistent match-find/parse/emit launch, then every frame of the batch is
// rANS-coded in parallel and gathered into the output stream.
// There is no CPU implementation of any stage in this library.
#include <hip/hip_runtime.h>
#include <dirent.h>
#include <unistd.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "nlzm_host_state.h"
#include "nlzm_cut_host.h"
#include "nlzm_dedup_host.h"
#include "nlzm_planes_host.h"
#include "nlzm_elem_host.h"
#include "nlzm_report.h"
#include "nlzm_stream_plan.h"

#include "nlzm_launch.h"

using namespace nlzm;
using namespace nlzm::host;

namespace {

char g_err[kErrText] = "";
std::mutex g_err_mu;            // block streams run on host threads
// the error text of the device state this thread works for (a multi-device call: one per device)
char *thread_err() { return t_dev ? t_dev->err : nullptr; }

int g_hwq_effective = 0;                           // what the HIP runtime reads as GPU_MAX_HW_QUEUES (dev_init)

inline uint32_t clampu(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

namespace nlzm {
// what fail() and HIPCHK end in, in every host file of the library
int host_error(int code, const char *text)
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    snprintf(g_err, sizeof g_err, "%s", text);
    if (char *te = thread_err()) memcpy(te, g_err, sizeof g_err);
    return code;
}
namespace host {

void error_prefixed(char (&out)[kErrText], const char *text, const char *prefix_fmt, ...)
{
    char prefix[32];
    va_list ap;
    va_start(ap, prefix_fmt);
    vsnprintf(prefix, sizeof prefix, prefix_fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_err_mu);
    snprintf(out, sizeof out, "%s%.*s", prefix, (int)sizeof out - 32, text ? text : g_err);
}
void error_replace(const char (&text)[kErrText])
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    memcpy(g_err, text, sizeof g_err);
}

DevState g_dev0;
thread_local DevState *t_dev = nullptr;

void free_stream_buffers(Ctx &C)
{
    for (void *p : C.owned) (void)hipFree(p);
    C.owned.clear();
    C.buf = StreamBuffers{}; C.set[0] = C.set[1] = LaunchSet{}; C.set_idx = 0;
    C.open = false;
}
void release_launch_stream(Ctx &C)
{
    for (auto &set : C.launch_ev) for (auto &ev : set) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (C.launch_st) { (void)hipStreamDestroy(C.launch_st); C.launch_st = nullptr; }
    if (C.launch_pack) { (void)hipHostFree(C.launch_pack); C.launch_pack = nullptr; }
}
namespace {
// the bytes of one stream's entry of a pack (nlzm_launch.h)
size_t pack_entry_bytes() { return (size_t)(stream2_pack_size() / stream2_pack_capacity()); }
// what a single stream's persistent launches are queued on and bracketed with (Ctx::launch_st): made once per context, by the first stream that is opened on it
int make_launch_stream(Ctx &C)
{
    if (C.launch_st) return 0;
    int lo_p = 0, hi_p = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
    HIPCHK(hipStreamCreateWithPriority(&C.launch_st, hipStreamNonBlocking, hi_p));
    for (auto &set : C.launch_ev) for (auto &ev : set) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipHostMalloc(&C.launch_pack, 2 * pack_entry_bytes(), hipHostMallocDefault));      // (one entry per launch set)
    return 0;
}
}  // namespace
void release_own_io(Ctx &C)
{
    if (C.own_in) { (void)hipFree(C.own_in); C.own_in = nullptr; }
    if (C.own_dst) { (void)hipFree(C.own_dst); C.own_dst = nullptr; }
}
// device copies for a host-buffer call: n input bytes and the 512 zero bytes the kernels may read behind them, `bound` bytes of output
int alloc_own_io(Ctx &C, uint64_t n, uint64_t bound)
{
    release_own_io(C);
    HIPCHK(hipMalloc(&C.own_in, n + 512));
    HIPCHK(hipMalloc(&C.own_dst, bound));
    HIPCHK(hipMemsetAsync(C.own_in + n, 0, 512, C.st));
    return 0;
}

void make_geom(uint64_t n, uint32_t hist_bits_req, Geom &g)
{
    uint32_t hb = hist_bits_req;
    while (hb > 10 && n < (1ull << (hb - 1))) --hb;                 // NLZM.cpp:1716-1718
    g.n = n;
    g.wbits = hb; g.wmask = (1u << hb) - 1;
    g.frame_bits = clampu(hb - 2, 14, 17);                          // :1722
    g.frame_size = 1u << g.frame_bits;
    g.chunk_size = ((g.frame_size * 15) / 16) - 0x200;              // :1724
    g.feed = g.chunk_size + kMatchMax + 1;                          // :1725
    g.ht3_shift = 32 - (12 + clampu(hb, 15, 17) - 15);              // :1751
    g.bt_shift = 32 - (13 + clampu(hb, 16, 20) - 16);               // :1752
    g.rk_shift = 32 - (15 + clampu(hb, 16, 22) - 16);               // :1753
    g.tag_mask = (uint32_t)((1ull << (32 - hb)) - 1);
    g.nchunks = (uint32_t)((n + g.chunk_size - 1) / g.chunk_size);
    g.bt_tmask = g.wmask;       // widened by stream_begin once the launch size is known
}

// log2 of the pre-filter table's slots.  32 slots per window position: a slot taken by another 65-gram of the window is a false mark.  Up to 2^33
// slots -- 32 GiB for the 1e9-byte stream at -window:28, which had the 32-bit hash's 2^32 until round 5: 6 % false marks at depth instead of 3 %.
// ... and by the input: 2^tbits_per entries per position (default 16; the 1e9-byte stream at -window:28 has four, the cap): a denser table marks
// more positions as undecided -- 300 MB with four instead of eight entries per position waited twice as long for BT4 results; every entry is
// cleared when a stream begins, which is what opening a set of 32 blocks spent most of its time on.  A smaller table: only more `unc` marks.
uint32_t prefilter_tbits(const Geom &g, int64_t tbits_per, int64_t tbits_max)
{
    uint32_t tb = clampu(g.wbits + 5, 16, 33);
    uint32_t lgn = 1; while ((1ull << lgn) < g.n) lgn++;
    const uint32_t want = lgn + (uint32_t)tbits_per;
    if (want < tb) tb = want < 16 ? 16 : want;
    if ((int64_t)tb > tbits_max) tb = (uint32_t)(tbits_max < 16 ? 16 : tbits_max);
    return tb;
}
// A stream that is no longer than its window -- every stream of a block set, whose window the reference shrinks to the block, :1716-1718 -- never
// meets an earlier position outside the window: one bit per slot says all a 32-bit position would; 2 GB -> 64 MB per stream of the bench's set.
bool prefilter_is_bitmap(const Geom &g) { return g.n <= (unsigned long long)g.wmask + 1; }
size_t prefilter_bytes(uint32_t t_bits, bool bitmap)
{
    return bitmap ? (((size_t)1 << t_bits) / 8 < 4 ? (size_t)4 : ((size_t)1 << t_bits) / 8) : (size_t)4 << t_bits;
}
// what the per-launch arrays take per chunk of a launch: about 2.3 KB per position
double launch_bytes_per_chunk(const Geom &g) { return 2300.0 * g.chunk_size + 8.0 * g.chunk_size * 4; }

namespace {
int alloc_launch_set(Ctx &C, LaunchSet &S)
{
    const StreamConfig &K = C.cfg;
    const unsigned long long bpos = (unsigned long long)K.batch * C.g.chunk_size;
    DEVALLOC(S.rkhash, K.rkhash_len * 4 + 16);
    DEVALLOC(S.syms, K.batch * K.syms_stride * 4);
    DEVALLOC(S.bits, K.batch * K.bits_stride);
    DEVALLOC(S.fmeta, K.batch * sizeof(FrameMeta));
    DEVALLOC(S.unc, bpos + 16);
    // hand-off arrays between workgroups (written with sc1 stores, read with sc1 loads: plain device memory)
    DEVALLOC(S.bt_ready, bpos * 4 * kBtRec);
    DEVALLOC(S.bt_flag, bpos * 4);
    DEVALLOC(S.abort_word, 4);
    DEVALLOC(S.bin_off, (size_t)K.batch * (K.nheads + 1) * 4);
    DEVALLOC(S.bin_pos, bpos * 8);
    if (K.hot_max) {
        DEVALLOC(S.hot_of_bin, (size_t)K.nheads * 4);
        DEVALLOC(S.hot_list, ((size_t)K.hot_max + 1) * 4);
    }
    DEVALLOC(S.snap, sizeof(v2::RoundSnap));
    return 0;
}
}  // namespace

// O: the options the stream is opened with (a stream of a block set: block_stream_options)
int stream_begin(Ctx &C, const Options &O, const void *d_src, uint64_t n, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap)
{
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (n >= 0xFFFF0000ull) return fail(NLZM_HIP_E_TOOBIG, "input of %llu bytes needs >32-bit positions", (unsigned long long)n);
    if (hist_bits_req < 10 || hist_bits_req > 28) return fail(NLZM_HIP_E_ARG, "hist_bits %u outside [10,28]", hist_bits_req);
    if (dst_cap < 8) return fail(NLZM_HIP_E_CAPACITY, "dst_cap < 8");
    free_stream_buffers(C);
    make_geom(n, hist_bits_req, C.g);
    const Geom &g = C.g;
    C.d_in = (const uint8_t *)d_src; C.d_dst = (uint8_t *)d_dst; C.dst_cap = dst_cap;
    C.out_pos = 0; C.next_chunk = 0; C.pre_chunk = 0; C.last_launch_ms = 0;
    memset(&C.stats, 0, sizeof C.stats);
    memset(&C.tm, 0, sizeof C.tm);
    C.stats.in_bytes = n;
    StreamConfig &K = C.cfg;
    StreamBuffers &B = C.buf;
    K = StreamConfig{};
    K.in_set = C.pool != nullptr;
    K.batch = (uint32_t)(O.batch < 1 ? 1 : O.batch);
    if (g.nchunks && K.batch > g.nchunks) K.batch = g.nchunks;
    {   // The persistent launch needs every block resident at once (the stages and the worker lanes wait on each other):
        // 512-thread blocks with > 80 KB of LDS, one per CU.  Fewer CUs than blocks (a partitioned or masked device)
        // would spin until the timeouts fire, so the worker blocks are clamped to what the device holds.
        const int64_t room = (int64_t)C.cu_count - (int64_t)pipeline2_role_blocks();
        if (room < 1) return fail(NLZM_HIP_E_ARG, "device has %d CUs: the pipeline needs at least %u", C.cu_count, pipeline2_role_blocks() + 1);
        K.worker_blocks = (uint32_t)(O.worker_blocks > room ? room : (O.worker_blocks < 1 ? 1 : O.worker_blocks));
    }
    K.worker_threads = (uint32_t)O.worker_threads;
    {   // one bin per worker lane (or per head when there are fewer heads than lanes)
        K.nheads = 1u << (32 - g.bt_shift);
        const unsigned long long lanes = (unsigned long long)K.worker_blocks * K.worker_threads;
        if (lanes < K.nheads) K.nheads = (uint32_t)lanes;
    }
    {   // hot bins: the waves of a worker block behind its bin-taking lanes
        int64_t hw = O.hot_waves;
        const int64_t spare = (512 - O.worker_threads) / 64;
        if (hw > spare) hw = spare;
        K.hot_max = hw > 0 ? (uint32_t)hw * K.worker_blocks : 0u;
    }
    K.hot_min = (uint32_t)O.hot_min; K.table_shape = (uint32_t)O.table_shape; K.test_fail_launch = O.test_fail_launch; K.helper = O.helper != 0;
    K.t_bits = prefilter_tbits(g, O.tbits_per, O.tbits_max);
    K.t_bitmap = prefilter_is_bitmap(g) ? 1u : 0u;
    // a position's pairs beyond the four in its record: the worst case (256 pairs, 2 KiB per position) reserved for a single stream; the
    // streams of a block set reserve 32 pairs (256 bytes) and take extension blocks from an arena for the positions that have more
    // (nlzm_core.h, bt_pair_ptr; a launch that uses the arena up fails with an error, it never drops a pair)
    K.pstride = K.in_set ? 32u : kBtMaxPairs;
    K.syms_stride = 3ull * g.chunk_size + 4096;          // <= 3 symbols per input byte
    K.bits_stride = 2ull * g.chunk_size + 64;            // <= 13 raw bits per input byte
    K.frame_stride = 12 + K.bits_stride + 16 + 2 * K.syms_stride;

    const size_t ht3_bytes = (size_t)8 << (32 - g.ht3_shift), rk_bytes = (size_t)4 << (32 - g.rk_shift), heads_bytes = (size_t)4 << (32 - g.bt_shift);
    {
        // node slots >= W + positions per launch (see Geom::bt_tmask)
        const unsigned long long need = (1ull << g.wbits) + (unsigned long long)K.batch * g.chunk_size;
        unsigned long long slots = 1ull << g.wbits;
        while (slots < need) slots <<= 1;
        C.g.bt_tmask = (uint32_t)(slots - 1);
    }
    const size_t tree_bytes = ((size_t)g.bt_tmask + 1) * 8;
    DEVALLOC(B.ht2, 4096 * 4);
    DEVALLOC(B.ht3, ht3_bytes);
    DEVALLOC(B.rk_table, rk_bytes);
    DEVALLOC(B.bt_heads, heads_bytes);
    DEVALLOC(B.bt_tree, tree_bytes);
    DEVALLOC(B.persist, sizeof(Persist));
    DEVFILL(hipMemsetAsync(B.ht2, 0xFF, 4096 * 4, C.st));                         // :902
    DEVFILL(hipMemsetAsync(B.ht3, 0xFF, ht3_bytes, C.st));
    DEVFILL(hipMemsetAsync(B.rk_table, 0xFF, rk_bytes, C.st));                    // :1040
    DEVFILL(hipMemsetAsync(B.bt_heads, 0xFF, heads_bytes, C.st));                 // :968
    DEVFILL(hipMemsetAsync(B.bt_tree, 0xFF, tree_bytes, C.st));                   // :969

    Persist P;
    memset(&P, 0, sizeof P);
    for (uint32_t ctx = 0; ctx < kNumCtx; ctx++) {                                // model_init :1183-1206, cdf_init :324-346
        const uint32_t ns = (ctx == kCtxCmd) ? 4 : ((ctx == kCtxLenDirect || ctx >= kCtxSlotHi) ? 8 : 16);
        for (uint32_t i = 0; i <= ns; i++) P.cdf[ctx * kCdfStride + i] = (uint16_t)(i * (16384 / ns));
    }
    for (int i = 0; i < 4; i++) P.rep[i] = (uint32_t)i + 1;                       // :1154-1158
    DEVFILL(hipMemcpyAsync(B.persist, &P, sizeof P, hipMemcpyHostToDevice, C.st));

    K.depth = 2;
    if (!K.in_set) {    // the per-launch arrays take about 2.3 KB per position of a launch: a launch that does not fit is cut down, and the stream
        // has a second launch set where that fits as well (nlzm_stream_plan.h)
        // (not for the streams of a block set: blocks_begin fitted their batch to the memory, and the free memory differs between the pass that
        //  measures what a stream takes and the pass that takes it -- the pool itself is allocated in between)
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        const stream_plan::Plan plan = stream_plan::make_plan((double)free_b, 4.0 * (double)(1ull << K.t_bits) /* the pre-filter table: up to 2^33 entries */,
                                                              launch_bytes_per_chunk(g), K.batch, g.nchunks);
        K.batch = plan.batch; K.depth = plan.depth;
        const int rc = make_launch_stream(C);
        if (rc) return rc;
    }
    // (RK256 hashes of ONE launch's positions -- the array is indexed by absolute position through a base pointer moved back by
    //  the launch's first hashed position, so only a launch's worth is ever resident: 4 B x (launch + lookahead) instead of 4 B
    //  per input byte, which was 4 GB at 1e9 bytes)
    const unsigned long long bpos = (unsigned long long)K.batch * g.chunk_size;
    K.rkhash_len = bpos + g.feed + 256 + 1024 + 2048;
    if (K.rkhash_len > n + 2048) K.rkhash_len = n + 2048;
    { uint32_t lg = 1; while ((1ull << lg) < bpos) lg++; K.m_bits = lg + 6 > 28 ? 28 : lg + 6; }
    K.ext_cap = K.pstride < kBtMaxPairs ? (uint32_t)(bpos / 64 + 1024) : 0u;
    if (K.ext_cap && O.block_ext_blocks >= 0) K.ext_cap = (uint32_t)(O.block_ext_blocks < 1 ? 1 : O.block_ext_blocks);

    DEVALLOC(B.scratch, K.batch * K.syms_stride * 4);
    DEVALLOC(B.frames, K.batch * K.frame_stride);
    DEVALLOC(B.dst_off, K.batch * sizeof(unsigned long long));
    for (uint32_t s = 0; s < K.depth; s++) { const int rc = alloc_launch_set(C, C.set[s]); if (rc) return rc; }

    // pre-filter tables, per-launch hand-off arrays, bins
    for (;;) {      // (a device with less free memory than the table wants: a smaller table only marks more positions as undecided)
        const int rc_t = dev_alloc(C, &B.pf_T, prefilter_bytes(K.t_bits, K.t_bitmap != 0));
        if (!rc_t) break;
        if (K.in_set || rc_t != NLZM_HIP_E_NOMEM || K.t_bits <= 28) return rc_t;
        (void)hipGetLastError();
        K.t_bits--;
    }
    DEVALLOC(B.pf_M, (size_t)4 << K.m_bits);
    DEVFILL(hipMemsetAsync(B.pf_T, 0, prefilter_bytes(K.t_bits, K.t_bitmap != 0), C.st));
    DEVFILL(hipMemsetAsync(B.pf_M, 0xFF, (size_t)4 << K.m_bits, C.st));
    DEVALLOC(B.pf_h, bpos * 4);
    DEVALLOC(B.pf_h2, bpos * 4);
    DEVALLOC(B.pf_c1, bpos);
    DEVALLOC(B.bt_pairs, bpos * (2ull * K.pstride * 4));
    if (K.ext_cap) DEVALLOC(B.bt_ext, (size_t)K.ext_cap * (2ull * (kBtMaxPairs - K.pstride) * 4));
    DEVALLOC(B.bin_cur, (size_t)K.batch * K.nheads * 4);
    DEVALLOC(B.wcnt, sizeof(WorkerCounters));
    DEVFILL(hipMemsetAsync(B.wcnt, 0, sizeof(WorkerCounters), C.st));
    DEVALLOC(B.bt_undo, (size_t)K.nheads * worker_undo_bytes_per_lane());     // (6 KB per lane)
    if (K.hot_max) DEVALLOC(B.hot_undo, (size_t)K.hot_max * worker_hot_undo_bytes_per_wave());

    // hand-off between the finder, table and parser stages
    DEVALLOC(B.v2_ft, (size_t)v2::kFtRing * v2::kFtStride * 4);
    DEVALLOC(B.v2_tp, (size_t)v2::kTpRing * v2::kTpStride * 4);
    DEVALLOC(B.v2_tf, (size_t)v2::kTpRing * v2::kTfStride * 4);
    DEVALLOC(B.v2_state, sizeof(v2::StateV2));
    DEVALLOC(B.v2_hx, sizeof(v2::Hx));
    if (K.helper) DEVALLOC(B.v2_hb, v2::kHelpers * sizeof(v2::HelpBox));
    DEVFILL(hipMemsetAsync(B.v2_state, 0, sizeof(v2::StateV2), C.st));
    C.v2_launch_no = 0;

    // stream header (:1762-1766)
    const uint8_t hdr[4] = { (uint8_t)(g.wbits >> 8), (uint8_t)g.wbits, (uint8_t)(g.frame_bits >> 8), (uint8_t)g.frame_bits };
    DEVFILL(hipMemcpyAsync(C.d_dst, hdr, 4, hipMemcpyHostToDevice, C.st));
    C.out_pos = 4;

    if (C.pool && C.pool->measuring) return 0;
    HIPCHK(hipStreamSynchronize(C.st));
    C.open = true;
    return 0;
}

// The hot bins of a launch whose bins are made (step_pre).  From how many positions a bin counts as hot: a single stream's threshold follows the
// pace of the launch before it (Options::hot_min), so this is queued when that launch has ended, in front of the launch itself.
static void select_hot_bins(Ctx &C, const StepPlan &P, hipStream_t st)
{
    const StreamConfig &K = C.cfg;
    const LaunchSet &L = C.set[P.set];
    const unsigned long long lpos = (unsigned long long)K.batch * C.g.chunk_size;
    // (the streams of a block set have a hundred heads to a lane: there a wave pays from positions / 480 on -- 112.6 -> 115.6 MB/s against 8,192)
    const double by_pace = K.in_set ? (double)lpos / 480.0 : (C.last_launch_ms > 0 ? 24.0 * C.last_launch_ms : (double)lpos / 240.0);
    const uint32_t hot_min = K.hot_min > 0 ? K.hot_min : (uint32_t)(by_pace < 512 ? 512 : (by_pace > 1e9 ? 1e9 : by_pace));
    launch_hot_select(L.bin_off, P.nb, K.nheads, K.hot_max, hot_min, L.hot_of_bin, L.hot_list, C.buf.wcnt, st);
}

// One launch's worth of a stream, in three parts so that several streams can share ONE persistent launch:
//   step_pre   pre-pass kernels and the hand-off arrays of chunks [c0, c1) on the stream's own HIP stream
//   (launch)   pipeline_kernel for this stream alone, or pipeline_multi_kernel for a group of streams
//   step_post  frame coder, frame lengths back to the host, checks, gather into the output
// The launch before this one may still be on the device: with two launch sets the other one is made the current one, and the progress
// words are set by round_open_kernel on the launch's own HIP stream, not by a copy from here.
int step_pre(Ctx &C, uint32_t todo, StepPlan &P)
{
    const Geom &g = C.g;
    const StreamConfig &K = C.cfg;
    const StreamBuffers &B = C.buf;
    if (K.depth > 1) C.set_idx ^= 1;
    const LaunchSet &L = C.set[C.set_idx];
    const uint32_t c0 = C.pre_chunk, nb = todo < K.batch ? todo : K.batch, c1 = c0 + nb;
    C.pre_chunk = c1;
    P.c0 = c0; P.c1 = c1; P.nb = nb;
    P.set = C.set_idx;
    hipEvent_t *ev = C.ev[P.set];
    Globals &G = P.G;
    memset(&G, 0, sizeof G);
    G.in = C.d_in; G.rkhash = nullptr; G.ht2 = B.ht2; G.ht3 = B.ht3; G.rk_table = B.rk_table;
    G.bt_heads = B.bt_heads; G.bt_tree = B.bt_tree; G.persist = B.persist;
    G.syms = L.syms; G.syms_stride = K.syms_stride; G.bits = L.bits; G.bits_stride = K.bits_stride;
    G.fmeta = L.fmeta; G.chunk0 = c0;
    G.cap_words = C.stage.cap_words; G.cap_cap = C.stage.cap_cap; G.cap_lo = C.stage.cap_lo; G.cap_hi = C.stage.cap_hi; G.cap_used = C.stage.cap_used;
    G.workers = 1;                      // BT4 always runs on the worker lanes
    const unsigned long long a0 = (unsigned long long)c0 * g.chunk_size;
    unsigned long long a1 = (unsigned long long)c1 * g.chunk_size;
    if (a1 > g.n) a1 = g.n;
    G.batch_a0 = (uint32_t)a0;
    {   // pre-pass: RK256 hash of every window the launch can touch (catch-up inserts reach back < 512 bytes).
        // Feed mode: the hashes of windows beyond the launch's last position (up to a1 + feed + 511) may be computed from bytes
        // whose upload is still in flight (feed_chunks_ready guarantees a1 + (feed - chunk) + 1024 only).  They are never used:
        // the finder reads rkhash[p] for p < a1 only, and the next launch hashes again from its own a0 - 1024 on.
        const unsigned long long lo = a0 > 1024 ? a0 - 1024 : 0;
        unsigned long long hi = a1 + g.feed + 256;
        if (hi + 255 > g.n) hi = g.n >= 255 ? g.n - 255 : 0;
        HIPCHK(hipEventRecord(ev[kEvRkBegin], C.st));
        if (hi > lo && hi - lo > K.rkhash_len) return fail(NLZM_HIP_E_ARG, "launch of %u chunks is larger than the stream was opened for", nb);
        G.rkhash = L.rkhash - lo;                       // rkhash[a] for a in [lo, hi): the launch's own array
        if (g.n >= 256 && hi > lo) launch_rk_hash(C.d_in, g.n, lo, hi, L.rkhash - lo, C.st);
    }
    HIPCHK(hipEventRecord(ev[kEvRkEnd], C.st));
    {
        const unsigned long long cnt = a1 - a0;
        G.bt_ready = L.bt_ready; G.bt_pairs = B.bt_pairs; G.bt_flag = L.bt_flag; G.unc = L.unc;
        G.bt_pstride = K.pstride; G.bt_ext = B.bt_ext; G.bt_ext_cap = K.ext_cap; G.bt_ext_cur = &B.v2_hx->ext_cur;
        G.bin_off = L.bin_off; G.bin_pos = L.bin_pos; G.nheads = K.nheads; G.wthreads = K.worker_threads;
        G.abort_word = L.abort_word; G.wcnt = B.wcnt; G.bt_undo = B.bt_undo;
        HIPCHK(hipMemsetAsync(L.bt_ready, 0, cnt * 4 * kBtRec, C.st));
        HIPCHK(hipMemsetAsync(L.bt_flag, 0, cnt * 4, C.st));
        HIPCHK(hipMemsetAsync(L.abort_word, 0, 4, C.st));
        HIPCHK(hipMemsetAsync(L.bin_off, 0, (size_t)nb * (K.nheads + 1) * 4, C.st));
        launch_prefilter(C.d_in, g.n, (uint32_t)a0, (uint32_t)a1, g.wmask, K.t_bits, K.t_bitmap, K.m_bits, B.pf_T, B.pf_M, B.pf_h, B.pf_h2,
                         B.pf_c1, L.unc, C.st);
        launch_bin(C.d_in, g, c0, nb, K.nheads, L.bin_off, B.bin_cur, L.bin_pos, L.unc, (uint32_t)a0, C.st);
        if (K.hot_max) {
            // (a single stream picks its hot bins by the pace of the launch before, which may still be on the device now: select_hot_bins is stream_step's to queue)
            if (K.in_set) select_hot_bins(C, P, C.st);
            G.hot_of_bin = L.hot_of_bin; G.hot_list = L.hot_list; G.hot_undo = B.hot_undo;
        }
    }
    {   // (the progress words of the stages -- everything before the launch's first position is done -- are round_open_kernel's to set)
        P.V.ft = B.v2_ft; P.V.tp = B.v2_tp; P.V.tf = B.v2_tf; P.V.hx = B.v2_hx; P.V.state = B.v2_state; P.V.hb = B.v2_hb;
        G.progress = &B.v2_hx->f_pos;
        G.test_fail = K.test_fail_launch >= 0 && (int64_t)C.v2_launch_no == K.test_fail_launch ? 1u : 0u;
        G.table_shape = K.table_shape; G.launch_par = (uint32_t)(C.v2_launch_no++ & 1u);
    }
    HIPCHK(hipEventRecord(ev[kEvPrepEnd], C.st));
    return 0;
}

// pipe_ms: time of the persistent launch between its own events (a group launch: 0, the set adds it up itself)
// (in three parts, so that the streams of a block set have their frame coders and gathers in flight together: every part of
//  every stream is queued before the next part waits for any of them)
int step_post_issue(Ctx &C, const StepPlan &P)
{
    const StreamConfig &K = C.cfg;
    const LaunchSet &L = C.set[P.set];
    hipEvent_t *ev = C.ev[P.set];
    const uint32_t nb = P.nb;
    C.post_hm.resize(nb); C.post_hoff.resize(nb);
    HIPCHK(hipEventRecord(ev[kEvLaunchEnd], C.st));
    launch_rans(L.syms, K.syms_stride, L.bits, K.bits_stride, L.fmeta, C.buf.scratch, K.syms_stride, C.buf.frames,
                K.frame_stride, (uint32_t)K.frame_stride, nb, C.st);
    HIPCHK(hipEventRecord(ev[kEvCoderEnd], C.st));
    HIPCHK(hipMemcpyAsync(C.post_hm.data(), L.fmeta, nb * sizeof(FrameMeta), hipMemcpyDeviceToHost, C.st));
    // (the stream's next launch may be running: the copy round_close_kernel made)
    HIPCHK(hipMemcpyAsync(&C.post_snap, L.snap, sizeof(v2::RoundSnap), hipMemcpyDeviceToHost, C.st));
    return 0;
}
int step_post_check(Ctx &C, const StepPlan &P)
{
    const Geom &g = C.g;
    const StreamConfig &K = C.cfg;
    const LaunchSet &L = C.set[P.set];
    hipEvent_t *ev = C.ev[P.set];
    const uint32_t c0 = P.c0, c1 = P.c1, nb = P.nb;
    std::vector<FrameMeta> &hm = C.post_hm;
    std::vector<unsigned long long> &hoff = C.post_hoff;
    HIPCHK(hipStreamSynchronize(C.st));
    HIPCHK(hipGetLastError());
    const v2::RoundSnap &Pst = C.post_snap;
    const v2::Hx &h = Pst.hx;
    const uint32_t aborted = Pst.aborted;
    float rk_ms = 0, pre_ms = 0;
    HIPCHK(hipEventElapsedTime(&rk_ms, ev[kEvRkBegin], ev[kEvRkEnd]));
    HIPCHK(hipEventElapsedTime(&pre_ms, ev[kEvRkEnd], ev[kEvPrepEnd]));
    C.tm.prep_ms += rk_ms + pre_ms; C.tm.prep_launches += 5; C.tm.total_ms += rk_ms + pre_ms;
    C.arena_out = false;
    if (Pst.error || h.err) {
        // the first error any stage raised, and where every stage was when it left (nlzm_v2.h: raise(), Hx::dbg)
        WorkerCounters wc{};
        (void)hipMemcpy(&wc, C.buf.wcnt, sizeof wc, hipMemcpyDeviceToHost);
        char where[kErrText];
        stage_error_text(where, sizeof where, h, wc);
        return fail(NLZM_HIP_E_KERNEL, "device error %u in chunks [%u,%u) (parser stopped at chunk %u): %s", Pst.error ? Pst.error : h.err, c0, c1, Pst.next_chunk, where);
    }
    // (the worker lanes drop a pair that finds no extension block and go on: the cursor says how many blocks were asked for)
    C.arena_out = K.ext_cap && h.ext_cur > K.ext_cap;
    if (C.arena_out) return fail(NLZM_HIP_E_KERNEL, "the extension arena of the BT4 pair lists (%u blocks per launch) was used up in chunks [%u,%u): more positions with over %u "
                                     "record-setters than a block set reserves for", K.ext_cap, c0, c1, K.pstride);
    if (aborted) return fail(NLZM_HIP_E_KERNEL, "worker lanes aborted (code %u) in chunks [%u,%u)", aborted, c0, c1);
    if (Pst.next_chunk != c1) return fail(NLZM_HIP_E_KERNEL, "master stopped at chunk %u, expected %u", Pst.next_chunk, c1);
    unsigned long long pos = C.out_pos;
    for (uint32_t f = 0; f < nb; f++) {
        // the reference asserts that the frame fits its buffer (:592, :610); the first one is 4 bytes shorter (:1784)
        const uint32_t room = g.frame_size - ((c0 + f) == 0 ? 4 : 0);
        if (hm[f].out_len > room)
            return fail(NLZM_HIP_E_KERNEL, "frame %u is %u bytes: the reference would assert (:610)", c0 + f, hm[f].out_len);
        hoff[f] = pos; pos += hm[f].out_len;
    }
    if (pos + 4 > C.dst_cap) return fail(NLZM_HIP_E_CAPACITY, "dst_cap %llu too small", (unsigned long long)C.dst_cap);
    if (StageCapture &S = C.stage; S.want_frame >= (int64_t)c0 && S.want_frame < (int64_t)c1) {
        const uint32_t f = (uint32_t)(S.want_frame - c0);
        S.got_meta = hm[f];
        S.got_syms.resize(hm[f].nsyms); S.got_bits.resize(hm[f].nbits_bytes);
        HIPCHK(hipMemcpy(S.got_syms.data(), L.syms + f * K.syms_stride, hm[f].nsyms * 4ull, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(S.got_bits.data(), L.bits + f * K.bits_stride, hm[f].nbits_bytes, hipMemcpyDeviceToHost));
        S.got = true;
    }
    HIPCHK(hipMemcpyAsync(C.buf.dst_off, hoff.data(), nb * sizeof(unsigned long long), hipMemcpyHostToDevice, C.st));
    HIPCHK(hipEventRecord(ev[kEvGatherBegin], C.st));
    launch_gather(C.buf.frames, K.frame_stride, C.buf.dst_off, L.fmeta, C.d_dst, nb, C.st);
    HIPCHK(hipEventRecord(ev[kEvGatherEnd], C.st));
    C.post_pos = pos;
    return 0;
}
int step_post_done(Ctx &C, const StepPlan &P, float pipe_ms)
{
    hipEvent_t *ev = C.ev[P.set];
    const unsigned long long pos = C.post_pos;
    const uint32_t c1 = P.c1;
    HIPCHK(hipStreamSynchronize(C.st));
    float a = pipe_ms, b = 0, c = 0;
    HIPCHK(hipEventElapsedTime(&b, ev[kEvLaunchEnd], ev[kEvCoderEnd]));
    HIPCHK(hipEventElapsedTime(&c, ev[kEvGatherBegin], ev[kEvGatherEnd]));
    C.tm.match_parse_ms += a; C.tm.match_parse_launches++;
    if (a > 0) C.last_launch_ms = a;
    C.tm.rans_ms += b + c; C.tm.rans_launches++;
    C.tm.total_ms += a + b + c;
    C.out_pos = pos;
    C.next_chunk = c1;
    return 0;
}
// A call's launches follow one another without the device waiting for the host's work between them (StreamConfig::depth 2).  The pre-pass of
// launch k + 1 is queued on the stream's HIP stream while launch k is on the device; when launch k has ended -- the hot bins of launch k + 1 are
// picked by the pace of launch k, as they always were -- launch k + 1 goes on the launch stream at once, and only then are the frames of launch k
// coded, copied and gathered, on the stream's HIP stream beside launch k + 1.  The per-stream buffers of the coder and the gather (scratch, frames,
// dst_off) are used in that HIP stream's order: launch k + 1's coder follows launch k's gather.  A launch is bracketed by round_open_kernel and
// round_close_kernel like a block set's: the progress words are set and copied aside on the device, and a launch queued behind a failed one -- the
// host has not looked at launch k when it queues k + 1 -- leaves at once (the sticky Persist::error).  With depth 1 -- no room for a second launch
// set -- every launch is collected before the next pre-pass is queued: the same loop.  Nothing stays queued when the call returns, whatever it returns.
int stream_step(Ctx &C, uint32_t max_chunks, uint64_t *in_done, uint64_t *out_done, int *finished)
{
    if (!C.open) return fail(NLZM_HIP_E_ARG, "no open stream");
    if (!C.launch_st) return fail(NLZM_HIP_E_ARG, "the stream has no launch stream (a stream of a block set steps with its set)");
    const Geom &g = C.g;
    uint32_t todo = g.nchunks - C.next_chunk;
    if (max_chunks && todo > max_chunks) todo = max_chunks;
    StepPlan plan[2];
    uint32_t head = 0, prepped = 0, launched = 0;       // of the launches plan[head & 1] ..: `prepped` have their pre-pass queued, the first `launched` of them the launch too
    auto prepare = [&](StepPlan &P) -> int {
        const int rc = step_pre(C, todo, P);
        if (!rc) todo -= P.nb;
        return rc;
    };
    auto launch = [&](const StepPlan &P) -> int {
        hipEvent_t *lev = C.launch_ev[P.set];
        void *pack = (uint8_t *)C.launch_pack + P.set * pack_entry_bytes();
        fill_stream2_args(pack, 0, g, P.G, P.V, P.c0, P.c1, C.set[P.set].snap);
        HIPCHK(hipStreamWaitEvent(C.launch_st, C.ev[P.set][kEvPrepEnd], 0));
        if (C.cfg.hot_max) select_hot_bins(C, P, C.launch_st);
        launch_round_open(pack, 1, C.launch_st);
        HIPCHK(hipEventRecord(lev[0], C.launch_st));
        launch_pipeline2(g, P.G, P.V, P.c0, P.c1, C.cfg.worker_blocks, C.launch_st);
        HIPCHK(hipEventRecord(lev[1], C.launch_st));
        launch_round_close(pack, 1, C.launch_st);
        HIPCHK(hipEventRecord(lev[2], C.launch_st));
        return 0;
    };
    auto ended = [&](const StepPlan &P, float &ms) -> int {         // waits for the launch itself, not for what is queued behind it
        hipEvent_t *lev = C.launch_ev[P.set];
        HIPCHK(hipEventSynchronize(lev[1]));
        HIPCHK(hipEventElapsedTime(&ms, lev[0], lev[1]));
        if (ms > 0) C.last_launch_ms = ms;
        return 0;
    };
    auto collect = [&](const StepPlan &P) -> int {
        HIPCHK(hipStreamWaitEvent(C.st, C.launch_ev[P.set][2], 0));
        int rc = step_post_issue(C, P);
        if (!rc) rc = step_post_check(C, P);
        float ms = 0;
        if (!rc) rc = ended(P, ms);
        return rc ? rc : step_post_done(C, P, ms);
    };
    int rc = 0;
    while (!rc && (todo || prepped)) {
        while (!rc && todo && prepped < C.cfg.depth) { rc = prepare(plan[(head + prepped) & 1]); if (!rc) prepped++; }
        if (!rc && !launched) { rc = launch(plan[head & 1]); launched = 1; }
        if (!rc && prepped > 1) { float ms = 0; rc = ended(plan[head & 1], ms); if (!rc) rc = launch(plan[(head + 1) & 1]); launched = 2; }
        if (!rc) { rc = collect(plan[head & 1]); head++; prepped--; launched--; }
    }
    if (rc) {       // (the text is the failing launch's; what is queued behind it is waited for -- every device wait is bounded -- and looked at by nobody)
        (void)hipStreamSynchronize(C.launch_st);
        (void)hipStreamSynchronize(C.st);
        (void)hipGetLastError();
        return rc;
    }
    if (in_done) {
        const unsigned long long d = (unsigned long long)C.next_chunk * g.chunk_size;
        *in_done = d < g.n ? d : g.n;
    }
    if (out_done) *out_done = C.out_pos;
    if (finished) *finished = C.next_chunk >= g.nchunks;
    return 0;
}

namespace {
// report: the stages' cycle accounting of the stream on stderr (option "stage_report")
int refresh_stats(Ctx &C, bool report)
{
    Persist P;
    HIPCHK(hipMemcpy(&P, C.buf.persist, sizeof P, hipMemcpyDeviceToHost));
    nlzm_hip_stats &s = C.stats;
    s.out_bytes = C.out_pos;
    s.bt_calls = P.cnt.bt_calls; s.bt_tests = P.cnt.bt_tests; s.cmp_bytes = P.cnt.cmp_bytes; s.ht_rows = P.cnt.ht_rows;
    s.rk_probes = P.cnt.rk_probes; s.rk_inserts = P.cnt.rk_inserts; s.positions = P.cnt.positions;
    s.nice_positions = P.cnt.nice_positions; s.segments = P.cnt.segments; s.n_literal = P.cnt.n_literal;
    s.n_dict = P.cnt.n_dict; s.n_rep = P.cnt.n_rep; s.rans_syms = P.cnt.rans_syms; s.bit_ops = P.cnt.bit_ops;
    s.frames = P.cnt.frames; s.shifts = P.cnt.shifts; s.uncertain_positions = P.cnt.uncertain_positions;
    memcpy(C.prof_last, P.prof, sizeof C.prof_last);
    acct_figures(P, C.acct);
    if (report) stage_report(stderr, P);
    WorkerCounters wc;
    HIPCHK(hipMemcpy(&wc, C.buf.wcnt, sizeof wc, hipMemcpyDeviceToHost));
    s.bt_calls += wc.bt_calls; s.bt_tests += wc.bt_tests; s.cmp_bytes += wc.cmp_bytes;
    C.wc_last = wc;
    if (report) worker_report(stderr, wc, C.cfg.hot_max != 0);
    return 0;
}
}  // namespace

int stream_finish(Ctx &C, uint64_t *dst_len, bool report)
{
    if (!C.open) return fail(NLZM_HIP_E_ARG, "no open stream");
    if (C.next_chunk < C.g.nchunks) return fail(NLZM_HIP_E_ARG, "stream not finished (%u of %u chunks)", C.next_chunk, C.g.nchunks);
    if (C.out_pos + 4 > C.dst_cap) return fail(NLZM_HIP_E_CAPACITY, "dst_cap too small");
    HIPCHK(hipMemsetAsync(C.d_dst + C.out_pos, 0, 4, C.st));        // terminator (:1891-1895)
    C.out_pos += 4;
    HIPCHK(hipStreamSynchronize(C.st));
    const int rc = refresh_stats(C, report);
    if (rc) return rc;
    if (dst_len) *dst_len = C.out_pos;
    return 0;
}

int dev_init(DevState &D, int device)
{
    Ctx &C = D.ctx;
    // Block mode queues the pre-pass kernels and frame coders of 32 streams beside a persistent launch, each stream on a HIP stream of its
    // own: with the runtime's default of 4 hardware queues they would line up behind one another.  The runtime reads the variable when it
    // starts, i.e. at this process's first HIP call -- ours, unless the host program has made one already (then it has to export
    // GPU_MAX_HW_QUEUES=16 itself: include/nlzm_hip.h).  A value the caller has set is left alone.  Set, never read: the library has no
    // environment knobs of its own.
    // (once per process, and only here -- the per-device threads of nlzm_hip_compress_blocks_multi come in with the runtime long started.  What the
    //  runtime will have read is kept for nlzm_hip_get_counter("gpu_max_hw_queues_effective"): the caller's value; 16 if this call set it in time;
    //  the runtime's default of 4 if the process had the GPU open already -- /dev/kfd among its files -- when this library was first called.)
    static std::once_flag hwq_once;
    std::call_once(hwq_once, [] {
        const char *have = getenv("GPU_MAX_HW_QUEUES");
        if (have && *have) { g_hwq_effective = atoi(have); return; }
        bool kfd = false;
        if (DIR *d = opendir("/proc/self/fd")) {
            while (struct dirent *e = readdir(d)) {
                char path[64], to[64];
                snprintf(path, sizeof path, "/proc/self/fd/%s", e->d_name);
                const ssize_t k = readlink(path, to, sizeof to - 1);
                if (k > 0) { to[k] = 0; if (!strcmp(to, "/dev/kfd")) kfd = true; }
            }
            closedir(d);
        }
        if (kfd) { g_hwq_effective = 4; return; }       // (too late to matter: left alone)
        (void)setenv("GPU_MAX_HW_QUEUES", "16", 0);
        g_hwq_effective = 16;
    });
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(NLZM_HIP_E_NODEVICE, "no HIP device (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(NLZM_HIP_E_ARG, "device %d out of range (%d present)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(NLZM_HIP_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    if (C.inited && C.device == device) return 0;
    if (C.inited) dev_shutdown(D);
    C.device = device;
    C.cu_count = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&C.st, hipStreamNonBlocking));
    for (auto &set : C.ev) for (auto &ev : set) HIPCHK(hipEventCreate(&ev));
    C.inited = true;
    return 0;
}

void dev_shutdown(DevState &D)
{
    Ctx &C = D.ctx;
    if (!C.inited) return;
    blocks_close(D, true);
    feed_close(D);
    free_stream_buffers(C);
    release_own_io(C);
    if (C.stage.cap_words) { (void)hipFree(C.stage.cap_words); C.stage.cap_words = nullptr; }
    if (C.stage.cap_used) { (void)hipFree(C.stage.cap_used); C.stage.cap_used = nullptr; }
    for (auto &set : C.ev) for (auto &ev : set) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    release_launch_stream(C);
    if (C.st) { (void)hipStreamDestroy(C.st); C.st = nullptr; }
    C.inited = false;
}

}  // namespace host

// ---- what the read side's entry points (nlzm_hip_decode.cpp, nlzm_hip_crc.cpp, nlzm_hip_range.cpp) use of this file's state: the
// library's stream; what this file uses of theirs is declared in the same header (nlzm_host_util.h) ----
int host_stream(hipStream_t *st)
{
    Ctx &C = cur().ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded (no device: there is no CPU fallback)");
    *st = C.st;
    return 0;
}
void host_decode_setup(int64_t *ring_option, int *cu_count)
{
    const DevState &D = cur();
    *ring_option = D.opt.decode_ring; *cu_count = D.ctx.cu_count;
}
}  // namespace nlzm

extern "C" {

int nlzm_hip_init(int device) { return dev_init(cur(), device); }
void nlzm_hip_shutdown(void) { dev_shutdown(cur()); }

const char *nlzm_hip_last_error(void) { return g_err; }

uint64_t nlzm_hip_compress_bound(uint64_t n)
{
    // worst ratio frame_size/chunk_size is 16384/14848 (hist_bits <= 16)
    return 16 + 131072 + (n / 14848 + 1) * 16384;
}

void nlzm_hip_geometry(uint64_t flen, uint32_t hist_bits_req, uint32_t *hist_bits, uint32_t *frame_bits,
                       uint32_t *chunk_size, uint32_t *feed_size)
{
    Geom g;
    make_geom(flen, hist_bits_req, g);
    if (hist_bits) *hist_bits = g.wbits;
    if (frame_bits) *frame_bits = g.frame_bits;
    if (chunk_size) *chunk_size = g.chunk_size;
    if (feed_size) *feed_size = g.feed;
}

int nlzm_hip_stream_begin(const void *d_src, uint64_t n, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap)
{
    DevState &D = cur();
    release_own_io(D.ctx);
    return stream_begin(D.ctx, D.opt, d_src, n, hist_bits_req, d_dst, dst_cap);
}
int nlzm_hip_stream_step(uint32_t max_chunks, uint64_t *in_done, uint64_t *out_done, int *finished) { return stream_step(cur().ctx, max_chunks, in_done, out_done, finished); }
int nlzm_hip_stream_finish(uint64_t *dst_len) { DevState &D = cur(); return stream_finish(D.ctx, dst_len, D.opt.report != 0); }

int nlzm_hip_compress_dev(const void *d_src, uint64_t n, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap,
                          uint64_t *dst_len)
{
    int rc = nlzm_hip_stream_begin(d_src, n, hist_bits_req, d_dst, dst_cap);
    if (rc) return rc;
    rc = nlzm_hip_stream_step(0, nullptr, nullptr, nullptr);
    if (rc) return rc;
    return nlzm_hip_stream_finish(dst_len);
}

int nlzm_hip_compress(const uint8_t *src, uint64_t n, uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap,
                      uint64_t *dst_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if ((!src && n) || !dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    if (n >= 0xFFFF0000ull) return fail(NLZM_HIP_E_TOOBIG, "input too large");
    const uint64_t bound = nlzm_hip_compress_bound(n);
    int rc = alloc_own_io(C, n, bound);
    if (rc) return rc;
    HIPCHK(hipEventRecord(C.ev[0][kEvCallBegin], C.st));
    if (n) HIPCHK(hipMemcpyAsync(C.own_in, src, n, hipMemcpyHostToDevice, C.st));
    HIPCHK(hipEventRecord(C.ev[0][kEvCallEnd], C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    float h2d = 0;
    HIPCHK(hipEventElapsedTime(&h2d, C.ev[0][kEvCallBegin], C.ev[0][kEvCallEnd]));
    rc = stream_begin(C, D.opt, C.own_in, n, hist_bits_req, C.own_dst, bound);
    if (rc) return rc;
    rc = stream_step(C, 0, nullptr, nullptr, nullptr);
    if (rc) return rc;
    uint64_t len = 0;
    rc = stream_finish(C, &len, D.opt.report != 0);
    if (rc) return rc;
    if (len > dst_cap) return fail(NLZM_HIP_E_CAPACITY, "stream is %llu bytes, dst_cap %llu", (unsigned long long)len, (unsigned long long)dst_cap);
    HIPCHK(hipEventRecord(C.ev[0][kEvCallBegin], C.st));
    HIPCHK(hipMemcpyAsync(dst, C.own_dst, len, hipMemcpyDeviceToHost, C.st));
    HIPCHK(hipEventRecord(C.ev[0][kEvCallEnd], C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    float d2h = 0;
    HIPCHK(hipEventElapsedTime(&d2h, C.ev[0][kEvCallBegin], C.ev[0][kEvCallEnd]));
    C.tm.h2d_ms = h2d; C.tm.d2h_ms = d2h;
    *dst_len = len;
    return 0;
}

int nlzm_hip_get_stats(nlzm_hip_stats *out)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!out) return fail(NLZM_HIP_E_ARG, "null argument");
    if (C.open) { const int rc = refresh_stats(C, D.opt.report != 0); if (rc) return rc; }
    *out = C.stats;
    return 0;
}

int nlzm_hip_get_counter(const char *key, uint64_t *value)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!key || !value) return fail(NLZM_HIP_E_ARG, "null argument");
    if (!strncmp(key, "decode_", 7)) return nlzm::decode_counter(key, value);
    if (!strncmp(key, "crc_", 4)) return nlzm::crc_counter(key, value);
    if (!strncmp(key, "range_", 6)) return nlzm::range_counter(key, value);
    if (!strncmp(key, "cut_", 4)) return nlzm::cut_counter(key, value);
    if (!strncmp(key, "dedup_", 6)) return nlzm::dedup_counter(key, value);
    if (!strncmp(key, "planes_", 7)) return nlzm::planes_counter(key, value);
    if (!strncmp(key, "elem_", 5)) return nlzm::elem_counter(key, value);
    if (C.open) { const int rc = refresh_stats(C, D.opt.report != 0); if (rc) return rc; }
    if (compress_counter(key, C.prof_last, C.wc_last, C.stats.positions, value)) return 0;
    if (!strcmp(key, "block_pool_bytes")) { *value = D.blocks_pool_size; return 0; }
    if (!strcmp(key, "block_redo_streams")) { *value = D.redo_streams; return 0; }
    if (!strcmp(key, "container_sets")) { *value = D.container_sets; return 0; }
    if (!strcmp(key, "gpu_max_hw_queues_effective")) { *value = (uint64_t)g_hwq_effective; return 0; }
    return fail(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

int nlzm_hip_get_timing(nlzm_hip_timing *out)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!out) return fail(NLZM_HIP_E_ARG, "null argument");
    *out = C.tm;
    return 0;
}

void nlzm_hip_block_placement(uint32_t nstreams, uint32_t blocks_per_stream, uint32_t workgroup, uint32_t *stream, uint32_t *local)
{
    uint32_t s = 0, l = 0;
    multi_block_of(nstreams * blocks_per_stream, blocks_per_stream, workgroup, s, l);
    if (stream) *stream = s;
    if (local) *local = l;
}

// Every key of nlzm_hip_set_option that stores a value: its member of Options, and what it accepts.  ("workers" stores nothing.)
enum OptKind { kOptRange,       // lo <= value <= hi
               kOptLanes,       // ... and a multiple of 64
               kOptFlag,        // stored as value != 0
               kOptRing,        // 0, or one of the rings the one-shot decoder is built with
               kOptAny };       // stored as it is
static const struct { const char *key; int64_t Options::*member; OptKind kind; int64_t lo, hi; } kOptions[] = {
    { "worker_blocks", &Options::worker_blocks, kOptRange, 1, 255 },
    { "hot_waves", &Options::hot_waves, kOptRange, 0, 6 },
    { "hot_min", &Options::hot_min, kOptRange, 0, 1 << 30 },
    { "worker_threads", &Options::worker_threads, kOptLanes, 64, 512 },
    { "block_worker_threads", &Options::block_threads, kOptLanes, 64, 512 },
    { "block_hot_waves", &Options::block_hot_waves, kOptRange, 0, 6 },
    { "prefilter_bits_per_position", &Options::tbits_per, kOptRange, 0, 8 },
    { "stage_report", &Options::report, kOptFlag, 0, 0 },
    { "parser_helper", &Options::helper, kOptFlag, 0, 0 },
    { "table_shape", &Options::table_shape, kOptRange, 0, 2 },
    { "multi_allow_same_device", &Options::multi_same, kOptFlag, 0, 0 },
    { "test_fail_launch", &Options::test_fail_launch, kOptAny, 0, 0 },
    { "test_fail_stream", &Options::test_fail_stream, kOptRange, 0, 63 },
    { "block_ext_blocks", &Options::block_ext_blocks, kOptAny, 0, 0 },
    { "block_parser_helper", &Options::block_helper, kOptFlag, 0, 0 },
    { "keep_block_pool", &Options::keep_pool, kOptFlag, 0, 0 },
    { "block_batch_chunks", &Options::block_batch, kOptRange, 1, 4096 },
    { "batch_chunks", &Options::batch, kOptRange, 1, 4096 },
    { "container_set_blocks", &Options::container_set_blocks, kOptRange, 1, 64 },      // (... and the device's capacity, once it is known)
    { "decode_ring", &Options::decode_ring, kOptRing, 0, 0 },
};

int nlzm_hip_set_option(const char *key, int64_t value)
{
    DevState &D = cur();
    if (!key) return fail(NLZM_HIP_E_ARG, "null key");
    if (!strcmp(key, "workers")) {      // BT4 always runs on the worker lanes (the three-stage pipeline has no other place for it)
        if (value != 1) return fail(NLZM_HIP_E_ARG, "workers: only 1 is supported");
        return 0;
    }
    if (const int rc = nlzm::dedup_set_option(key, value); rc <= 0) return rc;     // ("dedup_ranges", "test_dedup_hash_bits": nlzm_hip_dedup.cpp keeps them)
    for (const auto &o : kOptions) {
        if (strcmp(key, o.key)) continue;
        const bool ranged = o.kind == kOptRange || o.kind == kOptLanes;
        if (ranged && (value < o.lo || value > o.hi || (o.kind == kOptLanes && value % 64))) return fail(NLZM_HIP_E_ARG, "%s out of range", key);
        if (o.kind == kOptRing && value != 0 && value != 65536 && value != 16384) return fail(NLZM_HIP_E_ARG, "%s: 0 (automatic), 65536 or 16384", key);
        if (o.member == &Options::container_set_blocks && D.ctx.inited && value > (int64_t)blocks_capacity(D))
            return fail(NLZM_HIP_E_ARG, "%s out of range (this device holds %u streams at once)", key, blocks_capacity(D));
        D.opt.*o.member = o.kind == kOptFlag ? (int64_t)(value != 0) : value;
        if (o.member == &Options::keep_pool && !value && D.jobs.empty()) blocks_close(D, true);    // (the allocation a closed set left behind goes at once)
        return 0;
    }
    return fail(NLZM_HIP_E_ARG, "unknown option %s", key);
}

}  // extern "C"
