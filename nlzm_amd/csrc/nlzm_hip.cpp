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

#include <array>
#include <mutex>
#include <thread>
#include <chrono>
#include <algorithm>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_core.h"
#include "nlzm_v2.h"
#include "nlzm_report.h"

#include "nlzm_launch.h"

using namespace nlzm;

namespace {

char g_err[2048] = "";
std::mutex g_err_mu;            // block streams run on host threads
char *thread_err();             // the error text of the device state this thread works for (a multi-device call: one per device)
int set_err(int code, const char *fmt, ...)
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    if (char *te = thread_err()) memcpy(te, g_err, sizeof g_err);
    return code;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return set_err(e_ == hipErrorOutOfMemory ? NLZM_HIP_E_NOMEM : NLZM_HIP_E_NODEVICE,    \
                           "%s failed: %s", #expr, hipGetErrorString(e_));                        \
    } while (0)

int g_hwq_effective = 0;                           // what the HIP runtime reads as GPU_MAX_HW_QUEUES (dev_init)
struct DevState;
void blocks_close(DevState &D, bool drop_pool = false);    // defined with the block-set entry points
bool idle_block_pool_dropped();                    // no block set open and its kept allocation still there: frees it, true (defined there too)

inline uint32_t clampu(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One allocation for everything a stream keeps on the device (block mode: one for the whole block set).  A context without a
// pool takes every buffer from hipMalloc by itself.
struct Pool {
    uint8_t *base = nullptr;
    size_t size = 0, used = 0;
    bool measuring = false;             // only add up what the stream would take
};

// What the caller has set (nlzm_hip_set_option), one per device state.  A stream reads them when it is opened -- stream_begin resolves them
// into its StreamConfig -- and nothing but nlzm_hip_set_option writes them.
struct Options {
    int64_t batch = 32;
    int64_t worker_blocks = 240;            // + the stage blocks, one 512-thread block per CU.  Round 5: with the serial half at 400 - 460 cycles per position the
                                            // number of worker CUs matters again at depth -- a lane's bin holds the heads h with h % lanes equal, a long call of one
                                            // head holds up the positions of the others, and the finder stage waits: the whole 1e9-byte stream with 60 / 240
                                            // worker CUs 459 / 412 cycles per position (BT4 results waited for: 173 / 127), 300 MB 399 / 396.  Round 3 had measured (profiles/
                                            // r03_worker_cu_sweep.log): 240 / 120 / 60 / 30 / 16 / 8 worker CUs give 3.71 / 3.72 / 3.72 / 3.70 / 3.70 / 3.63 MB/s
                                            // at 150 MB depth and 240 / 60 / 32 the same at 20 MB and 300 MB -- the lanes are there for latency, and the hot
                                            // bins have waves of their own; 60 leaves a margin and three quarters of the device to other streams
    int64_t worker_threads = 128;           // lanes of a worker block that take bins (with two of a CU's eight waves walking trees a test takes less
                                            // time than with all eight -- measured at 60 MB: 512 lanes per CU 2.48 MB/s, 256 2.58, 128 2.62, 64 2.62)
    int64_t hot_waves = 2;                  // waves of a worker block behind its bin-taking lanes that take a hot bin each (0: none)
    int64_t hot_min = 0;                    // positions per launch from which a bin may count as hot; 0 (default): by the stream's pace.  A bin needs a wave when its calls
                                            // come faster than a lane serves them -- a lane's call costs ~42 us with its lockstep partners' --, and how fast they come hangs on
                                            // how fast the FINDER moves: bins of 24 positions per millisecond of the launch before and more (the first launch: positions / 240).
                                            // Measured at launches of 8 chunks (profiles/r06_ab_runs.txt): the stand-in (166 ms a launch) 401 / 390 / 382 / 371 cycles per position
                                            // at 8,192 / 6,144 / 4,096 / 2,048; markup (362 ms) 872 / 906 / 1,005 / 1,007 -- a wave's call takes twice a lane's (its steps are
                                            // heavier), which is lost where a lane would have kept up.  Rounds 3 - 5 had 8,192 fixed.
    int64_t tbits_max = 34;                 // log2 of the pre-filter table's entries at most (block mode shrinks it to fit)
    int64_t block_threads = 320;            // block mode: lanes of a worker block that take bins, and the waves behind them that take a hot bin each.  Measured
    int64_t block_hot_waves = 3;            // with 32 streams of 17 MB (4 worker CUs each): 512 lanes and no such waves 9.6 s, 256 + 4 waves 8.2 s, 128 + 6 waves 8.6 s
                                            // (profiles/r04_block_mode.txt): under load a stream waits for the serial chains of its busiest heads
    int64_t block_batch = 8;                // block mode: chunks of every stream per shared launch (the rounds overlap, so their length matters little --
                                            // 6 / 8 / 12 / 16 chunks: 88.9 / 89.8 / 88.7 / 89.6 MB/s; the pool holds 2.3 KB per position of a launch and stream)
    int64_t tbits_per = 4;                  // log2 of the pre-filter table's entries per input position (capped by window + 5 and 32 bits)
    int64_t keep_pool = 1;                  // block mode keeps its one allocation when a set is closed: the driver clears freed device memory, and an allocation
                                            // made soon after a large one was freed waits for that -- opening 32 streams took 0.12 s or 4.5 s (tests/gpu_begin_probe.py)
    int64_t helper = 1;                     // a helper parser workgroup (nlzm_v2.h, HelpBox): 1 CU more per stream.  The streams of a block
    int64_t block_helper = 0;               // set run without one unless "block_parser_helper" says otherwise (a stream of a full device waits for its BT4 results)
    int64_t multi_same = 0;                 // test only ("multi_allow_same_device"): nlzm_hip_compress_blocks_multi accepts a device twice, so that its
                                            // threads, device states and gather loop run with two parts on a box with one GPU
    int64_t table_shape = 0;                // the table stage's shape ("table_shape"): 0 every launch in the shape the launch before it asked for (nlzm_v2.h, TLds), 1 always 16-entry
                                            // fronts on seven waves, 2 always 24 entries on five
    int64_t test_fail_launch = -1;          // test only ("test_fail_launch", with "test_fail_stream" = index of the stream of a block set): the finder stage of that launch raises
    int64_t test_fail_stream = 0;           // an error at once -- the fault path of a round that is queued behind a failing one
    int64_t block_ext_blocks = -1;          // test only ("block_ext_blocks"): extension blocks of a block-set stream's pair-list arena per launch (default: positions / 64 + 1024)
    int64_t report = 0;                     // 1: the stages' cycle accounting of every finished stream on stderr (nlzm_hip_set_option "stage_report")
    int64_t container_set_blocks = 32;      // blocks per set of a container of more blocks than one launch holds ("container_set_blocks"; nlzm_container_plan.h)
    int64_t decode_ring = 0;                // the one-shot decoder's LDS ring ("decode_ring"): 0 by the number of streams, 65536 / 16384 the big / the small kernel
};

// What the open stream runs with: resolved by stream_begin from the options as they were then, the stream's geometry and its place (by itself,
// or one of a block set).  Its buffers are sized for it and every launch reads it: "what is open keeps what it was opened with".
struct StreamConfig {
    bool in_set = false;                    // a stream of a block set: buffers from the set's pool, two launch sets, short pair lists and an arena
    uint32_t batch = 0;                     // chunks per launch
    uint32_t worker_blocks = 0, worker_threads = 0;
    uint32_t nheads = 0;                    // bins: one per worker lane (or per head when there are fewer heads than lanes)
    uint32_t hot_max = 0;                   // waves that take a hot bin each, over all worker blocks (0: none)
    uint32_t hot_min = 0;                   // option "hot_min" (0: by the stream's pace)
    uint32_t t_bits = 0, m_bits = 0;
    uint32_t t_bitmap = 0;                  // the pre-filter table holds one bit per slot (a stream no longer than its window: every earlier position is inside it)
    uint32_t pstride = kBtMaxPairs, ext_cap = 0;       // pairs reserved per position; extension blocks for the rest
    bool helper = false;                    // a helper parser workgroup
    uint32_t table_shape = 0;
    int64_t test_fail_launch = -1;
    unsigned long long rkhash_len = 0;      // entries of rkhash (a launch's positions and their lookahead)
    unsigned long long syms_stride = 0, bits_stride = 0, frame_stride = 0;
};

// Everything that exists once per launch set: what a pre-pass writes or a frame coder reads.  A single stream has one.  Block mode queues
// launch k + 1 (and runs its pre-pass) while launch k is on the device and codes the frames of launch k while launch k + 1 is: a stream of
// a block set has two, and a pre-pass that runs ahead makes the other one the current one (Ctx::set_idx).
struct LaunchSet {
    uint32_t *rkhash = nullptr, *bt_ready = nullptr, *bt_flag = nullptr, *abort_word = nullptr, *bin_off = nullptr, *bin_pos = nullptr,
             *hot_of_bin = nullptr, *hot_list = nullptr, *syms = nullptr;
    uint8_t *unc = nullptr, *bits = nullptr;
    FrameMeta *fmeta = nullptr;
    v2::RoundSnap *snap = nullptr;          // (block mode) what round_close_kernel copies aside for the host
};

// The device buffers a stream has once, whatever the number of its launch sets.
struct StreamBuffers {
    uint32_t *ht2 = nullptr, *ht3 = nullptr, *rk_table = nullptr, *bt_heads = nullptr, *bt_tree = nullptr;
    Persist *persist = nullptr;
    uint32_t *scratch = nullptr;
    uint8_t *frames = nullptr;
    unsigned long long *dst_off = nullptr;
    uint32_t *pf_T = nullptr, *pf_M = nullptr, *pf_h = nullptr, *pf_h2 = nullptr; uint8_t *pf_c1 = nullptr;
    uint32_t *bt_pairs = nullptr, *bt_ext = nullptr;
    uint32_t *bin_cur = nullptr, *bt_undo = nullptr;
    unsigned long long *hot_undo = nullptr;
    WorkerCounters *wcnt = nullptr;
    // three-stage pipeline (nlzm_v2.h): hand-off rings, progress words, stage state
    uint32_t *v2_ft = nullptr, *v2_tp = nullptr, *v2_tf = nullptr, *v2_state = nullptr;
    v2::Hx *v2_hx = nullptr;
    v2::HelpBox *v2_hb = nullptr;
};

// the events of a launch set: what a step brackets with them, and two for a call's own timing (nlzm_hip_compress: upload and download; a block set's step: its device time)
enum { kEvLaunchBegin, kEvLaunchEnd /* = frame coder begin */, kEvCoderEnd, kEvGatherBegin, kEvGatherEnd, kEvRkBegin, kEvRkEnd /* = rest of the pre-pass begin */, kEvPrepEnd,
       kEvCallBegin, kEvCallEnd, kEvN };
struct Ctx {
    bool inited = false;
    int device = 0, cu_count = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[2][kEvN] = {};             // per launch set (the second one's: block mode)
    Pool *pool = nullptr;                   // (block mode) where the stream's buffers come from

    // the open stream
    bool open = false;
    StreamConfig cfg;
    Geom g{};
    const uint8_t *d_in = nullptr;
    uint8_t *d_dst = nullptr;
    uint64_t dst_cap = 0, out_pos = 0;
    uint32_t next_chunk = 0;                // chunks below this are coded and gathered
    uint32_t pre_chunk = 0;                 // chunks below this have had their pre-pass queued (block mode runs it a launch ahead)
    uint32_t v2_launch_no = 0;              // persistent launches of the open stream so far (its parity picks the table stage's shape slot)

    // device buffers: free_stream_buffers gives back what dev_alloc took from hipMalloc for them (the rest lies in the set's pool)
    StreamBuffers buf;
    LaunchSet set[2];
    uint32_t set_idx = 0;                   // the current launch set
    std::vector<void *> owned;
    // copies of the caller's buffers for the host-buffer entry points: kept across a stream_begin
    uint8_t *own_in = nullptr, *own_dst = nullptr;

    // capture (stage tests)
    uint32_t *cap_words = nullptr; unsigned long long cap_cap = 0, cap_lo = 0, cap_hi = 0; unsigned long long *cap_used = nullptr;
    // frame capture for parse_emit
    int64_t want_frame = -1;
    std::vector<uint32_t> got_syms; std::vector<uint8_t> got_bits; FrameMeta got_meta{};
    bool got = false;

    // run state: what the step's frame coder has reported (step_post_issue .. _done), the progress words on their way to or from the device,
    // timing.  Asynchronous copies read and write these: they stay where they are while the stream is open.
    v2::Hx hx_host;
    std::vector<FrameMeta> post_hm; std::vector<unsigned long long> post_hoff; Persist post_P; uint32_t post_aborted = 0; unsigned long long post_pos = 0;
    v2::RoundSnap post_snap;
    double last_launch_ms = 0;              // duration of the stream's last persistent launch (0: none yet)
    bool arena_out = false;                 // the last step_post_check failed because the launch used its pair-list arena up (block mode makes the stream again by itself)
    nlzm_hip_stats stats{};
    nlzm_hip_timing tm{};
    // of the last finished stream
    unsigned long long prof_last[kPfSlots] = {}; // Persist::prof and the worker lanes' counters (nlzm_hip_get_counter)
    WorkerCounters wc_last{};
    double acct[8] = {};                    // cycles per position, row by row of kAcctRows (nlzm_report.h)
};

// a device buffer of the stream: from its pool, or from hipMalloc (then the stream owns it)
template <class T> int dev_alloc(Ctx &C, T **p, size_t bytes)
{
    if (!C.pool) {
        hipError_t e = hipMalloc((void **)p, bytes);
        if (e == hipErrorOutOfMemory && idle_block_pool_dropped()) {    // (the allocation a closed block set left behind: given back, once, for this one)
            (void)hipGetLastError();
            e = hipMalloc((void **)p, bytes);
        }
        if (e != hipSuccess) return set_err(e == hipErrorOutOfMemory ? NLZM_HIP_E_NOMEM : NLZM_HIP_E_NODEVICE, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        C.owned.push_back(*p);
        return 0;
    }
    Pool &P = *C.pool;
    const size_t at = (P.used + 255) & ~(size_t)255;
    if (!P.measuring && at + bytes > P.size) return set_err(NLZM_HIP_E_NOMEM, "stream pool of %zu bytes is too small", P.size);
    *p = P.measuring ? nullptr : (T *)(P.base + at);
    P.used = at + bytes;
    return 0;
}
#define DEVALLOC(ptr, bytes) do { const int rc_ = dev_alloc(C, &(ptr), (bytes)); if (rc_) return rc_; } while (0)
#define DEVFILL(expr) do { if (!(C.pool && C.pool->measuring)) HIPCHK(expr); } while (0)

//   (the plan names the launch set -- buffers and events -- the step was queued with: block mode has two steps of a stream open at a time)
struct StepPlan {
    uint32_t c0 = 0, c1 = 0, nb = 0; Globals G; v2::GlobalsV2 V;
    uint32_t set = 0;
    bool ahead = false;                         // the launch is followed by round_close_kernel: the host reads the set's `snap`
};

struct BlockJob {
    Ctx c;
    uint64_t lo = 0, n = 0, len = 0, bound = 0;
    uint8_t *d_out = nullptr;
    int rc = 0;
    bool redo = false;                              // a launch of this stream used its pair-list arena up: the stream is made again, by itself, when the set is finished
    Pool pool;                                      // this stream's slice of the block set's one allocation
};

// Everything the entry points keep per device: the single-stream context and the open block set.  The process-wide one serves
// the one-device API (nlzm_hip_init picks its device); a multi-device call gives each of its per-device host threads one
// of its own and points `t_dev` at it, so that the same code runs on every device at once.
struct DevState {
    char err[sizeof g_err] = "";                    // the last error raised by a thread that works for this state
    Ctx ctx;                                        // the context behind the single-stream entry points
    Options opt;                                    // what nlzm_hip_set_option has set
    std::vector<BlockJob> jobs;                     // the open block set (nlzm_hip_blocks_begin .. _finish)
    uint8_t *blocks_pool = nullptr;                 // ... and the one allocation all its streams' buffers lie in: kept between block sets
    size_t blocks_pool_size = 0;                    //     (option keep_block_pool) and used again by the next set that fits
    std::vector<hipStream_t> group_st;              // one HIP stream and an event pair per shared launch of a round
    std::vector<std::array<hipEvent_t, 3>> group_ev;   // per launch set: launch begins / ends / its results are copied aside
    void *pack_host = nullptr, *pack_dev = nullptr; // the streams' launch arguments of a round: pinned host copy, device copy
    uint64_t blocks_n = 0;
    const uint8_t *blocks_src = nullptr;
    uint32_t blocks_hist = 0;
    int64_t blocks_wb = 0;
    uint64_t blocks_per = 0;                        // bytes per block when the caller fixes the partition (0: ceil(n / nblocks))
    uint64_t redo_streams = 0;                      // streams of the last block set that were made again as single streams (their pair-list arena had run out)
    uint64_t container_sets = 0;                    // block sets the last nlzm_hip_compress_blocks* call ran one after another (1: the blocks fitted one launch)
    // the rounds of the block set (blocks_step_impl): two are open at a time, and one may stay queued when a step returns
    struct Rounds {
        bool have = false;                          // round `q` is queued (pre-passes and launch) and not collected yet
        uint32_t q = 0;
        std::vector<StepPlan> plan[2];
        std::vector<uint32_t> act[2];
    } rounds;
    // streaming host input (nlzm_hip_feed_*): two pinned staging buffers on a copy stream of their own
    struct Feed {
        bool open = false, finished = false;               // finished: feed_finish has succeeded (the input is whole in HBM)
        uint64_t n = 0, fed = 0, arrived = 0, taken = 0;    // input bytes handed over / known to be in HBM; output bytes handed back
        uint8_t *pin[2] = { nullptr, nullptr };
        hipEvent_t ev[2] = { nullptr, nullptr };
        uint64_t end_of[2] = { 0, 0 };                      // input offset a staging buffer's last upload ends at
        hipStream_t st = nullptr;
        uint32_t next = 0;
    } feed;
};
constexpr uint64_t kFeedPiece = 32ull << 20;        // bytes per staging buffer
DevState g_dev0;
thread_local DevState *t_dev = nullptr;
inline DevState &cur() { return t_dev ? *t_dev : g_dev0; }
char *thread_err() { return t_dev ? t_dev->err : nullptr; }

// Streams one persistent launch of this device holds, as nlzm_hip_blocks_begin fits them: three stage CUs (and the helper parsers' where
// "block_parser_helper" is on) and one worker CU a stream, 64 at most -- 64 on an MI355X.  0 without a device.
uint32_t blocks_capacity(const DevState &D)
{
    if (!D.ctx.inited) return 0;
    const int64_t roles_live = (int64_t)pipeline2_role_blocks() - (D.opt.block_helper ? 0 : (int64_t)v2::kHelpers);
    const int64_t cap = D.ctx.cu_count / (roles_live + 1);
    return (uint32_t)(cap < 0 ? 0 : cap > 64 ? 64 : cap);
}

void free_stream_buffers(Ctx &C)
{
    for (void *p : C.owned) (void)hipFree(p);
    C.owned.clear();
    C.buf = StreamBuffers{}; C.set[0] = C.set[1] = LaunchSet{}; C.set_idx = 0;
    C.open = false;
}
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
inline bool prefilter_is_bitmap(const Geom &g) { return g.n <= (unsigned long long)g.wmask + 1; }
inline size_t prefilter_bytes(uint32_t t_bits, bool bitmap)
{
    return bitmap ? (((size_t)1 << t_bits) / 8 < 4 ? (size_t)4 : ((size_t)1 << t_bits) / 8) : (size_t)4 << t_bits;
}
// what the per-launch arrays take per chunk of a launch: about 2.3 KB per position
inline double launch_bytes_per_chunk(const Geom &g) { return 2300.0 * g.chunk_size + 8.0 * g.chunk_size * 4; }

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
    if (K.in_set) DEVALLOC(S.snap, sizeof(v2::RoundSnap));
    return 0;
}

// O: the options the stream is opened with (a stream of a block set: block_stream_options)
int stream_begin(Ctx &C, const Options &O, const void *d_src, uint64_t n, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap)
{
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (n >= 0xFFFF0000ull) return set_err(NLZM_HIP_E_TOOBIG, "input of %llu bytes needs >32-bit positions", (unsigned long long)n);
    if (hist_bits_req < 10 || hist_bits_req > 28) return set_err(NLZM_HIP_E_ARG, "hist_bits %u outside [10,28]", hist_bits_req);
    if (dst_cap < 8) return set_err(NLZM_HIP_E_CAPACITY, "dst_cap < 8");
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
        if (room < 1) return set_err(NLZM_HIP_E_ARG, "device has %d CUs: the pipeline needs at least %u", C.cu_count, pipeline2_role_blocks() + 1);
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

    if (!K.in_set) {    // the per-launch arrays take about 2.3 KB per position of a launch: a launch that does not fit is cut down
        // (not for the streams of a block set: blocks_begin fitted their batch to the memory, and the free memory differs between the pass that
        //  measures what a stream takes and the pass that takes it -- the pool itself is allocated in between)
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        const double room = 0.6 * (double)free_b - 4.0 * (double)(1ull << K.t_bits);        // (the pre-filter table: up to 2^33 entries)
        const double per_chunk = launch_bytes_per_chunk(g);
        if (room > per_chunk && (double)K.batch * per_chunk > room) K.batch = (uint32_t)(room / per_chunk);
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
    for (uint32_t s = 0; s < (K.in_set ? 2u : 1u); s++) { const int rc = alloc_launch_set(C, C.set[s]); if (rc) return rc; }

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

// One launch's worth of a stream, in three parts so that several streams can share ONE persistent launch:
//   step_pre   pre-pass kernels and the hand-off arrays of chunks [c0, c1) on the stream's own HIP stream
//   (launch)   pipeline_kernel for this stream alone, or pipeline_multi_kernel for a group of streams
//   step_post  frame coder, frame lengths back to the host, checks, gather into the output
// ahead: the launch before this one may still be on the device (block mode; the other launch set is made the current one, and
// the progress words are set by round_open_kernel on the launch's own HIP stream instead of a copy here)
int step_pre(Ctx &C, uint32_t todo, StepPlan &P, bool ahead = false)
{
    const Geom &g = C.g;
    const StreamConfig &K = C.cfg;
    const StreamBuffers &B = C.buf;
    if (ahead) { if (!K.in_set) return set_err(NLZM_HIP_E_ARG, "no second launch set"); C.set_idx ^= 1; }
    const LaunchSet &L = C.set[C.set_idx];
    const uint32_t c0 = C.pre_chunk, nb = todo < K.batch ? todo : K.batch, c1 = c0 + nb;
    C.pre_chunk = c1;
    P.c0 = c0; P.c1 = c1; P.nb = nb;
    P.set = C.set_idx; P.ahead = ahead;
    hipEvent_t *ev = C.ev[P.set];
    Globals &G = P.G;
    memset(&G, 0, sizeof G);
    G.in = C.d_in; G.rkhash = nullptr; G.ht2 = B.ht2; G.ht3 = B.ht3; G.rk_table = B.rk_table;
    G.bt_heads = B.bt_heads; G.bt_tree = B.bt_tree; G.persist = B.persist;
    G.syms = L.syms; G.syms_stride = K.syms_stride; G.bits = L.bits; G.bits_stride = K.bits_stride;
    G.fmeta = L.fmeta; G.chunk0 = c0;
    G.cap_words = C.cap_words; G.cap_cap = C.cap_cap; G.cap_lo = C.cap_lo; G.cap_hi = C.cap_hi; G.cap_used = C.cap_used;
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
        if (hi > lo && hi - lo > K.rkhash_len) return set_err(NLZM_HIP_E_ARG, "launch of %u chunks is larger than the stream was opened for", nb);
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
            const unsigned long long lpos = (unsigned long long)K.batch * g.chunk_size;
            // (the streams of a block set have a hundred heads to a lane: there a wave pays from positions / 480 on -- 112.6 -> 115.6 MB/s against 8,192)
            const double by_pace = K.in_set ? (double)lpos / 480.0 : (C.last_launch_ms > 0 ? 24.0 * C.last_launch_ms : (double)lpos / 240.0);
            const uint32_t hot_min = K.hot_min > 0 ? K.hot_min : (uint32_t)(by_pace < 512 ? 512 : (by_pace > 1e9 ? 1e9 : by_pace));
            launch_hot_select(L.bin_off, nb, K.nheads, K.hot_max, hot_min, L.hot_of_bin, L.hot_list, B.wcnt, C.st);
            G.hot_of_bin = L.hot_of_bin; G.hot_list = L.hot_list; G.hot_undo = B.hot_undo;
        }
    }
    {   // progress words of the stages: everything before the launch's first position is done
        v2::Hx &h = C.hx_host;          // (lives until the copy has been made)
        memset(&h, 0, sizeof h);
        h.f_pos = h.t_pos = h.t_out = h.p_pos = (uint32_t)a0;
        h.p_seg = ((unsigned long long)(uint32_t)a0 << 32) | (uint32_t)a0;
        if (!ahead) HIPCHK(hipMemcpyAsync(B.v2_hx, &h, sizeof h, hipMemcpyHostToDevice, C.st));
        P.V.ft = B.v2_ft; P.V.tp = B.v2_tp; P.V.tf = B.v2_tf; P.V.hx = B.v2_hx; P.V.state = B.v2_state; P.V.hb = B.v2_hb;
        G.progress = &B.v2_hx->f_pos;
        G.test_fail = K.test_fail_launch >= 0 && (int64_t)C.v2_launch_no == K.test_fail_launch ? 1u : 0u;
        G.table_shape = K.table_shape; G.launch_par = (uint32_t)(C.v2_launch_no++ & 1u);
    }
    HIPCHK(hipEventRecord(ev[kEvPrepEnd], C.st));
    return 0;
}

// pipe_ms: time of the persistent launch when it was not this stream's own (group launch), else < 0
// (in three parts, so that the streams of a block set have their frame coders and gathers in flight together: every part of
//  every stream is queued before the next part waits for any of them)
int step_post_issue(Ctx &C, const StepPlan &P)
{
    const StreamConfig &K = C.cfg;
    const LaunchSet &L = C.set[P.set];
    hipEvent_t *ev = C.ev[P.set];
    const uint32_t nb = P.nb;
    C.post_hm.resize(nb); C.post_hoff.resize(nb);
    C.post_aborted = 0;
    HIPCHK(hipEventRecord(ev[kEvLaunchEnd], C.st));
    launch_rans(L.syms, K.syms_stride, L.bits, K.bits_stride, L.fmeta, C.buf.scratch, K.syms_stride, C.buf.frames,
                K.frame_stride, (uint32_t)K.frame_stride, nb, C.st);
    HIPCHK(hipEventRecord(ev[kEvCoderEnd], C.st));
    HIPCHK(hipMemcpyAsync(C.post_hm.data(), L.fmeta, nb * sizeof(FrameMeta), hipMemcpyDeviceToHost, C.st));
    if (P.ahead) {          // (the stream's next launch may be running: the copy round_close_kernel made)
        HIPCHK(hipMemcpyAsync(&C.post_snap, L.snap, sizeof(v2::RoundSnap), hipMemcpyDeviceToHost, C.st));
        return 0;
    }
    HIPCHK(hipMemcpyAsync(&C.post_P, C.buf.persist, sizeof C.post_P, hipMemcpyDeviceToHost, C.st));
    HIPCHK(hipMemcpyAsync(&C.post_aborted, L.abort_word, 4, hipMemcpyDeviceToHost, C.st));
    HIPCHK(hipMemcpyAsync(&C.hx_host, C.buf.v2_hx, sizeof(v2::Hx), hipMemcpyDeviceToHost, C.st));
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
    if (P.ahead) { C.post_P.error = C.post_snap.error; C.post_P.next_chunk = C.post_snap.next_chunk; C.post_aborted = C.post_snap.aborted; C.hx_host = C.post_snap.hx; }
    const Persist &Pst = C.post_P;
    const uint32_t aborted = C.post_aborted;
    float rk_ms = 0, pre_ms = 0;
    HIPCHK(hipEventElapsedTime(&rk_ms, ev[kEvRkBegin], ev[kEvRkEnd]));
    HIPCHK(hipEventElapsedTime(&pre_ms, ev[kEvRkEnd], ev[kEvPrepEnd]));
    C.tm.prep_ms += rk_ms + pre_ms; C.tm.prep_launches += 5; C.tm.total_ms += rk_ms + pre_ms;
    C.arena_out = false;
    if (Pst.error || C.hx_host.err) {
        // the first error any stage raised, and where every stage was when it left (nlzm_v2.h: raise(), Hx::dbg)
        const v2::Hx &h = C.hx_host;
        WorkerCounters wc{};
        (void)hipMemcpy(&wc, C.buf.wcnt, sizeof wc, hipMemcpyDeviceToHost);
        char where[sizeof g_err];
        stage_error_text(where, sizeof where, h, wc);
        return set_err(NLZM_HIP_E_KERNEL, "device error %u in chunks [%u,%u) (parser stopped at chunk %u): %s", Pst.error ? Pst.error : h.err, c0, c1, Pst.next_chunk, where);
    }
    // (the worker lanes drop a pair that finds no extension block and go on: the cursor says how many blocks were asked for)
    C.arena_out = K.ext_cap && C.hx_host.ext_cur > K.ext_cap;
    if (C.arena_out) return set_err(NLZM_HIP_E_KERNEL, "the extension arena of the BT4 pair lists (%u blocks per launch) was used up in chunks [%u,%u): more positions with over %u "
                                     "record-setters than a block set reserves for", K.ext_cap, c0, c1, K.pstride);
    if (aborted) return set_err(NLZM_HIP_E_KERNEL, "worker lanes aborted (code %u) in chunks [%u,%u)", aborted, c0, c1);
    if (Pst.next_chunk != c1) return set_err(NLZM_HIP_E_KERNEL, "master stopped at chunk %u, expected %u", Pst.next_chunk, c1);
    unsigned long long pos = C.out_pos;
    for (uint32_t f = 0; f < nb; f++) {
        // the reference asserts that the frame fits its buffer (:592, :610); the first one is 4 bytes shorter (:1784)
        const uint32_t room = g.frame_size - ((c0 + f) == 0 ? 4 : 0);
        if (hm[f].out_len > room)
            return set_err(NLZM_HIP_E_KERNEL, "frame %u is %u bytes: the reference would assert (:610)", c0 + f, hm[f].out_len);
        hoff[f] = pos; pos += hm[f].out_len;
    }
    if (pos + 4 > C.dst_cap) return set_err(NLZM_HIP_E_CAPACITY, "dst_cap %llu too small", (unsigned long long)C.dst_cap);
    if (C.want_frame >= (int64_t)c0 && C.want_frame < (int64_t)c1) {
        const uint32_t f = (uint32_t)(C.want_frame - c0);
        C.got_meta = hm[f];
        C.got_syms.resize(hm[f].nsyms); C.got_bits.resize(hm[f].nbits_bytes);
        HIPCHK(hipMemcpy(C.got_syms.data(), L.syms + f * K.syms_stride, hm[f].nsyms * 4ull, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(C.got_bits.data(), L.bits + f * K.bits_stride, hm[f].nbits_bytes, hipMemcpyDeviceToHost));
        C.got = true;
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
    if (pipe_ms < 0) HIPCHK(hipEventElapsedTime(&a, ev[kEvLaunchBegin], ev[kEvLaunchEnd]));
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
int step_post(Ctx &C, const StepPlan &P, float pipe_ms)
{
    int rc = step_post_issue(C, P);
    if (!rc) rc = step_post_check(C, P);
    if (!rc) rc = step_post_done(C, P, pipe_ms);
    return rc;
}

int stream_step(Ctx &C, uint32_t max_chunks, uint64_t *in_done, uint64_t *out_done, int *finished)
{
    if (!C.open) return set_err(NLZM_HIP_E_ARG, "no open stream");
    const Geom &g = C.g;
    uint32_t todo = g.nchunks - C.next_chunk;
    if (max_chunks && todo > max_chunks) todo = max_chunks;
    while (todo) {
        StepPlan P;
        int rc = step_pre(C, todo, P);
        if (rc) return rc;
        HIPCHK(hipEventRecord(C.ev[P.set][kEvLaunchBegin], C.st));
        launch_pipeline2(g, P.G, P.V, P.c0, P.c1, C.cfg.worker_blocks, C.st);
        rc = step_post(C, P, -1.0f);
        if (rc) return rc;
        todo -= P.nb;
    }
    if (in_done) {
        const unsigned long long d = (unsigned long long)C.next_chunk * g.chunk_size;
        *in_done = d < g.n ? d : g.n;
    }
    if (out_done) *out_done = C.out_pos;
    if (finished) *finished = C.next_chunk >= g.nchunks;
    return 0;
}

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

int stream_finish(Ctx &C, uint64_t *dst_len, bool report)
{
    if (!C.open) return set_err(NLZM_HIP_E_ARG, "no open stream");
    if (C.next_chunk < C.g.nchunks) return set_err(NLZM_HIP_E_ARG, "stream not finished (%u of %u chunks)", C.next_chunk, C.g.nchunks);
    if (C.out_pos + 4 > C.dst_cap) return set_err(NLZM_HIP_E_CAPACITY, "dst_cap too small");
    HIPCHK(hipMemsetAsync(C.d_dst + C.out_pos, 0, 4, C.st));        // terminator (:1891-1895)
    C.out_pos += 4;
    HIPCHK(hipStreamSynchronize(C.st));
    const int rc = refresh_stats(C, report);
    if (rc) return rc;
    if (dst_len) *dst_len = C.out_pos;
    return 0;
}

}  // namespace

// ---- what the read side's entry points (nlzm_hip_decode.cpp, nlzm_hip_crc.cpp, nlzm_hip_range.cpp) use of this file's state: the error
// text, the library's stream; what this file uses of theirs is declared in the same header ----
#include "nlzm_host_util.h"
#include "nlzm_container_plan.h"
namespace nlzm {
int host_error(int code, const char *text) { return set_err(code, "%s", text); }
int host_stream(hipStream_t *st)
{
    Ctx &C = cur().ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded (no device: there is no CPU fallback)");
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

static void dev_shutdown(DevState &D);
static void feed_close(DevState &D);
static int dev_init(DevState &D, int device)
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
    if (e != hipSuccess || ndev <= 0) return set_err(NLZM_HIP_E_NODEVICE, "no HIP device (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return set_err(NLZM_HIP_E_ARG, "device %d out of range (%d present)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(NLZM_HIP_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    if (C.inited && C.device == device) return 0;
    if (C.inited) dev_shutdown(D);
    C.device = device;
    C.cu_count = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&C.st, hipStreamNonBlocking));
    for (auto &ev : C.ev[0]) HIPCHK(hipEventCreate(&ev));
    C.inited = true;
    return 0;
}

int nlzm_hip_init(int device) { return dev_init(cur(), device); }

static void dev_shutdown(DevState &D)
{
    Ctx &C = D.ctx;
    if (!C.inited) return;
    blocks_close(D, true);
    feed_close(D);
    free_stream_buffers(C);
    release_own_io(C);
    if (C.cap_words) { (void)hipFree(C.cap_words); C.cap_words = nullptr; }
    if (C.cap_used) { (void)hipFree(C.cap_used); C.cap_used = nullptr; }
    for (auto &ev : C.ev[0]) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (C.st) { (void)hipStreamDestroy(C.st); C.st = nullptr; }
    C.inited = false;
}
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
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if ((!src && n) || !dst || !dst_len) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (n >= 0xFFFF0000ull) return set_err(NLZM_HIP_E_TOOBIG, "input too large");
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
    if (len > dst_cap) return set_err(NLZM_HIP_E_CAPACITY, "stream is %llu bytes, dst_cap %llu", (unsigned long long)len, (unsigned long long)dst_cap);
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
    if (!out) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (C.open) { const int rc = refresh_stats(C, D.opt.report != 0); if (rc) return rc; }
    *out = C.stats;
    return 0;
}

int nlzm_hip_get_counter(const char *key, uint64_t *value)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!key || !value) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (!strncmp(key, "decode_", 7)) return nlzm::decode_counter(key, value);
    if (!strncmp(key, "crc_", 4)) return nlzm::crc_counter(key, value);
    if (!strncmp(key, "range_", 6)) return nlzm::range_counter(key, value);
    if (C.open) { const int rc = refresh_stats(C, D.opt.report != 0); if (rc) return rc; }
    if (compress_counter(key, C.prof_last, C.wc_last, C.stats.positions, value)) return 0;
    if (!strcmp(key, "block_pool_bytes")) { *value = D.blocks_pool_size; return 0; }
    if (!strcmp(key, "block_redo_streams")) { *value = D.redo_streams; return 0; }
    if (!strcmp(key, "container_sets")) { *value = D.container_sets; return 0; }
    if (!strcmp(key, "gpu_max_hw_queues_effective")) { *value = (uint64_t)g_hwq_effective; return 0; }
    return set_err(NLZM_HIP_E_ARG, "unknown counter %s", key);
}

int nlzm_hip_get_timing(nlzm_hip_timing *out)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!out) return set_err(NLZM_HIP_E_ARG, "null argument");
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
    if (!key) return set_err(NLZM_HIP_E_ARG, "null key");
    if (!strcmp(key, "workers")) {      // BT4 always runs on the worker lanes (the three-stage pipeline has no other place for it)
        if (value != 1) return set_err(NLZM_HIP_E_ARG, "workers: only 1 is supported");
        return 0;
    }
    for (const auto &o : kOptions) {
        if (strcmp(key, o.key)) continue;
        const bool ranged = o.kind == kOptRange || o.kind == kOptLanes;
        if (ranged && (value < o.lo || value > o.hi || (o.kind == kOptLanes && value % 64))) return set_err(NLZM_HIP_E_ARG, "%s out of range", key);
        if (o.kind == kOptRing && value != 0 && value != 65536 && value != 16384) return set_err(NLZM_HIP_E_ARG, "%s: 0 (automatic), 65536 or 16384", key);
        if (o.member == &Options::container_set_blocks && D.ctx.inited && value > (int64_t)blocks_capacity(D))
            return set_err(NLZM_HIP_E_ARG, "%s out of range (this device holds %u streams at once)", key, blocks_capacity(D));
        D.opt.*o.member = o.kind == kOptFlag ? (int64_t)(value != 0) : value;
        if (o.member == &Options::keep_pool && !value && D.jobs.empty()) blocks_close(D, true);    // (the allocation a closed set left behind goes at once)
        return 0;
    }
    return set_err(NLZM_HIP_E_ARG, "unknown option %s", key);
}

int nlzm_hip_rans_frames(const uint32_t *syms, const uint64_t *sym_off, const uint8_t *bits, const uint64_t *bits_off,
                         const uint32_t *num_ops, uint32_t nframes, uint8_t *out, uint64_t out_stride, uint32_t *out_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!nframes) return 0;
    if (!syms || !sym_off || !bits || !bits_off || !num_ops || !out || !out_len) return set_err(NLZM_HIP_E_ARG, "null argument");
    uint64_t max_syms = 1, max_bits = 4;
    for (uint32_t f = 0; f < nframes; f++) {
        if (sym_off[f + 1] - sym_off[f] > max_syms) max_syms = sym_off[f + 1] - sym_off[f];
        if (bits_off[f + 1] - bits_off[f] > max_bits) max_bits = bits_off[f + 1] - bits_off[f];
    }
    uint32_t *d_syms = nullptr, *d_scr = nullptr; uint8_t *d_bits = nullptr, *d_out = nullptr; FrameMeta *d_fm = nullptr;
    struct Guard {      // the device buffers go with the call, on every path out
        uint32_t *&a, *&b; uint8_t *&c, *&d; FrameMeta *&e;
        ~Guard() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (c) (void)hipFree(c); if (d) (void)hipFree(d); if (e) (void)hipFree(e); }
    } guard{ d_syms, d_scr, d_bits, d_out, d_fm };
    const unsigned long long fstride = 12 + max_bits + 16 + 2 * max_syms;
    HIPCHK(hipMalloc(&d_syms, nframes * max_syms * 4));
    HIPCHK(hipMalloc(&d_scr, nframes * max_syms * 4));
    HIPCHK(hipMalloc(&d_bits, nframes * max_bits));
    HIPCHK(hipMalloc(&d_out, nframes * fstride));
    HIPCHK(hipMalloc(&d_fm, nframes * sizeof(FrameMeta)));
    std::vector<FrameMeta> hm(nframes);
    for (uint32_t f = 0; f < nframes; f++) {
        const uint64_t ns = sym_off[f + 1] - sym_off[f], nb = bits_off[f + 1] - bits_off[f];
        hm[f].nsyms = (uint32_t)ns; hm[f].nbits_bytes = (uint32_t)nb; hm[f].num_ops = num_ops[f]; hm[f].out_len = 0;
        if (ns) HIPCHK(hipMemcpyAsync(d_syms + f * max_syms, syms + sym_off[f], ns * 4, hipMemcpyHostToDevice, C.st));
        if (nb) HIPCHK(hipMemcpyAsync(d_bits + f * max_bits, bits + bits_off[f], nb, hipMemcpyHostToDevice, C.st));
    }
    HIPCHK(hipMemcpyAsync(d_fm, hm.data(), nframes * sizeof(FrameMeta), hipMemcpyHostToDevice, C.st));
    launch_rans(d_syms, max_syms, d_bits, max_bits, d_fm, d_scr, max_syms, d_out, fstride, (uint32_t)fstride, nframes, C.st);
    HIPCHK(hipMemcpyAsync(hm.data(), d_fm, nframes * sizeof(FrameMeta), hipMemcpyDeviceToHost, C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    HIPCHK(hipGetLastError());
    int rc = 0;
    for (uint32_t f = 0; f < nframes && !rc; f++) {
        out_len[f] = hm[f].out_len;
        if (hm[f].out_len > out_stride) { rc = set_err(NLZM_HIP_E_CAPACITY, "frame %u needs %u bytes", f, hm[f].out_len); break; }
        HIPCHK(hipMemcpy(out + f * out_stride, d_out + f * fstride, hm[f].out_len, hipMemcpyDeviceToHost));
    }
    return rc;
}

int nlzm_hip_find_matches(const uint8_t *src, uint64_t n, uint32_t hist_bits_req, uint64_t pos_lo, uint64_t pos_hi,
                          uint32_t *out_words, uint64_t cap_words, uint64_t *used_words)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!out_words || !used_words) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (C.cap_words) { (void)hipFree(C.cap_words); C.cap_words = nullptr; }
    if (C.cap_used) { (void)hipFree(C.cap_used); C.cap_used = nullptr; }
    HIPCHK(hipMalloc(&C.cap_words, (cap_words + 1) * 4));
    HIPCHK(hipMalloc(&C.cap_used, 8));
    HIPCHK(hipMemset(C.cap_used, 0, 8));
    C.cap_cap = cap_words; C.cap_lo = pos_lo; C.cap_hi = pos_hi;
    const uint64_t bound = nlzm_hip_compress_bound(n);
    std::vector<uint8_t> tmp(bound);
    uint64_t len = 0;
    int rc = nlzm_hip_compress(src, n, hist_bits_req, tmp.data(), bound, &len);
    unsigned long long used = 0;
    if (!rc) {
        HIPCHK(hipMemcpy(&used, C.cap_used, 8, hipMemcpyDeviceToHost));
        // (the table stage's waves finish positions out of order: the records {position, max_len, delta[2..max_len]} are put
        //  into position order here)
        std::vector<uint32_t> raw(used);
        HIPCHK(hipMemcpy(raw.data(), C.cap_words, used * 4, hipMemcpyDeviceToHost));
        std::vector<std::pair<uint32_t, unsigned long long>> recs;      // position, offset
        for (unsigned long long at = 0; at + 2 <= used;) {
            recs.emplace_back(raw[at], at);
            at += 2 + (raw[at + 1] >= 2 ? raw[at + 1] - 1 : 0);
        }
        std::sort(recs.begin(), recs.end());
        unsigned long long o = 0;
        for (const auto &r : recs) {
            const unsigned long long len = 2 + (raw[r.second + 1] >= 2 ? raw[r.second + 1] - 1 : 0);
            memcpy(out_words + o, raw.data() + r.second, len * 4);
            o += len;
        }
        *used_words = used;
    }
    (void)hipFree(C.cap_words); (void)hipFree(C.cap_used);
    C.cap_words = nullptr; C.cap_used = nullptr; C.cap_cap = 0;
    return rc;
}

int nlzm_hip_parse_emit(const uint8_t *src, uint64_t n, uint32_t hist_bits_req, uint32_t frame_idx, uint32_t *syms,
                        uint32_t cap_syms, uint8_t *bits, uint32_t cap_bits, uint32_t *sizes_out)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!syms || !bits || !sizes_out) return set_err(NLZM_HIP_E_ARG, "null argument");
    C.want_frame = frame_idx; C.got = false;
    const uint64_t bound = nlzm_hip_compress_bound(n);
    std::vector<uint8_t> tmp(bound);
    uint64_t len = 0;
    int rc = nlzm_hip_compress(src, n, hist_bits_req, tmp.data(), bound, &len);
    C.want_frame = -1;
    if (rc) return rc;
    if (!C.got) return set_err(NLZM_HIP_E_ARG, "frame %u does not exist", frame_idx);
    if (C.got_meta.nsyms > cap_syms || C.got_meta.nbits_bytes > cap_bits) return set_err(NLZM_HIP_E_CAPACITY, "capture buffers too small");
    memcpy(syms, C.got_syms.data(), C.got_meta.nsyms * 4ull);
    memcpy(bits, C.got_bits.data(), C.got_meta.nbits_bytes);
    sizes_out[0] = C.got_meta.nsyms; sizes_out[1] = C.got_meta.nbits_bytes; sizes_out[2] = C.got_meta.num_ops;
    return 0;
}

}  // extern "C"

// ---- independent blocks --------------------------------------------------------------
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

// "keep_block_pool" keeps a closed set's one allocation (most of the device's memory for the bench's set) for the next set; anything
// else that then cannot allocate -- a single stream, a feed, find_matches -- takes it back here instead of failing with NOMEM.
bool idle_block_pool_dropped()
{
    DevState &D = cur();
    if (!D.jobs.empty() || !D.blocks_pool) return false;
    (void)hipFree(D.blocks_pool);
    D.blocks_pool = nullptr; D.blocks_pool_size = 0;
    return true;
}

void blocks_close(DevState &D, bool drop_pool)
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
    const uint64_t per_fixed = D.blocks_per;        // (a multi-device call fixes the partition; cleared here)
    D.blocks_per = 0;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!nblocks || nblocks > 64) return set_err(NLZM_HIP_E_ARG, "nblocks out of range");
    blocks_close(D);
    // every block is in flight at once: one master CU + its worker CUs per stream, all resident together
    // (a spare CU per stream while there is room for it; every workgroup of the launch has a CU of its own either way:
    //  at most CUs / 4 streams -- three stage CUs and one worker CU each -- which is 64 on an MI355X)
    // (the helper parser's workgroup leaves at once where the streams run without one: it takes no CU then)
    const int64_t roles_live = (int64_t)pipeline2_role_blocks() - (O.block_helper ? 0 : (int64_t)v2::kHelpers);
    int64_t wb = C.cu_count / (int64_t)nblocks - roles_live;
    if (wb > 1 && nblocks > 1) wb--;
    if (wb > O.worker_blocks) wb = O.worker_blocks;
    if (wb < 1) return set_err(NLZM_HIP_E_ARG, "%u streams do not fit %d CUs (at most %d)", nblocks, C.cu_count,
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
        make_geom(per_fixed ? per_fixed : (n + nblocks - 1) / nblocks, hist_bits_req, g0);
        const double fixed = 8.0 * ((double)g0.wmask + 1) * 2 + 5e7;     // BT4 tree (widened), the rest
        double left = per_stream - fixed;
        if (left < 2e8) return set_err(NLZM_HIP_E_NOMEM, "%u streams of %llu bytes at -window:%u do not fit %.1f GB of free memory", nblocks,
                                       (unsigned long long)g0.n, g0.wbits, free_b / 1e9);
        const bool bitmap = prefilter_is_bitmap(g0);
        while (tbits_max > 16 && (double)prefilter_bytes((uint32_t)tbits_max, bitmap) > 0.4 * left) tbits_max--;
        left -= (double)prefilter_bytes(prefilter_tbits(g0, O.tbits_per, tbits_max), bitmap);
        const int64_t fit = (int64_t)(left / launch_bytes_per_chunk(g0));
        if (fit < 1) return set_err(NLZM_HIP_E_NOMEM, "%u streams do not fit the device memory", nblocks);
        if (batch > fit) batch = fit;
    }
    const uint64_t per = per_fixed ? per_fixed : (n + nblocks - 1) / nblocks;     // block i = [i*per, min(n, (i+1)*per))
    D.jobs.resize(nblocks);
    for (uint32_t i = 0; i < nblocks; i++) {
        D.jobs[i].lo = (uint64_t)i * per < n ? (uint64_t)i * per : n;
        const uint64_t hi = (uint64_t)(i + 1) * per < n ? (uint64_t)(i + 1) * per : n;
        D.jobs[i].n = hi - D.jobs[i].lo;
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
            if (hipMalloc(&D.blocks_pool, total) != hipSuccess) { D.blocks_pool = nullptr; blocks_close(D); return set_err(NLZM_HIP_E_NOMEM, "block set: %zu bytes for %u streams", total, nblocks); }
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

static int blocks_step_impl(DevState &D, uint32_t max_chunks_per_block, uint64_t *in_done_total, int *finished, double *device_ms);
int nlzm_hip_blocks_step(uint32_t max_chunks_per_block, uint64_t *in_done_total, int *finished, double *device_ms)
{
    DevState &D = cur();
    if (D.jobs.empty()) return set_err(NLZM_HIP_E_ARG, "no open block set");
    const int rc = blocks_step_impl(D, max_chunks_per_block, in_done_total, finished, device_ms);
    if (rc) {
        // A failed round ends the block set: blocks_close waits for whatever is still queued (every device wait is bounded), then frees
        // every stream's buffers -- the caller's source buffer is not read after this returns.
        char keep[sizeof g_err];
        { std::lock_guard<std::mutex> lk(g_err_mu); memcpy(keep, g_err, sizeof keep); }
        blocks_close(D);
        { std::lock_guard<std::mutex> lk(g_err_mu); memcpy(g_err, keep, sizeof keep); }
    }
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
    if (nj > stream2_pack_capacity()) return set_err(NLZM_HIP_E_ARG, "too many streams for one launch");
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
        for (uint32_t i : act) { const int rc = step_pre(D.jobs[i].c, todo[i], R.plan[q][i], true); if (rc) return rc; }
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
            char first_msg[sizeof g_err] = "";
            std::vector<int> rcs(nj, 0);
            auto note = [&](uint32_t i, int rc) {
                if (rc && !rcs[i]) rcs[i] = rc;
                if (rc && !first_rc) {
                    first_rc = rc;
                    std::lock_guard<std::mutex> lk(g_err_mu);
                    snprintf(first_msg, sizeof first_msg, "block %u: %.*s", i, (int)sizeof first_msg - 32, g_err);
                }
            };
            // (a stream marked `redo` -- a launch of it used its pair-list arena up -- is out of the set's rounds: what is still queued of it runs on
            //  a state that is valid but not the reference's, and nothing of it is looked at; nlzm_hip_blocks_finish makes the stream again)
            for (uint32_t i : R.act[q]) {
                if (D.jobs[i].redo) continue;
                const hipError_t e = hipStreamWaitEvent(D.jobs[i].c.st, D.group_ev[q][2], 0);
                note(i, e == hipSuccess ? step_post_issue(D.jobs[i].c, R.plan[q][i]) : set_err(NLZM_HIP_E_NODEVICE, "hipStreamWaitEvent failed: %s", hipGetErrorString(e)));
            }
            for (uint32_t i : R.act[q]) if (!rcs[i] && !D.jobs[i].redo) {
                Ctx &c = D.jobs[i].c;
                const int rc = step_post_check(c, R.plan[q][i]);
                if (rc && c.arena_out) { D.jobs[i].redo = true; c.next_chunk = c.pre_chunk = c.g.nchunks; continue; }
                note(i, rc);
            }
            for (uint32_t i : R.act[q]) if (!rcs[i] && !D.jobs[i].redo) note(i, step_post_done(D.jobs[i].c, R.plan[q][i], 0.0f));
            if (first_rc) { std::lock_guard<std::mutex> lk(g_err_mu); memcpy(g_err, first_msg, sizeof g_err); return first_rc; }
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

int nlzm_hip_blocks_finish(void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (D.jobs.empty()) return set_err(NLZM_HIP_E_ARG, "no open block set");
    if (!d_dst || !dst_len) return set_err(NLZM_HIP_E_ARG, "null argument");
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
        if (pos + j.len > dst_cap) { rc = set_err(NLZM_HIP_E_CAPACITY, "dst_cap %llu too small", (unsigned long long)dst_cap); break; }
        if (hipMemcpyAsync((uint8_t *)d_dst + pos, j.d_out, j.len, hipMemcpyDeviceToDevice, C.st) != hipSuccess)
            rc = set_err(NLZM_HIP_E_NODEVICE, "gathering block %zu failed", i);
        if (block_len) block_len[i] = j.len;
        pos += j.len;
        uint64_t *dst = (uint64_t *)&C.stats; const uint64_t *src = (const uint64_t *)&j.c.stats;   // counters of the whole job
        for (size_t k = 0; k < sizeof(C.stats) / 8; k++) dst[k] += src[k];
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
    static_assert(sizeof(nlzm_hip_stats) % sizeof(uint64_t) == 0 && alignof(nlzm_hip_stats) == alignof(uint64_t), "nlzm_hip_stats is uint64_t counters and nothing else: they are added up as an array");
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
        uint64_t *to = (uint64_t *)&total; const uint64_t *from = (const uint64_t *)&D.ctx.stats;   // counters of the whole container
        for (size_t k = 0; k < sizeof(total) / 8; k++) to[k] += from[k];
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
    if (!d_dst || !dst_len) return set_err(NLZM_HIP_E_ARG, "null argument");
    container::Plan P;
    char text[256] = "";
    const uint32_t set_blocks = (uint32_t)(D.opt.container_set_blocks < (int64_t)cap ? D.opt.container_set_blocks : (int64_t)cap);
    if (const int rc = container::make_plan(P, n, nblocks, set_blocks, cap, nlzm_hip_compress_bound, ErrText{ text, sizeof text })) return set_err(rc, "%s", text);
    return compress_container(D, P, d_src, hist_bits_req, d_dst, dst_cap, block_len, dst_len);
}

int nlzm_hip_compress_blocks(const uint8_t *src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req, uint8_t *dst,
                             uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if ((!src && n) || !dst || !dst_len || !nblocks) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (nblocks > container::kMaxBlocks) return set_err(NLZM_HIP_E_ARG, "nblocks out of range (1 .. %u)", container::kMaxBlocks);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    const uint64_t bound = nlzm_hip_compress_blocks_bound(n, nblocks);
    HIPCHK(hipMalloc(&d_in, n + 512));
    if (hipMalloc(&d_out, bound) != hipSuccess) { (void)hipFree(d_in); return set_err(NLZM_HIP_E_NOMEM, "output buffer"); }
    if (hipMemset(d_in + n, 0, 512) != hipSuccess || (n && hipMemcpy(d_in, src, n, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(d_in); (void)hipFree(d_out);
        return set_err(NLZM_HIP_E_NODEVICE, "copying the input to the device failed");
    }
    uint64_t len = 0;
    int rc = nlzm_hip_compress_blocks_dev(d_in, n, nblocks, hist_bits_req, d_out, bound, block_len, &len);
    if (!rc && len > dst_cap) rc = set_err(NLZM_HIP_E_CAPACITY, "streams are %llu bytes, dst_cap %llu", (unsigned long long)len, (unsigned long long)dst_cap);
    if (!rc && hipMemcpy(dst, d_out, len, hipMemcpyDeviceToHost) != hipSuccess) rc = set_err(NLZM_HIP_E_NODEVICE, "copy back failed");
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (!rc) *dst_len = len;
    return rc;
}

// ---- streaming host input (the reference reads and writes as it goes: NLZM.cpp:1774-1778, :1853, :1870-1885) ----
// The caller hands the input over in pieces, in order, and takes the stream back in pieces.  A piece goes through one of
// two pinned staging buffers onto a copy stream; while it travels, the chunks whose input has arrived are compressed, so
// host reads, uploads and kernels overlap and the host never holds more than a piece (the input stays whole in HBM:
// matches reach back a window).
static void feed_close(DevState &D)
{
    DevState::Feed &F = D.feed;
    for (int k = 0; k < 2; k++) { if (F.pin[k]) (void)hipHostFree(F.pin[k]); if (F.ev[k]) (void)hipEventDestroy(F.ev[k]); F.pin[k] = nullptr; F.ev[k] = nullptr; }
    if (F.st) (void)hipStreamDestroy(F.st);
    F = DevState::Feed{};
}
// chunks whose input (with the lookahead the launch's kernels read) lies below `arrived`
static uint32_t feed_chunks_ready(const Geom &g, uint64_t arrived)
{
    if (arrived >= g.n) return g.nchunks;
    const uint64_t slack = (uint64_t)g.feed - g.chunk_size + 1024;      // lookahead of the last chunk + RK256 / pre-filter windows
    // (what a launch READS AND USES lies below its last position + slack; its RK256 pre-pass also hashes a little further, into bytes
    //  that may still be arriving -- those hashes are recomputed by the next launch before anything looks at them: step_pre)
    if (arrived < slack + g.chunk_size) return 0;
    return (uint32_t)((arrived - slack) / g.chunk_size);
}
static int feed_run(DevState &D)
{
    Ctx &C = D.ctx;
    const uint32_t ready = feed_chunks_ready(C.g, D.feed.arrived);
    if (ready > C.next_chunk) return stream_step(C, ready - C.next_chunk, nullptr, nullptr, nullptr);
    return 0;
}

int nlzm_hip_feed_begin(uint64_t n, uint32_t hist_bits_req)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return set_err(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (n >= 0xFFFF0000ull) return set_err(NLZM_HIP_E_TOOBIG, "input too large");
    feed_close(D);
    const uint64_t bound = nlzm_hip_compress_bound(n);
    int rc = alloc_own_io(C, n, bound);
    if (rc) return rc;
    rc = stream_begin(C, D.opt, C.own_in, n, hist_bits_req, C.own_dst, bound);
    if (rc) return rc;
    DevState::Feed &F = D.feed;
    rc = [&]() -> int {
        HIPCHK(hipStreamCreateWithFlags(&F.st, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) { HIPCHK(hipHostMalloc((void **)&F.pin[k], kFeedPiece, hipHostMallocDefault)); HIPCHK(hipEventCreate(&F.ev[k])); }
        return 0;
    }();
    if (rc) { feed_close(D); return rc; }
    F.open = true; F.n = n;
    return 0;
}

int nlzm_hip_feed(const uint8_t *piece, uint64_t len)
{
    DevState &D = cur();
    DevState::Feed &F = D.feed;
    if (!F.open) return set_err(NLZM_HIP_E_ARG, "no open feed");
    if ((!piece && len) || F.fed + len > F.n) return set_err(NLZM_HIP_E_ARG, "feed of %llu bytes at %llu exceeds the %llu announced", (unsigned long long)len,
                                                             (unsigned long long)F.fed, (unsigned long long)F.n);
    while (len) {
        const uint32_t k = F.next;
        const uint64_t m = len < kFeedPiece ? len : kFeedPiece;
        // the staging buffer is free once its last upload has landed; what landed is input the kernels may read
        HIPCHK(hipEventSynchronize(F.ev[k]));
        if (F.end_of[k] > F.arrived) F.arrived = F.end_of[k];
        memcpy(F.pin[k], piece, m);
        HIPCHK(hipMemcpyAsync(D.ctx.own_in + F.fed, F.pin[k], m, hipMemcpyHostToDevice, F.st));
        HIPCHK(hipEventRecord(F.ev[k], F.st));
        F.fed += m; F.end_of[k] = F.fed; F.next = k ^ 1u;
        piece += m; len -= m;
        // (this piece is on its way: meanwhile, the chunks whose input is there)
        const int rc = feed_run(D);
        if (rc) { feed_close(D); return rc; }
    }
    return 0;
}

// the bytes of the stream produced since the last call (whole frames); *len = 0: nothing new
int nlzm_hip_feed_output(uint8_t *dst, uint64_t cap, uint64_t *len)
{
    DevState &D = cur();
    DevState::Feed &F = D.feed;
    if (!F.open) return set_err(NLZM_HIP_E_ARG, "no open feed");
    if (!dst || !len) return set_err(NLZM_HIP_E_ARG, "null argument");
    const uint64_t have = D.ctx.out_pos - F.taken, m = have < cap ? have : cap;
    if (m) HIPCHK(hipMemcpy(dst, D.ctx.own_dst + F.taken, m, hipMemcpyDeviceToHost));
    F.taken += m;
    *len = m;
    return 0;
}

// after the last piece: the remaining chunks and the terminator; then nlzm_hip_feed_output until it returns 0 bytes, then
// nlzm_hip_feed_end
int nlzm_hip_feed_finish(void)
{
    DevState &D = cur();
    DevState::Feed &F = D.feed;
    if (!F.open) return set_err(NLZM_HIP_E_ARG, "no open feed");
    if (F.fed != F.n) { const unsigned long long a = F.fed, b = F.n; feed_close(D); return set_err(NLZM_HIP_E_ARG, "%llu of %llu input bytes were fed", a, b); }
    HIPCHK(hipStreamSynchronize(F.st));
    F.arrived = F.n;
    int rc = feed_run(D);
    if (!rc) { uint64_t total = 0; rc = stream_finish(D.ctx, &total, D.opt.report != 0); }
    if (rc) feed_close(D);
    else F.finished = true;
    return rc;
}
// between feed_finish and feed_end: the CRC32 of the input that was fed, hashed where it lies (nlzm_hip_crc.cpp)
int nlzm_hip_feed_input_crc32(uint32_t *crc)
{
    DevState &D = cur();
    DevState::Feed &F = D.feed;
    if (!F.open || !F.finished) return set_err(NLZM_HIP_E_ARG, "no finished feed (nlzm_hip_feed_input_crc32 goes between feed_finish and feed_end)");
    if (!crc) return set_err(NLZM_HIP_E_ARG, "null argument");
    nlzm::crc_begin_call();
    const uint64_t off = 0, n = F.n;
    return nlzm::crc_ranges_on(D.ctx.st, D.ctx.own_in, n, 1, &off, &n, 0, crc);
}
void nlzm_hip_feed_end(void) { feed_close(cur()); }

// ---- independent blocks on several GPUs of one node -------------------------------------------------
// One host thread and one device state per GPU; device i compresses blocks [i*m, (i+1)*m) of the n-byte input's partition into
// ndev*m blocks (the same byte ranges nlzm_hip_compress_blocks uses for that many blocks) in block mode; there is no traffic
// between the GPUs while they compress.  The only exchange is the final gather of the streams onto the first device of the
// list, GPU to GPU (hipMemcpyPeerAsync: over xGMI where the devices are linked), from where the artifact goes to the host.
int nlzm_hip_compress_blocks_multi(const int *devices, uint32_t ndev, uint32_t blocks_per_dev, const uint8_t *src, uint64_t n,
                                   uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (!devices || !ndev || !blocks_per_dev || (!src && n) || !dst || !dst_len) return set_err(NLZM_HIP_E_ARG, "null argument");
    if (ndev > 64) return set_err(NLZM_HIP_E_ARG, "more than 64 devices");
    if (!g_dev0.opt.multi_same)
        for (uint32_t i = 0; i < ndev; i++)
            for (uint32_t k = 0; k < i; k++)
                if (devices[i] == devices[k]) return set_err(NLZM_HIP_E_ARG, "device %d is listed twice", devices[i]);
    const uint64_t nb_total = (uint64_t)ndev * blocks_per_dev;
    const uint64_t per = n ? (n + nb_total - 1) / nb_total : 1;
    struct Part {
        DevState D;
        int device = 0, rc = 0;
        uint64_t lo = 0, n = 0, bound = 0, len = 0;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        std::vector<uint64_t> blens;
        char msg[sizeof g_err] = "";
        bool pinned = false, direct = false;
        double h2d_ms = 0, run_ms = 0, gather_ms = 0;
    };
    std::vector<Part> parts(ndev);
    int dev_before = -1;
    (void)hipGetDevice(&dev_before);                // (the caller's current device is put back on the way out)
    // the caller's pages pinned for the uploads when the driver allows it (a pageable copy goes through a bounce buffer): the whole
    // range once, page-aligned, before the threads start -- their parts share pages
    bool pinned_all = false;
    uint8_t *pin_lo = nullptr; size_t pin_len = 0;
    if (n) {
        const uintptr_t pg = 4096, lo = (uintptr_t)src & ~(pg - 1), hi = ((uintptr_t)src + n + pg - 1) & ~(pg - 1);
        pin_lo = (uint8_t *)lo; pin_len = (size_t)(hi - lo);
        pinned_all = hipHostRegister(pin_lo, pin_len, hipHostRegisterPortable) == hipSuccess;
        if (!pinned_all) (void)hipGetLastError();
    }
    auto run_part = [&](uint32_t i) {
        Part &P = parts[i];
        t_dev = &P.D;
        P.device = devices[i];
        P.lo = (uint64_t)i * blocks_per_dev * per < n ? (uint64_t)i * blocks_per_dev * per : n;
        const uint64_t hi = (uint64_t)(i + 1) * blocks_per_dev * per < n ? (uint64_t)(i + 1) * blocks_per_dev * per : n;
        P.n = hi - P.lo;
        P.bound = nlzm_hip_compress_bound(P.n) + (uint64_t)blocks_per_dev * (16 + 131072);
        P.blens.assign(blocks_per_dev, 0);
        P.rc = [&]() -> int {
            int rc = dev_init(P.D, P.device);
            if (rc) return rc;
            {   // the options set through nlzm_hip_set_option hold for every device of the call -- but for the test-only knobs and what is the process's own
                const Options dflt;
                Options &o = P.D.opt;
                o = g_dev0.opt;
                o.test_fail_launch = dflt.test_fail_launch; o.test_fail_stream = dflt.test_fail_stream; o.block_ext_blocks = dflt.block_ext_blocks; o.multi_same = dflt.multi_same; o.keep_pool = dflt.keep_pool;
            }
            HIPCHK(hipMalloc(&P.d_in, P.n + 512));
            HIPCHK(hipMalloc(&P.d_out, P.bound));
            HIPCHK(hipMemset(P.d_in + P.n, 0, 512));
            const auto t0 = std::chrono::steady_clock::now();
            P.pinned = pinned_all;
            if (P.n) HIPCHK(hipMemcpy(P.d_in, src + P.lo, P.n, hipMemcpyHostToDevice));
            const auto t1 = std::chrono::steady_clock::now();
            P.D.blocks_per = per;
            rc = nlzm_hip_compress_blocks_dev(P.d_in, P.n, blocks_per_dev, hist_bits_req, P.d_out, P.bound, P.blens.data(), &P.len);
            P.h2d_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            P.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            return rc;
        }();
        if (P.rc) snprintf(P.msg, sizeof P.msg, "device %d: %.*s", P.device, (int)sizeof P.msg - 32, P.D.err);      // (this thread's own text)
        t_dev = nullptr;
    };
    {
        std::vector<std::thread> th;
        for (uint32_t i = 0; i < ndev; i++) th.emplace_back(run_part, i);
        for (auto &t : th) t.join();
    }
    if (pinned_all) (void)hipHostUnregister(pin_lo);
    int rc = 0;
    uint64_t total = 0;
    for (auto &P : parts) { if (P.rc && !rc) { rc = P.rc; std::lock_guard<std::mutex> lk(g_err_mu); memcpy(g_err, P.msg, sizeof g_err); } total += P.len; }
    if (!rc && total > dst_cap) rc = set_err(NLZM_HIP_E_CAPACITY, "streams are %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
    if (!rc) {
        // the gather: every device's streams onto the first one, in block order, then one copy to the host
        const int root = parts[0].device;
        uint8_t *d_all = nullptr;
        rc = [&]() -> int {
            HIPCHK(hipSetDevice(root));
            if (ndev == 1) { HIPCHK(hipMemcpy(dst, parts[0].d_out, total, hipMemcpyDeviceToHost)); return 0; }
            HIPCHK(hipMalloc(&d_all, total ? total : 1));
            // GPU to GPU: directly over the link where the root may address the device's memory (xGMI inside a node), else staged by the
            // runtime; which it was is reported.  Every copy is queued before any is waited for; events on the root's stream time them.
            std::vector<hipEvent_t> ev(2 * parts.size(), nullptr);
            std::vector<int> enabled_here;
            uint64_t off = 0;
            int grc = 0;
            for (size_t k = 0; k < parts.size() && !grc; k++) {
                Part &P = parts[k];
                if (P.device != root) {
                    int can = 0;
                    if (hipDeviceCanAccessPeer(&can, root, P.device) == hipSuccess && can) {
                        const hipError_t e = hipDeviceEnablePeerAccess(P.device, 0);
                        P.direct = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
                        if (e == hipSuccess) enabled_here.push_back(P.device);
                        (void)hipGetLastError();
                    }
                } else P.direct = true;
                if (hipEventCreate(&ev[2 * k]) != hipSuccess || hipEventCreate(&ev[2 * k + 1]) != hipSuccess) { grc = set_err(NLZM_HIP_E_NODEVICE, "hipEventCreate failed"); break; }
                (void)hipEventRecord(ev[2 * k], nullptr);
                if (P.len && hipMemcpyPeerAsync(d_all + off, root, P.d_out, P.device, P.len, nullptr) != hipSuccess)
                    grc = set_err(NLZM_HIP_E_NODEVICE, "gather from device %d failed: %s", P.device, hipGetErrorString(hipGetLastError()));
                (void)hipEventRecord(ev[2 * k + 1], nullptr);
                off += P.len;
            }
            if (!grc && hipDeviceSynchronize() != hipSuccess) grc = set_err(NLZM_HIP_E_NODEVICE, "gather failed: %s", hipGetErrorString(hipGetLastError()));
            for (size_t k = 0; k < parts.size(); k++) {
                float ms = 0;
                if (!grc && ev[2 * k] && ev[2 * k + 1] && hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) == hipSuccess) parts[k].gather_ms = ms;
                if (ev[2 * k]) (void)hipEventDestroy(ev[2 * k]);
                if (ev[2 * k + 1]) (void)hipEventDestroy(ev[2 * k + 1]);
            }
            for (int d : enabled_here) (void)hipDeviceDisablePeerAccess(d);     // (only what this call enabled: the caller's settings stay)
            if (grc) return grc;
            HIPCHK(hipMemcpy(dst, d_all, total, hipMemcpyDeviceToHost));
            return 0;
        }();
        if (d_all) (void)hipFree(d_all);
        if (!rc) {
            if (block_len) for (uint32_t i = 0; i < ndev; i++) for (uint32_t k = 0; k < blocks_per_dev; k++) block_len[(uint64_t)i * blocks_per_dev + k] = parts[i].blens[k];
            *dst_len = total;
        }
    }
    // the job's counters (nlzm_hip_get_stats of the process-wide context reports them) and the clean-up, device by device
    memset(&g_dev0.ctx.stats, 0, sizeof g_dev0.ctx.stats);
    for (auto &P : parts) {
        uint64_t *d = (uint64_t *)&g_dev0.ctx.stats; const uint64_t *q = (const uint64_t *)&P.D.ctx.stats;
        for (size_t k = 0; k < sizeof(nlzm_hip_stats) / 8; k++) d[k] += q[k];
        (void)hipSetDevice(P.device);
        if (P.d_in) (void)hipFree(P.d_in);
        if (P.d_out) (void)hipFree(P.d_out);
        dev_shutdown(P.D);
    }
    if (g_dev0.opt.report)
        for (auto &P : parts)
            fprintf(stderr, "device %d: %llu bytes in %u blocks -- upload %.1f ms (%s), compress %.1f ms, gather %.1f ms (%s), %llu bytes out\n", P.device,
                    (unsigned long long)P.n, blocks_per_dev, P.h2d_ms, P.pinned ? "pinned" : "pageable", P.run_ms, P.gather_ms,
                    P.device == parts[0].device ? "local" : (P.direct ? "peer access" : "staged by the runtime"), (unsigned long long)P.len);
    if (dev_before >= 0) (void)hipSetDevice(dev_before);
    return rc;
}

}  // extern "C"
