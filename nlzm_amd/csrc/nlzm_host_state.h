// nlzm_host_state.h -- what the compress side's host files share (nlzm_hip.cpp, nlzm_hip_blocks.cpp, nlzm_hip_multi.cpp, nlzm_hip_feed.cpp,
// nlzm_hip_stage.cpp; nothing else includes this): the state they keep per device -- options, the stream context, the open block set, the
// feed -- and THE prototypes of what crosses a file boundary between them.  The error and buffer scaffolding is the read side's too:
// nlzm_host_util.h (fail, HIPCHK, DevBuf, Events).
#pragma once

#include "nlzm_host_util.h"

#include <array>
#include <vector>

#include "nlzm_core.h"
#include "nlzm_v2.h"

namespace nlzm {
namespace host {

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
    uint32_t depth = 1;                     // launch sets: 2 -- the pre-pass and the launch of k + 1 are queued before launch k is collected (a block set's streams always;
                                            // a single stream where a second set fits the device: nlzm_stream_plan.h)
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

// Everything that exists once per launch set: what a pre-pass writes or a frame coder reads.  Launch k + 1 is queued (and its pre-pass runs) while
// launch k is on the device, and the frames of launch k are coded while launch k + 1 is: a stream has two (StreamConfig::depth; a single stream
// on a device too small for the second has one, and collects every launch before it queues the next), and a pre-pass makes the other one the
// current one (Ctx::set_idx).
struct LaunchSet {
    uint32_t *rkhash = nullptr, *bt_ready = nullptr, *bt_flag = nullptr, *abort_word = nullptr, *bin_off = nullptr, *bin_pos = nullptr,
             *hot_of_bin = nullptr, *hot_list = nullptr, *syms = nullptr;
    uint8_t *unc = nullptr, *bits = nullptr;
    FrameMeta *fmeta = nullptr;
    v2::RoundSnap *snap = nullptr;          // what round_close_kernel copies aside for the host
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
enum { kEvLaunchEnd /* = frame coder begin */, kEvCoderEnd, kEvGatherBegin, kEvGatherEnd, kEvRkBegin, kEvRkEnd /* = rest of the pre-pass begin */, kEvPrepEnd,
       kEvCallBegin, kEvCallEnd, kEvN };

// Stage tests only: what nlzm_hip_find_matches and nlzm_hip_parse_emit (nlzm_hip_stage.cpp) set before they run a stream, and dev_shutdown frees.
// step_pre hands cap_* to the kernels (Globals), step_post_check copies frame `want_frame` aside.
struct StageCapture {
    uint32_t *cap_words = nullptr; unsigned long long cap_cap = 0, cap_lo = 0, cap_hi = 0; unsigned long long *cap_used = nullptr;
    // frame capture for parse_emit
    int64_t want_frame = -1;
    std::vector<uint32_t> got_syms; std::vector<uint8_t> got_bits; FrameMeta got_meta{};
    bool got = false;
};
struct Ctx {
    bool inited = false;
    int device = 0, cu_count = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[2][kEvN] = {};             // per launch set
    // a single stream's persistent launches: a HIP stream of higher priority than `st`, i.e. a hardware queue apart from the pre-passes and frame coders
    // that run beside them on `st`; per launch set the events launch begins / ends / its results are copied aside, and the launch's arguments as
    // round_open_kernel and round_close_kernel read them: a pack of one entry in pinned host memory (made by stream_begin when first needed)
    hipStream_t launch_st = nullptr;
    hipEvent_t launch_ev[2][3] = {};
    void *launch_pack = nullptr;
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

    StageCapture stage;                     // (stage tests)

    // run state: what the step's frame coder has reported (step_post_issue .. _done), what round_close_kernel copied aside of the launch (the progress
    // words among it), timing.  Asynchronous copies write these: they stay where they are while the stream is open.
    std::vector<FrameMeta> post_hm; std::vector<unsigned long long> post_hoff; unsigned long long post_pos = 0;
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

bool idle_block_pool_dropped();                    // nlzm_hip_blocks.cpp: no block set open and its kept allocation still there: frees it, true

// a device buffer of the stream: from its pool, or from hipMalloc (then the stream owns it)
template <class T> int dev_alloc(Ctx &C, T **p, size_t bytes)
{
    if (!C.pool) {
        hipError_t e = hipMalloc((void **)p, bytes);
        if (e == hipErrorOutOfMemory && idle_block_pool_dropped()) {    // (the allocation a closed block set left behind: given back, once, for this one)
            (void)hipGetLastError();
            e = hipMalloc((void **)p, bytes);
        }
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? NLZM_HIP_E_NOMEM : NLZM_HIP_E_NODEVICE, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        C.owned.push_back(*p);
        return 0;
    }
    Pool &P = *C.pool;
    const size_t at = (P.used + 255) & ~(size_t)255;
    if (!P.measuring && at + bytes > P.size) return fail(NLZM_HIP_E_NOMEM, "stream pool of %zu bytes is too small", P.size);
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
    char err[kErrText] = "";                        // the last error raised by a thread that works for this state
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
    const uint64_t *blocks_off = nullptr, *blocks_len = nullptr;   // the next set's blocks as ranges of the caller's choosing, one entry per block (nlzm_hip_compress_ranges*; read and cleared by nlzm_hip_blocks_begin)
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
extern DevState g_dev0;                             // nlzm_hip.cpp
extern thread_local DevState *t_dev;
inline DevState &cur() { return t_dev ? *t_dev : g_dev0; }

// counters of a whole job: one stream's, set's or device's added to the total
static_assert(sizeof(nlzm_hip_stats) % sizeof(uint64_t) == 0 && alignof(nlzm_hip_stats) == alignof(uint64_t), "nlzm_hip_stats is uint64_t counters and nothing else: they are added up as an array");
inline void add_stats(nlzm_hip_stats &to, const nlzm_hip_stats &from)
{
    uint64_t *d = (uint64_t *)&to; const uint64_t *s = (const uint64_t *)&from;
    for (size_t k = 0; k < sizeof(nlzm_hip_stats) / sizeof(uint64_t); k++) d[k] += s[k];
}

// nlzm_hip.cpp keeps the error text, its lock and the per-thread copies to itself.  The one way to put a prefix in front of a text:
// out = "<prefix><text>", the text cut to kErrText - 32 bytes (the prefix is shorter than that); text nullptr: the library's current text,
// read under its lock ...
void error_prefixed(char (&out)[kErrText], const char *text, const char *prefix_fmt, ...);
// ... and such a text made the library's current one (the process-wide text alone: a thread's own copy stays as it is)
void error_replace(const char (&text)[kErrText]);

// nlzm_hip.cpp: the device, geometry, the single stream
int dev_init(DevState &D, int device);
void dev_shutdown(DevState &D);
void make_geom(uint64_t n, uint32_t hist_bits_req, Geom &g);
uint32_t prefilter_tbits(const Geom &g, int64_t tbits_per, int64_t tbits_max);
bool prefilter_is_bitmap(const Geom &g);
size_t prefilter_bytes(uint32_t t_bits, bool bitmap);
double launch_bytes_per_chunk(const Geom &g);
int stream_begin(Ctx &C, const Options &O, const void *d_src, uint64_t n, uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap);
int step_pre(Ctx &C, uint32_t todo, StepPlan &P);
int step_post_issue(Ctx &C, const StepPlan &P);
int step_post_check(Ctx &C, const StepPlan &P);
int step_post_done(Ctx &C, const StepPlan &P, float pipe_ms);
int stream_step(Ctx &C, uint32_t max_chunks, uint64_t *in_done, uint64_t *out_done, int *finished);
int stream_finish(Ctx &C, uint64_t *dst_len, bool report);
void free_stream_buffers(Ctx &C);
void release_launch_stream(Ctx &C);
int alloc_own_io(Ctx &C, uint64_t n, uint64_t bound);
void release_own_io(Ctx &C);
// nlzm_hip_blocks.cpp
void blocks_close(DevState &D, bool drop_pool = false);
uint32_t blocks_capacity(const DevState &D);
// nlzm_hip_feed.cpp
void feed_close(DevState &D);

}  // namespace host
}  // namespace nlzm
