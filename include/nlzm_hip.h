/*
 * nlzm_hip.h -- C ABI of the MI355X (gfx950) implementation of NLZM 1.03's
 * compress-side hot path.
 *
 * The reference has no library/FFI surface: its only seam for this path is
 *
 *     void encode_file(FILE *fin, FILE *fout, uint32 hist_bits)      NLZM.cpp:1711
 *
 * called from main() (NLZM.cpp:2114).  nlzm_hip_compress() replaces the body of
 * that function -- everything between the first fread (NLZM.cpp:1774) and the
 * terminator fwrite (NLZM.cpp:1895) -- and produces the same bytes.  The
 * stage-level entry points below expose the same work split at the reference's
 * internal function boundaries so each stage can be checked on its own.
 *
 * Conventions: plain C types only; `const uint8_t *` host buffers are owned by
 * the caller; `void *d_*` arguments are device (HBM) pointers owned by the
 * caller; every function returns 0 on success or a negative NLZM_HIP_E_* code
 * (never exit()s, unlike the reference's ASSERT, NLZM.cpp:25);
 * nlzm_hip_last_error() gives a message.  One context per process and device;
 * calls are not re-entrant (the reference is single-threaded too).
 */
#ifndef NLZM_HIP_H
#define NLZM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLZM_HIP_E_ARG        (-1)   /* bad argument                                   */
#define NLZM_HIP_E_NODEVICE   (-2)   /* no usable gfx950 device / HIP runtime error    */
#define NLZM_HIP_E_NOMEM      (-3)   /* device allocation failed                       */
#define NLZM_HIP_E_CAPACITY   (-4)   /* dst_cap too small                              */
#define NLZM_HIP_E_KERNEL     (-5)   /* kernel reported an internal error / timeout    */
#define NLZM_HIP_E_TOOBIG     (-6)   /* input >= 2^32-2^16 bytes (32-bit positions)    */
#define NLZM_HIP_E_FORMAT     (-7)   /* not an NLZM stream / malformed / cut off       */

/* Operation counters: same definitions as SURVEY.md section 8d (algorithmic bytes). */
typedef struct nlzm_hip_stats {
    uint64_t in_bytes, out_bytes;
    uint64_t bt_calls, bt_tests, cmp_bytes, ht_rows, rk_probes, rk_inserts;
    uint64_t positions, nice_positions, segments;
    uint64_t n_literal, n_dict, n_rep, rans_syms, bit_ops, frames, shifts;
    uint64_t uncertain_positions;     /* positions whose finder set needed the master's decision */
} nlzm_hip_stats;

/* Device-side timings of the last nlzm_hip_compress*() call (HIP events on the
 * library's own stream), in milliseconds. */
typedef struct nlzm_hip_timing {
    double total_ms;        /* first launch .. last launch complete                 */
    double h2d_ms, d2h_ms;  /* copies (0 for the *_dev entry point)                 */
    double prep_ms;         /* position-parallel pre-pass kernels                   */
    double match_parse_ms;  /* the persistent match-find + parse + emit kernel(s)   */
    double rans_ms;         /* frame rANS kernel(s)                                 */
    uint32_t match_parse_launches, rans_launches, prep_launches;
} nlzm_hip_timing;

/* ---- lifetime ------------------------------------------------------------ */

/* Select the device and create the library's stream.  Fails (NLZM_HIP_E_NODEVICE)
 * when there is no GPU: there is no CPU fallback behind this ABI. */
/* The process's FIRST nlzm_hip_init sets GPU_MAX_HW_QUEUES=16 in the process environment -- once, and only if the caller has not set it and the
 * process does not have the GPU open yet (block mode runs the small kernels of 32 streams beside one persistent launch; with the HIP runtime's
 * default of 4 hardware queues they serialise: ~70 instead of ~100 MB/s).  The runtime reads the variable at the process's FIRST HIP call: a host
 * program that uses HIP before nlzm_hip_init must export it itself.  nlzm_hip_get_counter("gpu_max_hw_queues_effective") says what the runtime
 * has read: the caller's value, 16, or 4 when it was too late. */
int nlzm_hip_init(int device);
void nlzm_hip_shutdown(void);
const char *nlzm_hip_last_error(void);

/* Upper bound on the stream size for n input bytes (every frame fits a 128 KiB
 * buffer in the reference: NLZM.cpp:1722-1724, 1738). */
uint64_t nlzm_hip_compress_bound(uint64_t n);

/* Window/frame geometry the stream will use for a file of flen bytes when
 * `-window:hist_bits_req` was asked (auto-shrink NLZM.cpp:1716-1718, frame sizes
 * NLZM.cpp:1722-1725). */
void nlzm_hip_geometry(uint64_t flen, uint32_t hist_bits_req, uint32_t *hist_bits,
                       uint32_t *frame_bits, uint32_t *chunk_size, uint32_t *feed_size);

/* ---- whole path: replaces encode_file (NLZM.cpp:1711-1910) ---------------- */

/* src/dst are host buffers.  hist_bits_req is the value after the CLI clamp to
 * [15,28] (NLZM.cpp:2085).  *dst_len receives header + frames + terminator. */
int nlzm_hip_compress(const uint8_t *src, uint64_t n, uint32_t hist_bits_req,
                      uint8_t *dst, uint64_t dst_cap, uint64_t *dst_len);

/* Same, but input and output already live in HBM (d_src must be followed by at
 * least 128 readable padding bytes).  Used by bench.py so the timed region starts
 * with the input resident. */
int nlzm_hip_compress_dev(const void *d_src, uint64_t n, uint32_t hist_bits_req,
                          void *d_dst, uint64_t dst_cap, uint64_t *dst_len);

/* Incremental form of the same call, for time-boxed runs: begin binds the input,
 * each step compresses the next `max_chunks` chunks (one chunk = one frame's
 * worth of input, NLZM.cpp:1724), finish appends the terminator.  The bytes
 * produced are identical to the one-shot call. */
int nlzm_hip_stream_begin(const void *d_src, uint64_t n, uint32_t hist_bits_req,
                          void *d_dst, uint64_t dst_cap);
int nlzm_hip_stream_step(uint32_t max_chunks, uint64_t *in_done, uint64_t *out_done, int *finished);
int nlzm_hip_stream_finish(uint64_t *dst_len);

int nlzm_hip_get_stats(nlzm_hip_stats *out);
int nlzm_hip_get_timing(nlzm_hip_timing *out);
/* Diagnostic counters of the pipeline stages for the last stream (what "stage_report" prints, by name; also "block_pool_bytes", "block_redo_streams",
 * "container_sets", "gpu_max_hw_queues_effective"): cycles are summed over the
 * stream's launches, e.g. "parser_total_cycles", "parser_wait_cycles", "parser_pass_cycles", "parser_passes", "parser_blocks",
 * "finder_total_cycles", "finder_wait_cycles", "finder_bt_wait_cycles", "table_total_cycles", "table_wait_cycles", "helper_jobs",
 * "helper_taken", "helper_taken_nodes", "helper_wait_cycles", "worker_call_cycles", "worker_call_tests", "worker_calls",
 * "hot_bin_calls", "positions".  No reference counterpart (the reference prints a progress line, NLZM.cpp:1861-1864); bench.py's
 * latency bound and the tests read them. */
int nlzm_hip_get_counter(const char *key, uint64_t *value);

/* ---- stage: frame coder, replaces CodeFrame::Flush (NLZM.cpp:590-640) ------ */

/* For each frame f: syms[sym_off[f] .. sym_off[f+1]) are the (freq<<16)+start
 * words buffered by WriteRange (NLZM.cpp:565); bits[bits_off[f] .. bits_off[f+1])
 * are the raw-bit bytes INCLUDING the four pad bytes Flush appends
 * (NLZM.cpp:591-597); num_ops[f] is the op count.  Frame f is written to
 * out + f*out_stride and its length to out_len[f].  Host pointers. */
int nlzm_hip_rans_frames(const uint32_t *syms, const uint64_t *sym_off,
                         const uint8_t *bits, const uint64_t *bits_off,
                         const uint32_t *num_ops, uint32_t nframes,
                         uint8_t *out, uint64_t out_stride, uint32_t *out_len);

/* ---- stage: match finding, replaces the finder block of parse_table -------- */
/* (NLZM.cpp:1501-1543: carry + HT2/HT3/BT4/RK256 -> the table copied to mt_carry)
 *
 * Runs the whole path on src but returns, for positions [pos_lo, pos_hi), the
 * per-position match tables as records {pos, max_len, delta[2..max_len]} of
 * uint32 words (same record format as the oracle's capture).  Host pointers. */
int nlzm_hip_find_matches(const uint8_t *src, uint64_t n, uint32_t hist_bits_req,
                          uint64_t pos_lo, uint64_t pos_hi,
                          uint32_t *out_words, uint64_t cap_words, uint64_t *used_words);

/* ---- stage: parse + emit, replaces parse_table's relaxations and the -------- */
/* model_encode_* calls of the driver loop (NLZM.cpp:1545-1650, 1809-1843)
 *
 * Returns the symbol/bit streams of frame `frame_idx` before rANS coding:
 * sizes_out = {nsyms, nbits_bytes (incl. pad), num_ops}.  Host pointers. */
int nlzm_hip_parse_emit(const uint8_t *src, uint64_t n, uint32_t hist_bits_req,
                        uint32_t frame_idx, uint32_t *syms, uint32_t cap_syms,
                        uint8_t *bits, uint32_t cap_bits, uint32_t *sizes_out);

/* ---- independent blocks (the path's only shard axis) ---- */
/* The reference has no block mode: k blocks = k runs of encode_file (NLZM.cpp:1711) on the byte ranges
 * [i*ceil(n/k), min(n, (i+1)*ceil(n/k))), each with its own header, window, model and terminator; the streams are
 * self-delimiting (frame headers carry sizes, :645-663; terminator :646-648) and are written back to back in block
 * order.  On one GPU all k streams are in flight at once, in one persistent launch per round: a stream needs three CUs for
 * the stages of its serial half and at least one CU of BT4 worker lanes, so k <= CUs / 4 (64 on an MI355X; the CUs left
 * are divided among the streams); an MI355X does best with 32 to 40.  d_src needs 128 readable bytes behind it (the host-buffer entry points allocate 512).
 * begin binds the input and allocates every stream's state, each step advances every stream by max_chunks chunks
 * (0: to its end), finish appends the terminators and concatenates into d_dst.  The launches of consecutive rounds are
 * queued back to back (the pre-pass kernels of the next round and the frame coder of the round before run beside a launch,
 * out of two sets of per-launch buffers), and a step that has delivered its max_chunks leaves the NEXT round of the same
 * size queued on the device for the next step to collect, so that the device does not idle between the calls: in_done_total
 * counts what has been collected (a step whose max_chunks is SMALLER than the step's before it still collects the round that one
 * left queued, i.e. more than it asked for: max_chunks bounds what a step starts, not what it finds started).  d_src and the set's
 * device buffers are therefore read and written between the calls too: the input must not change until finish or abandon.
 * A begin or step that fails has closed
 * the set (every stream's buffers freed, nothing left queued that reads d_src): there is nothing to abandon then;
 * nlzm_hip_blocks_abandon() drops a set the caller does not want to finish.  A stream whose launch fails hands its error on to the launch
 * that is already queued behind it, whose stages leave at once: the failing step returns within the time of a launch, not after a wait's bound.
 * Memory: the streams of a set reserve 32 BT4 (distance, length) pairs per position of a launch and take the rest from a per-launch arena of
 * positions / 64 + 1024 extension blocks (a single stream reserves all 256 pairs a position can have, NLZM.cpp:777).  An input with more such
 * positions than the arena serves (contrived: nlzm_amd/corpus.py `spines`) does not fail: the stream concerned is made again from its first
 * byte as a single stream, with buffers of its own, when the set is finished -- the same bytes, later; nlzm_hip_get_counter("block_redo_streams")
 * counts them. */
int nlzm_hip_blocks_begin(const void *d_src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req);
int nlzm_hip_blocks_step(uint32_t max_chunks_per_block, uint64_t *in_done_total, int *finished, double *device_ms);
int nlzm_hip_blocks_finish(void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
void nlzm_hip_blocks_abandon(void);
/* One-shot form.  nblocks: 1 .. 65536.  Up to the device's capacity (what nlzm_hip_blocks_begin takes: 64 on an MI355X) this is begin, one step to
 * the end and finish -- ONE set, 33 to 64 blocks included.  More blocks than that are the same ceil(n / nblocks) partition, compressed in
 * ceil(nblocks / "container_set_blocks") sets one after another, as equal as they can be (65 blocks by 32: 22 + 22 + 21): every set is such a block set
 * with the partition fixed, its streams go straight to their place in d_dst and block_len, and block i holds the bytes of the reference run on its byte
 * range whatever set it falls into (a block wholly behind the input's end: the empty stream; a whole set may consist of those).  The sets neither
 * overlap nor change a kernel; the block set's one allocation is used again from set to set (with "keep_block_pool" 0 too: it is then released when the call
 * ends, and "block_pool_bytes" reads 0 as after any set).  A set that fails ends the call with
 * its error and nothing open.  Afterwards nlzm_hip_get_stats is the sum over all sets, "block_redo_streams" counts over all of them,
 * "block_pool_bytes" is the largest set's and "container_sets" says how many sets ran (1: the blocks fitted one launch).  d_dst needs room for
 * nlzm_hip_compress_blocks_bound(n, nblocks) at most.  (nlzm_hip_get_timing is the single stream's: no block set, and no container, writes it.)  The stepping form above keeps its limit: there is none for containers. */
int nlzm_hip_compress_blocks_dev(const void *d_src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req,
                                 void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);

/* Room the streams of nblocks blocks of n bytes take at most, for d_dst / dst of the one-shot forms: up to 64 blocks nlzm_hip_compress_bound(n) and
 * a margin of 128 KiB a stream, as ever; above that the sum of nlzm_hip_compress_bound(block's length) over the blocks -- a guaranteed bound for a
 * container compressed in sets (about 148 KB a block: 9.7 GB at 65,536 blocks, most of it never touched).  Needs no device.  0 when nblocks is 0 or
 * above 65536. */
uint64_t nlzm_hip_compress_blocks_bound(uint64_t n, uint32_t nblocks);

/* same, host buffers (the device output is sized by nlzm_hip_compress_blocks_bound) */
int nlzm_hip_compress_blocks(const uint8_t *src, uint64_t n, uint32_t nblocks, uint32_t hist_bits_req,
                             uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);

/* ---- blocks of the caller's choosing -------------------------------------------------------------------------- */
/* k ranges of ONE buffer, each compressed as a stream of its own: range i is [off[i], off[i] + len[i]) of the n bytes at d_src (records, the files of
 * an archive, tensors, pages -- or the blocks nlzm_hip_cut_points* finds).  k: 1 .. 65536.  off / len / block_len: host arrays of k entries.  Ranges
 * may be empty, overlap, repeat and come in any order (the idiom of nlzm_hip_crc32_ranges and nlzm_hip_read_ranges).  Stream i is byte for byte the
 * reference run on those bytes at hist_bits_req (encode_file, NLZM.cpp:1711), with the geometry of that range's own length, as an equal block's is; the
 * streams are written back to back in the caller's order and block_len[i] (may be NULL) holds their lengths: a block container that every read-side
 * entry point takes, with raw lengths len[i].  d_src needs the 128 readable bytes behind n that nlzm_hip_compress_blocks_dev asks for.
 * Errors, all before any launch: a range with len > n - off is NLZM_HIP_E_ARG (the text names it); dst_cap below
 * nlzm_hip_compress_ranges_bound(k, len) is NLZM_HIP_E_CAPACITY.  A call that fails leaves nothing open.
 * Up to the device's capacity (64 on an MI355X) the ranges run as ONE block set, sized by its longest range: it opens wherever the equal split of
 * count x longest bytes would.  More ranges run in sets of consecutive ranges, split as nlzm_hip_compress_blocks_dev splits its blocks ("container_set_blocks";
 * 65 by 32: 22 + 22 + 21), one after another; "container_sets" counts them, nlzm_hip_get_stats sums over them.  No kernel differs from the equal split's. */
int nlzm_hip_compress_ranges_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len,
                                 uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
/* the same on host buffers (the 128 bytes behind the input are the library's; dst_cap is held to the same bound) */
int nlzm_hip_compress_ranges(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len,
                             uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
/* Room the streams of k ranges of these lengths take at most: the sum of nlzm_hip_compress_bound(len[i]).  Needs no device.  0 when k is 0 or above
 * 65536, or when the sum does not fit 64 bits. */
uint64_t nlzm_hip_compress_ranges_bound(uint32_t k, const uint64_t *len);

/* ---- content-defined cut points ----------------------------------------------------------------------------------- */
/* Where to cut n bytes into blocks so that the cuts follow the content: an insertion or deletion moves the cuts around it and leaves the blocks
 * further on as they were (byte for byte, so their streams and CRC32s too), which the equal partition cannot.  The rule (nlzm_amd/csrc/nlzm_cut.h;
 * tests/cut_model.py restates it): G[b] = the upper 32 bits of splitmix64(b); h(p) = sum over j = 0 .. 31 of G[x[p - j]] << j modulo 2^32 for p >= 31
 * (the gear hash h = (h << 1) + G[byte]); p is a candidate when the top avg_bits bits of h(p) are zero, its boundary p + 1.  From s = 0, while
 * n - s > min_len: e = the first candidate boundary in [s + min_len, min(s + max_len, n)], else that upper end; stop if e >= n; cut[i++] = e; s = e.
 * The blocks are the pieces between the cuts: all but the last hold min_len .. max_len bytes, 2^avg_bits on average beyond min_len where the
 * content is varied; n = 0 has no cut (one empty block).  cut: a host array of cut_cap entries, ascending; *ncuts: how many were written.  More
 * cuts than cut_cap: NLZM_HIP_E_CAPACITY, *ncuts the number needed, nothing written to cut.  Checked without a device or a launch: avg_bits 1 .. 30,
 * 32 <= min_len <= max_len <= 2^31.  Reads stay inside [d_src, d_src + n): no padding, no alignment is asked for.
 * On the device: one wave per segment of nlzm_hip_get_counter("cut_segment_bytes") bytes hashes every position and marks the candidates in a
 * bitmap, then one wave walks the rule over the bitmap; device memory n / 8 bytes, a word per segment and the list; only the list comes back.
 * Counters of the last call: "cut_us" (device time of both launches), "cut_candidates", "cut_segment_bytes" (needs no device). */
int nlzm_hip_cut_points_dev(const void *d_src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len,
                            uint64_t *cut, uint32_t cut_cap, uint32_t *ncuts);
int nlzm_hip_cut_points(const uint8_t *src, uint64_t n, uint32_t avg_bits, uint64_t min_len, uint64_t max_len,
                        uint64_t *cut, uint32_t cut_cap, uint32_t *ncuts);         /* uploads first */

/* ---- equal ranges ------------------------------------------------------------------------------------------------ */
/* Which of k ranges of ONE buffer hold the same bytes: first_of[i] = the smallest j <= i whose range [off[j], off[j] + len[j]) of the buf_len bytes at
 * d_buf holds the bytes of range i (a range is equal to itself, so first_of[i] == i says "not seen before").  k: 1 .. 65536; off / len / first_of /
 * fingerprint: host arrays of k entries.  Ranges may be empty, overlap, repeat and come in any order.  The answer is EXACT: a 64-bit fingerprint of
 * every range groups them, and every member of a group is compared byte by byte with its representative before it is called equal; a fingerprint
 * collision costs a second round of compares, never a wrong or a missed duplicate.  Two ranges with the same (off, len) are equal without a compare,
 * all empty ranges are equal to the first empty one.  A range with len > buf_len - off is NLZM_HIP_E_ARG (the text names it): checked before any
 * launch, with or without a device.  Reads stay inside the ranges: no padding, no alignment is asked for.
 * The fingerprint (nlzm_amd/csrc/nlzm_dedup.h; tests/dedup_model.py restates it) is a function of the range's bytes and its length alone: the range
 * is cut into segments of nlzm_hip_get_counter("dedup_segment_bytes") bytes from its own first byte; a segment's bytes, zeros behind them up to a
 * multiple of 16, are little-endian 32-bit words w[j]; with K(j) = mix32(j + 1), h = the sum over the 16-byte units u of (w[4u] + K(4u)) * (w[4u + 1]
 * + K(4u + 1)) + (w[4u + 2] + K(4u + 2)) * (w[4u + 3] + K(4u + 3)), the factors modulo 2^32, the sum modulo 2^64; F = splitmix64((sum over the
 * segments g of splitmix64(h(g) + (g + 1) * 0x9E3779B97F4A7C15) modulo 2^64) XOR splitmix64(len)).  fingerprint (may be NULL) receives F of every range.
 * On the device: one wave per segment in ONE launch for all ranges (unaligned 16-byte loads, the tail byte by byte), one wave per range to combine;
 * per round of compares one wave per 32 KiB chunk of a pair, then one per pair; no atomics.  Only fingerprints and verdicts come back to the host.
 * Counters of the last call: "dedup_distinct" (ranges that are their own first), "dedup_dup_bytes" (bytes of the ranges that are another's copy),
 * "dedup_rounds", "dedup_pairs", "dedup_compared_bytes" (the compared pairs' lengths), "dedup_us" (device time of all its launches),
 * "dedup_segment_bytes" (needs no device); "dedup_ranges" reads the option of that name as it stands.
 * With option "dedup_ranges" set, nlzm_hip_compress_ranges* finds first_of first and compresses the distinct ranges only -- stream i is a function of
 * range i's bytes and hist_bits_req alone, so equal ranges have equal streams: the distinct ranges, in order of first occurrence, run as sets into a
 * scratch allocation of the library's sized by their bound (NLZM_HIP_E_NOMEM when there is no room), and one launch of the range reader's gather kernel
 * puts stream first_of[i] at stream i's place ("dedup_gather_us").  d_dst, block_len and *dst_len are byte for byte what the call gives with the option
 * off, dst_cap is held to the same bound; "container_sets" counts the sets that ran and nlzm_hip_get_stats sums over the streams that were compressed.
 * With every range distinct the call runs what it runs with the option off. */
int nlzm_hip_equal_ranges_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len,
                              uint32_t *first_of, uint64_t *fingerprint /* may be NULL */);
int nlzm_hip_equal_ranges(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len,
                          uint32_t *first_of, uint64_t *fingerprint /* may be NULL */);      /* uploads first */

/* ---- typed ranges: byte planes ----------------------------------------------------------------------------------------- */
/* The filter in front of the coder for arrays of fixed-size elements (bf16 / fp16 / fp32 weights, int32 / int64 ids, offsets): every element's byte j
 * goes to plane j, so that the bytes that carry structure -- sign and exponent, the high bytes of small integers -- lie together.  The rule
 * (nlzm_amd/csrc/nlzm_planes.h; tests/planes_model.py restates it): for a range x of n bytes and an element size e in {1, 2, 4, 8}, m = n div e,
 * planes_e(x) = y with y[j m + i] = x[i e + j] for 0 <= j < e, 0 <= i < m, and y[e m + t] = x[e m + t] for the n - e m tail bytes.  e = 1 is the
 * identity; both directions keep the length; elements are counted from the range's own first byte, no address and no alignment enters.
 * nlzm_hip_planes*: k ranges in ONE launch (k: 1 .. 65536; src_off / dst_off / len / elem: host arrays of k entries): range i is len[i] bytes at
 * src_off[i] of the src_len bytes at d_src and goes to dst_off[i] of the dst_len bytes at d_dst, filtered (inverse == 0) or with the filter undone
 * (inverse != 0).  Source ranges may be empty, overlap and repeat.  All NLZM_HIP_E_ARG, the text naming the range, checked before any launch, with or
 * without a device: destinations that overlap each other, the two buffers overlapping (there is no in-place form), an elem outside {1, 2, 4, 8}, a
 * range that runs over its buffer.  Reads stay inside the source ranges and writes inside the destination ranges: no padding, no alignment is asked
 * for, of either side or of one relative to the other.  The host form uploads the source and copies back the destination ranges only: the bytes
 * between them stay the caller's.
 * On the device: one wave per segment of nlzm_hip_get_counter("planes_segment_bytes") bytes of a range keeps an image of the segment's planes in LDS;
 * every byte is loaded once and stored once, in 16-byte units but for up to 15 bytes at the ends of a run; no atomics.
 * nlzm_hip_compress_ranges_typed*: nlzm_hip_compress_ranges* with an element size per range.  The ranges are filtered in one launch into a scratch
 * allocation of the library's (the sum of len and the 128 bytes behind it; NLZM_HIP_E_NOMEM when there is no room, and nothing is left open), and
 * nlzm_hip_compress_ranges_dev runs on that scratch: stream i is byte for byte the reference run on planes_elem[i](range i), the reference
 * decompressor reads it, and option "dedup_ranges" is honoured as it stands (on the filtered bytes).  Nothing but the reads of d_src differs:
 * arguments, errors, bound and counters are the untyped call's.  elem == NULL, or every elem 1, IS the untyped call, with no scratch.
 * nlzm_hip_decompress_blocks_typed*: nlzm_hip_decompress_blocks* with an element size per block: block_len / raw_len / d_dst == NULL (a size pass,
 * which needs no filter) as there; the blocks are decoded into scratch (sized first when raw_len is NULL) and one inverse launch puts every block at
 * its place in d_dst.  elem == NULL, or every elem 1, is the untyped call.
 * Counters of the last call: "planes_us" (device time of its planes launch), "planes_bytes" (what it moved), "planes_segment_bytes" (needs no device). */
int nlzm_hip_planes_dev(const void *d_src, uint64_t src_len, void *d_dst, uint64_t dst_len, uint32_t k,
                        const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, const uint8_t *elem, int inverse);
int nlzm_hip_planes(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_len, uint32_t k,
                    const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, const uint8_t *elem, int inverse);      /* uploads, downloads */
int nlzm_hip_compress_ranges_typed_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem,
                                       uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
int nlzm_hip_compress_ranges_typed(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, const uint8_t *elem,
                                   uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
int nlzm_hip_decompress_blocks_typed_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                                         const uint8_t *elem, void *d_dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len);
int nlzm_hip_decompress_blocks_typed(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                                     const uint8_t *elem, uint8_t *dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len);

/* ---- streaming host input and output ---------------------- */
/* The reference reads its input and writes its frames as it goes (NLZM.cpp:1774-1778, :1853, :1870-1885).  Here the
 * caller announces the input's length, hands the bytes over in pieces, in order (any piece size; a piece travels through
 * pinned staging buffers on a copy stream while the chunks whose input has arrived are being compressed), and takes the
 * stream back in pieces (whole frames, as they are finished).  The host side never holds more than a piece; the input stays
 * whole in HBM (matches reach back a window).  feed_finish after the last piece, feed_output until it gives 0 bytes,
 * feed_end to release the buffers.  A call that fails has ended the feed. */
int nlzm_hip_feed_begin(uint64_t n, uint32_t hist_bits_req);
int nlzm_hip_feed(const uint8_t *piece, uint64_t len);
int nlzm_hip_feed_output(uint8_t *dst, uint64_t cap, uint64_t *len);
int nlzm_hip_feed_finish(void);
void nlzm_hip_feed_end(void);

/* ---- independent blocks on several GPUs of one node ------------------------ */
/* devices[0..ndev): HIP device ordinals, each listed once.  The input is cut into ndev * blocks_per_dev blocks exactly as
 * nlzm_hip_compress_blocks cuts it for that many blocks (the reference side: one encode_file call per byte range,
 * NLZM.cpp:1711); device i compresses blocks [i*blocks_per_dev, (i+1)*blocks_per_dev) in block mode on a host thread and a
 * device context of its own (nlzm_hip_init is not needed for it, and the process-wide context is left as it was).  No GPU
 * talks to another while compressing; the streams are then gathered onto devices[0], GPU to GPU (over xGMI where the
 * devices are linked), and copied out in block order.  block_len: ndev * blocks_per_dev entries (may be NULL). */
int nlzm_hip_compress_blocks_multi(const int *devices, uint32_t ndev, uint32_t blocks_per_dev,
                                   const uint8_t *src, uint64_t n, uint32_t hist_bits_req,
                                   uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);

/* Block mode's placement rule, for inspection (no device needed): workgroup `workgroup` of the shared persistent launch of
 * nstreams streams with blocks_per_stream workgroups each (three stage workgroups + the worker CUs) belongs to *stream and is
 * its block *local (0 finder, 1 table, 2 parser, 3.. workers).  With a multiple of eight streams all blocks of a stream have the
 * same workgroup index modulo 8, i.e. lie on one XCD under the round-robin dispatch (speed only). */
void nlzm_hip_block_placement(uint32_t nstreams, uint32_t blocks_per_stream, uint32_t workgroup, uint32_t *stream, uint32_t *local);

/* ---- decoding on the device: decode_file (NLZM.cpp:1912-2039), one workgroup per stream ---------------- */
/* The streams this library writes are read back where they lie: one workgroup (a single wave) decodes one stream, the streams of a block
 * container all at once.  The bytes accepted and produced are exactly those of the host decoder behind `nlzm d` (nlzm_amd/csrc/nlzm_host_decode.h):
 * hist_bits 10 .. 28, frame_bits 12 .. 20, frames until the zero num_ops word.  A lone wave is an order of magnitude slower than a host core
 * on ONE stream (DESIGN.md section 16 has the figures); the entry points are for data that is in HBM already -- verifying what was just
 * compressed before the source is dropped, and block containers, whose streams decode beside each other.
 * Bounds: reads stay inside [d_stream, d_stream + stream_len) -- no padding is needed behind a stream --, writes inside [d_dst, d_dst + dst_cap).
 * A stream that is not well-formed ends with NLZM_HIP_E_FORMAT (what was decoded up to there may have been written), never with a fault; a
 * decode that overruns a generous time bound ends with NLZM_HIP_E_KERNEL.
 * Counters of the last call, by nlzm_hip_get_counter: "decode_syms", "decode_raw_ops", "decode_n_literal", "decode_n_dict", "decode_n_rep" (the
 * oracle's rans_syms, bit_ops, n_literal, n_dict, n_rep), "decode_out_bytes", "decode_ring_bytes" / "decode_global_bytes" (match bytes served
 * from the LDS ring / from memory), "decode_cycles", "decode_window_cycles", "decode_copy_cycles" (wave cycles summed over the streams: in all,
 * waiting for input windows, copying and flushing), "decode_max_stream_cycles" and "decode_slowest_stream" (the stream with the most cycles and its index), "decode_streams", "decode_passes", "decode_ms" / "decode_us"
 * (device time of the call's decode launches; nlzm_hip_timing stays the compress path's), "decode_ring_size" (the LDS ring of the kernel the call's last
 * decode launch ran).
 * Two one-shot kernels run the same role: decode_kernel with a 64 KiB ring -- a CU's LDS holds two of its one-wave workgroups, 2 x CUs streams are at work
 * at once, each wave with a SIMD to itself -- and decode_small_kernel with a 16 KiB ring, ten workgroups to a CU, whose waves fill each other's issue gaps;
 * matches that reach further back than the ring are served from memory by either.  Option "decode_ring" picks: 0 (default) by the launch -- more
 * streams than 2 x CUs run the small kernel, every other launch the big one --, 65536 / 16384 force one.  It holds for every one-shot decode launch:
 * nlzm_hip_decompress*, nlzm_hip_verify*, nlzm_hip_check*, nlzm_hip_read_ranges* (prefix mode included).  The stepping form always has 64 KiB. */

/* d_dst == NULL: size query, *dst_len = uncompressed length (the format stores none: the stream is decoded without storing).
 * dst_cap too small: NLZM_HIP_E_CAPACITY, nothing written at or beyond d_dst + dst_cap. */
int nlzm_hip_decompress_dev(const void *d_stream, uint64_t stream_len, void *d_dst, uint64_t dst_cap, uint64_t *dst_len);
/* the same on host buffers (dst == NULL: size query) */
int nlzm_hip_decompress(const uint8_t *stream, uint64_t stream_len, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_len);

/* nblocks streams back to back (what nlzm_hip_compress_blocks* writes).  block_len: their lengths, or NULL (found by their frame headers).
 * raw_len_in: the blocks' uncompressed lengths where known (the .idx of `nlzm c -blocks:k` has them), else NULL (a size pass runs first).
 * raw_len_out (may be NULL): what each block decoded to.  The blocks' bytes land in d_dst in block order, contiguous; a block that does not
 * decode to exactly its raw_len_in is an error (NLZM_HIP_E_CAPACITY if longer, NLZM_HIP_E_FORMAT if shorter), and no block writes into
 * another's range.  d_dst == NULL: size query (raw_len_out, *dst_len) -- by a decode without stores when raw_len_in is NULL; with raw_len_in
 * given NOTHING is decoded and the caller's own numbers come back (their sum in *dst_len). */
int nlzm_hip_decompress_blocks_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in,
                                   void *d_dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len);
/* the same on host buffers */
int nlzm_hip_decompress_blocks(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len_in,
                               uint8_t *dst, uint64_t dst_cap, uint64_t *raw_len_out, uint64_t *dst_len);

/* Decode (nblocks = 1: one stream) into a buffer of the library's own and compare with the n original bytes at d_orig.
 * *decoded_len: what the stream(s) decoded to; *first_mismatch: the first offset below min(n, *decoded_len) at which the bytes differ, else
 * that minimum (a wrong length is a mismatch at the shorter length).  EQUAL means BOTH *first_mismatch == n AND *decoded_len == n -- a stream
 * that decodes to the n bytes and more behind them has *first_mismatch == n too, which is why the length is not optional:
 * NLZM_HIP_VERIFY_EQUAL spells the test.  One decode pass when the blocks are the ceil(n / nblocks) partition nlzm_hip_compress_blocks*
 * makes; any other container is sized first. */
#define NLZM_HIP_VERIFY_EQUAL(first_mismatch, decoded_len, n) ((first_mismatch) == (n) && (decoded_len) == (n))
int nlzm_hip_verify_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len,
                        const void *d_orig, uint64_t n, uint64_t *first_mismatch, uint64_t *decoded_len);
/* the same for a caller without device pointers (`nlzm c -verify`): both buffers are uploaded first */
int nlzm_hip_verify(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len,
                    const uint8_t *orig, uint64_t n, uint64_t *first_mismatch, uint64_t *decoded_len);

/* ---- decoding in steps: stop at a frame boundary, resume --------------------------------------------------------------------- */
/* The same decode, one launch per step: a stream stops in front of a frame header and a later launch picks it up from a record the library keeps
 * in device memory (nlzm_hip_get_counter("decode_state_bytes") per stream; needs no device) at the price of reloading the last 64 KiB it wrote.  One
 * decode set is open per device at a time, in the idiom of nlzm_hip_blocks_begin / _step / _finish / _abandon; a second begin closes the set before it.
 * begin binds the buffers, splits the container (block_len, or the hop over the frame headers when it is NULL) and decodes NOTHING.  Block i's bytes
 * go to d_dst + sum(raw_len[0..i)), bounded by raw_len[i], as in nlzm_hip_decompress_blocks_dev; raw_len may be NULL for nblocks == 1 only (the bound
 * is dst_cap then); d_dst == NULL: size-only stepping.  The host form uploads the container, runs the size pass when raw_len is NULL and decodes into
 * a buffer of the library's own (nlzm_hip_decode_fetch reads it).  flags: NLZM_HIP_DECODE_MORE, for the _dev form with ONE stream: src_len is what
 * has arrived so far, the caller vouches for nothing behind it, and a step pauses in front of the first frame that is not wholly there;
 * nlzm_hip_decode_extend_dev says that more has been written behind it (an extend without growth, a step that still pauses for input: the stream
 * is cut off, and finish answers NLZM_HIP_E_FORMAT).  Any other flag is NLZM_HIP_E_ARG: a prefix read is cut in the middle of an op and cannot resume.
 * step: ONE launch over the blocks that are neither finished nor at their target (none such: no launch).  Every launched block advances by at most
 * max_frames frames (0: no limit) and stops at the first frame boundary with at least target[i] bytes decoded (target: nblocks entries or NULL; ~0: to
 * its end); a stream's terminator ends it whatever the limits.  done[i] (may be NULL): block i's decoded bytes; *finished: every block has reached its
 * terminator.  A block that ends longer / shorter than its raw_len: NLZM_HIP_E_CAPACITY / NLZM_HIP_E_FORMAT; a step that fails has closed the set.
 * fetch: off / len address the container's decoded bytes; a part that is not decoded yet, or len > total - off, is NLZM_HIP_E_ARG.
 * finish needs *finished -- otherwise NLZM_HIP_E_ARG, and the set stays open -- and releases the states; abandon always works.
 * Counters: after a step the "decode_*" counters are the SET's totals so far (after the last step: the one-shot decode's of the same container),
 * "decode_steps" its launches, "decode_step_us" the device time of the last step. */
#define NLZM_HIP_DECODE_MORE 1u
int nlzm_hip_decode_begin_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len,
                              const uint64_t *raw_len, void *d_dst, uint64_t dst_cap, uint32_t flags);
int nlzm_hip_decode_begin(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len,
                          const uint64_t *raw_len, uint32_t flags);
int nlzm_hip_decode_step(uint32_t max_frames, const uint64_t *target, uint64_t *done, int *finished, double *device_ms);
int nlzm_hip_decode_extend_dev(uint64_t src_len_now);
int nlzm_hip_decode_fetch(uint64_t off, uint64_t len, uint8_t *dst);
int nlzm_hip_decode_finish(uint64_t *raw_len_out, uint64_t *dst_len);
void nlzm_hip_decode_abandon(void);

/* ---- CRC32 of bytes in device memory, and checking a container without its original ------------------------ */
/* The CRC is the reference's crc32_calc (NLZM.cpp:126-199): reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF -- zlib.crc32, and what
 * `nlzm h` prints.  The format stores none; `nlzm c -crc` keeps one per block in the sidecar index (NLZMIDX 2).  A range is cut into segments of
 * nlzm_hip_get_counter("crc_segment_bytes") bytes, one wave each, whose results are combined on the device, always in the same order.
 * Bounds: reads stay inside [d_buf + off, d_buf + off + len) of every range -- no padding, no alignment is asked for.  `seed` chains calls as
 * zlib.crc32(b, seed) does.  Counters of the last call: "crc_us" (device time of its CRC launches), "crc_bytes", "crc_segment_bytes" (needs no device). */
int nlzm_hip_crc32_dev(const void *d_buf, uint64_t n, uint32_t seed, uint32_t *crc);
int nlzm_hip_crc32(const uint8_t *buf, uint64_t n, uint32_t seed, uint32_t *crc);          /* uploads first */
/* nranges ranges of one buffer in one call (seed 0): they may be empty, overlap and be unaligned; a range with off + len > buf_len is
 * NLZM_HIP_E_ARG.  off / len / crc: host arrays of nranges entries. */
int nlzm_hip_crc32_ranges_dev(const void *d_buf, uint64_t buf_len, uint32_t nranges,
                              const uint64_t *off, const uint64_t *len, uint32_t *crc);
int nlzm_hip_crc32_ranges(const uint8_t *buf, uint64_t buf_len, uint32_t nranges,
                          const uint64_t *off, const uint64_t *len, uint32_t *crc);         /* uploads first (the command line holds no device pointers) */
/* CRC32 of A || B from crc_a = CRC32 of A, crc_b = CRC32 of B and len_b = |B| (zlib's crc32_combine).  A pure function: it needs no device, cannot
 * fail and returns the CRC itself. */
uint32_t nlzm_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* between feed_finish and feed_end: CRC32 of the fed input, which is whole in HBM */
int nlzm_hip_feed_input_crc32(uint32_t *crc);

/* Decode (as nlzm_hip_verify_dev does, into a buffer of the library's own) and compare every block's CRC32 and length with what the
 * caller holds -- the original is not needed.  raw_len may be NULL (a size pass runs first; then only the CRCs are checked).
 * *first_bad: index of the first block whose decoded length or CRC32 differs, nblocks when none does.  crc_out (may be NULL): what each
 * block's bytes hash to.  A stream that is not well-formed is NLZM_HIP_E_FORMAT as everywhere else. */
int nlzm_hip_check_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                       const uint32_t *crc, uint32_t *first_bad, uint32_t *crc_out);
int nlzm_hip_check(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                   const uint32_t *crc, uint32_t *first_bad, uint32_t *crc_out);

/* ---- byte ranges out of a block container ---------------------------------------------------------------- */
/* off[i], len[i] address the container's DECODED bytes: the blocks' contents back to back.  Ranges may be empty, overlap, repeat and come in any
 * order; their bytes land in d_dst back to back in the caller's order, *dst_len is their sum (nranges == 0: success, *dst_len = 0).  A range with
 * len > total - off is NLZM_HIP_E_ARG; *dst_len > dst_cap is NLZM_HIP_E_CAPACITY with nothing written.  nblocks: 1 .. 65536 (one stream: 1).
 * block_len / raw_len as for nlzm_hip_decompress_blocks_dev: either may be NULL (the hop over the frame headers; a size pass of ALL blocks).
 * With both given nothing but the needed blocks is touched: a block is needed when a non-empty range intersects it, is decoded ONCE per call, from
 * its first byte (matches reach back) up to the furthest byte any range wants of it and no further (the decoder role's prefix mode, nlzm_decode.h),
 * all needed blocks in one launch.  A block that exactly one range needs, from its first byte on, is decoded straight into d_dst; every other one
 * into one scratch allocation of the library's (the sum of the prefixes needed; NLZM_HIP_E_NOMEM when there is no room -- no rounds), from where
 * one gather launch moves all wanted parts out.  A block read in full that is longer / shorter than raw_len says: NLZM_HIP_E_CAPACITY /
 * NLZM_HIP_E_FORMAT, as in nlzm_hip_decompress_blocks_dev; a block read in part that ends before the part does: NLZM_HIP_E_FORMAT.  A prefix
 * read vouches for nothing behind the bytes it returns.
 * crc (may be NULL; with it first_bad must not be): every block this call decoded IN FULL is hashed where it lies and compared; *first_bad is the
 * first such block that differs, nblocks when none does; the return code is 0 either way, as nlzm_hip_check* has it.  Blocks read in part cannot
 * be checked and are not: "range_blocks_checked" says how many were.
 * Counters of the last call: "range_blocks_decoded", "range_blocks_direct", "range_blocks_checked", "range_decoded_bytes" (what the decoder
 * produced: the cost), "range_returned_bytes", "range_scratch_bytes", "range_pieces" (what the gather launch moved), "range_us" (device time of
 * the decode and the gather launch: "range_decode_us" + "range_gather_us"), "range_chunk_bytes" (needs no device); the "decode_*" counters
 * describe the call's decode launch. */
int nlzm_hip_read_ranges_dev(const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                             const uint32_t *crc, uint32_t nranges, const uint64_t *off, const uint64_t *len,
                             void *d_dst, uint64_t dst_cap, uint64_t *dst_len, uint32_t *first_bad);
/* the same on host buffers: with block_len and raw_len given only the needed blocks' streams are uploaded, not the container */
int nlzm_hip_read_ranges(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, const uint64_t *raw_len,
                         const uint32_t *crc, uint32_t nranges, const uint64_t *off, const uint64_t *len,
                         uint8_t *dst, uint64_t dst_cap, uint64_t *dst_len, uint32_t *first_bad);

/* ---- tuning knobs (defaults are what bench.py measures) -------------------- */
/* key: "workers" (only 1: BT4 runs on per-head worker lanes), "batch_chunks" (chunks per persistent launch), "worker_blocks" (worker CUs of a stream, default 240: the stage CUs and these fill the device),
 * "worker_threads" (bin-taking lanes per worker CU, 64..512, default 128), "hot_waves" (waves per worker CU that take a hot
 * BT4 bin each, 0..6, default 2), "hot_min" (positions per launch from which a bin counts as hot, default 0: by the stream's pace -- 24 positions per millisecond of the launch before);
 * block mode: "block_worker_threads" (default 320) and "block_hot_waves" (default 3), the same two for the streams of a block set
 * (their worker CUs are few: the count follows from the number of streams), "block_batch_chunks" (chunks of every stream per
 * shared launch, default 8); "prefilter_bits_per_position" (log2 of the pre-filter table's entries per input position, default 4);
 * "keep_block_pool" (default 1: the one device allocation of a block set is kept when the set is closed and used again by the
 * next set that fits -- the driver clears freed device memory, and an allocation made soon after a large one was freed waits for it;
 * 0 releases it, as nlzm_hip_shutdown does; the kept allocation is what the set needed -- up to 0.85 of the device's free memory --
 * and is given back by itself when any other allocation of the library, e.g. a single stream's, fails for lack of memory);
 * "parser_helper" (default 1: a stream gets a helper parser workgroup -- one CU more -- that parses the back of every segment that is cut
 * at 4,096 positions while the parser stage parses its front; "block_parser_helper", default 0, the same for the streams of a block set);
 * "table_shape" (default 0: the table stage runs every launch with 16-entry fronts on seven waves or with 24-entry fronts on five, whichever the
 * launch before it asked for -- the share of its blocks in which some position had more entries than the fronts hold decides; 1 / 2 fix the
 * shape: source code runs ~20 % faster in the wide one, prose ~8 % faster in the narrow one);
 * test only: "test_fail_launch" (default -1) / "test_fail_stream": the finder stage of that launch of that stream of a block set (of the single stream)
 * raises an error at once; "block_ext_blocks" (default -1: by the launch's size): extension blocks of a block-set stream's pair-list arena;
 * "stage_report" (1: the stages' cycle accounting of
 * every finished stream, and of a block set per stream, on stderr; a container compressed in sets reports set by set);
 * "container_set_blocks" (default 32, 1 .. the device's capacity -- 64 on an MI355X: blocks per set of a container that nlzm_hip_compress_blocks* compresses
 * in sets); "decode_ring" (0, 65536 or 16384: which one-shot decode kernel runs, see the decoding section; read by every decode launch);
 * "dedup_ranges" (default 0; 1: nlzm_hip_compress_ranges* does not compress a range again whose bytes an earlier range of the call holds, see the
 * equal-ranges section; read by every such call, the process's rather than a device's); test only: "test_dedup_hash_bits" (default 64, 0 .. 64: the
 * equal-range finder keeps that many low bits of every fingerprint before it groups, so that its rounds can be exercised).
 * There are no environment knobs.
 * None of them changes a byte of the output.  The options are read when a stream or a block set is opened
 * (nlzm_hip_stream_begin, nlzm_hip_blocks_begin, nlzm_hip_feed_begin, the one-call entries): what is open keeps what it was opened with.
 * nlzm_hip_compress_blocks_multi is EXPERIMENTAL until a run on more than one device has been recorded (it has only been run with one). */
int nlzm_hip_set_option(const char *key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif
