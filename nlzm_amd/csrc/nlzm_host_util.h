// nlzm_host_util.h -- what ALL the library's host files share (the -x hip ones: the compress side's through nlzm_host_state.h, and
// nlzm_hip_decode.cpp, nlzm_hip_crc.cpp, nlzm_hip_range.cpp; nothing else includes this): the error and buffer scaffolding of the entry
// points, the per-device record of a call's counters, and THE prototypes of every function that crosses the boundary between the compress
// side and the read side -- a changed signature fails to compile.
#pragma once

#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/nlzm_hip.h"

namespace nlzm {
namespace dec { struct StreamArgs; struct StreamResult; }
namespace crc { struct Args; }
namespace range { struct Args; struct Piece; }

// nlzm_hip.cpp: the library's error text (what fail and HIPCHK end in) and its stream (an error if nlzm_hip_init has not succeeded)
int host_error(int code, const char *text);
int host_stream(hipStream_t *st);
void host_decode_setup(int64_t *ring_option, int *cu_count);     // option "decode_ring" and the device's CUs (0 without a device)
// nlzm_decode.hip, nlzm_decode_small.hip, nlzm_crc.hip, nlzm_range.hip
void launch_decode(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st);
void launch_decode_small(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st);      // the one-shot role with the small ring: the same args and results
uint32_t decode_small_ring();                       // ... and the bytes of that ring
void launch_decode_steps(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st);      // the stepping form: args carry state, max_frames, target
void launch_split(const void *d_src, unsigned long long len, uint32_t nblocks, unsigned long long *d_block_len, uint32_t *d_bad, hipStream_t st);
void launch_compare(const void *d_a, const void *d_b, unsigned long long n, unsigned long long *d_first, hipStream_t st);
void launch_crc(const crc::Args &a, uint32_t max_blocks, hipStream_t st);
void launch_gather(const range::Args &a, uint32_t max_blocks, hipStream_t st);
// nlzm_hip_range.cpp: ONE gather launch for the non-empty pieces (no piece, no launch), its tables uploaded and its device time ADDED to *us
int gather_on(hipStream_t st, const char *what, const std::vector<range::Piece> &pieces, double *us);
// nlzm_hip_decode.cpp
void decode_begin_call();                           // a new call: its device time and pass count start at 0
double decode_call_ms();                            // device time of the call's passes so far
dec::StreamArgs decode_stream_args(const uint8_t *d_stream, uint64_t len, uint8_t *d_dst, uint64_t cap);
int decode_run_streams(hipStream_t st, const std::vector<dec::StreamArgs> &args, std::vector<dec::StreamResult> &res);
int decode_sizes(hipStream_t st, const uint8_t *d_src, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, std::vector<uint64_t> &raw);
int decode_split(hipStream_t st, const void *d_src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len);
int decode_split_host(const uint8_t *src, uint64_t src_len, uint32_t nblocks, const uint64_t *block_len, std::vector<uint64_t> &off, std::vector<uint64_t> &len);
// nlzm_hip_crc.cpp
void crc_begin_call();
int crc_ranges_on(hipStream_t st, const void *d_buf, uint64_t buf_len, uint32_t nranges, const uint64_t *off, const uint64_t *len, uint32_t seed, uint32_t *crc_out);
// nlzm_hip_get_counter's "decode_*", "crc_*" and "range_*": nlzm_hip_decode.cpp, nlzm_hip_crc.cpp, nlzm_hip_range.cpp
int decode_counter(const char *key, uint64_t *value);
int crc_counter(const char *key, uint64_t *value);
int range_counter(const char *key, uint64_t *value);

constexpr size_t kErrText = 2048;                   // bytes of the library's error text, the terminator among them
inline int fail(int code, const char *fmt, ...)
{
    char text[kErrText];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return host_error(code, text);
}
#define HIPCHK(expr)                                                                                                        \
    do {                                                                                                                    \
        hipError_t e_ = (expr);                                                                                             \
        if (e_ != hipSuccess)                                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? NLZM_HIP_E_NOMEM : NLZM_HIP_E_NODEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// workgroups of a launch at most, beyond them the waves stride (nlzm_units.h): the launches of four waves a workgroup, and the CRC's and the cut
// points' (as they were first set; nobody has measured another value of either)
constexpr uint32_t kStrideBlocks = 1u << 20, kStrideBlocksWide = 1u << 22;

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, bytes ? bytes : 16)); return 0; }
    // a scratch allocation of a size the caller's arguments decide: NLZM_HIP_E_NOMEM when there is no room, and nothing is left open
    int alloc_for(uint64_t bytes, const char *what)
    {
        if (hipMalloc(&p, bytes ? bytes : 16) == hipSuccess) return 0;
        (void)hipGetLastError(); p = nullptr;
        return fail(NLZM_HIP_E_NOMEM, "no %llu bytes of device memory for %s", (unsigned long long)bytes, what);
    }
    template <class T> T *as() const { return (T *)p; }
};
// a host buffer onto the device: d allocated, the n bytes at src copied (n = 0: none), the stream synchronised
inline int upload(DevBuf &d, const void *src, uint64_t n, hipStream_t st)
{
    if (const int rc = d.alloc(n)) return rc;
    if (n) HIPCHK(hipMemcpyAsync(d.p, src, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
struct Events {
    hipEvent_t ev[2] = { nullptr, nullptr };
    ~Events() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    int create() { for (auto &e : ev) HIPCHK(hipEventCreate(&e)); return 0; }
};

// One record per device, like the rest of the library's state: what nlzm_hip_get_counter reports of the last call.  The map is guarded, a
// record is its device's (calls are not re-entrant per device).  No device: one record under -1, which only ever holds zeros.
template <class T> class PerDevice {
    std::mutex mu;
    std::map<int, T> of;
public:
    T &here()
    {
        int device = -1;
        (void)hipGetDevice(&device);
        std::lock_guard<std::mutex> lk(mu);
        return of[device];
    }
};

// One timed launch on `st`: before() queues what the kernel reads, launch() starts it, after() queues what comes back; each but launch()
// returns a hipError_t.  The stream is synchronised EVEN ON FAILURE: nothing queued before the failure may outlive the host memory the
// copies name.  ms: the kernel's device time, between two events.
template <class Before, class Launch, class After>
int timed_launch(hipStream_t st, const char *what, float *ms, Before before, Launch launch, After after)
{
    Events E;
    if (const int rc = E.create()) return rc;
    hipError_t e = before();
    if (e == hipSuccess) e = hipEventRecord(E.ev[0], st);
    if (e == hipSuccess) { launch(); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(E.ev[1], st);
    if (e == hipSuccess) e = after();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, E.ev[0], E.ev[1]);
    if (e != hipSuccess) return fail(NLZM_HIP_E_NODEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace nlzm
