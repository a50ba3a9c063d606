// prep_probe.hip -- the compress path's pre-pass and gather kernels, each launched alone on host arrays.  TEST CODE ONLY: built by
// nlzm_amd/csrc/Makefile into a shared object of its own (nlzm_amd/libprep_probe.so) that is linked AGAINST the product's library and is
// never part of it.  tests/test_gpu_prep.py loads it; tests/prep_model.py is what the results are held to.
//
// There is no kernel in this file: every entry point calls the launch wrappers of nlzm_kernels.hip (nlzm_launch.h), so what runs is the
// code that ships.  Every entry point
//   * checks its sizes first and answers -1, having launched nothing, where they do not fit what the kernels index by;
//   * allocates, uploads, launches on one stream of its own, waits, downloads and frees -- nothing in here can wait for a workgroup;
//   * fills every buffer a kernel writes with kFill (0xA5 in every byte) and puts kSlack elements of it in front of and behind the range
//     the kernel may write: the arrays the caller gets back are slack + body + slack, so a stray or a missing store can be seen.
// Answers: 0, -1 (refused), or the HIP error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "nlzm_launch.h"

using namespace nlzm;

namespace {

constexpr uint64_t kSlack = 64;             // elements of sentinel on either side of every returned array (prep_probe_slack())
constexpr int kFill = 0xA5;

// what a call holds on the device, freed on every path out
struct Dev {
    std::vector<void *> bufs;
    hipStream_t st = nullptr;
    hipError_t err = hipSuccess;
    ~Dev()
    {
        for (void *p : bufs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    bool ok(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; return err == hipSuccess; }
    bool open() { return ok(hipStreamCreate(&st)); }
    // `bytes` of device memory with `fill` in every byte
    template <class T> T *get(uint64_t bytes, int fill)
    {
        void *p = nullptr;
        if (!ok(hipMalloc(&p, bytes ? bytes : 1))) return nullptr;
        bufs.push_back(p);
        ok(hipMemsetAsync(p, fill, bytes ? bytes : 1, st));
        return (T *)p;
    }
    template <class T> T *put(const void *src, uint64_t bytes)
    {
        T *p = get<T>(bytes, 0);
        if (p && bytes) ok(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st));
        return p;
    }
    bool back(void *dst, const void *src, uint64_t bytes) { return ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); }
    bool wait() { return ok(hipStreamSynchronize(st)) && ok(hipGetLastError()); }
};

}  // namespace

extern "C" uint64_t prep_probe_slack() { return kSlack; }

// rk_hash_kernel over the positions [pos0, pos1) of in[0, n).  out: slack + (pos1 - pos0) + slack words; out_words must say exactly that.
// The kernel is handed `out - pos0`, as the host pipeline hands it the launch's own array.
extern "C" int prep_probe_rk_hash(const uint8_t *in, uint64_t n, uint64_t pos0, uint64_t pos1, uint32_t *out, uint64_t out_words)
{
    if (!in || !out || !n || n > (1ull << 28) || pos1 <= pos0 || pos1 - pos0 > (1ull << 24) || pos0 > (1ull << 28)) return -1;
    const uint64_t cnt = pos1 - pos0;
    if (out_words != cnt + 2 * kSlack) return -1;
    Dev D;
    if (!D.open()) return (int)D.err;
    const uint8_t *d_in = D.put<uint8_t>(in, n);
    uint32_t *d_out = D.get<uint32_t>(out_words * 4, kFill);
    if (D.err != hipSuccess) return (int)D.err;
    launch_rk_hash(d_in, n, pos0, pos1, d_out + kSlack - pos0, D.st);
    D.back(out, d_out, out_words * 4);
    D.wait();
    return (int)D.err;
}

// The three pre-filter kernels, once per launch [launches[i][0], launches[i][1]) in order, on ONE T (zeroed) and ONE M (0xFF in every byte),
// as the host pipeline's stream has them: T and M live on from one launch to the next.
//   unc_out     per launch, back to back: slack + cnt + slack bytes (unc_bytes must be their sum); the buffer is refilled before every launch
//   m_live      per launch: the entries of M that are not kNone after it (the insert kernel leaves none)
//   m_out       M after the last launch, 2^m_bits words
//   t_idx, t_val, t_count   the words of the final T that are not 0, ascending: index and value, t_cap of them at most (t_count says how many
//               there are); every other word is 0.  T has 2^t_bits words, in bitmap form 2^t_bits / 32 (1 GiB at t_bits 33: read back in pieces)
extern "C" int prep_probe_prefilter(const uint8_t *in, uint64_t n, const uint32_t *launches, uint32_t nlaunch, uint32_t wmask, uint32_t t_bits,
                                    uint32_t t_bitmap, uint32_t m_bits, uint8_t *unc_out, uint64_t unc_bytes, uint32_t *m_live, uint32_t *m_out,
                                    uint64_t *t_idx, uint32_t *t_val, uint64_t t_cap, uint64_t *t_count)
{
    if (!in || !launches || !unc_out || !m_live || !m_out || !t_idx || !t_val || !t_count) return -1;
    if (!n || n > (1ull << 28) || !nlaunch || nlaunch > 64 || t_bitmap > 1 || m_bits < 1 || m_bits > 24) return -1;
    if (t_bitmap ? (t_bits < 5 || t_bits > 33) : (t_bits < 1 || t_bits > 26)) return -1;
    uint64_t need = 0, max_cnt = 0, prev = 0;
    for (uint32_t i = 0; i < nlaunch; i++) {
        const uint64_t a0 = launches[2 * i], a1 = launches[2 * i + 1];
        if (a0 < prev || a1 <= a0 || a1 > n || a1 - a0 > (1ull << 24)) return -1;       // ascending, not empty, inside the input
        prev = a1;
        need += a1 - a0 + 2 * kSlack;
        if (a1 - a0 > max_cnt) max_cnt = a1 - a0;
    }
    if (unc_bytes != need) return -1;
    const uint64_t t_words = t_bitmap ? 1ull << (t_bits - 5) : 1ull << t_bits, m_words = 1ull << m_bits;
    Dev D;
    if (!D.open()) return (int)D.err;
    const uint8_t *d_in = D.put<uint8_t>(in, n);
    uint32_t *T = D.get<uint32_t>(t_words * 4, 0), *M = D.get<uint32_t>(m_words * 4, 0xFF);
    uint32_t *hbuf = D.get<uint32_t>(max_cnt * 4, kFill), *hbuf2 = D.get<uint32_t>(max_cnt * 4, kFill);
    uint8_t *c1 = D.get<uint8_t>(max_cnt, kFill), *unc = D.get<uint8_t>(max_cnt + 2 * kSlack, kFill);
    if (D.err != hipSuccess) return (int)D.err;
    std::vector<uint32_t> m_host(m_words);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nlaunch; i++) {
        const uint32_t a0 = launches[2 * i], a1 = launches[2 * i + 1];
        const uint64_t len = (uint64_t)(a1 - a0) + 2 * kSlack;
        D.ok(hipMemsetAsync(unc, kFill, max_cnt + 2 * kSlack, D.st));
        launch_prefilter(d_in, n, a0, a1, wmask, t_bits, t_bitmap, m_bits, T, M, hbuf, hbuf2, c1, unc + kSlack, D.st);
        D.back(unc_out + at, unc, len);
        D.back(m_host.data(), M, m_words * 4);
        if (!D.wait()) return (int)D.err;
        at += len;
        uint32_t live = 0;
        for (uint64_t k = 0; k < m_words; k++) live += m_host[k] != kNone;
        m_live[i] = live;
    }
    memcpy(m_out, m_host.data(), m_words * 4);
    // the final T, as the list of its words that are not 0
    const uint64_t piece = 1ull << 24;          // words: 64 MiB at a time
    std::vector<uint32_t> t_host((size_t)(t_words < piece ? t_words : piece));
    uint64_t cnt = 0;
    for (uint64_t w0 = 0; w0 < t_words; w0 += piece) {
        const uint64_t m = t_words - w0 < piece ? t_words - w0 : piece;
        D.back(t_host.data(), T + w0, m * 4);
        if (!D.wait()) return (int)D.err;
        for (uint64_t k = 0; k < m; k++) {
            if (!t_host[k]) continue;
            if (cnt < t_cap) { t_idx[cnt] = w0 + k; t_val[cnt] = t_host[k]; }
            cnt++;
        }
    }
    *t_count = cnt;
    return 0;
}

// bin_kernel for the chunks [c0, c0 + nchunks) of in[0, n): the Geom is built from n, chunk_size, feed and bt_shift (the kernel reads no other
// field), `off` is zeroed and `cur` handed over as scratch, as the host pipeline's pre-pass does; batch_a0 must be the first chunk's first position.
//   unc         the marks of the launch's positions and ONE behind them (unc_len >= positions + 1; the kernel reads unc[a - batch_a0 + 1])
//   off_out     slack + nchunks * (nheads + 1) + slack words          pos_out     slack + nchunks * chunk_size * 2 + slack words
extern "C" int prep_probe_bin(const uint8_t *in, uint64_t n, uint32_t chunk_size, uint32_t feed, uint32_t bt_shift, uint32_t c0, uint32_t nchunks,
                              uint32_t nheads, const uint8_t *unc, uint64_t unc_len, uint32_t batch_a0, uint32_t *off_out, uint64_t off_words,
                              uint32_t *pos_out, uint64_t pos_words)
{
    if (!in || !unc || !off_out || !pos_out) return -1;
    if (!n || n > (1ull << 28) || chunk_size < 1 || chunk_size > (1u << 20) || feed < chunk_size || feed > (1u << 21)) return -1;
    if (bt_shift < 3 || bt_shift > 31 || !nchunks || nchunks > 64 || c0 > (1u << 20) || !nheads || nheads > (1u << 20)) return -1;
    const uint64_t a0 = (uint64_t)c0 * chunk_size, last = (uint64_t)(c0 + nchunks - 1) * chunk_size;
    if (last >= n || batch_a0 != a0) return -1;                             // every chunk begins inside the input
    uint64_t a1 = (uint64_t)(c0 + nchunks) * chunk_size;
    if (a1 > n) a1 = n;
    if (unc_len < a1 - a0 + 1) return -1;
    const uint64_t off_body = (uint64_t)nchunks * (nheads + 1), pos_body = (uint64_t)nchunks * chunk_size * 2;
    if (off_words != off_body + 2 * kSlack || pos_words != pos_body + 2 * kSlack) return -1;
    Geom g;
    memset(&g, 0, sizeof g);
    g.n = n; g.chunk_size = chunk_size; g.feed = feed; g.bt_shift = bt_shift;
    Dev D;
    if (!D.open()) return (int)D.err;
    const uint8_t *d_in = D.put<uint8_t>(in, n);
    const uint8_t *d_unc = D.put<uint8_t>(unc, unc_len);
    uint32_t *off = D.get<uint32_t>(off_words * 4, kFill), *pos = D.get<uint32_t>(pos_words * 4, kFill);
    uint32_t *cur = D.get<uint32_t>(((uint64_t)nchunks * nheads + 2 * kSlack) * 4, kFill);
    if (D.err != hipSuccess) return (int)D.err;
    D.ok(hipMemsetAsync(off + kSlack, 0, off_body * 4, D.st));
    launch_bin(d_in, g, c0, nchunks, nheads, off + kSlack, cur + kSlack, pos + kSlack, d_unc, batch_a0, D.st);
    D.back(off_out, off, off_words * 4);
    D.back(pos_out, pos, pos_words * 4);
    D.wait();
    return (int)D.err;
}

// hot_select_kernel on off[nchunks][nheads + 1].
//   hot_of_bin_out   slack + nheads + slack words          hot_list_out   slack + 1 + hmax + slack words
//   counter          in: what WorkerCounters::hot_bins holds before the launch; out: after it
//   other_counters   out: the other words of the WorkerCounters that are not 0 afterwards (they were all 0 before)
extern "C" int prep_probe_hot_select(const uint32_t *off, uint32_t nchunks, uint32_t nheads, uint32_t hmax, uint32_t min_count,
                                     uint32_t *hot_of_bin_out, uint64_t hob_words, uint32_t *hot_list_out, uint64_t list_words,
                                     uint64_t *counter, uint32_t *other_counters)
{
    if (!off || !hot_of_bin_out || !hot_list_out || !counter || !other_counters) return -1;
    if (!nchunks || nchunks > 64 || !nheads || nheads > (1u << 20) || hmax > (1u << 16)) return -1;
    if (hob_words != nheads + 2 * kSlack || list_words != 1 + (uint64_t)hmax + 2 * kSlack) return -1;
    WorkerCounters wc;
    memset(&wc, 0, sizeof wc);
    wc.hot_bins = *counter;
    Dev D;
    if (!D.open()) return (int)D.err;
    const uint32_t *d_off = D.put<uint32_t>(off, (uint64_t)nchunks * (nheads + 1) * 4);
    uint32_t *hob = D.get<uint32_t>(hob_words * 4, kFill), *list = D.get<uint32_t>(list_words * 4, kFill);
    WorkerCounters *d_wc = D.put<WorkerCounters>(&wc, sizeof wc);
    if (D.err != hipSuccess) return (int)D.err;
    launch_hot_select(d_off, nchunks, nheads, hmax, min_count, hob + kSlack, list + kSlack, d_wc, D.st);
    D.back(hot_of_bin_out, hob, hob_words * 4);
    D.back(hot_list_out, list, list_words * 4);
    D.back(&wc, d_wc, sizeof wc);
    if (!D.wait()) return (int)D.err;
    *counter = wc.hot_bins;
    wc.hot_bins = 0;
    uint32_t other = 0;
    const unsigned long long *w = (const unsigned long long *)&wc;
    for (size_t k = 0; k < sizeof wc / 8; k++) other += w[k] != 0;
    *other_counters = other;
    return 0;
}

// gather_frames_kernel: frame f is out_len[f] bytes at frames + f * stride and goes to dst + dst_off[f].
//   dst_out     slack + body + slack bytes (dst_bytes says so); every frame must end inside the body
extern "C" int prep_probe_gather(const uint8_t *frames, uint64_t stride, const uint64_t *dst_off, const uint32_t *out_len, uint32_t nframes,
                                 uint8_t *dst_out, uint64_t dst_bytes)
{
    if (!frames || !dst_off || !out_len || !dst_out || !nframes || nframes > 4096 || !stride || stride > (1ull << 24)) return -1;
    if (dst_bytes < 2 * kSlack || dst_bytes > (1ull << 28)) return -1;
    const uint64_t body = dst_bytes - 2 * kSlack;
    std::vector<FrameMeta> fm(nframes);
    for (uint32_t f = 0; f < nframes; f++) {
        if (out_len[f] > stride || dst_off[f] > body || out_len[f] > body - dst_off[f]) return -1;
        fm[f].nsyms = 0; fm[f].nbits_bytes = 0; fm[f].num_ops = 0; fm[f].out_len = out_len[f];
    }
    Dev D;
    if (!D.open()) return (int)D.err;
    const uint8_t *d_frames = D.put<uint8_t>(frames, (uint64_t)nframes * stride);
    const unsigned long long *d_off = D.put<unsigned long long>(dst_off, (uint64_t)nframes * 8);
    const FrameMeta *d_fm = D.put<FrameMeta>(fm.data(), (uint64_t)nframes * sizeof(FrameMeta));
    uint8_t *dst = D.get<uint8_t>(dst_bytes, kFill);
    if (D.err != hipSuccess) return (int)D.err;
    launch_gather(d_frames, stride, d_off, d_fm, dst + kSlack, nframes, D.st);
    D.back(dst_out, dst, dst_bytes);
    D.wait();
    return (int)D.err;
}
