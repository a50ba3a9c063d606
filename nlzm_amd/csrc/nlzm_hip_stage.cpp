// nlzm_hip_stage.cpp -- the three stage-test entry points: the frame coder alone, and what the finder and the parser of a whole stream
// produce, captured (StageCapture, nlzm_host_state.h).  Tests call these; the product does not.
#include <string.h>

#include <algorithm>
#include <vector>

#include "nlzm_host_state.h"
#include "nlzm_launch.h"

using namespace nlzm;
using namespace nlzm::host;

extern "C" {

int nlzm_hip_rans_frames(const uint32_t *syms, const uint64_t *sym_off, const uint8_t *bits, const uint64_t *bits_off,
                         const uint32_t *num_ops, uint32_t nframes, uint8_t *out, uint64_t out_stride, uint32_t *out_len)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!nframes) return 0;
    if (!syms || !sym_off || !bits || !bits_off || !num_ops || !out || !out_len) return fail(NLZM_HIP_E_ARG, "null argument");
    uint64_t max_syms = 1, max_bits = 4;
    for (uint32_t f = 0; f < nframes; f++) {
        if (sym_off[f + 1] - sym_off[f] > max_syms) max_syms = sym_off[f + 1] - sym_off[f];
        if (bits_off[f + 1] - bits_off[f] > max_bits) max_bits = bits_off[f + 1] - bits_off[f];
    }
    DevBuf b_syms, b_scr, b_bits, b_out, b_fm;      // the device buffers go with the call, on every path out (no size is 0: a frame at least, max_syms >= 1, max_bits >= 4)
    const unsigned long long fstride = 12 + max_bits + 16 + 2 * max_syms;
    int arc = b_syms.alloc(nframes * max_syms * 4);
    if (!arc) arc = b_scr.alloc(nframes * max_syms * 4);
    if (!arc) arc = b_bits.alloc(nframes * max_bits);
    if (!arc) arc = b_out.alloc(nframes * fstride);
    if (!arc) arc = b_fm.alloc(nframes * sizeof(FrameMeta));
    if (arc) return arc;
    uint32_t *d_syms = b_syms.as<uint32_t>(), *d_scr = b_scr.as<uint32_t>(); uint8_t *d_bits = b_bits.as<uint8_t>(), *d_out = b_out.as<uint8_t>(); FrameMeta *d_fm = b_fm.as<FrameMeta>();
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
        if (hm[f].out_len > out_stride) { rc = fail(NLZM_HIP_E_CAPACITY, "frame %u needs %u bytes", f, hm[f].out_len); break; }
        HIPCHK(hipMemcpy(out + f * out_stride, d_out + f * fstride, hm[f].out_len, hipMemcpyDeviceToHost));
    }
    return rc;
}

int nlzm_hip_find_matches(const uint8_t *src, uint64_t n, uint32_t hist_bits_req, uint64_t pos_lo, uint64_t pos_hi,
                          uint32_t *out_words, uint64_t cap_words, uint64_t *used_words)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!out_words || !used_words) return fail(NLZM_HIP_E_ARG, "null argument");
    if (C.stage.cap_words) { (void)hipFree(C.stage.cap_words); C.stage.cap_words = nullptr; }
    if (C.stage.cap_used) { (void)hipFree(C.stage.cap_used); C.stage.cap_used = nullptr; }
    HIPCHK(hipMalloc(&C.stage.cap_words, (cap_words + 1) * 4));
    HIPCHK(hipMalloc(&C.stage.cap_used, 8));
    HIPCHK(hipMemset(C.stage.cap_used, 0, 8));
    C.stage.cap_cap = cap_words; C.stage.cap_lo = pos_lo; C.stage.cap_hi = pos_hi;
    const uint64_t bound = nlzm_hip_compress_bound(n);
    std::vector<uint8_t> tmp(bound);
    uint64_t len = 0;
    int rc = nlzm_hip_compress(src, n, hist_bits_req, tmp.data(), bound, &len);
    unsigned long long used = 0;
    if (!rc) {
        HIPCHK(hipMemcpy(&used, C.stage.cap_used, 8, hipMemcpyDeviceToHost));
        // (the table stage's waves finish positions out of order: the records {position, max_len, delta[2..max_len]} are put
        //  into position order here)
        std::vector<uint32_t> raw(used);
        HIPCHK(hipMemcpy(raw.data(), C.stage.cap_words, used * 4, hipMemcpyDeviceToHost));
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
    (void)hipFree(C.stage.cap_words); (void)hipFree(C.stage.cap_used);
    C.stage.cap_words = nullptr; C.stage.cap_used = nullptr; C.stage.cap_cap = 0;
    return rc;
}

int nlzm_hip_parse_emit(const uint8_t *src, uint64_t n, uint32_t hist_bits_req, uint32_t frame_idx, uint32_t *syms,
                        uint32_t cap_syms, uint8_t *bits, uint32_t cap_bits, uint32_t *sizes_out)
{
    DevState &D = cur();
    Ctx &C = D.ctx;
    if (!C.inited) return fail(NLZM_HIP_E_NODEVICE, "nlzm_hip_init() has not succeeded");
    if (!syms || !bits || !sizes_out) return fail(NLZM_HIP_E_ARG, "null argument");
    C.stage.want_frame = frame_idx; C.stage.got = false;
    const uint64_t bound = nlzm_hip_compress_bound(n);
    std::vector<uint8_t> tmp(bound);
    uint64_t len = 0;
    int rc = nlzm_hip_compress(src, n, hist_bits_req, tmp.data(), bound, &len);
    C.stage.want_frame = -1;
    if (rc) return rc;
    if (!C.stage.got) return fail(NLZM_HIP_E_ARG, "frame %u does not exist", frame_idx);
    if (C.stage.got_meta.nsyms > cap_syms || C.stage.got_meta.nbits_bytes > cap_bits) return fail(NLZM_HIP_E_CAPACITY, "capture buffers too small");
    memcpy(syms, C.stage.got_syms.data(), C.stage.got_meta.nsyms * 4ull);
    memcpy(bits, C.stage.got_bits.data(), C.stage.got_meta.nbits_bytes);
    sizes_out[0] = C.stage.got_meta.nsyms; sizes_out[1] = C.stage.got_meta.nbits_bytes; sizes_out[2] = C.stage.got_meta.num_ops;
    return 0;
}

}  // extern "C"
