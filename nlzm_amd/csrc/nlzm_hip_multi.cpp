// nlzm_hip_multi.cpp -- independent blocks on several GPUs of one node.
// One host thread and one device state per GPU; device i compresses blocks [i*m, (i+1)*m) of the n-byte input's partition into
// ndev*m blocks (the same byte ranges nlzm_hip_compress_blocks uses for that many blocks) in block mode; there is no traffic
// between the GPUs while they compress.  The only exchange is the final gather of the streams onto the first device of the
// list, GPU to GPU (hipMemcpyPeerAsync: over xGMI where the devices are linked), from where the artifact goes to the host.
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

#include "nlzm_host_state.h"
#include "nlzm_container_plan.h"

using namespace nlzm;
using namespace nlzm::host;

extern "C" {

int nlzm_hip_compress_blocks_multi(const int *devices, uint32_t ndev, uint32_t blocks_per_dev, const uint8_t *src, uint64_t n,
                                   uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len)
{
    if (!devices || !ndev || !blocks_per_dev || (!src && n) || !dst || !dst_len) return fail(NLZM_HIP_E_ARG, "null argument");
    if (ndev > 64) return fail(NLZM_HIP_E_ARG, "more than 64 devices");
    if (!g_dev0.opt.multi_same)
        for (uint32_t i = 0; i < ndev; i++)
            for (uint32_t k = 0; k < i; k++)
                if (devices[i] == devices[k]) return fail(NLZM_HIP_E_ARG, "device %d is listed twice", devices[i]);
    const uint64_t nb_total = (uint64_t)ndev * blocks_per_dev;
    const uint64_t per = n ? container::per_block(n, nb_total) : 1;      // (never 0, which nlzm_hip_blocks_begin reads as "not fixed")
    struct Part {
        DevState D;
        int device = 0, rc = 0;
        uint64_t lo = 0, n = 0, bound = 0, len = 0;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        std::vector<uint64_t> blens;
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
        container::block_range(n, per * blocks_per_dev, i, P.lo, P.n);         // its blocks back to back: part i of blocks_per_dev * per bytes a part
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
    for (auto &P : parts) {
        if (P.rc && !rc) {
            char msg[kErrText] = "";
            error_prefixed(msg, P.D.err, "device %d: ", P.device);     // (the text of the part's own thread)
            error_replace(msg);
            rc = P.rc;
        }
        total += P.len;
    }
    if (!rc && total > dst_cap) rc = fail(NLZM_HIP_E_CAPACITY, "streams are %llu bytes, dst_cap %llu", (unsigned long long)total, (unsigned long long)dst_cap);
    if (!rc) {
        // the gather: every device's streams onto the first one, in block order, then one copy to the host
        const int root = parts[0].device;
        rc = [&]() -> int {
            HIPCHK(hipSetDevice(root));
            if (ndev == 1) { HIPCHK(hipMemcpy(dst, parts[0].d_out, total, hipMemcpyDeviceToHost)); return 0; }
            DevBuf all;                             // (on the root, which stays the current device to the end of the gather)
            if (const int arc = all.alloc(total)) return arc;
            uint8_t *d_all = all.as<uint8_t>();
            // GPU to GPU: directly over the link where the root may address the device's memory (xGMI inside a node), else staged by the
            // runtime; which it was is reported.  Every copy is queued before any is waited for; events on the root's stream time them.
            std::vector<Events> ev(parts.size());
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
                if (hipEventCreate(&ev[k].ev[0]) != hipSuccess || hipEventCreate(&ev[k].ev[1]) != hipSuccess) { grc = fail(NLZM_HIP_E_NODEVICE, "hipEventCreate failed"); break; }
                (void)hipEventRecord(ev[k].ev[0], nullptr);
                if (P.len && hipMemcpyPeerAsync(d_all + off, root, P.d_out, P.device, P.len, nullptr) != hipSuccess)
                    grc = fail(NLZM_HIP_E_NODEVICE, "gather from device %d failed: %s", P.device, hipGetErrorString(hipGetLastError()));
                (void)hipEventRecord(ev[k].ev[1], nullptr);
                off += P.len;
            }
            if (!grc && hipDeviceSynchronize() != hipSuccess) grc = fail(NLZM_HIP_E_NODEVICE, "gather failed: %s", hipGetErrorString(hipGetLastError()));
            for (size_t k = 0; k < parts.size(); k++) {
                float ms = 0;
                if (!grc && ev[k].ev[0] && ev[k].ev[1] && hipEventElapsedTime(&ms, ev[k].ev[0], ev[k].ev[1]) == hipSuccess) parts[k].gather_ms = ms;
            }
            for (int d : enabled_here) (void)hipDeviceDisablePeerAccess(d);     // (only what this call enabled: the caller's settings stay)
            if (grc) return grc;
            HIPCHK(hipMemcpy(dst, d_all, total, hipMemcpyDeviceToHost));
            return 0;
        }();
        if (!rc) {
            if (block_len) for (uint32_t i = 0; i < ndev; i++) for (uint32_t k = 0; k < blocks_per_dev; k++) block_len[(uint64_t)i * blocks_per_dev + k] = parts[i].blens[k];
            *dst_len = total;
        }
    }
    // the job's counters (nlzm_hip_get_stats of the process-wide context reports them) and the clean-up, device by device
    memset(&g_dev0.ctx.stats, 0, sizeof g_dev0.ctx.stats);
    for (auto &P : parts) {
        add_stats(g_dev0.ctx.stats, P.D.ctx.stats);
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
