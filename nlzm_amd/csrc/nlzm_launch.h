// nlzm_launch.h -- the launch wrappers of nlzm_kernels.hip, declared once: the host pipeline (nlzm_hip.cpp, nlzm_hip_blocks.cpp, nlzm_hip_stage.cpp) calls them, and so does the
// pre-pass probe (tests/prep_probe, test code), which is how the probe runs the kernels that ship and not copies of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_core.h"
#include "nlzm_v2.h"

namespace nlzm {
void launch_rk_hash(const uint8_t *in, unsigned long long n, unsigned long long pos0, unsigned long long pos1,
                    uint32_t *out, hipStream_t st);
void launch_pipeline2(const Geom &g, const Globals &G, const v2::GlobalsV2 &V, uint32_t c0, uint32_t c1, uint32_t worker_blocks, hipStream_t st);
unsigned long long stream2_pack_size();
uint32_t stream2_pack_capacity();
uint32_t pipeline2_role_blocks();
void fill_stream2_args(void *host_pack, uint32_t i, const Geom &g, const Globals &G, const v2::GlobalsV2 &V, uint32_t c0, uint32_t c1, v2::RoundSnap *snap);
void launch_pipeline2_multi(const void *dev_pack, uint32_t nstreams, uint32_t worker_blocks, hipStream_t st);
void launch_round_open(const void *dev_pack, uint32_t nstreams, hipStream_t st);
void launch_round_close(const void *dev_pack, uint32_t nstreams, hipStream_t st);
void launch_prefilter(const uint8_t *in, unsigned long long n, uint32_t a0, uint32_t a1, uint32_t wmask, uint32_t t_bits, uint32_t t_bitmap,
                      uint32_t m_bits, uint32_t *T, uint32_t *M, uint32_t *hbuf, uint32_t *hbuf2, uint8_t *c1, uint8_t *unc, hipStream_t st);
unsigned long long worker_undo_bytes_per_lane();
unsigned long long worker_hot_undo_bytes_per_wave();
void launch_hot_select(const uint32_t *off, uint32_t nchunks, uint32_t nheads, uint32_t hmax, uint32_t min_count, uint32_t *hot_of_bin,
                       uint32_t *hot_list, WorkerCounters *wcnt, hipStream_t st);
void launch_bin(const uint8_t *in, const Geom &g, uint32_t c0, uint32_t nchunks, uint32_t nheads, uint32_t *off, uint32_t *cur,
                uint32_t *pos, const uint8_t *unc, uint32_t batch_a0, hipStream_t st);
void launch_rans(const uint32_t *syms, unsigned long long syms_stride, const uint8_t *bits, unsigned long long bits_stride,
                 FrameMeta *fmeta, uint32_t *scratch, unsigned long long scratch_stride, uint8_t *out,
                 unsigned long long out_stride, uint32_t out_cap, uint32_t nframes, hipStream_t st);
void launch_gather(const uint8_t *frames, unsigned long long stride, const unsigned long long *dst_off,
                   const FrameMeta *fmeta, uint8_t *dst, uint32_t nframes, hipStream_t st);
}  // namespace nlzm
