// nlzm_dedup_host.h -- the prototypes of the equal-range finder that cross a file boundary inside the library: the launches (nlzm_dedup.hip, called by
// nlzm_hip_dedup.cpp), the "dedup_*" counters and the two options (nlzm_hip_dedup.cpp, called by nlzm_hip_get_counter and nlzm_hip_set_option in
// nlzm_hip.cpp), and what nlzm_hip_compress_ranges_dev (nlzm_hip_blocks.cpp) calls when "dedup_ranges" is set.  A header of its own, as nlzm_cut_host.h
// is, so that nlzm_host_util.h and nlzm_host_state.h are the texts they were: no object of the read side or of the rest of the compress side has a
// reason to differ.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nlzm {
namespace dedup { struct FpArgs; struct PairArgs; }

void launch_fingerprints(const dedup::FpArgs &a, uint32_t max_blocks, hipStream_t st);
void launch_pairs(const dedup::PairArgs &a, uint32_t max_blocks, hipStream_t st);
int dedup_counter(const char *key, uint64_t *value);
// "dedup_ranges" (0 / 1) and "test_dedup_hash_bits" (0 .. 64): 0 when the key is one of them and the value was taken, NLZM_HIP_E_ARG with the
// library's text when its value is out of range, 1 when the key is not one of them
int dedup_set_option(const char *key, int64_t value);
bool dedup_ranges_option();
// first_of (k entries) of k checked ranges of the buf_len bytes at d_buf, on the library's stream; the "dedup_*" counters describe it
int dedup_first_of(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint32_t *first_of);
// k pieces copied inside device memory in ONE launch of the range reader's gather role: len[i] bytes from d_from + from[i] to d_to + to[i]
// (the destinations do not overlap); its device time is added to "dedup_gather_us"
int dedup_place(const uint8_t *d_from, uint8_t *d_to, uint32_t k, const uint64_t *from, const uint64_t *to, const uint64_t *len);

}  // namespace nlzm
