// nlzm_cut_host.h -- the two prototypes of the cut points that cross a file boundary inside the library: the launch (nlzm_cut.hip, called by
// nlzm_hip_cut.cpp) and the "cut_*" counters (nlzm_hip_cut.cpp, called by nlzm_hip_get_counter in nlzm_hip.cpp).  A header of its own, so that
// nlzm_host_util.h -- which every host file of the read side is compiled from -- is the text it was: no object of the read side has a reason to differ.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nlzm {
namespace cut { struct Args; }

void launch_cut(const cut::Args &a, uint32_t max_blocks, hipStream_t st);
int cut_counter(const char *key, uint64_t *value);

}  // namespace nlzm
