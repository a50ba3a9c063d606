// nlzm_planes_host.h -- the two prototypes of the byte-plane filter that cross a file boundary inside the library: the launch (nlzm_planes.hip, called
// by nlzm_hip_planes.cpp) and the "planes_*" counters (nlzm_hip_planes.cpp, called by nlzm_hip_get_counter in nlzm_hip.cpp).  A header of its own, as
// nlzm_cut_host.h is, so that nlzm_host_util.h is the text it was.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nlzm {
namespace planes { struct Args; }

void launch_planes(const planes::Args &a, bool inverse, uint32_t max_blocks, hipStream_t st);
int planes_counter(const char *key, uint64_t *value);

}  // namespace nlzm
