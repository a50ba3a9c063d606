// nlzm_elem_host.h -- the two prototypes of the element-size statistic that cross a file boundary inside the library: the launches (nlzm_elem.hip,
// called by nlzm_hip_elem.cpp) and the "elem_*" counters (nlzm_hip_elem.cpp, called by nlzm_hip_get_counter in nlzm_hip.cpp).  A header of its own, as
// nlzm_planes_host.h is.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nlzm {
namespace elem { struct Args; }

void launch_elem(const elem::Args &a, uint32_t max_blocks, hipStream_t st);
int elem_counter(const char *key, uint64_t *value);

}  // namespace nlzm
