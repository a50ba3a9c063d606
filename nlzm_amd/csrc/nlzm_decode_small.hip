// nlzm_decode_small.hip -- the one-shot decoder role (nlzm_decode.h) a second time, with a 16 KiB LDS ring: decode_small_kernel.  The ring is
// all the LDS the role has, and the 64 KiB one of decode_kernel (nlzm_decode.hip) lets a CU hold two one-wave workgroups; at 16 KiB a CU's
// 160 KiB hold ten, two or three waves a SIMD (the role's 105 VGPRs would allow four), which fill each other's issue gaps.  Matches that
// reach further back than the ring come from memory, as they do behind 64 KiB.  The copy lives in a namespace of its own, nlzm::dec_small, so
// that nothing of it is shared with -- or changes -- the kernels of nlzm_decode.hip; the host side (nlzm_hip_decode.cpp) picks the kernel by the
// number of streams and fills the same StreamArgs for either.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NLZM_DEC_NS dec_small
#ifndef NLZM_DEC_RING
#define NLZM_DEC_RING 16384
#endif
#include "nlzm_decode.h"
#include "nlzm_units.h"

namespace nlzm {
// the stream's output ring: a file-scope __shared__ object, every access is a ds_* instruction
__shared__ dec_small::Lds g_dec_small_lds;
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_dec_small_lds); }
}
namespace nlzm {


// Workgroup b decodes stream b, as in decode_kernel.
__global__ __launch_bounds__(64) void decode_small_kernel(const dec_small::StreamArgs *__restrict__ args, dec_small::StreamResult *__restrict__ res)
{
    dec_small::StreamArgs a = args[blockIdx.x];
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.dst = NLZM_GLOBAL(uint8_t, a.dst);
    dec_small::decode_role(a, res + blockIdx.x);
}

void launch_decode_small(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(decode_small_kernel, dim3(nstreams), dim3(64), 0, st, (const dec_small::StreamArgs *)d_args, (dec_small::StreamResult *)d_res);
}
uint32_t decode_small_ring() { return dec_small::kRing; }

}  // namespace nlzm
