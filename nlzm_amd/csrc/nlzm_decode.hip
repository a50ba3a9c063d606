// nlzm_decode.hip -- the decoder's kernels for gfx950: the decoder role (nlzm_decode.h) one workgroup of one wave per stream, one-shot
// (decode_kernel) and in steps that stop at a frame boundary and resume (decode_steps_kernel), the hop
// over the frame headers that splits a back-to-back container, and the compare of verify.  Nothing here is shared with the compress
// pipeline (nlzm_kernels.hip); the host side is nlzm_hip_decode.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlzm_decode.h"
#include "nlzm_units.h"

namespace nlzm {
// the stream's output ring: a file-scope __shared__ object, every access is a ds_* instruction
__shared__ dec::Lds g_dec_lds;
}  // namespace nlzm
namespace xw {
template <class T> XW_FN T *lds() { return reinterpret_cast<T *>(&nlzm::g_dec_lds); }
}
namespace nlzm {


// Workgroup b decodes stream b.  More streams than the device has room for wait in the dispatcher and start as workgroups end.
__global__ __launch_bounds__(64) void decode_kernel(const dec::StreamArgs *__restrict__ args, dec::StreamResult *__restrict__ res)
{
    dec::StreamArgs a = args[blockIdx.x];
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.dst = NLZM_GLOBAL(uint8_t, a.dst);
    dec::decode_role(a, res + blockIdx.x);
}

// The stepping form of the same role (dec::decode_role_steps): workgroup b takes stream b up to its next pause or its end.  A kernel of its
// own, so that decode_kernel stays the code it was.
__global__ __launch_bounds__(64) void decode_steps_kernel(const dec::StreamArgs *__restrict__ args, dec::StreamResult *__restrict__ res)
{
    dec::StreamArgs a = args[blockIdx.x];
    a.src = NLZM_GLOBAL(const uint8_t, a.src);
    a.dst = NLZM_GLOBAL(uint8_t, a.dst);
    a.state = NLZM_GLOBAL(dec::StepState, a.state);
    dec::decode_role_steps(a, res + blockIdx.x);
}

// the split of a container in device memory (dec::split_walk, nlzm_decode.h): one lane follows the sizes the frame headers carry
__global__ __launch_bounds__(64) void split_kernel(const uint8_t *__restrict__ src, unsigned long long len, uint32_t nblocks,
                                                   unsigned long long *__restrict__ block_len, uint32_t *__restrict__ bad)
{
    if (threadIdx.x || blockIdx.x) return;
    dec::split_walk(src, len, nblocks, block_len, bad);
}

// verify: *first = min(*first, the first offset below n at which a and b differ).  Sixteen bytes per lane and step (one 16-byte load
// each where both pointers are aligned), the minimum by an agent-scope atomic.
__global__ __launch_bounds__(256) void compare_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, unsigned long long n,
                                                      unsigned long long *__restrict__ first)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const bool aligned = ((((unsigned long long)a) | ((unsigned long long)b)) & 15ull) == 0;
    const unsigned long long stride = 16ull * gridDim.x * blockDim.x;
    for (unsigned long long p = 16ull * (blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x); p < n; p += stride) {
        const uint32_t m = n - p < 16 ? (uint32_t)(n - p) : 16u;
        uint32_t diff = 16;
        if (aligned && m == 16) {
            const u4 x = *(const u4 *)(a + p), y = *(const u4 *)(b + p);
            if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) {
#pragma unroll
                for (int w = 3; w >= 0; w--) { const uint32_t d = x[w] ^ y[w]; if (d) diff = 4 * w + ((uint32_t)__builtin_ctz(d) >> 3); }
            }
        } else {
            for (uint32_t k = m; k-- > 0;) if (a[p + k] != b[p + k]) diff = k;
        }
        if (diff < m) (void)__hip_atomic_fetch_min(first, p + diff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void launch_decode(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(decode_kernel, dim3(nstreams), dim3(64), 0, st, (const dec::StreamArgs *)d_args, (dec::StreamResult *)d_res);
}
void launch_decode_steps(const void *d_args, void *d_res, uint32_t nstreams, hipStream_t st)
{
    hipLaunchKernelGGL(decode_steps_kernel, dim3(nstreams), dim3(64), 0, st, (const dec::StreamArgs *)d_args, (dec::StreamResult *)d_res);
}
void launch_split(const void *d_src, unsigned long long len, uint32_t nblocks, unsigned long long *d_block_len, uint32_t *d_bad, hipStream_t st)
{
    hipLaunchKernelGGL(split_kernel, dim3(1), dim3(64), 0, st, (const uint8_t *)d_src, len, nblocks, d_block_len, d_bad);
}
void launch_compare(const void *d_a, const void *d_b, unsigned long long n, unsigned long long *d_first, hipStream_t st)
{
    const unsigned long long want = (n / 16 + 255) / 256 + 1;
    hipLaunchKernelGGL(compare_kernel, dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0, st, (const uint8_t *)d_a, (const uint8_t *)d_b, n, d_first);
}

}  // namespace nlzm
