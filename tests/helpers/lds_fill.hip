// Test support (tests/test_gpu_mlp_shapes.py): fill every CU's LDS with one 32-bit pattern, so that a kernel launched behind it
// on the same stream starts on LDS holding that pattern instead of whatever ran before.  Each workgroup declares all 160 KiB of
// a gfx950 CU's LDS (one workgroup per CU at a time) and writes only that; the grid is several times the CU count, so every CU
// takes at least one of them.  The stores are volatile (nothing reads them back, and the compiler must not drop them).
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int LDS_WORDS = 160 * 1024 / 4;

__global__ __launch_bounds__(1024) void lds_fill_kernel(uint32_t value, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[LDS_WORDS];
    volatile uint32_t* v = lds;
    for (int i = threadIdx.x; i < LDS_WORDS; i += blockDim.x) v[i] = value;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = v[(blockIdx.x * 977u) % LDS_WORDS];  // (one word back: the workgroup's own store)
}

// out: `blocks` uint32 words of device memory.  Returns a hipError_t.
extern "C" int lds_fill(uint32_t value, int blocks, void* out, void* stream) {
    hipLaunchKernelGGL(lds_fill_kernel, dim3(blocks), dim3(1024), 0, static_cast<hipStream_t>(stream), value,
                       static_cast<uint32_t*>(out));
    return (int)hipGetLastError();
}
