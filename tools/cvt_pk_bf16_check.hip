// Diagnostic: does v_cvt_pk_bf16_f32 (what a float2 -> bf16x2 conversion compiles to on gfx950) equal f32_to_bf16
// (csrc/common.h: round to nearest even, a NaN quieted with sign and payload kept) on ALL 2^32 inputs, in both halves?
// The gather's feature store relies on it (csrc/grid_gather.hip, bf16_pair).  Every input u goes through the low half
// and ~u through the high half.  A second of GPU time; exit status 0 = equal everywhere, 1 = a mismatch (printed).
//     hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -o cvt_pk_bf16_check tools/cvt_pk_bf16_check.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// out[0] = mismatches (saturating count), out[1] = first mismatching input seen, out[2] = hw, out[3] = sw
__global__ void __launch_bounds__(256) k_check(unsigned int *out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;   // 2^20 threads x 4096 inputs
    for (uint32_t k = 0; k < 4096u; ++k) {
        const uint32_t u = t * 4096u + k;
        const float a = __uint_as_float(u), b = __uint_as_float(~u);
        f32x2 v = {a, b};
        bf16x2 h = __builtin_convertvector(v, bf16x2);
        uint32_t hw;
        __builtin_memcpy(&hw, &h, 4);
        const uint32_t sw = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
        if (hw != sw) {
            if (atomicAdd(&out[0], 1u) == 0u) { out[1] = u; out[2] = hw; out[3] = sw; }
        }
    }
}

int main() {
    unsigned int *d = nullptr, h[4] = {0, 0, 0, 0};
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return 2;
    hipLaunchKernelGGL(k_check, dim3(4096), dim3(256), 0, 0, d);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("cvt_check: mismatches %u first input 0x%08x hw 0x%08x sw 0x%08x\n", h[0], h[1], h[2], h[3]);
    return h[0] ? 1 : 0;
}
