// Adam arithmetic shared by the optimiser kernels (optim.hip) and the scatter's fused table update (grid.hip):
// one definition, so that both paths produce bit-identical parameters.
#pragma once
#include "common.h"

namespace lnerf {

// The bias corrections of ONE step as data (lnerf_adam_constants_bind): whoever advances a bound device step counter
// evaluates adam_bias_at for the new value and leaves the result here, tagged with that value; every kernel that reads
// the counter reads the record with it and, where the tag equals the step it has read, takes the four numbers instead
// of two powf and two divisions per lane.  The numbers ARE adam_bias_at's (one definition, evaluated by one thread), so
// both forms produce the same bits.  A tag that differs -- a counter written from the host, a record nobody has filled
// yet -- is the cold arm: adam_bias_at as before.
struct AdamConsts {
    float bc1, bc2, inv_bc1, inv_bc2;
    int32_t tag;         // the step the four values belong to (-1: none)
    int32_t pad[3];
};
static_assert(sizeof(AdamConsts) == LNERF_ADAM_CONSTANTS_BYTES, "the record's size is part of the C ABI");

struct AdamArgs {
    float lr, beta1, beta2, eps, bc1, bc2, grad_scale;
    float inv_bc1, inv_bc2;   // 1 / bias corrections (per launch, not per element)
    int zero_grad;
    const int32_t *step_dev;  // optional device-side step counter (hipGraph replays): overrides bc1/bc2
    AdamConsts *consts;       // optional: the record bound to step_dev (for these betas), else null
};

// bias corrections from the device step counter (same value in every thread; a handful of SALU/VALU ops)
__device__ __forceinline__ void adam_bias_at(AdamArgs &a, int32_t step) {
    const float t = (float)step;
    a.bc1 = 1.0f - powf(a.beta1, t);
    a.bc2 = 1.0f - powf(a.beta2, t);
    a.inv_bc1 = 1.0f / a.bc1;
    a.inv_bc2 = 1.0f / a.bc2;
}
// The record as a kernel requests it, next to the counter: device-scope atomic loads like the counter's own (the last
// workgroup of a ticking launch rewrites both once every workgroup has arrived, i.e. has these values in registers).
// No record: tag -1, which no step equals.
__device__ __forceinline__ AdamConsts adam_consts_request(const AdamConsts *c) {
    AdamConsts r;
    r.bc1 = r.bc2 = r.inv_bc1 = r.inv_bc2 = 0.f;
    r.tag = -1;
    if (c) {
        r.bc1 = __hip_atomic_load(&c->bc1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.bc2 = __hip_atomic_load(&c->bc2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.inv_bc1 = __hip_atomic_load(&c->inv_bc1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.inv_bc2 = __hip_atomic_load(&c->inv_bc2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.tag = __hip_atomic_load(&c->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return r;
}
// the bias corrections of `step`: the record's where it is this step's, else computed (uniform, cold)
__device__ __forceinline__ void adam_bias_from(AdamArgs &a, int32_t step, const AdamConsts &r) {
    if (r.tag == step) {
        a.bc1 = r.bc1; a.bc2 = r.bc2; a.inv_bc1 = r.inv_bc1; a.inv_bc2 = r.inv_bc2;
    } else {
        adam_bias_at(a, step);
    }
}
// ONE thread, when it has advanced the counter to `step`: the values first, the tag last.  No fence (DESIGN.md section
// 10): the readers are later launches, or workgroups of this launch that have all arrived.
__device__ __forceinline__ void adam_consts_publish(AdamArgs a, int32_t step) {
    if (!a.consts) return;
    adam_bias_at(a, step);
    __hip_atomic_store(&a.consts->bc1, a.bc1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.consts->bc2, a.bc2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.consts->inv_bc1, a.inv_bc1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.consts->inv_bc2, a.inv_bc2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.consts->tag, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void adam_bias(AdamArgs &a) {
    if (a.step_dev) {
        const AdamConsts r = adam_consts_request(a.consts);
        adam_bias_from(a, *a.step_dev, r);
        return;
    }
    a.inv_bc1 = 1.0f / a.bc1;
    a.inv_bc2 = 1.0f / a.bc2;
}

__device__ __forceinline__ void adam_one(float &p, float &g, float &m, float &v, const AdamArgs &a) {
    const float gs = g * a.grad_scale;
    m = fmaf(a.beta1, m, (1.0f - a.beta1) * gs);
    v = fmaf(a.beta2, v, (1.0f - a.beta2) * gs * gs);
    // bias corrections as multiplications by per-launch reciprocals, the final quotient through v_sqrt_f32 / v_rcp_f32
    // (1 ulp each): the element-wise divisions were a quarter of the fused reduce + Adam pass's vector instructions.
    // Against float64 Adam (tests/test_gpu_adam.py, gradients 1e-30 .. 1e4, warm moments, t = 1 .. 20000; u = 2^-24): a
    // count of the roundings bounds the update term's error by 14 u of itself plus m's error carried through
    // (tests/adam_reference.py adam_bounds); measured where vhat is normal and m does not cancel: 5.4 u with the host's
    // bias corrections, 12.9 u with the device step counter's (1 - powf: cancellation at small t).  v_sqrt_f32 reads a
    // subnormal vhat as zero: the denominator is eps instead of sqrt(vhat) + eps there, < 2^-63 / eps = 1.1e-4 of the
    // update at eps = 1e-15 (measured: 0.99 of that) -- rows whose vhat is below 1.2e-38, i.e. gradients around 1e-19.
    const float mhat = m * a.inv_bc1;
    const float vhat = v * a.inv_bc2;
    p = p - (a.lr * mhat) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vhat) + a.eps);
    if (a.zero_grad) g = 0.f;
}

// host side: the record bound to a counter for these betas and the "adam_consts" form switch (optim.hip); null otherwise
AdamConsts *adam_consts_lookup(const int32_t *step_dev, float beta1, float beta2);
extern int g_adam_consts;

// host side: bias corrections for a host-side step number (overridden on the device when step_dev is set)
static inline void adam_host_args(AdamArgs &a, float lr, float beta1, float beta2, float eps, int step,
                                  const int32_t *step_dev, float grad_scale, int zero_grad) {
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.bc1 = (float)(1.0 - pow((double)beta1, (double)(step < 1 ? 1 : step)));
    a.bc2 = (float)(1.0 - pow((double)beta2, (double)(step < 1 ? 1 : step)));
    a.inv_bc1 = 1.0f / a.bc1;
    a.inv_bc2 = 1.0f / a.bc2;
    a.grad_scale = grad_scale;
    a.zero_grad = zero_grad;
    a.step_dev = step_dev;
    a.consts = adam_consts_lookup(step_dev, beta1, beta2);
}

}  // namespace lnerf
