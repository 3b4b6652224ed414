// The vocabulary of the one-wavefront-per-ray kernels: composite.hip (training compositing), distortion.hip,
// normal_image.hip and the orientation term of shade.hip.  Each walks a ray's sample span with lanes on consecutive
// samples, in chunks of 64 chained through scalar carries.  What they share is defined HERE, once: the span of a ray, the
// compositing weight of a sample, the finite-difference normal and its backward projection.  The chunk loop itself (the
// cur / nxt prefetch, the per-ray sums) stays written out in every kernel.
//
// What is deliberately NOT shared, because the bits differ:
//   - dL/dtau_i = g_i T_{i+1} - sum_{k>i} g_k w_k is  fmaf(g, Te, -(total - pinc))  in the compositing backward and
//     g * Te - (total - pinc)  in the distortion and normal-image backwards.  The compositing predates the "no explicit
//     fmaf" contract of the later terms (f32 + - * / sqrt in the stated order, so that a numpy restatement follows them
//     operation by operation), and its bits are pinned by byte comparisons of whole training runs; the later terms' are
//     pinned by their restatements.  One rounding apart, neither can take the other's form.
//   - how a kernel adds its per-ray sums (fmaf or not, which scans, the order of the carries): same reason.
#pragma once
#include "common.h"

namespace lnerf {

// lane 63's value in every lane: the chunk total of an inclusive scan
__device__ __forceinline__ float lane63(float v) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Optical depth in front of this lane's sample, from the chunk's inclusive scan `inc` and the depth `carry` of the chunks
// before it: the NEIGHBOURING lane's inclusive sum (lane 0: nothing), never `inc - tau`.  The lane's own tau can be
// arbitrarily large (sigma = exp(h) is unclamped, a surface sample has sigma dt ~ 1e4 and more); subtracting it back out
// of a sum that contains it rounds the small prefix in front of it away (error 2^-24 tau in excl, i.e. in T and the
// weight; inf - inf = NaN at sigma = +inf).
__device__ __forceinline__ float exclusive_depth(float inc, float carry) { return lane_prev_f(inc, 0.f) + carry; }

// row r of the march's ray table: the ray's id and the span [off, off + cnt) of its samples
struct RaySpan {
    int64_t id, off;
    int cnt;
};
__device__ __forceinline__ RaySpan load_span(const int32_t *__restrict__ rays, int64_t r) {
    return {rays[r * 3], rays[r * 3 + 1], rays[r * 3 + 2]};
}
// row `row` of a [rows, C] f32 array: one 16-byte access for the four latent channels (the callers check the alignment)
template <int C>
__device__ __forceinline__ void load_row(const float *p, int64_t row, float (&v)[C]) {
    if (C == 4) {
        const float4 q = reinterpret_cast<const float4 *>(p)[row];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[C - 1] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p[row * C + c];
    }
}
template <int C>
__device__ __forceinline__ void store_row(float *p, int64_t row, const float (&v)[C]) {
    if (C == 4) {
        reinterpret_cast<float4 *>(p)[row] = make_float4(v[0], v[1], v[2], v[C - 1]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) p[row * C + c] = v[c];
    }
}

// (dt, t) of sample s: the march's 8-byte pair as ONE load.  Like load_row and load_fd_rows it does not test the span's end:
// a chunk loader zero-fills its record and puts all its loads under one `i < cnt` (one exec region, not one per array).
struct Step {
    float dt, t;
};
__device__ __forceinline__ Step load_step(const float *__restrict__ deltas, int64_t s) {
    const float2 d = reinterpret_cast<const float2 *>(deltas)[s];
    return {d.x, d.y};
}

// ---- THE compositing weight.  With tau_i = sigma_i dt_i of this lane's sample (zero on a lane past the span), `carry`
// the optical depth of the chunks before this one:
//   T_i = expf(-(depth in front of i)),  e_i = expf(-tau_i),  live_i = valid && T_i >= T_thresh,
//   w_i = live_i ? (1 - e_i) T_i : 0,    Te_i = T_i e_i = T_{i+1},   carry += the chunk's tau total.
// Called by ALL 64 lanes (a wave scan); a lane past the span gives w = 0.  There is no early stop in here: behind
// T < T_thresh the weights are 0 and the carry goes on; a kernel that stops there (the compositing does, T is monotone
// along the ray) tests the carry this function advanced.  A NaN T is not live (the comparison is false), a NaN tau with a
// live T gives a NaN weight: nothing is clamped.  Every backward recomputes the forward's `live` through this same code,
// which is what makes the two agree bit for bit.
struct SpanWeight {
    float w, Te;
    bool live;
};
__device__ __forceinline__ SpanWeight span_weight(float tau, bool valid, float T_thresh, float &carry) {
    SpanWeight o;
    const float inc = wave_inclusive_sum(tau);
    const float excl = exclusive_depth(inc, carry);
    const float T = expf(-excl);
    const float e = expf(-tau);
    const float alpha = 1.0f - e;
    o.live = valid && T >= T_thresh;
    o.w = o.live ? alpha * T : 0.f;
    o.Te = T * e;
    carry += lane63(inc);
    return o;
}

// ---- the finite-difference normal of a sample from its seven densities (the sample and its +-eps neighbours along x, y,
// z: rows 7 i .. 7 i + 6 of sigmas7), f32 + - * / sqrt in the stated order, no fmaf
constexpr int FD_ROWS = 7;

// the seven densities of the sample whose first row is s7
__device__ __forceinline__ void load_fd_rows(const float *__restrict__ sigmas7, int64_t s7, float (&sg)[FD_ROWS]) {
#pragma unroll
    for (int j = 0; j < FD_ROWS; ++j) sg[j] = sigmas7[s7 + j];
}

// n = -g / |g| with g the central differences, s = |g|^2, r = 1 / sqrt(max(s, 1e-20)); a NaN component of n becomes 0
struct FdNormal {
    float n[3], s, r;
};
__device__ __forceinline__ FdNormal fd_normal(const float (&sg)[FD_ROWS], float inv_2eps) {
    FdNormal o;
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = (sg[1 + 2 * a] - sg[2 + 2 * a]) * inv_2eps;
    o.s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    o.r = 1.0f / sqrtf(fmaxf(o.s, 1e-20f));          // (fmaxf: a NaN s gives the floor)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = -(g[a] * o.r);
        o.n[a] = v != v ? 0.f : v;
    }
    return o;
}

// Its backward: dn = dL/dn -> the gradient of the six offset densities, rows 1..6 of the sample's seven, through
// n = -g / |g| (the projection onto the tangent plane is skipped where the floor held, s <= 1e-20 or NaN).
struct FdGrad {
    float row[FD_ROWS - 1];
};
__device__ __forceinline__ FdGrad fd_normal_backward(const FdNormal &o, const float (&dn)[3], float inv_2eps) {
    FdGrad d;
    const float ndn = (o.n[0] * dn[0] + o.n[1] * dn[1]) + o.n[2] * dn[2];
    const bool project = o.s > 1e-20f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = project ? dn[a] - o.n[a] * ndn : dn[a];
        const float dg = -(o.r * t);
        const float v = dg * inv_2eps;
        d.row[2 * a] = v;
        d.row[2 * a + 1] = -v;
    }
    return d;
}
// the seven dsigmas7 rows of the sample whose first row is s7: the centre's gradient, then the six offsets'
__device__ __forceinline__ void store_fd_rows(float *__restrict__ dsigmas7, int64_t s7, float centre, const FdGrad &d) {
    dsigmas7[s7] = centre;
#pragma unroll
    for (int j = 1; j < FD_ROWS; ++j) dsigmas7[s7 + j] = d.row[j - 1];
}

}  // namespace lnerf
