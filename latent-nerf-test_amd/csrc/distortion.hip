// Distortion loss of the training renders (mip-NeRF 360's L_dist on the march's samples), forward + backward.
// Contract and order of operations: include/lnerf_hip.h, "distortion loss"; numpy restatement: tests/distortion_reference.py.
//
// One wavefront per ray, lanes on consecutive samples of the ray's span, chunks of 64 chained through scalar carries --
// the shape of the training compositing (composite.hip).  The weights are the compositing's (span_walk.h, span_weight),
// and here they are NOT detached: the backward is the compositing backward's identity with g_i = dL/dw_i of this term.
// No LDS, no atomics: every output element has one writer.
#include "span_walk.h"

namespace lnerf {

// one lane's sample of a 64-sample chunk (zeros past the end of the span)
struct DistChunk {
    float sigma, dt, t;
};
__device__ __forceinline__ DistChunk load_dist_chunk(const float *__restrict__ sigmas, const float *__restrict__ deltas,
                                                     int64_t off, int cnt, int i) {
    DistChunk k = {0.f, 0.f, 0.f};
    if (i < cnt) {
        const Step d = load_step(deltas, off + i);
        k.dt = d.dt; k.t = d.t;
        k.sigma = sigmas[off + i];
    }
    return k;
}

// What one chunk of a ray knows about this lane's sample, and the three carries it moves forward.  Called by ALL 64 lanes
// (wave scans); lanes past the span carry w = 0.
struct DistTerms : SpanWeight {   // the compositing weight: w, Te = T_{i+1}, live
    float m, dt, u;               // shifted mid-point, dt, u = m A - B
};
struct DistCarry {
    float tau, A, B;         // optical depth, sum of w, sum of w m of the chunks before this one
};
__device__ __forceinline__ DistTerms dist_terms(const DistChunk &k, bool valid, float t0, float T_thresh, DistCarry &c) {
    DistTerms o = {span_weight(k.sigma * k.dt, valid, T_thresh, c.tau)};
    o.dt = k.dt;
    o.m = (k.t - t0) + 0.5f * k.dt;
    const float wm = o.w * o.m;
    const float incA = wave_inclusive_sum(o.w);
    const float incB = wave_inclusive_sum(wm);
    const float A = lane_prev_f(incA, 0.f) + c.A;     // exclusive: the neighbouring lane's inclusive sum
    const float B = lane_prev_f(incB, 0.f) + c.B;
    o.u = o.m * A - B;
    c.A += lane63(incA);
    c.B += lane63(incB);
    return o;
}

// loss[id] = sum_i w_i (2 (m_i A_i - B_i) + (1/3) w_i dt_i);  sums[id] = (A_tot, B_tot) for the backward.
// A ray without samples writes zeros (the buffers are uninitialised): no early return before the stores.
__global__ void __launch_bounds__(256)
k_distortion_fwd(const float *__restrict__ sigmas, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                 int64_t N, float T_thresh, float *__restrict__ loss, float *__restrict__ sums) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    const float third = 1.0f / 3.0f;
    DistCarry c = {0.f, 0.f, 0.f};
    float acc = 0.f, t0 = 0.f;
    if (cnt > 0) t0 = deltas[off * 2 + 1];
    DistChunk cur = load_dist_chunk(sigmas, deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        DistChunk nxt = cur;    // the next chunk's inputs, requested before this chunk's scans
        if (base + 64 < cnt) nxt = load_dist_chunk(sigmas, deltas, off, cnt, base + 64 + lane);
        const DistTerms o = dist_terms(cur, base + lane < cnt, t0, T_thresh, c);
        acc += o.w * (2.0f * o.u + third * (o.w * o.dt));
        cur = nxt;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        loss[id] = acc;
        sums[id * 2] = c.A;
        sums[id * 2 + 1] = c.B;
    }
}

// dsigmas of every sample of every span.  One forward sweep: with (A_tot, B_tot) and L of the forward,
//   g_i = 2 (2 u_i + (B_tot - m_i A_tot)) + (2/3) w_i dt_i,   sum_{j > i} g_j w_j = 2 L - (inclusive prefix of g w).
__global__ void __launch_bounds__(256)
k_distortion_bwd(const float *__restrict__ sigmas, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                 int64_t N, float T_thresh, const float *__restrict__ d_loss, const float *__restrict__ loss,
                 const float *__restrict__ sums, float *__restrict__ dsigmas) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    if (cnt <= 0) return;
    const float two_thirds = 2.0f / 3.0f;
    const float go = d_loss[id];
    const float A_tot = sums[id * 2], B_tot = sums[id * 2 + 1];
    const float total = loss[id] + loss[id];
    const float t0 = deltas[off * 2 + 1];
    DistCarry c = {0.f, 0.f, 0.f};
    float carry_g = 0.f;
    DistChunk cur = load_dist_chunk(sigmas, deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        DistChunk nxt = cur;
        if (base + 64 < cnt) nxt = load_dist_chunk(sigmas, deltas, off, cnt, base + 64 + lane);
        const int i = base + lane;
        const bool valid = i < cnt;
        const DistTerms o = dist_terms(cur, valid, t0, T_thresh, c);
        const float g = 2.0f * ((o.u + o.u) + (B_tot - o.m * A_tot)) + two_thirds * (o.w * o.dt);
        const float pinc = wave_inclusive_sum(g * o.w) + carry_g;
        if (valid) {
            // dL/dtau_i = g_i T_{i+1} - sum_{j>i} g_j w_j
            const float dtau = o.live ? g * o.Te - (total - pinc) : 0.f;
            dsigmas[off + i] = (go * o.dt) * dtau;
        }
        carry_g = lane63(pinc);
        cur = nxt;
    }
}

}  // namespace lnerf

using namespace lnerf;

static int check_distortion(const char *name, const float *sigmas, const float *deltas, const int32_t *rays, int64_t N,
                            float T_thresh) {
    LNERF_REQUIRE(N >= 0, "%s: negative N", name);
    LNERF_REQUIRE(T_thresh >= 0.f && T_thresh < 1.f, "%s: T_thresh must be in [0, 1)", name);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(sigmas && deltas && rays, "%s: null pointer (sigmas / deltas / rays)", name);
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0, "%s: deltas must be 8-byte aligned", name);
    return LNERF_OK;
}

extern "C" {

int lnerf_distortion_forward(const float *sigmas, const float *deltas, const int32_t *rays, int64_t N, float T_thresh,
                             float *loss, float *ray_sums, lnerf_stream_t stream) {
    if (check_distortion("distortion_forward", sigmas, deltas, rays, N, T_thresh) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(loss && ray_sums, "distortion_forward: null pointer (loss / ray_sums)");
    hipLaunchKernelGGL(k_distortion_fwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream), sigmas, deltas, rays,
                       N, T_thresh, loss, ray_sums);
    LNERF_CHECK_LAUNCH("distortion_forward");
    return LNERF_OK;
}

int lnerf_distortion_backward(const float *sigmas, const float *deltas, const int32_t *rays, int64_t N, float T_thresh,
                              const float *d_loss, const float *loss, const float *ray_sums, float *dsigmas,
                              lnerf_stream_t stream) {
    if (check_distortion("distortion_backward", sigmas, deltas, rays, N, T_thresh) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(d_loss && loss && ray_sums && dsigmas, "distortion_backward: null pointer (d_loss / loss / ray_sums / dsigmas)");
    hipLaunchKernelGGL(k_distortion_bwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream), sigmas, deltas, rays,
                       N, T_thresh, d_loss, loss, ray_sums, dsigmas);
    LNERF_CHECK_LAUNCH("distortion_backward");
    return LNERF_OK;
}

}  // extern "C"
