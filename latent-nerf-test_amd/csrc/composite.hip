// H8/H9 front-to-back alpha compositing, training form (forward + backward).
//
// One wavefront per ray: lanes take consecutive samples of the ray's span (coalesced loads),
// transmittance comes from a log-space prefix scan of tau = sigma*dt across the 64 lanes with
// a scalar carry between 64-sample chunks, and the per-ray sums are wave reductions.
// The early stop "T < T_thresh" is wave-uniform because T is monotone along the ray.
// The weight itself (span_weight) and the span vocabulary live in span_walk.h, shared with the regularisers that weight
// samples the way this image does.
#include "span_walk.h"

namespace lnerf {

// one lane's sample of a 64-sample chunk (zeros past the end of the span)
template <int C>
struct Chunk {
    float sigma, dt, t, rgb[C];
};
template <int C>
__device__ __forceinline__ Chunk<C> load_chunk(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                               const float *__restrict__ deltas, int64_t off, int cnt, int base, int lane) {
    Chunk<C> k;
    k.sigma = 0.f; k.dt = 0.f; k.t = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) k.rgb[c] = 0.f;
    const int i = base + lane;
    if (i < cnt) {
        const int64_t s = off + i;
        const Step d = load_step(deltas, s);
        k.dt = d.dt; k.t = d.t;
        k.sigma = sigmas[s];
        load_row<C>(rgbs, s, k.rgb);
    }
    return k;
}

// One ray's forward loop over its span: each lane's share of weights_sum, depth and the C colour sums (no background);
// the caller adds them across the wave.
template <int C>
__device__ __forceinline__ void composite_ray_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                  const float *__restrict__ deltas, int64_t off, int cnt, float T_thresh,
                                                  int lane, float &a_ws, float &a_d, float (&a_c)[C]) {
    a_ws = 0.f; a_d = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) a_c[c] = 0.f;
    float carry = 0.f;
    // The chunks of a ray are a chain through `carry`, but their INPUTS are not: the next chunk's sigma, (dt, t) and
    // latents are requested before this chunk is processed (the kernel is a few dependent memory round trips long,
    // nothing else), each as one load (8-byte delta pair, 16-byte latent row).
    Chunk<C> cur = load_chunk<C>(sigmas, rgbs, deltas, off, cnt, 0, lane);
    for (int base = 0; base < cnt; base += 64) {
        Chunk<C> nxt = cur;
        if (base + 64 < cnt) nxt = load_chunk<C>(sigmas, rgbs, deltas, off, cnt, base + 64, lane);
        const float tau = cur.sigma * cur.dt;     // (invalid lanes carry zeros)
        const float w = span_weight(tau, base + lane < cnt, T_thresh, carry).w;
        a_ws += w;
        a_d = fmaf(w, cur.t, a_d);
        if (w != 0.f) {
#pragma unroll
            for (int c = 0; c < C; ++c) a_c[c] = fmaf(w, cur.rgb[c], a_c[c]);
        }
        if (expf(-carry) < T_thresh) break;  // every later sample starts below the threshold
        cur = nxt;
    }
}

template <int C>
__global__ void __launch_bounds__(256)
k_composite_train_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                      const int32_t *__restrict__ rays, int64_t N, float T_thresh, const float *__restrict__ bg,
                      float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    float a_ws, a_d, a_c[C];
    composite_ray_fwd<C>(sigmas, rgbs, deltas, off, cnt, T_thresh, lane, a_ws, a_d, a_c);
    a_ws = wave_sum(a_ws);
    a_d = wave_sum(a_d);
#pragma unroll
    for (int c = 0; c < C; ++c) a_c[c] = wave_sum(a_c[c]);
    if (lane == 0) {
        weights_sum[id] = a_ws;
        depth[id] = a_d;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v = a_c[c];
            if (bg) v = fmaf(1.0f - a_ws, bg[id * C + c], v);
            image[id * C + c] = v;
        }
    }
}

// RGB of one ray / pixel from its composited latents L and weights_sum (the refinement stage's decoder D, f32 [3][4], no
// bias):  image_c = (sum_j D[c][j] L_j + ws) / 2 + (1 - ws) bg_c  -- the per-ray form of compositing (D z_k + 1) / 2.
__device__ __forceinline__ void decode_pixel(const float *__restrict__ D, const float (&L)[4], float ws,
                                             const float *__restrict__ bg, float *__restrict__ image) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = D[c * 4] * L[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) v = fmaf(D[c * 4 + j], L[j], v);
        v = 0.5f * (v + ws);
        if (bg) v = fmaf(1.0f - ws, bg[c], v);
        image[c] = v;
    }
}

// The C = 4 forward with the decoder in lane 0's epilogue: latent_image (no background) and the decoded RGB image.
__global__ void __launch_bounds__(256)
k_composite_train_decode_fwd(const float *__restrict__ sigmas, const float *__restrict__ latents,
                             const float *__restrict__ deltas, const int32_t *__restrict__ rays, int64_t N, float T_thresh,
                             const float *__restrict__ decoder, const float *__restrict__ bg,
                             float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ latent_image,
                             float *__restrict__ image) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    float a_ws, a_d, a_c[4];
    composite_ray_fwd<4>(sigmas, latents, deltas, off, cnt, T_thresh, lane, a_ws, a_d, a_c);
    a_ws = wave_sum(a_ws);
    a_d = wave_sum(a_d);
#pragma unroll
    for (int c = 0; c < 4; ++c) a_c[c] = wave_sum(a_c[c]);
    if (lane == 0) {
        weights_sum[id] = a_ws;
        depth[id] = a_d;
        reinterpret_cast<float4 *>(latent_image)[id] = make_float4(a_c[0], a_c[1], a_c[2], a_c[3]);
        decode_pixel(decoder, a_c, a_ws, bg ? bg + id * 3 : nullptr, image + id * 3);
    }
}

// The inference loop's epilogue: one thread per pixel.
__global__ void __launch_bounds__(256)
k_decode_image(const float *__restrict__ latent_image, const float *__restrict__ weights_sum,
               const float *__restrict__ decoder, const float *__restrict__ bg, int64_t N, float *__restrict__ image) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4 v = reinterpret_cast<const float4 *>(latent_image)[i];
    const float L[4] = {v.x, v.y, v.z, v.w};
    decode_pixel(decoder, L, weights_sum[i], bg ? bg + i * 3 : nullptr, image + i * 3);
}

// total = sum_k g_k w_k of one ray, from the forward outputs (g_k = dws + ddp t_k + sum_c di_c (rgb_kc - bg_c))
template <int C>
__device__ __forceinline__ float ray_total(float dws, float ddp, float ws, float depth, const float (&di)[C],
                                           const float (&bgc)[C], const float *__restrict__ image) {
    float total = fmaf(ddp, depth, dws * ws);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float fg = image[c] - (1.0f - ws) * bgc[c];  // sum_k w_k rgb_kc
        total = fmaf(di[c], fg - bgc[c] * ws, total);
    }
    return total;
}

// One ray's backward over its span: d_sigmas and d_rgbs of every sample of it (zeros behind the early stop).
template <int C>
__device__ __forceinline__ void composite_ray_bwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                  const float *__restrict__ deltas, int64_t off, int cnt, float T_thresh,
                                                  int lane, float dws, float ddp, const float (&di)[C],
                                                  const float (&bgc)[C], float total, float *__restrict__ d_sigmas,
                                                  float *__restrict__ d_rgbs) {
    float carry_tau = 0.f, carry_p = 0.f;
    bool stopped = false;  // wave-uniform
    Chunk<C> cur = load_chunk<C>(sigmas, rgbs, deltas, off, cnt, 0, lane);
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane;
        const bool valid = i < cnt;
        const int64_t s = off + (valid ? i : 0);
        if (stopped) {  // zero-fill the tail of the span
            if (valid) {
                d_sigmas[s] = 0.f;
                const float zero[C] = {};
                store_row<C>(d_rgbs, s, zero);
            }
            continue;
        }
        Chunk<C> nxt = cur;   // the next chunk's inputs, requested before this chunk's arithmetic (see the forward)
        if (base + 64 < cnt) nxt = load_chunk<C>(sigmas, rgbs, deltas, off, cnt, base + 64, lane);
        const float dt = cur.dt;
        const SpanWeight k = span_weight(cur.sigma * dt, valid, T_thresh, carry_tau);
        float g = fmaf(ddp, cur.t, dws);
#pragma unroll
        for (int c = 0; c < C; ++c) g = fmaf(di[c], cur.rgb[c] - bgc[c], g);
        const float gw = g * k.w;
        const float pinc = wave_inclusive_sum(gw) + carry_p;  // inclusive prefix of g_k w_k
        if (valid) {
            // dL/dtau_i = g_i T_{i+1} - sum_{k>i} g_k w_k
            const float dtau = k.live ? fmaf(g, k.Te, -(total - pinc)) : 0.f;
            d_sigmas[s] = dt * dtau;
            float drgb[C];    // d_rgbs[s][c] = di[c] * w
#pragma unroll
            for (int c = 0; c < C; ++c) drgb[c] = di[c] * k.w;
            store_row<C>(d_rgbs, s, drgb);
        }
        carry_p = lane63(pinc);
        if (expf(-carry_tau) < T_thresh) stopped = true;
        cur = nxt;
    }
}

template <int C>
__global__ void __launch_bounds__(256)
k_composite_train_bwd(const float *__restrict__ g_ws, const float *__restrict__ g_depth, const float *__restrict__ g_img,
                      const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                      const int32_t *__restrict__ rays, const float *__restrict__ weights_sum,
                      const float *__restrict__ depth, const float *__restrict__ image, const float *__restrict__ bg,
                      int64_t N, float T_thresh, float *__restrict__ d_sigmas, float *__restrict__ d_rgbs,
                      float *__restrict__ d_bg) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    const float ws = weights_sum[id];
    const float dws = g_ws ? g_ws[id] : 0.f;
    const float ddp = g_depth ? g_depth[id] : 0.f;
    float di[C], bgc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        di[c] = g_img[id * C + c];
        bgc[c] = bg ? bg[id * C + c] : 0.f;
    }
    const float total = ray_total<C>(dws, ddp, ws, depth[id], di, bgc, image + id * C);
    if (d_bg && lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) d_bg[id * C + c] = (1.0f - ws) * di[c];
    }
    composite_ray_bwd<C>(sigmas, rgbs, deltas, off, cnt, T_thresh, lane, dws, ddp, di, bgc, total, d_sigmas, d_rgbs);
}

// Backward of k_composite_train_decode_fwd.  With g = grad_image the decoder's chain rule is a per-ray prologue,
//   di_j = 1/2 sum_c g_c D[c][j],   dws' = dws + sum_c g_c (1/2 - bg_c),   grad_bg = (1 - ws) g,
// and the rest is the C = 4 backward on (di, dws', no background, latent_image as the image).
__global__ void __launch_bounds__(256)
k_composite_train_decode_bwd(const float *__restrict__ g_ws, const float *__restrict__ g_depth,
                             const float *__restrict__ g_img, const float *__restrict__ sigmas,
                             const float *__restrict__ latents, const float *__restrict__ deltas,
                             const int32_t *__restrict__ rays, const float *__restrict__ weights_sum,
                             const float *__restrict__ depth, const float *__restrict__ latent_image,
                             const float *__restrict__ decoder, const float *__restrict__ bg, int64_t N, float T_thresh,
                             float *__restrict__ d_sigmas, float *__restrict__ d_latents, float *__restrict__ d_bg) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    const float ws = weights_sum[id];
    float dws = g_ws ? g_ws[id] : 0.f;
    const float ddp = g_depth ? g_depth[id] : 0.f;
    float g[3], di[4], bgc[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g[c] = g_img[id * 3 + c];
        dws = fmaf(g[c], 0.5f - (bg ? bg[id * 3 + c] : 0.f), dws);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = g[0] * decoder[j];
        v = fmaf(g[1], decoder[4 + j], v);
        v = fmaf(g[2], decoder[8 + j], v);
        di[j] = 0.5f * v;
        bgc[j] = 0.f;
    }
    const float total = ray_total<4>(dws, ddp, ws, depth[id], di, bgc, latent_image + id * 4);
    if (d_bg && lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d_bg[id * 3 + c] = (1.0f - ws) * g[c];
    }
    composite_ray_bwd<4>(sigmas, latents, deltas, off, cnt, T_thresh, lane, dws, ddp, di, bgc, total, d_sigmas, d_latents);
}

// grad_decoder[c][j] = 1/2 sum_i grad_image[i][c] latent_image[i][j] over all N rays, by ONE workgroup in a fixed order
// (thread t takes rays t, t + 1024, ...; wave sums; the 16 wave totals added in wave order): a function of the inputs
// alone, no atomics, no workspace.  The result is overwritten.
constexpr int DECODER_GRAD_THREADS = 1024;
__global__ void __launch_bounds__(DECODER_GRAD_THREADS)
k_decoder_grad(const float *__restrict__ g_img, const float *__restrict__ latent_image, int64_t N,
               float *__restrict__ d_decoder) {
    __shared__ float part[DECODER_GRAD_THREADS / 64][12];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    for (int64_t i = threadIdx.x; i < N; i += DECODER_GRAD_THREADS) {
        const float4 v = reinterpret_cast<const float4 *>(latent_image)[i];
        const float L[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = g_img[i * 3 + c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c * 4 + j] = fmaf(gc, L[j], acc[c * 4 + j]);
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) part[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        float v = 0.f;
        for (int w = 0; w < DECODER_GRAD_THREADS / 64; ++w) v += part[w][threadIdx.x];
        d_decoder[threadIdx.x] = 0.5f * v;
    }
}

}  // namespace lnerf

using namespace lnerf;

// Gradient of the opacity-entropy regulariser (the trainer's sparsity term) with respect to weights_sum, one launch:
//   L = scale * mean_i H(p_i),  p = clamp(ws, eps, 1 - eps),  H(p) = -p log2 p - (1 - p) log2(1 - p)
//   dL/dws_i = scale / N * (log2(1 - p_i) - log2 p_i)   inside the clamp, 0 outside (the clamp's subgradient)
__global__ void __launch_bounds__(256) k_entropy_grad(const float *__restrict__ ws, int64_t N, float scale, float eps,
                                                      float *__restrict__ grad) {
    const float k = scale / (float)N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float w = ws[i];
        const bool inside = w >= eps && w <= 1.0f - eps;
        grad[i] = inside ? k * (log2f(1.0f - w) - log2f(w)) : 0.0f;
    }
}

extern "C" {

int lnerf_opacity_entropy_grad(const float *weights_sum, int64_t N, float scale, float eps, float *grad,
                               lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0 && eps > 0.f && eps < 0.5f, "opacity_entropy_grad: bad arguments");
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(weights_sum && grad, "opacity_entropy_grad: null pointer");
    int64_t blocks = div_up(N, (int64_t)256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_entropy_grad, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), weights_sum, N, scale, eps,
                       grad);
    LNERF_CHECK_LAUNCH("opacity_entropy_grad");
    return LNERF_OK;
}

int lnerf_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                       const int32_t *rays, int64_t N, int C, float T_thresh, const float *bg_color,
                                       float *weights_sum, float *depth, float *image, lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "composite_rays_train_forward: negative N");
    LNERF_REQUIRE(C == 3 || C == 4, "composite_rays_train_forward: C must be 3 or 4 (got %d)", C);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(rays && weights_sum && depth && image, "composite_rays_train_forward: null pointer");
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0 && (C != 4 || ((uintptr_t)rgbs & 15) == 0),
                  "composite_rays_train_forward: deltas must be 8-byte and (C = 4) rgbs 16-byte aligned");
    const dim3 grid((unsigned)div_up(N, 4)), block(256);
    if (C == 4)
        hipLaunchKernelGGL(k_composite_train_fwd<4>, grid, block, 0, as_stream(stream), sigmas, rgbs, deltas, rays, N,
                           T_thresh, bg_color, weights_sum, depth, image);
    else
        hipLaunchKernelGGL(k_composite_train_fwd<3>, grid, block, 0, as_stream(stream), sigmas, rgbs, deltas, rays, N,
                           T_thresh, bg_color, weights_sum, depth, image);
    LNERF_CHECK_LAUNCH("composite_rays_train_forward");
    return LNERF_OK;
}

int lnerf_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_depth,
                                        const float *grad_image, const float *sigmas, const float *rgbs,
                                        const float *deltas, const int32_t *rays, const float *weights_sum,
                                        const float *depth, const float *image, const float *bg_color, int64_t N,
                                        int C, float T_thresh, float *grad_sigmas, float *grad_rgbs, float *grad_bg,
                                        lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "composite_rays_train_backward: negative N");
    LNERF_REQUIRE(C == 3 || C == 4, "composite_rays_train_backward: C must be 3 or 4 (got %d)", C);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(grad_image && rays && weights_sum && depth && image && grad_sigmas && grad_rgbs,
                  "composite_rays_train_backward: null pointer");
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0 && (C != 4 || (((uintptr_t)rgbs | (uintptr_t)grad_rgbs) & 15) == 0),
                  "composite_rays_train_backward: deltas must be 8-byte and (C = 4) rgbs / grad_rgbs 16-byte aligned");
    const dim3 grid((unsigned)div_up(N, 4)), block(256);
    if (C == 4)
        hipLaunchKernelGGL(k_composite_train_bwd<4>, grid, block, 0, as_stream(stream), grad_weights_sum, grad_depth,
                           grad_image, sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg_color, N, T_thresh,
                           grad_sigmas, grad_rgbs, grad_bg);
    else
        hipLaunchKernelGGL(k_composite_train_bwd<3>, grid, block, 0, as_stream(stream), grad_weights_sum, grad_depth,
                           grad_image, sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg_color, N, T_thresh,
                           grad_sigmas, grad_rgbs, grad_bg);
    LNERF_CHECK_LAUNCH("composite_rays_train_backward");
    return LNERF_OK;
}

int lnerf_composite_rays_train_decode_forward(const float *sigmas, const float *latents, const float *deltas,
                                              const int32_t *rays, int64_t N, float T_thresh, const float *decoder,
                                              const float *bg_color, float *weights_sum, float *depth,
                                              float *latent_image, float *image, lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "composite_rays_train_decode_forward: negative N");
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(rays && decoder && weights_sum && depth && latent_image && image,
                  "composite_rays_train_decode_forward: null pointer");
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0 && (((uintptr_t)latents | (uintptr_t)latent_image) & 15) == 0,
                  "composite_rays_train_decode_forward: deltas must be 8-byte, latents / latent_image 16-byte aligned");
    hipLaunchKernelGGL(k_composite_train_decode_fwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream), sigmas,
                       latents, deltas, rays, N, T_thresh, decoder, bg_color, weights_sum, depth, latent_image, image);
    LNERF_CHECK_LAUNCH("composite_rays_train_decode_forward");
    return LNERF_OK;
}

int lnerf_composite_rays_train_decode_backward(const float *grad_weights_sum, const float *grad_depth,
                                               const float *grad_image, const float *sigmas, const float *latents,
                                               const float *deltas, const int32_t *rays, const float *weights_sum,
                                               const float *depth, const float *latent_image, const float *decoder,
                                               const float *bg_color, int64_t N, float T_thresh, float *grad_sigmas,
                                               float *grad_latents, float *grad_bg, float *grad_decoder,
                                               lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "composite_rays_train_decode_backward: negative N");
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(grad_image && rays && weights_sum && depth && latent_image && decoder && grad_sigmas && grad_latents &&
                      grad_decoder,
                  "composite_rays_train_decode_backward: null pointer");
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0 &&
                      (((uintptr_t)latents | (uintptr_t)grad_latents | (uintptr_t)latent_image) & 15) == 0,
                  "composite_rays_train_decode_backward: deltas must be 8-byte, latents / grad_latents / latent_image "
                  "16-byte aligned");
    hipLaunchKernelGGL(k_composite_train_decode_bwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream),
                       grad_weights_sum, grad_depth, grad_image, sigmas, latents, deltas, rays, weights_sum, depth,
                       latent_image, decoder, bg_color, N, T_thresh, grad_sigmas, grad_latents, grad_bg);
    LNERF_CHECK_LAUNCH("composite_rays_train_decode_backward");
    hipLaunchKernelGGL(k_decoder_grad, dim3(1), dim3(DECODER_GRAD_THREADS), 0, as_stream(stream), grad_image,
                       latent_image, N, grad_decoder);
    LNERF_CHECK_LAUNCH("composite_rays_train_decode_backward (decoder gradient)");
    return LNERF_OK;
}

int lnerf_decode_image(const float *latent_image, const float *weights_sum, const float *decoder, const float *bg_color,
                       int64_t N, float *image, lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "decode_image: negative N");
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(latent_image && weights_sum && decoder && image, "decode_image: null pointer");
    LNERF_REQUIRE(((uintptr_t)latent_image & 15) == 0, "decode_image: latent_image must be 16-byte aligned");
    hipLaunchKernelGGL(k_decode_image, dim3((unsigned)div_up(N, 256)), dim3(256), 0, as_stream(stream), latent_image,
                       weights_sum, decoder, bg_color, N, image);
    LNERF_CHECK_LAUNCH("decode_image");
    return LNERF_OK;
}

}  // extern "C"
