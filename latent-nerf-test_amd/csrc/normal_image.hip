// Composited normal image of the shaded training renders and the 2D smoothness stencil on an image, forward + backward.
// Contract and order of operations: include/lnerf_hip.h, "composited normal image"; numpy restatement:
// tests/normal_image_reference.py.
//
//   k_normal_image_fwd   normal_image[ray] = sum_i w_i n_i: the finite-difference normal and the compositing weight of
//                        span_walk.h -- one wavefront per ray, chunks of 64 chained through a scalar carry
//   k_normal_image_bwd   ONE forward sweep per ray: the weights are NOT detached (sum_i g_i w_i = N . dN comes from the
//                        forward's output), and the normal's gradient goes through span_walk.h's projection
//   k_image_smooth_fwd   squared differences to the right and the lower neighbour, one lane per pixel
//   k_image_smooth_bwd   its gradient in gather form (own-h, own-v, left, up)
//
// All arithmetic is f32 + - * / sqrt in the stated order (-ffp-contract=off, no explicit fmaf) except expf and the 64-lane
// scans.  No LDS, no atomics: every output element has one writer.
#include "span_walk.h"

namespace lnerf {

// one lane's sample of a 64-sample chunk (zeros past the end of the span)
struct NormalChunk {
    float sg[FD_ROWS], dt;
};
__device__ __forceinline__ NormalChunk load_normal_chunk(const float *__restrict__ sigmas7, const float *__restrict__ deltas,
                                                         int64_t off, int cnt, int i) {
    NormalChunk k;
#pragma unroll
    for (int j = 0; j < FD_ROWS; ++j) k.sg[j] = 0.f;
    k.dt = 0.f;
    if (i < cnt) {
        load_fd_rows(sigmas7, (off + i) * FD_ROWS, k.sg);
        k.dt = load_step(deltas, off + i).dt;
    }
    return k;
}

// normal_image[id] = sum_i w_i n_i.  A ray without samples writes zeros (the buffer is uninitialised): no early return
// before the stores.
__global__ void __launch_bounds__(256)
k_normal_image_fwd(const float *__restrict__ sigmas7, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                   int64_t N, float inv_2eps, float density_scale, float T_thresh, float *__restrict__ normal_image) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    float acc[3] = {0.f, 0.f, 0.f}, carry = 0.f;
    NormalChunk cur = load_normal_chunk(sigmas7, deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        NormalChunk nxt = cur;    // the next chunk's inputs, requested before this chunk's scan
        if (base + 64 < cnt) nxt = load_normal_chunk(sigmas7, deltas, off, cnt, base + 64 + lane);
        const FdNormal o = fd_normal(cur.sg, inv_2eps);
        const SpanWeight k = span_weight((density_scale * cur.sg[0]) * cur.dt, base + lane < cnt, T_thresh, carry);
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] += k.w * o.n[a];
        cur = nxt;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[a] = wave_sum(acc[a]);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) normal_image[(int64_t)id * 3 + a] = acc[a];
    }
}

// The seven dsigmas7 rows of every sample of every span.  One forward sweep: with N = normal_image[id] of the forward,
//   g_i = n_i . dN,   sum_{j > i} g_j w_j = N . dN - (inclusive prefix of g w).
__global__ void __launch_bounds__(256)
k_normal_image_bwd(const float *__restrict__ sigmas7, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                   int64_t N, float inv_2eps, float density_scale, float T_thresh, const float *__restrict__ d_normal_image,
                   const float *__restrict__ normal_image, float *__restrict__ dsigmas7) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    if (cnt <= 0) return;
    float dN[3], Nf[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        dN[a] = d_normal_image[(int64_t)id * 3 + a];
        Nf[a] = normal_image[(int64_t)id * 3 + a];
    }
    const float total = (Nf[0] * dN[0] + Nf[1] * dN[1]) + Nf[2] * dN[2];
    float carry = 0.f, carry_g = 0.f;
    NormalChunk cur = load_normal_chunk(sigmas7, deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        NormalChunk nxt = cur;
        if (base + 64 < cnt) nxt = load_normal_chunk(sigmas7, deltas, off, cnt, base + 64 + lane);
        const int i = base + lane;
        const bool valid = i < cnt;
        const FdNormal o = fd_normal(cur.sg, inv_2eps);
        const SpanWeight k = span_weight((density_scale * cur.sg[0]) * cur.dt, valid, T_thresh, carry);
        const float g = (o.n[0] * dN[0] + o.n[1] * dN[1]) + o.n[2] * dN[2];
        const float pinc = wave_inclusive_sum(g * k.w) + carry_g;
        if (valid) {
            // dL/dtau_i = g_i T_{i+1} - sum_{j>i} g_j w_j
            const float dtau = k.live ? g * k.Te - (total - pinc) : 0.f;
            float dn[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) dn[a] = k.w * dN[a];
            store_fd_rows(dsigmas7, (off + i) * FD_ROWS, (density_scale * cur.dt) * dtau,
                          fd_normal_backward(o, dn, inv_2eps));
        }
        carry_g = lane63(pinc);
        cur = nxt;
    }
}

// loss[p] = (sum_c (img[right of p][c] - img[p][c])^2, sum_c (img[below p][c] - img[p][c])^2), 0 at the last column / row
template <int C>
__global__ void __launch_bounds__(256)
k_image_smooth_fwd(const float *__restrict__ img, int64_t n_pix, int H, int W, float *__restrict__ loss) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const float *own = img + p * C;
    float h = 0.f, v = 0.f;
    if (x + 1 < W) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = own[C + c] - own[c];
            h = c == 0 ? d * d : h + d * d;
        }
    }
    if (y + 1 < H) {
        const float *below = own + (int64_t)W * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = below[c] - own[c];
            v = c == 0 ? d * d : v + d * d;
        }
    }
    loss[p * 2] = h;
    loss[p * 2 + 1] = v;
}

// d_img[p][c]: the pixel's own two pairs, then the left neighbour's horizontal and the upper neighbour's vertical pair
template <int C>
__global__ void __launch_bounds__(256)
k_image_smooth_bwd(const float *__restrict__ img, int64_t n_pix, int H, int W, const float *__restrict__ d_loss,
                   float *__restrict__ d_img) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const int64_t row = (int64_t)W * C;
    const float *own = img + p * C;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    if (x + 1 < W) {
        const float k = 2.0f * d_loss[p * 2];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] - k * (own[C + c] - own[c]);
    }
    if (y + 1 < H) {
        const float k = 2.0f * d_loss[p * 2 + 1];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] - k * (own[row + c] - own[c]);
    }
    if (x > 0) {
        const float k = 2.0f * d_loss[(p - 1) * 2];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + k * (own[c] - own[c - C]);
    }
    if (y > 0) {
        const float k = 2.0f * d_loss[(p - W) * 2 + 1];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + k * (own[c] - own[c - row]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) d_img[p * C + c] = acc[c];
}

}  // namespace lnerf

using namespace lnerf;

static int check_normal_image(const char *name, const float *sigmas7, const float *deltas, const int32_t *rays, int64_t N,
                              float density_scale, float T_thresh) {
    LNERF_REQUIRE(N >= 0, "%s: negative N", name);
    LNERF_REQUIRE(T_thresh >= 0.f && T_thresh < 1.f, "%s: T_thresh must be in [0, 1)", name);
    LNERF_REQUIRE(density_scale >= 0.f, "%s: density_scale must be >= 0", name);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(sigmas7 && deltas && rays, "%s: null pointer (sigmas7 / deltas / rays)", name);
    LNERF_REQUIRE(((uintptr_t)deltas & 7) == 0, "%s: deltas must be 8-byte aligned", name);
    return LNERF_OK;
}

static int check_image_smooth(const char *name, const float *img, int B, int H, int W, int C) {
    LNERF_REQUIRE(B >= 0 && H >= 0 && W >= 0, "%s: negative size (B, H, W = %d, %d, %d)", name, B, H, W);
    LNERF_REQUIRE(C >= 1 && C <= 4, "%s: C must be in 1..4 (got %d)", name, C);
    if (B == 0 || H == 0 || W == 0) return LNERF_OK;
    LNERF_REQUIRE(img, "%s: null pointer (img)", name);
    return LNERF_OK;
}

extern "C" {

int lnerf_normal_image_forward(const float *sigmas7, const float *deltas, const int32_t *rays, int64_t N, float inv_2eps,
                               float density_scale, float T_thresh, float *normal_image, lnerf_stream_t stream) {
    if (check_normal_image("normal_image_forward", sigmas7, deltas, rays, N, density_scale, T_thresh) != LNERF_OK)
        return LNERF_ERR_INVALID_ARG;
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(normal_image, "normal_image_forward: null pointer (normal_image)");
    hipLaunchKernelGGL(k_normal_image_fwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream), sigmas7, deltas,
                       rays, N, inv_2eps, density_scale, T_thresh, normal_image);
    LNERF_CHECK_LAUNCH("normal_image_forward");
    return LNERF_OK;
}

int lnerf_normal_image_backward(const float *sigmas7, const float *deltas, const int32_t *rays, int64_t N, float inv_2eps,
                                float density_scale, float T_thresh, const float *d_normal_image, const float *normal_image,
                                float *dsigmas7, lnerf_stream_t stream) {
    if (check_normal_image("normal_image_backward", sigmas7, deltas, rays, N, density_scale, T_thresh) != LNERF_OK)
        return LNERF_ERR_INVALID_ARG;
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(d_normal_image && normal_image && dsigmas7,
                  "normal_image_backward: null pointer (d_normal_image / normal_image / dsigmas7)");
    hipLaunchKernelGGL(k_normal_image_bwd, dim3((unsigned)div_up(N, 4)), dim3(256), 0, as_stream(stream), sigmas7, deltas,
                       rays, N, inv_2eps, density_scale, T_thresh, d_normal_image, normal_image, dsigmas7);
    LNERF_CHECK_LAUNCH("normal_image_backward");
    return LNERF_OK;
}

int lnerf_image_smooth_forward(const float *img, int B, int H, int W, int C, float *loss, lnerf_stream_t stream) {
    if (check_image_smooth("image_smooth_forward", img, B, H, W, C) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    const int64_t n_pix = (int64_t)B * H * W;
    if (n_pix == 0) return LNERF_OK;
    LNERF_REQUIRE(loss, "image_smooth_forward: null pointer (loss)");
    const dim3 grid((unsigned)div_up(n_pix, 256)), block(256);
    switch (C) {
    case 1: hipLaunchKernelGGL(k_image_smooth_fwd<1>, grid, block, 0, as_stream(stream), img, n_pix, H, W, loss); break;
    case 2: hipLaunchKernelGGL(k_image_smooth_fwd<2>, grid, block, 0, as_stream(stream), img, n_pix, H, W, loss); break;
    case 3: hipLaunchKernelGGL(k_image_smooth_fwd<3>, grid, block, 0, as_stream(stream), img, n_pix, H, W, loss); break;
    default: hipLaunchKernelGGL(k_image_smooth_fwd<4>, grid, block, 0, as_stream(stream), img, n_pix, H, W, loss); break;
    }
    LNERF_CHECK_LAUNCH("image_smooth_forward");
    return LNERF_OK;
}

int lnerf_image_smooth_backward(const float *img, int B, int H, int W, int C, const float *d_loss, float *d_img,
                                lnerf_stream_t stream) {
    if (check_image_smooth("image_smooth_backward", img, B, H, W, C) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    const int64_t n_pix = (int64_t)B * H * W;
    if (n_pix == 0) return LNERF_OK;
    LNERF_REQUIRE(d_loss && d_img, "image_smooth_backward: null pointer (d_loss / d_img)");
    const dim3 grid((unsigned)div_up(n_pix, 256)), block(256);
    switch (C) {
    case 1: hipLaunchKernelGGL(k_image_smooth_bwd<1>, grid, block, 0, as_stream(stream), img, n_pix, H, W, d_loss, d_img); break;
    case 2: hipLaunchKernelGGL(k_image_smooth_bwd<2>, grid, block, 0, as_stream(stream), img, n_pix, H, W, d_loss, d_img); break;
    case 3: hipLaunchKernelGGL(k_image_smooth_bwd<3>, grid, block, 0, as_stream(stream), img, n_pix, H, W, d_loss, d_img); break;
    default: hipLaunchKernelGGL(k_image_smooth_bwd<4>, grid, block, 0, as_stream(stream), img, n_pix, H, W, d_loss, d_img); break;
    }
    LNERF_CHECK_LAUNCH("image_smooth_backward");
    return LNERF_OK;
}

}  // extern "C"
