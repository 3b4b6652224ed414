// Composited normal image of the shaded training renders and the 2D smoothness stencil on an image, forward + backward.
// Contract and order of operations: include/lnerf_hip.h, "composited normal image"; numpy restatement:
// tests/normal_image_reference.py.
//
//   k_normal_image_fwd   normal_image[ray] = sum_i w_i n_i: the finite-difference normal of shade.hip, the compositing weight
//                        of the orientation term -- one wavefront per ray, chunks of 64 chained through a scalar carry
//   k_normal_image_bwd   ONE forward sweep per ray: the weights are NOT detached (sum_i g_i w_i = N . dN comes from the
//                        forward's output), and the normal's gradient goes through shade.hip's projection
//   k_image_smooth_fwd   squared differences to the right and the lower neighbour, one lane per pixel
//   k_image_smooth_bwd   its gradient in gather form (own-h, own-v, left, up)
//
// All arithmetic is f32 + - * / sqrt in the stated order (-ffp-contract=off, no explicit fmaf) except expf and the 64-lane
// scans.  No LDS, no atomics: every output element has one writer.
#include "common.h"

namespace lnerf {

constexpr int NI_ROWS = 7;       // the sample and its six neighbours (shade.hip's FD_ROWS)

// one lane's sample of a 64-sample chunk (zeros past the end of the span)
struct NormalChunk {
    float sg[NI_ROWS], dt;
};
__device__ __forceinline__ NormalChunk load_normal_chunk(const float *__restrict__ sigmas7, const float *__restrict__ deltas,
                                                         int64_t off, int cnt, int i) {
    NormalChunk k;
#pragma unroll
    for (int j = 0; j < NI_ROWS; ++j) k.sg[j] = 0.f;
    k.dt = 0.f;
    if (i < cnt) {
        const int64_t s7 = (off + i) * NI_ROWS;
#pragma unroll
        for (int j = 0; j < NI_ROWS; ++j) k.sg[j] = sigmas7[s7 + j];
        k.dt = reinterpret_cast<const float2 *>(deltas)[off + i].x;
    }
    return k;
}

// finite-difference normal of one sample, as lnerf_shade_fd_forward defines it
struct FdNormal {
    float n[3], s, r;
};
__device__ __forceinline__ FdNormal fd_normal(const float (&sg)[NI_ROWS], float inv_2eps) {
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

// Compositing weight of this lane's sample, as lnerf_shade_fd_orient_forward defines it, with what the backward needs of
// it.  Called by ALL 64 lanes (a wave scan); lanes past the span carry w = 0.  No early stop.
struct NormalWeight {
    float w, Te;     // weight, T_{i+1} = T e
    bool live;       // valid && T >= T_thresh
};
__device__ __forceinline__ NormalWeight normal_weight(float sigma, float dt, bool valid, float T_thresh, float &carry) {
    NormalWeight o;
    const float tau = sigma * dt;
    const float inc = wave_inclusive_sum(tau);
    const float excl = exclusive_depth(inc, carry);
    const float T = expf(-excl);
    const float e = expf(-tau);
    const float alpha = 1.0f - e;
    o.live = valid && T >= T_thresh;
    o.w = o.live ? alpha * T : 0.f;
    o.Te = T * e;
    carry += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc), 63));
    return o;
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
        const NormalWeight k = normal_weight(density_scale * cur.sg[0], cur.dt, base + lane < cnt, T_thresh, carry);
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
        const NormalWeight k = normal_weight(density_scale * cur.sg[0], cur.dt, valid, T_thresh, carry);
        const float g = (o.n[0] * dN[0] + o.n[1] * dN[1]) + o.n[2] * dN[2];
        const float pinc = wave_inclusive_sum(g * k.w) + carry_g;
        if (valid) {
            // dL/dtau_i = g_i T_{i+1} - sum_{j>i} g_j w_j
            const float dtau = k.live ? g * k.Te - (total - pinc) : 0.f;
            float dn[3], ds[NI_ROWS];
#pragma unroll
            for (int a = 0; a < 3; ++a) dn[a] = k.w * dN[a];
            const float q = (o.n[0] * dn[0] + o.n[1] * dn[1]) + o.n[2] * dn[2];
            const bool project = o.s > 1e-20f;
            ds[0] = (density_scale * cur.dt) * dtau;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t = project ? dn[a] - o.n[a] * q : dn[a];
                const float dg = -(o.r * t);
                const float v = dg * inv_2eps;
                ds[1 + 2 * a] = v;
                ds[2 + 2 * a] = -v;
            }
            const int64_t s7 = (off + i) * NI_ROWS;
#pragma unroll
            for (int j = 0; j < NI_ROWS; ++j) dsigmas7[s7 + j] = ds[j];
        }
        carry_g = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pinc), 63));
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
