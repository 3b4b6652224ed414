// Mip-mapped texture lookup of the Latent-Paint renderer (`guide.texture_interpolation_mode mipmap`): the filter a
// 64 x 64 render of a 1024 x 1024 texture needs, where one pixel covers on the order of a hundred texels and a point
// lookup reads four of them.  Three stages, all stated in include/lnerf_hip.h:
//   lnerf_uv_footprint         k_uv_footprint   per pixel, the length in UV units of the longer screen-space UV derivative
//                                               per one-pixel step, analytic on the winning face (no pixel differences:
//                                               those break at face borders and silhouettes)
//   lnerf_mip_build (+ bwd)    k_mip_down/up    levels 1..L = 2 x 2 box averages, one launch per level; the backward is the
//                                               transpose in gather form (no atomics)
//   lnerf_texture_mip_* (f/b)  k_texture_mip    lambda = clamp(log2(rho R) + bias, 0, L), the bilinear lookup of raster.hip
//                                               on the two levels around lambda, mixed linearly
// The kaolin path the reference calls has no such filter (its texture_mapping is a point lookup); the convention is the
// `linear-mipmap-linear` one of rasteriser-based texture optimisers, isotropic, with the longer axis choosing the level.
#include <math.h>

#include "common.h"
#include "tex_shared.h"

namespace lnerf {

// One thread per pixel of the B views.  px, py, area, e0, e1 and the weights are k_rasterize's expressions (raster.hip
// raster_face_test), so bw_k are the barycentrics that rasteriser wrote.  Every operation is rounded on its own.
__global__ void __launch_bounds__(256)
k_uv_footprint(const int32_t *__restrict__ face_idx, const float *__restrict__ face_xy,
               const float *__restrict__ face_z, const float *__restrict__ face_uv, int64_t P, int H, int W, int F,
               float *__restrict__ rho) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int f = face_idx[p];
    if (f < 0 || f >= F) {
        rho[p] = 0.f;
        return;
    }
    const int64_t hw = (int64_t)H * W;
    const int64_t b = p / hw;
    const int q = (int)(p - b * hw);
    const int i = q / W, j = q - i * W;
    const float px = (2.0f * (float)j + 1.0f) / (float)W - 1.0f;
    const float py = 1.0f - (2.0f * (float)i + 1.0f) / (float)H;
    const float *xy = face_xy + (b * F + f) * 6, *zz = face_z + (b * F + f) * 3, *uv = face_uv + (int64_t)f * 6;
    const float x0 = xy[0], y0 = xy[1], x1 = xy[2], y1 = xy[3], x2 = xy[4], y2 = xy[5];
    const float z0 = zz[0], z1 = zz[1], z2 = zz[2];
    const float area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    const float e0 = (x1 - px) * (y2 - py) - (x2 - px) * (y1 - py);
    const float e1 = (x2 - px) * (y0 - py) - (x0 - px) * (y2 - py);
    const float inv = 1.0f / area;
    const float w0 = e0 * inv, w1 = e1 * inv, w2 = 1.0f - w0 - w1;
    const float q0 = w0 / z0, q1 = w1 / z1, q2 = w2 / z2;
    const float qs = q0 + q1 + q2;
    const float z = 1.0f / qs;
    const float bw0 = q0 * z, bw1 = q1 * z, bw2 = q2 * z;
    // the screen barycentrics are affine in (px, py): d w_k / d px, d w_k / d py
    const float w0x = (y1 - y2) * inv, w0y = (x2 - x1) * inv;
    const float w1x = (y2 - y0) * inv, w1y = (x0 - x2) * inv;
    const float w2x = -w0x - w1x, w2y = -w0y - w1y;
    // d bw_k = (d w_k / z_k - bw_k * sum_m d w_m / z_m) / qs
    const float a0x = w0x / z0, a1x = w1x / z1, a2x = w2x / z2;
    const float a0y = w0y / z0, a1y = w1y / z1, a2y = w2y / z2;
    const float sx = a0x + a1x + a2x, sy = a0y + a1y + a2y;
    const float b0x = (a0x - bw0 * sx) * z, b1x = (a1x - bw1 * sx) * z, b2x = (a2x - bw2 * sx) * z;
    const float b0y = (a0y - bw0 * sy) * z, b1y = (a1y - bw1 * sy) * z, b2y = (a2y - bw2 * sy) * z;
    const float ux = uv[0] * b0x + uv[2] * b1x + uv[4] * b2x, vx = uv[1] * b0x + uv[3] * b1x + uv[5] * b2x;
    const float uy = uv[0] * b0y + uv[2] * b1y + uv[4] * b2y, vy = uv[1] * b0y + uv[3] * b1y + uv[5] * b2y;
    // one pixel step is 2 / W in px and 2 / H in py
    const float lx = sqrtf(ux * ux + vx * vx) * (2.0f / (float)W);
    const float ly = sqrtf(uy * uy + vy * vy) * (2.0f / (float)H);
    rho[p] = fmaxf(lx, ly);
}

// Level l (side Rd) from level l - 1 (side 2 Rd): a coarse texel covers exactly four fine ones (texel centres,
// align_corners=False).  One thread per (channel, coarse texel); `sstride` / `dstride` are the channel strides.
__global__ void __launch_bounds__(256)
k_mip_down(const float *__restrict__ src, int64_t sstride, float *__restrict__ dst, int64_t dstride, int C, int Rd) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)Rd * Rd;
    if (t >= n * C) return;
    const int c = (int)(t / n);
    const int64_t r = t - c * n;
    const int i = (int)(r / Rd), j = (int)(r - (int64_t)i * Rd);
    const int Rs = 2 * Rd;
    const float *s = src + c * sstride + (int64_t)(2 * i) * Rs + 2 * j;
    dst[c * dstride + r] = ((s[0] + s[1]) + (s[Rs] + s[Rs + 1])) * 0.25f;
}

// The transpose, as a gather: every fine texel (side Rf) adds a quarter of its one coarse parent's gradient.
__global__ void __launch_bounds__(256)
k_mip_up(const float *__restrict__ dcoarse, int64_t cstride, float *__restrict__ dfine, int64_t fstride, int C, int Rf) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)Rf * Rf;
    if (t >= n * C) return;
    const int c = (int)(t / n);
    const int64_t r = t - c * n;
    const int i = (int)(r / Rf), j = (int)(r - (int64_t)i * Rf);
    const int Rc = Rf / 2;
    dfine[c * fstride + r] += 0.25f * dcoarse[c * cstride + (int64_t)(i / 2) * Rc + j / 2];
}

// One thread per (pixel, channel), as k_texture_map.  tex = level 0 [C,R,R], pyr = levels 1..L packed [C,S]; in the
// backward both are the gradients the atomics add to.
template <bool BWD>
__global__ void __launch_bounds__(256)
k_texture_mip(const float *__restrict__ uv, const float *__restrict__ rho, const int32_t *__restrict__ face_idx,
              float *tex, float *pyr, int64_t P, int C, int R, int L, int64_t S, float bias, float *out_or_dout) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P * C) return;
    const int64_t p = t / C;
    const int c = (int)(t - p * C);
    const bool fg = !face_idx || face_idx[p] >= 0;
    if (!fg) {
        if (!BWD) out_or_dout[t] = 0.f;
        return;
    }
    const float s = rho[p] * (float)R;   // the footprint in level-0 texels
    const float lam = s > 0.f ? clampf(log2f(s) + bias, 0.f, (float)L) : 0.f;
    const int l0 = min((int)floorf(lam), L);
    const float mix = lam - (float)l0;
    const float u = uv[p * 2], v = uv[p * 2 + 1];
    float *t0 = l0 == 0 ? tex + (int64_t)c * R * R : pyr + c * S + mip_offset(R, l0);
    const BilTaps b0 = bil_taps(u, v, R >> l0);
    if (mix == 0.f) {   // one level: where the footprint is at most a texel this is mode bilinear bit for bit
        if (BWD) bil_add(t0, b0, out_or_dout[t]);
        else out_or_dout[t] = bil_read(t0, b0);
        return;
    }
    float *t1 = pyr + c * S + mip_offset(R, l0 + 1);   // mix > 0 only below level L
    const BilTaps b1 = bil_taps(u, v, R >> (l0 + 1));
    if (BWD) {
        const float g = out_or_dout[t];
        bil_add(t0, b0, (1.f - mix) * g);
        bil_add(t1, b1, mix * g);
    } else {
        out_or_dout[t] = (1.f - mix) * bil_read(t0, b0) + mix * bil_read(t1, b1);
    }
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_uv_footprint(const int32_t *face_idx, const float *face_xy, const float *face_z, const float *face_uv, int B,
                       int H, int W, int n_faces, float *rho, lnerf_stream_t stream) {
    LNERF_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 32767 && W <= 32767 && (int64_t)B * H * W <= 2147483647,
                  "uv_footprint: B, H, W must be >= 1, H and W <= 32767 and B * H * W < 2^31 (got %d, %d, %d)", B, H, W);
    LNERF_REQUIRE(n_faces > 0, "uv_footprint: no faces");
    LNERF_REQUIRE(face_idx && face_xy && face_z && face_uv && rho, "uv_footprint: null pointer");
    const int64_t P = (int64_t)B * H * W;
    hipLaunchKernelGGL(k_uv_footprint, dim3((unsigned)div_up(P, 256)), dim3(256), 0, as_stream(stream), face_idx,
                       face_xy, face_z, face_uv, P, H, W, n_faces, rho);
    LNERF_CHECK_LAUNCH("uv_footprint");
    return LNERF_OK;
}

int lnerf_mip_build(const float *texture, int C, int R, int L, float *pyramid, lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mip_build", C, R, L)) return rc;
    LNERF_REQUIRE(texture && (pyramid || L == 0), "mip_build: null pointer");
    const int64_t S = mip_texels(R, L);
    for (int l = 1; l <= L; ++l) {
        const int Rd = R >> l;
        const float *src = l == 1 ? texture : pyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(k_mip_down, dim3((unsigned)div_up((int64_t)C * Rd * Rd, 256)), dim3(256), 0,
                           as_stream(stream), src, l == 1 ? (int64_t)R * R : S, pyramid + mip_offset(R, l), S, C, Rd);
        LNERF_CHECK_LAUNCH("mip_build");
    }
    return LNERF_OK;
}

int lnerf_mip_build_backward(float *dpyramid, int C, int R, int L, float *dtexture, lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mip_build_backward", C, R, L)) return rc;
    LNERF_REQUIRE(dtexture && (dpyramid || L == 0), "mip_build_backward: null pointer");
    const int64_t S = mip_texels(R, L);
    for (int l = L; l >= 1; --l) {   // level l's gradient is complete once every coarser level has been folded into it
        const int Rf = R >> (l - 1);
        float *fine = l == 1 ? dtexture : dpyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(k_mip_up, dim3((unsigned)div_up((int64_t)C * Rf * Rf, 256)), dim3(256), 0,
                           as_stream(stream), dpyramid + mip_offset(R, l), S, fine, l == 1 ? (int64_t)R * R : S, C, Rf);
        LNERF_CHECK_LAUNCH("mip_build_backward");
    }
    return LNERF_OK;
}

int lnerf_texture_mip_forward(const float *uv, const float *rho, const int32_t *face_idx, const float *texture,
                              const float *pyramid, int n_pixels, int C, int R, int L, float bias, float *out,
                              lnerf_stream_t stream) {
    if (int rc = check_mip_shape("texture_mip_forward", C, R, L)) return rc;
    LNERF_REQUIRE(n_pixels > 0, "texture_mip_forward: n_pixels must be > 0 (got %d)", n_pixels);
    LNERF_REQUIRE(__builtin_isfinite(bias), "texture_mip_forward: bias must be finite");
    LNERF_REQUIRE(uv && rho && texture && out && (pyramid || L == 0), "texture_mip_forward: null pointer");
    hipLaunchKernelGGL(k_texture_mip<false>, dim3((unsigned)div_up((int64_t)n_pixels * C, 256)), dim3(256), 0,
                       as_stream(stream), uv, rho, face_idx, const_cast<float *>(texture), const_cast<float *>(pyramid),
                       (int64_t)n_pixels, C, R, L, mip_texels(R, L), bias, out);
    LNERF_CHECK_LAUNCH("texture_mip_forward");
    return LNERF_OK;
}

int lnerf_texture_mip_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                               int n_pixels, int C, int R, int L, float bias, float *dtexture, float *dpyramid,
                               lnerf_stream_t stream) {
    if (int rc = check_mip_shape("texture_mip_backward", C, R, L)) return rc;
    LNERF_REQUIRE(n_pixels > 0, "texture_mip_backward: n_pixels must be > 0 (got %d)", n_pixels);
    LNERF_REQUIRE(__builtin_isfinite(bias), "texture_mip_backward: bias must be finite");
    LNERF_REQUIRE(uv && rho && dout && dtexture && (dpyramid || L == 0), "texture_mip_backward: null pointer");
    hipLaunchKernelGGL(k_texture_mip<true>, dim3((unsigned)div_up((int64_t)n_pixels * C, 256)), dim3(256), 0,
                       as_stream(stream), uv, rho, face_idx, dtexture, dpyramid, (int64_t)n_pixels, C, R, L,
                       mip_texels(R, L), bias, const_cast<float *>(dout));
    LNERF_CHECK_LAUNCH("texture_mip_backward");
    return LNERF_OK;
}

}  // extern "C"
