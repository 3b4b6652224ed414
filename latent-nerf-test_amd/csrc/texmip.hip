// Texture pyramids of the Latent-Paint renderer and of the exports: the mip-mapped lookup a 64 x 64 render of a
// 1024 x 1024 texture needs (`guide.texture_interpolation_mode mipmap`: one pixel covers on the order of a hundred
// texels and a point lookup reads four of them), plain or coverage-weighted (`guide.texture_mip_coverage`: level l is
// the coverage-weighted mean of level l - 1, the weights carried along, read normalised), and the pull-push fill that
// pushes the weighted pyramid back down into the texels no surface point owns.  All stated in include/lnerf_hip.h:
//   lnerf_uv_footprint                k_uv_footprint  per pixel, the length in UV units of the longer screen-space UV
//                                                     derivative per one-pixel step, analytic on the winning face (no
//                                                     pixel differences: those break at face borders and silhouettes)
//   lnerf_mip_build, _mipcov_pull,    k_pyr_down      levels 1..L, one launch per level: 2 x 2 box averages, or
//   lnerf_mipcov_weights                              sum w v / sum w over the four children (0 where nothing is
//                                                     covered); the weights' own levels are the plain build with C = 1
//   their backwards                   k_pyr_up        the transpose in gather form (no atomics)
//   lnerf_mipcov_push                 k_cov_push      from the coarsest level down, F_l = k v_l + (1 - k) up(F_{l+1})
//   lnerf_texture_mip_*, _mipcov_*    k_texture_mip   lambda = clamp(log2(rho R) + bias, 0, L), the bilinear lookup of
//                                                     raster.hip on the two levels around lambda, mixed linearly; with
//                                                     weights, numerator and denominator filtered alike and divided
// Plain and weighted are the two instantiations (COV) of one kernel each, so "every weight 1 gives the plain result bit
// for bit" is one set of source lines, not two that agree.  The weighted pyramid kernels run one lane per texel and loop
// over the channels, so a texel's weights are read once; the plain ones run one lane per (channel, texel).
// The kaolin path the reference calls has no such filter (its texture_mapping is a point lookup); the convention is the
// `linear-mipmap-linear` one of rasteriser-based texture optimisers, isotropic, with the longer axis choosing the level.
#include <math.h>

#include "common.h"
#include "raster_shared.h"
#include "tex_shared.h"

namespace lnerf {

// One thread per pixel of the B views.  Calls the rasteriser's own pixel centre and both weight stages (raster_shared.h),
// so bw_k are the barycentrics raster.hip wrote.  Every operation is rounded on its own.
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
    const auto [b, i, j] = pixel_of(p, H, W);
    const auto [px, py] = pixel_centre(i, j, H, W);
    const int64_t bf = (int64_t)b * F + f;
    const float *xy = face_xy + bf * 6, *zz = face_z + bf * 3, *uv = face_uv + (int64_t)f * 6;
    const float x0 = xy[0], y0 = xy[1], x1 = xy[2], y1 = xy[3], x2 = xy[4], y2 = xy[5];
    const float z0 = zz[0], z1 = zz[1], z2 = zz[2];
    const FaceW w = face_weights(face_area(x0, y0, x1, y1, x2, y2), px, py, x0, y0, x1, y1, x2, y2);
    const FaceP pw = face_perspective(w, z0, z1, z2);
    const float inv = w.inv, z = pw.z, bw0 = pw.b0, bw1 = pw.b1, bw2 = pw.b2;
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

// the weights of level l: w0 [R,R] or the packed wpyr [S]
__host__ __device__ __forceinline__ const float *cov_level(const float *w0, const float *wpyr, int R, int l) {
    return l == 0 ? w0 : wpyr + mip_offset(R, l);
}

// Level l (side Rd) from level l - 1 (side 2 Rd): a coarse texel covers exactly four fine ones (texel centres,
// align_corners=False).  One thread per coarse texel and `cpb` channels, the channel group on blockIdx.y; `sstride` /
// `dstride` are the channel strides.  COV: the mean weighted by level l - 1's weights `wsrc` (not read otherwise).
template <bool COV>
__global__ void __launch_bounds__(256)
k_pyr_down(const float *__restrict__ src, int64_t sstride, const float *__restrict__ wsrc, float *__restrict__ dst,
           int64_t dstride, int C, int cpb, int Rd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rd * Rd) return;
    const int i = (int)(r / Rd), j = (int)(r - (int64_t)i * Rd);
    const int Rs = 2 * Rd;
    const int64_t at = (int64_t)(2 * i) * Rs + 2 * j;
    float wa = 1.f, wb = 1.f, wc = 1.f, wd = 1.f;
    if (COV) wa = wsrc[at], wb = wsrc[at + 1], wc = wsrc[at + Rs], wd = wsrc[at + Rs + 1];
    const float s = (wa + wb) + (wc + wd);
    for (int c = blockIdx.y * cpb, ce = min(c + cpb, C); c < ce; ++c) {
        const float *t = src + c * sstride + at;
        if (COV) dst[c * dstride + r] = s > 0.f ? ((wa * t[0] + wb * t[1]) + (wc * t[Rs] + wd * t[Rs + 1])) / s : 0.f;
        else dst[c * dstride + r] = ((t[0] + t[1]) + (t[Rs] + t[Rs + 1])) * 0.25f;
    }
}

// The transpose, as a gather: every fine texel (side Rf) adds a quarter of its one coarse parent's gradient, COV: (its
// weight / its block's sum) of it, and nothing where the block has no weight.  One thread per fine texel and `cpb`
// channels, as k_pyr_down.
template <bool COV>
__global__ void __launch_bounds__(256)
k_pyr_up(const float *__restrict__ dcoarse, int64_t cstride, const float *__restrict__ wfine, float *__restrict__ dfine,
         int64_t fstride, int C, int cpb, int Rf) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rf * Rf) return;
    const int i = (int)(r / Rf), j = (int)(r - (int64_t)i * Rf);
    float q = 0.25f;
    if (COV) {
        const float *b = wfine + (int64_t)(i & ~1) * Rf + (j & ~1);
        const float s = (b[0] + b[1]) + (b[Rf] + b[Rf + 1]);
        if (!(s > 0.f)) return;
        q = wfine[r] / s;
    }
    const int Rc = Rf / 2;
    const int64_t parent = (int64_t)(i / 2) * Rc + j / 2;
    for (int c = blockIdx.y * cpb, ce = min(c + cpb, C); c < ce; ++c)
        dfine[c * fstride + r] += q * dcoarse[c * cstride + parent];
}

// One level of the push; one thread per texel of level l (side Rf), every channel.  `wk` = the weights k is made of
// (LEVEL0: w0 itself; else level l - 1, side 2 Rf), `wtop` = the weights of level L (side Rtop), `shift` = L - (l + 1),
// `val` = level l (v on entry, F on exit), `coarse` = F of level l + 1 (side Rf / 2).  coarse == NULL (L = 0): there is
// nothing to push, only `filled` is cleared.
template <bool LEVEL0>
__global__ void __launch_bounds__(256)
k_cov_push(const float *__restrict__ wk, const float *__restrict__ wtop, int Rtop, int shift, float *val, int64_t vstride,
           const float *coarse, int64_t cstride, int C, int Rf, uint8_t *__restrict__ filled) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rf * Rf) return;
    if (LEVEL0 && !coarse) {
        if (filled) filled[r] = 0;
        return;
    }
    const int i = (int)(r / Rf), j = (int)(r - (int64_t)i * Rf);
    float k;
    if (LEVEL0) {
        k = wk[r];
    } else {
        const int Rs = 2 * Rf;
        const float *s = wk + (int64_t)(2 * i) * Rs + 2 * j;
        k = fminf((s[0] + s[1]) + (s[Rs] + s[Rs + 1]), 1.f);
    }
    const int Rc = Rf / 2;
    const int pi = i >> 1, pj = j >> 1;
    const int ni = (i & 1) ? min(pi + 1, Rc - 1) : max(pi - 1, 0), nj = (j & 1) ? min(pj + 1, Rc - 1) : max(pj - 1, 0);
    const float *tp = wtop + (int64_t)(pi >> shift) * Rtop, *tn = wtop + (int64_t)(ni >> shift) * Rtop;
    const bool write = tp[pj >> shift] > 0.f && k != 1.f;
    if (LEVEL0 && filled) filled[r] = write;
    if (!write) return;
    const bool rpn = tp[nj >> shift] > 0.f, rnp = tn[pj >> shift] > 0.f, rnn = tn[nj >> shift] > 0.f;
    const bool all = rpn && rnp && rnn;
    const float den = (0.5625f + (rpn ? 0.1875f : 0.f)) + ((rnp ? 0.1875f : 0.f) + (rnn ? 0.0625f : 0.f));
    const int64_t pp = (int64_t)pi * Rc + pj, pn = (int64_t)pi * Rc + nj, np = (int64_t)ni * Rc + pj, nn = (int64_t)ni * Rc + nj;
    for (int c = 0; c < C; ++c) {
        const float *F = coarse + c * cstride;
        float up = (0.5625f * F[pp] + (rpn ? 0.1875f * F[pn] : 0.f)) + ((rnp ? 0.1875f * F[np] : 0.f) + (rnn ? 0.0625f * F[nn] : 0.f));
        if (!all) up = up / den;
        float *v = val + c * vstride + r;
        *v = k == 0.f ? up : k * *v + (1.f - k) * up;
    }
}

// The four products b_k * W_k of one level's read, their sum in bil_read's order, and whether every W is exactly 1
struct CovTaps {
    float w00, w01, w10, w11, d;
    bool ones;
};
__device__ __forceinline__ CovTaps cov_taps(const float *wl, const BilTaps &b) {
    const float W00 = wl[b.i00], W01 = wl[b.i01], W10 = wl[b.i10], W11 = wl[b.i11];
    CovTaps c;
    c.w00 = b.w00 * W00; c.w01 = b.w01 * W01; c.w10 = b.w10 * W10; c.w11 = b.w11 * W11;
    c.d = c.w00 + c.w01 + c.w10 + c.w11;
    c.ones = W00 == 1.f && W01 == 1.f && W10 == 1.f && W11 == 1.f;
    return c;
}
__device__ __forceinline__ float cov_read(const float *tc, const BilTaps &b, const CovTaps &c) {
    return c.w00 * tc[b.i00] + c.w01 * tc[b.i01] + c.w10 * tc[b.i10] + c.w11 * tc[b.i11];
}
__device__ __forceinline__ void cov_add(float *tc, const BilTaps &b, const CovTaps &c, float q) {
    atomicAdd(&tc[b.i00], c.w00 * q); atomicAdd(&tc[b.i01], c.w01 * q);
    atomicAdd(&tc[b.i10], c.w10 * q); atomicAdd(&tc[b.i11], c.w11 * q);
}

// The normalised lookup (case (c) of the header) on levels l0 and, when mix != 0, l0 + 1, whose values and taps the
// caller has; returns false where the plain arithmetic applies instead: every weight read is 1 (a), or D == 0 (b).
template <bool BWD>
__device__ __forceinline__ bool mip_normalised(float *t0, const BilTaps &b0, float *t1, const BilTaps &b1, const float *w0,
                                               const float *wpyr, int R, int l0, float mix, float *o) {
    const bool two = mix != 0.f;
    const CovTaps c0 = cov_taps(cov_level(w0, wpyr, R, l0), b0);
    const CovTaps c1 = two ? cov_taps(cov_level(w0, wpyr, R, l0 + 1), b1) : c0;
    const float D = two ? (1.f - mix) * c0.d + mix * c1.d : c0.d;
    if ((c0.ones && c1.ones) || D == 0.f) return false;
    if (BWD) {
        const float g = *o;
        cov_add(t0, b0, c0, (two ? (1.f - mix) * g : g) / D);
        if (two) cov_add(t1, b1, c1, (mix * g) / D);
    } else {
        const float N = two ? (1.f - mix) * cov_read(t0, b0, c0) + mix * cov_read(t1, b1, c1) : cov_read(t0, b0, c0);
        *o = N / D;
    }
    return true;
}

// One thread per (pixel, channel), as k_texture_map.  tex = level 0 [C,R,R], pyr = levels 1..L packed [C,S]; in the
// backward both are the gradients the atomics add to.  COV: w0 / wpyr are the weights of the same levels (not read
// otherwise), and the plain lines below are its cases (a) and (b).
template <bool BWD, bool COV>
__global__ void __launch_bounds__(256)
k_texture_mip(const float *__restrict__ uv, const float *__restrict__ rho, const int32_t *__restrict__ face_idx,
              float *tex, float *pyr, const float *__restrict__ w0, const float *__restrict__ wpyr, int64_t P, int C,
              int R, int L, int64_t S, float bias, float *out_or_dout) {
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
        if (COV && mip_normalised<BWD>(t0, b0, t0, b0, w0, wpyr, R, l0, mix, &out_or_dout[t])) return;
        if (BWD) bil_add(t0, b0, out_or_dout[t]);
        else out_or_dout[t] = bil_read(t0, b0);
        return;
    }
    float *t1 = pyr + c * S + mip_offset(R, l0 + 1);   // mix > 0 only below level L
    const BilTaps b1 = bil_taps(u, v, R >> (l0 + 1));
    if (COV && mip_normalised<BWD>(t0, b0, t1, b1, w0, wpyr, R, l0, mix, &out_or_dout[t])) return;
    if (BWD) {
        const float g = out_or_dout[t];
        bil_add(t0, b0, (1.f - mix) * g);
        bil_add(t1, b1, mix * g);
    } else {
        out_or_dout[t] = (1.f - mix) * bil_read(t0, b0) + mix * bil_read(t1, b1);
    }
}

// ---- the launches.  `who` names the entry point in every error; w0 == NULL is the plain pyramid (the entry points of
// the weighted one refuse a NULL w0 before they come here).
// Channels per block of the pyramid kernels: the weighted ones take every channel, so a texel's weights are read once;
// the plain ones have nothing to share and take one (more only where C is beyond the grid's y range).
static int pyr_cpb(const float *w0, int C) { return w0 ? C : (int)div_up(C, 65535); }

static int pyr_build(const char *who, const float *texture, const float *w0, const float *wpyr, int C, int R, int L,
                     float *pyramid, lnerf_stream_t stream) {
    if (int rc = check_mip_shape(who, C, R, L)) return rc;
    LNERF_REQUIRE(texture && (pyramid || L == 0), "%s: null pointer", who);
    const int64_t S = mip_texels(R, L);
    const auto kernel = w0 ? k_pyr_down<true> : k_pyr_down<false>;
    const int cpb = pyr_cpb(w0, C);
    for (int l = 1; l <= L; ++l) {
        const int Rd = R >> l;
        const float *src = l == 1 ? texture : pyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(kernel, dim3((unsigned)div_up((int64_t)Rd * Rd, 256), (unsigned)div_up(C, cpb)), dim3(256), 0,
                           as_stream(stream), src, l == 1 ? (int64_t)R * R : S,
                           w0 ? cov_level(w0, wpyr, R, l - 1) : nullptr, pyramid + mip_offset(R, l), S, C, cpb, Rd);
        LNERF_CHECK_LAUNCH(who);
    }
    return LNERF_OK;
}

static int pyr_fold(const char *who, float *dpyramid, const float *w0, const float *wpyr, int C, int R, int L,
                    float *dtexture, lnerf_stream_t stream) {
    if (int rc = check_mip_shape(who, C, R, L)) return rc;
    LNERF_REQUIRE(dtexture && (dpyramid || L == 0), "%s: null pointer", who);
    const int64_t S = mip_texels(R, L);
    const auto kernel = w0 ? k_pyr_up<true> : k_pyr_up<false>;
    const int cpb = pyr_cpb(w0, C);
    for (int l = L; l >= 1; --l) {   // level l's gradient is complete once every coarser level has been folded into it
        const int Rf = R >> (l - 1);
        float *fine = l == 1 ? dtexture : dpyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(kernel, dim3((unsigned)div_up((int64_t)Rf * Rf, 256), (unsigned)div_up(C, cpb)), dim3(256), 0,
                           as_stream(stream), dpyramid + mip_offset(R, l), S,
                           w0 ? cov_level(w0, wpyr, R, l - 1) : nullptr, fine, l == 1 ? (int64_t)R * R : S, C, cpb, Rf);
        LNERF_CHECK_LAUNCH(who);
    }
    return LNERF_OK;
}

// forward: tex / pyr are read and `out_or_dout` written; backward: the other way round
template <bool BWD>
static int mip_lookup(const char *who, const float *uv, const float *rho, const int32_t *face_idx, float *tex, float *pyr,
                      const float *w0, const float *wpyr, int n_pixels, int C, int R, int L, float bias,
                      float *out_or_dout, lnerf_stream_t stream) {
    if (int rc = check_mip_shape(who, C, R, L)) return rc;
    LNERF_REQUIRE(n_pixels > 0, "%s: n_pixels must be > 0 (got %d)", who, n_pixels);
    LNERF_REQUIRE(__builtin_isfinite(bias), "%s: bias must be finite", who);
    LNERF_REQUIRE(uv && rho && tex && out_or_dout && (pyr || L == 0), "%s: null pointer", who);
    const auto kernel = w0 ? k_texture_mip<BWD, true> : k_texture_mip<BWD, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)div_up((int64_t)n_pixels * C, 256)), dim3(256), 0, as_stream(stream), uv,
                       rho, face_idx, tex, pyr, w0, wpyr, (int64_t)n_pixels, C, R, L, mip_texels(R, L), bias, out_or_dout);
    LNERF_CHECK_LAUNCH(who);
    return LNERF_OK;
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
    LNERF_LAUNCH(k_uv_footprint, P, 256, as_stream(stream), face_idx, face_xy, face_z, face_uv, P, H, W, n_faces, rho);
    LNERF_CHECK_LAUNCH("uv_footprint");
    return LNERF_OK;
}

int lnerf_mip_build(const float *texture, int C, int R, int L, float *pyramid, lnerf_stream_t stream) {
    return pyr_build("mip_build", texture, nullptr, nullptr, C, R, L, pyramid, stream);
}

int lnerf_mip_build_backward(float *dpyramid, int C, int R, int L, float *dtexture, lnerf_stream_t stream) {
    return pyr_fold("mip_build_backward", dpyramid, nullptr, nullptr, C, R, L, dtexture, stream);
}

int lnerf_texture_mip_forward(const float *uv, const float *rho, const int32_t *face_idx, const float *texture,
                              const float *pyramid, int n_pixels, int C, int R, int L, float bias, float *out,
                              lnerf_stream_t stream) {
    return mip_lookup<false>("texture_mip_forward", uv, rho, face_idx, const_cast<float *>(texture),
                             const_cast<float *>(pyramid), nullptr, nullptr, n_pixels, C, R, L, bias, out, stream);
}

int lnerf_texture_mip_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                               int n_pixels, int C, int R, int L, float bias, float *dtexture, float *dpyramid,
                               lnerf_stream_t stream) {
    return mip_lookup<true>("texture_mip_backward", uv, rho, face_idx, dtexture, dpyramid, nullptr, nullptr, n_pixels, C,
                            R, L, bias, const_cast<float *>(dout), stream);
}

int lnerf_mipcov_weights(const float *w0, int R, int L, float *wpyr, lnerf_stream_t stream) {
    return pyr_build("mipcov_weights", w0, nullptr, nullptr, 1, R, L, wpyr, stream);   // the plain build of one channel
}

int lnerf_mipcov_pull(const float *texture, const float *w0, const float *wpyr, int C, int R, int L, float *pyramid,
                      lnerf_stream_t stream) {
    LNERF_REQUIRE(w0 && (wpyr || L == 0), "mipcov_pull: null pointer");
    return pyr_build("mipcov_pull", texture, w0, wpyr, C, R, L, pyramid, stream);
}

int lnerf_mipcov_pull_backward(float *dpyramid, const float *w0, const float *wpyr, int C, int R, int L, float *dtexture,
                               lnerf_stream_t stream) {
    LNERF_REQUIRE(w0 && (wpyr || L == 0), "mipcov_pull_backward: null pointer");
    return pyr_fold("mipcov_pull_backward", dpyramid, w0, wpyr, C, R, L, dtexture, stream);
}

int lnerf_mipcov_push(float *texture, const float *w0, const float *wpyr, float *pyramid, int C, int R, int L,
                      uint8_t *filled, lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mipcov_push", C, R, L)) return rc;
    LNERF_REQUIRE(texture && w0 && ((pyramid && wpyr) || L == 0), "mipcov_push: null pointer");
    const int64_t S = mip_texels(R, L);
    const float *wtop = cov_level(w0, wpyr, R, L);
    const int Rtop = R >> L;
    for (int l = L - 1; l >= 1; --l) {   // F of level l + 1 is complete before level l reads it
        const int Rf = R >> l;
        hipLaunchKernelGGL(k_cov_push<false>, dim3((unsigned)div_up((int64_t)Rf * Rf, 256)), dim3(256), 0,
                           as_stream(stream), cov_level(w0, wpyr, R, l - 1), wtop, Rtop, L - (l + 1),
                           pyramid + mip_offset(R, l), S, pyramid + mip_offset(R, l + 1), S, C, Rf, (uint8_t *)nullptr);
        LNERF_CHECK_LAUNCH("mipcov_push");
    }
    if (L >= 1 || filled) {
        hipLaunchKernelGGL(k_cov_push<true>, dim3((unsigned)div_up((int64_t)R * R, 256)), dim3(256), 0, as_stream(stream),
                           w0, wtop, Rtop, L - 1, texture, (int64_t)R * R, L >= 1 ? pyramid + mip_offset(R, 1) : nullptr, S,
                           C, R, filled);
        LNERF_CHECK_LAUNCH("mipcov_push");
    }
    return LNERF_OK;
}

int lnerf_texture_mipcov_forward(const float *uv, const float *rho, const int32_t *face_idx, const float *texture,
                                 const float *pyramid, const float *w0, const float *wpyr, int n_pixels, int C, int R,
                                 int L, float bias, float *out, lnerf_stream_t stream) {
    LNERF_REQUIRE(w0 && (wpyr || L == 0), "texture_mipcov_forward: null pointer");
    return mip_lookup<false>("texture_mipcov_forward", uv, rho, face_idx, const_cast<float *>(texture),
                             const_cast<float *>(pyramid), w0, wpyr, n_pixels, C, R, L, bias, out, stream);
}

int lnerf_texture_mipcov_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                                  const float *w0, const float *wpyr, int n_pixels, int C, int R, int L, float bias,
                                  float *dtexture, float *dpyramid, lnerf_stream_t stream) {
    LNERF_REQUIRE(w0 && (wpyr || L == 0), "texture_mipcov_backward: null pointer");
    return mip_lookup<true>("texture_mipcov_backward", uv, rho, face_idx, dtexture, dpyramid, w0, wpyr, n_pixels, C, R, L,
                            bias, const_cast<float *>(dout), stream);
}

}  // extern "C"
