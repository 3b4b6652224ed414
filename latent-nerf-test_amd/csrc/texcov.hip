// Coverage-weighted texture pyramids: a pyramid whose level l is the coverage-weighted mean of level l - 1, with the
// weights carried along, read either normalised (`guide.texture_mip_coverage`) or pushed back down into the texels no
// surface point owns (the pull-push fill of the exports).  All stated in include/lnerf_hip.h:
//   lnerf_mipcov_weights           k_cov_weights    w_l = the 2 x 2 box average of w_{l-1}, one launch per level
//   lnerf_mipcov_pull (+ bwd)      k_cov_pull/up    v_l = sum w v / sum w over the four children (0 where nothing is
//                                                   covered); the backward is the transpose in gather form (no atomics)
//   lnerf_mipcov_push              k_cov_push       from the coarsest level down, F_l = k v_l + (1 - k) up(F_{l+1})
//   lnerf_texture_mipcov_* (f/b)   k_texture_mipcov k_texture_mip's levels and taps, numerator and denominator filtered
//                                                   alike and divided
// The packing, the taps and the shape check are texmip.hip's (tex_shared.h).  The pyramid kernels run one lane per texel
// and loop over the channels, so a texel's weights are read once.
#include <math.h>

#include "common.h"
#include "tex_shared.h"

namespace lnerf {

// the weights of level l: w0 [R,R] or the packed wpyr [S]
__host__ __device__ __forceinline__ const float *cov_level(const float *w0, const float *wpyr, int R, int l) {
    return l == 0 ? w0 : wpyr + mip_offset(R, l);
}

// Level l (side Rd) of the weights from level l - 1 (side 2 Rd); one thread per coarse texel.
__global__ void __launch_bounds__(256)
k_cov_weights(const float *__restrict__ src, float *__restrict__ dst, int Rd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rd * Rd) return;
    const int i = (int)(r / Rd), j = (int)(r - (int64_t)i * Rd);
    const int Rs = 2 * Rd;
    const float *s = src + (int64_t)(2 * i) * Rs + 2 * j;
    dst[r] = ((s[0] + s[1]) + (s[Rs] + s[Rs + 1])) * 0.25f;
}

// Level l (side Rd) of the values from level l - 1 and its weights `wsrc`; one thread per coarse texel, every channel.
__global__ void __launch_bounds__(256)
k_cov_pull(const float *__restrict__ src, int64_t sstride, const float *__restrict__ wsrc, float *__restrict__ dst,
           int64_t dstride, int C, int Rd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rd * Rd) return;
    const int i = (int)(r / Rd), j = (int)(r - (int64_t)i * Rd);
    const int Rs = 2 * Rd;
    const int64_t at = (int64_t)(2 * i) * Rs + 2 * j;
    const float wa = wsrc[at], wb = wsrc[at + 1], wc = wsrc[at + Rs], wd = wsrc[at + Rs + 1];
    const float s = (wa + wb) + (wc + wd);
    for (int c = 0; c < C; ++c) {
        const float *t = src + c * sstride + at;
        dst[c * dstride + r] = s > 0.f ? ((wa * t[0] + wb * t[1]) + (wc * t[Rs] + wd * t[Rs + 1])) / s : 0.f;
    }
}

// The transpose, as a gather: every fine texel (side Rf) adds (its weight / its block's sum) of its one coarse parent's
// gradient; one thread per fine texel, every channel.
__global__ void __launch_bounds__(256)
k_cov_up(const float *__restrict__ dcoarse, int64_t cstride, const float *__restrict__ wfine, float *__restrict__ dfine,
         int64_t fstride, int C, int Rf) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)Rf * Rf) return;
    const int i = (int)(r / Rf), j = (int)(r - (int64_t)i * Rf);
    const float *b = wfine + (int64_t)(i & ~1) * Rf + (j & ~1);
    const float s = (b[0] + b[1]) + (b[Rf] + b[Rf + 1]);
    if (!(s > 0.f)) return;
    const float q = wfine[r] / s;
    const int Rc = Rf / 2;
    const int64_t parent = (int64_t)(i / 2) * Rc + j / 2;
    for (int c = 0; c < C; ++c) dfine[c * fstride + r] += q * dcoarse[c * cstride + parent];
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

// k_texture_mip with the weights: the same thread per (pixel, channel), lambda, l0, t and taps.  tex / pyr are the
// values (the gradients the atomics add to when BWD), w0 / wpyr the weights of the same levels.
template <bool BWD>
__global__ void __launch_bounds__(256)
k_texture_mipcov(const float *__restrict__ uv, const float *__restrict__ rho, const int32_t *__restrict__ face_idx,
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
    const bool two = mix != 0.f;          // mix > 0 only below level L
    float *t0 = l0 == 0 ? tex + (int64_t)c * R * R : pyr + c * S + mip_offset(R, l0);
    float *t1 = two ? pyr + c * S + mip_offset(R, l0 + 1) : t0;
    const BilTaps b0 = bil_taps(u, v, R >> l0);
    const BilTaps b1 = two ? bil_taps(u, v, R >> (l0 + 1)) : b0;
    const CovTaps c0 = cov_taps(cov_level(w0, wpyr, R, l0), b0);
    const CovTaps c1 = two ? cov_taps(cov_level(w0, wpyr, R, l0 + 1), b1) : c0;
    const float D = two ? (1.f - mix) * c0.d + mix * c1.d : c0.d;
    const bool plain = (c0.ones && c1.ones) || D == 0.f;   // case (a) and case (b): the plain mode's taps
    if (BWD) {
        const float g = out_or_dout[t];
        const float g0 = two ? (1.f - mix) * g : g, g1 = mix * g;
        if (plain) {
            bil_add(t0, b0, g0);
            if (two) bil_add(t1, b1, g1);
        } else {
            cov_add(t0, b0, c0, g0 / D);
            if (two) cov_add(t1, b1, c1, g1 / D);
        }
    } else if (plain) {
        out_or_dout[t] = two ? (1.f - mix) * bil_read(t0, b0) + mix * bil_read(t1, b1) : bil_read(t0, b0);
    } else {
        const float N = two ? (1.f - mix) * cov_read(t0, b0, c0) + mix * cov_read(t1, b1, c1) : cov_read(t0, b0, c0);
        out_or_dout[t] = N / D;
    }
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_mipcov_weights(const float *w0, int R, int L, float *wpyr, lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mipcov_weights", 1, R, L)) return rc;
    LNERF_REQUIRE(w0 && (wpyr || L == 0), "mipcov_weights: null pointer");
    for (int l = 1; l <= L; ++l) {
        const int Rd = R >> l;
        hipLaunchKernelGGL(k_cov_weights, dim3((unsigned)div_up((int64_t)Rd * Rd, 256)), dim3(256), 0, as_stream(stream),
                           cov_level(w0, wpyr, R, l - 1), wpyr + mip_offset(R, l), Rd);
        LNERF_CHECK_LAUNCH("mipcov_weights");
    }
    return LNERF_OK;
}

int lnerf_mipcov_pull(const float *texture, const float *w0, const float *wpyr, int C, int R, int L, float *pyramid,
                      lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mipcov_pull", C, R, L)) return rc;
    LNERF_REQUIRE(texture && w0 && ((pyramid && wpyr) || L == 0), "mipcov_pull: null pointer");
    const int64_t S = mip_texels(R, L);
    for (int l = 1; l <= L; ++l) {
        const int Rd = R >> l;
        const float *src = l == 1 ? texture : pyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(k_cov_pull, dim3((unsigned)div_up((int64_t)Rd * Rd, 256)), dim3(256), 0, as_stream(stream), src,
                           l == 1 ? (int64_t)R * R : S, cov_level(w0, wpyr, R, l - 1), pyramid + mip_offset(R, l), S, C, Rd);
        LNERF_CHECK_LAUNCH("mipcov_pull");
    }
    return LNERF_OK;
}

int lnerf_mipcov_pull_backward(float *dpyramid, const float *w0, const float *wpyr, int C, int R, int L, float *dtexture,
                               lnerf_stream_t stream) {
    if (int rc = check_mip_shape("mipcov_pull_backward", C, R, L)) return rc;
    LNERF_REQUIRE(dtexture && w0 && ((dpyramid && wpyr) || L == 0), "mipcov_pull_backward: null pointer");
    const int64_t S = mip_texels(R, L);
    for (int l = L; l >= 1; --l) {   // level l's gradient is complete once every coarser level has been folded into it
        const int Rf = R >> (l - 1);
        float *fine = l == 1 ? dtexture : dpyramid + mip_offset(R, l - 1);
        hipLaunchKernelGGL(k_cov_up, dim3((unsigned)div_up((int64_t)Rf * Rf, 256)), dim3(256), 0, as_stream(stream),
                           dpyramid + mip_offset(R, l), S, cov_level(w0, wpyr, R, l - 1), fine,
                           l == 1 ? (int64_t)R * R : S, C, Rf);
        LNERF_CHECK_LAUNCH("mipcov_pull_backward");
    }
    return LNERF_OK;
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
    if (int rc = check_mip_shape("texture_mipcov_forward", C, R, L)) return rc;
    LNERF_REQUIRE(n_pixels > 0, "texture_mipcov_forward: n_pixels must be > 0 (got %d)", n_pixels);
    LNERF_REQUIRE(__builtin_isfinite(bias), "texture_mipcov_forward: bias must be finite");
    LNERF_REQUIRE(uv && rho && texture && w0 && out && ((pyramid && wpyr) || L == 0),
                  "texture_mipcov_forward: null pointer");
    hipLaunchKernelGGL(k_texture_mipcov<false>, dim3((unsigned)div_up((int64_t)n_pixels * C, 256)), dim3(256), 0,
                       as_stream(stream), uv, rho, face_idx, const_cast<float *>(texture), const_cast<float *>(pyramid),
                       w0, wpyr, (int64_t)n_pixels, C, R, L, mip_texels(R, L), bias, out);
    LNERF_CHECK_LAUNCH("texture_mipcov_forward");
    return LNERF_OK;
}

int lnerf_texture_mipcov_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                                  const float *w0, const float *wpyr, int n_pixels, int C, int R, int L, float bias,
                                  float *dtexture, float *dpyramid, lnerf_stream_t stream) {
    if (int rc = check_mip_shape("texture_mipcov_backward", C, R, L)) return rc;
    LNERF_REQUIRE(n_pixels > 0, "texture_mipcov_backward: n_pixels must be > 0 (got %d)", n_pixels);
    LNERF_REQUIRE(__builtin_isfinite(bias), "texture_mipcov_backward: bias must be finite");
    LNERF_REQUIRE(uv && rho && dout && w0 && dtexture && ((dpyramid && wpyr) || L == 0),
                  "texture_mipcov_backward: null pointer");
    hipLaunchKernelGGL(k_texture_mipcov<true>, dim3((unsigned)div_up((int64_t)n_pixels * C, 256)), dim3(256), 0,
                       as_stream(stream), uv, rho, face_idx, dtexture, dpyramid, w0, wpyr, (int64_t)n_pixels, C, R, L,
                       mip_texels(R, L), bias, const_cast<float *>(dout));
    LNERF_CHECK_LAUNCH("texture_mipcov_backward");
    return LNERF_OK;
}

}  // extern "C"
