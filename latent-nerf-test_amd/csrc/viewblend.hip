// Exposure matching and two-band blending of a view bake (src/view_bake.py, blend = "bands" / exposure = True).
// Contracts: include/lnerf_hip.h (lnerf_view_lowpass, lnerf_view_overlap_stats, lnerf_uv_project_views_bands); float64
// restatement: tests/view_blend_reference.py.  Which views a point accepts is view_shared.h's decision, the one
// k_uv_project takes.
//
// k_lowpass_rows / k_lowpass_cols: one lane per pixel of one view, all channels; a lane walks its 2r + 1 taps in
//   ascending order, so the sums have one order whatever the launch shape.  Neighbouring lanes read neighbouring
//   pixels (the rows pass along the row, the columns pass one row at a time), so every tap is a coalesced load.
// k_overlap_stats: one lane per point.  A wave first finds, view by view, which lanes accept it (a ballot), then walks
//   the ordered pairs (i, j) of the views ANY of its lanes accepted: the lanes that accept both contribute, the wave
//   sums their fixed-point samples (64-bit butterfly) and lane 0 adds the pair's count and sums with 64-bit integer
//   atomics.  That is one atomic per wave, pair and word instead of one per point: the [K,K] tables are a few KiB and
//   every point of a chart hits the same few pairs, so unaggregated adds would all queue on the same addresses.
//   Integer sums do not depend on the order the atomics land in: the tables are bitwise reproducible.
// k_uv_project_bands: k_uv_project with a second image stack (the low band), optional gains and the best view.
#include "view_shared.h"

namespace lnerf {

constexpr int LOWPASS_MAX_R = LNERF_LOWPASS_MAX_R;
constexpr int STATS_MAX_K = LNERF_STATS_MAX_K;   // a lane keeps its accepted views as one 64-bit mask

struct LowpassArgs {
    const float *images, *zbuf;
    float *num, *den, *low;
    int64_t pixels;   // K * H * W
    int C, H, W, r;
    float g[2 * LOWPASS_MAX_R + 1];
};

// pass 1: num [K,C,H,W] = sum_t g[t] I(i, j + t), den [K,H,W] = sum_t g[t], over the taps inside the row AND usable
__global__ void __launch_bounds__(256) k_lowpass_rows(LowpassArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.pixels) return;
    const int j = (int)(idx % a.W);
    const int64_t row = idx / a.W;                       // k * H + i
    const int64_t k = row / a.H, i = row - k * a.H, plane = (int64_t)a.H * a.W;
    const float *z = a.zbuf + row * a.W;
    const float *im = a.images + k * a.C * plane + i * a.W;
    float den = 0.f, num[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f};
    const int lo = max(-a.r, -j), hi = min(a.r, a.W - 1 - j);
    for (int t = lo; t <= hi; ++t) {
        if (!(z[j + t] < 0.f)) continue;                 // skipped, never multiplied by 0: its colour may be NaN
        const float g = a.g[t + a.r];
        den += g;
#pragma unroll
        for (int ch = 0; ch < PROJ_MAX_C; ++ch)
            if (ch < a.C) num[ch] += g * im[ch * plane + j + t];
    }
    a.den[idx] = den;
#pragma unroll
    for (int ch = 0; ch < PROJ_MAX_C; ++ch)
        if (ch < a.C) a.num[(k * a.C + ch) * plane + i * a.W + j] = num[ch];
}

// pass 2: the same sums of num and den down the column, over the taps inside the image; low = num / den
__global__ void __launch_bounds__(256) k_lowpass_cols(LowpassArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.pixels) return;
    const int j = (int)(idx % a.W);
    const int64_t row = idx / a.W;
    const int64_t k = row / a.H, plane = (int64_t)a.H * a.W;
    const int i = (int)(row - k * a.H);
    const float *d = a.den + k * plane + j;
    const float *nm = a.num + k * a.C * plane + j;
    float den = 0.f, num[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f};
    const int lo = max(-a.r, -i), hi = min(a.r, a.H - 1 - i);
    for (int t = lo; t <= hi; ++t) {
        const float g = a.g[t + a.r];
        const int64_t o = (int64_t)(i + t) * a.W;
        den += g * d[o];
#pragma unroll
        for (int ch = 0; ch < PROJ_MAX_C; ++ch)
            if (ch < a.C) num[ch] += g * nm[ch * plane + o];
    }
#pragma unroll
    for (int ch = 0; ch < PROJ_MAX_C; ++ch)
        if (ch < a.C) a.low[(k * a.C + ch) * plane + (int64_t)i * a.W + j] = den > 0.f ? num[ch] / den : 0.f;
}

struct StatsArgs {
    const float *pos, *nrm, *cams, *zbuf, *low;
    int64_t P;
    int K, H, W, C;
    float cos_min, slack;
    unsigned long long *N, *S;
};

// sum over the wave's 64 lanes, in every lane (all lanes must be active)
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, LNERF_WAVE);
    return v;
}

__global__ void __launch_bounds__(PROJ_THREADS) k_overlap_stats(StatsArgs a) {
    static_assert(STATS_MAX_K <= 64, "the accepted views of a lane are one 64-bit mask");
    __shared__ float s_cam[STATS_MAX_K * CAM_FLOATS];
    for (int t = threadIdx.x; t < a.K * CAM_FLOATS; t += PROJ_THREADS) s_cam[t] = a.cams[t];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * PROJ_THREADS + threadIdx.x;
    const bool live = p < a.P;
    float x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[d] = a.pos[p * 3 + d];
            n[d] = a.nrm[p * 3 + d];
        }
    }
    const float Wf = (float)a.W, Hf = (float)a.H;
    const int64_t plane = (int64_t)a.H * a.W;
    // every lane stays in every loop below: the trip counts are the wave's, not the lane's
    unsigned long long mine = 0, wave = 0;
    for (int k = 0; k < a.K; ++k) {
        ViewTap t;
        const bool ok = live && view_accept(x, n, s_cam + k * CAM_FLOATS, a.zbuf + k * plane, a.W, Wf, Hf, a.cos_min, a.slack, t);
        if (ok) mine |= 1ull << k;
        if (__ballot(ok) != 0ull) wave |= 1ull << k;
    }
    for (unsigned long long wi = wave; wi != 0ull; wi &= wi - 1) {
        const int i = __ffsll((long long)wi) - 1;
        const bool has_i = (mine >> i) & 1ull;
        long long q[PROJ_MAX_C] = {0, 0, 0, 0};
        ViewTap t;
        // (the same arithmetic on the same inputs: accepted again, and the taps are inside the image)
        if (has_i && view_accept(x, n, s_cam + i * CAM_FLOATS, a.zbuf + i * plane, a.W, Wf, Hf, a.cos_min, a.slack, t)) {
            const float *lw = a.low + (int64_t)i * a.C * plane + t.off;
#pragma unroll
            for (int ch = 0; ch < PROJ_MAX_C; ++ch)
                if (ch < a.C) q[ch] = llrintf(view_bilinear(lw + ch * plane, a.W, t.tu, t.tv) * 16777216.0f);
        }
        for (unsigned long long wj = wave & ~(1ull << i); wj != 0ull; wj &= wj - 1) {
            const int j = __ffsll((long long)wj) - 1;
            const bool both = has_i && ((mine >> j) & 1ull);
            const unsigned long long who = __ballot(both);
            if (who == 0ull) continue;
            const int64_t cell = (int64_t)i * a.K + j;
            if (lane_id() == 0) atomicAdd(a.N + cell, (unsigned long long)__popcll(who));
#pragma unroll
            for (int ch = 0; ch < PROJ_MAX_C; ++ch) {
                if (ch < a.C) {
                    const long long s = wave_sum_i64(both ? q[ch] : 0ll);
                    if (lane_id() == 0) atomicAdd(a.S + cell * a.C + ch, (unsigned long long)s);
                }
            }
        }
    }
}

struct BandsArgs {
    const float *pos, *nrm, *cams, *zbuf, *images, *low, *gains;
    int64_t P;
    int K, H, W, C;
    float cos_min, power, slack;
    float *out, *weight;
    int32_t *count, *best;
};

__global__ void __launch_bounds__(PROJ_THREADS) k_uv_project_bands(BandsArgs a) {
    __shared__ float s_cam[PROJ_CAM_TILE * CAM_FLOATS];
    const int64_t p = (int64_t)blockIdx.x * PROJ_THREADS + threadIdx.x;
    const bool live = p < a.P;
    float x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[d] = a.pos[p * 3 + d];
            n[d] = a.nrm[p * 3 + d];
        }
    }
    const float Wf = (float)a.W, Hf = (float)a.H;
    const int64_t plane = (int64_t)a.H * a.W;
    float acc[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f}, first[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f};   // of the low band
    float best_i[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f}, best_l[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f, wbest = -1.0f;
    int cnt = 0, best = -1;
    for (int k0 = 0; k0 < a.K; k0 += PROJ_CAM_TILE) {
        const int nk = min(PROJ_CAM_TILE, a.K - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < nk * CAM_FLOATS; t += PROJ_THREADS) s_cam[t] = a.cams[(int64_t)k0 * CAM_FLOATS + t];
        __syncthreads();
        if (!live) continue;
        for (int kk = 0; kk < nk; ++kk) {
            const int k = k0 + kk;
            ViewTap t;
            if (!view_accept(x, n, s_cam + kk * CAM_FLOATS, a.zbuf + (int64_t)k * plane, a.W, Wf, Hf, a.cos_min, a.slack, t)) continue;
            const float w = powf(t.c, a.power);
            const bool better = w > wbest;          // strict: the lowest k wins an exact tie
            const int64_t at = (int64_t)k * a.C * plane + t.off;
#pragma unroll
            for (int ch = 0; ch < PROJ_MAX_C; ++ch) {
                if (ch < a.C) {
                    float col = view_bilinear(a.images + at + ch * plane, a.W, t.tu, t.tv);
                    float lw = view_bilinear(a.low + at + ch * plane, a.W, t.tu, t.tv);
                    if (a.gains) {                   // NULL: no multiplication, the samples keep their bits
                        const float g = a.gains[(int64_t)k * a.C + ch];
                        col = g * col;
                        lw = g * lw;
                    }
                    if (cnt == 0) first[ch] = lw;
                    acc[ch] += w * (lw - first[ch]);
                    if (better) {
                        best_i[ch] = col;
                        best_l[ch] = lw;
                    }
                }
            }
            if (better) {
                wbest = w;
                best = k;
            }
            wsum += w;
            ++cnt;
        }
    }
    if (!live) return;
#pragma unroll
    for (int ch = 0; ch < PROJ_MAX_C; ++ch) {
        if (ch < a.C) {
            const float lowmean = first[ch] + acc[ch] / wsum;
            a.out[p * a.C + ch] = wsum > 0.f ? best_i[ch] + (lowmean - best_l[ch]) : 0.f;
        }
    }
    a.weight[p] = wsum;
    a.count[p] = cnt;
    a.best[p] = best;
}

static bool lowpass_shape_ok(int K, int C, int H, int W) {
    return K >= 1 && K <= 65535 && C >= 1 && C <= PROJ_MAX_C && H >= 1 && W >= 1 && H <= 32767 && W <= 32767 &&
           (int64_t)K * C * H * W < ((int64_t)1 << 31);
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

size_t lnerf_view_lowpass_scratch_bytes(int K, int C, int H, int W) {
    if (!lowpass_shape_ok(K, C, H, W)) return 0;
    return (size_t)K * (size_t)(C + 1) * (size_t)H * (size_t)W * sizeof(float);
}

int lnerf_view_lowpass(const float *images, const float *zbuf, int K, int C, int H, int W, const float *taps_host, int r,
                       void *scratch, size_t scratch_bytes, float *low, lnerf_stream_t stream) {
    LNERF_REQUIRE(lowpass_shape_ok(K, C, H, W),
                  "view_lowpass: needs 1 <= K <= 65535, 1 <= C <= %d, 1 <= H, W <= 32767 and K C H W < 2^31", PROJ_MAX_C);
    LNERF_REQUIRE(r >= 0 && r <= LOWPASS_MAX_R, "view_lowpass: r must be in [0, %d]", LOWPASS_MAX_R);
    LNERF_REQUIRE(images && zbuf && taps_host && scratch && low, "view_lowpass: null pointer");
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "view_lowpass: scratch must be 16-byte aligned");
    LNERF_REQUIRE(scratch_bytes >= lnerf_view_lowpass_scratch_bytes(K, C, H, W), "view_lowpass: scratch too small");
    LowpassArgs a;
    for (int t = 0; t <= 2 * r; ++t) {
        LNERF_REQUIRE(taps_host[t] >= 0.f && taps_host[t] <= 1.f, "view_lowpass: taps must be in [0, 1]");
        a.g[t] = taps_host[t];
    }
    for (int t = 2 * r + 1; t <= 2 * LOWPASS_MAX_R; ++t) a.g[t] = 0.f;
    a.images = images; a.zbuf = zbuf; a.low = low;
    a.pixels = (int64_t)K * H * W;
    a.num = (float *)scratch;
    a.den = a.num + (int64_t)K * C * H * W;
    a.C = C; a.H = H; a.W = W; a.r = r;
    LNERF_LAUNCH(k_lowpass_rows, a.pixels, 256, as_stream(stream), a);
    LNERF_CHECK_LAUNCH("view_lowpass (rows)");
    LNERF_LAUNCH(k_lowpass_cols, a.pixels, 256, as_stream(stream), a);
    LNERF_CHECK_LAUNCH("view_lowpass (columns)");
    return LNERF_OK;
}

int lnerf_view_overlap_stats(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                             const float *zbuf, const float *low, int C, float cos_min, float slack, int64_t *N, int64_t *S,
                             lnerf_stream_t stream) {
    LNERF_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "view_overlap_stats: P = %lld outside [0, 2^31)", (long long)P);
    LNERF_REQUIRE(K >= 1 && K <= STATS_MAX_K, "view_overlap_stats: K must be in [1, %d]", STATS_MAX_K);
    LNERF_REQUIRE(H >= 2 && W >= 2 && H <= 32767 && W <= 32767, "view_overlap_stats: H and W must be in [2, 32767]");
    LNERF_REQUIRE(C >= 1 && C <= PROJ_MAX_C, "view_overlap_stats: C must be in [1, %d]", PROJ_MAX_C);
    LNERF_REQUIRE(cos_min > 0.f && cos_min <= 1.f, "view_overlap_stats: cos_min must be in (0, 1]");
    LNERF_REQUIRE(slack >= 0.f && slack < 3.0e38f, "view_overlap_stats: slack must be finite and >= 0");
    LNERF_REQUIRE(cams_dev && zbuf && low && N && S, "view_overlap_stats: null pointer");
    if (P == 0) return LNERF_OK;
    LNERF_REQUIRE(pos && nrm, "view_overlap_stats: null pointer");
    StatsArgs a;
    a.pos = pos; a.nrm = nrm; a.cams = cams_dev; a.zbuf = zbuf; a.low = low;
    a.P = P; a.K = K; a.H = H; a.W = W; a.C = C;
    a.cos_min = cos_min; a.slack = slack;
    a.N = (unsigned long long *)N; a.S = (unsigned long long *)S;
    LNERF_LAUNCH(k_overlap_stats, P, PROJ_THREADS, as_stream(stream), a);
    LNERF_CHECK_LAUNCH("view_overlap_stats");
    return LNERF_OK;
}

int lnerf_uv_project_views_bands(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                                 const float *zbuf, const float *images, const float *low, const float *gains, int C,
                                 float cos_min, float power, float slack, float *out, float *weight, int32_t *count,
                                 int32_t *best, lnerf_stream_t stream) {
    LNERF_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "uv_project_views_bands: P = %lld outside [0, 2^31)", (long long)P);
    LNERF_REQUIRE(K >= 1 && K <= 65535, "uv_project_views_bands: K must be in [1, 65535]");
    LNERF_REQUIRE(H >= 2 && W >= 2 && H <= 32767 && W <= 32767, "uv_project_views_bands: H and W must be in [2, 32767]");
    LNERF_REQUIRE(C >= 1 && C <= PROJ_MAX_C, "uv_project_views_bands: C must be in [1, %d]", PROJ_MAX_C);
    LNERF_REQUIRE(cos_min > 0.f && cos_min <= 1.f, "uv_project_views_bands: cos_min must be in (0, 1]");
    LNERF_REQUIRE(power >= 0.f && power < 3.0e38f && slack >= 0.f && slack < 3.0e38f,
                  "uv_project_views_bands: power and slack must be finite and >= 0");
    LNERF_REQUIRE(cams_dev && zbuf && images && low, "uv_project_views_bands: null pointer");
    if (P == 0) return LNERF_OK;
    LNERF_REQUIRE(pos && nrm && out && weight && count && best, "uv_project_views_bands: null pointer");
    BandsArgs a;
    a.pos = pos; a.nrm = nrm; a.cams = cams_dev; a.zbuf = zbuf; a.images = images; a.low = low; a.gains = gains;
    a.P = P; a.K = K; a.H = H; a.W = W; a.C = C;
    a.cos_min = cos_min; a.power = power; a.slack = slack;
    a.out = out; a.weight = weight; a.count = count; a.best = best;
    LNERF_LAUNCH(k_uv_project_bands, P, PROJ_THREADS, as_stream(stream), a);
    LNERF_CHECK_LAUNCH("uv_project_views_bands");
    return LNERF_OK;
}

}  // extern "C"
