// Multi-view projection of images onto surface points: the kernel behind NeRFRenderer.bake_views and Latent-Paint's
// view bake (src/view_bake.py).  Contract and the rule per (point, view): include/lnerf_hip.h, lnerf_uv_project_views;
// float64 restatement: tests/test_gpu_view_bake.py.
//
// k_uv_project: one lane per point, 256 per workgroup.  The camera records are staged into LDS once per workgroup
// (PROJ_CAM_TILE at a time, so any K fits), and every lane of a wave reads the same record: a broadcast.  A lane walks
// the views in ascending k and keeps its sums in registers, so the result does not depend on the launch shape and
// needs no atomics.  The z-buffer and image taps are gathers; neighbouring texels of a chart are neighbouring surface
// points, so a wave's taps of one view fall into a few cache lines of that view's planes.
#include "view_shared.h"

namespace lnerf {

struct ProjArgs {
    const float *pos, *nrm, *cams, *zbuf, *images;
    int64_t P;
    int K, H, W, C;
    float cos_min, power, slack;
    float *out, *weight;
    int32_t *count;
};

__global__ void __launch_bounds__(PROJ_THREADS) k_uv_project(ProjArgs a) {
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
    float acc[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f}, first[PROJ_MAX_C] = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f;
    int cnt = 0;
    for (int k0 = 0; k0 < a.K; k0 += PROJ_CAM_TILE) {
        const int nk = min(PROJ_CAM_TILE, a.K - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < nk * CAM_FLOATS; t += PROJ_THREADS) s_cam[t] = a.cams[(int64_t)k0 * CAM_FLOATS + t];
        __syncthreads();
        if (!live) continue;
        for (int kk = 0; kk < nk; ++kk) {
            const int k = k0 + kk;
            ViewTap t;
            // 1-5. does the point accept this view (view_shared.h)
            if (!view_accept(x, n, s_cam + kk * CAM_FLOATS, a.zbuf + (int64_t)k * plane, a.W, Wf, Hf, a.cos_min, a.slack, t)) continue;
            // 6. accumulate the weighted mean around the first accepted colour: the differences are exact zeros where
            // the taps or the views agree, so a colour all views share comes back as it is
            const float w = powf(t.c, a.power);
            const float *im = a.images + (int64_t)k * a.C * plane + t.off;
#pragma unroll
            for (int ch = 0; ch < PROJ_MAX_C; ++ch) {
                if (ch < a.C) {
                    const float col = view_bilinear(im + ch * plane, a.W, t.tu, t.tv);
                    if (cnt == 0) first[ch] = col;
                    acc[ch] += w * (col - first[ch]);
                }
            }
            wsum += w;
            ++cnt;
        }
    }
    if (!live) return;
#pragma unroll
    for (int ch = 0; ch < PROJ_MAX_C; ++ch)
        if (ch < a.C) a.out[p * a.C + ch] = wsum > 0.f ? first[ch] + acc[ch] / wsum : 0.f;
    a.weight[p] = wsum;
    a.count[p] = cnt;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_uv_project_views(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                           const float *zbuf, const float *images, int C, float cos_min, float power, float slack,
                           float *out, float *weight, int32_t *count, lnerf_stream_t stream) {
    LNERF_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "uv_project_views: P = %lld outside [0, 2^31)", (long long)P);
    LNERF_REQUIRE(K >= 1 && K <= 65535, "uv_project_views: K must be in [1, 65535]");
    LNERF_REQUIRE(H >= 2 && W >= 2 && H <= 32767 && W <= 32767, "uv_project_views: H and W must be in [2, 32767]");
    LNERF_REQUIRE(C >= 1 && C <= PROJ_MAX_C, "uv_project_views: C must be in [1, %d]", PROJ_MAX_C);
    LNERF_REQUIRE(cos_min > 0.f && cos_min <= 1.f, "uv_project_views: cos_min must be in (0, 1]");
    LNERF_REQUIRE(power >= 0.f && power < 3.0e38f && slack >= 0.f && slack < 3.0e38f,
                  "uv_project_views: power and slack must be finite and >= 0");
    LNERF_REQUIRE(cams_dev && zbuf && images, "uv_project_views: null pointer");
    if (P == 0) return LNERF_OK;
    LNERF_REQUIRE(pos && nrm && out && weight && count, "uv_project_views: null pointer");
    ProjArgs a;
    a.pos = pos; a.nrm = nrm; a.cams = cams_dev; a.zbuf = zbuf; a.images = images;
    a.P = P; a.K = K; a.H = H; a.W = W; a.C = C;
    a.cos_min = cos_min; a.power = power; a.slack = slack;
    a.out = out; a.weight = weight; a.count = count;
    LNERF_LAUNCH(k_uv_project, P, PROJ_THREADS, as_stream(stream), a);
    LNERF_CHECK_LAUNCH("uv_project_views");
    return LNERF_OK;
}

}  // extern "C"
