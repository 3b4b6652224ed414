// Shaded training renders (shading = "lambertian" / "textureless"): the kernels around the field.
// Contract: include/lnerf_hip.h, "shaded renders"; numpy restatement: tests/shading_reference.py.
//
//   k_fd_points   sample -> itself + its six +-eps neighbours (clamped to the box), rows 7 i .. 7 i + 6, and m7 = 7 m
//   k_shade_fwd<C, ORIENT>   the seven densities of a sample -> finite-difference normal -> Lambert term -> colour
//   k_shade_bwd<C, ORIENT>   recomputes the normal and the Lambert term, writes the gradient of all seven rows (one writer
//                  each)
//   ORIENT = true  the same with the orientation term fused in: orient[ray] = sum_i w_i max(0, n_i . v)^2, w the
//                  compositing weight (span_walk.h's, scanned here, detached), its gradient added to dn before the projection
// The finite-difference normal and its backward projection are span_walk.h's, shared with normal_image.hip.
//
// All arithmetic is f32 + - * / sqrt in the stated order: the library is built with -ffp-contract=off and nothing here
// is an explicit fmaf, so the numpy restatement matches bit for bit.
#include "span_walk.h"

namespace lnerf {

constexpr int FD_BLOCK = 256;
constexpr int FD_FLOATS = FD_ROWS * 3;       // floats of pts7 per sample (FD_ROWS: the sample and its six neighbours)

// One lane per sample.  The 21 floats of a sample are contiguous in pts7, so the 64 samples of a wave own one
// contiguous span of 64 * 84 bytes: it is staged in LDS and stored with consecutive lanes on consecutive floats.
__global__ void __launch_bounds__(FD_BLOCK)
k_fd_points(const float *__restrict__ xyzs, float bound, float eps, int64_t m_host, const int32_t *__restrict__ m_dev,
            float *__restrict__ pts7, int32_t *__restrict__ m7_dev) {
    __shared__ float stage[FD_BLOCK * FD_FLOATS];
    int64_t M = valid_count(m_host, m_dev);
    if (M < 0) M = 0;
    if (m7_dev && blockIdx.x == 0 && threadIdx.x == 0) m7_dev[0] = (int32_t)(FD_ROWS * M);
    for (int64_t base = (int64_t)blockIdx.x * FD_BLOCK; base < M; base += (int64_t)gridDim.x * FD_BLOCK) {   // block-uniform
        const int64_t i = base + threadIdx.x;
        if (i < M) {
            const float p[3] = {xyzs[i * 3], xyzs[i * 3 + 1], xyzs[i * 3 + 2]};
            float *row = stage + threadIdx.x * FD_FLOATS;
#pragma unroll
            for (int k = 0; k < FD_ROWS; ++k) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float v = p[a];
                    if (k == 1 + 2 * a) v = clampf(p[a] + eps, -bound, bound);
                    if (k == 2 + 2 * a) v = clampf(p[a] - eps, -bound, bound);
                    row[k * 3 + a] = v;
                }
            }
        }
        __syncthreads();
        const int64_t left = M - base;
        const int n = (int)(left < FD_BLOCK ? left : FD_BLOCK) * FD_FLOATS;
        float *dst = pts7 + base * FD_FLOATS;
        for (int j = threadIdx.x; j < n; j += FD_BLOCK) dst[j] = stage[j];
        __syncthreads();
    }
}

// per-view record: unit vector toward the light, ambient share, textureless flag
struct Light {
    float l[3], ambient, diffuse;   // diffuse = 1 - ambient
    bool textureless;
};
__device__ __forceinline__ Light load_light(const float *__restrict__ shade, int64_t id, int rays_per_view, int B) {
    int64_t b = id / rays_per_view;
    b = b < 0 ? 0 : (b >= B ? B - 1 : b);          // (a ray id past the last view reads the last record, never past it)
    const float *s = shade + b * 5;
    Light L;
    L.l[0] = s[0]; L.l[1] = s[1]; L.l[2] = s[2];
    L.ambient = s[3];
    L.diffuse = 1.0f - s[3];
    L.textureless = s[4] != 0.f;
    return L;
}

// one lane's sample: the seven densities and the albedo (row 7 i of the field's colours)
template <int C>
struct Sample7 {
    float sg[FD_ROWS], alb[C];
};
template <int C>
__device__ __forceinline__ Sample7<C> load_sample7(const float *__restrict__ sigmas7, const float *__restrict__ rgbs7,
                                                   int64_t off, int cnt, int i) {
    Sample7<C> k;
#pragma unroll
    for (int j = 0; j < FD_ROWS; ++j) k.sg[j] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) k.alb[c] = 0.f;
    if (i < cnt) {
        const int64_t s7 = (off + i) * FD_ROWS;
        load_fd_rows(sigmas7, s7, k.sg);
        load_row<C>(rgbs7, s7, k.alb);
    }
    return k;
}

// finite-difference normal of one sample and its Lambert term
struct Lambert : FdNormal {
    float d, lam;
};
__device__ __forceinline__ Lambert lambert_of(const float (&sg)[FD_ROWS], float inv_2eps, const Light &L) {
    Lambert o = {fd_normal(sg, inv_2eps)};
    o.d = (o.n[0] * L.l[0] + o.n[1] * L.l[1]) + o.n[2] * L.l[2];
    o.lam = L.ambient + L.diffuse * (o.d > 0.f ? o.d : 0.f);
    return o;
}

// the forward's two rows of sample s: its own density and its shaded colour
template <int C>
__device__ __forceinline__ void store_shaded(const Sample7<C> &k, const Lambert &o, const Light &L, int64_t s,
                                             float *__restrict__ sigma_c, float *__restrict__ colours) {
    sigma_c[s] = k.sg[0];
    float col[C];
#pragma unroll
    for (int c = 0; c < C; ++c) col[c] = L.textureless ? o.lam : k.alb[c] * o.lam;
    store_row<C>(colours, s, col);
}

// ---- the orientation term (contract: include/lnerf_hip.h, "orientation regulariser"; numpy: tests/orient_reference.py)

// unit view direction of ray `id`
__device__ __forceinline__ void view_dir(const float *__restrict__ rays_d, int64_t id, float (&v)[3]) {
    const float d[3] = {rays_d[id * 3], rays_d[id * 3 + 1], rays_d[id * 3 + 2]};
    const float s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float r = 1.0f / sqrtf(fmaxf(s, 1e-20f));
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = d[a] * r;
}

// dt of sample i of the span (0 past its end)
__device__ __forceinline__ float load_dt(const float *__restrict__ deltas, int64_t off, int cnt, int i) {
    return i < cnt ? load_step(deltas, off + i).dt : 0.f;
}

// max(0, n . v)
__device__ __forceinline__ float facing_away(const FdNormal &o, const float (&v)[3]) {
    const float c = (o.n[0] * v[0] + o.n[1] * v[1]) + o.n[2] * v[2];
    return c > 0.f ? c : 0.f;
}

// What the orientation term adds to a kernel's arguments, as ONE trailing parameter: the plain instantiations' block is
// empty and their other arguments lie where they always did.
template <bool ORIENT>
struct OrientArgs {};
template <>
struct OrientArgs<true> {
    const float *deltas, *rays_d;
    float density_scale, T_thresh;
    float *orient;             // forward: the output, one element per ray id
    const float *d_orient;     // backward: its upstream gradient
};

// One wavefront per ray, lanes striding over the ray's samples; the next 64 samples' loads are requested before this
// chunk's arithmetic (the kernel is a few memory round trips long, nothing else).
// ORIENT: plus orient[id] = sum_i w_i q_i^2.  A ray without samples writes 0 (the buffer is uninitialised), so there is no
// early return, and the chunk's arithmetic runs on ALL 64 lanes: span_weight is a wave scan.
template <int C, bool ORIENT>
__global__ void __launch_bounds__(256)
k_shade_fwd(const float *__restrict__ sigmas7, const float *__restrict__ rgbs7, const int32_t *__restrict__ rays, int64_t N,
            int rays_per_view, const float *__restrict__ shade, int B, float inv_2eps, float *__restrict__ sigma_c,
            float *__restrict__ colours, OrientArgs<ORIENT> oa) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    if (!ORIENT && cnt <= 0) return;
    const Light L = load_light(shade, id, rays_per_view, B);
    float v[3], acc = 0.f, carry = 0.f, dt = 0.f;
    if constexpr (ORIENT) view_dir(oa.rays_d, id, v);
    Sample7<C> cur = load_sample7<C>(sigmas7, rgbs7, off, cnt, lane);
    if constexpr (ORIENT) dt = load_dt(oa.deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        Sample7<C> nxt = cur;
        float dt_nxt = dt;
        if (base + 64 < cnt) {
            nxt = load_sample7<C>(sigmas7, rgbs7, off, cnt, base + 64 + lane);
            if constexpr (ORIENT) dt_nxt = load_dt(oa.deltas, off, cnt, base + 64 + lane);
        }
        const int i = base + lane;
        const bool valid = i < cnt;
        if (ORIENT || valid) {
            const Lambert o = lambert_of(cur.sg, inv_2eps, L);
            if (valid) store_shaded<C>(cur, o, L, off + i, sigma_c, colours);
            if constexpr (ORIENT) {
                const float w = span_weight((oa.density_scale * cur.sg[0]) * dt, valid, oa.T_thresh, carry).w;
                const float q = facing_away(o, v);
                acc += w * (q * q);
            }
        }
        cur = nxt;
        dt = dt_nxt;
    }
    if constexpr (ORIENT) {
        acc = wave_sum(acc);
        if (lane == 0) oa.orient[id] = acc;
    }
}

// one lane's upstream gradient
template <int C>
struct Grad7 {
    float dsig, dcol[C];
};
template <int C>
__device__ __forceinline__ Grad7<C> load_grad7(const float *__restrict__ dsigma_c, const float *__restrict__ dcolours,
                                               int64_t off, int cnt, int i) {
    Grad7<C> k;
    k.dsig = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) k.dcol[c] = 0.f;
    if (i < cnt) {
        const int64_t s = off + i;
        k.dsig = dsigma_c[s];
        load_row<C>(dcolours, s, k.dcol);
    }
    return k;
}

// The backward's first half: gradient of the colours w.r.t. the normal (dn, before the projection onto its tangent plane)
// and the albedo.
template <int C>
__device__ __forceinline__ void lambert_grad(const Sample7<C> &cur, const Grad7<C> &gcur, const Lambert &o, const Light &L,
                                             float (&dn)[3], float (&dalb)[C]) {
    float dlam;
    if (L.textureless) {
        dlam = gcur.dcol[0];
#pragma unroll
        for (int c = 1; c < C; ++c) dlam = dlam + gcur.dcol[c];
#pragma unroll
        for (int c = 0; c < C; ++c) dalb[c] = 0.f;
    } else {
        dlam = gcur.dcol[0] * cur.alb[0];
#pragma unroll
        for (int c = 1; c < C; ++c) dlam = dlam + gcur.dcol[c] * cur.alb[c];
#pragma unroll
        for (int c = 0; c < C; ++c) dalb[c] = gcur.dcol[c] * o.lam;
    }
    const float k = L.diffuse * dlam;
#pragma unroll
    for (int a = 0; a < 3; ++a) dn[a] = o.d > 0.f ? k * L.l[a] : 0.f;
}

// The backward's second half: the seven rows of both outputs of the sample whose first row is s7 (dn -> the six offset
// densities' gradient is fd_normal_backward).
template <int C>
__device__ __forceinline__ void project_and_store(const Lambert &o, const float (&dn)[3], float dsig, const float (&dalb)[C],
                                                  float inv_2eps, int64_t s7, float *__restrict__ dsigmas7,
                                                  float *__restrict__ drgbs7) {
    store_fd_rows(dsigmas7, s7, dsig, fd_normal_backward(o, dn, inv_2eps));
    store_row<C>(drgbs7, s7, dalb);
    if (C == 4) {
        float4 *row = reinterpret_cast<float4 *>(drgbs7) + s7;
#pragma unroll
        for (int j = 1; j < FD_ROWS; ++j) row[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float *row = drgbs7 + s7 * C;
#pragma unroll
        for (int j = C; j < FD_ROWS * C; ++j) row[j] = 0.f;
    }
}

// Same launch shape as the forward.  Every element of rows 7 (off + i) .. 7 (off + i) + 6 of dsigmas7 and drgbs7 is
// written by the lane that owns sample i: no atomics.
// ORIENT: with the term's gradient in dn:  dn_a += (go w (2 q)) v_a, go = d_orient[id], w recomputed (on all 64 lanes) and
// DETACHED (no gradient reaches sg[0] or deltas through it).
template <int C, bool ORIENT>
__global__ void __launch_bounds__(256)
k_shade_bwd(const float *__restrict__ sigmas7, const float *__restrict__ rgbs7, const int32_t *__restrict__ rays, int64_t N,
            int rays_per_view, const float *__restrict__ shade, int B, float inv_2eps, const float *__restrict__ dsigma_c,
            const float *__restrict__ dcolours, float *__restrict__ dsigmas7, float *__restrict__ drgbs7,
            OrientArgs<ORIENT> oa) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= N) return;
    const int lane = lane_id();
    const auto [id, off, cnt] = load_span(rays, r);
    if (cnt <= 0) return;
    const Light L = load_light(shade, id, rays_per_view, B);
    float v[3], go = 0.f, carry = 0.f, dt = 0.f;
    if constexpr (ORIENT) {
        view_dir(oa.rays_d, id, v);
        go = oa.d_orient[id];
    }
    Sample7<C> cur = load_sample7<C>(sigmas7, rgbs7, off, cnt, lane);
    Grad7<C> gcur = load_grad7<C>(dsigma_c, dcolours, off, cnt, lane);
    if constexpr (ORIENT) dt = load_dt(oa.deltas, off, cnt, lane);
    for (int base = 0; base < cnt; base += 64) {      // (wave-uniform)
        Sample7<C> nxt = cur;
        Grad7<C> gnxt = gcur;
        float dt_nxt = dt;
        if (base + 64 < cnt) {
            nxt = load_sample7<C>(sigmas7, rgbs7, off, cnt, base + 64 + lane);
            gnxt = load_grad7<C>(dsigma_c, dcolours, off, cnt, base + 64 + lane);
            if constexpr (ORIENT) dt_nxt = load_dt(oa.deltas, off, cnt, base + 64 + lane);
        }
        const int i = base + lane;
        const bool valid = i < cnt;
        if (ORIENT || valid) {
            const Lambert o = lambert_of(cur.sg, inv_2eps, L);
            float w = 0.f;
            if constexpr (ORIENT) w = span_weight((oa.density_scale * cur.sg[0]) * dt, valid, oa.T_thresh, carry).w;
            if (valid) {
                float dn[3], dalb[C];
                lambert_grad<C>(cur, gcur, o, L, dn, dalb);
                if constexpr (ORIENT) {
                    const float q = facing_away(o, v);
                    const float e = go * w;
                    const float k = e * (2.0f * q);
#pragma unroll
                    for (int a = 0; a < 3; ++a) dn[a] = dn[a] + k * v[a];
                }
                project_and_store<C>(o, dn, gcur.dsig, dalb, inv_2eps, (off + i) * FD_ROWS, dsigmas7, drgbs7);
            }
        }
        cur = nxt;
        gcur = gnxt;
        dt = dt_nxt;
    }
}

}  // namespace lnerf

using namespace lnerf;

// ---- the four shading entry points: one validate-and-launch path per direction.  `name` is the entry point's, for the
// messages; `oa` is the orient calls' argument block (plain calls: nullptr).
static int check_orient(const char *name, const OrientArgs<true> &oa) {
    LNERF_REQUIRE(oa.deltas && oa.rays_d, "%s: null pointer (deltas / rays_d)", name);
    LNERF_REQUIRE(((uintptr_t)oa.deltas & 7) == 0, "%s: deltas must be 8-byte aligned", name);
    LNERF_REQUIRE(oa.density_scale >= 0.f, "%s: density_scale must be >= 0", name);
    return LNERF_OK;
}

static int shade_forward(const char *name, const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                         int rays_per_view, const float *shade, int B, float inv_2eps, float *sigma_c, float *colours,
                         const OrientArgs<true> *oa, lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "%s: negative N", name);
    LNERF_REQUIRE(C >= 1 && C <= 4, "%s: C must be 1..4 (got %d)", name, C);
    LNERF_REQUIRE(rays_per_view > 0, "%s: rays_per_view must be > 0", name);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(B > 0, "%s: B must be > 0", name);
    LNERF_REQUIRE(sigmas7 && rgbs7 && rays && shade && sigma_c && colours && (!oa || oa->orient), "%s: null pointer", name);
    LNERF_REQUIRE(C != 4 || (((uintptr_t)rgbs7 | (uintptr_t)colours) & 15) == 0,
                  "%s: (C = 4) rgbs7 / colours must be 16-byte aligned", name);
    if (oa && check_orient(name, *oa) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    const dim3 grid((unsigned)div_up(N, 4)), block(256);
    const auto launch = [&](auto kernel, auto orient_args) {
        hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), sigmas7, rgbs7, rays, N, rays_per_view, shade, B,
                           inv_2eps, sigma_c, colours, orient_args);
    };
#define LNERF_SHADE_FWD(CC)                                                                                            \
    if (oa) launch(k_shade_fwd<CC, true>, *oa);                                                                        \
    else launch(k_shade_fwd<CC, false>, OrientArgs<false>{})
    switch (C) {
        case 1: LNERF_SHADE_FWD(1); break;
        case 2: LNERF_SHADE_FWD(2); break;
        case 3: LNERF_SHADE_FWD(3); break;
        default: LNERF_SHADE_FWD(4); break;
    }
#undef LNERF_SHADE_FWD
    LNERF_CHECK_LAUNCH(name);
    return LNERF_OK;
}

static int shade_backward(const char *name, const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                          int rays_per_view, const float *shade, int B, float inv_2eps, const float *dsigma_c,
                          const float *dcolours, float *dsigmas7, float *drgbs7, const OrientArgs<true> *oa,
                          lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "%s: negative N", name);
    LNERF_REQUIRE(C >= 1 && C <= 4, "%s: C must be 1..4 (got %d)", name, C);
    LNERF_REQUIRE(rays_per_view > 0, "%s: rays_per_view must be > 0", name);
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(B > 0, "%s: B must be > 0", name);
    LNERF_REQUIRE(sigmas7 && rgbs7 && rays && shade && dsigma_c && dcolours && dsigmas7 && drgbs7, "%s: null pointer", name);
    LNERF_REQUIRE(C != 4 || (((uintptr_t)rgbs7 | (uintptr_t)dcolours | (uintptr_t)drgbs7) & 15) == 0,
                  "%s: (C = 4) rgbs7 / dcolours / drgbs7 must be 16-byte aligned", name);
    if (oa && check_orient(name, *oa) != LNERF_OK) return LNERF_ERR_INVALID_ARG;
    const dim3 grid((unsigned)div_up(N, 4)), block(256);
    const auto launch = [&](auto kernel, auto orient_args) {
        hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), sigmas7, rgbs7, rays, N, rays_per_view, shade, B,
                           inv_2eps, dsigma_c, dcolours, dsigmas7, drgbs7, orient_args);
    };
#define LNERF_SHADE_BWD(CC)                                                                                            \
    if (oa) launch(k_shade_bwd<CC, true>, *oa);                                                                        \
    else launch(k_shade_bwd<CC, false>, OrientArgs<false>{})
    switch (C) {
        case 1: LNERF_SHADE_BWD(1); break;
        case 2: LNERF_SHADE_BWD(2); break;
        case 3: LNERF_SHADE_BWD(3); break;
        default: LNERF_SHADE_BWD(4); break;
    }
#undef LNERF_SHADE_BWD
    LNERF_CHECK_LAUNCH(name);
    return LNERF_OK;
}

extern "C" {

int lnerf_fd_points(const float *xyzs, float bound, float eps, int64_t m_host, const int32_t *m_dev, float *pts7,
                    int32_t *m7_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(m_host >= 0, "fd_points: m_host must be >= 0");
    LNERF_REQUIRE(eps > 0.f, "fd_points: eps must be > 0");
    LNERF_REQUIRE(bound > 0.f, "fd_points: bound must be > 0");
    LNERF_REQUIRE(m_host <= (int64_t)0x7FFFFFFF / FD_ROWS, "fd_points: 7 * m_host must fit int32");
    if (m_host == 0) return LNERF_OK;
    LNERF_REQUIRE(xyzs && pts7, "fd_points: null pointer");
    int64_t blocks = div_up(m_host, (int64_t)FD_BLOCK);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_fd_points, dim3((unsigned)blocks), dim3(FD_BLOCK), 0, as_stream(stream), xyzs, bound, eps, m_host,
                       m_dev, pts7, m7_dev);
    LNERF_CHECK_LAUNCH("fd_points");
    return LNERF_OK;
}

int lnerf_shade_fd_forward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                           int rays_per_view, const float *shade, int B, float inv_2eps, float *sigma_c, float *colours,
                           lnerf_stream_t stream) {
    return shade_forward("shade_fd_forward", sigmas7, rgbs7, C, rays, N, rays_per_view, shade, B, inv_2eps, sigma_c, colours,
                         nullptr, stream);
}

int lnerf_shade_fd_backward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                            int rays_per_view, const float *shade, int B, float inv_2eps, const float *dsigma_c,
                            const float *dcolours, float *dsigmas7, float *drgbs7, lnerf_stream_t stream) {
    return shade_backward("shade_fd_backward", sigmas7, rgbs7, C, rays, N, rays_per_view, shade, B, inv_2eps, dsigma_c,
                          dcolours, dsigmas7, drgbs7, nullptr, stream);
}

int lnerf_shade_fd_orient_forward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                                  int rays_per_view, const float *shade, int B, float inv_2eps, const float *deltas,
                                  const float *rays_d, float density_scale, float T_thresh, float *sigma_c, float *colours,
                                  float *orient, lnerf_stream_t stream) {
    const OrientArgs<true> oa = {deltas, rays_d, density_scale, T_thresh, orient, nullptr};
    return shade_forward("shade_fd_orient_forward", sigmas7, rgbs7, C, rays, N, rays_per_view, shade, B, inv_2eps, sigma_c,
                         colours, &oa, stream);
}

int lnerf_shade_fd_orient_backward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                                   int rays_per_view, const float *shade, int B, float inv_2eps, const float *dsigma_c,
                                   const float *dcolours, const float *deltas, const float *rays_d, float density_scale,
                                   float T_thresh, const float *d_orient, float *dsigmas7, float *drgbs7,
                                   lnerf_stream_t stream) {
    // no gradient for the term: the plain backward, the same kernel and hence the same bits
    if (!d_orient)
        return lnerf_shade_fd_backward(sigmas7, rgbs7, C, rays, N, rays_per_view, shade, B, inv_2eps, dsigma_c, dcolours,
                                       dsigmas7, drgbs7, stream);
    const OrientArgs<true> oa = {deltas, rays_d, density_scale, T_thresh, nullptr, d_orient};
    return shade_backward("shade_fd_orient_backward", sigmas7, rgbs7, C, rays, N, rays_per_view, shade, B, inv_2eps,
                          dsigma_c, dcolours, dsigmas7, drgbs7, &oa, stream);
}

}  // extern "C"
