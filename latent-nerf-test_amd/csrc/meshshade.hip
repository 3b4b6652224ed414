// Shading of the Latent-Paint renders ("Shaded Latent-Paint renders"): smooth vertex normals of the mesh in world
// space, once per step for all views, and per pixel the interpolated unit normal, nine-term spherical-harmonic lighting and
// depth, with the transposes that carry an image's gradient to the vertices.  The rasteriser is raster.hip's: these kernels
// read its face_idx, bary and face_z.  Contracts: include/lnerf_hip.h.  f32, each operation rounded alone, in the written order.
#include "common.h"
#include "raster_shared.h"
#include "mesh_shared.h"

namespace lnerf {

constexpr float SHADE_MIN_NORM = 1e-6f;   // below it a summed or interpolated normal is 0 and passes no gradient
constexpr float LIGHT_MIN = 1e-8f, LIGHT_MAX = 1.0f;
constexpr int N_LIGHTS = 9;
// the real SH basis up to l = 2
constexpr float SH0 = 0.28209479177387814f, SH1 = 0.4886025119029199f, SH2 = 1.0925484305920792f,
                SH20 = 0.94617469575755997f, SH20C = 0.31539156525251999f, SH22 = 0.5462742152960396f;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3_load(const float *__restrict__ p, int64_t i) { return {p[i * 3], p[i * 3 + 1], p[i * 3 + 2]}; }
__device__ __forceinline__ void v3_store(float *__restrict__ p, int64_t i, V3 a) { p[i * 3] = a.x; p[i * 3 + 1] = a.y; p[i * 3 + 2] = a.z; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ bool is_zero(V3 a) { return a.x == 0.f && a.y == 0.f && a.z == 0.f; }

// ------------------------------------------------------------------------------------------------ vertex normals
// The unit normal of face f with its edges and length; false: the face contributes nothing (an index outside [0, V), a
// zero or non-finite length) and nothing beyond its three indices was read.
struct FaceN { int v[3]; V3 e1, e2, n; float l; };
__device__ __forceinline__ bool face_normal(const float *__restrict__ verts, const int32_t *__restrict__ faces, int V, int f,
                                            FaceN &r) {
    if (!face_ok(faces, V, f, r.v)) return false;
    const V3 p0 = v3_load(verts, r.v[0]);
    r.e1 = v3_load(verts, r.v[1]) - p0;
    r.e2 = v3_load(verts, r.v[2]) - p0;
    const V3 c = cross3(r.e1, r.e2);
    r.l = sqrtf(dot3(c, c));
    if (!(r.l > 0.f) || !(r.l < INFINITY)) return false;
    r.n = c / r.l;
    return true;
}

// the entries of vertex i in the corner table, clamped into corner_list [n3]: a wrong table reads nothing out of range
__device__ __forceinline__ void corner_range(const int32_t *__restrict__ corner_start, int i, int n3, int &b, int &e) {
    b = min(max(corner_start[i], 0), n3);
    e = min(max(corner_start[i + 1], 0), n3);
}
// corner c = 3 f + k of vertex i, or false: an entry that is no corner of i is skipped
__device__ __forceinline__ bool corner_of(const int32_t *__restrict__ corner_list, const int32_t *__restrict__ faces, int s,
                                          int i, int n3, int &f, int &k) {
    const int c = corner_list[s];
    if (c < 0 || c >= n3 || faces[c] != i) return false;
    f = c / 3;
    k = c - f * 3;
    return true;
}

// s_i = the sum of the unit normals of i's faces in table order
__device__ __forceinline__ V3 vertex_sum(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                         const int32_t *__restrict__ corner_start, const int32_t *__restrict__ corner_list,
                                         int i, int V, int F) {
    int b, e, f, k;
    corner_range(corner_start, i, F * 3, b, e);
    V3 s = {0.f, 0.f, 0.f};
    for (int t = b; t < e; ++t) {
        FaceN fn;
        if (corner_of(corner_list, faces, t, i, F * 3, f, k) && face_normal(verts, faces, V, f, fn)) s = s + fn.n;
    }
    return s;
}

// one lane per vertex: vn_i = s_i / |s_i|, 0 below SHADE_MIN_NORM
__global__ void __launch_bounds__(MESH_THREADS)
k_vertex_normals_fwd(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F,
                     const int32_t *__restrict__ corner_start, const int32_t *__restrict__ corner_list,
                     float *__restrict__ vnormals) {
    const int i = mesh_gid();
    if (i >= V) return;
    const V3 s = vertex_sum(verts, faces, corner_start, corner_list, i, V, F);
    const float m = sqrtf(dot3(s, s));
    v3_store(vnormals, i, m >= SHADE_MIN_NORM ? s / m : V3{0.f, 0.f, 0.f});
}

// backward, pass 1, one lane per vertex: gs_i = dL/ds_i = (g_i - vn_i (vn_i . g_i)) / m, 0 where vn_i was zeroed
__global__ void __launch_bounds__(MESH_THREADS)
k_vertex_normals_bwd_sum(const float *__restrict__ gvn, const float *__restrict__ verts, int V,
                         const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ corner_start,
                         const int32_t *__restrict__ corner_list, float *__restrict__ gs) {
    const int i = mesh_gid();
    if (i >= V) return;
    const V3 s = vertex_sum(verts, faces, corner_start, corner_list, i, V, F);
    const float m = sqrtf(dot3(s, s));
    V3 r = {0.f, 0.f, 0.f};
    if (m >= SHADE_MIN_NORM) {
        const V3 vn = s / m, g = v3_load(gvn, i);
        r = (g - vn * dot3(vn, g)) / m;
    }
    v3_store(gs, i, r);
}

// backward, pass 2, one lane per vertex j: over j's corners (f, k) in table order, the share of corner k in the transpose
// of n_f = c / |c|, c = e1 x e2, under dL/dn_f = (gs_v0 + gs_v1) + gs_v2.  Each face is recomputed by its three corners.
__global__ void __launch_bounds__(MESH_THREADS)
k_vertex_normals_bwd_gather(const float *__restrict__ gs, const float *__restrict__ verts, int V,
                            const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ corner_start,
                            const int32_t *__restrict__ corner_list, float *__restrict__ gverts) {
    const int j = mesh_gid();
    if (j >= V) return;
    int b, e, f, k;
    corner_range(corner_start, j, F * 3, b, e);
    V3 acc = {0.f, 0.f, 0.f};
    for (int t = b; t < e; ++t) {
        FaceN fn;
        if (!corner_of(corner_list, faces, t, j, F * 3, f, k) || !face_normal(verts, faces, V, f, fn)) continue;
        const V3 gn = (v3_load(gs, fn.v[0]) + v3_load(gs, fn.v[1])) + v3_load(gs, fn.v[2]);
        const V3 gc = (gn - fn.n * dot3(fn.n, gn)) / fn.l;
        const V3 ge1 = cross3(fn.e2, gc), ge2 = cross3(gc, fn.e1);   // dL/d(v1 - v0), dL/d(v2 - v0)
        if (k == 0) acc = (acc - ge1) - ge2;
        else acc = acc + (k == 1 ? ge1 : ge2);
    }
    v3_store(gverts, j, acc);
}

static size_t vertex_normals_scratch_bytes(int V, int F) {
    if (V < 1 || V > 0x7fffffff / 3 || F < 1 || F > LNERF_MESH_MAX_FACES) return 0;
    return ((size_t)V * 3 * sizeof(float) + 15) & ~(size_t)15;
}

// ------------------------------------------------------------------------------------------------ pixel shading
// What a foreground pixel reads and derives; ok = false: background (face_idx outside [0, F), or a vertex id outside [0, V)).
struct ShadePixel {
    bool ok;
    int v[3];
    int64_t bf;        // b * F + f
    float b[3], z[3];
    V3 vn[3], n;       // the corners' normals and the unit normal (0 where m < SHADE_MIN_NORM)
    float m;
};
__device__ __forceinline__ ShadePixel shade_pixel(int64_t p, const int32_t *__restrict__ face_idx, const float *__restrict__ bary,
                                                  const float *__restrict__ face_z, const int32_t *__restrict__ faces,
                                                  const float *__restrict__ vnormals, int view, int F, int V) {
    ShadePixel r;
    const int f = face_idx[p];
    r.ok = f >= 0 && f < F && face_ok(faces, V, f, r.v);
    if (!r.ok) return r;
    r.bf = (int64_t)view * F + f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.b[k] = bary[p * 3 + k];
        r.z[k] = face_z[r.bf * 3 + k];
        r.vn[k] = v3_load(vnormals, r.v[k]);
    }
    const V3 a = (r.vn[0] * r.b[0] + r.vn[1] * r.b[1]) + r.vn[2] * r.b[2];
    r.m = sqrtf(dot3(a, a));
    r.n = r.m >= SHADE_MIN_NORM ? a / r.m : V3{0.f, 0.f, 0.f};
    return r;
}

// the unclamped lighting sum_k L_k Y_k(n), k ascending
__device__ __forceinline__ float sh_light(const float *__restrict__ L, V3 n) {
    float acc = L[0] * SH0;
    acc = acc + L[1] * -(SH1 * n.y);
    acc = acc + L[2] * (SH1 * n.z);
    acc = acc + L[3] * -(SH1 * n.x);
    acc = acc + L[4] * ((SH2 * n.x) * n.y);
    acc = acc + L[5] * -((SH2 * n.y) * n.z);
    acc = acc + L[6] * ((SH20 * n.z) * n.z - SH20C);
    acc = acc + L[7] * -((SH2 * n.x) * n.z);
    acc = acc + L[8] * (SH22 * (n.x * n.x - n.y * n.y));
    return acc;
}
// its derivative by n, the terms of each component in ascending k
__device__ __forceinline__ V3 sh_light_grad(const float *__restrict__ L, V3 n) {
    V3 g;
    g.x = ((-(L[3] * SH1) + L[4] * (SH2 * n.y)) - L[7] * (SH2 * n.z)) + L[8] * ((2.0f * SH22) * n.x);
    g.y = ((-(L[1] * SH1) + L[4] * (SH2 * n.x)) - L[5] * (SH2 * n.z)) - L[8] * ((2.0f * SH22) * n.y);
    g.z = ((L[2] * SH1 - L[5] * (SH2 * n.y)) + L[6] * ((2.0f * SH20) * n.z)) - L[7] * (SH2 * n.x);
    return g;
}

// one thread per pixel; every output element is written (0 on background), a NULL output is skipped
__global__ void __launch_bounds__(256)
k_raster_shade_fwd(const int32_t *__restrict__ face_idx, const float *__restrict__ bary, const float *__restrict__ face_z,
                   const int32_t *__restrict__ faces, const float *__restrict__ vnormals, const float *__restrict__ lights,
                   int64_t P, int64_t HW, int F, int V, float *__restrict__ normal, float *__restrict__ lighting,
                   float *__restrict__ depth) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int view = (int)(p / HW);
    const ShadePixel s = shade_pixel(p, face_idx, bary, face_z, faces, vnormals, view, F, V);
    V3 n = {0.f, 0.f, 0.f};
    float li = 0.f, d = 0.f;
    if (s.ok) {
        n = s.n;
        d = -((s.b[0] * s.z[0] + s.b[1] * s.z[1]) + s.b[2] * s.z[2]);
        if (lighting) li = fminf(fmaxf(sh_light(lights + view * N_LIGHTS, n), LIGHT_MIN), LIGHT_MAX);
    }
    if (normal) v3_store(normal, p, n);
    if (lighting) lighting[p] = li;
    if (depth) depth[p] = d;
}

// one thread per pixel: grad_bary in gather form; the atomics into grad_vnormals and grad_face_z
__global__ void __launch_bounds__(256)
k_raster_shade_bwd(const float *__restrict__ gnormal, const float *__restrict__ glighting, const float *__restrict__ gdepth,
                   const int32_t *__restrict__ face_idx, const float *__restrict__ bary, const float *__restrict__ face_z,
                   const int32_t *__restrict__ faces, const float *__restrict__ vnormals, const float *__restrict__ lights,
                   int64_t P, int64_t HW, int F, int V, float *__restrict__ gbary, float *__restrict__ gvn,
                   float *__restrict__ gz) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int view = (int)(p / HW);
    const ShadePixel s = shade_pixel(p, face_idx, bary, face_z, faces, vnormals, view, F, V);
    float gb[3] = {0.f, 0.f, 0.f};
    if (s.ok) {
        // dL/dn: the normal image's gradient plus the lighting's where its clamp is not active
        V3 gn = gnormal ? v3_load(gnormal, p) : V3{0.f, 0.f, 0.f};
        if (glighting) {
            const float *L = lights + view * N_LIGHTS;
            const float acc = sh_light(L, s.n);
            if (acc >= LIGHT_MIN && acc <= LIGHT_MAX) gn = gn + sh_light_grad(L, s.n) * glighting[p];
        }
        // n = a / m
        V3 ga = {0.f, 0.f, 0.f};
        if (s.m >= SHADE_MIN_NORM) ga = (gn - s.n * dot3(s.n, gn)) / s.m;
        const float gd = gdepth ? gdepth[p] : 0.f;
        const bool live = !is_zero(ga);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gb[k] = dot3(ga, s.vn[k]) - gd * s.z[k];
            if (live) {
                float *g = gvn + (int64_t)s.v[k] * 3;
                atomicAdd(&g[0], ga.x * s.b[k]);
                atomicAdd(&g[1], ga.y * s.b[k]);
                atomicAdd(&g[2], ga.z * s.b[k]);
            }
            if (gd != 0.f) atomicAdd(&gz[s.bf * 3 + k], -(gd * s.b[k]));
        }
    }
    gbary[p * 3] = gb[0]; gbary[p * 3 + 1] = gb[1]; gbary[p * 3 + 2] = gb[2];
}

static int check_shade_mesh(const char *who, int V) {
    LNERF_REQUIRE(V >= 1 && V <= 0x7fffffff / 3, "%s: n_verts must be in [1, %d] (got %d)", who, 0x7fffffff / 3, V);
    return LNERF_OK;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_vertex_normals_forward(const float *verts, int n_verts, const int32_t *faces, int n_faces,
                                 const int32_t *corner_start, const int32_t *corner_list, float *vnormals,
                                 lnerf_stream_t stream) {
    LNERF_REQUIRE(vertex_normals_scratch_bytes(n_verts, n_faces) > 0,
                  "vertex_normals_forward: n_verts (%d) or n_faces (%d) out of range", n_verts, n_faces);
    LNERF_REQUIRE(verts && faces && corner_start && corner_list && vnormals, "vertex_normals_forward: null pointer");
    hipStream_t s = as_stream(stream);
    MESH_LAUNCH(k_vertex_normals_fwd, n_verts, verts, n_verts, faces, n_faces, corner_start, corner_list, vnormals);
    LNERF_CHECK_LAUNCH("vertex_normals_forward");
    return LNERF_OK;
}

size_t lnerf_vertex_normals_scratch_bytes(int n_verts, int n_faces) { return vertex_normals_scratch_bytes(n_verts, n_faces); }

int lnerf_vertex_normals_backward(const float *grad_vnormals, const float *verts, int n_verts, const int32_t *faces,
                                  int n_faces, const int32_t *corner_start, const int32_t *corner_list, void *scratch,
                                  size_t scratch_bytes, float *grad_verts, lnerf_stream_t stream) {
    const size_t need = vertex_normals_scratch_bytes(n_verts, n_faces);
    LNERF_REQUIRE(need > 0, "vertex_normals_backward: n_verts (%d) or n_faces (%d) out of range", n_verts, n_faces);
    LNERF_REQUIRE(grad_vnormals && verts && faces && corner_start && corner_list && grad_verts,
                  "vertex_normals_backward: null pointer");
    LNERF_REQUIRE(scratch && scratch_bytes >= need && ((uintptr_t)scratch & 15) == 0,
                  "vertex_normals_backward: scratch must be 16-byte aligned and hold %zu bytes", need);
    hipStream_t s = as_stream(stream);
    float *gs = static_cast<float *>(scratch);
    MESH_LAUNCH(k_vertex_normals_bwd_sum, n_verts, grad_vnormals, verts, n_verts, faces, n_faces, corner_start, corner_list, gs);
    MESH_LAUNCH(k_vertex_normals_bwd_gather, n_verts, gs, verts, n_verts, faces, n_faces, corner_start, corner_list, grad_verts);
    LNERF_CHECK_LAUNCH("vertex_normals_backward");
    return LNERF_OK;
}

int lnerf_raster_shade_forward(const int32_t *face_idx, const float *bary, const float *face_z, const int32_t *faces,
                               const float *vnormals, const float *lights, int B, int H, int W, int n_faces, int n_verts,
                               float *normal, float *lighting, float *depth, lnerf_stream_t stream) {
    if (int e = check_raster_dims("raster_shade_forward", B, H, W, n_faces)) return e;
    if (int e = check_shade_mesh("raster_shade_forward", n_verts)) return e;
    LNERF_REQUIRE(face_idx && bary && face_z && faces && vnormals && lights, "raster_shade_forward: null pointer");
    LNERF_REQUIRE(normal || lighting || depth, "raster_shade_forward: every output is null");
    const int64_t P = (int64_t)B * H * W;
    LNERF_LAUNCH(k_raster_shade_fwd, P, 256, as_stream(stream), face_idx, bary, face_z, faces, vnormals, lights, P,
                 (int64_t)H * W, n_faces, n_verts, normal, lighting, depth);
    LNERF_CHECK_LAUNCH("raster_shade_forward");
    return LNERF_OK;
}

int lnerf_raster_shade_backward(const float *grad_normal, const float *grad_lighting, const float *grad_depth,
                                const int32_t *face_idx, const float *bary, const float *face_z, const int32_t *faces,
                                const float *vnormals, const float *lights, int B, int H, int W, int n_faces, int n_verts,
                                float *grad_bary, float *grad_vnormals, float *grad_face_z, lnerf_stream_t stream) {
    if (int e = check_raster_dims("raster_shade_backward", B, H, W, n_faces)) return e;
    if (int e = check_shade_mesh("raster_shade_backward", n_verts)) return e;
    LNERF_REQUIRE(face_idx && bary && face_z && faces && vnormals && lights && grad_bary && grad_vnormals && grad_face_z,
                  "raster_shade_backward: null pointer");
    LNERF_REQUIRE(grad_normal || grad_lighting || grad_depth, "raster_shade_backward: every incoming gradient is null");
    const int64_t P = (int64_t)B * H * W;
    LNERF_LAUNCH(k_raster_shade_bwd, P, 256, as_stream(stream), grad_normal, grad_lighting, grad_depth, face_idx, bary,
                 face_z, faces, vnormals, lights, P, (int64_t)H * W, n_faces, n_verts, grad_bary, grad_vnormals, grad_face_z);
    LNERF_CHECK_LAUNCH("raster_shade_backward");
    return LNERF_OK;
}

}  // extern "C"
