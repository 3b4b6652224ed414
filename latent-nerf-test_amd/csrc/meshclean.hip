// Mesh cleaning between marching cubes and the decimation: connected components, a stable face / vertex filter and
// Taubin smoothing.  Contract: include/lnerf_hip.h, "mesh cleaning"; numpy restatement: tests/meshclean_reference.py.
// Every loop in a kernel has a bound known at launch (the lists' lengths are fixed before the kernels that walk them
// start); nothing here waits on another workgroup.  Integer atomics only (min / max / add commute, so the results do
// not depend on their order); f32 / f64 arithmetic is + - * / sqrt in the order written.
//
//   lnerf_mesh_components_begin   k_mcc_begin    label[v] = v; the faces with an index out of range are counted
//   lnerf_mesh_components_round   k_mcc_hook     one lane per face: the smallest label of its corners -> atomicMin onto
//                                                every larger corner label and that label's label
//                                 k_mcc_jump     one lane per vertex: MC_JUMP_HOPS steps of label = label[label]
//   lnerf_mesh_components_finish  k_mcc_mark     referenced[v] = 1 for the corners of the valid faces
//                                 k_mcc_roots    referenced roots ranked inside each block (scan.h), block totals of the
//                                                roots and of the referenced vertices
//                                 k_scan_top     (scan.h) prefix of both -> counts = {components, referenced vertices}
//                                 k_mcc_assign   vert_comp = rank of the vertex's root
//                                 k_mcc_faces    face_comp, comp_faces (atomicAdd; one per wave where a wave agrees)
//                                 k_mcc_box      atomicMin / atomicMax of the order-preserving encoding of the vertex
//                                                coordinates into the component's box (one per wave where a wave agrees)
//                                 k_mcc_unbox    one lane per component: back to f32
//   lnerf_mesh_filter             k_mf_mark      used[v] = 1 for the corners of the kept faces
//                                 k_mf_rank      kept faces and used vertices ranked inside each block, block totals
//                                 k_scan_top     prefix of both -> counts = {vertices out, faces out}
//                                 k_mf_emit      vert_src, re-indexed faces
//   lnerf_mesh_smooth             k_ms_check     faces with an index out of range are counted -- host read --
//                                 k_ms_count, k_ms_rank, k_scan_top, k_ms_fill, k_ms_sort   vertex -> (face, corner)
//                                                incidence lists, each ascending in 3 f + k
//                                 k_ms_step      one lane per vertex: p' = p + w (mean of the incident faces' other
//                                                corners - p) in f64, from the positions before the step
//                                 k_ms_normals   one lane per vertex: f32 sum of its faces' cross products, normalised
#include <algorithm>

#include "common.h"
#include "mesh_shared.h"
#include "scan.h"

namespace lnerf {

constexpr int MC_THREADS = 256;
constexpr int MC_LOG2 = 8;
constexpr int MC_JUMP_HOPS = LNERF_MESH_JUMP_HOPS;

__device__ __forceinline__ int mc_gid() { return blockIdx.x * MC_THREADS + threadIdx.x; }

// the three indices of face f; false if one lies outside [0, n_verts) (nothing may be read through them then)
__device__ __forceinline__ bool mc_face_ok(const int32_t *__restrict__ faces, int n_verts, int f, int v[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = faces[(int64_t)f * 3 + k];
        ok = ok && v[k] >= 0 && v[k] < n_verts;
    }
    return ok;
}

// the value of `x` in the first lane of `mask` (mask != 0)
__device__ __forceinline__ int mc_first(unsigned long long mask, int x) {
    return __shfl(x, __ffsll((long long)mask) - 1, LNERF_WAVE);
}

// ---------------------------------------------------------------- connected components
__global__ void __launch_bounds__(MC_THREADS)
k_mcc_begin(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *__restrict__ label,
            unsigned long long *__restrict__ n_bad) {
    const int i = mc_gid();
    if (i < n_verts) label[i] = i;
    bool bad = false;
    if (i < n_faces) {
        int v[3];
        bad = !mc_face_ok(faces, n_verts, i, v);
    }
    const unsigned long long mask = __ballot(bad);
    if (lane_id() == 0 && mask != 0) atomicAdd(n_bad, (unsigned long long)__popcll(mask));
}

// Labels only ever decrease and always name a vertex of the same component, so a plain read that misses another
// workgroup's atomicMin of the same launch sees an older valid label: it costs at most a round, never the result.  A
// launch in which no lane raises `changed` wrote nothing, so all it read was the settled state (see k_atlas_hook).
__global__ void __launch_bounds__(MC_THREADS)
k_mcc_hook(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *label, int32_t *__restrict__ changed) {
    const int f = mc_gid();
    if (f >= n_faces) return;
    int v[3], l[3];
    if (!mc_face_ok(faces, n_verts, f, v)) return;
    int m = n_verts;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        l[k] = label[v[k]];
        if (l[k] < 0 || l[k] >= n_verts) return;
        m = min(m, l[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (m < l[k]) {
            atomicMin(&label[l[k]], m);
            atomicMin(&label[v[k]], m);
            *changed = 1;
        }
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcc_jump(int n_verts, int32_t *label) {
    const int v = mc_gid();
    if (v >= n_verts) return;
    const int l0 = label[v];
    int l = l0;
#pragma unroll
    for (int h = 0; h < MC_JUMP_HOPS; ++h) {
        if (l < 0 || l >= n_verts) return;
        const int ll = label[l];
        if (ll < l) l = ll;
    }
    if (l >= 0 && l < l0) atomicMin(&label[v], l);
}

// (several faces may mark one vertex: every writer stores the same 1)
__global__ void __launch_bounds__(MC_THREADS)
k_mcc_mark(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *__restrict__ referenced) {
    const int f = mc_gid();
    if (f >= n_faces) return;
    int v[3];
    if (!mc_face_ok(faces, n_verts, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) referenced[v[k]] = 1;
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcc_roots(const int32_t *__restrict__ referenced, const int32_t *__restrict__ label, int n_verts,
            int32_t *__restrict__ root_rank, int64_t *__restrict__ blk_roots, int64_t *__restrict__ blk_ref) {
    const int v = mc_gid();
    const int r = (v < n_verts && referenced[v]) ? 1 : 0;
    const int n[2] = {(r && label[v] == v) ? 1 : 0, r};
    int excl[2], total[2];
    block_exclusive_scan<MC_THREADS>(n, excl, total);
    if (v < n_verts) root_rank[v] = excl[0];
    if (threadIdx.x == 0) {
        blk_roots[blockIdx.x] = total[0];
        blk_ref[blockIdx.x] = total[1];
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcc_assign(const int32_t *__restrict__ referenced, const int32_t *__restrict__ label, int n_verts,
             const int32_t *__restrict__ root_rank, const int64_t *__restrict__ blk_roots,
             int32_t *__restrict__ vert_comp) {
    const int v = mc_gid();
    if (v >= n_verts) return;
    const int l = label[v];
    int c = -1;
    if (referenced[v] && l >= 0 && l < n_verts) c = (int)blk_roots[l >> MC_LOG2] + root_rank[l];
    vert_comp[v] = c;
}

// One lane per face.  Where every counted face of a wave lies in one component (the usual case: faces of a component are
// neighbours in the list) the wave adds its count once.
__global__ void __launch_bounds__(MC_THREADS)
k_mcc_faces(const int32_t *__restrict__ faces, int n_verts, int n_faces, const int32_t *__restrict__ vert_comp, int cap,
            int32_t *__restrict__ face_comp, int32_t *comp_faces) {
    const int f = mc_gid();
    int c = -1;
    if (f < n_faces) {
        int v[3];
        if (mc_face_ok(faces, n_verts, f, v)) c = vert_comp[v[0]];
        if (c >= cap) c = -1;
        face_comp[f] = c;
    }
    const unsigned long long mask = __ballot(c >= 0);
    if (mask == 0) return;
    const int c0 = mc_first(mask, c);
    if (__ballot(c >= 0 && c != c0) == 0) {
        if (lane_id() == 0) atomicAdd(&comp_faces[c0], (int)__popcll(mask));
    } else if (c >= 0) {
        atomicAdd(&comp_faces[c], 1);
    }
}

// enc: [6][cap] u32 = x_lo, y_lo, z_lo (cleared to ~0), x_hi, y_hi, z_hi (cleared to 0)
__global__ void __launch_bounds__(MC_THREADS)
k_mcc_box(const float *__restrict__ verts, int n_verts, const int32_t *__restrict__ vert_comp, int cap, uint32_t *enc) {
    const int v = mc_gid();
    int c = -1;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (v < n_verts) {
        c = vert_comp[v];
        if (c >= cap) c = -1;
        if (c >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = hi[a] = ordered_encode(verts[(int64_t)v * 3 + a]);
        }
    }
    const unsigned long long mask = __ballot(c >= 0);
    if (mask == 0) return;
    const int c0 = mc_first(mask, c);
    if (__ballot(c >= 0 && c != c0) == 0) {     // one component in the wave: reduce (idle lanes hold the neutral values)
#pragma unroll
        for (int o = 1; o < LNERF_WAVE; o <<= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o, LNERF_WAVE));
                hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o, LNERF_WAVE));
            }
        if (lane_id() != 0) return;
        c = c0;
    } else if (c < 0) {
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(&enc[(int64_t)a * cap + c], lo[a]);
        atomicMax(&enc[(int64_t)(3 + a) * cap + c], hi[a]);
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcc_unbox(const uint32_t *__restrict__ enc, int cap, const int64_t *__restrict__ counts, float *__restrict__ comp_box) {
    const int c = mc_gid();
    if (c >= cap || c >= counts[0]) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) comp_box[(int64_t)c * 6 + k] = ordered_decode(enc[(int64_t)k * cap + c]);
}

// ---------------------------------------------------------------- filter
__device__ __forceinline__ bool mf_kept(const int32_t *__restrict__ faces, int n_verts, const uint8_t *__restrict__ keep,
                                        int f, int v[3]) {
    return keep[f] != 0 && mc_face_ok(faces, n_verts, f, v);
}

__global__ void __launch_bounds__(MC_THREADS)
k_mf_mark(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          int32_t *__restrict__ used) {
    const int f = mc_gid();
    if (f >= n_faces) return;
    int v[3];
    if (!mf_kept(faces, n_verts, keep, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) used[v[k]] = 1;
}

// lane i ranks vertex i and face i
__global__ void __launch_bounds__(MC_THREADS)
k_mf_rank(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          const int32_t *__restrict__ used, int32_t *__restrict__ vert_at, int32_t *__restrict__ face_at,
          int64_t *__restrict__ blk_v, int64_t *__restrict__ blk_f) {
    const int i = mc_gid();
    int v[3];
    const int n[2] = {(i < n_verts && used[i]) ? 1 : 0, (i < n_faces && mf_kept(faces, n_verts, keep, i, v)) ? 1 : 0};
    int excl[2], total[2];
    block_exclusive_scan<MC_THREADS>(n, excl, total);
    if (i < n_verts) vert_at[i] = excl[0];
    if (i < n_faces) face_at[i] = excl[1];
    if (threadIdx.x == 0) {
        blk_v[blockIdx.x] = total[0];
        blk_f[blockIdx.x] = total[1];
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_mf_emit(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          const int32_t *__restrict__ used, const int32_t *__restrict__ vert_at, const int32_t *__restrict__ face_at,
          const int64_t *__restrict__ blk_v, const int64_t *__restrict__ blk_f, int32_t *__restrict__ faces_out,
          int32_t *__restrict__ vert_src) {
    const int i = mc_gid();
    if (i < n_verts && used[i]) vert_src[blk_v[blockIdx.x] + vert_at[i]] = i;
    int v[3];
    if (i < n_faces && mf_kept(faces, n_verts, keep, i, v)) {
        const int64_t o = (blk_f[blockIdx.x] + face_at[i]) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) faces_out[o + k] = (int32_t)(blk_v[v[k] >> MC_LOG2] + vert_at[v[k]]);
    }
}

// ---------------------------------------------------------------- smoothing
__device__ __forceinline__ bool ms_degenerate(const int v[3]) { return v[0] == v[1] || v[1] == v[2] || v[2] == v[0]; }

__global__ void __launch_bounds__(MC_THREADS)
k_ms_check(const int32_t *__restrict__ faces, int n_verts, int n_faces, unsigned long long *__restrict__ n_bad) {
    const int f = mc_gid();
    bool bad = false;
    if (f < n_faces) {
        int v[3];
        bad = !mc_face_ok(faces, n_verts, f, v);
    }
    const unsigned long long mask = __ballot(bad);
    if (lane_id() == 0 && mask != 0) atomicAdd(n_bad, (unsigned long long)__popcll(mask));
}

// (the faces passed k_ms_check: every index is in range)
__global__ void __launch_bounds__(MC_THREADS)
k_ms_count(const int32_t *__restrict__ faces, int n_faces, int32_t *cnt) {
    const int f = mc_gid();
    if (f >= n_faces) return;
    const int v[3] = {faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]};
    if (ms_degenerate(v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&cnt[v[k]], 1);
}

__global__ void __launch_bounds__(MC_THREADS)
k_ms_rank(const int32_t *__restrict__ cnt, int n_verts, int32_t *__restrict__ loc, int64_t *__restrict__ blk) {
    const int v = mc_gid();
    const int n[1] = {v < n_verts ? cnt[v] : 0};
    int excl[1], total[1];
    block_exclusive_scan<MC_THREADS>(n, excl, total);
    if (v < n_verts) loc[v] = excl[0];
    if (threadIdx.x == 0) blk[blockIdx.x] = total[0];
}

__global__ void __launch_bounds__(MC_THREADS)
k_ms_fill(const int32_t *__restrict__ faces, int n_faces, const int32_t *__restrict__ loc, const int64_t *__restrict__ blk,
          int32_t *cur, int32_t *__restrict__ list) {
    const int f = mc_gid();
    if (f >= n_faces) return;
    const int v[3] = {faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]};
    if (ms_degenerate(v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        list[blk[v[k] >> MC_LOG2] + loc[v[k]] + atomicAdd(&cur[v[k]], 1)] = 3 * f + k;
}

__global__ void __launch_bounds__(MC_THREADS)
k_ms_sort(const int32_t *__restrict__ cnt, const int32_t *__restrict__ loc, const int64_t *__restrict__ blk, int n_verts,
          int32_t *__restrict__ list) {
    const int v = mc_gid();
    if (v >= n_verts) return;
    int32_t *l = list + (blk[blockIdx.x] + loc[v]);
    const int n = cnt[v];
    for (int i = 1; i < n; ++i) {          // insertion sort: the lists are short
        const int x = l[i];
        int j = i - 1;
        while (j >= 0 && l[j] > x) {
            l[j + 1] = l[j];
            --j;
        }
        l[j + 1] = x;
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_ms_step(const float *__restrict__ src, const int32_t *__restrict__ faces, const int32_t *__restrict__ cnt,
          const int32_t *__restrict__ loc, const int64_t *__restrict__ blk, const int32_t *__restrict__ list, int n_verts,
          float w, float *__restrict__ dst) {
    const int v = mc_gid();
    if (v >= n_verts) return;
    const float p[3] = {src[(int64_t)v * 3], src[(int64_t)v * 3 + 1], src[(int64_t)v * 3 + 2]};
    const int n = cnt[v];
    if (n == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) dst[(int64_t)v * 3 + a] = p[a];
        return;
    }
    const int32_t *l = list + (blk[blockIdx.x] + loc[v]);
    double S[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < n; ++s) {
        const int e = l[s];
        const int f = e / 3, k = e - 3 * f;
        const int64_t a = faces[(int64_t)f * 3 + (k == 2 ? 0 : k + 1)], b = faces[(int64_t)f * 3 + (k == 0 ? 2 : k - 1)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            S[c] = S[c] + (double)src[a * 3 + c];
            S[c] = S[c] + (double)src[b * 3 + c];
        }
    }
    const double den = (double)(2 * (int64_t)n);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double mean = S[c] / den;
        dst[(int64_t)v * 3 + c] = (float)((double)p[c] + (double)w * (mean - (double)p[c]));
    }
}

// lnerf_decimate's normals (k_dc_normals) over the incidence lists: a face that does not repeat an index holds the vertex
// once, so ascending 3 f + k is ascending f
__global__ void __launch_bounds__(MC_THREADS)
k_ms_normals(const float *__restrict__ verts, const int32_t *__restrict__ faces, const int32_t *__restrict__ cnt,
             const int32_t *__restrict__ loc, const int64_t *__restrict__ blk, const int32_t *__restrict__ list,
             int n_verts, float *__restrict__ normals) {
    const int v = mc_gid();
    if (v >= n_verts) return;
    const int32_t *l = list + (blk[blockIdx.x] + loc[v]);
    const int n = cnt[v];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int s = 0; s < n; ++s) {
        const int64_t f = l[s] / 3;
        const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        const float e1x = verts[b * 3] - verts[a * 3], e1y = verts[b * 3 + 1] - verts[a * 3 + 1],
                    e1z = verts[b * 3 + 2] - verts[a * 3 + 2];
        const float e2x = verts[c * 3] - verts[a * 3], e2y = verts[c * 3 + 1] - verts[a * 3 + 1],
                    e2z = verts[c * 3 + 2] - verts[a * 3 + 2];
        s0 = s0 + (e1y * e2z - e1z * e2y);
        s1 = s1 + (e1z * e2x - e1x * e2z);
        s2 = s2 + (e1x * e2y - e1y * e2x);
    }
    const float l2 = s0 * s0 + s1 * s1 + s2 * s2;
    const float inv = l2 > 0.f ? 1.0f / sqrtf(l2) : 0.f;
    normals[(int64_t)v * 3] = s0 * inv;
    normals[(int64_t)v * 3 + 1] = s1 * inv;
    normals[(int64_t)v * 3 + 2] = s2 * inv;
}

// ---------------------------------------------------------------- host side
static bool mc_sizes_ok(int n_verts, int n_faces) {
    return n_verts >= 0 && n_faces >= 0 && n_faces <= LNERF_MESH_MAX_FACES && n_verts <= 3 * LNERF_MESH_MAX_FACES;
}

static unsigned mc_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, div_up(n, MC_THREADS)); }

static bool mc_hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_error("%s failed: %s", what, hipGetErrorString(e));
    return false;
}

struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    }
};

struct CompLayout {
    int cap;
    int64_t nb;
    size_t referenced, root_rank, blk_roots, blk_ref, enc, bytes;
};

static CompLayout comp_layout(int V, int F) {
    CompLayout L;
    Carve c;
    L.cap = std::min(V, F);          // every component holds a face and a vertex of its own
    L.nb = div_up(V, MC_THREADS);
    L.referenced = c.take((size_t)V * 4);
    L.root_rank = c.take((size_t)V * 4);
    L.blk_roots = c.take((size_t)L.nb * 8);
    L.blk_ref = c.take((size_t)L.nb * 8);
    L.enc = c.take((size_t)L.cap * 24);
    L.bytes = std::max<size_t>(c.o, 256);
    return L;
}

struct FilterLayout {
    int64_t nb;
    size_t used, vert_at, face_at, blk_v, blk_f, bytes;
};

static FilterLayout filter_layout(int V, int F) {
    FilterLayout L;
    Carve c;
    L.nb = div_up(std::max(V, F), MC_THREADS);
    L.used = c.take((size_t)V * 4);
    L.vert_at = c.take((size_t)V * 4);
    L.face_at = c.take((size_t)F * 4);
    L.blk_v = c.take((size_t)L.nb * 8);
    L.blk_f = c.take((size_t)L.nb * 8);
    L.bytes = std::max<size_t>(c.o, 256);
    return L;
}

struct SmoothLayout {
    int64_t nb;
    size_t dev, cnt, cur, loc, blk, list, tmp, bytes;
};

static SmoothLayout smooth_layout(int V, int F) {
    SmoothLayout L;
    Carve c;
    L.nb = div_up(V, MC_THREADS);
    L.dev = c.take(64);
    L.cnt = c.take((size_t)V * 4);
    L.cur = c.take((size_t)V * 4);
    L.loc = c.take((size_t)V * 4);
    L.blk = c.take(((size_t)L.nb + 1) * 8);
    L.list = c.take((size_t)F * 12);
    L.tmp = c.take((size_t)V * 12);
    L.bytes = c.o;
    return L;
}

}  // namespace lnerf

using namespace lnerf;

#define MC_LAUNCH(kernel, n, ...) hipLaunchKernelGGL(kernel, dim3(mc_grid(n)), dim3(MC_THREADS), 0, s, __VA_ARGS__)
#define MC_AT(T, off) reinterpret_cast<T *>(reinterpret_cast<char *>(scratch) + (off))

extern "C" {

int lnerf_mesh_components_begin(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int64_t *counts_dev,
                                lnerf_stream_t stream) {
    LNERF_REQUIRE(mc_sizes_ok(n_verts, n_faces), "mesh_components_begin: %d vertices / %d faces out of range (faces <= %d)",
                  n_verts, n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(counts_dev && (n_verts == 0 || label) && (n_faces == 0 || faces), "mesh_components_begin: null pointer");
    hipStream_t s = as_stream(stream);
    if (!mc_hip_ok(hipMemsetAsync(counts_dev, 0, 8, s), "mesh_components_begin: clearing the count")) return LNERF_ERR_HIP;
    if (std::max(n_verts, n_faces) > 0) {
        MC_LAUNCH(k_mcc_begin, std::max(n_verts, n_faces), faces, n_verts, n_faces, label,
                  reinterpret_cast<unsigned long long *>(counts_dev));
        LNERF_CHECK_LAUNCH("mesh_components_begin");
    }
    return LNERF_OK;
}

int lnerf_mesh_components_round(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int32_t *changed_dev,
                                lnerf_stream_t stream) {
    LNERF_REQUIRE(mc_sizes_ok(n_verts, n_faces), "mesh_components_round: %d vertices / %d faces out of range (faces <= %d)",
                  n_verts, n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(changed_dev && (n_verts == 0 || label) && (n_faces == 0 || faces), "mesh_components_round: null pointer");
    hipStream_t s = as_stream(stream);
    if (!mc_hip_ok(hipMemsetAsync(changed_dev, 0, 4, s), "mesh_components_round: clearing the flag")) return LNERF_ERR_HIP;
    if (n_faces > 0 && n_verts > 0) {
        MC_LAUNCH(k_mcc_hook, n_faces, faces, n_verts, n_faces, label, changed_dev);
        LNERF_CHECK_LAUNCH("mesh_components_round(hook)");
        MC_LAUNCH(k_mcc_jump, n_verts, n_verts, label);
        LNERF_CHECK_LAUNCH("mesh_components_round(jump)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_components_scratch_bytes(int n_verts, int n_faces) {
    if (!mc_sizes_ok(n_verts, n_faces)) return 0;
    return comp_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_components_finish(const float *verts, int n_verts, const int32_t *faces, int n_faces, const int32_t *label,
                                 void *scratch, size_t scratch_bytes, int32_t *vert_comp, int32_t *face_comp,
                                 int32_t *comp_faces, float *comp_box, int64_t *counts_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(mc_sizes_ok(n_verts, n_faces), "mesh_components_finish: %d vertices / %d faces out of range (faces <= %d)",
                  n_verts, n_faces, LNERF_MESH_MAX_FACES);
    const CompLayout L = comp_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch && counts_dev, "mesh_components_finish: null pointer");
    LNERF_REQUIRE((n_verts == 0 || (verts && label && vert_comp)) && (n_faces == 0 || (faces && face_comp)) &&
                  (L.cap == 0 || (comp_faces && comp_box)), "mesh_components_finish: null pointer");
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "mesh_components_finish: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh_components_finish: scratch must be 16-byte aligned");
    const int V = n_verts, F = n_faces, cap = L.cap;
    int32_t *referenced = MC_AT(int32_t, L.referenced), *root_rank = MC_AT(int32_t, L.root_rank);
    int64_t *blk_roots = MC_AT(int64_t, L.blk_roots), *blk_ref = MC_AT(int64_t, L.blk_ref);
    uint32_t *enc = MC_AT(uint32_t, L.enc);
    hipStream_t s = as_stream(stream);
    if (V > 0 && !mc_hip_ok(hipMemsetAsync(referenced, 0, (size_t)V * 4, s), "mesh_components_finish: clearing the marks"))
        return LNERF_ERR_HIP;
    if (cap > 0 && (!mc_hip_ok(hipMemsetAsync(comp_faces, 0, (size_t)cap * 4, s), "mesh_components_finish: clearing") ||
                    !mc_hip_ok(hipMemsetAsync(enc, 0xff, (size_t)cap * 12, s), "mesh_components_finish: clearing") ||
                    !mc_hip_ok(hipMemsetAsync(enc + (size_t)3 * cap, 0, (size_t)cap * 12, s),
                               "mesh_components_finish: clearing")))
        return LNERF_ERR_HIP;
    if (V > 0) {
        if (F > 0) MC_LAUNCH(k_mcc_mark, F, faces, V, F, referenced);
        MC_LAUNCH(k_mcc_roots, V, referenced, label, V, root_rank, blk_roots, blk_ref);
        LNERF_CHECK_LAUNCH("mesh_components_finish(roots)");
    }
    hipLaunchKernelGGL(k_scan_top<int64_t>, dim3(1), dim3(SCAN_TOP_THREADS), 0, s, blk_roots, blk_ref, L.nb, counts_dev,
                       counts_dev + 1);
    LNERF_CHECK_LAUNCH("mesh_components_finish(scan)");
    if (V > 0) {
        MC_LAUNCH(k_mcc_assign, V, referenced, label, V, root_rank, blk_roots, vert_comp);
        LNERF_CHECK_LAUNCH("mesh_components_finish(assign)");
    }
    if (F > 0) {
        MC_LAUNCH(k_mcc_faces, F, faces, V, F, vert_comp, cap, face_comp, comp_faces);
        LNERF_CHECK_LAUNCH("mesh_components_finish(faces)");
    }
    if (cap > 0) {
        MC_LAUNCH(k_mcc_box, V, verts, V, vert_comp, cap, enc);
        MC_LAUNCH(k_mcc_unbox, cap, enc, cap, counts_dev, comp_box);
        LNERF_CHECK_LAUNCH("mesh_components_finish(boxes)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_filter_scratch_bytes(int n_verts, int n_faces) {
    if (!mc_sizes_ok(n_verts, n_faces)) return 0;
    return filter_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_filter(const int32_t *faces, int n_verts, int n_faces, const uint8_t *face_keep, void *scratch,
                      size_t scratch_bytes, int32_t *faces_out, int32_t *vert_src, int64_t *counts_dev,
                      lnerf_stream_t stream) {
    LNERF_REQUIRE(mc_sizes_ok(n_verts, n_faces), "mesh_filter: %d vertices / %d faces out of range (faces <= %d)", n_verts,
                  n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(scratch && counts_dev && (n_verts == 0 || vert_src) && (n_faces == 0 || (faces && face_keep && faces_out)),
                  "mesh_filter: null pointer");
    const FilterLayout L = filter_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "mesh_filter: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh_filter: scratch must be 16-byte aligned");
    const int V = n_verts, F = n_faces, n = std::max(V, F);
    int32_t *used = MC_AT(int32_t, L.used), *vert_at = MC_AT(int32_t, L.vert_at), *face_at = MC_AT(int32_t, L.face_at);
    int64_t *blk_v = MC_AT(int64_t, L.blk_v), *blk_f = MC_AT(int64_t, L.blk_f);
    hipStream_t s = as_stream(stream);
    if (V > 0 && !mc_hip_ok(hipMemsetAsync(used, 0, (size_t)V * 4, s), "mesh_filter: clearing the marks")) return LNERF_ERR_HIP;
    if (n > 0) {
        if (F > 0 && V > 0) MC_LAUNCH(k_mf_mark, F, faces, V, F, face_keep, used);
        MC_LAUNCH(k_mf_rank, n, faces, V, F, face_keep, used, vert_at, face_at, blk_v, blk_f);
        LNERF_CHECK_LAUNCH("mesh_filter(rank)");
    }
    hipLaunchKernelGGL(k_scan_top<int64_t>, dim3(1), dim3(SCAN_TOP_THREADS), 0, s, blk_v, blk_f, L.nb, counts_dev,
                       counts_dev + 1);
    LNERF_CHECK_LAUNCH("mesh_filter(scan)");
    if (n > 0) {
        MC_LAUNCH(k_mf_emit, n, faces, V, F, face_keep, used, vert_at, face_at, blk_v, blk_f, faces_out, vert_src);
        LNERF_CHECK_LAUNCH("mesh_filter(emit)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_smooth_scratch_bytes(int n_verts, int n_faces) {
    if (!mc_sizes_ok(n_verts, n_faces)) return 0;
    return smooth_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_smooth(const float *verts, int n_verts, const int32_t *faces, int n_faces, int iterations, float lambda,
                      float mu, void *scratch, size_t scratch_bytes, float *verts_out, float *normals_out,
                      lnerf_stream_t stream) {
    LNERF_REQUIRE(mc_sizes_ok(n_verts, n_faces), "mesh_smooth: %d vertices / %d faces out of range (faces <= %d)", n_verts,
                  n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(iterations >= 0 && iterations <= LNERF_SMOOTH_MAX_ITER, "mesh_smooth: %d iterations outside [0, %d]",
                  iterations, LNERF_SMOOTH_MAX_ITER);
    LNERF_REQUIRE(lambda > 0.f && lambda <= 1.f, "mesh_smooth: lambda must be in (0, 1]");
    LNERF_REQUIRE(mu >= -1.5f && mu <= 0.f, "mesh_smooth: mu must be in [-1.5, 0]");
    LNERF_REQUIRE(scratch && (n_verts == 0 || (verts && verts_out)) && (n_faces == 0 || faces), "mesh_smooth: null pointer");
    LNERF_REQUIRE(verts != verts_out || n_verts == 0, "mesh_smooth: verts_out must not be verts");
    const SmoothLayout L = smooth_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "mesh_smooth: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh_smooth: scratch must be 16-byte aligned");
    const int V = n_verts, F = n_faces;
    if (V == 0) {
        LNERF_REQUIRE(F == 0, "mesh_smooth: %d faces index outside [0, 0)", F);
        return LNERF_OK;
    }
    unsigned long long *n_bad = MC_AT(unsigned long long, L.dev);
    int32_t *cnt = MC_AT(int32_t, L.cnt), *cur = MC_AT(int32_t, L.cur), *loc = MC_AT(int32_t, L.loc);
    int32_t *list = MC_AT(int32_t, L.list);
    int64_t *blk = MC_AT(int64_t, L.blk);
    float *tmp = MC_AT(float, L.tmp);
    hipStream_t s = as_stream(stream);
    // ---- index range first: no kernel reads through a face before this
    if (F > 0) {
        if (!mc_hip_ok(hipMemsetAsync(n_bad, 0, 8, s), "mesh_smooth: clearing the count")) return LNERF_ERR_HIP;
        MC_LAUNCH(k_ms_check, F, faces, V, F, n_bad);
        LNERF_CHECK_LAUNCH("mesh_smooth(check)");
        unsigned long long bad = 0;
        if (!mc_hip_ok(hipMemcpyAsync(&bad, n_bad, 8, hipMemcpyDeviceToHost, s), "mesh_smooth: read-back") ||
            !mc_hip_ok(hipStreamSynchronize(s), "mesh_smooth: read-back"))
            return LNERF_ERR_HIP;
        LNERF_REQUIRE(bad == 0, "mesh_smooth: %llu faces index outside [0, %d)", bad, V);
    }
    // ---- incidence lists
    if (!mc_hip_ok(hipMemsetAsync(cnt, 0, (size_t)V * 4, s), "mesh_smooth: clearing the counts") ||
        !mc_hip_ok(hipMemsetAsync(cur, 0, (size_t)V * 4, s), "mesh_smooth: clearing the cursors"))
        return LNERF_ERR_HIP;
    if (F > 0) MC_LAUNCH(k_ms_count, F, faces, F, cnt);
    MC_LAUNCH(k_ms_rank, V, cnt, V, loc, blk);
    hipLaunchKernelGGL(k_scan_top<int64_t>, dim3(1), dim3(SCAN_TOP_THREADS), 0, s, blk, (int64_t *)nullptr, L.nb, blk + L.nb,
                       (int64_t *)nullptr);
    LNERF_CHECK_LAUNCH("mesh_smooth(scan)");
    if (F > 0) {
        MC_LAUNCH(k_ms_fill, F, faces, F, loc, blk, cur, list);
        MC_LAUNCH(k_ms_sort, V, cnt, loc, blk, V, list);
        LNERF_CHECK_LAUNCH("mesh_smooth(lists)");
    }
    // ---- steps: ping-pong between verts_out and the scratch copy, arranged so that the last step lands in verts_out
    const float w[2] = {lambda, mu};
    const int per_iter = mu != 0.f ? 2 : 1;
    const int64_t steps = (int64_t)iterations * per_iter;
    if (steps == 0) {
        if (!mc_hip_ok(hipMemcpyAsync(verts_out, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, s), "mesh_smooth: copy"))
            return LNERF_ERR_HIP;
    }
    const float *src = verts;
    for (int64_t i = 0; i < steps; ++i) {
        float *dst = ((steps - 1 - i) & 1) ? tmp : verts_out;
        MC_LAUNCH(k_ms_step, V, src, faces, cnt, loc, blk, list, V, w[i % per_iter], dst);
        LNERF_CHECK_LAUNCH("mesh_smooth(step)");
        src = dst;
    }
    if (normals_out) {
        MC_LAUNCH(k_ms_normals, V, verts_out, faces, cnt, loc, blk, list, V, normals_out);
        LNERF_CHECK_LAUNCH("mesh_smooth(normals)");
    }
    return LNERF_OK;
}

}  // extern "C"
