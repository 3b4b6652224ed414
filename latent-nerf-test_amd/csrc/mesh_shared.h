// The primitives of the mesh kernels after marching cubes (meshclean.hip, decimate.hip, atlas.hip), each written once:
//   faces        face_ok (index range: nothing may be read through a face that fails it), face_repeats, face_corner,
//                count_bad (one atomic per wave)
//   labels       k_label_jump (pointer jumping), root_number (the number of a ranked root after k_scan_top)
//   boxes        ordered_encode / ordered_decode, box_clear, k_box_decode: boxes by integer atomicMin / atomicMax
//   lists        vertex_face_lists (k_vf_count, scan_flat, k_vf_fill, k_vf_sort): off [V+1], list of faces, ascending per
//                vertex, faces that repeat an index left out; k_vertex_normals over them
// One lane per face, half-edge or vertex in workgroups of MESH_THREADS.  Every loop has a bound known at launch; integer
// atomics only (min / max / add commute, so the results do not depend on their order).
#pragma once
#include "common.h"
#include "scan.h"

namespace lnerf {

constexpr int MESH_THREADS = 256;
constexpr int MESH_LOG2 = 8;
static_assert(LNERF_ATLAS_JUMP_HOPS == LNERF_MESH_JUMP_HOPS, "k_label_jump serves both with one hop count");
constexpr int LABEL_JUMP_HOPS = LNERF_MESH_JUMP_HOPS;

__device__ __forceinline__ int mesh_gid() { return blockIdx.x * MESH_THREADS + threadIdx.x; }

// one lane per item of n on the stream `s` of the calling function
#define MESH_LAUNCH(kernel, n, ...) LNERF_LAUNCH(kernel, n, ::lnerf::MESH_THREADS, s, __VA_ARGS__)

// ---------------------------------------------------------------- faces
// the three indices of face f; false if one lies outside [0, n_verts) (nothing may be read through them then)
__device__ __forceinline__ bool face_ok(const int32_t *__restrict__ faces, int n_verts, int f, int v[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = faces[(int64_t)f * 3 + k];
        ok = ok && v[k] >= 0 && v[k] < n_verts;
    }
    return ok;
}

__device__ __forceinline__ bool face_repeats(int a, int b, int c) { return a == b || b == c || c == a; }

// the vertices after / before w in face f (w must be a corner of f)
__device__ __forceinline__ void face_corner(const int32_t *__restrict__ faces, int f, int w, int &nxt, int &prv) {
    const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
    if (a == w) { nxt = b; prv = c; }
    else if (b == w) { nxt = c; prv = a; }
    else { nxt = a; prv = b; }
}

// *n_bad += the lanes of this wave with `bad`, one atomic per wave.  EVERY lane of the wave calls it.
__device__ __forceinline__ void count_bad(bool bad, unsigned long long *__restrict__ n_bad) {
    const unsigned long long mask = __ballot(bad);
    if (lane_id() == 0 && mask != 0) atomicAdd(n_bad, (unsigned long long)__popcll(mask));
}

// ---------------------------------------------------------------- labels
// LABEL_JUMP_HOPS steps of label = label[label] over label[0, n).  Labels only ever decrease and always name an entry of
// the same component, so a plain read that misses another workgroup's atomicMin sees an older valid label.
static __global__ void __launch_bounds__(MESH_THREADS)
k_label_jump(int n, int32_t *label) {
    const int i = mesh_gid();
    if (i >= n) return;
    const int l0 = label[i];
    int l = l0;
#pragma unroll
    for (int h = 0; h < LABEL_JUMP_HOPS; ++h) {
        if (l < 0 || l >= n) return;
        const int ll = label[l];
        if (ll < l) l = ll;
    }
    if (l >= 0 && l < l0) atomicMin(&label[i], l);
}

// the number of root l: its rank inside its block of MESH_THREADS entries + the block's prefix (after k_scan_top)
__device__ __forceinline__ int root_number(const int64_t *__restrict__ blk_roots, const int32_t *__restrict__ root_rank,
                                           int l) {
    return (int)blk_roots[l >> MESH_LOG2] + root_rank[l];
}

// ---------------------------------------------------------------- boxes
// f32 -> u32 with the same order (negative values reversed below the positive ones, so -0 < +0)
__device__ __forceinline__ uint32_t ordered_encode(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_decode(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

// enc: K planes of n encoded bounds -> box [n][K] f32; entries from *count on (count may be NULL) are left alone
template <int K>
static __global__ void __launch_bounds__(MESH_THREADS)
k_box_decode(const uint32_t *__restrict__ enc, int n, const int64_t *__restrict__ count, float *__restrict__ box) {
    const int c = mesh_gid();
    if (c >= n || (count && c >= *count)) return;
#pragma unroll
    for (int k = 0; k < K; ++k) box[(int64_t)c * K + k] = ordered_decode(enc[(int64_t)k * n + c]);
}

// the neutral values of atomicMin / atomicMax: n lower bounds at lo to ~0, n upper bounds at hi to 0
static inline bool box_clear(uint32_t *lo, uint32_t *hi, size_t n, hipStream_t s, const char *what) {
    return hip_ok(hipMemsetAsync(lo, 0xff, n * 4, s), what) && hip_ok(hipMemsetAsync(hi, 0, n * 4, s), what);
}

// ---------------------------------------------------------------- vertex -> face lists
// One lane per face.  A face that repeats an index is in no list (a kept face holds each of its vertices once).
static __global__ void __launch_bounds__(MESH_THREADS)
k_vf_count(const int32_t *__restrict__ faces, int F, int32_t *__restrict__ cnt) {
    const int f = mesh_gid();
    if (f >= F) return;
    const int v[3] = {faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]};
    if (face_repeats(v[0], v[1], v[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&cnt[v[k]], 1);
}

static __global__ void __launch_bounds__(MESH_THREADS)
k_vf_fill(const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ off, int32_t *__restrict__ cur,
          int32_t *__restrict__ list) {
    const int f = mesh_gid();
    if (f >= F) return;
    const int v[3] = {faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]};
    if (face_repeats(v[0], v[1], v[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) list[off[v[k]] + atomicAdd(&cur[v[k]], 1)] = f;
}

static __global__ void __launch_bounds__(MESH_THREADS)
k_vf_sort(const int32_t *__restrict__ off, int V, int32_t *__restrict__ list) {
    const int w = mesh_gid();
    if (w >= V) return;
    const int b = off[w], e = off[w + 1];
    for (int i = b + 1; i < e; ++i) {          // insertion sort: the lists are short
        const int x = list[i];
        int j = i - 1;
        while (j >= b && list[j] > x) {
            list[j + 1] = list[j];
            --j;
        }
        list[j + 1] = x;
    }
}

// Lists of faces [F] (every index in [0, V)) over V vertices: off [V+1], list [3F]; cnt [V] and blk (scan_flat_blk_bytes(V))
// are scratch.  `what` names the caller in an error.
static inline int vertex_face_lists(const int32_t *faces, int F, int V, int32_t *cnt, int32_t *off, int32_t *list,
                                    int32_t *blk, hipStream_t s, const char *what) {
    if (!hip_ok(hipMemsetAsync(cnt, 0, (size_t)V * 4, s), what)) return LNERF_ERR_HIP;
    MESH_LAUNCH(k_vf_count, F, faces, F, cnt);
    const int rc = scan_flat(cnt, V, off, blk, s, what);
    if (rc != LNERF_OK) return rc;
    if (!hip_ok(hipMemsetAsync(cnt, 0, (size_t)V * 4, s), what)) return LNERF_ERR_HIP;
    MESH_LAUNCH(k_vf_fill, F, faces, F, off, cnt, list);
    MESH_LAUNCH(k_vf_sort, V, off, V, list);
    LNERF_CHECK_LAUNCH(what);
    return LNERF_OK;
}

// one lane per vertex: the f32 sum of its faces' cross products in ascending face order, normalised (0 where it is 0)
static __global__ void __launch_bounds__(MESH_THREADS)
k_vertex_normals(const float *__restrict__ verts, const int32_t *__restrict__ faces, const int32_t *__restrict__ off,
                 const int32_t *__restrict__ list, int V, float *__restrict__ normals) {
    const int w = mesh_gid();
    if (w >= V) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int s = off[w]; s < off[w + 1]; ++s) {
        const int64_t f = list[s];
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
    normals[(int64_t)w * 3] = s0 * inv;
    normals[(int64_t)w * 3 + 1] = s1 * inv;
    normals[(int64_t)w * 3 + 2] = s2 * inv;
}

// ---------------------------------------------------------------- host side
static inline bool mesh_sizes_ok(int n_verts, int n_faces, int max_faces) {
    return n_verts >= 0 && n_faces >= 0 && n_faces <= max_faces && n_verts <= 3 * (int64_t)max_faces;
}
#define MESH_REQUIRE_SIZES(op, V, F, max_faces)                                                                     \
    LNERF_REQUIRE(::lnerf::mesh_sizes_ok(V, F, max_faces), op ": %d vertices / %d faces out of range (faces <= %d)", \
                  V, F, max_faces)

}  // namespace lnerf
