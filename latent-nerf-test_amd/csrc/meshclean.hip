// Mesh cleaning between marching cubes and the decimation: connected components, a stable face / vertex filter and
// Taubin smoothing.  Contract: include/lnerf_hip.h, "mesh cleaning"; numpy restatement: tests/meshclean_reference.py.
// Every loop in a kernel has a bound known at launch (the lists' lengths are fixed before the kernels that walk them
// start); nothing here waits on another workgroup.  Integer atomics only (min / max / add commute, so the results do
// not depend on their order); f32 / f64 arithmetic is + - * / sqrt in the order written.
//
//   lnerf_mesh_components_begin   k_mcc_begin    label[v] = v; the faces with an index out of range are counted
//   lnerf_mesh_components_round   k_mcc_hook     one lane per face: the smallest label of its corners -> atomicMin onto
//                                                every larger corner label and that label's label
//                                 k_label_jump   (mesh_shared.h) one lane per vertex: pointer jumping
//   lnerf_mesh_components_finish  k_mcc_mark     referenced[v] = 1 for the corners of the valid faces
//                                 k_mcc_roots    referenced roots ranked inside each block (scan.h), block totals of the
//                                                roots and of the referenced vertices
//                                 scan_top       (scan.h) prefix of both -> counts = {components, referenced vertices}
//                                 k_mcc_assign   vert_comp = root_number (mesh_shared.h) of the vertex's root
//                                 k_mcc_faces    face_comp, comp_faces (atomicAdd; one per wave where a wave agrees)
//                                 k_mcc_box      atomicMin / atomicMax of the order-preserving encoding of the vertex
//                                                coordinates into the component's box (one per wave where a wave agrees)
//                                 k_box_decode   (mesh_shared.h) one lane per component: back to f32
//   lnerf_mesh_filter             k_mf_mark      used[v] = 1 for the corners of the kept faces
//                                 k_mf_rank      kept faces and used vertices ranked inside each block, block totals
//                                 scan_top       prefix of both -> counts = {vertices out, faces out}
//                                 k_mf_emit      vert_src, re-indexed faces
//   lnerf_mesh_smooth             k_ms_check     faces with an index out of range are counted -- host read --
//                                 vertex_face_lists   (mesh_shared.h) vertex -> face lists, each ascending
//                                 k_ms_step      one lane per vertex: p' = p + w (mean of the incident faces' other
//                                                corners - p) in f64, from the positions before the step
//                                 k_vertex_normals   (mesh_shared.h) lnerf_decimate's normals
#include <algorithm>

#include "common.h"
#include "mesh_shared.h"
#include "scan.h"

namespace lnerf {

// the value of `x` in the first lane of `mask` (mask != 0)
__device__ __forceinline__ int wave_first(unsigned long long mask, int x) {
    return __shfl(x, __ffsll((long long)mask) - 1, LNERF_WAVE);
}

// ---------------------------------------------------------------- connected components
__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_begin(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *__restrict__ label,
            unsigned long long *__restrict__ n_bad) {
    const int i = mesh_gid();
    if (i < n_verts) label[i] = i;
    bool bad = false;
    if (i < n_faces) {
        int v[3];
        bad = !face_ok(faces, n_verts, i, v);
    }
    count_bad(bad, n_bad);
}

// Labels only ever decrease and always name a vertex of the same component, so a plain read that misses another
// workgroup's atomicMin of the same launch sees an older valid label: it costs at most a round, never the result.  A
// launch in which no lane raises `changed` wrote nothing, so all it read was the settled state (see k_atlas_hook).
__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_hook(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *label, int32_t *__restrict__ changed) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    int v[3], l[3];
    if (!face_ok(faces, n_verts, f, v)) return;
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

// (several faces may mark one vertex: every writer stores the same 1)
__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_mark(const int32_t *__restrict__ faces, int n_verts, int n_faces, int32_t *__restrict__ referenced) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    int v[3];
    if (!face_ok(faces, n_verts, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) referenced[v[k]] = 1;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_roots(const int32_t *__restrict__ referenced, const int32_t *__restrict__ label, int n_verts,
            int32_t *__restrict__ root_rank, int64_t *__restrict__ blk_roots, int64_t *__restrict__ blk_ref) {
    const int v = mesh_gid();
    const int r = (v < n_verts && referenced[v]) ? 1 : 0;
    const int n[2] = {(r && label[v] == v) ? 1 : 0, r};
    int excl[2], total[2];
    block_exclusive_scan<MESH_THREADS>(n, excl, total);
    if (v < n_verts) root_rank[v] = excl[0];
    if (threadIdx.x == 0) {
        blk_roots[blockIdx.x] = total[0];
        blk_ref[blockIdx.x] = total[1];
    }
}

__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_assign(const int32_t *__restrict__ referenced, const int32_t *__restrict__ label, int n_verts,
             const int32_t *__restrict__ root_rank, const int64_t *__restrict__ blk_roots,
             int32_t *__restrict__ vert_comp) {
    const int v = mesh_gid();
    if (v >= n_verts) return;
    const int l = label[v];
    int c = -1;
    if (referenced[v] && l >= 0 && l < n_verts) c = root_number(blk_roots, root_rank, l);
    vert_comp[v] = c;
}

// One lane per face.  Where every counted face of a wave lies in one component (the usual case: faces of a component are
// neighbours in the list) the wave adds its count once.
__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_faces(const int32_t *__restrict__ faces, int n_verts, int n_faces, const int32_t *__restrict__ vert_comp, int cap,
            int32_t *__restrict__ face_comp, int32_t *comp_faces) {
    const int f = mesh_gid();
    int c = -1;
    if (f < n_faces) {
        int v[3];
        if (face_ok(faces, n_verts, f, v)) c = vert_comp[v[0]];
        if (c >= cap) c = -1;
        face_comp[f] = c;
    }
    const unsigned long long mask = __ballot(c >= 0);
    if (mask == 0) return;
    const int c0 = wave_first(mask, c);
    if (__ballot(c >= 0 && c != c0) == 0) {
        if (lane_id() == 0) atomicAdd(&comp_faces[c0], (int)__popcll(mask));
    } else if (c >= 0) {
        atomicAdd(&comp_faces[c], 1);
    }
}

// enc: [6][cap] u32 = x_lo, y_lo, z_lo (cleared to ~0), x_hi, y_hi, z_hi (cleared to 0)
__global__ void __launch_bounds__(MESH_THREADS)
k_mcc_box(const float *__restrict__ verts, int n_verts, const int32_t *__restrict__ vert_comp, int cap, uint32_t *enc) {
    const int v = mesh_gid();
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
    const int c0 = wave_first(mask, c);
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

// ---------------------------------------------------------------- filter
__device__ __forceinline__ bool mf_kept(const int32_t *__restrict__ faces, int n_verts, const uint8_t *__restrict__ keep,
                                        int f, int v[3]) {
    return keep[f] != 0 && face_ok(faces, n_verts, f, v);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_mf_mark(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          int32_t *__restrict__ used) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    int v[3];
    if (!mf_kept(faces, n_verts, keep, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) used[v[k]] = 1;
}

// lane i ranks vertex i and face i
__global__ void __launch_bounds__(MESH_THREADS)
k_mf_rank(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          const int32_t *__restrict__ used, int32_t *__restrict__ vert_at, int32_t *__restrict__ face_at,
          int64_t *__restrict__ blk_v, int64_t *__restrict__ blk_f) {
    const int i = mesh_gid();
    int v[3];
    const int n[2] = {(i < n_verts && used[i]) ? 1 : 0, (i < n_faces && mf_kept(faces, n_verts, keep, i, v)) ? 1 : 0};
    int excl[2], total[2];
    block_exclusive_scan<MESH_THREADS>(n, excl, total);
    if (i < n_verts) vert_at[i] = excl[0];
    if (i < n_faces) face_at[i] = excl[1];
    if (threadIdx.x == 0) {
        blk_v[blockIdx.x] = total[0];
        blk_f[blockIdx.x] = total[1];
    }
}

__global__ void __launch_bounds__(MESH_THREADS)
k_mf_emit(const int32_t *__restrict__ faces, int n_verts, int n_faces, const uint8_t *__restrict__ keep,
          const int32_t *__restrict__ used, const int32_t *__restrict__ vert_at, const int32_t *__restrict__ face_at,
          const int64_t *__restrict__ blk_v, const int64_t *__restrict__ blk_f, int32_t *__restrict__ faces_out,
          int32_t *__restrict__ vert_src) {
    const int i = mesh_gid();
    if (i < n_verts && used[i]) vert_src[blk_v[blockIdx.x] + vert_at[i]] = i;
    int v[3];
    if (i < n_faces && mf_kept(faces, n_verts, keep, i, v)) {
        const int64_t o = (blk_f[blockIdx.x] + face_at[i]) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) faces_out[o + k] = (int32_t)(blk_v[v[k] >> MESH_LOG2] + vert_at[v[k]]);
    }
}

// ---------------------------------------------------------------- smoothing
__global__ void __launch_bounds__(MESH_THREADS)
k_ms_check(const int32_t *__restrict__ faces, int n_verts, int n_faces, unsigned long long *__restrict__ n_bad) {
    const int f = mesh_gid();
    bool bad = false;
    if (f < n_faces) {
        int v[3];
        bad = !face_ok(faces, n_verts, f, v);
    }
    count_bad(bad, n_bad);
}

// (the faces passed k_ms_check: every index is in range)
__global__ void __launch_bounds__(MESH_THREADS)
k_ms_step(const float *__restrict__ src, const int32_t *__restrict__ faces, const int32_t *__restrict__ off,
          const int32_t *__restrict__ list, int n_verts, float w, float *__restrict__ dst) {
    const int v = mesh_gid();
    if (v >= n_verts) return;
    const float p[3] = {src[(int64_t)v * 3], src[(int64_t)v * 3 + 1], src[(int64_t)v * 3 + 2]};
    const int s0 = off[v], n = off[v + 1] - s0;
    if (n == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) dst[(int64_t)v * 3 + a] = p[a];
        return;
    }
    double S[3] = {0.0, 0.0, 0.0};
    for (int s = s0; s < s0 + n; ++s) {
        int nxt, prv;
        face_corner(faces, list[s], v, nxt, prv);
        const int64_t a = nxt, b = prv;
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

// ---------------------------------------------------------------- host side
struct CompLayout {
    int cap;
    int64_t nb;
    size_t referenced, root_rank, blk_roots, blk_ref, enc, bytes;
};

static CompLayout comp_layout(int V, int F) {
    CompLayout L;
    Carve c;
    L.cap = std::min(V, F);          // every component holds a face and a vertex of its own
    L.nb = div_up(V, MESH_THREADS);
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
    L.nb = div_up(std::max(V, F), MESH_THREADS);
    L.used = c.take((size_t)V * 4);
    L.vert_at = c.take((size_t)V * 4);
    L.face_at = c.take((size_t)F * 4);
    L.blk_v = c.take((size_t)L.nb * 8);
    L.blk_f = c.take((size_t)L.nb * 8);
    L.bytes = std::max<size_t>(c.o, 256);
    return L;
}

struct SmoothLayout {
    size_t dev, cnt, off, list, blk, tmp, bytes;
};

static SmoothLayout smooth_layout(int V, int F) {
    SmoothLayout L;
    Carve c;
    L.dev = c.take(64);
    L.cnt = c.take((size_t)V * 4);
    L.off = c.take(((size_t)V + 1) * 4);
    L.list = c.take((size_t)F * 12);
    L.blk = c.take(scan_flat_blk_bytes(V));
    L.tmp = c.take((size_t)V * 12);
    L.bytes = c.o;
    return L;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_mesh_components_begin(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int64_t *counts_dev,
                                lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("mesh_components_begin", n_verts, n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(counts_dev && (n_verts == 0 || label) && (n_faces == 0 || faces), "mesh_components_begin: null pointer");
    hipStream_t s = as_stream(stream);
    if (!hip_ok(hipMemsetAsync(counts_dev, 0, 8, s), "mesh_components_begin: clearing the count")) return LNERF_ERR_HIP;
    if (std::max(n_verts, n_faces) > 0) {
        MESH_LAUNCH(k_mcc_begin, std::max(n_verts, n_faces), faces, n_verts, n_faces, label,
                    reinterpret_cast<unsigned long long *>(counts_dev));
        LNERF_CHECK_LAUNCH("mesh_components_begin");
    }
    return LNERF_OK;
}

int lnerf_mesh_components_round(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int32_t *changed_dev,
                                lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("mesh_components_round", n_verts, n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(changed_dev && (n_verts == 0 || label) && (n_faces == 0 || faces), "mesh_components_round: null pointer");
    hipStream_t s = as_stream(stream);
    if (!hip_ok(hipMemsetAsync(changed_dev, 0, 4, s), "mesh_components_round: clearing the flag")) return LNERF_ERR_HIP;
    if (n_faces > 0 && n_verts > 0) {
        MESH_LAUNCH(k_mcc_hook, n_faces, faces, n_verts, n_faces, label, changed_dev);
        LNERF_CHECK_LAUNCH("mesh_components_round(hook)");
        MESH_LAUNCH(k_label_jump, n_verts, n_verts, label);
        LNERF_CHECK_LAUNCH("mesh_components_round(jump)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_components_scratch_bytes(int n_verts, int n_faces) {
    if (!mesh_sizes_ok(n_verts, n_faces, LNERF_MESH_MAX_FACES)) return 0;
    return comp_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_components_finish(const float *verts, int n_verts, const int32_t *faces, int n_faces, const int32_t *label,
                                 void *scratch, size_t scratch_bytes, int32_t *vert_comp, int32_t *face_comp,
                                 int32_t *comp_faces, float *comp_box, int64_t *counts_dev, lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("mesh_components_finish", n_verts, n_faces, LNERF_MESH_MAX_FACES);
    const CompLayout L = comp_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch && counts_dev, "mesh_components_finish: null pointer");
    LNERF_REQUIRE((n_verts == 0 || (verts && label && vert_comp)) && (n_faces == 0 || (faces && face_comp)) &&
                  (L.cap == 0 || (comp_faces && comp_box)), "mesh_components_finish: null pointer");
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "mesh_components_finish: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh_components_finish: scratch must be 16-byte aligned");
    const int V = n_verts, F = n_faces, cap = L.cap;
    int32_t *referenced = at<int32_t>(scratch, L.referenced), *root_rank = at<int32_t>(scratch, L.root_rank);
    int64_t *blk_roots = at<int64_t>(scratch, L.blk_roots), *blk_ref = at<int64_t>(scratch, L.blk_ref);
    uint32_t *enc = at<uint32_t>(scratch, L.enc);
    hipStream_t s = as_stream(stream);
    if (V > 0 && !hip_ok(hipMemsetAsync(referenced, 0, (size_t)V * 4, s), "mesh_components_finish: clearing the marks"))
        return LNERF_ERR_HIP;
    if (cap > 0 && (!hip_ok(hipMemsetAsync(comp_faces, 0, (size_t)cap * 4, s), "mesh_components_finish: clearing") ||
                    !box_clear(enc, enc + (size_t)3 * cap, (size_t)3 * cap, s, "mesh_components_finish: clearing")))
        return LNERF_ERR_HIP;
    if (V > 0) {
        if (F > 0) MESH_LAUNCH(k_mcc_mark, F, faces, V, F, referenced);
        MESH_LAUNCH(k_mcc_roots, V, referenced, label, V, root_rank, blk_roots, blk_ref);
        LNERF_CHECK_LAUNCH("mesh_components_finish(roots)");
    }
    scan_top(blk_roots, blk_ref, L.nb, counts_dev, counts_dev + 1, s);
    LNERF_CHECK_LAUNCH("mesh_components_finish(scan)");
    if (V > 0) {
        MESH_LAUNCH(k_mcc_assign, V, referenced, label, V, root_rank, blk_roots, vert_comp);
        LNERF_CHECK_LAUNCH("mesh_components_finish(assign)");
    }
    if (F > 0) {
        MESH_LAUNCH(k_mcc_faces, F, faces, V, F, vert_comp, cap, face_comp, comp_faces);
        LNERF_CHECK_LAUNCH("mesh_components_finish(faces)");
    }
    if (cap > 0) {
        MESH_LAUNCH(k_mcc_box, V, verts, V, vert_comp, cap, enc);
        MESH_LAUNCH(k_box_decode<6>, cap, enc, cap, counts_dev, comp_box);
        LNERF_CHECK_LAUNCH("mesh_components_finish(boxes)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_filter_scratch_bytes(int n_verts, int n_faces) {
    if (!mesh_sizes_ok(n_verts, n_faces, LNERF_MESH_MAX_FACES)) return 0;
    return filter_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_filter(const int32_t *faces, int n_verts, int n_faces, const uint8_t *face_keep, void *scratch,
                      size_t scratch_bytes, int32_t *faces_out, int32_t *vert_src, int64_t *counts_dev,
                      lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("mesh_filter", n_verts, n_faces, LNERF_MESH_MAX_FACES);
    LNERF_REQUIRE(scratch && counts_dev && (n_verts == 0 || vert_src) && (n_faces == 0 || (faces && face_keep && faces_out)),
                  "mesh_filter: null pointer");
    const FilterLayout L = filter_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "mesh_filter: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh_filter: scratch must be 16-byte aligned");
    const int V = n_verts, F = n_faces, n = std::max(V, F);
    int32_t *used = at<int32_t>(scratch, L.used), *vert_at = at<int32_t>(scratch, L.vert_at);
    int32_t *face_at = at<int32_t>(scratch, L.face_at);
    int64_t *blk_v = at<int64_t>(scratch, L.blk_v), *blk_f = at<int64_t>(scratch, L.blk_f);
    hipStream_t s = as_stream(stream);
    if (V > 0 && !hip_ok(hipMemsetAsync(used, 0, (size_t)V * 4, s), "mesh_filter: clearing the marks")) return LNERF_ERR_HIP;
    if (n > 0) {
        if (F > 0 && V > 0) MESH_LAUNCH(k_mf_mark, F, faces, V, F, face_keep, used);
        MESH_LAUNCH(k_mf_rank, n, faces, V, F, face_keep, used, vert_at, face_at, blk_v, blk_f);
        LNERF_CHECK_LAUNCH("mesh_filter(rank)");
    }
    scan_top(blk_v, blk_f, L.nb, counts_dev, counts_dev + 1, s);
    LNERF_CHECK_LAUNCH("mesh_filter(scan)");
    if (n > 0) {
        MESH_LAUNCH(k_mf_emit, n, faces, V, F, face_keep, used, vert_at, face_at, blk_v, blk_f, faces_out, vert_src);
        LNERF_CHECK_LAUNCH("mesh_filter(emit)");
    }
    return LNERF_OK;
}

size_t lnerf_mesh_smooth_scratch_bytes(int n_verts, int n_faces) {
    if (!mesh_sizes_ok(n_verts, n_faces, LNERF_MESH_MAX_FACES)) return 0;
    return smooth_layout(n_verts, n_faces).bytes;
}

int lnerf_mesh_smooth(const float *verts, int n_verts, const int32_t *faces, int n_faces, int iterations, float lambda,
                      float mu, void *scratch, size_t scratch_bytes, float *verts_out, float *normals_out,
                      lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("mesh_smooth", n_verts, n_faces, LNERF_MESH_MAX_FACES);
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
    unsigned long long *n_bad = at<unsigned long long>(scratch, L.dev);
    int32_t *off = at<int32_t>(scratch, L.off), *list = at<int32_t>(scratch, L.list);
    float *tmp = at<float>(scratch, L.tmp);
    hipStream_t s = as_stream(stream);
    // ---- index range first: no kernel reads through a face before this
    if (F > 0) {
        if (!hip_ok(hipMemsetAsync(n_bad, 0, 8, s), "mesh_smooth: clearing the count")) return LNERF_ERR_HIP;
        MESH_LAUNCH(k_ms_check, F, faces, V, F, n_bad);
        LNERF_CHECK_LAUNCH("mesh_smooth(check)");
        unsigned long long bad = 0;
        if (!read_back(n_bad, &bad, s, "mesh_smooth: read-back")) return LNERF_ERR_HIP;
        LNERF_REQUIRE(bad == 0, "mesh_smooth: %llu faces index outside [0, %d)", bad, V);
    }
    const int rc = vertex_face_lists(faces, F, V, at<int32_t>(scratch, L.cnt), off, list, at<int32_t>(scratch, L.blk), s,
                                     "mesh_smooth(lists)");
    if (rc != LNERF_OK) return rc;
    // ---- steps: ping-pong between verts_out and the scratch copy, arranged so that the last step lands in verts_out
    const float w[2] = {lambda, mu};
    const int per_iter = mu != 0.f ? 2 : 1;
    const int64_t steps = (int64_t)iterations * per_iter;
    if (steps == 0) {
        if (!hip_ok(hipMemcpyAsync(verts_out, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, s), "mesh_smooth: copy"))
            return LNERF_ERR_HIP;
    }
    const float *src = verts;
    for (int64_t i = 0; i < steps; ++i) {
        float *dst = ((steps - 1 - i) & 1) ? tmp : verts_out;
        MESH_LAUNCH(k_ms_step, V, src, faces, off, list, V, w[i % per_iter], dst);
        LNERF_CHECK_LAUNCH("mesh_smooth(step)");
        src = dst;
    }
    if (normals_out) {
        MESH_LAUNCH(k_vertex_normals, V, verts_out, faces, off, list, V, normals_out);
        LNERF_CHECK_LAUNCH("mesh_smooth(normals)");
    }
    return LNERF_OK;
}

}  // extern "C"
