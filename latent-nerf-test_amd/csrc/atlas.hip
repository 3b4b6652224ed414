// Chart UV atlas of a triangle mesh: raymarching.chart_atlas's kernels.  Contract: include/lnerf_hip.h, "chart atlas";
// numpy restatement: tests/atlas_reference.py.  Every loop in a kernel has a bound known at launch; nothing here waits
// on another workgroup.  Integer atomics only (min / max / add commute, so the results do not depend on their order).
//
//   lnerf_atlas_buckets  k_atlas_bucket   one lane per face: index check, axis bucket of the face normal, label = f
//   lnerf_atlas_round    k_atlas_hook     one lane per face: the smallest label among the face and its linked
//                                         same-bucket neighbours -> atomicMin onto the face's label and its label's label
//                        k_label_jump     (mesh_shared.h) one lane per face: pointer jumping
//   lnerf_atlas_compact  k_atlas_roots    roots (label[f] == f) ranked inside each block (scan.h), block totals
//                        scan_top         (scan.h) prefix of the block totals -> counts[0] = charts
//                        k_atlas_assign   face_chart = root_number (mesh_shared.h) of the face's root; chart_axis from
//                                         the root
//   lnerf_atlas_boxes    k_atlas_box      one lane per face: atomicMin / atomicMax of the order-preserving encoding of
//                                         its corners' plane coordinates into its chart's box
//                        k_box_decode     (mesh_shared.h) one lane per chart: back to f32
//   lnerf_atlas_uv       k_atlas_uv       one lane per face: its three texture vertices (a vertex shared inside a chart
//                                         is written by several faces, each with the same bits)
//   lnerf_atlas_fold     k_fold_setup     the item list of uvbake.hip (uv_shared.h) over the packed UVs
//                        k_fold_pass      one lane per (face, candidate texel).  <false>, pass A: atomicMax of the face
//                                         index over STRICT coverage; <true>, pass B: a face strictly covering a texel
//                                         it did not win is marked evicted (every writer stores the same 1)
#include "common.h"
#include "mesh_shared.h"
#include "scan.h"
#include "uv_shared.h"

namespace lnerf {

// plane coordinates (p, q) of a point in bucket b: p x q = the bucket's axis
__device__ __forceinline__ void atlas_plane(int b, float x, float y, float z, float &p, float &q) {
    switch (b) {
        case 0: p = y; q = z; break;
        case 1: p = z; q = y; break;
        case 2: p = z; q = x; break;
        case 3: p = x; q = z; break;
        case 4: p = x; q = y; break;
        default: p = y; q = x; break;
    }
}

__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_bucket(const float *__restrict__ verts, int n_verts, const int32_t *__restrict__ faces, int n_faces,
               int32_t *__restrict__ bucket, int32_t *__restrict__ label, unsigned long long *__restrict__ n_bad) {
    const int f = mesh_gid();
    bool bad = false;
    if (f < n_faces) {
        int v[3];
        int b = -1;
        if (face_ok(faces, n_verts, f, v)) {
            float P[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) P[k][a] = verts[(int64_t)v[k] * 3 + a];
            const float ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
            const float bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
            const float mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;
            const float score[6] = {mx, -mx, my, -my, mz, -mz};
            b = 0;
            float best = score[0];
#pragma unroll
            for (int k = 1; k < 6; ++k)
                if (score[k] > best) {          // the first maximum wins; a NaN never does
                    best = score[k];
                    b = k;
                }
        } else {
            bad = true;
        }
        bucket[f] = b;
        label[f] = f;
    }
    count_bad(bad, n_bad);
}

// Labels only ever decrease and always name a face of the same component, so a plain read that misses another
// workgroup's atomicMin of the same launch sees an older valid label: it costs at most a round, never the result.  A
// launch in which no lane raises `changed` wrote nothing, so all it read was the settled state.
__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_hook(const int32_t *__restrict__ bucket, const int32_t *__restrict__ twin, int n_faces, int32_t *label,
             int32_t *__restrict__ changed) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    const int b = bucket[f];
    const int lf = label[f];
    if (b < 0 || lf < 0 || lf >= n_faces) return;
    int m = lf;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int t = twin[(int64_t)f * 3 + k];
        if (t < 0 || t / 3 >= n_faces) continue;
        const int g = t / 3;
        if (bucket[g] != b) continue;
        const int lg = label[g];
        if (lg >= 0 && lg < m) m = lg;
    }
    if (m < lf) {
        atomicMin(&label[lf], m);
        atomicMin(&label[f], m);
        *changed = 1;
    }
}

__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_roots(const int32_t *__restrict__ bucket, const int32_t *__restrict__ label, int n_faces,
              int32_t *__restrict__ root_rank, int64_t *__restrict__ blk_roots) {
    const int f = mesh_gid();
    const int n[1] = {(f < n_faces && bucket[f] >= 0 && label[f] == f) ? 1 : 0};
    int excl[1], total[1];
    block_exclusive_scan<MESH_THREADS>(n, excl, total);
    if (f < n_faces) root_rank[f] = excl[0];
    if (threadIdx.x == 0) blk_roots[blockIdx.x] = total[0];
}

__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_assign(const int32_t *__restrict__ bucket, const int32_t *__restrict__ label, int n_faces,
               const int32_t *__restrict__ root_rank, const int64_t *__restrict__ blk_roots,
               int32_t *__restrict__ face_chart, int32_t *__restrict__ chart_axis) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    const int b = bucket[f], l = label[f];
    int c = -1;
    if (b >= 0 && l >= 0 && l < n_faces) {
        c = root_number(blk_roots, root_rank, l);
        if (l == f) chart_axis[c] = b;
    }
    face_chart[f] = c;
}

// enc: [4][n_charts] u32 = p_lo, p_hi, q_lo, q_hi (lo cleared to ~0, hi to 0)
__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_box(const float *__restrict__ verts, int n_verts, const int32_t *__restrict__ faces,
            const int32_t *__restrict__ bucket, const int32_t *__restrict__ face_chart, int n_faces, int n_charts,
            uint32_t *enc) {
    const int f = mesh_gid();
    if (f >= n_faces) return;
    const int b = bucket[f], c = face_chart[f];
    int v[3];
    if (b < 0 || b > 5 || c < 0 || c >= n_charts || !face_ok(faces, n_verts, f, v)) return;
    uint32_t plo = 0xFFFFFFFFu, phi = 0u, qlo = 0xFFFFFFFFu, qhi = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float p, q;
        atlas_plane(b, verts[(int64_t)v[k] * 3], verts[(int64_t)v[k] * 3 + 1], verts[(int64_t)v[k] * 3 + 2], p, q);
        const uint32_t ep = ordered_encode(p), eq = ordered_encode(q);
        plo = min(plo, ep); phi = max(phi, ep);
        qlo = min(qlo, eq); qhi = max(qhi, eq);
    }
    atomicMin(&enc[c], plo);
    atomicMax(&enc[(int64_t)n_charts + c], phi);
    atomicMin(&enc[(int64_t)2 * n_charts + c], qlo);
    atomicMax(&enc[(int64_t)3 * n_charts + c], qhi);
}

struct AtlasUv {
    const float *verts;
    const int32_t *faces, *ft, *face_chart, *chart_axis, *chart_org;
    const float *chart_box;
    int n_verts, n_faces, n_charts, n_vt, pad;
    float scale, Rf;
};

__global__ void __launch_bounds__(MESH_THREADS)
k_atlas_uv(AtlasUv a, float *__restrict__ vt) {
    const int f = mesh_gid();
    if (f >= a.n_faces) return;
    const int c = a.face_chart[f];
    int v[3];
    if (c < 0 || c >= a.n_charts || !face_ok(a.faces, a.n_verts, f, v)) return;
    const int b = a.chart_axis[c];
    if (b < 0 || b > 5) return;
    const float p_lo = a.chart_box[(int64_t)c * 4], q_hi = a.chart_box[(int64_t)c * 4 + 3];
    const float x0 = (float)(a.chart_org[(int64_t)c * 2] + a.pad) + 0.5f;
    const float y0 = (float)(a.chart_org[(int64_t)c * 2 + 1] + a.pad) + 0.5f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int t = a.ft[(int64_t)f * 3 + k];
        if (t < 0 || t >= a.n_vt) continue;
        float p, q;
        atlas_plane(b, a.verts[(int64_t)v[k] * 3], a.verts[(int64_t)v[k] * 3 + 1], a.verts[(int64_t)v[k] * 3 + 2], p, q);
        const float X = x0 + (p - p_lo) * a.scale;
        const float Y = y0 + (q_hi - q) * a.scale;
        vt[(int64_t)t * 2] = X / a.Rf;
        vt[(int64_t)t * 2 + 1] = 1.0f - Y / a.Rf;
    }
}

__device__ __forceinline__ bool fold_indices_ok(const UvMesh &m, int f) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int t = m.ft[(int64_t)f * 3 + k];
        ok = ok && t >= 0 && t < m.n_vt;
    }
    return ok;
}

__global__ void __launch_bounds__(UV_THREADS)
k_fold_setup(UvMesh m, int64_t *__restrict__ face_off, int64_t *__restrict__ blk_items) {
    const int f = blockIdx.x * UV_THREADS + threadIdx.x;
    long long items = 0;
    if (f < m.n_faces && fold_indices_ok(m, f)) {
        UvTri t;
        uv_tri(m, f, t);
        items = (long long)t.w * t.h;
    }
    const long long n[1] = {items};
    long long excl[1], total[1];
    block_exclusive_scan<UV_THREADS>(n, excl, total);
    if (f < m.n_faces) face_off[f] = excl[0];
    if (threadIdx.x == 0) blk_items[blockIdx.x] = total[0];
}

// items [base, base + n) of the item list; lanes past the device total (counts[0]) do nothing.
// EVICT = false: pass A (owner = largest strictly covering face); true: pass B (the losers)
template <bool EVICT>
__global__ void __launch_bounds__(UV_THREADS)
k_fold_pass(UvMesh m, const int64_t *__restrict__ face_off, const int64_t *__restrict__ blk_items, int64_t nb,
            const int64_t *__restrict__ counts, int64_t base, int64_t n, int32_t *owner, int32_t *__restrict__ evicted) {
    const int64_t t = base + (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    if (t >= base + n || t >= counts[0]) return;
    int r;
    const int f = uv_item_face(face_off, blk_items, nb, m.n_faces, t, r);
    UvTri tri;
    uv_tri(m, f, tri);
    const int di = r / tri.w;
    const int i = tri.i0 + di, j = tri.j0 + (r - di * tri.w);
    if (!uv_cover_strict(tri, i, j)) return;
    if (!EVICT) atomicMax(&owner[(int64_t)i * m.R + j], f);
    else if (owner[(int64_t)i * m.R + j] != f) evicted[f] = 1;
}

struct FoldLayout {
    int64_t nbF;
    size_t face_off, blk_items, bytes;
};

static FoldLayout fold_layout(int n_faces) {
    FoldLayout L;
    Carve c;
    L.nbF = div_up(n_faces, UV_THREADS);
    L.face_off = c.take((size_t)n_faces * 8);
    L.blk_items = c.take((size_t)L.nbF * 8);
    L.bytes = c.o;
    return L;
}

struct CompactLayout {
    int64_t nb;
    size_t root_rank, blk_roots, bytes;
};

static CompactLayout compact_layout(int n_faces) {
    CompactLayout L;
    Carve c;
    L.nb = div_up(n_faces, MESH_THREADS);
    L.root_rank = c.take((size_t)n_faces * 4);
    L.blk_roots = c.take((size_t)L.nb * 8);
    L.bytes = c.o;
    return L;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_atlas_buckets(const float *verts, int n_verts, const int32_t *faces, int n_faces, int32_t *bucket,
                        int32_t *label, int64_t *counts_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES && n_verts >= 0,
                  "atlas_buckets: %d faces / %d vertices outside [0, %d] / >= 0", n_faces, n_verts, LNERF_ATLAS_MAX_FACES);
    LNERF_REQUIRE(counts_dev, "atlas_buckets: null counts");
    LNERF_REQUIRE(n_faces == 0 || (verts && faces && bucket && label), "atlas_buckets: null pointer");
    hipStream_t s = as_stream(stream);
    if (!hip_ok(hipMemsetAsync(counts_dev, 0, 8, s), "atlas_buckets: clearing the count")) return LNERF_ERR_HIP;
    if (n_faces > 0) {
        MESH_LAUNCH(k_atlas_bucket, n_faces, verts, n_verts, faces, n_faces, bucket, label,
                    reinterpret_cast<unsigned long long *>(counts_dev));
        LNERF_CHECK_LAUNCH("atlas_buckets");
    }
    return LNERF_OK;
}

int lnerf_atlas_round(const int32_t *bucket, const int32_t *twin, int n_faces, int32_t *label, int32_t *changed_dev,
                      lnerf_stream_t stream) {
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES, "atlas_round: %d faces outside [0, %d]", n_faces,
                  LNERF_ATLAS_MAX_FACES);
    LNERF_REQUIRE(changed_dev, "atlas_round: null flag");
    LNERF_REQUIRE(n_faces == 0 || (bucket && twin && label), "atlas_round: null pointer");
    hipStream_t s = as_stream(stream);
    if (!hip_ok(hipMemsetAsync(changed_dev, 0, 4, s), "atlas_round: clearing the flag")) return LNERF_ERR_HIP;
    if (n_faces > 0) {
        MESH_LAUNCH(k_atlas_hook, n_faces, bucket, twin, n_faces, label, changed_dev);
        LNERF_CHECK_LAUNCH("atlas_round(hook)");
        MESH_LAUNCH(k_label_jump, n_faces, n_faces, label);
        LNERF_CHECK_LAUNCH("atlas_round(jump)");
    }
    return LNERF_OK;
}

size_t lnerf_atlas_compact_scratch_bytes(int n_faces) {
    if (n_faces < 0 || n_faces > LNERF_ATLAS_MAX_FACES) return 0;
    return compact_layout(n_faces).bytes;
}

int lnerf_atlas_compact(const int32_t *bucket, const int32_t *label, int n_faces, void *scratch, size_t scratch_bytes,
                        int32_t *face_chart, int32_t *chart_axis, int64_t *counts_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES, "atlas_compact: %d faces outside [0, %d]", n_faces,
                  LNERF_ATLAS_MAX_FACES);
    LNERF_REQUIRE(scratch && counts_dev, "atlas_compact: null pointer");
    LNERF_REQUIRE(n_faces == 0 || (bucket && label && face_chart && chart_axis), "atlas_compact: null pointer");
    const CompactLayout L = compact_layout(n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "atlas_compact: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "atlas_compact: scratch must be 16-byte aligned");
    int32_t *root_rank = at<int32_t>(scratch, L.root_rank);
    int64_t *blk_roots = at<int64_t>(scratch, L.blk_roots);
    hipStream_t s = as_stream(stream);
    if (n_faces > 0) {
        MESH_LAUNCH(k_atlas_roots, n_faces, bucket, label, n_faces, root_rank, blk_roots);
        LNERF_CHECK_LAUNCH("atlas_compact(roots)");
    }
    scan_top(blk_roots, nullptr, L.nb, counts_dev, nullptr, s);
    LNERF_CHECK_LAUNCH("atlas_compact(scan)");
    if (n_faces > 0) {
        MESH_LAUNCH(k_atlas_assign, n_faces, bucket, label, n_faces, root_rank, blk_roots, face_chart, chart_axis);
        LNERF_CHECK_LAUNCH("atlas_compact(assign)");
    }
    return LNERF_OK;
}

size_t lnerf_atlas_boxes_scratch_bytes(int n_charts) {
    if (n_charts < 0 || n_charts > LNERF_ATLAS_MAX_FACES) return 0;
    return align256((size_t)n_charts * 16);
}

int lnerf_atlas_boxes(const float *verts, int n_verts, const int32_t *faces, const int32_t *bucket,
                      const int32_t *face_chart, int n_faces, int n_charts, void *scratch, size_t scratch_bytes,
                      float *chart_box, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES && n_verts >= 0 && n_charts >= 0 &&
                  n_charts <= LNERF_ATLAS_MAX_FACES, "atlas_boxes: %d faces / %d vertices / %d charts out of range",
                  n_faces, n_verts, n_charts);
    LNERF_REQUIRE(n_faces == 0 || (verts && faces && bucket && face_chart), "atlas_boxes: null mesh pointer");
    LNERF_REQUIRE(n_charts == 0 || (scratch && chart_box), "atlas_boxes: null pointer");
    const size_t need = align256((size_t)n_charts * 16);
    LNERF_REQUIRE(scratch_bytes >= need, "atlas_boxes: scratch of %zu bytes, need %zu", scratch_bytes, need);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "atlas_boxes: scratch must be 16-byte aligned");
    if (n_charts == 0) return LNERF_OK;
    hipStream_t s = as_stream(stream);
    uint32_t *enc = reinterpret_cast<uint32_t *>(scratch);
    for (int k = 0; k < 4; k += 2)      // p_lo, p_hi, then q_lo, q_hi
        if (!box_clear(enc + (size_t)k * n_charts, enc + (size_t)(k + 1) * n_charts, n_charts, s,
                       "atlas_boxes: clearing the boxes"))
            return LNERF_ERR_HIP;
    if (n_faces > 0) {
        MESH_LAUNCH(k_atlas_box, n_faces, verts, n_verts, faces, bucket, face_chart, n_faces, n_charts, enc);
        LNERF_CHECK_LAUNCH("atlas_boxes(box)");
    }
    MESH_LAUNCH(k_box_decode<4>, n_charts, enc, n_charts, (const int64_t *)nullptr, chart_box);
    LNERF_CHECK_LAUNCH("atlas_boxes(unbox)");
    return LNERF_OK;
}

int lnerf_atlas_uv(const float *verts, int n_verts, const int32_t *faces, const int32_t *ft, int n_faces,
                   const int32_t *face_chart, const int32_t *chart_axis, const int32_t *chart_org, const float *chart_box,
                   int n_charts, int pad, float scale, int R, float *vt, int n_vt, lnerf_stream_t stream) {
    LNERF_REQUIRE(R >= 1 && R <= LNERF_UV_MAX_RES, "atlas_uv: resolution %d outside [1, %d]", R, LNERF_UV_MAX_RES);
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES && n_verts >= 0 && n_charts >= 0 && n_vt >= 0,
                  "atlas_uv: %d faces / %d vertices / %d charts / %d texture vertices out of range", n_faces, n_verts,
                  n_charts, n_vt);
    LNERF_REQUIRE(pad >= 0 && pad <= R, "atlas_uv: pad %d outside [0, %d]", pad, R);
    LNERF_REQUIRE(scale >= 0.f && scale <= 3.402823466e38f, "atlas_uv: the scale must be finite and >= 0");
    LNERF_REQUIRE(n_faces == 0 || (verts && faces && ft && face_chart && chart_axis && chart_org && chart_box && vt),
                  "atlas_uv: null pointer");
    if (n_faces == 0) return LNERF_OK;
    AtlasUv a;
    a.verts = verts; a.faces = faces; a.ft = ft; a.face_chart = face_chart; a.chart_axis = chart_axis;
    a.chart_org = chart_org; a.chart_box = chart_box;
    a.n_verts = n_verts; a.n_faces = n_faces; a.n_charts = n_charts; a.n_vt = n_vt; a.pad = pad;
    a.scale = scale; a.Rf = (float)R;
    hipStream_t s = as_stream(stream);
    MESH_LAUNCH(k_atlas_uv, n_faces, a, vt);
    LNERF_CHECK_LAUNCH("atlas_uv");
    return LNERF_OK;
}

size_t lnerf_atlas_fold_scratch_bytes(int n_faces, int R) {
    if (n_faces < 0 || n_faces > LNERF_ATLAS_MAX_FACES || R < 1 || R > LNERF_UV_MAX_RES) return 0;
    return fold_layout(n_faces).bytes;
}

int lnerf_atlas_fold(const float *vt, int n_vt, const int32_t *ft, int n_faces, int R, int stages, int64_t n_items,
                     void *scratch, size_t scratch_bytes, int32_t *texel_owner, int32_t *evicted, int64_t *counts_dev,
                     lnerf_stream_t stream) {
    LNERF_REQUIRE(R >= 1 && R <= LNERF_UV_MAX_RES, "atlas_fold: resolution %d outside [1, %d]", R, LNERF_UV_MAX_RES);
    LNERF_REQUIRE(n_faces >= 0 && n_faces <= LNERF_ATLAS_MAX_FACES && n_vt >= 0,
                  "atlas_fold: %d faces / %d texture vertices out of range", n_faces, n_vt);
    LNERF_REQUIRE((stages & ~(LNERF_UV_ITEMS | LNERF_UV_COVER)) == 0 && stages != 0, "atlas_fold: bad stage bits 0x%x",
                  stages);
    LNERF_REQUIRE(scratch && counts_dev, "atlas_fold: null pointer");
    LNERF_REQUIRE(n_faces == 0 || (vt && ft), "atlas_fold: null atlas pointer");
    LNERF_REQUIRE(!(stages & LNERF_UV_COVER) || (texel_owner && (n_faces == 0 || evicted) && n_items >= 0),
                  "atlas_fold: null output or negative item count");
    const FoldLayout L = fold_layout(n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "atlas_fold: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "atlas_fold: scratch must be 16-byte aligned");
    UvMesh m;
    m.verts = nullptr; m.faces = nullptr; m.vt = vt; m.ft = ft;
    m.n_verts = 0; m.n_vt = n_vt; m.n_faces = n_faces; m.R = R;
    m.Rf = (float)R;
    int64_t *face_off = at<int64_t>(scratch, L.face_off), *blk_items = at<int64_t>(scratch, L.blk_items);
    hipStream_t s = as_stream(stream);
    if (stages & LNERF_UV_ITEMS) {
        if (n_faces > 0) {
            LNERF_LAUNCH(k_fold_setup, n_faces, UV_THREADS, s, m, face_off, blk_items);
            LNERF_CHECK_LAUNCH("atlas_fold(setup)");
        }
        scan_top(blk_items, nullptr, L.nbF, counts_dev, nullptr, s);
        LNERF_CHECK_LAUNCH("atlas_fold(scan)");
    }
    if (stages & LNERF_UV_COVER) {
        if (!hip_ok(hipMemsetAsync(texel_owner, 0xff, (size_t)R * R * 4, s), "atlas_fold: clearing texel_owner") ||
            (n_faces > 0 && !hip_ok(hipMemsetAsync(evicted, 0, (size_t)n_faces * 4, s), "atlas_fold: clearing evicted")))
            return LNERF_ERR_HIP;
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t base = 0; base < n_items; base += UV_ITEMS_PER_LAUNCH) {
                const int64_t n = min(n_items - base, UV_ITEMS_PER_LAUNCH);
                LNERF_LAUNCH(pass == 0 ? k_fold_pass<false> : k_fold_pass<true>, n, UV_THREADS, s, m, face_off, blk_items,
                             L.nbF, counts_dev, base, n, texel_owner, evicted);
                LNERF_CHECK_LAUNCH("atlas_fold(pass)");
            }
    }
    return LNERF_OK;
}

}  // extern "C"
