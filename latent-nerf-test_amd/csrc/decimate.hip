// Mesh decimation by rounds of independent quadric-error edge collapses: NeRFRenderer.export_mesh's `target_faces`.
// Contract: include/lnerf_hip.h, lnerf_decimate; numpy restatement: tests/decimate_reference.py.
//
// Launches (one lane per face, half-edge or vertex; the only atomics are order-independent: counts and a 64-bit min):
//   setup      k_dc_check    index range and repeated indices of the input faces -> keep flags, bad-face count
//              (scan)        compaction of the kept faces (k_dc_compact_faces)
//   lists      vertex_face_lists (mesh_shared.h)   vertex -> face lists, each sorted ascending
//   quadrics   k_dc_quadric  per vertex, its faces' plane quadrics in ascending face order (f64)
//   round      k_dc_status   locked flag, K1 = none, remap = identity
//              k_dc_eval     per half-edge: validity, v*, cost, key; atomic min of the key into K1 of both ends
//              k_dc_face_key, k_dc_k2, k_dc_select, (scan), k_dc_gather   the selected edges in edge order
//              -- host read of the selected count --
//              k_dc_rank     (only in the round that would pass the target) keep the m smallest keys
//              k_dc_apply, k_dc_remap, (scan), k_dc_compact_faces, lists of the new faces
//   output     k_vf_count, k_dc_used, (scan), k_dc_out_verts, k_dc_out_faces, lists, k_vertex_normals (mesh_shared.h),
//              k_dc_counts
// scan = scan_flat (scan.h): exclusive int32 prefix with the total at [n].
#include <algorithm>
#include <utility>

#include "common.h"
#include "mesh_shared.h"
#include "scan.h"

namespace lnerf {

constexpr unsigned long long DC_NONE = ~0ull;

// ---------------------------------------------------------------- faces
__global__ void __launch_bounds__(MESH_THREADS)
k_dc_check(const int32_t *__restrict__ faces, int F, int V, int32_t *__restrict__ keep,
           unsigned long long *__restrict__ n_bad) {
    const int f = mesh_gid();
    bool bad = false;
    if (f < F) {
        int v[3];
        bad = !face_ok(faces, V, f, v);
        keep[f] = !bad && !face_repeats(v[0], v[1], v[2]) ? 1 : 0;
    }
    count_bad(bad, n_bad);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_compact_faces(const int32_t *__restrict__ src, int F, const int32_t *__restrict__ keep,
                   const int32_t *__restrict__ at, int32_t *__restrict__ dst) {
    const int f = mesh_gid();
    if (f >= F || !keep[f]) return;
    const int64_t o = (int64_t)at[f] * 3;
    dst[o] = src[(int64_t)f * 3];
    dst[o + 1] = src[(int64_t)f * 3 + 1];
    dst[o + 2] = src[(int64_t)f * 3 + 2];
}

// ---------------------------------------------------------------- quadrics: a00 a01 a02 a11 a12 a22 b0 b1 b2 c
__device__ __forceinline__ void dc_face_quadric(const float *__restrict__ pos, const int32_t *__restrict__ faces, int f,
                                                double q[10]) {
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t v = faces[(int64_t)f * 3 + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = (double)pos[v * 3 + a];
    }
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
    const double l = sqrt(mx * mx + my * my + mz * mz);
    if (l == 0.0) {
#pragma unroll
        for (int i = 0; i < 10; ++i) q[i] = 0.0;
        return;
    }
    const double n0 = mx / l, n1 = my / l, n2 = mz / l;
    const double d = -(n0 * p[0][0] + n1 * p[0][1] + n2 * p[0][2]);
    const double w = l * 0.5;
    q[0] = w * (n0 * n0); q[1] = w * (n0 * n1); q[2] = w * (n0 * n2);
    q[3] = w * (n1 * n1); q[4] = w * (n1 * n2); q[5] = w * (n2 * n2);
    q[6] = w * (n0 * d); q[7] = w * (n1 * d); q[8] = w * (n2 * d); q[9] = w * (d * d);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_quadric(const float *__restrict__ pos, const int32_t *__restrict__ faces, const int32_t *__restrict__ off,
             const int32_t *__restrict__ list, int V, double *__restrict__ Q) {
    const int w = mesh_gid();
    if (w >= V) return;
    double acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.0;
    for (int s = off[w]; s < off[w + 1]; ++s) {
        double q[10];
        dc_face_quadric(pos, faces, list[s], q);
#pragma unroll
        for (int i = 0; i < 10; ++i) acc[i] = acc[i] + q[i];
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) Q[(int64_t)w * 10 + i] = acc[i];
}

// ---------------------------------------------------------------- a round
__global__ void __launch_bounds__(MESH_THREADS)
k_dc_status(const int32_t *__restrict__ faces, const int32_t *__restrict__ off, const int32_t *__restrict__ list, int V,
            int32_t *__restrict__ locked, unsigned long long *__restrict__ K1, int32_t *__restrict__ remap) {
    const int w = mesh_gid();
    if (w >= V) return;
    K1[w] = DC_NONE;
    remap[w] = w;
    const int b = off[w], deg = off[w + 1] - b;
    bool lock = deg == 0;
    // every neighbour must follow w in exactly one face and precede it in exactly one
    for (int k = 0; k < deg && !lock; ++k) {
        int nk, pk;
        face_corner(faces, list[b + k], w, nk, pk);
        int nn = 0, pn = 0, np = 0, pp = 0;
        for (int j = 0; j < deg; ++j) {
            int nj, pj;
            face_corner(faces, list[b + j], w, nj, pj);
            nn += nj == nk; pn += pj == nk; np += nj == pk; pp += pj == pk;
        }
        lock = nn != 1 || pn != 1 || np != 1 || pp != 1;
    }
    if (!lock) {   // one closed fan: from the first face, the next is the one whose prv is this one's nxt
        int cur = 0, len = 0;
        for (int s = 1; s <= deg; ++s) {
            int nc, pc;
            face_corner(faces, list[b + cur], w, nc, pc);
            int j = 0;
            for (; j < deg - 1; ++j) {   // (there is one: every nxt is exactly one face's prv)
                int nj, pj;
                face_corner(faces, list[b + j], w, nj, pj);
                if (pj == nc) break;
            }
            cur = j;
            if (cur == 0) { len = s; break; }
        }
        lock = len != deg;
    }
    locked[w] = lock ? 1 : 0;
}

__device__ __forceinline__ double dc_cost(const double q[10], double x0, double x1, double x2) {
    const double t0 = q[0] * x0 + q[1] * x1 + q[2] * x2 + q[6];
    const double t1 = q[1] * x0 + q[3] * x1 + q[4] * x2 + q[7];
    const double t2 = q[2] * x0 + q[4] * x1 + q[5] * x2 + q[8];
    return (t0 * x0 + t1 * x1 + t2 * x2) + (q[6] * x0 + q[7] * x1 + q[8] * x2) + q[9];
}

__device__ __forceinline__ uint32_t dc_tag(uint32_t x) {
    x *= 0x9E3779B1u;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    return x;
}

// does face f (unless it holds both u and v) flip, or gain area from zero, when u and v move to x?
__device__ __forceinline__ bool dc_face_blocks(const float *__restrict__ pos, const int32_t *__restrict__ faces, int f,
                                               int u, int v, const float x[3]) {
    double P[3][3], N[3][3];
    bool hu = false, hv = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = faces[(int64_t)f * 3 + k];
        hu |= c == u;
        hv |= c == v;
        const bool moved = c == u || c == v;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[k][a] = (double)pos[(int64_t)c * 3 + a];
            N[k][a] = moved ? (double)x[a] : P[k][a];
        }
    }
    if (hu && hv) return false;   // one of the edge's two faces
    double m[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double(*p)[3] = s ? N : P;
        const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        m[s][0] = e1y * e2z - e1z * e2y;
        m[s][1] = e1z * e2x - e1x * e2z;
        m[s][2] = e1x * e2y - e1y * e2x;
    }
    const bool nz0 = m[0][0] != 0.0 || m[0][1] != 0.0 || m[0][2] != 0.0;
    const bool nz1 = m[1][0] != 0.0 || m[1][1] != 0.0 || m[1][2] != 0.0;
    if (!nz0) return nz1;
    return !(m[0][0] * m[1][0] + m[0][1] * m[1][1] + m[0][2] * m[1][2] > 0.0);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_eval(const float *__restrict__ pos, const int32_t *__restrict__ faces, int F, const double *__restrict__ Q,
          const int32_t *__restrict__ off, const int32_t *__restrict__ list, const int32_t *__restrict__ locked,
          float max_error, unsigned long long *__restrict__ keys, float *__restrict__ vstar,
          unsigned long long *__restrict__ K1) {
    const int e = mesh_gid();
    if (e >= 3 * F) return;
    const int f = e / 3, k = e - 3 * f;
    const int u = faces[e], v = faces[(int64_t)f * 3 + (k == 2 ? 0 : k + 1)];
    keys[e] = DC_NONE;
    if (u >= v || locked[u] || locked[v]) return;
    const int bu = off[u], du = off[u + 1] - bu, bv = off[v], dv = off[v + 1] - bv;
    if (du == 3 && dv == 3) return;
    // link condition: exactly the two opposite vertices are common neighbours
    int common = 0;
    for (int i = 0; i < du; ++i) {
        int ni, pi;
        face_corner(faces, list[bu + i], u, ni, pi);
        for (int j = 0; j < dv; ++j) {
            int nj, pj;
            face_corner(faces, list[bv + j], v, nj, pj);
            common += nj == ni;
        }
    }
    if (common != 2) return;
    double q[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = Q[(int64_t)u * 10 + i] + Q[(int64_t)v * 10 + i];
    const double c00 = q[3] * q[5] - q[4] * q[4];
    const double c01 = q[2] * q[4] - q[1] * q[5];
    const double c02 = q[1] * q[4] - q[2] * q[3];
    const double c11 = q[0] * q[5] - q[2] * q[2];
    const double c12 = q[1] * q[2] - q[0] * q[4];
    const double c22 = q[0] * q[3] - q[1] * q[1];
    const double det = q[0] * c00 + q[1] * c01 + q[2] * c02;
    const double tr = q[0] + q[3] + q[5];
    float x[3];
    x[0] = (float)(-(c00 * q[6] + c01 * q[7] + c02 * q[8]) / det);
    x[1] = (float)(-(c01 * q[6] + c11 * q[7] + c12 * q[8]) / det);
    x[2] = (float)(-(c02 * q[6] + c12 * q[7] + c22 * q[8]) / det);
    double cost;
    if (fabs(det) > LNERF_DECIMATE_SINGULAR_REL * (tr * tr * tr) && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
        cost = dc_cost(q, (double)x[0], (double)x[1], (double)x[2]);
    } else {   // the cheapest of u, v, the midpoint (earlier wins a tie)
        float pu[3], pv[3], pm[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pu[a] = pos[(int64_t)u * 3 + a];
            pv[a] = pos[(int64_t)v * 3 + a];
            pm[a] = (pu[a] + pv[a]) * 0.5f;
            x[a] = pu[a];
        }
        cost = dc_cost(q, (double)pu[0], (double)pu[1], (double)pu[2]);
        const double cv = dc_cost(q, (double)pv[0], (double)pv[1], (double)pv[2]);
        if (cv < cost) { cost = cv; x[0] = pv[0]; x[1] = pv[1]; x[2] = pv[2]; }
        const double cm = dc_cost(q, (double)pm[0], (double)pm[1], (double)pm[2]);
        if (cm < cost) { cost = cm; x[0] = pm[0]; x[1] = pm[1]; x[2] = pm[2]; }
    }
    if (!isfinite(cost)) return;
    if (!(cost > 0.0)) cost = 0.0;     // (-0.0 and below -> +0.0: the key's high word sorts like the value)
    const float cf = (float)cost;
    if (cf > max_error) return;
    for (int i = 0; i < du; ++i)
        if (dc_face_blocks(pos, faces, list[bu + i], u, v, x)) return;
    for (int j = 0; j < dv; ++j)
        if (dc_face_blocks(pos, faces, list[bv + j], u, v, x)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(cf) << 32) | dc_tag((uint32_t)e);
    keys[e] = key;
    vstar[(int64_t)e * 3] = x[0];
    vstar[(int64_t)e * 3 + 1] = x[1];
    vstar[(int64_t)e * 3 + 2] = x[2];
    atomicMin(&K1[u], key);
    atomicMin(&K1[v], key);
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_face_key(const int32_t *__restrict__ faces, int F, const unsigned long long *__restrict__ K1,
              unsigned long long *__restrict__ FK) {
    const int f = mesh_gid();
    if (f >= F) return;
    const unsigned long long a = K1[faces[(int64_t)f * 3]], b = K1[faces[(int64_t)f * 3 + 1]],
                             c = K1[faces[(int64_t)f * 3 + 2]];
    FK[f] = min(a, min(b, c));
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_k2(const int32_t *__restrict__ off, const int32_t *__restrict__ list, int V,
        const unsigned long long *__restrict__ FK, unsigned long long *__restrict__ K2) {
    const int w = mesh_gid();
    if (w >= V) return;
    unsigned long long m = DC_NONE;
    for (int s = off[w]; s < off[w + 1]; ++s) m = min(m, FK[list[s]]);
    K2[w] = m;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_select(const int32_t *__restrict__ faces, int F, const unsigned long long *__restrict__ keys,
            const unsigned long long *__restrict__ K2, int32_t *__restrict__ flag) {
    const int e = mesh_gid();
    if (e >= 3 * F) return;
    const unsigned long long key = keys[e];
    bool s = false;
    if (key != DC_NONE) {
        const int f = e / 3, k = e - 3 * f;
        const int u = faces[e], v = faces[(int64_t)f * 3 + (k == 2 ? 0 : k + 1)];
        s = K2[u] == key && K2[v] == key;
    }
    flag[e] = s ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_gather(const int32_t *__restrict__ flag, const int32_t *__restrict__ at, int n, int cap,
            int32_t *__restrict__ sel) {
    const int e = mesh_gid();
    if (e < n && flag[e] && at[e] < cap) sel[at[e]] = e;
}

// keep[i] = 1 iff the key of selected edge i is among the m smallest (keys are distinct)
__global__ void __launch_bounds__(MESH_THREADS)
k_dc_rank(const int32_t *__restrict__ sel, int S, int m, const unsigned long long *__restrict__ keys,
          int32_t *__restrict__ keep) {
    __shared__ unsigned long long s_k[MESH_THREADS];
    const int i = mesh_gid();
    const unsigned long long mine = i < S ? keys[sel[i]] : DC_NONE;
    int rank = 0;
    for (int t = 0; t < S; t += MESH_THREADS) {
        __syncthreads();
        s_k[threadIdx.x] = t + (int)threadIdx.x < S ? keys[sel[t + threadIdx.x]] : DC_NONE;
        __syncthreads();
        const int n = min(MESH_THREADS, S - t);
        for (int j = 0; j < n; ++j) rank += s_k[j] < mine;
    }
    if (i < S) keep[i] = rank < m ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_apply(const int32_t *__restrict__ faces, const int32_t *__restrict__ sel, int S, const int32_t *__restrict__ keep,
           const float *__restrict__ vstar, float *__restrict__ pos, double *__restrict__ Q,
           int32_t *__restrict__ remap) {
    const int i = mesh_gid();
    if (i >= S || (keep && !keep[i])) return;
    const int e = sel[i];
    const int f = e / 3, k = e - 3 * f;
    const int u = faces[e], v = faces[(int64_t)f * 3 + (k == 2 ? 0 : k + 1)];
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[(int64_t)u * 3 + a] = vstar[(int64_t)e * 3 + a];
#pragma unroll
    for (int j = 0; j < 10; ++j) Q[(int64_t)u * 10 + j] = Q[(int64_t)u * 10 + j] + Q[(int64_t)v * 10 + j];
    remap[v] = u;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_remap(int32_t *__restrict__ faces, int F, const int32_t *__restrict__ remap, int32_t *__restrict__ keep) {
    const int f = mesh_gid();
    if (f >= F) return;
    const int a = remap[faces[(int64_t)f * 3]], b = remap[faces[(int64_t)f * 3 + 1]], c = remap[faces[(int64_t)f * 3 + 2]];
    faces[(int64_t)f * 3] = a;
    faces[(int64_t)f * 3 + 1] = b;
    faces[(int64_t)f * 3 + 2] = c;
    keep[f] = face_repeats(a, b, c) ? 0 : 1;
}

// ---------------------------------------------------------------- output
__global__ void __launch_bounds__(MESH_THREADS)
k_dc_used(const int32_t *__restrict__ cnt, int V, int32_t *__restrict__ used) {
    const int w = mesh_gid();
    if (w < V) used[w] = cnt[w] > 0 ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_out_verts(const float *__restrict__ pos, const int32_t *__restrict__ used, const int32_t *__restrict__ at, int V,
               float *__restrict__ out) {
    const int w = mesh_gid();
    if (w >= V || !used[w]) return;
    const int64_t o = (int64_t)at[w] * 3;
    out[o] = pos[(int64_t)w * 3];
    out[o + 1] = pos[(int64_t)w * 3 + 1];
    out[o + 2] = pos[(int64_t)w * 3 + 2];
}

__global__ void __launch_bounds__(MESH_THREADS)
k_dc_out_faces(const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ at, int32_t *__restrict__ out) {
    const int i = mesh_gid();
    if (i < 3 * F) out[i] = at[faces[i]];
}

__global__ void k_dc_counts(const int32_t *__restrict__ vtot, int F, int rounds, int64_t collapses,
                            int64_t *__restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = *vtot;
        counts[1] = F;
        counts[2] = rounds;
        counts[3] = collapses;
    }
}

// ---------------------------------------------------------------- host side
struct DcLayout {
    size_t pos, Q, fa, fb, cnt, off, list, locked, remap, K1, K2, FK, keys, vstar, flag, pfx, sel, keep, blk, dev, bytes;
};

static DcLayout dc_layout(int V, int F) {
    const int64_t n = std::max(3 * (int64_t)F, (int64_t)V) + 1;     // longest scan input, plus its total
    DcLayout L;
    Carve c;
    L.pos = c.take((size_t)V * 12);
    L.Q = c.take((size_t)V * 80);
    L.fa = c.take((size_t)F * 12);
    L.fb = c.take((size_t)F * 12);
    L.cnt = c.take((size_t)V * 4);
    L.off = c.take(((size_t)V + 1) * 4);
    L.list = c.take((size_t)F * 12);
    L.locked = c.take((size_t)V * 4);
    L.remap = c.take((size_t)V * 4);
    L.K1 = c.take((size_t)V * 8);
    L.K2 = c.take((size_t)V * 8);
    L.FK = c.take((size_t)F * 8);
    L.keys = c.take((size_t)F * 24);
    L.vstar = c.take((size_t)F * 36);
    L.flag = c.take((size_t)n * 4);
    L.pfx = c.take((size_t)n * 4);
    L.sel = c.take(((size_t)F + 1) * 4);
    L.keep = c.take(((size_t)F + 1) * 4);
    L.blk = c.take(scan_flat_blk_bytes(n));
    L.dev = c.take(64);
    L.bytes = c.o;
    return L;
}

#define DC_TRY(x)                          \
    do {                                   \
        const int rc__ = (x);              \
        if (rc__ != LNERF_OK) return rc__; \
    } while (0)

}  // namespace lnerf

using namespace lnerf;

extern "C" {

size_t lnerf_decimate_scratch_bytes(int n_verts, int n_faces) {
    if (!mesh_sizes_ok(n_verts, n_faces, LNERF_DECIMATE_MAX_FACES)) return 0;
    return dc_layout(n_verts, n_faces).bytes;
}

int lnerf_decimate(const float *verts, int n_verts, const int32_t *faces, int n_faces, int target_faces, float max_error,
                   int max_rounds, void *scratch, size_t scratch_bytes, float *verts_out, int32_t *faces_out,
                   float *normals_out, int64_t *counts_dev, lnerf_stream_t stream) {
    MESH_REQUIRE_SIZES("decimate", n_verts, n_faces, LNERF_DECIMATE_MAX_FACES);
    LNERF_REQUIRE(target_faces >= 0 && max_rounds >= 0, "decimate: target_faces %d and max_rounds %d must be >= 0",
                  target_faces, max_rounds);
    LNERF_REQUIRE(max_error >= 0.f, "decimate: max_error must be >= 0 (+inf: none)");
    LNERF_REQUIRE(scratch && counts_dev && (n_verts == 0 || (verts && verts_out)) &&
                  (n_faces == 0 || (faces && faces_out)), "decimate: null pointer");
    const DcLayout L = dc_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "decimate: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "decimate: scratch must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const int V = n_verts;
    float *pos = at<float>(scratch, L.pos), *vstar = at<float>(scratch, L.vstar);
    double *Q = at<double>(scratch, L.Q);
    int32_t *fa = at<int32_t>(scratch, L.fa), *fb = at<int32_t>(scratch, L.fb);
    int32_t *off = at<int32_t>(scratch, L.off), *list = at<int32_t>(scratch, L.list), *cnt = at<int32_t>(scratch, L.cnt);
    int32_t *locked = at<int32_t>(scratch, L.locked), *remap = at<int32_t>(scratch, L.remap);
    int32_t *flag = at<int32_t>(scratch, L.flag), *pfx = at<int32_t>(scratch, L.pfx), *sel = at<int32_t>(scratch, L.sel);
    int32_t *keep = at<int32_t>(scratch, L.keep), *blk = at<int32_t>(scratch, L.blk);
    unsigned long long *K1 = at<unsigned long long>(scratch, L.K1), *K2 = at<unsigned long long>(scratch, L.K2);
    unsigned long long *FK = at<unsigned long long>(scratch, L.FK), *keys = at<unsigned long long>(scratch, L.keys);
    unsigned long long *n_bad = at<unsigned long long>(scratch, L.dev);
    const int32_t *zero = at<int32_t>(scratch, L.dev) + 2;      // (a word that stays cleared)
    // exclusive prefix of in[0, n) into pfx[0, n], pfx[n] = total
    auto scan = [&](const int32_t *in, int n) { return scan_flat(in, n, pfx, blk, s, "decimate(scan)"); };
    // vertex -> face lists of f [nf] over nv vertices: off [nv+1], list [3 nf], ascending per vertex
    auto lists = [&](const int32_t *f, int nf, int nv) {
        return vertex_face_lists(f, nf, nv, cnt, off, list, blk, s, "decimate(lists)");
    };
    auto read = [&](const int32_t *src, int32_t *dst) {
        return read_back(src, dst, s, "decimate(read-back)") ? LNERF_OK : LNERF_ERR_HIP;
    };

    // ---- input: index range first (no kernel reads through a face before this), repeated indices, compaction
    if (!hip_ok(hipMemsetAsync(n_bad, 0, 64, s), "decimate(memset)")) return LNERF_ERR_HIP;
    int F = 0;
    if (n_faces > 0) {
        MESH_LAUNCH(k_dc_check, n_faces, faces, n_faces, V, flag, n_bad);
        LNERF_CHECK_LAUNCH("decimate(check)");
        unsigned long long bad = 0;
        if (!read_back(n_bad, &bad, s, "decimate(read-back)")) return LNERF_ERR_HIP;
        LNERF_REQUIRE(bad == 0, "decimate: %d faces index outside [0, %d)", (int)bad, V);
        DC_TRY(scan(flag, n_faces));
        MESH_LAUNCH(k_dc_compact_faces, n_faces, faces, n_faces, flag, pfx, fa);
        LNERF_CHECK_LAUNCH("decimate(compact)");
        DC_TRY(read(pfx + n_faces, &F));
    }
    if (V > 0 && !hip_ok(hipMemcpyAsync(pos, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, s), "decimate(copy)"))
        return LNERF_ERR_HIP;
    DC_TRY(lists(fa, F, V));
    MESH_LAUNCH(k_dc_quadric, V, pos, fa, off, list, V, Q);
    LNERF_CHECK_LAUNCH("decimate(quadric)");

    // ---- rounds
    int rounds = 0;
    int64_t collapses = 0;
    while (rounds < max_rounds && F > target_faces) {
        const int E = 3 * F;
        MESH_LAUNCH(k_dc_status, V, fa, off, list, V, locked, K1, remap);
        MESH_LAUNCH(k_dc_eval, E, pos, fa, F, Q, off, list, locked,
                           max_error, keys, vstar, K1);
        MESH_LAUNCH(k_dc_face_key, F, fa, F, K1, FK);
        MESH_LAUNCH(k_dc_k2, V, off, list, V, FK, K2);
        MESH_LAUNCH(k_dc_select, E, fa, F, keys, K2, flag);
        LNERF_CHECK_LAUNCH("decimate(select)");
        DC_TRY(scan(flag, E));
        MESH_LAUNCH(k_dc_gather, E, flag, pfx, E, F + 1, sel);
        LNERF_CHECK_LAUNCH("decimate(gather)");
        int S = 0;
        DC_TRY(read(pfx + E, &S));
        if (S == 0) break;
        // independent collapses own disjoint face pairs, so S <= F / 2 (the gather wrote at most F + 1 entries)
        LNERF_REQUIRE(2 * (int64_t)S <= F, "decimate: internal: %d independent collapses among %d faces", S, F);
        int m = S;
        if (F - 2 * S < target_faces) {
            m = (F - target_faces + 1) / 2;
            MESH_LAUNCH(k_dc_rank, S, sel, S, m, keys, keep);
        }
        MESH_LAUNCH(k_dc_apply, S, fa, sel, S, m < S ? keep : nullptr,
                           vstar, pos, Q, remap);
        MESH_LAUNCH(k_dc_remap, F, fa, F, remap, flag);
        LNERF_CHECK_LAUNCH("decimate(apply)");
        DC_TRY(scan(flag, F));
        MESH_LAUNCH(k_dc_compact_faces, F, fa, F, flag, pfx, fb);
        LNERF_CHECK_LAUNCH("decimate(compact)");
        std::swap(fa, fb);
        F -= 2 * m;          // each collapse removes exactly its edge's two faces (link condition)
        ++rounds;
        collapses += m;
        DC_TRY(lists(fa, F, V));
    }

    // ---- output: referenced vertices in order, faces renumbered, normals
    const int32_t *vtot = zero;      // (no vertices)
    if (V > 0) {
        if (!hip_ok(hipMemsetAsync(cnt, 0, (size_t)V * 4, s), "decimate(memset)")) return LNERF_ERR_HIP;
        MESH_LAUNCH(k_vf_count, F, fa, F, cnt);
        MESH_LAUNCH(k_dc_used, V, cnt, V, flag);
        LNERF_CHECK_LAUNCH("decimate(used)");
        DC_TRY(scan(flag, V));
        MESH_LAUNCH(k_dc_out_verts, V, pos, flag, pfx, V, verts_out);
        MESH_LAUNCH(k_dc_out_faces, 3 * (int64_t)F, fa, F, pfx, faces_out);
        LNERF_CHECK_LAUNCH("decimate(output)");
        vtot = pfx + V;
    }
    LNERF_LAUNCH(k_dc_counts, 1, 64, s, vtot, F, rounds, collapses, counts_dev);
    LNERF_CHECK_LAUNCH("decimate(counts)");
    if (normals_out && V > 0) {
        int Vout = 0;
        DC_TRY(read(vtot, &Vout));
        DC_TRY(lists(faces_out, F, Vout));   // lists of the output faces over the output vertices
        MESH_LAUNCH(k_vertex_normals, Vout, verts_out, faces_out, off, list, Vout, normals_out);
        LNERF_CHECK_LAUNCH("decimate(normals)");
    }
    return LNERF_OK;
}

}  // extern "C"
