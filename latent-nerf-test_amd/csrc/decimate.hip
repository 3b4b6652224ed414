// Mesh decimation by rounds of independent quadric-error edge collapses: NeRFRenderer.export_mesh's `target_faces`.
// Contract: include/lnerf_hip.h, lnerf_decimate; numpy restatement: tests/decimate_reference.py.
//
// Launches (one lane per face, half-edge or vertex; the only atomics are order-independent: counts and a 64-bit min):
//   setup      k_dc_check    index range and repeated indices of the input faces -> keep flags, bad-face count
//              (scan)        compaction of the kept faces (k_dc_compact_faces)
//   lists      k_dc_count, (scan), k_dc_fill, k_dc_sort   vertex -> face lists, each sorted ascending
//   quadrics   k_dc_quadric  per vertex, its faces' plane quadrics in ascending face order (f64)
//   round      k_dc_status   locked flag, K1 = none, remap = identity
//              k_dc_eval     per half-edge: validity, v*, cost, key; atomic min of the key into K1 of both ends
//              k_dc_face_key, k_dc_k2, k_dc_select, (scan), k_dc_gather   the selected edges in edge order
//              -- host read of the selected count --
//              k_dc_rank     (only in the round that would pass the target) keep the m smallest keys
//              k_dc_apply, k_dc_remap, (scan), k_dc_compact_faces, lists of the new faces
//   output     k_dc_count, k_dc_used, (scan), k_dc_out_verts, k_dc_out_faces, lists, k_dc_normals, k_dc_counts
// scan = k_dc_scan_blocks, k_scan_top (scan.h, one workgroup), k_dc_scan_add: exclusive int32 prefix with the total at [n].
#include <algorithm>
#include <utility>

#include "common.h"
#include "scan.h"

namespace lnerf {

constexpr int DC_THREADS = 256;
constexpr int DC_PPT = 16;
constexpr int DC_BLOCK = DC_THREADS * DC_PPT;
constexpr unsigned long long DC_NONE = ~0ull;

__device__ __forceinline__ int dc_gid() { return blockIdx.x * DC_THREADS + threadIdx.x; }

// ---------------------------------------------------------------- exclusive scan, int32, total at out[n]
__global__ void __launch_bounds__(DC_THREADS)
k_dc_scan_blocks(const int32_t *__restrict__ in, int n, int32_t *__restrict__ out, int32_t *__restrict__ blk) {
    const int base = blockIdx.x * DC_BLOCK + threadIdx.x * DC_PPT;
    int sum[1] = {0}, run[1], tot[1];
    for (int q = 0; q < DC_PPT; ++q)
        if (base + q < n) sum[0] += in[base + q];
    block_exclusive_scan<DC_THREADS>(sum, run, tot);
    for (int q = 0; q < DC_PPT; ++q)
        if (base + q < n) {
            const int x = in[base + q];
            out[base + q] = run[0];
            run[0] += x;
        }
    if (threadIdx.x == 0) blk[blockIdx.x] = tot[0];
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_scan_add(int32_t *__restrict__ out, int n, const int32_t *__restrict__ blk, int nb) {
    const int i = dc_gid();
    if (i < n) out[i] += blk[i / DC_BLOCK];
    if (i == 0) out[n] = blk[nb];
}

// ---------------------------------------------------------------- faces and vertex -> face lists
__device__ __forceinline__ bool dc_degenerate(int a, int b, int c) { return a == b || b == c || c == a; }

__global__ void __launch_bounds__(DC_THREADS)
k_dc_check(const int32_t *__restrict__ faces, int F, int V, int32_t *__restrict__ keep, int32_t *__restrict__ bad) {
    const int f = dc_gid();
    if (f >= F) return;
    const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
    const bool in = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
    if (!in) atomicAdd(bad, 1);
    keep[f] = in && !dc_degenerate(a, b, c) ? 1 : 0;
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_compact_faces(const int32_t *__restrict__ src, int F, const int32_t *__restrict__ keep,
                   const int32_t *__restrict__ at, int32_t *__restrict__ dst) {
    const int f = dc_gid();
    if (f >= F || !keep[f]) return;
    const int64_t o = (int64_t)at[f] * 3;
    dst[o] = src[(int64_t)f * 3];
    dst[o + 1] = src[(int64_t)f * 3 + 1];
    dst[o + 2] = src[(int64_t)f * 3 + 2];
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_count(const int32_t *__restrict__ faces, int F, int32_t *__restrict__ cnt) {
    const int i = dc_gid();
    if (i < 3 * F) atomicAdd(&cnt[faces[i]], 1);
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_fill(const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ off, int32_t *__restrict__ cur,
          int32_t *__restrict__ list) {
    const int i = dc_gid();
    if (i >= 3 * F) return;
    const int w = faces[i];
    list[off[w] + atomicAdd(&cur[w], 1)] = i / 3;
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_sort(const int32_t *__restrict__ off, int V, int32_t *__restrict__ list) {
    const int w = dc_gid();
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

__global__ void __launch_bounds__(DC_THREADS)
k_dc_quadric(const float *__restrict__ pos, const int32_t *__restrict__ faces, const int32_t *__restrict__ off,
             const int32_t *__restrict__ list, int V, double *__restrict__ Q) {
    const int w = dc_gid();
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
// the vertices after / before w in face f (w must be a corner of f)
__device__ __forceinline__ void dc_corner(const int32_t *__restrict__ faces, int f, int w, int &nxt, int &prv) {
    const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
    if (a == w) { nxt = b; prv = c; }
    else if (b == w) { nxt = c; prv = a; }
    else { nxt = a; prv = b; }
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_status(const int32_t *__restrict__ faces, const int32_t *__restrict__ off, const int32_t *__restrict__ list, int V,
            int32_t *__restrict__ locked, unsigned long long *__restrict__ K1, int32_t *__restrict__ remap) {
    const int w = dc_gid();
    if (w >= V) return;
    K1[w] = DC_NONE;
    remap[w] = w;
    const int b = off[w], deg = off[w + 1] - b;
    bool lock = deg == 0;
    // every neighbour must follow w in exactly one face and precede it in exactly one
    for (int k = 0; k < deg && !lock; ++k) {
        int nk, pk;
        dc_corner(faces, list[b + k], w, nk, pk);
        int nn = 0, pn = 0, np = 0, pp = 0;
        for (int j = 0; j < deg; ++j) {
            int nj, pj;
            dc_corner(faces, list[b + j], w, nj, pj);
            nn += nj == nk; pn += pj == nk; np += nj == pk; pp += pj == pk;
        }
        lock = nn != 1 || pn != 1 || np != 1 || pp != 1;
    }
    if (!lock) {   // one closed fan: from the first face, the next is the one whose prv is this one's nxt
        int cur = 0, len = 0;
        for (int s = 1; s <= deg; ++s) {
            int nc, pc;
            dc_corner(faces, list[b + cur], w, nc, pc);
            int j = 0;
            for (; j < deg - 1; ++j) {   // (there is one: every nxt is exactly one face's prv)
                int nj, pj;
                dc_corner(faces, list[b + j], w, nj, pj);
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

__global__ void __launch_bounds__(DC_THREADS)
k_dc_eval(const float *__restrict__ pos, const int32_t *__restrict__ faces, int F, const double *__restrict__ Q,
          const int32_t *__restrict__ off, const int32_t *__restrict__ list, const int32_t *__restrict__ locked,
          float max_error, unsigned long long *__restrict__ keys, float *__restrict__ vstar,
          unsigned long long *__restrict__ K1) {
    const int e = dc_gid();
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
        dc_corner(faces, list[bu + i], u, ni, pi);
        for (int j = 0; j < dv; ++j) {
            int nj, pj;
            dc_corner(faces, list[bv + j], v, nj, pj);
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

__global__ void __launch_bounds__(DC_THREADS)
k_dc_face_key(const int32_t *__restrict__ faces, int F, const unsigned long long *__restrict__ K1,
              unsigned long long *__restrict__ FK) {
    const int f = dc_gid();
    if (f >= F) return;
    const unsigned long long a = K1[faces[(int64_t)f * 3]], b = K1[faces[(int64_t)f * 3 + 1]],
                             c = K1[faces[(int64_t)f * 3 + 2]];
    FK[f] = min(a, min(b, c));
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_k2(const int32_t *__restrict__ off, const int32_t *__restrict__ list, int V,
        const unsigned long long *__restrict__ FK, unsigned long long *__restrict__ K2) {
    const int w = dc_gid();
    if (w >= V) return;
    unsigned long long m = DC_NONE;
    for (int s = off[w]; s < off[w + 1]; ++s) m = min(m, FK[list[s]]);
    K2[w] = m;
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_select(const int32_t *__restrict__ faces, int F, const unsigned long long *__restrict__ keys,
            const unsigned long long *__restrict__ K2, int32_t *__restrict__ flag) {
    const int e = dc_gid();
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

__global__ void __launch_bounds__(DC_THREADS)
k_dc_gather(const int32_t *__restrict__ flag, const int32_t *__restrict__ at, int n, int cap,
            int32_t *__restrict__ sel) {
    const int e = dc_gid();
    if (e < n && flag[e] && at[e] < cap) sel[at[e]] = e;
}

// keep[i] = 1 iff the key of selected edge i is among the m smallest (keys are distinct)
__global__ void __launch_bounds__(DC_THREADS)
k_dc_rank(const int32_t *__restrict__ sel, int S, int m, const unsigned long long *__restrict__ keys,
          int32_t *__restrict__ keep) {
    __shared__ unsigned long long s_k[DC_THREADS];
    const int i = dc_gid();
    const unsigned long long mine = i < S ? keys[sel[i]] : DC_NONE;
    int rank = 0;
    for (int t = 0; t < S; t += DC_THREADS) {
        __syncthreads();
        s_k[threadIdx.x] = t + (int)threadIdx.x < S ? keys[sel[t + threadIdx.x]] : DC_NONE;
        __syncthreads();
        const int n = min(DC_THREADS, S - t);
        for (int j = 0; j < n; ++j) rank += s_k[j] < mine;
    }
    if (i < S) keep[i] = rank < m ? 1 : 0;
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_apply(const int32_t *__restrict__ faces, const int32_t *__restrict__ sel, int S, const int32_t *__restrict__ keep,
           const float *__restrict__ vstar, float *__restrict__ pos, double *__restrict__ Q,
           int32_t *__restrict__ remap) {
    const int i = dc_gid();
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

__global__ void __launch_bounds__(DC_THREADS)
k_dc_remap(int32_t *__restrict__ faces, int F, const int32_t *__restrict__ remap, int32_t *__restrict__ keep) {
    const int f = dc_gid();
    if (f >= F) return;
    const int a = remap[faces[(int64_t)f * 3]], b = remap[faces[(int64_t)f * 3 + 1]], c = remap[faces[(int64_t)f * 3 + 2]];
    faces[(int64_t)f * 3] = a;
    faces[(int64_t)f * 3 + 1] = b;
    faces[(int64_t)f * 3 + 2] = c;
    keep[f] = dc_degenerate(a, b, c) ? 0 : 1;
}

// ---------------------------------------------------------------- output
__global__ void __launch_bounds__(DC_THREADS)
k_dc_used(const int32_t *__restrict__ cnt, int V, int32_t *__restrict__ used) {
    const int w = dc_gid();
    if (w < V) used[w] = cnt[w] > 0 ? 1 : 0;
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_out_verts(const float *__restrict__ pos, const int32_t *__restrict__ used, const int32_t *__restrict__ at, int V,
               float *__restrict__ out) {
    const int w = dc_gid();
    if (w >= V || !used[w]) return;
    const int64_t o = (int64_t)at[w] * 3;
    out[o] = pos[(int64_t)w * 3];
    out[o + 1] = pos[(int64_t)w * 3 + 1];
    out[o + 2] = pos[(int64_t)w * 3 + 2];
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_out_faces(const int32_t *__restrict__ faces, int F, const int32_t *__restrict__ at, int32_t *__restrict__ out) {
    const int i = dc_gid();
    if (i < 3 * F) out[i] = at[faces[i]];
}

__global__ void __launch_bounds__(DC_THREADS)
k_dc_normals(const float *__restrict__ verts, const int32_t *__restrict__ faces, const int32_t *__restrict__ off,
             const int32_t *__restrict__ list, int V, float *__restrict__ normals) {
    const int w = dc_gid();
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
    size_t pos, Q, fa, fb, cnt, off, list, locked, remap, K1, K2, FK, keys, vstar, flag, at, sel, keep, blk, dev, bytes;
};

static DcLayout dc_layout(int V, int F) {
    const int64_t n = std::max(3 * (int64_t)F, (int64_t)V) + 1;     // longest scan input, plus its total
    const int64_t nb = div_up(n, DC_BLOCK) + 1;
    DcLayout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    L.pos = take((size_t)V * 12);
    L.Q = take((size_t)V * 80);
    L.fa = take((size_t)F * 12);
    L.fb = take((size_t)F * 12);
    L.cnt = take((size_t)V * 4);
    L.off = take(((size_t)V + 1) * 4);
    L.list = take((size_t)F * 12);
    L.locked = take((size_t)V * 4);
    L.remap = take((size_t)V * 4);
    L.K1 = take((size_t)V * 8);
    L.K2 = take((size_t)V * 8);
    L.FK = take((size_t)F * 8);
    L.keys = take((size_t)F * 24);
    L.vstar = take((size_t)F * 36);
    L.flag = take((size_t)n * 4);
    L.at = take((size_t)n * 4);
    L.sel = take(((size_t)F + 1) * 4);
    L.keep = take(((size_t)F + 1) * 4);
    L.blk = take((size_t)nb * 4);
    L.dev = take(64);
    L.bytes = o;
    return L;
}

struct DcRun {
    char *base;
    DcLayout L;
    hipStream_t s;
    template <class T> T *at(size_t o) const { return reinterpret_cast<T *>(base + o); }
};

static unsigned dc_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, div_up(n, DC_THREADS)); }

#define DC_TRY(x)                          \
    do {                                   \
        const int rc__ = (x);              \
        if (rc__ != LNERF_OK) return rc__; \
    } while (0)

#define DC_HIP(x, what)                                                               \
    do {                                                                              \
        const hipError_t e__ = (x);                                                   \
        if (e__ != hipSuccess) {                                                      \
            ::lnerf::set_error("decimate(%s): %s", what, hipGetErrorString(e__));     \
            return LNERF_ERR_HIP;                                                     \
        }                                                                             \
    } while (0)

// exclusive prefix of in[0, n) into out[0, n], out[n] = total
static int dc_scan(const DcRun &r, const int32_t *in, int n, int32_t *out) {
    const int nb = (int)div_up(std::max(n, 1), DC_BLOCK);
    int32_t *blk = r.at<int32_t>(r.L.blk);
    hipLaunchKernelGGL(k_dc_scan_blocks, dim3(nb), dim3(DC_THREADS), 0, r.s, in, n, out, blk);
    // (int32: more than 1024 blocks, where a thread of k_scan_top owns several entries, takes over 1.4 M faces, too many
    // for a test through the Python restatement; the int64 instantiation of the same template is tested on that side)
    hipLaunchKernelGGL(k_scan_top<int32_t>, dim3(1), dim3(SCAN_TOP_THREADS), 0, r.s, blk, (int32_t *)nullptr, (int64_t)nb,
                       blk + nb, (int32_t *)nullptr);
    hipLaunchKernelGGL(k_dc_scan_add, dim3(dc_grid(std::max(n, 1))), dim3(DC_THREADS), 0, r.s, out, n, blk, nb);
    LNERF_CHECK_LAUNCH("decimate(scan)");
    return LNERF_OK;
}

// vertex -> face lists of faces [F] over V vertices: off [V+1], list [3F], ascending per vertex
static int dc_lists(const DcRun &r, const int32_t *faces, int F, int V) {
    int32_t *cnt = r.at<int32_t>(r.L.cnt), *off = r.at<int32_t>(r.L.off), *list = r.at<int32_t>(r.L.list);
    DC_HIP(hipMemsetAsync(cnt, 0, (size_t)V * 4, r.s), "memset");
    hipLaunchKernelGGL(k_dc_count, dim3(dc_grid(3 * (int64_t)F)), dim3(DC_THREADS), 0, r.s, faces, F, cnt);
    LNERF_CHECK_LAUNCH("decimate(count)");
    DC_TRY(dc_scan(r, cnt, V, off));
    DC_HIP(hipMemsetAsync(cnt, 0, (size_t)V * 4, r.s), "memset");
    hipLaunchKernelGGL(k_dc_fill, dim3(dc_grid(3 * (int64_t)F)), dim3(DC_THREADS), 0, r.s, faces, F, off, cnt, list);
    hipLaunchKernelGGL(k_dc_sort, dim3(dc_grid(V)), dim3(DC_THREADS), 0, r.s, off, V, list);
    LNERF_CHECK_LAUNCH("decimate(lists)");
    return LNERF_OK;
}

static int dc_read(const DcRun &r, const int32_t *src, int32_t *dst) {
    DC_HIP(hipMemcpyAsync(dst, src, 4, hipMemcpyDeviceToHost, r.s), "read-back");
    DC_HIP(hipStreamSynchronize(r.s), "read-back");
    return LNERF_OK;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

size_t lnerf_decimate_scratch_bytes(int n_verts, int n_faces) {
    if (n_verts < 0 || n_faces < 0 || n_faces > LNERF_DECIMATE_MAX_FACES || n_verts > 3 * LNERF_DECIMATE_MAX_FACES)
        return 0;
    return dc_layout(n_verts, n_faces).bytes;
}

int lnerf_decimate(const float *verts, int n_verts, const int32_t *faces, int n_faces, int target_faces, float max_error,
                   int max_rounds, void *scratch, size_t scratch_bytes, float *verts_out, int32_t *faces_out,
                   float *normals_out, int64_t *counts_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_faces <= LNERF_DECIMATE_MAX_FACES &&
                  n_verts <= 3 * LNERF_DECIMATE_MAX_FACES,
                  "decimate: %d vertices / %d faces out of range (faces <= %d)", n_verts, n_faces,
                  LNERF_DECIMATE_MAX_FACES);
    LNERF_REQUIRE(target_faces >= 0 && max_rounds >= 0, "decimate: target_faces %d and max_rounds %d must be >= 0",
                  target_faces, max_rounds);
    LNERF_REQUIRE(max_error >= 0.f, "decimate: max_error must be >= 0 (+inf: none)");
    LNERF_REQUIRE(scratch && counts_dev && (n_verts == 0 || (verts && verts_out)) &&
                  (n_faces == 0 || (faces && faces_out)), "decimate: null pointer");
    const DcLayout L = dc_layout(n_verts, n_faces);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "decimate: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "decimate: scratch must be 16-byte aligned");
    const DcRun r{reinterpret_cast<char *>(scratch), L, as_stream(stream)};
    hipStream_t s = r.s;
    const int V = n_verts;
    float *pos = r.at<float>(L.pos), *vstar = r.at<float>(L.vstar);
    double *Q = r.at<double>(L.Q);
    int32_t *fa = r.at<int32_t>(L.fa), *fb = r.at<int32_t>(L.fb);
    int32_t *off = r.at<int32_t>(L.off), *list = r.at<int32_t>(L.list), *cnt = r.at<int32_t>(L.cnt);
    int32_t *locked = r.at<int32_t>(L.locked), *remap = r.at<int32_t>(L.remap);
    int32_t *flag = r.at<int32_t>(L.flag), *at = r.at<int32_t>(L.at), *sel = r.at<int32_t>(L.sel);
    int32_t *keep = r.at<int32_t>(L.keep), *dev = r.at<int32_t>(L.dev);
    unsigned long long *K1 = r.at<unsigned long long>(L.K1), *K2 = r.at<unsigned long long>(L.K2);
    unsigned long long *FK = r.at<unsigned long long>(L.FK), *keys = r.at<unsigned long long>(L.keys);

    // ---- input: index range first (no kernel reads through a face before this), repeated indices, compaction
    DC_HIP(hipMemsetAsync(dev, 0, 64, s), "memset");
    int F = 0;
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_dc_check, dim3(dc_grid(n_faces)), dim3(DC_THREADS), 0, s, faces, n_faces, V, flag, dev);
        LNERF_CHECK_LAUNCH("decimate(check)");
        int bad = 0;
        DC_TRY(dc_read(r, dev, &bad));
        LNERF_REQUIRE(bad == 0, "decimate: %d faces index outside [0, %d)", bad, V);
        DC_TRY(dc_scan(r, flag, n_faces, at));
        hipLaunchKernelGGL(k_dc_compact_faces, dim3(dc_grid(n_faces)), dim3(DC_THREADS), 0, s, faces, n_faces, flag, at,
                           fa);
        LNERF_CHECK_LAUNCH("decimate(compact)");
        DC_TRY(dc_read(r, at + n_faces, &F));
    }
    if (V > 0) DC_HIP(hipMemcpyAsync(pos, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, s), "copy");
    DC_TRY(dc_lists(r, fa, F, V));
    hipLaunchKernelGGL(k_dc_quadric, dim3(dc_grid(V)), dim3(DC_THREADS), 0, s, pos, fa, off, list, V, Q);
    LNERF_CHECK_LAUNCH("decimate(quadric)");

    // ---- rounds
    int rounds = 0;
    int64_t collapses = 0;
    while (rounds < max_rounds && F > target_faces) {
        const int E = 3 * F;
        hipLaunchKernelGGL(k_dc_status, dim3(dc_grid(V)), dim3(DC_THREADS), 0, s, fa, off, list, V, locked, K1, remap);
        hipLaunchKernelGGL(k_dc_eval, dim3(dc_grid(E)), dim3(DC_THREADS), 0, s, pos, fa, F, Q, off, list, locked,
                           max_error, keys, vstar, K1);
        hipLaunchKernelGGL(k_dc_face_key, dim3(dc_grid(F)), dim3(DC_THREADS), 0, s, fa, F, K1, FK);
        hipLaunchKernelGGL(k_dc_k2, dim3(dc_grid(V)), dim3(DC_THREADS), 0, s, off, list, V, FK, K2);
        hipLaunchKernelGGL(k_dc_select, dim3(dc_grid(E)), dim3(DC_THREADS), 0, s, fa, F, keys, K2, flag);
        LNERF_CHECK_LAUNCH("decimate(select)");
        DC_TRY(dc_scan(r, flag, E, at));
        hipLaunchKernelGGL(k_dc_gather, dim3(dc_grid(E)), dim3(DC_THREADS), 0, s, flag, at, E, F + 1, sel);
        LNERF_CHECK_LAUNCH("decimate(gather)");
        int S = 0;
        DC_TRY(dc_read(r, at + E, &S));
        if (S == 0) break;
        // independent collapses own disjoint face pairs, so S <= F / 2 (the gather wrote at most F + 1 entries)
        LNERF_REQUIRE(2 * (int64_t)S <= F, "decimate: internal: %d independent collapses among %d faces", S, F);
        int m = S;
        if (F - 2 * S < target_faces) {
            m = (F - target_faces + 1) / 2;
            hipLaunchKernelGGL(k_dc_rank, dim3(dc_grid(S)), dim3(DC_THREADS), 0, s, sel, S, m, keys, keep);
        }
        hipLaunchKernelGGL(k_dc_apply, dim3(dc_grid(S)), dim3(DC_THREADS), 0, s, fa, sel, S, m < S ? keep : nullptr,
                           vstar, pos, Q, remap);
        hipLaunchKernelGGL(k_dc_remap, dim3(dc_grid(F)), dim3(DC_THREADS), 0, s, fa, F, remap, flag);
        LNERF_CHECK_LAUNCH("decimate(apply)");
        DC_TRY(dc_scan(r, flag, F, at));
        hipLaunchKernelGGL(k_dc_compact_faces, dim3(dc_grid(F)), dim3(DC_THREADS), 0, s, fa, F, flag, at, fb);
        LNERF_CHECK_LAUNCH("decimate(compact)");
        std::swap(fa, fb);
        F -= 2 * m;          // each collapse removes exactly its edge's two faces (link condition)
        ++rounds;
        collapses += m;
        DC_TRY(dc_lists(r, fa, F, V));
    }

    // ---- output: referenced vertices in order, faces renumbered, normals
    const int32_t *vtot = dev;      // (0: no vertices)
    if (V > 0) {
        DC_HIP(hipMemsetAsync(cnt, 0, (size_t)V * 4, s), "memset");
        hipLaunchKernelGGL(k_dc_count, dim3(dc_grid(3 * (int64_t)F)), dim3(DC_THREADS), 0, s, fa, F, cnt);
        hipLaunchKernelGGL(k_dc_used, dim3(dc_grid(V)), dim3(DC_THREADS), 0, s, cnt, V, flag);
        LNERF_CHECK_LAUNCH("decimate(used)");
        DC_TRY(dc_scan(r, flag, V, at));
        hipLaunchKernelGGL(k_dc_out_verts, dim3(dc_grid(V)), dim3(DC_THREADS), 0, s, pos, flag, at, V, verts_out);
        hipLaunchKernelGGL(k_dc_out_faces, dim3(dc_grid(3 * (int64_t)F)), dim3(DC_THREADS), 0, s, fa, F, at, faces_out);
        LNERF_CHECK_LAUNCH("decimate(output)");
        vtot = at + V;
    }
    hipLaunchKernelGGL(k_dc_counts, dim3(1), dim3(64), 0, s, vtot, F, rounds, collapses, counts_dev);
    LNERF_CHECK_LAUNCH("decimate(counts)");
    if (normals_out && V > 0) {
        int Vout = 0;
        DC_TRY(dc_read(r, vtot, &Vout));
        DC_TRY(dc_lists(r, faces_out, F, Vout));   // lists of the output faces over the output vertices
        hipLaunchKernelGGL(k_dc_normals, dim3(dc_grid(Vout)), dim3(DC_THREADS), 0, s, verts_out, faces_out, off, list,
                           Vout, normals_out);
        LNERF_CHECK_LAUNCH("decimate(normals)");
    }
    return LNERF_OK;
}

}  // extern "C"
