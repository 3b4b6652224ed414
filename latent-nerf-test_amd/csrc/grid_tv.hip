// Total-variation regulariser of the hash table (`gridencoder.grad_total_variation` of the upstream encoder; the trainers'
// `lambda_tv`): the one gradient of the step that never touches a ray sample.  Definition (ours; restated in float64 in
// tests/tv_reference.py): level l has the vertex lattice [0, res_l]^3; for every SAMPLED vertex p and channel c
//     dtable[offsets[l] + row_l(p), c] += w_l * sum over q in N(p) of (e_c(p) - e_c(q)),      e(p) = table[offsets[l] + row_l(p)]
// N(p) = the up to six axis neighbours of p inside the lattice, row_l the level's index function (dense, hash, blocked,
// tiled: one definition with corner_rows of grid_shared.h).  Nothing is written to the neighbours' rows.  With every vertex
// sampled and w_l = lambda / N_l this is the exact gradient, hash collisions included, of
//     R_l = lambda / (2 N_l) * sum over the lattice edges (p, q) of |e(p) - e(q)|^2
// and with n_l of the N_l vertices sampled and w_l = lambda / n_l its unbiased estimate.
//
// Why lines and not points.  The upstream op draws ~10^6 random points and issues one scattered float atomic per (point,
// level, channel): 64 lanes in 64 different rows, the access shape MI355X_MICROARCH.md "Global float atomics" prices at
// 0.08 TB/s.  Here the unit of sampling is a LINE, all res + 1 vertices that share one (y, z): consecutive lanes own
// consecutive x, so on a dense level their rows are consecutive (plain coalesced read-modify-write), and on the hashed
// levels they sit in one contiguous block of rows (`hash`: x enters the XOR unmultiplied; `tiled`: the dense index
// wrapped; `blocked`: runs of four) -- contiguous atomics, the shape that runs at the full atomic rate.
//
// Sampling, per step and level: n_lines = min((res + 1)^2, max(1, tv_vertices / (res + 1))) (lnerf_grid_tv_plan).  All
// lines taken: the level is swept whole, line j is plane index j.  Otherwise line j is drawn from stratum j of the
// (res + 1)^2 plane indices, lo_j = floor(j S / n), idx = lo_j + h mod (lo_{j+1} - lo_j) in 64-bit integers, y = idx mod
// (res + 1), z = idx / (res + 1), h = counter_hash(j, seed, step, level) of common.h: distinct lines by
// construction.  `step` is read from the optimiser's device counter when one is given -- a replayed graph draws fresh
// lines every step.
//
// Reproducibility.  A dense level's index is a bijection and the lines are distinct, so every sampled row has exactly one
// writer: plain float2 read-modify-write, bitwise reproducible.  On a hashed level several vertices may share a row:
// atomicAdd per channel, the sum of a row with more than one contribution depends on the arrival order.
#include "grid_shared.h"

#include <limits.h>

namespace lnerf {

// line j of n of a level with `stride` = res + 1 vertices per axis -> (y, z)
__host__ __device__ __forceinline__ void tv_line(uint32_t j, uint32_t n, uint32_t stride, uint32_t seed, uint32_t step,
                                                 uint32_t level, uint32_t &y, uint32_t &z) {
    const unsigned long long S = (unsigned long long)stride * stride;
    unsigned long long idx = j;
    if ((unsigned long long)n != S) {   // (uniform per level.  j S < n S < 2^62: checked on the host)
        const unsigned long long lo = (unsigned long long)j * S / n, hi = ((unsigned long long)j + 1ull) * S / n;
        idx = lo + (unsigned long long)counter_hash(j, seed, step, level) % (hi - lo);   // n <= S: no stratum is empty
    }
    y = (uint32_t)(idx % stride);
    z = (uint32_t)(idx / stride);
}

constexpr int TV_THREADS = 256;

struct TvMeta {
    int num_levels;
    int layout;                              // 0 hash, 1 blocked, 2 tiled (GridMeta::blocked)
    int offsets[LNERF_MAX_LEVELS + 1];       // table rows
    int res[LNERF_MAX_LEVELS];
    int loff[LNERF_MAX_LEVELS + 1];          // first line of the level
    float w[LNERF_MAX_LEVELS];
    uint32_t bstart[LNERF_MAX_LEVELS + 1];   // first workgroup of the level (a workgroup serves ONE level: res, the table
                                             // size and the layout branch are scalar)
};

// row of ONE vertex inside its level: corner_rows' definitions
__device__ __forceinline__ uint32_t tv_row(uint32_t x, uint32_t y, uint32_t z, uint32_t stride, uint32_t hsize, bool dense,
                                           int layout) {
    if (dense) return x + y * stride + z * stride * stride;
    if (layout == 2) {
        const uint32_t i = x + y * stride + z * (stride * stride);   // (uint32 wrap-around)
        return (hsize & (hsize - 1u)) == 0u ? (i & (hsize - 1u)) : i % hsize;
    }
    if (layout == 1) {
        const uint32_t nblk = hsize >> 4;
        const uint32_t h = (x >> 2) ^ ((y >> 1) * 2654435761u) ^ ((z >> 1) * 805459861u);
        const uint32_t b = (nblk & (nblk - 1u)) == 0u ? (h & (nblk - 1u)) : h % nblk;
        return (b << 4) | (x & 3u) | ((y & 1u) << 2) | ((z & 1u) << 3);
    }
    const uint32_t h = x ^ (y * 2654435761u) ^ (z * 805459861u);
    return (hsize & (hsize - 1u)) == 0u ? (h & (hsize - 1u)) : h % hsize;
}

__device__ __forceinline__ int tv_level_of_block(const TvMeta &m) {
    int l = 0;
    while (l + 1 < m.num_levels && blockIdx.x >= m.bstart[l + 1]) ++l;   // (scalar: <= 31 compares)
    return l;
}

__global__ void __launch_bounds__(TV_THREADS)
k_grid_tv_lines(TvMeta m, uint32_t seed, uint32_t step, const int32_t *__restrict__ step_dev, int32_t *__restrict__ lines) {
    const int l = tv_level_of_block(m);
    const uint32_t n = (uint32_t)(m.loff[l + 1] - m.loff[l]);
    const uint32_t j = (blockIdx.x - m.bstart[l]) * TV_THREADS + threadIdx.x;
    if (j >= n) return;
    if (step_dev) step = (uint32_t)*step_dev;
    uint32_t y, z;
    tv_line(j, n, (uint32_t)m.res[l] + 1u, seed, step, (uint32_t)l, y, z);
    reinterpret_cast<int2 *>(lines)[(int64_t)m.loff[l] + j] = make_int2((int)y, (int)z);
}

// One lane per vertex of the flattened (line, x) index of its level (short lines share a wave).  The lane reads e(p) and
// its six neighbours -- a neighbour outside the lattice is replaced by p itself: its difference is an exact zero -- and
// writes its own row only.
__global__ void __launch_bounds__(TV_THREADS)
k_grid_tv_grad(const float *__restrict__ table, TvMeta m, const int32_t *__restrict__ lines, uint32_t seed, uint32_t step,
               const int32_t *__restrict__ step_dev, float *__restrict__ dtable) {
    const int l = tv_level_of_block(m);
    const uint32_t res = (uint32_t)m.res[l], stride = res + 1u;
    const uint32_t hsize = (uint32_t)(m.offsets[l + 1] - m.offsets[l]);
    const uint32_t n = (uint32_t)(m.loff[l + 1] - m.loff[l]);
    const uint32_t v = (blockIdx.x - m.bstart[l]) * TV_THREADS + threadIdx.x;   // n * stride < 2^31 (host)
    if (v >= n * stride) return;
    const uint32_t j = v / stride, x = v - j * stride;
    uint32_t y, z;
    if (lines) {
        const int2 yz = reinterpret_cast<const int2 *>(lines)[(int64_t)m.loff[l] + j];
        y = (uint32_t)yz.x;
        z = (uint32_t)yz.y;
        if (y > res || z > res) return;   // a line outside the lattice is ignored (it must never become a wild row)
    } else {
        if (step_dev) step = (uint32_t)*step_dev;
        tv_line(j, n, stride, seed, step, (uint32_t)l, y, z);
    }
    const bool dense = (uint64_t)stride * stride * stride <= (uint64_t)hsize;   // scalar
    const int layout = m.layout;
    const float2 *__restrict__ T = reinterpret_cast<const float2 *>(table) + m.offsets[l];
    const uint32_t xm = x > 0u ? x - 1u : x, xp = x < res ? x + 1u : x;
    const uint32_t ym = y > 0u ? y - 1u : y, yp = y < res ? y + 1u : y;
    const uint32_t zm = z > 0u ? z - 1u : z, zp = z < res ? z + 1u : z;
    const uint32_t row = tv_row(x, y, z, stride, hsize, dense, layout);
    const float2 e = T[row];
    const float2 q0 = T[tv_row(xm, y, z, stride, hsize, dense, layout)];
    const float2 q1 = T[tv_row(xp, y, z, stride, hsize, dense, layout)];
    const float2 q2 = T[tv_row(x, ym, z, stride, hsize, dense, layout)];
    const float2 q3 = T[tv_row(x, yp, z, stride, hsize, dense, layout)];
    const float2 q4 = T[tv_row(x, y, zm, stride, hsize, dense, layout)];
    const float2 q5 = T[tv_row(x, y, zp, stride, hsize, dense, layout)];
    // fixed order x-, x+, y-, y+, z-, z+
    float a = e.x - q0.x, b = e.y - q0.y;
    a = a + (e.x - q1.x); b = b + (e.y - q1.y);
    a = a + (e.x - q2.x); b = b + (e.y - q2.y);
    a = a + (e.x - q3.x); b = b + (e.y - q3.y);
    a = a + (e.x - q4.x); b = b + (e.y - q4.y);
    a = a + (e.x - q5.x); b = b + (e.y - q5.y);
    const float w = m.w[l];
    a = w * a;
    b = w * b;
    float2 *__restrict__ D = reinterpret_cast<float2 *>(dtable) + m.offsets[l];
    if (dense) {   // one writer per row
        float2 d = D[row];
        d.x = d.x + a;
        d.y = d.y + b;
        D[row] = d;
    } else {
        float *d = reinterpret_cast<float *>(D + row);
        unsafeAtomicAdd(d, a);
        unsafeAtomicAdd(d + 1, b);
    }
}

// level table + line plan of the two device entry points -> TvMeta (bstart: `per_vertex` false = one lane per line, true =
// one lane per vertex; a level with weight 0 gets no workgroup)
static int tv_fill(const char *who, TvMeta &m, int num_levels, const int32_t *res_host, const int32_t *line_offsets_host,
                   bool per_vertex, const float *weights_host, uint32_t *blocks) {
    LNERF_REQUIRE(num_levels >= 1 && num_levels <= LNERF_MAX_LEVELS, "%s: num_levels out of range (%d)", who, num_levels);
    LNERF_REQUIRE(res_host && line_offsets_host, "%s: null level metadata", who);
    LNERF_REQUIRE(line_offsets_host[0] == 0, "%s: line_offsets_host[0] must be 0", who);
    m.num_levels = num_levels;
    uint64_t nb = 0;
    for (int l = 0; l < num_levels; ++l) {
        LNERF_REQUIRE(res_host[l] >= 1 && res_host[l] <= 1 << 20, "%s: bad resolution at level %d", who, l);
        const int64_t n = (int64_t)line_offsets_host[l + 1] - (int64_t)line_offsets_host[l];
        const uint64_t stride = (uint64_t)res_host[l] + 1u;
        LNERF_REQUIRE(n >= 1, "%s: line offsets must increase (level %d has %lld lines)", who, l, (long long)n);
        LNERF_REQUIRE((uint64_t)n <= stride * stride, "%s: level %d has %lld lines, its lattice only %llu", who, l,
                      (long long)n, (unsigned long long)(stride * stride));
        LNERF_REQUIRE((uint64_t)n * stride <= (uint64_t)INT32_MAX, "%s: level %d samples more than 2^31 - 1 vertices", who, l);
        m.res[l] = res_host[l];
        m.loff[l] = line_offsets_host[l];
        m.w[l] = weights_host ? weights_host[l] : 1.0f;
        m.bstart[l] = (uint32_t)nb;
        if (!(weights_host && weights_host[l] == 0.0f))
            nb += (uint64_t)div_up(per_vertex ? (int64_t)((uint64_t)n * stride) : n, (int64_t)TV_THREADS);
    }
    m.loff[num_levels] = line_offsets_host[num_levels];
    m.bstart[num_levels] = (uint32_t)nb;
    LNERF_REQUIRE(nb <= (uint64_t)INT32_MAX, "%s: too many workgroups", who);
    *blocks = (uint32_t)nb;
    return LNERF_OK;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" int lnerf_grid_tv_plan(int num_levels, const int32_t *res_host, int64_t tv_vertices, int32_t *line_offsets_host) {
    LNERF_REQUIRE(num_levels >= 1 && num_levels <= LNERF_MAX_LEVELS, "grid_tv_plan: num_levels out of range (%d)", num_levels);
    LNERF_REQUIRE(res_host && line_offsets_host, "grid_tv_plan: null pointer");
    LNERF_REQUIRE(tv_vertices >= 1 && tv_vertices <= (int64_t)1 << 30, "grid_tv_plan: the vertex budget must be in [1, 2^30] (got %lld)",
                  (long long)tv_vertices);
    for (int l = 0; l < num_levels; ++l)
        LNERF_REQUIRE(res_host[l] >= 1 && res_host[l] <= 1 << 20, "grid_tv_plan: bad resolution at level %d", l);
    int64_t total = 0;
    line_offsets_host[0] = 0;
    for (int l = 0; l < num_levels; ++l) {
        const int64_t stride = (int64_t)res_host[l] + 1, S = stride * stride;
        int64_t n = tv_vertices / stride;
        n = n < 1 ? 1 : n;
        n = n > S ? S : n;
        total += n;
        LNERF_REQUIRE(total <= (int64_t)INT32_MAX, "grid_tv_plan: more than 2^31 - 1 lines");
        line_offsets_host[l + 1] = (int32_t)total;
    }
    return LNERF_OK;
}

extern "C" int lnerf_grid_tv_lines(int num_levels, const int32_t *res_host, const int32_t *line_offsets_host, uint32_t seed,
                                   uint32_t step, const int32_t *step_dev, int32_t *lines, lnerf_stream_t stream) {
    TvMeta m;
    memset(&m, 0, sizeof(m));
    uint32_t blocks = 0;
    const int rc = tv_fill("grid_tv_lines", m, num_levels, res_host, line_offsets_host, false, nullptr, &blocks);
    if (rc != LNERF_OK) return rc;
    LNERF_REQUIRE(lines, "grid_tv_lines: null pointer");
    hipLaunchKernelGGL(k_grid_tv_lines, dim3(blocks), dim3(TV_THREADS), 0, as_stream(stream), m, seed, step, step_dev, lines);
    LNERF_CHECK_LAUNCH("grid_tv_lines");
    return LNERF_OK;
}

extern "C" int lnerf_grid_tv_grad(const float *table, int num_levels, int level_dim, const int32_t *offsets_host,
                                  const int32_t *res_host, int layout_flags, const int32_t *line_offsets_host,
                                  const int32_t *lines, uint32_t seed, uint32_t step, const int32_t *step_dev,
                                  const float *weights_host, float *dtable, lnerf_stream_t stream) {
    LNERF_REQUIRE(level_dim == 2, "grid_tv_grad: only level_dim == 2 is built (got %d)", level_dim);
    LNERF_REQUIRE((layout_flags & ~(LNERF_GRID_BLOCKED | LNERF_GRID_TILED)) == 0, "grid_tv_grad: unknown layout flag 0x%x",
                  layout_flags);
    LNERF_REQUIRE(layout_flags != (LNERF_GRID_BLOCKED | LNERF_GRID_TILED),
                  "grid_tv_grad: LNERF_GRID_BLOCKED and LNERF_GRID_TILED exclude each other");
    LNERF_REQUIRE(offsets_host && weights_host, "grid_tv_grad: null level metadata");
    TvMeta m;
    memset(&m, 0, sizeof(m));
    uint32_t blocks = 0;
    const int rc = tv_fill("grid_tv_grad", m, num_levels, res_host, line_offsets_host, true, weights_host, &blocks);
    if (rc != LNERF_OK) return rc;
    m.layout = (layout_flags & LNERF_GRID_BLOCKED) ? 1 : ((layout_flags & LNERF_GRID_TILED) ? 2 : 0);
    LNERF_REQUIRE(offsets_host[0] >= 0, "grid_tv_grad: negative row offset");
    for (int l = 0; l < num_levels; ++l) {
        LNERF_REQUIRE(offsets_host[l + 1] > offsets_host[l], "grid_tv_grad: row offsets must increase (empty level %d)", l);
        LNERF_REQUIRE(m.layout != 1 || offsets_host[l + 1] - offsets_host[l] >= 16,
                      "grid_tv_grad: blocked layout needs >= 16 rows per level");
        LNERF_REQUIRE(weights_host[l] == weights_host[l] && weights_host[l] - weights_host[l] == 0.0f,
                      "grid_tv_grad: weight of level %d is not finite", l);
    }
    for (int l = 0; l <= num_levels; ++l) m.offsets[l] = offsets_host[l];
    LNERF_REQUIRE(table && dtable, "grid_tv_grad: null pointer");
    if (blocks == 0) return LNERF_OK;   // every weight is zero
    hipLaunchKernelGGL(k_grid_tv_grad, dim3(blocks), dim3(TV_THREADS), 0, as_stream(stream), table, m, lines, seed, step,
                       step_dev, dtable);
    LNERF_CHECK_LAUNCH("grid_tv_grad");
    return LNERF_OK;
}
