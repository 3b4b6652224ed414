// H10 occupancy refresh: cell points, the steady-state sampling (compaction of the occupied cells + draw), the
// order-independent per-cell maximum and the mean in a fixed summation order.
#include "scan.h"

#include <math.h>

namespace lnerf {

// Morton index + jitter in [0, 1)^3 -> point of that cell.  Op order restated in oracle/nerf_oracle.py.
__device__ __forceinline__ void cell_point(uint32_t idx, float nx, float ny, float nz, int G, float mip_bound,
                                           float *__restrict__ xyz) {
    const float cx = (float)compact_bits(idx), cy = (float)compact_bits(idx >> 1), cz = (float)compact_bits(idx >> 2);
    const float s = 2.0f / (float)G;
    float ux = cx + nx, uy = cy + ny, uz = cz + nz;
    ux = ux * s; uy = uy * s; uz = uz * s;
    ux = ux - 1.0f; uy = uy - 1.0f; uz = uz - 1.0f;
    xyz[0] = ux * mip_bound;
    xyz[1] = uy * mip_bound;
    xyz[2] = uz * mip_bound;
}
__global__ void __launch_bounds__(256)
k_occ_cell_points(const uint32_t *__restrict__ indices, int64_t n, float mip_bound, int G,
                  const float *__restrict__ noise, float *__restrict__ xyzs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float nx = noise ? noise[i * 3] : 0.5f, ny = noise ? noise[i * 3 + 1] : 0.5f,
                    nz = noise ? noise[i * 3 + 2] : 0.5f;
        cell_point(indices ? indices[i] : (uint32_t)i, nx, ny, nz, G, mip_bound, xyzs + i * 3);
    }
}

// ---- steady-state sampling of the refresh, on the device (lnerf_occ_sample): n_rand uniformly random cells + n_rand
// cells drawn uniformly from the OCCUPIED ones, jittered points inside them.  The upstream form (torch.nonzero of the
// grid, two randint, an index, a cat, a rand) is six launches and a host synchronisation on the size of the occupied
// list; here the list is compacted in ascending cell order by two launches (deterministic: replicas of a data-parallel
// run draw the same cells), its length stays on the device, and one launch draws cells and points from the counter-based
// generator u = counter_hash(i, seed, step, k) -- restated in oracle/nerf_oracle.py occ_sample.
constexpr int OCC_BLOCK_CELLS = 4096;                  // cells per workgroup of the compaction
constexpr int OCC_ROUNDS = OCC_BLOCK_CELLS / 256;      // of 256 consecutive cells, one per thread
__global__ void __launch_bounds__(256) k_occ_count(const float *__restrict__ grid, int64_t n_cells, int32_t *__restrict__ counts) {
    const int64_t base = (int64_t)blockIdx.x * OCC_BLOCK_CELLS;
    int c[1] = {0}, before[1], total[1];
#pragma unroll 4
    for (int k = 0; k < OCC_ROUNDS; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        c[0] += (i < n_cells && grid[i] > 0.f) ? 1 : 0;
    }
    block_exclusive_scan<256>(c, before, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total[0];
}
// Ascending cell order: round k of a workgroup is its k-th 256 consecutive cells.  The rounds keep their coalesced loads
// and all go through ONE block scan of OCC_ROUNDS counters (one barrier, the loads of all rounds in flight together; a
// thread owning 16 consecutive cells would scan one counter but load and store with a 64-byte stride).
__global__ void __launch_bounds__(256) k_occ_fill(const float *__restrict__ grid, int64_t n_cells,
                                                  const int32_t *__restrict__ counts, int n_blocks,
                                                  int32_t *__restrict__ list, int32_t *__restrict__ total_dev) {
    const int tid = threadIdx.x;
    // cells in earlier workgroups; workgroup 0 has none before it and sums all counts instead: the total
    const int upto = blockIdx.x == 0 ? n_blocks : (int)blockIdx.x;
    int part[1] = {0}, unused[1], sum[1];
    for (int b = tid; b < upto; b += 256) part[0] += counts[b];
    block_exclusive_scan<256>(part, unused, sum);
    if (blockIdx.x == 0 && tid == 0) *total_dev = sum[0];
    int offset = blockIdx.x == 0 ? 0 : sum[0];
    const int64_t base = (int64_t)blockIdx.x * OCC_BLOCK_CELLS + tid;
    int occ[OCC_ROUNDS], rank[OCC_ROUNDS], round_total[OCC_ROUNDS];
#pragma unroll
    for (int k = 0; k < OCC_ROUNDS; ++k) occ[k] = (base + k * 256 < n_cells && grid[base + k * 256] > 0.f) ? 1 : 0;
    block_exclusive_scan<256>(occ, rank, round_total);   // (its own slots: another <THREADS, T, N> than the one above)
#pragma unroll
    for (int k = 0; k < OCC_ROUNDS; ++k) {
        if (occ[k]) list[offset + rank[k]] = (int32_t)(base + k * 256);
        offset += round_total[k];
    }
}
__global__ void __launch_bounds__(256)
k_occ_draw(const int32_t *__restrict__ list, const int32_t *__restrict__ total_dev, int64_t n_cells, int64_t n_rand,
           uint32_t seed, uint32_t step, float mip_bound, int G, uint32_t *__restrict__ indices, float *__restrict__ xyzs) {
    const int total = *total_dev;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n_rand; i += (int64_t)gridDim.x * blockDim.x) {
        // STRATIFIED draws, ascending by construction: draw j of a half takes one element, uniformly, from the j-th of
        // n_rand equal strata of its population -- the cells in (Morton) order for the first half, the ascending list of
        // occupied cells for the second (a stratum of less than one element repeats its element: with fewer occupied cells
        // than draws every occupied cell is drawn total / n_rand times in a row, each time with its own jitter).  Every
        // cell keeps the marginal probability of the independent draws the upstream refresh makes (n_rand / n_cells;
        // n_rand / total), no stratum is left out by chance, and consecutive lanes evaluate NEIGHBOURING cells: the density
        // query on the candidates runs at the rate of ray samples instead of that of unrelated points (gather + MLP
        // 285 -> 195 us per refresh, the per-cell maximum 75 -> 60: measured by sorting the independent draws).
        const uint32_t h = counter_hash((uint32_t)i, seed, step, 0u);
        const unsigned long long j = (unsigned long long)(i < n_rand ? i : i - n_rand);
        const unsigned long long pop = (i >= n_rand && total > 0) ? (unsigned long long)total : (unsigned long long)n_cells;
        const unsigned long long lo = j * pop / (unsigned long long)n_rand, hi = (j + 1ull) * pop / (unsigned long long)n_rand;
        unsigned long long pick = lo + (((unsigned long long)h * (hi - lo)) >> 32);   // (hi == lo: the stratum's one element)
        pick = pick < pop ? pick : pop - 1ull;
        const uint32_t idx = (i >= n_rand && total > 0) ? (uint32_t)list[(int)pick] : (uint32_t)pick;
        indices[i] = idx;
        const float nx = hash_unit(counter_hash((uint32_t)i, seed, step, 1u));
        const float ny = hash_unit(counter_hash((uint32_t)i, seed, step, 2u));
        const float nz = hash_unit(counter_hash((uint32_t)i, seed, step, 3u));
        cell_point(idx, nx, ny, nz, G, mip_bound, xyzs + i * 3);
    }
}

// Occupancy refresh, order-independent form (replicas of a data-parallel run must stay bit-identical, and the sampled
// index list may name a cell more than once): pass 1 takes the MAXIMUM of the new densities per cell into a scratch
// grid (non-negative floats order as unsigned integers: atomicMax on the bits), pass 2 applies
// grid = max(grid * decay, scratch) to the touched cells.  scratch: one uint32 per cell, all zero between calls.
__global__ void __launch_bounds__(256) k_occ_update_max(unsigned int *__restrict__ scratch,
                                                        const uint32_t *__restrict__ indices, int64_t n,
                                                        const float *__restrict__ sig) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t idx = indices ? indices[i] : (uint32_t)i;
        const float s = sig[i];
        // bit 31 marks "touched" (a density of exactly 0 must still decay the cell); densities < 0 never update
        if (s >= 0.f) atomicMax(&scratch[idx], __float_as_uint(s) | 0x80000000u);
    }
}
__global__ void __launch_bounds__(256) k_occ_update_apply(float *__restrict__ grid, unsigned int *__restrict__ scratch,
                                                          const uint32_t *__restrict__ indices, int64_t n, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t idx = indices ? indices[i] : (uint32_t)i;
        // the first entry of a cell takes its maximum (and leaves the scratch word zero for the next call); further
        // entries of the same cell find zero: exactly one thread updates the cell, whatever the order
        const unsigned int m = atomicExch(&scratch[idx], 0u);
        if (!(m & 0x80000000u)) continue;
        const float old = grid[idx];
        if (old >= 0.f) grid[idx] = fmaxf(old * decay, __uint_as_float(m & 0x7FFFFFFFu));
    }
}

// mean of max(grid, 0) over all cells, in a FIXED summation order (a float atomicAdd over the partial sums would make
// the mean -- and with it the occupancy threshold min(mean, thresh) and the bitfield -- depend on arrival order):
// OCC_MEAN_BLOCKS workgroups each sum a fixed strided slice into partial[block]; one workgroup adds the partials in
// index order.
constexpr int OCC_MEAN_BLOCKS = 256;
// the sum over a 256-thread workgroup, every thread calls it: wave sums, then the 4 waves in order
__device__ __forceinline__ float block_sum_ordered(float s) {
    __shared__ float s_w[4];
    s = wave_sum(s);
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
__global__ void __launch_bounds__(256) k_occ_mean_partial(const float *__restrict__ grid, int64_t n,
                                                          float *__restrict__ partial) {
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += fmaxf(grid[i], 0.f);
    s = block_sum_ordered(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// apply + mean in ONE pass over the CELLS (not the candidates): a cell whose scratch word is marked takes
// grid = max(grid * decay, maximum) and the word goes back to zero; every thread adds max(grid, 0) of its cells in the
// slice order of k_occ_mean_partial, so the mean is the one the two separate launches give, bit for bit.  Streaming
// (16 B per cell) instead of one atomicExch per candidate: 58 + 9 us -> 8 us for 2 M cells / 1 M candidates.
__global__ void __launch_bounds__(256) k_occ_apply_mean(float *__restrict__ grid, unsigned int *__restrict__ scratch,
                                                        int64_t n, float decay, float *__restrict__ partial) {
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float g = grid[i];
        const unsigned int m = scratch[i];
        if (m & 0x80000000u) {
            scratch[i] = 0u;
            if (g >= 0.f) {
                g = fmaxf(g * decay, __uint_as_float(m & 0x7FFFFFFFu));
                grid[i] = g;
            }
        }
        s += fmaxf(g, 0.f);
    }
    s = block_sum_ordered(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void __launch_bounds__(64) k_occ_mean_final(const float *__restrict__ partial, int blocks, float n,
                                                       float *__restrict__ mean) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < blocks; ++b) s += partial[b];
        *mean = s / n;
    }
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_occ_cell_points(const uint32_t *indices, int64_t n, int cascade_level, int grid_size, float bound,
                          const float *noise, float *xyzs, lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0 && cascade_level >= 0 && cascade_level < 8 && grid_size > 0 && bound > 0.f,
                  "occ_cell_points: bad arguments");
    if (n == 0) return LNERF_OK;
    LNERF_REQUIRE(xyzs, "occ_cell_points: null xyzs");
    const float mip_bound = fminf((float)(1 << cascade_level), bound);
    hipLaunchKernelGGL(k_occ_cell_points, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), indices, n, mip_bound,
                       grid_size, noise, xyzs);
    LNERF_CHECK_LAUNCH("occ_cell_points");
    return LNERF_OK;
}

int lnerf_occ_sample(const float *grid_level, int64_t n_cells, int cascade_level, int grid_size, float bound,
                     int64_t n_rand, uint32_t seed, uint32_t step, int32_t *scratch, uint32_t *indices, float *xyzs,
                     lnerf_stream_t stream) {
    LNERF_REQUIRE(n_cells > 0 && n_cells <= ((int64_t)1 << 31) && n_rand >= 0 && 2 * n_rand < ((int64_t)1 << 31),
                  "occ_sample: sizes out of range");
    LNERF_REQUIRE(cascade_level >= 0 && cascade_level < 8 && grid_size > 0 && bound > 0.f, "occ_sample: bad arguments");
    if (n_rand == 0) return LNERF_OK;
    LNERF_REQUIRE(grid_level && scratch && indices && xyzs, "occ_sample: null pointer");
    const int n_blocks = (int)div_up(n_cells, (int64_t)OCC_BLOCK_CELLS);
    int32_t *counts = scratch, *total = scratch + n_blocks, *list = scratch + n_blocks + 1;   // [n_blocks | 1 | n_cells]
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_occ_count, dim3((unsigned)n_blocks), dim3(256), 0, s, grid_level, n_cells, counts);
    LNERF_CHECK_LAUNCH("occ_sample(count)");
    hipLaunchKernelGGL(k_occ_fill, dim3((unsigned)n_blocks), dim3(256), 0, s, grid_level, n_cells, counts, n_blocks, list, total);
    LNERF_CHECK_LAUNCH("occ_sample(fill)");
    const float mip_bound = fminf((float)(1 << cascade_level), bound);
    hipLaunchKernelGGL(k_occ_draw, dim3(grid_for(2 * n_rand)), dim3(256), 0, s, list, total, n_cells, n_rand, seed, step,
                       mip_bound, grid_size, indices, xyzs);
    LNERF_CHECK_LAUNCH("occ_sample(draw)");
    return LNERF_OK;
}

size_t lnerf_occ_sample_scratch_bytes(int64_t n_cells) {
    if (n_cells <= 0) return 0;
    return (size_t)(div_up(n_cells, (int64_t)OCC_BLOCK_CELLS) + 1 + n_cells) * sizeof(int32_t);
}

int lnerf_occ_update(float *grid_level, const uint32_t *indices, int64_t n, const float *new_sigmas, float decay,
                     uint32_t *scratch_cells, lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0, "occ_update: negative n");
    if (n == 0) return LNERF_OK;
    LNERF_REQUIRE(grid_level && new_sigmas && scratch_cells, "occ_update: null pointer");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_occ_update_max, dim3(grid_for(n)), dim3(256), 0, s, scratch_cells, indices, n, new_sigmas);
    LNERF_CHECK_LAUNCH("occ_update(max)");
    hipLaunchKernelGGL(k_occ_update_apply, dim3(grid_for(n)), dim3(256), 0, s, grid_level, scratch_cells, indices, n, decay);
    LNERF_CHECK_LAUNCH("occ_update(apply)");
    return LNERF_OK;
}

int lnerf_occ_update_mean(float *grid_level, int64_t n_cells, const uint32_t *indices, int64_t n, const float *new_sigmas,
                          float decay, uint32_t *scratch_cells, float *mean_dev, float *scratch256,
                          lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0 && n_cells > 0, "occ_update_mean: bad sizes");
    LNERF_REQUIRE(grid_level && scratch_cells && mean_dev && scratch256 && (n == 0 || new_sigmas),
                  "occ_update_mean: null pointer");
    hipStream_t s = as_stream(stream);
    if (n > 0) {
        hipLaunchKernelGGL(k_occ_update_max, dim3(grid_for(n)), dim3(256), 0, s, scratch_cells, indices, n, new_sigmas);
        LNERF_CHECK_LAUNCH("occ_update_mean(max)");
    }
    hipLaunchKernelGGL(k_occ_apply_mean, dim3(OCC_MEAN_BLOCKS), dim3(256), 0, s, grid_level, scratch_cells, n_cells, decay,
                       scratch256);
    LNERF_CHECK_LAUNCH("occ_update_mean(apply)");
    hipLaunchKernelGGL(k_occ_mean_final, dim3(1), dim3(64), 0, s, scratch256, OCC_MEAN_BLOCKS, (float)n_cells, mean_dev);
    LNERF_CHECK_LAUNCH("occ_update_mean(final)");
    return LNERF_OK;
}

int lnerf_occ_mean(const float *grid, int64_t n, float *mean_dev, float *scratch256, lnerf_stream_t stream) {
    LNERF_REQUIRE(n > 0 && grid && mean_dev && scratch256, "occ_mean: bad arguments");
    hipLaunchKernelGGL(k_occ_mean_partial, dim3(OCC_MEAN_BLOCKS), dim3(256), 0, as_stream(stream), grid, n, scratch256);
    LNERF_CHECK_LAUNCH("occ_mean(partial)");
    hipLaunchKernelGGL(k_occ_mean_final, dim3(1), dim3(64), 0, as_stream(stream), scratch256, OCC_MEAN_BLOCKS, (float)n,
                       mean_dev);
    LNERF_CHECK_LAUNCH("occ_mean(final)");
    return LNERF_OK;
}

}  // extern "C"
