// Integer prefix sums of the library, and the scratch layout of the mesh-export kernels.  block_exclusive_scan and the
// 64-bit wave scan serve every workgroup scan outside the scatter (grid.hip and grid_bin.hip keep their tuned ones): the
// march's scan kernel and overflow totals and the live-ray compaction (rays.hip), the occupied-cell list of the refresh
// (occupancy.hip), and the mesh-export kernels (isosurface.hip, uvbake.hip, decimate.hip, atlas.hip, meshclean.hip,
// mesh_shared.h).  A compaction of the mesh export is
//   per block   block_exclusive_scan inside the kernel that counts, its block total -> blk[block]
//   scan_top    k_scan_top, ONE workgroup: exclusive prefix of the block totals (in place) and the grand total
//   per block   block prefix + position in the block
// and where the counts already lie in memory, scan_flat: the int32 exclusive prefix of in[0, n) with the total at out[n].
// Integer sums only, so every order of addition gives the same bits.
// Scratch: a layout function takes its regions from a Carve, the entry point reads them with at<T>().
#pragma once
#include "common.h"

namespace lnerf {

constexpr int SCAN_TOP_THREADS = 1024;

static inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// consecutive 256-byte aligned regions of one scratch buffer: take() gives a region's offset, `o` is the size so far
struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    }
};
template <typename T>
static inline T *at(void *scratch, size_t off) { return reinterpret_cast<T *>(reinterpret_cast<char *>(scratch) + off); }

// inclusive wave scan (sum) of a 64-bit value: wave_inclusive_sum_i's DPP steps move 32 bits, so this one shuffles
__device__ __forceinline__ long long wave_inclusive_sum_ll(long long x) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < LNERF_WAVE; o <<= 1) {
        const long long u = __shfl_up(x, o, LNERF_WAVE);
        if (lane >= o) x += u;
    }
    return x;
}
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum_int(T x) {
    if constexpr (sizeof(T) == 4) return (T)wave_inclusive_sum_i((int)x);
    else return (T)wave_inclusive_sum_ll((long long)x);
}

// Exclusive prefix over a workgroup of THREADS threads of N counters carried together (one barrier for all of them):
// excl[c] = sum of v[c] over the threads before this one, total[c] = sum over the workgroup.
//   - EVERY thread of the workgroup calls it: there is a barrier inside.
//   - The per-wave slots are the function's own (declared here, not passed in: a pointer parameter loses the LDS
//     address space, see grid.hip scatter_reduce_one), one set per <THREADS, T, N>.  A second call with the same
//     arguments in one kernel reuses them, so it needs a __syncthreads() between the two calls.
template <int THREADS, typename T, int N>
__device__ __forceinline__ void block_exclusive_scan(const T (&v)[N], T (&excl)[N], T (&total)[N]) {
    constexpr int WAVES = THREADS / LNERF_WAVE;
    __shared__ T s_w[N][WAVES];
    const int w = threadIdx.x / LNERF_WAVE;
    T incl[N];
#pragma unroll
    for (int c = 0; c < N; ++c) incl[c] = wave_inclusive_sum_int(v[c]);
    if (lane_id() == LNERF_WAVE - 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) s_w[c][w] = incl[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {
            const T x = s_w[c][k];
            if (k < w) before += x;
            all += x;
        }
        excl[c] = before + incl[c] - v[c];
        total[c] = all;
    }
}

// ONE workgroup: exclusive prefix of a[0, nb) in place and its total -> *total_a; the same for b and *total_b unless b is
// NULL.  Thread t owns the ceil(nb / SCAN_TOP_THREADS) consecutive entries from t * that on.  total_a may be a + nb.
template <typename T>
__global__ void __launch_bounds__(SCAN_TOP_THREADS)
k_scan_top(T *__restrict__ a, T *__restrict__ b, int64_t nb, T *__restrict__ total_a, T *__restrict__ total_b) {
    const int64_t chunk = (nb + SCAN_TOP_THREADS - 1) / SCAN_TOP_THREADS;
    const int64_t b0 = min((int64_t)threadIdx.x * chunk, nb), b1 = min(b0 + chunk, nb);
    T sum[2] = {0, 0}, run[2], total[2];
    for (int64_t k = b0; k < b1; ++k) {
        sum[0] += a[k];
        if (b) sum[1] += b[k];
    }
    block_exclusive_scan<SCAN_TOP_THREADS>(sum, run, total);
    for (int64_t k = b0; k < b1; ++k) {
        const T x = a[k], y = b ? b[k] : 0;
        a[k] = run[0];
        run[0] += x;
        if (b) {
            b[k] = run[1];
            run[1] += y;
        }
    }
    if (threadIdx.x == 0) {
        *total_a = total[0];
        if (b) *total_b = total[1];
    }
}

static inline void scan_top(int64_t *a, int64_t *b, int64_t nb, int64_t *total_a, int64_t *total_b, hipStream_t s) {
    LNERF_LAUNCH(k_scan_top<int64_t>, 1, SCAN_TOP_THREADS, s, a, b, nb, total_a, total_b);
}

// ---------------------------------------------------------------- scan_flat
constexpr int SCAN_FLAT_THREADS = 256;
constexpr int SCAN_FLAT_PPT = 16;
constexpr int SCAN_FLAT_BLOCK = SCAN_FLAT_THREADS * SCAN_FLAT_PPT;

static __global__ void __launch_bounds__(SCAN_FLAT_THREADS)
k_scan_flat_blocks(const int32_t *__restrict__ in, int n, int32_t *__restrict__ out, int32_t *__restrict__ blk) {
    const int base = blockIdx.x * SCAN_FLAT_BLOCK + threadIdx.x * SCAN_FLAT_PPT;
    int sum[1] = {0}, run[1], tot[1];
    for (int q = 0; q < SCAN_FLAT_PPT; ++q)
        if (base + q < n) sum[0] += in[base + q];
    block_exclusive_scan<SCAN_FLAT_THREADS>(sum, run, tot);
    for (int q = 0; q < SCAN_FLAT_PPT; ++q)
        if (base + q < n) {
            const int x = in[base + q];
            out[base + q] = run[0];
            run[0] += x;
        }
    if (threadIdx.x == 0) blk[blockIdx.x] = tot[0];
}

static __global__ void __launch_bounds__(SCAN_FLAT_THREADS)
k_scan_flat_add(int32_t *__restrict__ out, int n, const int32_t *__restrict__ blk, int nb) {
    const int i = blockIdx.x * SCAN_FLAT_THREADS + threadIdx.x;
    if (i < n) out[i] += blk[i / SCAN_FLAT_BLOCK];
    if (i == 0) out[n] = blk[nb];
}

// the block totals of scan_flat over n entries, and their total
static inline size_t scan_flat_blk_bytes(int64_t n) { return (size_t)(div_up(n > 1 ? n : 1, SCAN_FLAT_BLOCK) + 1) * 4; }

// exclusive prefix of in[0, n) into out[0, n], out[n] = total; blk: scan_flat_blk_bytes(n) of scratch
static inline int scan_flat(const int32_t *in, int n, int32_t *out, int32_t *blk, hipStream_t s, const char *what) {
    const int nb = (int)div_up(n > 1 ? n : 1, SCAN_FLAT_BLOCK);
    LNERF_LAUNCH(k_scan_flat_blocks, (int64_t)nb * SCAN_FLAT_THREADS, SCAN_FLAT_THREADS, s, in, n, out, blk);
    // (int32: more than 1024 blocks, where a thread of k_scan_top owns several entries, takes over 1.4 M faces, too many
    // for a test through the Python restatement; the int64 instantiation of the same template is tested on that side)
    LNERF_LAUNCH(k_scan_top<int32_t>, 1, SCAN_TOP_THREADS, s, blk, (int32_t *)nullptr, (int64_t)nb, blk + nb,
                 (int32_t *)nullptr);
    LNERF_LAUNCH(k_scan_flat_add, n, SCAN_FLAT_THREADS, s, out, n, blk, nb);
    LNERF_CHECK_LAUNCH(what);
    return LNERF_OK;
}

}  // namespace lnerf
