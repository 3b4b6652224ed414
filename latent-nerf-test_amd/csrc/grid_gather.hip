// H5/H6 multiresolution hash grid (Instant-NGP encoding, F = 2 features per vertex).
//
// Forward is the roofline kernel of the path: per sample and level it gathers
// 8 vertices x 2 features.  One thread handles one (sample, level); a wavefront handles 64
// consecutive samples of ONE level, so its 8 gather instructions hit one level's table and its
// output is 512 contiguous bytes (level-major feature layout).  The level is blockIdx.y.
#include "grid_shared.h"

namespace lnerf {

// Nothing here spends a vector instruction on an address: the level's table, the tile's positions and the (level,
// tile)'s features are wave-uniform 64-bit bases in scalar registers, and every load and the store add a 32-bit byte
// offset to one of them (`global_load_dword v, v_off, s[base]`).  The entry point checks what that needs: a level of at
// most 4 GiB, at most 2^31 - 1 samples.  (With the other cuts of DESIGN.md section 4, H5 the launch issues 14.3 M vector
// instructions instead of 27.5 M and runs 60.8 us instead of 65.5: instructions are a part of its time, not its bound.)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef u32x2 u32x2_dw __attribute__((aligned(4)));   // 8 or 16 bytes at a DWORD-aligned address
typedef f32x4 f32x4_dw __attribute__((aligned(4)));
template <typename T> __device__ __forceinline__ T load_at(const char *base, uint32_t byte_off) {
    return *reinterpret_cast<const T *>(base + byte_off);
}

// the vertex values of one cell as raw dwords: 8 (bf16 pairs) or 16 (f32 pairs).  load_pair fetches two consecutive
// table rows with one load (x-adjacent vertices are adjacent rows on dense levels, inside a block of the blocked layout,
// and on hashed levels when x is even: row(x+1) = row(x) ^ 1): half the cache accesses of those lookups.
// `lt` is the level's table as bytes.
template <typename TT> struct CellRaw;
template <> struct CellRaw<uint16_t> {
    uint32_t d[8];
    __device__ __forceinline__ void load_pair(const char *lt, uint32_t row, int c) {  // rows row, row+1 -> c, c+1
        const u32x2 v = load_at<u32x2_dw>(lt, row << 2);
        d[c] = v.x; d[c + 1] = v.y;
    }
    __device__ __forceinline__ void load_one(const char *lt, uint32_t row, int c) { d[c] = load_at<uint32_t>(lt, row << 2); }
    // rows r0, r1 of ONE aligned group of four rows (16 bytes) with one load -> c, c + 1
    __device__ __forceinline__ void load_quad(const char *lt, uint32_t r0, uint32_t r1, int c) {
        const uint4 v = load_at<uint4>(lt, (r0 & ~3u) << 2);
        const uint32_t k0 = r0 & 3u, k1 = r1 & 3u;
        d[c] = (k0 & 2u) ? ((k0 & 1u) ? v.w : v.z) : ((k0 & 1u) ? v.y : v.x);
        d[c + 1] = (k1 & 2u) ? ((k1 & 1u) ? v.w : v.z) : ((k1 & 1u) ? v.y : v.x);
    }
    static constexpr bool kHasQuad = true;
    static constexpr uint32_t kMaxLevelRows = 1u << 30;   // row << 2 is a 32-bit byte offset
    __device__ __forceinline__ void swap_pair(int c) { const uint32_t t = d[c]; d[c] = d[c + 1]; d[c + 1] = t; }
    // The cell of a lane that fetches nothing: its registers as they are.  Nothing reads them -- such a lane is either
    // past the end (it stores nothing) or takes its run's cell from the fetching lane -- so they are DEFINED here without
    // an instruction; cleared registers were eight moves per tile in front of the loads.
    __device__ __forceinline__ void unfetched() {
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "=v"(d[i]));
    }
    __device__ __forceinline__ void take_from_lane(int src4) {  // every lane reads the cell of lane src4 / 4
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (uint32_t)__builtin_amdgcn_ds_bpermute(src4, (int)d[i]);
    }
    __device__ __forceinline__ float2 get(int c) const {
        return make_float2(__uint_as_float(d[c] << 16), __uint_as_float(d[c] & 0xFFFF0000u));
    }
};
template <> struct CellRaw<float> {
    float2 d[8];
    __device__ __forceinline__ void load_pair(const char *lt, uint32_t row, int c) {
        const f32x4 v = load_at<f32x4_dw>(lt, row << 3);
        d[c] = make_float2(v.x, v.y); d[c + 1] = make_float2(v.z, v.w);
    }
    __device__ __forceinline__ void load_one(const char *lt, uint32_t row, int c) { d[c] = load_at<float2>(lt, row << 3); }
    __device__ __forceinline__ void load_quad(const char *, uint32_t, uint32_t, int) {}   // (32 bytes: not used)
    static constexpr bool kHasQuad = false;
    static constexpr uint32_t kMaxLevelRows = 1u << 29;
    __device__ __forceinline__ void swap_pair(int c) { const float2 t = d[c]; d[c] = d[c + 1]; d[c + 1] = t; }
    __device__ __forceinline__ void unfetched() {
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "=v"(d[i].x), "=v"(d[i].y));
    }
    __device__ __forceinline__ void take_from_lane(int src4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            d[i].x = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(d[i].x)));
            d[i].y = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(d[i].y)));
        }
    }
    __device__ __forceinline__ float2 get(int c) const { return d[c]; }
};

// level_pos_xyz (grid_shared.h) with the reciprocal of a power-of-two 2 * bound computed once on the host
// (`inv_two_b`, 0 for any other bound) instead of per lane: the same operations in the same order on either arm.
__device__ __forceinline__ LevelPos gather_level_pos(float x, float y, float z, float bound, float inv_two_b, float scale) {
    float px = x + bound, py = y + bound, pz = z + bound;
    if (inv_two_b != 0.f) {  // wave-uniform.  x / 2^k == x * 2^-k exactly
        px = px * inv_two_b; py = py * inv_two_b; pz = pz * inv_two_b;
    } else {
        const float two_b = 2.0f * bound;
        px = px / two_b; py = py / two_b; pz = pz / two_b;
    }
    px = px * scale; py = py * scale; pz = pz * scale;
    px = px + 0.5f; py = py + 0.5f; pz = pz + 0.5f;
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    LevelPos r;
    r.gx = (uint32_t)(int)flx; r.gy = (uint32_t)(int)fly; r.gz = (uint32_t)(int)flz;
    r.fx = px - flx; r.fy = py - fly; r.fz = pz - flz;
    return r;
}

// two f32 -> one dword of bf16 with ONE instruction, v_cvt_pk_bf16_f32: equal to f32_to_bf16 (common.h) on every one of
// the 2^32 inputs, in either half (round to nearest even, infinities kept, a NaN quieted with its sign and payload
// kept) -- checked exhaustively on the device (tools/cvt_pk_bf16_check.hip) before it replaced the ten integer
// instructions and two branches of the two casts
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    const f32x2 v = {a, b};
    const bf16x2 h = __builtin_convertvector(v, bf16x2);
    uint32_t r;
    __builtin_memcpy(&r, &h, sizeof(r));
    return r;
}
// one feature pair of the (level, tile)'s features `fb`
template <typename TO> __device__ __forceinline__ void store_feat(char *fb, uint32_t lane_in_tile, float a, float b);
template <> __device__ __forceinline__ void store_feat<float>(char *fb, uint32_t lane_in_tile, float a, float b) {
    *reinterpret_cast<float2 *>(fb + lane_in_tile * 8u) = make_float2(a, b);
}
template <> __device__ __forceinline__ void store_feat<uint16_t>(char *fb, uint32_t lane_in_tile, float a, float b) {
    *reinterpret_cast<uint32_t *>(fb + lane_in_tile * 4u) = bf16_pair(a, b);
}

template <typename TT, typename TO>
__global__ void __launch_bounds__(256)
k_grid_forward(const float *__restrict__ xyzs, float bound, float inv_two_b, const TT *__restrict__ table, GridMeta meta,
               uint32_t m_host, const int32_t *__restrict__ m_dev, int64_t level_stride, TO *__restrict__ feat,
               int pair_loads, int dedup_max_res) {
    uint32_t M = m_host;   // (< 2^31: checked by the entry point)
    if (m_dev) { const int32_t md = *m_dev; M = md < 0 ? 0u : ((uint32_t)md < M ? (uint32_t)md : M); }
    const TileMap tm = tile_map(0, meta.num_levels);
    const int l = tm.level;
    const float scale = meta.scales[l];
    const uint32_t res = (uint32_t)meta.res[l];
    const uint32_t off = (uint32_t)meta.offsets[l];
    const char *lt = reinterpret_cast<const char *>(table + (int64_t)off * 2);
    // Coarse levels: the 64 lanes of a wave are consecutive samples of a ray and sit in a handful of cells: only the
    // first lane of each run of equal cells fetches the 8 vertices, the others take them from it through the LDS
    // crossbar.
    const bool dedup = (int)res <= dedup_max_res;  // wave-uniform
    const int lane = lane_id();
    const uint32_t tid = threadIdx.x;
    for (uint32_t tile = (uint32_t)tm.tile0; tile * 256u < M; tile += (uint32_t)tm.tstep) {   // (tile * 256 < 2^31 + 2^19)
        const bool valid = tile * 256u + tid < M;  // (no early exit: the run logic below needs every lane of the wave)
        // The level's size is re-read as an opaque scalar every tile: what the compiler derives from a loop invariant it
        // computes in front of the loop, for every arm at once -- the reciprocals of `% hsize` and `% (hsize / 16)`
        // (two v_rcp_iflag_f32 and ten more vector instructions) were paid by every wave of the power-of-two tables,
        // and a wave runs one or two tiles.  What is left to recompute per tile is scalar.
        uint32_t hsize = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
        asm volatile("" : "+s"(hsize));
        const bool dense = (uint64_t)(res + 1) * (res + 1) * (res + 1) <= (uint64_t)hsize;  // wave-uniform
        const bool pow2 = (hsize & (hsize - 1u)) == 0u;
        const bool blocked = meta.blocked == 1 && !dense;
        LevelPos p;
        if (valid) {
            // (the tile's part of the address is a scalar the compiler cannot fold into the lane's part: the base stays
            // in scalar registers and the lane's byte offset stays 32 bits)
            uint64_t tile_off = (uint64_t)tile * (256u * 12u);
            uint32_t poff = tid * 12u;
            asm volatile("" : "+s"(tile_off), "+v"(poff));
            const char *pb = reinterpret_cast<const char *>(xyzs) + tile_off;   // wave-uniform
            const float *pp = reinterpret_cast<const float *>(pb + poff);
            p = gather_level_pos(pp[0], pp[1], pp[2], bound, inv_two_b, scale);
        } else {
            // a lane past the end heads its own run (wave_cell_runs), fetches nothing and stores nothing: its
            // position is whatever its registers hold
            asm volatile("" : "=v"(p.gx), "=v"(p.gy), "=v"(p.gz), "=v"(p.fx), "=v"(p.fy), "=v"(p.fz));
        }
        uint32_t rows[8];
        corner_rows(p.gx, p.gy, p.gz, res, hsize, rows, meta.blocked);
        bool fetch = valid;
        int src4;
        if (dedup) {
            const RunInfo ri = wave_cell_runs(p.gx, p.gy, p.gz, valid, lane);
            src4 = ri.start << 2;
            fetch = valid && ri.start == lane;
        } else {
            asm volatile("" : "=v"(src4));   // (not read)
        }
        // issue the gathers first, blend afterwards (keeps up to 8 loads in flight per lane)
        CellRaw<TT> cell;
        if (fetch) {
            // (one arm per kind of load; the conditions of a level's layout are wave-uniform, those on x are not)
            const bool x_in_group = (p.gx & 3u) != 3u;
            const bool hashed = pair_loads && meta.blocked == 0 && pow2 && !dense;
            const bool quads = hashed && pair_loads == 2 && CellRaw<TT>::kHasQuad && x_in_group;
            if (pair_loads && (dense || (blocked && x_in_group))) {
                // rows[c + 1] == rows[c] + 1: a dense level, or both x-neighbours in one block of the blocked layout (a
                // block's 16 rows are one aligned 64-byte line of the bf16 table and x & 3 < 3: the 8 bytes stay inside
                // it) -- one dword-aligned load per x pair, nothing to select
#pragma unroll
                for (int c = 0; c < 8; c += 2) cell.load_pair(lt, rows[c], c);
            } else if (quads) {
                // hashed, x mod 4 != 3: both x-neighbours sit in one aligned group of four rows (row = x ^ h: the group
                // is (x ^ h) & ~3) -- one 16-byte access instead of one 8-byte or two 4-byte ones
#pragma unroll
                for (int c = 0; c < 8; c += 2) cell.load_quad(lt, rows[c], rows[c + 1], c);
            } else if (hashed && !(p.gx & 1u)) {
                // hashed, x even: the two x-neighbours are the two halves of one aligned pair
#pragma unroll
                for (int c = 0; c < 8; c += 2) {
                    cell.load_pair(lt, rows[c] & ~1u, c);
                    if (rows[c] & 1u) cell.swap_pair(c);
                }
            } else {
                // no pairing asked for; tiled (rows follow the dense index mod hsize: no x ^ h structure to pair loads
                // on); blocked with the x pair in two blocks; hashed with x odd
#pragma unroll
                for (int c = 0; c < 8; ++c) cell.load_one(lt, rows[c], c);
            }
        } else {
            cell.unfetched();
        }
        if (dedup) cell.take_from_lane(src4);
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t bx = c & 1, by = (c >> 1) & 1, bz = (c >> 2) & 1;
            const float wx = bx ? p.fx : 1.0f - p.fx;
            const float wy = by ? p.fy : 1.0f - p.fy;
            const float wz = bz ? p.fz : 1.0f - p.fz;
            const float w = (wx * wy) * wz;
            const float2 v = cell.get(c);
            a0 = fmaf(w, v.x, a0);
            a1 = fmaf(w, v.y, a1);
        }
        if (valid) {
            uint64_t tile_off = ((uint64_t)l * (uint64_t)level_stride + (uint64_t)tile * 256u) * (2 * sizeof(TO));
            uint32_t lane_in_tile = tid;
            asm volatile("" : "+s"(tile_off), "+v"(lane_in_tile));   // (a scalar base and a 32-bit offset, as for the loads)
            char *fb = reinterpret_cast<char *>(feat) + tile_off;   // wave-uniform
            store_feat<TO>(fb, lane_in_tile, a0, a1);
        }
    }
}

// Backward, variant 0: one (sample, level) per thread, 16 global float atomics each.
template <typename TG>
__global__ void __launch_bounds__(256)
k_grid_backward_atomic(const float *__restrict__ xyzs, float bound, const TG *__restrict__ dfeat, GridMeta meta,
                       int64_t m_host, const int32_t *__restrict__ m_dev, int64_t level_stride,
                       float *__restrict__ dtable, int variant) {
    const int64_t M = valid_count(m_host, m_dev);
    const TileMap tm = tile_map(variant, meta.num_levels);
    if (!tm.ok) return;
    const int l = tm.level;
    const float scale = meta.scales[l];
    const uint32_t res = (uint32_t)meta.res[l];
    const uint32_t off = (uint32_t)meta.offsets[l];
    const uint32_t hsize = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
    float *lt = dtable + (int64_t)off * 2;
    for (int64_t tile = tm.tile0; tile * 256 < M; tile += tm.tstep) {
        const int64_t m = tile * 256 + threadIdx.x;
        if (m >= M) continue;
        const LevelPos p = level_pos(xyzs, m, bound, scale);
        const float2 gg = Feat2<TG>::load(dfeat + ((int64_t)l * level_stride + m) * 2, 0);
        uint32_t rows[8];
        corner_rows(p.gx, p.gy, p.gz, res, hsize, rows, meta.blocked);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t bx = c & 1, by = (c >> 1) & 1, bz = (c >> 2) & 1;
            const uint32_t row = rows[c];
            const float wx = bx ? p.fx : 1.0f - p.fx;
            const float wy = by ? p.fy : 1.0f - p.fy;
            const float wz = bz ? p.fz : 1.0f - p.fz;
            const float w = (wx * wy) * wz;
            atomicAdd(lt + (int64_t)row * 2, w * gg.x);
            atomicAdd(lt + (int64_t)row * 2 + 1, w * gg.y);
        }
    }
}

static void launch_dims(int variant, int L, int64_t m_host, dim3 &grid) {
    const int64_t tiles = div_up(m_host, 256);
    if (variant == 0) {
        int64_t gx = tiles < 1 ? 1 : tiles;
        if (gx > 2048) gx = 2048;
        grid = dim3((unsigned)gx, (unsigned)L, 1);
    } else {
        const int lv_per_xcd = (L + 7) / 8;
        int64_t per_level = tiles < 1 ? 1 : tiles;
        if (per_level > 256) per_level = 256;  // workgroups per level
        grid = dim3((unsigned)(8 * lv_per_xcd * per_level), 1, 1);
    }
}

void launch_grid_backward_atomic(const float *xyzs, float bound, const float *dfeat, const GridMeta &meta, int64_t m_host,
                                 const int32_t *m_dev, int64_t level_stride, float *dtable, int variant, hipStream_t s) {
    dim3 grid;
    launch_dims(variant, meta.num_levels, m_host, grid);
    hipLaunchKernelGGL((k_grid_backward_atomic<float>), grid, dim3(256), 0, s, xyzs, bound, dfeat, meta, m_host, m_dev,
                       level_stride, dtable, variant);
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_grid_encode_forward(const float *xyzs, float bound, const void *table, int table_dtype, int num_levels,
                              int level_dim, const int32_t *offsets_host, const float *scales_host,
                              const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                              void *feat, int feat_dtype, int variant, lnerf_stream_t stream) {
    GridMeta meta;
    const int blocked = variant & (LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    variant &= ~(LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    int rc = fill_meta("grid_encode_forward", meta, num_levels, level_dim, offsets_host, scales_host, res_host, blocked);
    if (rc) return rc;
    LNERF_REQUIRE(m_host >= 0 && level_stride >= m_host, "grid_encode_forward: need 0 <= m_host <= level_stride");
    LNERF_REQUIRE(bound > 0.f, "grid_encode_forward: bound must be > 0");
    // (XCD-pinned levels and XCD-owned level sets, variants 1 / 2, were measured no faster and removed)
    LNERF_REQUIRE(variant == 0, "grid_encode_forward: unknown variant %d", variant);
    LNERF_REQUIRE((table_dtype == LNERF_F32 || table_dtype == LNERF_BF16) &&
                      (feat_dtype == LNERF_F32 || feat_dtype == LNERF_BF16),
                  "grid_encode_forward: bad dtype tag");
    if (m_host == 0) return LNERF_OK;
    LNERF_REQUIRE(xyzs && table && feat, "grid_encode_forward: null pointer");
    // the kernel keeps sample indices and byte offsets into a level's table in 32 bits
    LNERF_REQUIRE(m_host <= (int64_t)INT32_MAX, "grid_encode_forward: m_host must be < 2^31 (32-bit sample indices)");
    const uint32_t max_rows = table_dtype == LNERF_F32 ? CellRaw<float>::kMaxLevelRows : CellRaw<uint16_t>::kMaxLevelRows;
    for (int l = 0; l < num_levels; ++l)
        LNERF_REQUIRE((uint32_t)(offsets_host[l + 1] - offsets_host[l]) <= max_rows,
                      "grid_encode_forward: level %d is larger than 4 GiB (32-bit byte offsets)", l);
    // 1 / (2 bound) when 2 bound is a power of two (exact; the kernel multiplies by it), 0 otherwise (the kernel divides)
    const float two_b = 2.0f * bound;
    uint32_t two_b_bits;
    memcpy(&two_b_bits, &two_b, sizeof(two_b_bits));
    const float inv_two_b = (two_b_bits & 0x007FFFFFu) == 0u ? 1.0f / two_b : 0.f;
    dim3 grid;
    launch_dims(0, num_levels, m_host, grid);
    hipStream_t s = as_stream(stream);
#define LAUNCH_FWD(TT, TO)                                                                                         \
    hipLaunchKernelGGL((k_grid_forward<TT, TO>), grid, dim3(256), (size_t)g_gather_lds_pad, s, xyzs, bound, inv_two_b, (const TT *)table, meta, \
                       (uint32_t)m_host, m_dev, level_stride, (TO *)feat, g_gather_pairs, g_gather_dedup_res)
    if (table_dtype == LNERF_F32 && feat_dtype == LNERF_F32) LAUNCH_FWD(float, float);
    else if (table_dtype == LNERF_F32) LAUNCH_FWD(float, uint16_t);
    else if (feat_dtype == LNERF_F32) LAUNCH_FWD(uint16_t, float);
    else LAUNCH_FWD(uint16_t, uint16_t);
#undef LAUNCH_FWD
    LNERF_CHECK_LAUNCH("grid_encode_forward");
    return LNERF_OK;
}

}  // extern "C"
