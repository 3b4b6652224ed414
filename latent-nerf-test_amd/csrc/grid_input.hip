// Gradient of the hash-grid features with respect to the SAMPLE POSITION (the upstream encoder's
// `grid_backward_input`), and the elementwise finish that turns it into the density gradient / surface normal.
//
// feat[l, m, f] = sum_c w_c(frac) table[row_c, f] is trilinear inside a cell, frac = pos - floor(pos),
// pos = (x + bound) / (2 bound) * scale_l + 0.5, so
//     d feat / d x_a = scale_l / (2 bound) * sum_c table[row_c, f] * d w_c / d frac_a
// with d w_c / d frac_x = (bx ? +1 : -1) wy wz (and likewise for y, z).  floor() has no gradient: on a lattice plane
// the result is the one-sided derivative of the cell the FORWARD put the sample in (same level_pos, same cell).
//
// One lane per sample, looping over the levels in the fixed order 0 .. L-1: dxyz[m] is WRITTEN once by its own lane
// -- no atomics, no partial buffer, the same bits on every call.  A wave reads 512 contiguous bytes of dfeat per level
// and keeps the 8 vertex loads of the level in flight before it blends them, as the forward does.
#include "grid_shared.h"
#include "mlp_shared.h"

namespace lnerf {

template <typename TT>
__global__ void __launch_bounds__(256)
k_grid_backward_input(const float *__restrict__ xyzs, float bound, const TT *__restrict__ table, GridMeta meta,
                      int64_t m_host, const int32_t *__restrict__ m_dev, int64_t level_stride,
                      const float *__restrict__ dfeat, float *__restrict__ dxyz) {
    const int64_t M = valid_count(m_host, m_dev);
    const float two_b = 2.0f * bound;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const float x = xyzs[m * 3], y = xyzs[m * 3 + 1], z = xyzs[m * 3 + 2];
        float dx = 0.f, dy = 0.f, dz = 0.f;
        for (int l = 0; l < meta.num_levels; ++l) {   // (l is wave-uniform: the level's metadata are scalar loads)
            const float scale = meta.scales[l];
            const uint32_t res = (uint32_t)meta.res[l];
            const uint32_t hsize = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
            const TT *lt = table + (int64_t)meta.offsets[l] * 2;
            const LevelPos p = level_pos_xyz(x, y, z, bound, scale);
            uint32_t rows[8];
            corner_rows(p.gx, p.gy, p.gz, res, hsize, rows, meta.blocked);
            // issue the loads first, blend afterwards
            const nt_f2 g = __builtin_nontemporal_load(
                reinterpret_cast<const nt_f2 *>(dfeat + ((int64_t)l * level_stride + m) * 2));
            float2 v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = Feat2<TT>::load(lt, rows[c]);
            // s_c = <dfeat, table[row_c]>; the three partial derivatives share it
            float s[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) s[c] = fmaf(g.y, v[c].y, g.x * v[c].x);
            const float ux = 1.0f - p.fx, uy = 1.0f - p.fy, uz = 1.0f - p.fz;
            // differences along x of the four (y, z) edges, along y of the four (x, z) edges, along z of the (x, y) ones
            float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b0 = k & 1, b1 = (k >> 1) & 1;
                // x: corners (0, b0, b1) and (1, b0, b1); weight wy(b0) wz(b1)
                ax = fmaf((b0 ? p.fy : uy) * (b1 ? p.fz : uz), s[1 + 2 * b0 + 4 * b1] - s[2 * b0 + 4 * b1], ax);
                // y: corners (b0, 0, b1) and (b0, 1, b1); weight wx(b0) wz(b1)
                ay = fmaf((b0 ? p.fx : ux) * (b1 ? p.fz : uz), s[b0 + 2 + 4 * b1] - s[b0 + 4 * b1], ay);
                // z: corners (b0, b1, 0) and (b0, b1, 1); weight wx(b0) wy(b1)
                az = fmaf((b0 ? p.fx : ux) * (b1 ? p.fy : uy), s[b0 + 2 * b1 + 4] - s[b0 + 2 * b1], az);
            }
            const float k = scale / two_b;
            dx = fmaf(k, ax, dx);
            dy = fmaf(k, ay, dy);
            dz = fmaf(k, az, dz);
        }
        dxyz[m * 3] = dx;
        dxyz[m * 3 + 1] = dy;
        dxyz[m * 3 + 2] = dz;
    }
}

// grad sigma = dxyz_enc + e grad blob(x), normal = -safe_normalize(grad sigma)
__global__ void __launch_bounds__(256)
k_density_normals(const float *__restrict__ dxyz_enc, const float *__restrict__ xyzs, const float *__restrict__ sigmas,
                  float blob_scale, float blob_denom, int64_t m_host, const int32_t *__restrict__ m_dev,
                  float *__restrict__ grad_sigma, float *__restrict__ normals) {
    const int64_t M = valid_count(m_host, m_dev);
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const float x = xyzs[m * 3], y = xyzs[m * 3 + 1], z = xyzs[m * 3 + 2];
        const float d2 = (x * x + y * y) + z * z;
        const float e = trunc_exp_grad(sigmas[m]);   // (the MLP backward's d sigma / d z)
        const float b = blob_scale * expf(-d2 / blob_denom);   // (= blob_of: the forward's value)
        const float eb = e * b;
        const float gx = fmaf(eb, -2.0f * x / blob_denom, dxyz_enc[m * 3]);
        const float gy = fmaf(eb, -2.0f * y / blob_denom, dxyz_enc[m * 3 + 1]);
        const float gz = fmaf(eb, -2.0f * z / blob_denom, dxyz_enc[m * 3 + 2]);
        if (grad_sigma) {
            grad_sigma[m * 3] = gx; grad_sigma[m * 3 + 1] = gy; grad_sigma[m * 3 + 2] = gz;
        }
        if (normals) {
            const float n2 = (gx * gx + gy * gy) + gz * gz;
            const float r = sqrtf(fmaxf(n2, 1e-20f));
            float nx = -gx / r, ny = -gy / r, nz = -gz / r;
            nx = nx != nx ? 0.f : nx; ny = ny != ny ? 0.f : ny; nz = nz != nz ? 0.f : nz;
            normals[m * 3] = nx; normals[m * 3 + 1] = ny; normals[m * 3 + 2] = nz;
        }
    }
}

static unsigned stream_blocks(int64_t m_host) {
    int64_t b = div_up(m_host, 256);
    return (unsigned)(b > 16384 ? 16384 : b);
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_grid_encode_backward_input(const float *xyzs, float bound, const void *table, int table_dtype, int num_levels,
                                     int level_dim, const int32_t *offsets_host, const float *scales_host,
                                     const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                                     const float *dfeat, float *dxyz, int variant, lnerf_stream_t stream) {
    GridMeta meta;
    const int layout = variant & (LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    variant &= ~(LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    int rc = fill_meta("grid_encode_backward_input", meta, num_levels, level_dim, offsets_host, scales_host, res_host,
                       layout);
    if (rc) return rc;
    LNERF_REQUIRE(m_host >= 0 && level_stride >= m_host, "grid_encode_backward_input: need 0 <= m_host <= level_stride");
    LNERF_REQUIRE(bound > 0.f, "grid_encode_backward_input: bound must be > 0");
    LNERF_REQUIRE(variant == 0, "grid_encode_backward_input: unknown variant %d", variant);
    LNERF_REQUIRE(table_dtype == LNERF_F32 || table_dtype == LNERF_BF16, "grid_encode_backward_input: bad dtype tag");
    if (m_host == 0) return LNERF_OK;
    LNERF_REQUIRE(xyzs && table && dfeat && dxyz, "grid_encode_backward_input: null pointer");
    const dim3 grid(stream_blocks(m_host));
    hipStream_t s = as_stream(stream);
    if (table_dtype == LNERF_F32)
        hipLaunchKernelGGL((k_grid_backward_input<float>), grid, dim3(256), 0, s, xyzs, bound, (const float *)table, meta,
                           m_host, m_dev, level_stride, dfeat, dxyz);
    else
        hipLaunchKernelGGL((k_grid_backward_input<uint16_t>), grid, dim3(256), 0, s, xyzs, bound, (const uint16_t *)table,
                           meta, m_host, m_dev, level_stride, dfeat, dxyz);
    LNERF_CHECK_LAUNCH("grid_encode_backward_input");
    return LNERF_OK;
}

int lnerf_density_normals(const float *dxyz_enc, const float *xyzs, const float *sigmas, float blob_scale,
                          float blob_std, int64_t m_host, const int32_t *m_dev, float *grad_sigma, float *normals,
                          lnerf_stream_t stream) {
    LNERF_REQUIRE(m_host >= 0, "density_normals: m_host must be >= 0");
    LNERF_REQUIRE(blob_std > 0.f, "density_normals: blob_std must be > 0");
    if (m_host == 0 || (!grad_sigma && !normals)) return LNERF_OK;
    LNERF_REQUIRE(dxyz_enc && xyzs && sigmas, "density_normals: null pointer");
    hipLaunchKernelGGL(k_density_normals, dim3(stream_blocks(m_host)), dim3(256), 0, as_stream(stream), dxyz_enc, xyzs,
                       sigmas, blob_scale, 2.0f * blob_std * blob_std, m_host, m_dev, grad_sigma, normals);
    LNERF_CHECK_LAUNCH("density_normals");
    return LNERF_OK;
}

}  // extern "C"
