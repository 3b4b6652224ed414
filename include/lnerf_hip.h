/* lnerf_hip.h -- C ABI of the MI355X (gfx950) latent-NeRF render kernels.
 *
 * This is the drop-in boundary of the hot path named by BASELINE.json `north_star`
 * (SURVEY.md §8): everything `NeRFRenderer.render()/run_cuda()` needs per optimisation step.
 * The reference checkout calls this path at scripts/train_latent_nerf.py:3-4,10-14
 * (`from src.latent_nerf... import Trainer` -> trainer -> renderer) but does not contain it
 * (README.md:152-156 lists `src/latent_nerf/raymarching`, "The CUDA ray marching modules");
 * each entry point below names the extension op of that absent module it stands in for, as
 * enumerated in SURVEY.md §8(b).  The caller-side contract that IS present in the reference --
 * the renderer hands the trainer `{'image': [B,4,H,W]}` and receives the SDS gradient through
 * `pred.backward(gradient=grad)` -- is src/latent_paint/models/textured_mesh.py:181-220 and
 * src/latent_paint_mesh/training/trainer.py:657-658; the Python host side above this ABI
 * (latent-nerf-test_amd/src/latent_nerf) honours it.
 *
 * Conventions
 *   - plain C: device pointers, sizes, a stream handle.  No torch types.  All pointers are
 *     DEVICE pointers unless the name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every call only
 *     enqueues work; none synchronises, allocates or frees (all are hipGraph-capturable).
 *   - return value: LNERF_OK (0) or a negative LNERF_ERR_*; lnerf_last_error() gives a
 *     thread-local message.  Arguments are validated on the host before any launch.
 *   - data-dependent sizes (the number of samples M a march produced) stay on the device:
 *     kernels that consume samples take `m_host` (an upper bound, usually the buffer
 *     capacity) and an optional device pointer `m_dev`; they process min(m_host, *m_dev).
 *   - sample-major feature tensors are stored LEVEL-MAJOR: feat[(l*F+f)] lives at
 *     base + (l * level_stride + m) * F + f  (F = 2), so every wave writes/reads 512 contiguous
 *     bytes per level.  `level_stride` is in samples (normally the buffer capacity).
 */
#ifndef LNERF_HIP_H
#define LNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNERF_ABI_VERSION 7

#define LNERF_OK 0
#define LNERF_ERR_INVALID_ARG (-1)
#define LNERF_ERR_HIP (-2)
#define LNERF_ERR_UNSUPPORTED (-3)

/* dtype tags for `void*` tensors */
#define LNERF_F32 0
#define LNERF_BF16 1

#define LNERF_MAX_LEVELS 32

typedef void *lnerf_stream_t;

int lnerf_abi_version(void);
const char *lnerf_last_error(void);
/* "gfx950;<git or build tag>" -- lets the host side assert what it loaded */
const char *lnerf_build_info(void);

/* Performance knobs (never change results beyond float summation order).  Keys:
 *   "scatter_compact_max_res": levels with resolution <= value merge per-wavefront runs of samples in one cell
 *                              before binning (default 512).
 *   "scatter_bin_per_cu":      persistent workgroups of the binning pass per CU, 1 .. 4 (default 3).
 *   "scatter_bin_wgs":         persistent workgroups of the binning pass (default 0 = 256 x scatter_bin_per_cu).
 *   "scatter_skip_zero":       1 (default) = contributions that are exactly zero are not binned.
 *   "scatter_reduce_threads":  threads per workgroup of the reduce pass, 512 or 1024 (default 1024).
 *   "gather_pair_loads":       0 = one load per vertex; 1 = x-adjacent vertices with one load where they are adjacent rows
 *                              (dense levels, inside a block of the blocked layout, aligned pairs of the vertex hash);
 *                              2 (default) = additionally one aligned 16-byte load per 4-row group of a bf16 table
 *                              (vertex hash).
 *   "gather_dedup_max_res":    levels with resolution <= value fetch a cell's 8 vertices once per run of
 *                              lanes (consecutive samples of a ray) in that cell (default 512; 0 = off).
 *   "gather_lds_pad":          experiment knob: bytes of unused dynamic LDS per gather workgroup, 0 .. 65536 (default 0).
 *   "scatter_level_groups":    experiment knob: bin + reduce per level group, 1 .. 32 (default 1); the closing-scatter form refuses > 1.
 *   "mlp_fwd_blocks":          persistent workgroups of the bf16 MLP forward (default 768).
 *   "mlp_fwd_wps":             wavefronts per SIMD the bf16 forward is compiled for, 3 (default) or 2.
 *   "mlp_bwd_blocks":          persistent workgroups of the MLP backward (default and maximum 512 = slab count).
 * and two switches between two forms of the same result (any value is taken as on / off):
 *   "adam_skip":               1 (default) = the fused table update leaves 16-row groups with all-zero moments and zero
 *                              gradient alone where a moment map is bound (lnerf_moment_map_bind); 0 = the map is still
 *                              maintained, every group takes the step.  Bit-identical either way.
 *   "adam_consts":             1 (default) = launches on a device step counter with a bound record
 *                              (lnerf_adam_constants_bind) publish and read the step's bias corrections; 0 = every
 *                              lane computes them from the counter, the record is neither read nor written.
 *                              Bit-identical either way.
 */
int lnerf_set_tuning(const char *key, int value);

/* ---- H1: ray generation (absent upstream: `get_rays` of nerf_utils; camera convention
 * src/latent_paint/models/render.py:19-31).  c2w [B,4,4] row-major, columns (right,down,forward,eye).
 * rays_o, rays_d [B, H*W, 3]. */
int lnerf_get_rays(const float *c2w, int B, int H, int W, float fx, float fy, float cx, float cy,
                   float *rays_o, float *rays_d, lnerf_stream_t stream);

/* ---- H2: `raymarching.near_far_from_aabb`.  aabb = (xmin,ymin,zmin,xmax,ymax,zmax) by value.
 * Misses get near = far = FLT_MAX. */
int lnerf_near_far_from_aabb(const float *rays_o, const float *rays_d, int64_t N, float xmin, float ymin, float zmin,
                             float xmax, float ymax, float zmax, float min_near, float *nears, float *fars,
                             lnerf_stream_t stream);

/* ---- H3: `raymarching.morton3D`, `morton3D_invert`, `packbits`. */
int lnerf_morton3d(const int32_t *coords, int64_t n, uint32_t *indices, lnerf_stream_t stream);
int lnerf_morton3d_invert(const uint32_t *indices, int64_t n, int32_t *coords, lnerf_stream_t stream);
/* bit k of byte b = grid[8b+k] > min(thresh, *mean_dev)  (mean_dev may be NULL) */
int lnerf_packbits(const float *grid, int64_t n_cells, float thresh, const float *mean_dev, uint8_t *bitfield,
                   lnerf_stream_t stream);

/* ---- H4: `raymarching.march_rays_train`.
 * Two launches up to 8192 rays: per-ray count (one wavefront per ray, ballot + popcount over 64 lattice points at a
 * time), per-ray write (ballot prefix-sum compaction) whose wavefront first sums the counts of the rays before its own;
 * three launches above (count, single-workgroup exclusive scan, write).  Output order is deterministic: samples of ray
 * n follow those of ray n-1.
 *   rays    int32 [N,3]  (ray id, offset, count)
 *   counter int32 [lnerf_march_counter_len(N)]
 *                        [0]=M total samples written, [1]=number of rays with count>0,
 *                        [2]=rays dropped because offset+count exceeded `capacity`,
 *                        [3]=running maximum of  M | (rays dropped ? 2^30 : 0)  over the calls since the CALLER last
 *                        zeroed it (zero it when the buffer is allocated): the peak a training loop sizes its sample
 *                        buffers from, kept without a launch of its own,
 *                        [4 ...) scratch of the call (two-launch form: per-ray counts, per-workgroup sums)
 *   the step, ONE rule for the training march and lnerf_march_rays: dt(t) = fminf(fmaxf(t * dt_gamma, dt_min), dt_max)
 *     with dt_min = 2 sqrt(3) / max_steps and dt_max = 2 sqrt(3) 2^(cascade-1) / grid_size, also at dt_gamma = 0
 *     (the closed-form lattice t_k = t0 + k dt(0), dt(0) computed once on the host).  Where dt_min > dt_max, that is
 *     max_steps < grid_size / 2^(cascade-1), the rule yields dt_max everywhere.
 *   jitter of the march start t0 = near + dt(near) * u_n, one of
 *     noises [N] in [0,1)          the upstream form (`noises = torch.rand(N)`);
 *     noise_counter (device int32) counter-based generator: u_n = hash(n, noise_seed, *noise_counter) in [0,1)
 *                                  (24 bits; the hash is restated in oracle/nerf_oracle.py `march_noise`), and the
 *                                  call advances *noise_counter by one -- fresh jitter on every replay of a
 *                                  captured hipGraph, no host RNG state;
 *     both NULL                    no jitter.
 *   xyzs [capacity,3], dirs [capacity,3], deltas [capacity,2] = (dt, t). */
int64_t lnerf_march_counter_len(int64_t N);
int lnerf_march_rays_train(const float *rays_o, const float *rays_d, const float *nears, const float *fars, int64_t N,
                           const uint8_t *bitfield, float bound, int cascade, int grid_size, int max_steps,
                           float dt_gamma, const float *noises, uint32_t noise_seed, int32_t *noise_counter,
                           int64_t capacity, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                           lnerf_stream_t stream);
/* The same with the AABB clip of lnerf_near_far_from_aabb done inside the two march passes (identical arithmetic):
 * the training path of `NeRFRenderer.run_cuda` (SURVEY.md §8(a) H2 -> H4, line 465) calls near_far_from_aabb only
 * to feed march_rays_train, and in a replayed graph every dispatch of a few thousand rays costs ~4.5 us whatever it
 * computes. */
int lnerf_march_rays_train_aabb(const float *rays_o, const float *rays_d, float xmin, float ymin, float zmin, float xmax,
                                float ymax, float zmax, float min_near, int64_t N, const uint8_t *bitfield, float bound,
                                int cascade, int grid_size, int max_steps, float dt_gamma, const float *noises,
                                uint32_t noise_seed, int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs,
                                float *deltas, int32_t *rays, int32_t *counter, lnerf_stream_t stream);
/* ... and with the ray generation of lnerf_get_rays folded into the count pass as well (same arithmetic): the rays of B
 * views of H x W pixels are generated, written to rays_o_out / rays_d_out [B*H*W, 3] (the caller's background and
 * direction-dependent heads read them there) and marched.  One more dispatch off the step. */
int lnerf_march_rays_train_pose(const float *c2w, int B, int H, int W, float fx, float fy, float cx, float cy,
                                float *rays_o_out, float *rays_d_out, float xmin, float ymin, float zmin, float xmax,
                                float ymax, float zmax, float min_near, const uint8_t *bitfield, float bound, int cascade,
                                int grid_size, int max_steps, float dt_gamma, const float *noises, uint32_t noise_seed,
                                int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs, float *deltas,
                                int32_t *rays, int32_t *counter, lnerf_stream_t stream);
/* The same with the intrinsics in DEVICE memory: intrinsics f32 [B,4] = (fx, fy, cx, cy) per view.  Nothing about the
 * camera is baked into the launch, so a captured hipGraph renders whatever pose / field of view its caller copied into
 * `c2w` / `intrinsics` before the replay (the trainer's graphed step: a new random view every step). */
int lnerf_march_rays_train_camera(const float *c2w, const float *intrinsics, int B, int H, int W, float *rays_o_out,
                                  float *rays_d_out, float xmin, float ymin, float zmin, float xmax, float ymax,
                                  float zmax, float min_near, const uint8_t *bitfield, float bound, int cascade,
                                  int grid_size, int max_steps, float dt_gamma, const float *noises, uint32_t noise_seed,
                                  int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs, float *deltas,
                                  int32_t *rays, int32_t *counter, lnerf_stream_t stream);

/* ---- H4 (inference): `raymarching.march_rays` / `composite_rays` and the live-ray compaction
 * the upstream renderer does on the host (`rays_alive = rays_alive[rays_alive >= 0]`). */
int lnerf_march_rays(int64_t n_alive, int n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                     const float *rays_d, const float *fars, const uint8_t *bitfield, float bound, int cascade,
                     int grid_size, int max_steps, float dt_gamma, float *xyzs, float *dirs, float *deltas,
                     lnerf_stream_t stream);
int lnerf_composite_rays(int64_t n_alive, int n_step, int32_t *rays_alive, float *rays_t, const float *sigmas,
                         const float *rgbs, const float *deltas, int C, float T_thresh, float *weights_sum,
                         float *depth, float *image, float *transmittance, lnerf_stream_t stream);
/* alive_out[0..n) = entries of alive_in that are >= 0, order preserved; n -> *n_alive_dev.
 * Wave ballot + prefix-sum compaction, one launch. */
int lnerf_compact_rays(const int32_t *alive_in, int64_t n, int32_t *alive_out, int32_t *n_alive_dev,
                       lnerf_stream_t stream);

/* ---- H5/H6: `gridencoder.grid_encode_forward/backward` (multiresolution hash grid, F = 2).
 * Level metadata is passed from the host (num_levels <= LNERF_MAX_LEVELS):
 *   offsets_host [L+1] row offsets, scales_host [L] per-level scale, res_host [L] resolution.
 * xyzs are world positions; the kernels normalise x01 = (x + bound) / (2*bound).
 * `variant` must be 0 (level on blockIdx.y), optionally with the layout flags LNERF_GRID_BLOCKED / LNERF_GRID_TILED.
 * The forward kernel keeps sample indices and byte offsets into a level in 32 bits: m_host < 2^31, and a level has at
 * most 2^30 rows with a bf16 table, 2^29 with an f32 table (4 GiB); anything larger is refused. */
int lnerf_grid_encode_forward(const float *xyzs, float bound, const void *table, int table_dtype, int num_levels,
                              int level_dim, const int32_t *offsets_host, const float *scales_host,
                              const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                              void *feat, int feat_dtype, int variant, lnerf_stream_t stream);
/* dtable (f32, [rows, F]) is ACCUMULATED into (+=).
 * variant 0/1: per-lane global float atomics (blockIdx.y level map / XCD-aware map); no workspace.
 * variant 2  : two-pass bucketed scatter -- records binned per 64 KiB table chunk with plain
 *              stores, then reduced in LDS in 64-bit fixed point and added with coalesced stores
 *              (heavily loaded coarse chunks are cut into slices whose exact integer partial sums the
 *              slice that finishes last adds up): the sums do not depend on execution order, the
 *              gradient is bitwise reproducible.  Needs `workspace` of
 *              lnerf_grid_encode_backward_workspace_bytes() bytes (16-byte aligned) whose first
 *              LNERF_SCATTER_ZERO_HEAD_BYTES were zero when it was FIRST used (arrival counters that
 *              every call leaves zero again; the rest may hold anything).
 * variant 3  : variant 2 with packed 8-byte records (12-bit row inside the bucket + two values rounded
 *              to 26-bit floats, 17 mantissa bits): a third less record traffic, relative rounding
 *              2^-18 per addend; same workspace.
 * Variants 2 / 3, numeric contract (DESIGN.md "Numeric contract of the bucketed scatter"; tested in
 * tests/test_gpu_scatter_numerics.py): every row is within a derived bound of the exact sum of its f32 addends; the
 * result scales bit for bit with a power-of-two scaling of dfeat; a level's rows depend on that level's gradients
 * only, and on nothing a previous call left in the workspace.
 * NON-FINITE dfeat (NaN, +-inf): the call returns normally, the result is reproducible, and every OTHER level is bit
 * for bit what it is without the value.  What the rows of the level that holds the value contain is UNSPECIFIED INSIDE
 * THAT LEVEL: pass 1 raises the level's bound to 3e38, so the level's finite addends are quantised to 2^-44 (2^-30) of
 * 2^128 and come out as zero, and the non-finite addend goes through a float -> integer conversion that is not defined
 * for it.  Observed on an MI355X: a NaN converts to 0, so the whole level reads zero; +-inf leaves +-inf in the 8 rows of
 * its sample with 8-byte records and -+2^116 there with 12-byte records, the rest of the level zero.  This is tolerable
 * because the MLP's own gradients are non-finite in the same step: the failure is loud anyway. */
#define LNERF_SCATTER_ZERO_HEAD_BYTES (64 * 1024)
size_t lnerf_grid_encode_backward_workspace_bytes(int num_levels, const int32_t *offsets_host, int64_t m_host);
/* The first lnerf_grid_scatter_clear_bytes() bytes of that workspace (bucket cursors, level maxima) are cleared by every
 * bucketed scatter call with a fill dispatch of its own -- ~5 us in a replayed graph for a few KiB.  A caller that
 * launches something right before the scatter anyway can clear them there (lnerf_mlp_backward takes such a region)
 * and pass `variant | LNERF_SCATTER_CLEARED`. */
#define LNERF_SCATTER_CLEARED 0x100
/* variant | LNERF_GRID_BLOCKED (forward AND backward entry points, consistently): an opt-in layout of the HASHED levels
 * (not Instant-NGP's): the vertex lattice is cut into blocks of 4 x 2 x 2, the block coordinate is hashed and the 16 rows
 * of a block are consecutive: row = (hash(x >> 2, y >> 1, z >> 1) mod (rows / 16)) * 16 + (x & 3) + 4 (y & 1) + 8 (z & 1).
 * One block = one 64-byte line of the bf16 table: a sample's 8 vertices touch 2.8 lines on average instead of 4.25.
 * Dense levels are unchanged.  Restated in oracle/nerf_oracle.py (grid_corner_indices(blocked=True)). */
#define LNERF_GRID_BLOCKED 0x400
/* variant | LNERF_GRID_TILED (forward AND backward entry points, consistently; not together with LNERF_GRID_BLOCKED): the
 * upstream encoder's `gridtype = "tiled"` -- a level too large for its table wraps its dense index,
 * row = (x + y (res + 1) + z (res + 1)^2 mod 2^32) mod rows, instead of hashing the vertex.  Restated in
 * oracle/nerf_oracle.py (grid_corner_indices(layout="tiled")). */
#define LNERF_GRID_TILED 0x800
/* variant | LNERF_SCATTER_DEFER_FINISH: accepted and ignored (ABI 4 deferred a separate finishing pass of the sliced
 * buckets to lnerf_step_tail; pass 2 finishes them itself now). */
#define LNERF_SCATTER_DEFER_FINISH 0x200
size_t lnerf_grid_scatter_clear_bytes(int num_levels, const int32_t *offsets_host, int64_t m_host);
int lnerf_grid_encode_backward(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                               int level_dim, const int32_t *offsets_host, const float *scales_host,
                               const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                               float *dtable, int variant, void *workspace, size_t workspace_bytes,
                               lnerf_stream_t stream);
/* Backward of the hash grid with the gradient WRITTEN (not accumulated) as bf16 pairs, the wire format of
 * the data-parallel all-reduce: `grad_bf16` ([rows, 2] bf16) needs no zero fill and every row is written
 * exactly once by the kernel that finishes its sum -- no read-modify-write of an f32 table gradient and no
 * cast afterwards.  variant 2 or 3.  `dtable_zero` (f32 [rows, 2]) only carries the records of overflowing
 * buckets; it must be ZERO on entry and is zero again on return. */
int lnerf_grid_encode_backward_bf16(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                    int level_dim, const int32_t *offsets_host, const float *scales_host,
                                    const int32_t *res_host, int64_t m_host, const int32_t *m_dev,
                                    int64_t level_stride, float *dtable_zero, int variant, void *workspace,
                                    size_t workspace_bytes, void *grad_bf16, lnerf_stream_t stream);
/* Split form of lnerf_grid_encode_backward_bf16 for a PIPELINED data-parallel exchange: pass 1 once for all levels
 * (lnerf_grid_scatter_bin; clears the level maxima), then pass 2 per level range
 * (lnerf_grid_scatter_reduce_bf16: writes rows offsets[level_lo] .. offsets[level_hi] of grad_bf16), so that the
 * all-reduce of a level group can be launched while the next group is still being summed.  Same workspace, same
 * arithmetic, same bits as the one-call form. */
int lnerf_grid_scatter_bin(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                           int level_dim, const int32_t *offsets_host, const float *scales_host, const int32_t *res_host,
                           int64_t m_host, const int32_t *m_dev, int64_t level_stride, float *dtable_zero, int variant,
                           void *workspace, size_t workspace_bytes, lnerf_stream_t stream);
int lnerf_grid_scatter_reduce_bf16(float bound, int num_levels, int level_dim, const int32_t *offsets_host,
                                   const float *scales_host, const int32_t *res_host, int64_t m_host,
                                   int64_t level_stride, int level_lo, int level_hi, float *dtable_zero, int variant,
                                   void *workspace, size_t workspace_bytes, void *grad_bf16, lnerf_stream_t stream);

/* Backward of the hash grid fused with the table's optimiser step (single-GPU training: no gradient
 * exchange sits between the two).  Same scatter as above (variant 2 or 3), but the kernel that
 * finishes a row's sum (pass 2: a bucket's only workgroup, or the last of its slices to arrive) applies
 * Adam(beta1, beta2, eps) to it straight from the fixed-point sum -- `table`, `exp_avg`, `exp_avg_sq`
 * (f32 [rows, 2]) and the optional bf16 `shadow_bf16` are updated in place and the gradient never
 * reaches HBM.  `dtable_zero` (f32 [rows, 2]) only carries the records of overflowing buckets; it
 * must be ZERO on entry and is zero again on return.  Arithmetic and results are bit-identical to
 * lnerf_grid_encode_backward + lnerf_adam_step (one shared definition).
 * Covers `optimizer.zero_grad() ... optimizer.step()` of src/latent_paint/training/trainer.py:127-131
 * for the table parameter only. */
int lnerf_grid_encode_backward_adam(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                    int level_dim, const int32_t *offsets_host, const float *scales_host,
                                    const int32_t *res_host, int64_t m_host, const int32_t *m_dev,
                                    int64_t level_stride, float *dtable_zero, int variant, void *workspace,
                                    size_t workspace_bytes, float *table, float *exp_avg, float *exp_avg_sq,
                                    void *shadow_bf16, float lr, float beta1, float beta2, float eps, int step,
                                    const int32_t *step_dev, float grad_scale, lnerf_stream_t stream);

/* Gradient of the hash-grid features with respect to the sample POSITION (the upstream encoder's `grid_backward_input`).
 * `dfeat` is f32, level-major [L, level_stride, 2]: exactly what lnerf_mlp_backward writes.  For every row
 * m < min(m_host, *m_dev) the kernel WRITES (does not accumulate)
 *   dxyz[m, a] = sum_l scale_l / (2 bound) * sum_c sum_f dfeat[l, m, f] * table[row_c, f] * d w_c / d frac_a
 * with w_c = (wx wy) wz the forward's corner weight and d w_c / d frac_x = (bx ? +1 : -1) wy wz (likewise y, z); rows at or
 * beyond that limit are not touched.  Cell, fractions and rows are the forward's (one shared definition): on a lattice
 * plane the result is the one-sided derivative of the cell the forward put the sample in.  `table` is the table the
 * forward read (f32 or bf16, table_dtype); `variant` must be 0, optionally with LNERF_GRID_BLOCKED / LNERF_GRID_TILED.
 * One lane per sample sums its levels in the fixed order 0 .. L-1: no atomics, no workspace, bitwise reproducible. */
int lnerf_grid_encode_backward_input(const float *xyzs, float bound, const void *table, int table_dtype, int num_levels,
                                     int level_dim, const int32_t *offsets_host, const float *scales_host,
                                     const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                                     const float *dfeat, float *dxyz, int variant, lnerf_stream_t stream);

/* ---- `gridencoder.grad_total_variation` (the upstream trainers' `lambda_tv`): total-variation regulariser of the hash
 * table itself.  Definition (ours; float64 restatement in tests/tv_reference.py): level l has the vertex lattice
 * [0, res_l]^3; for every SAMPLED vertex p and channel c
 *   dtable[offsets[l] + row_l(p), c] += w_l * sum over q in N(p) of (e_c(p) - e_c(q)),   e(p) = table[offsets[l] + row_l(p)],
 * N(p) = the up to six axis neighbours of p inside the lattice, row_l the level's index function (dense / hash / blocked /
 * tiled).  Only p's own row is written.  With every vertex of the level sampled and w_l = lambda / N_l this is the exact
 * gradient (hash collisions included) of lambda / (2 N_l) * sum over lattice edges |e(p) - e(q)|^2; with n_l vertices sampled
 * and w_l = lambda / n_l its unbiased estimate.
 * The unit of sampling is a LINE: all res_l + 1 vertices that share one (y, z), consecutive lanes = consecutive x.
 *
 * lnerf_grid_tv_plan (HOST ONLY, no device work): line_offsets_host[L + 1], level l takes
 *   n_l = min((res_l + 1)^2, max(1, tv_vertices / (res_l + 1))) lines; tv_vertices in [1, 2^30].
 * lnerf_grid_tv_lines: lines int32 [line_offsets_host[L], 2] = (y, z) of every line.  A level whose plan takes all
 *   (res_l + 1)^2 lines is swept in plane order (line j = plane index j); otherwise line j is drawn from stratum j of the
 *   S = (res_l + 1)^2 plane indices: lo_j = floor(j S / n_l), idx = lo_j + h mod (lo_{j+1} - lo_j) (64-bit integers),
 *   y = idx mod (res_l + 1), z = idx / (res_l + 1), h = the counter-based hash of lnerf_synthetic_guidance / lnerf_occ_sample
 *   keyed by (j, seed, step, l) -- the lines of a level are distinct by construction.  `step_dev` (optional, device int32):
 *   when given, *step_dev replaces `step` (the optimiser's device counter: a replayed hipGraph draws fresh lines).
 * lnerf_grid_tv_grad: `table` is the f32 MASTER table [rows, 2]; `layout_flags` is 0, LNERF_GRID_BLOCKED or LNERF_GRID_TILED;
 *   `lines` as written by lnerf_grid_tv_lines, or NULL: the kernel then draws the very same lines itself from
 *   (seed, step, step_dev) -- one launch.  Given lines outside the lattice are ignored.  weights_host[L]: w_l, finite; a
 *   weight of exactly 0 skips the level.  dtable (f32 [rows, 2]) is ACCUMULATED into; rows of unsampled vertices keep
 *   their bits.
 *   Reproducibility: on a DENSE level the sampled rows are distinct (distinct lines, bijective index; lines passed in must
 *   be distinct there) and are updated by a plain read-modify-write: bitwise reproducible.  On a HASHED level every
 *   contribution is one float atomic add per channel: a row that collects more than one contribution is summed in arrival
 *   order, its last bits may differ from run to run. */
int lnerf_grid_tv_plan(int num_levels, const int32_t *res_host, int64_t tv_vertices, int32_t *line_offsets_host);
int lnerf_grid_tv_lines(int num_levels, const int32_t *res_host, const int32_t *line_offsets_host, uint32_t seed,
                        uint32_t step, const int32_t *step_dev, int32_t *lines, lnerf_stream_t stream);
int lnerf_grid_tv_grad(const float *table, int num_levels, int level_dim, const int32_t *offsets_host,
                       const int32_t *res_host, int layout_flags, const int32_t *line_offsets_host, const int32_t *lines,
                       uint32_t seed, uint32_t step, const int32_t *step_dev, const float *weights_host, float *dtable,
                       lnerf_stream_t stream);

/* ---- H7 helper: inverse of the bf16 weight-fragment layout at the head of the MLP workspace: map_wK[2 i], map_wK[2 i + 1] = the two
 * bf16 elements of that image which hold weight i of wK (forward / transposed fragments).  map_w1 int32[64*32*2],
 * map_w2 int32[64*64*2], map_w3 int32[out_dim*64*2].  For lnerf_adam_step_multi_shadow. */
int lnerf_mlp_fragment_maps(int out_dim, int32_t *map_w1, int32_t *map_w2, int32_t *map_w3, lnerf_stream_t stream);

/* ---- H7: fused sigma/latent MLP  32 -> 64 -> 64 -> out_dim (= 1 + C), ReLU hidden.
 * Weights are PyTorch nn.Linear layout: w1 [64,32], b1 [64], w2 [64,64], b2 [64], w3 [out_dim,64],
 * b3 [out_dim], all f32.  sigma = exp(h0 + blob_scale*exp(-|x|^2/(2 blob_std^2))), rgbs = h[1:].
 * out_dim is 2 .. 8 (anything else: LNERF_ERR_INVALID_ARG); the weight-gradient outputs dw3 / db3 hold out_dim rows and
 * nothing beyond them is written.
 * Rows m < min(m_host, *m_dev) are computed (m_dev may be NULL: m_host rows; *m_dev above m_host counts as m_host).  Rows
 * at or beyond that count are NOT written in sigmas, rgbs and dfeat, and what the inputs hold there (stale samples of
 * an earlier step, NaN included) reaches no output and no gradient.
 * precision: LNERF_F32 -> exact-f32 MFMA (v_mfma_f32_16x16x4_f32), LNERF_BF16 -> bf16 MFMA, f32 acc.
 * level_stride <= 2^24 samples with LNERF_BF16 (32-bit byte offsets inside the bf16 kernels; the exact-f32 kernels take
 * any stride below 2^30); with out_dim == 5 the bf16 path moves the
 * latent rows (rgbs, drgbs: [*, 4] f32) 16 bytes at a time: those buffers must be 16-byte aligned.
 * workspace (optional, 16-byte aligned, >= 36 KiB; the buffer of lnerf_mlp_backward_workspace_bytes() serves): with
 * it the bf16 path builds its weight fragments (the backward's too) once per launch instead of once per workgroup;
 * precision | LNERF_MLP_FRAGMENTS_READY: they are current already (fragment shadow of the optimiser, or an earlier
 * forward with the same weights) -- no build at all. */
int lnerf_mlp_forward(const void *feat, int feat_dtype, int64_t level_stride, const float *xyzs, const float *w1,
                      const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, int out_dim,
                      float blob_scale, float blob_std, int64_t m_host, const int32_t *m_dev, float *sigmas,
                      float *rgbs, int precision, void *workspace, size_t workspace_bytes, lnerf_stream_t stream);
/* Recomputes the hidden activations.  dfeat is written (level-major, f32); the d* parameter gradients
 * are accumulated (accumulate != 0: +=) or overwritten (accumulate == 0) deterministically:
 * per-workgroup partial slabs in `workspace` (lnerf_mlp_backward_workspace_bytes()) followed by one
 * reduction launch that sums them in a fixed order.
 * precision: LNERF_F32 or LNERF_BF16; LNERF_BF16 | LNERF_MLP_FRAGMENTS_READY says that the head of `workspace`
 * still holds the fragments lnerf_mlp_forward built from these very weights (same workspace, no weight update in
 * between), so the backward does not rebuild them.
 * clear_ptr / clear_bytes (may be NULL / 0; 4-byte granular): a small region the slab-reduction launch also zeroes
 * -- e.g. the cursors of the scatter that follows (LNERF_SCATTER_CLEARED): one dispatch less per step. */
#define LNERF_MLP_FRAGMENTS_READY 0x100
/* precision | LNERF_MLP_DEFER_REDUCE: the per-workgroup gradient slabs stay in `workspace` (lnerf_mlp_backward_slabs() of
 * them); the d* outputs are not written (may be NULL), clear_bytes must be 0.  lnerf_step_tail sums the slabs and applies
 * the Adam step of the six tensors. */
#define LNERF_MLP_DEFER_REDUCE 0x200
int lnerf_mlp_backward_slabs(int64_t m_host, int precision);
#define LNERF_MLP_FRAGMENT_BYTES (36 * 1024) /* the bf16 weight-fragment image at the head of the workspace */
size_t lnerf_mlp_backward_workspace_bytes(int out_dim);
int lnerf_mlp_backward(const void *feat, int feat_dtype, int64_t level_stride, const float *xyzs, const float *w1,
                       const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, int out_dim,
                       float blob_scale, float blob_std, int64_t m_host, const int32_t *m_dev, const float *sigmas,
                       const float *dsigmas, const float *drgbs, float *dfeat, float *dw1, float *db1, float *dw2,
                       float *db2, float *dw3, float *db3, int accumulate, void *workspace, size_t workspace_bytes,
                       int precision, void *clear_ptr, size_t clear_bytes, lnerf_stream_t stream);

/* Density gradient and surface normal of the field (the upstream renderer's `normal()`, analytic instead of six finite
 * differences).  `dxyz_enc` [m, 3] is lnerf_grid_encode_backward_input of the `dfeat` that lnerf_mlp_backward produced
 * with dsigmas == 1, drgbs == 0: it already carries the trunc-exp factor e = exp(min(pre, 15)) = min(sigma, exp(15)).
 * This elementwise finish adds the density blob's share and normalises:
 *   grad_sigma = dxyz_enc + e * blob_scale * exp(-|x|^2 / denom) * (-2 x / denom),   denom = (2 blob_std) blob_std
 *   normal     = -grad_sigma / sqrt(max(|grad_sigma|^2, 1e-20)), a NaN component becomes 0   (upstream safe_normalize)
 * for rows m < min(m_host, *m_dev); the other rows are not touched.  grad_sigma and normals (f32 [m, 3]) may each be NULL. */
int lnerf_density_normals(const float *dxyz_enc, const float *xyzs, const float *sigmas, float blob_scale,
                          float blob_std, int64_t m_host, const int32_t *m_dev, float *grad_sigma, float *normals,
                          lnerf_stream_t stream);

/* ---- trainer helper: gradient of the opacity-entropy regulariser of the NeRF trainer (sparsity term) w.r.t.
 * weights_sum [N], in one launch:  L = scale * mean_i H(clamp(ws_i, eps, 1 - eps)),  H(p) = -p log2 p - (1-p) log2(1-p);
 * grad_i = scale / N * (log2(1 - ws_i) - log2 ws_i) for eps <= ws_i <= 1 - eps, else 0.  The result is handed to the
 * compositing backward as grad_weights_sum. */
int lnerf_opacity_entropy_grad(const float *weights_sum, int64_t N, float scale, float eps, float *grad,
                               lnerf_stream_t stream);

/* ---- trainer helper: the SEEDED SYNTHETIC guidance (the stand-in for `grad = diffusion.train_step(text_z, pred)` of the
 * reference's src/stable_diffusion.py:248-334 where no diffusion model is available) and, optionally, the entropy gradient
 * above, in ONE launch and in the renderer's own image layout:
 *   t = t_lo + floor(u (t_hi - t_lo + 1)),  w = weights[t]   (weights f32 [>= t_hi + 1]: sqrt(a_t)(1 - a_t), :274, :320)
 *   grad_image[v, p, c] = w * (noise_scale * z + (image[v, p, c] - targets[dirs[v], p, c]))
 * image / grad_image f32 [n_views, rays_per_view, C]; targets f32 [n_buckets, rays_per_view, C]; dirs int32 [n_views]
 * (clamped into range).  u and the normal deviates z come from a counter-based generator of (seed, *step_dev, element)
 * -- *step_dev is only read (the optimiser's device step counter: it advances once per step), so a replayed hipGraph
 * draws fresh noise without host RNG state.  grad_weights_sum != NULL: also lnerf_opacity_entropy_grad over
 * weights_sum [n_views * rays_per_view].  Restated in oracle/nerf_oracle.py synthetic_guidance(). */
int lnerf_synthetic_guidance(const float *image, const float *targets, const int32_t *dirs, const float *weights,
                             int64_t n_views, int rays_per_view, int C, int n_buckets, int t_lo, int t_hi,
                             float noise_scale, uint32_t seed, const int32_t *step_dev, float *grad_image,
                             const float *weights_sum, float ent_scale, float ent_eps, float *grad_weights_sum,
                             lnerf_stream_t stream);

/* ---- H8/H9: `raymarching.composite_rays_train_forward/backward`.  One wavefront per ray,
 * log-space prefix scan of sigma*dt across lanes.  C = colour channels (3 or 4).
 * bg_color [N,C] or NULL: image += (1 - weights_sum) * bg.
 *
 * THE COMPOSITING WEIGHT (csrc/span_walk.h, span_weight: one definition, which every op below that weights samples
 * "as the compositing does" calls).  For ray r with (id, off, cnt) = rays[r], sample s = off + i, i < cnt, front to back,
 * on a density sigma (an op that takes density_scale says so: sigma = density_scale * its density):
 *     tau = sigma * dt (dt = deltas[s][0]), 64-lane inclusive scan of tau with a scalar carry between the chunks of 64,
 *     excl = (the previous lane's inclusive sum; lane 0: 0) + carry -- never inc - tau --, T = expf(-excl),
 *     e = expf(-tau),   alpha = 1 - e,   live = T >= T_thresh,   w = live ? alpha * T : 0,   T e = T_{i+1}.
 *   Nothing is clamped: a NaN T is not live, behind the first T < T_thresh every w is 0 (T falls along the ray).  The
 *   weight itself has no early stop.  The compositing stops reading a ray there (weights_sum, depth, image are sums of the
 *   live samples; the backward writes zeros behind it); the regularisers walk on, because every sample still gets its rows.
 *   expf and the scan are tolerance-checked, not restated bit for bit.
 *   weights_sum = sum_i w_i,  depth = sum_i w_i t_i,  image_c = sum_i w_i rgb_ic. */
int lnerf_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                       const int32_t *rays, int64_t N, int C, float T_thresh, const float *bg_color,
                                       float *weights_sum, float *depth, float *image, lnerf_stream_t stream);
/* grad_weights_sum / grad_depth / grad_bg may be NULL.  grad_sigmas [.], grad_rgbs [.,C] are
 * written for every sample inside a ray's span (zeros after early termination). */
int lnerf_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_depth,
                                        const float *grad_image, const float *sigmas, const float *rgbs,
                                        const float *deltas, const int32_t *rays, const float *weights_sum,
                                        const float *depth, const float *image, const float *bg_color, int64_t N,
                                        int C, float T_thresh, float *grad_sigmas, float *grad_rgbs, float *grad_bg,
                                        lnerf_stream_t stream);

/* ---- RGB refinement stage (render.nerf_type = latent_tune): the C = 4 compositing above with a linear latent -> RGB
 * decoder D (f32 [3][4], row-major `decoder[12]`, no bias) behind it.  Per sample c_k = (D z_k + 1) / 2, no clamp; the
 * kernels compute the per-ray regrouping of the same sum:
 *   latent_image = sum_k w_k z_k  (no background),   image = (D latent_image + ws) / 2 + (1 - ws) bg_color
 * bg_color is RGB, [N,3] or NULL.  latents, latent_image (and grad_latents) must be 16-byte aligned. */
int lnerf_composite_rays_train_decode_forward(const float *sigmas, const float *latents, const float *deltas,
                                              const int32_t *rays, int64_t N, float T_thresh, const float *decoder,
                                              const float *bg_color, float *weights_sum, float *depth,
                                              float *latent_image, float *image, lnerf_stream_t stream);
/* grad_weights_sum / grad_depth / grad_bg may be NULL; grad_image is [N,3].  grad_sigmas [.], grad_latents [.,4] as in
 * lnerf_composite_rays_train_backward.  grad_decoder[c][j] = 1/2 sum_rays grad_image[.][c] latent_image[.][j] is
 * OVERWRITTEN, by a second launch of one workgroup that adds in a fixed order: the same bits on every run. */
int lnerf_composite_rays_train_decode_backward(const float *grad_weights_sum, const float *grad_depth,
                                               const float *grad_image, const float *sigmas, const float *latents,
                                               const float *deltas, const int32_t *rays, const float *weights_sum,
                                               const float *depth, const float *latent_image, const float *decoder,
                                               const float *bg_color, int64_t N, float T_thresh, float *grad_sigmas,
                                               float *grad_latents, float *grad_bg, float *grad_decoder,
                                               lnerf_stream_t stream);
/* The same epilogue per pixel, for the inference loop (which composites the 4 latent channels with lnerf_composite_rays):
 * image [N,3] from latent_image [N,4] and weights_sum [N].  Forward only. */
int lnerf_decode_image(const float *latent_image, const float *weights_sum, const float *decoder, const float *bg_color,
                       int64_t N, float *image, lnerf_stream_t stream);

/* ---- H10: occupancy grid refresh pieces (`update_extra_state`): cell sample points,
 * decayed max update, mean, then lnerf_packbits.  Update and mean are ORDER-INDEPENDENT (replicas of a data-parallel
 * run refresh their grids redundantly and must stay bit-identical): a cell listed several times takes the maximum of
 * its new densities, the mean is summed in a fixed order. */
int lnerf_occ_cell_points(const uint32_t *indices, int64_t n, int cascade_level, int grid_size, float bound,
                          const float *noise, float *xyzs, lnerf_stream_t stream);
/* Steady-state cell sampling of the refresh, on the device: indices [2*n_rand] = n_rand random cells followed by n_rand
 * cells of the occupied ones (grid > 0; of all cells when none is), xyzs [2*n_rand, 3] = a jittered point in each (the
 * formula of lnerf_occ_cell_points).  The draws are STRATIFIED (ABI 7): draw j of a half takes one element, uniformly, from
 * the j-th of n_rand equal strata of its population (the cells in Morton order; the ascending list of occupied cells) --
 * the marginal probabilities of independent draws, ascending output, neighbouring cells on neighbouring lanes of the
 * density query that follows.  Random numbers: u = hash(i, seed, step, k), restated in oracle/nerf_oracle.py `occ_sample`.  The occupied list is built in ascending cell order and its length never visits
 * the host (the upstream form synchronises on torch.nonzero).  scratch: lnerf_occ_sample_scratch_bytes(n_cells). */
size_t lnerf_occ_sample_scratch_bytes(int64_t n_cells);
int lnerf_occ_sample(const float *grid_level, int64_t n_cells, int cascade_level, int grid_size, float bound,
                     int64_t n_rand, uint32_t seed, uint32_t step, int32_t *scratch, uint32_t *indices, float *xyzs,
                     lnerf_stream_t stream);
/* grid[idx] = max(grid[idx] * decay, max of the new_sigmas listed for idx) for every listed cell with a new density
 * >= 0 (cells holding a negative value are never updated).  indices == NULL means cells 0..n-1.  scratch_cells: one
 * uint32 per cell of the level, all zero on entry; left all zero. */
int lnerf_occ_update(float *grid_level, const uint32_t *indices, int64_t n, const float *new_sigmas, float decay,
                     uint32_t *scratch_cells, lnerf_stream_t stream);
/* mean of max(grid,0) over n cells -> *mean_dev ; scratch256: 256 floats of device scratch */
/* lnerf_occ_update + lnerf_occ_mean of ONE cascade level in three launches instead of four, the apply pass streaming over
 * the CELLS (n_cells) instead of exchanging one scratch word per candidate: same grid, same mean, bit for bit.  For a
 * renderer with a single cascade (bound <= 1). */
int lnerf_occ_update_mean(float *grid_level, int64_t n_cells, const uint32_t *indices, int64_t n, const float *new_sigmas,
                          float decay, uint32_t *scratch_cells, float *mean_dev, float *scratch256,
                          lnerf_stream_t stream);
int lnerf_occ_mean(const float *grid, int64_t n, float *mean_dev, float *scratch256, lnerf_stream_t stream);

/* ---- H11: background net, frequency encoding (degree 6: 39 dims) -> 64 -> C (1..4), one thread per ray.
 * out [N,C] is overwritten.  lnerf_bg_backward ACCUMULATES: it adds the gradients of the N rays to what dw1 [64,39],
 * db1 [64], dw2 [C,64], db2 [C] hold (atomic adds per 64-ray tile), so the caller zeroes them for a plain gradient. */
int lnerf_bg_forward(const float *dirs, int64_t N, const float *w1, const float *b1, const float *w2, const float *b2,
                     int C, float *out, lnerf_stream_t stream);
int lnerf_bg_backward(const float *dirs, int64_t N, const float *w1, const float *b1, const float *w2, const float *b2,
                      int C, const float *dout, float *dw1, float *db1, float *dw2, float *db2, lnerf_stream_t stream);

/* ---- sketch-shape guidance (the reference names igl's winding number, README.md:119-122).
 * triangles [F, 3, 3] f32 (vertex positions), points [n,3].  Brute force with LDS-tiled triangles; meant for a
 * one-off evaluation on a dense grid.
 * Zero-area triangles (marching-cubes output has them where a lattice value equals the iso level):
 * lnerf_mesh_distance counts one as its segments, a == b == c as the point a; lnerf_mesh_winding_number gives it the
 * solid angle 0 at every point off that segment (its triple product vanishes).  lnerf_mesh_winding_number accepts n_faces == 0 (out = 0);
 * lnerf_mesh_distance needs n_faces >= 1.  n == 0 writes nothing; out [n] is written and nothing behind it. */
int lnerf_mesh_winding_number(const float *points, int64_t n, const float *triangles, int n_faces, float *out,
                              lnerf_stream_t stream);
int lnerf_mesh_distance(const float *points, int64_t n, const float *triangles, int n_faces, float *out,
                        lnerf_stream_t stream);

/* ---- Latent-Paint raster path (the kaolin calls of src/latent_paint/models/render.py:34-69).
 * cam_host: 14 host floats = world->camera rotation rows (9), camera position (3), fx, fy (= 1/tan(fov/2)).
 * prepare_vertices -> face_z [F,3] (camera z), face_xy [F,3,2] (NDC);  rasterize -> face_idx [H*W] (-1 =
 * background) and perspective-correct barycentrics [H*W,3];  interpolate_attributes: per-face-vertex
 * attributes [F,3,D] -> [H*W,D] (differentiable w.r.t. the attributes);  texture_map: tex [C,R,R] sampled at
 * uv [H*W,2] with grid_sample(align_corners=False, padding 'border') semantics on (u, 1-v), mode 0 nearest /
 * 1 bilinear / 2 bicubic (A = -0.75, every tap clamped to the border) = `guide.texture_interpolation_mode` of
 * src/latent_paint/configs/train_config.py:42-43; pixels with face_idx < 0 give 0.  The backward entry points
 * ACCUMULATE (+=). */
int lnerf_raster_prepare(const float *verts, int n_verts, const int32_t *faces, int n_faces, const float *cam_host,
                         float *face_z, float *face_xy, lnerf_stream_t stream);
int lnerf_rasterize(int H, int W, const float *face_z, const float *face_xy, int n_faces, int32_t *face_idx,
                    float *bary, lnerf_stream_t stream);
/* ---- B views per call on a tile-culled rasteriser.  Additive to ABI 7.  lnerf_raster_prepare / lnerf_rasterize above
 * stay as the definition these two are held to.
 * lnerf_raster_prepare_batch: cams_dev = DEVICE [B,14] f32, each row laid out as cam_host.  face_z [B,F,3] and face_xy
 *   [B,F,3,2] use lnerf_raster_prepare's arithmetic unchanged: slice b equals a single-view call with camera b bit for
 *   bit.  face_box [B,F] x 4 int16 (8-byte aligned) = the face's inclusive pixel range (j_lo, j_hi, i_lo, i_hi) in the
 *   H x W image, which is why H and W are arguments of THIS call (1 <= H, W <= 32767; 1 <= B <= 65535).
 * The box rule, in f32, every operation rounded on its own (no fused multiply-add), in this order:
 *   1. !(z0 < 0 && z1 < 0 && z2 < 0), or area == 0 with area = (x1-x0)*(y2-y0) - (x2-x0)*(y1-y0)  (the faces the
 *      rasteriser rejects outright)                                   -> the empty box (0, -1, 0, -1);
 *   2. any of the six xy coordinates NaN or infinite                  -> the whole image (0, W-1, 0, H-1);
 *   3. with the pixel centres px = (2j+1)/W - 1, py = 1 - (2i+1)/H and min / max over the three corners:
 *        j_lo = max(floor(((min_x + 1)*W - 1)*0.5) - 1, 0)      j_hi = min(ceil(((max_x + 1)*W - 1)*0.5) + 1, W-1)
 *        i_lo = max(floor(((1 - max_y)*H - 1)*0.5) - 1, 0)      i_hi = min(ceil(((1 - min_y)*H - 1)*0.5) + 1, H-1)
 *      (one pixel of padding each side, then clipped to the image; evaluated in f32 before the conversion to int16);
 *   4. j_lo > j_hi or i_lo > i_hi (wholly off the image)              -> the empty box (0, -1, 0, -1).
 * lnerf_rasterize_batch: face_idx [B,H*W], bary [B,H*W,3] = lnerf_rasterize's result restricted to the (pixel, face)
 *   pairs whose pixel lies in the face's box: the same per-face test, the same depth, the same tie rule (the lower face
 *   index wins an exact tie).  Where lnerf_rasterize accepts no pair outside a box the two agree bit for bit.  face_box
 *   is an input: any boxes may be given (e.g. from another source than the call above).  A pixel no face reaches gets
 *   face_idx = -1, bary = 0.
 * Both: no allocation, no synchronisation, no host read-back; capturable. */
int lnerf_raster_prepare_batch(const float *verts, int n_verts, const int32_t *faces, int n_faces,
                               const float *cams_dev, int B, int H, int W, float *face_z, float *face_xy,
                               int16_t *face_box, lnerf_stream_t stream);
int lnerf_rasterize_batch(int B, int H, int W, const float *face_z, const float *face_xy, const int16_t *face_box,
                          int n_faces, int32_t *face_idx, float *bary, lnerf_stream_t stream);
int lnerf_interpolate_attributes(const int32_t *face_idx, const float *bary, const float *attr, int n_pixels, int D,
                                 float *feat, lnerf_stream_t stream);
int lnerf_interpolate_attributes_backward(const int32_t *face_idx, const float *bary, const float *dfeat,
                                          int n_pixels, int D, float *dattr, lnerf_stream_t stream);
int lnerf_texture_map_forward(const float *uv, const int32_t *face_idx, const float *texture, int n_pixels, int C,
                              int R, int mode, float *out, lnerf_stream_t stream);
int lnerf_texture_map_backward(const float *uv, const int32_t *face_idx, const float *dout, int n_pixels, int C, int R,
                               int mode, float *dtexture, lnerf_stream_t stream);

/* ---- Mip-mapped texture lookup (`guide.texture_interpolation_mode mipmap`; csrc/texmip.hip).  Additive to ABI 7; the
 * three point lookups above are unchanged.  The reference has no counterpart (kaolin's texture_mapping is a point
 * lookup): this is the trilinear filter of rasteriser-based texture optimisers, isotropic, the longer of the two
 * screen-space UV derivatives choosing the level.  f32, every operation rounded on its own (no fused multiply-add).
 *
 * lnerf_uv_footprint: rho [B*H*W] = the length, in UV units, of the longer of the two screen-space UV derivative
 *   vectors per one-pixel step; 0 where face_idx < 0.  face_idx [B*H*W], face_xy [B,F,3,2] and face_z [B,F,3] are what
 *   lnerf_raster_prepare_batch / lnerf_rasterize_batch wrote; face_uv [F,3,2] = the per-face-vertex UVs (u_k, v_k).
 *   The definition is analytic on the winning face, not a difference of neighbouring pixels (those break at face
 *   borders and silhouettes).  With the pixel centre (px, py), area, e0, e1 of lnerf_rasterize:
 *     inv = 1 / area;  w0 = e0 * inv;  w1 = e1 * inv;  w2 = 1 - w0 - w1;
 *     q_k = w_k / z_k;  qs = q0 + q1 + q2;  z = 1 / qs;  bw_k = q_k * z            (the rasteriser's barycentrics)
 *     dw0/dpx = (y1 - y2) * inv   dw0/dpy = (x2 - x1) * inv
 *     dw1/dpx = (y2 - y0) * inv   dw1/dpy = (x0 - x2) * inv      dw2 = -dw0 - dw1
 *     a_k = dw_k / z_k;  s = a0 + a1 + a2;  dbw_k = (a_k - bw_k * s) * z           (per axis)
 *     du = u0 * dbw0 + u1 * dbw1 + u2 * dbw2,  dv likewise                          (per axis)
 *     rho = max(sqrt(du/dpx^2 + dv/dpx^2) * (2 / W), sqrt(du/dpy^2 + dv/dpy^2) * (2 / H))
 *   (one pixel step is 2/W in px and 2/H in py).  rho does not depend on the texture's side: one call serves textures
 *   of any resolution.  1 <= H, W <= 32767, B >= 1, B * H * W < 2^31.
 *
 * The pyramid of a square texture [C,R,R] with L levels, R divisible by 2^L: level l (1..L) has side R >> l and is the
 *   2 x 2 box average of level l - 1, ((t00 + t01) + (t10 + t11)) * 0.25 -- with texel centres (align_corners=False) a
 *   coarse texel covers exactly four fine ones.  Level 0 is the texture itself and is not copied.  Levels 1..L are
 *   packed [C, S], S = sum_l (R >> l)^2, level l of channel c starting at c * S + sum_{m<l} (R >> m)^2.  C * R * R <= 2^38.
 * lnerf_mip_build: texture -> pyramid, one launch per level.  L = 0 launches nothing (pyramid may be NULL).
 * lnerf_mip_build_backward: the exact transpose in gather form (no atomics, deterministic), from the coarsest level
 *   down: d[l-1][c,i,j] += 0.25 * d[l][c,i/2,j/2] INSIDE dpyramid (which it therefore changes), ending with
 *   dtexture[c,i,j] += 0.25 * d[1][c,i/2,j/2].  dtexture is ACCUMULATED into.
 *
 * lnerf_texture_mip_forward: out [n_pixels, C]; uv [n_pixels,2], rho [n_pixels] (lnerf_uv_footprint), face_idx may be
 *   NULL (every pixel is foreground); pixels with face_idx < 0 give 0.
 *     s = rho * R;  lambda = s > 0 ? clamp(log2f(s) + bias, 0, L) : 0;  l0 = min(floor(lambda), L);  t = lambda - l0
 *     out = t == 0 ? bil(l0) : (1 - t) * bil(l0) + t * bil(l0 + 1)
 *   bil(l) = lnerf_texture_map_forward's mode 1 (bilinear) on level l: the same texel coordinates for side R >> l,
 *   the same four taps and weights, the same sum.  When t == 0 only level l0 is read, so wherever the footprint is at
 *   most one texel (and bias <= 0) the result is mode 1's bit for bit.  bias must be finite.
 * lnerf_texture_mip_backward: float atomics of w * ((1 - t) * g) into level l0 and w * (t * g) into level l0 + 1
 *   (w * g when t == 0), level 0 being dtexture and the others dpyramid (same packing); both are ACCUMULATED into.
 *   lnerf_mip_build_backward then folds dpyramid into dtexture.  uv and rho carry no gradient.
 * All five: no allocation, no synchronisation, no host read-back; capturable.  Every argument is checked before the
 * first launch. */
int lnerf_uv_footprint(const int32_t *face_idx, const float *face_xy, const float *face_z, const float *face_uv, int B,
                       int H, int W, int n_faces, float *rho, lnerf_stream_t stream);
int lnerf_mip_build(const float *texture, int C, int R, int L, float *pyramid, lnerf_stream_t stream);
int lnerf_mip_build_backward(float *dpyramid, int C, int R, int L, float *dtexture, lnerf_stream_t stream);
int lnerf_texture_mip_forward(const float *uv, const float *rho, const int32_t *face_idx, const float *texture,
                              const float *pyramid, int n_pixels, int C, int R, int L, float bias, float *out,
                              lnerf_stream_t stream);
int lnerf_texture_mip_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                               int n_pixels, int C, int R, int L, float bias, float *dtexture, float *dpyramid,
                               lnerf_stream_t stream);

/* ---- Coverage-weighted texture pyramids (`guide.texture_mip_coverage`, the pull-push fill of the exports;
 * csrc/texmip.hip: the plain pyramid's kernels, instantiated with weights).  Additive to ABI 7; the plain pyramid above
 * is unchanged.  A pyramid whose level l is the coverage-weighted mean of level l - 1, the weights carried along, read
 * normalised (the lookup) or pushed back down into the texels no surface point owns (the fill).  f32, every operation
 * rounded on its own.  Shapes, packing, argument rules, lambda, l0, t and the taps are the plain pyramid's: texture
 * [C,R,R], R divisible by 2^L, values of levels 1..L packed [C,S], their weights [S].
 *
 * Weights.  w0 [R,R] in [0,1] (the callers pass 0 or 1).  With a, b, c, d the four children of a level-l texel (i, j) in
 *   the order (2i, 2j), (2i, 2j+1), (2i+1, 2j), (2i+1, 2j+1) of level l - 1:
 *     s   = (wa + wb) + (wc + wd)
 *     w_l = s * 0.25
 *   For 0/1 weights at level 0 every w_l is a multiple of 4^-l not above 1: exact in f32 (up to L = 11).
 * lnerf_mipcov_weights: w0 -> wpyr = lnerf_mip_build of the one-channel texture w0, bit for bit.  L = 0 launches nothing
 *   (wpyr may be NULL, here and below).
 *
 * lnerf_mipcov_pull: texture, w0, wpyr -> pyramid, one launch per level, t the values of level l - 1:
 *     v_l = s > 0 ? ((wa * ta + wb * tb) + (wc * tc + wd * td)) / s : 0
 *   With every weight 1 this is lnerf_mip_build bit for bit (s = 4, and / 4 is * 0.25).
 * lnerf_mipcov_pull_backward: the exact transpose in gather form (no atomics, deterministic), from the coarsest level
 *   down, INSIDE dpyramid (which it therefore changes), ending in dtexture, which is ACCUMULATED into:
 *     d[l-1][child] += (w_child / s) * d[l][parent]      s recomputed from the parent's four children
 *   Nothing is added where s == 0 (s > 0 is false).
 *
 * lnerf_mipcov_push: the pull-push fill.  `pyramid` holds lnerf_mipcov_pull's values on entry and the filled levels on
 *   exit; level 0 is `texture`, filled in place.  With L >= 1:
 *     F_L = v_L
 *     for l = L - 1 ... 0:
 *       k   = l >= 1 ? min(s_l, 1) : w0      s_l as above: a coarse texel with one whole covered child counts as known
 *       F_l = k == 1 ? v_l : k == 0 ? up(F_{l+1}) : k * v_l + (1 - k) * up(F_{l+1})
 *   (k == 0 is the general rule without reading v_l: an uncovered texel of the texture may hold anything.)
 *   A texel of any level is REACHED when its ancestor on level L has w_L > 0.  Texels that are not reached are left
 *   alone on every level, so texels under a coarsest-level texel of weight 0 stay as they were.
 *   up = the 2 x bilinear upsample with texel centres (align_corners=False), edges clamped.  For the texel (i, j) of
 *   level l, on level l + 1 (side Rc):
 *     pi = i / 2;  ni = i odd ? min(pi + 1, Rc - 1) : max(pi - 1, 0);   pj, nj likewise
 *     taps in the order (pi, pj), (pi, nj), (ni, pj), (ni, nj) with b = 9/16, 3/16, 3/16, 1/16
 *     up = (b0 * F0 + b1 * F1) + (b2 * F2 + b3 * F3)
 *   (pi, pj) is the texel's parent and is reached when the texel is.  A tap that is not reached holds no value: its
 *   term is 0 in the sum, and up is then divided by (b0 + b1') + (b2' + b3'), b' = b on reached taps and 0 elsewhere
 *   (at least 9/16).  With all four reached there is no division.
 *   filled [R,R] uint8 (may be NULL): 1 where w0 != 1 and the texel is reached, i.e. where level 0 was written; else 0.
 *   Texels with w0 == 1 are not written at all.  With L = 0 nothing is pushed (filled = 0 everywhere).
 *
 * lnerf_texture_mipcov_forward / _backward: lnerf_texture_mip_* with the weights, (i_k, b_k), k = 00, 01, 10, 11, its
 *   taps; V = `pyramid` from lnerf_mipcov_pull (level 0 = texture), W = w0 / wpyr.  Per level read, in the order of the
 *   plain mode's sum:
 *     n(l) = (b00 * W00) * V00 + (b01 * W01) * V01 + (b10 * W10) * V10 + (b11 * W11) * V11
 *     d(l) = (b00 * W00) + (b01 * W01) + (b10 * W10) + (b11 * W11)
 *     N = t == 0 ? n(l0) : (1 - t) * n(l0) + t * n(l0 + 1);   D likewise from d
 *   Three cases, decided from these f32 values only:
 *     (a) every W read is exactly 1:  out = N.  No division: the plain mode's result bit for bit.
 *     (b) D == 0 (a sliver face that covers no texel centre): the plain mode's result, every W taken as 1.
 *     (c) otherwise:  out = N / D.
 *   Backward: float atomics of (b_k * W_k) * (m * g / D) into tap k of level l, m * g = (1 - t) * g on l0 and t * g on
 *   l0 + 1 (g when t == 0); in cases (a) and (b) the plain mode's addends b_k * (m * g).  Level 0 is dtexture, the
 *   others dpyramid; both are ACCUMULATED into.  lnerf_mipcov_pull_backward then folds dpyramid into dtexture.  The
 *   weights, uv and rho carry no gradient.
 * All six: no allocation, no synchronisation, no host read-back; capturable.  Every argument is checked before the
 * first launch. */
int lnerf_mipcov_weights(const float *w0, int R, int L, float *wpyr, lnerf_stream_t stream);
int lnerf_mipcov_pull(const float *texture, const float *w0, const float *wpyr, int C, int R, int L, float *pyramid,
                      lnerf_stream_t stream);
int lnerf_mipcov_pull_backward(float *dpyramid, const float *w0, const float *wpyr, int C, int R, int L,
                               float *dtexture, lnerf_stream_t stream);
int lnerf_mipcov_push(float *texture, const float *w0, const float *wpyr, float *pyramid, int C, int R, int L,
                      uint8_t *filled, lnerf_stream_t stream);
int lnerf_texture_mipcov_forward(const float *uv, const float *rho, const int32_t *face_idx, const float *texture,
                                 const float *pyramid, const float *w0, const float *wpyr, int n_pixels, int C, int R,
                                 int L, float bias, float *out, lnerf_stream_t stream);
int lnerf_texture_mipcov_backward(const float *uv, const float *rho, const int32_t *face_idx, const float *dout,
                                  const float *w0, const float *wpyr, int n_pixels, int C, int R, int L, float bias,
                                  float *dtexture, float *dpyramid, lnerf_stream_t stream);

/* ---- optimiser step used by the bench/trainer (Adam, src/latent_paint/training/trainer.py:93-95:
 * betas (0.9, 0.99), eps 1e-15).  g is multiplied by grad_scale (1/world_size) first; if
 * zero_grad != 0 the gradient is cleared in the same pass; if shadow_bf16 != NULL the bf16
 * copy read by the gather is refreshed in the same pass.  grad_dtype: LNERF_F32, or LNERF_BF16 to
 * consume the bf16 wire buffer of the data-parallel all-reduce directly. */
int lnerf_adam_step(float *p, void *g, int grad_dtype, float *m, float *v, void *shadow_bf16, int64_t n, float lr,
                    float beta1, float beta2, float eps, int step, const int32_t *step_dev, float grad_scale,
                    int zero_grad, lnerf_stream_t stream);
/* `step_dev` (may be NULL): device-side step counter read by the kernels instead of the host `step`, so a
 * captured hipGraph of the whole optimisation step can be replayed; lnerf_adam_tick() increments it. */
int lnerf_adam_tick(int32_t *step_dev, lnerf_stream_t stream);
/* The same update for up to 16 small tensors in ONE launch (MLP / background parameters).  The pointer
 * and size arrays are HOST arrays of `count` entries holding device pointers.
 * zero_grad | LNERF_ADAM_TICK: the launch also advances *step_dev once all its workgroups have read it (saves the
 * lnerf_adam_tick dispatch when this is the step's last Adam launch); step_dev is then int32[2], [1] = 0 on entry
 * (arrival counter, 0 again on exit). */
#define LNERF_ADAM_TICK 2
int lnerf_adam_step_multi(int count, float *const *p_host, float *const *g_host, float *const *m_host,
                          float *const *v_host, const int64_t *n_host, const float *lr_host, float beta1, float beta2,
                          float eps, int step, const int32_t *step_dev, float grad_scale, int zero_grad,
                          lnerf_stream_t stream);
/* The same launch, which also mirrors tensors into a bf16 image: map_host[k] (NULL: tensor k is not mirrored) holds two
 * int32 positions per element of tensor k (-1: none); the updated value is stored as bf16 at shadow_bf16[position].
 * With the maps of lnerf_mlp_fragment_maps and the head of the MLP workspace as the image, the optimiser keeps the MLP's
 * weight fragments current and lnerf_mlp_forward(... | LNERF_MLP_FRAGMENTS_READY) skips its per-step build (one
 * dispatch of the step). */
int lnerf_adam_step_multi_shadow(int count, float *const *p_host, float *const *g_host, float *const *m_host,
                                 float *const *v_host, const int64_t *n_host, const float *lr_host, float beta1,
                                 float beta2, float eps, int step, const int32_t *step_dev, float grad_scale,
                                 int zero_grad, const int32_t *const *map_host, void *shadow_bf16,
                                 lnerf_stream_t stream);
/* ---- the TAIL of a single-GPU optimisation step: what is left of it besides the scatter (a dependent dispatch in a
 * replayed graph costs ~4.5 us whatever it computes; three of them sat behind the scatter for a few microseconds of work):
 *   - sum of the MLP's gradient slabs (after lnerf_mlp_backward(precision | LNERF_MLP_DEFER_REDUCE)) in the fixed order
 *     of the ordinary reduction, and the Adam step of w1, b1, w2, b2, w3, b3 straight from the sums
 *     (params / exp_avg / exp_avg_sq: host arrays of six device pointers; maps_host: optional, the three fragment maps of
 *     lnerf_mlp_fragment_maps -- the updated weights are mirrored into the fragment image at the head of mlp_workspace;
 *     mlp_workspace = NULL: skipped -- the tick / the clearing below still run, as one workgroup);
 *   - LNERF_TAIL_TICK: *step_dev += 1 once every workgroup has read it (the arrival counters live in the header of the
 *     scatter workspace: LNERF_SCATTER_ZERO_HEAD_BYTES);
 *   - LNERF_TAIL_CLEAR_SCATTER: the scatter's level maxima (first lnerf_grid_scatter_clear_bytes() bytes of its
 *     workspace) are zero on exit, i.e. the NEXT scatter call may pass LNERF_SCATTER_CLEARED.
 * Same arithmetic as the separate launches (csrc/adam_shared.h): parameters and moments are bit-identical.
 * Two forms:
 *   lnerf_grid_encode_backward_adam_tail  the scatter with the fused table update (lnerf_grid_encode_backward_adam) whose
 *     pass 2 ALSO runs the tail, as extra workgroups of the same launch: the step has no launch behind the scatter.
 *     For a step whose only parameters are the table and the MLP's six tensors; needs step_dev and m_host > 0.
 *   lnerf_step_tail  the tail as a launch of its own, behind lnerf_grid_encode_backward_adam (when other small parameters
 *     are stepped in between).  num_levels = 0: no scatter workspace (then no tick / clear). */
#define LNERF_TAIL_TICK 1
#define LNERF_TAIL_CLEAR_SCATTER 2
int lnerf_step_tail(int num_levels, int level_dim, const int32_t *offsets_host, const float *scales_host,
                    const int32_t *res_host, int64_t m_host, int variant, void *scatter_workspace,
                    size_t scatter_workspace_bytes, float *dtable_zero, float *table, float *exp_avg, float *exp_avg_sq,
                    void *shadow_bf16, float table_lr, const void *mlp_workspace, size_t mlp_workspace_bytes,
                    int mlp_precision, int out_dim, float *const *params_host, float *const *exp_avg_host,
                    float *const *exp_avg_sq_host, float mlp_lr, const int32_t *const *maps_host, float beta1, float beta2,
                    float eps, int step, int32_t *step_dev, float grad_scale, int flags, lnerf_stream_t stream);
int lnerf_grid_encode_backward_adam_tail(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                         int level_dim, const int32_t *offsets_host, const float *scales_host,
                                         const int32_t *res_host, int64_t m_host, const int32_t *m_dev,
                                         int64_t level_stride, float *dtable_zero, int variant, void *workspace,
                                         size_t workspace_bytes, float *table, float *exp_avg, float *exp_avg_sq,
                                         void *shadow_bf16, float lr, const void *mlp_workspace,
                                         size_t mlp_workspace_bytes, int mlp_precision, int out_dim,
                                         float *const *params_host, float *const *exp_avg_host,
                                         float *const *exp_avg_sq_host, float mlp_lr, const int32_t *const *maps_host,
                                         float beta1, float beta2, float eps, int step, int32_t *step_dev, float grad_scale,
                                         int flags, lnerf_stream_t stream);
/* ---- moment map of the fused table update (additive to ABI 7).  With g = +-0, m = v = +0 the Adam step returns m, v and
 * p as they were, bit for bit (finite lr, eps > 0), so a 16-row group of the table whose moments are all-zero bits and
 * which gets no gradient needs no load and no store: the part of the table no sample has ever reached.  The map holds one
 * byte per (bucket, 16-row group) of the scatter's bucket plan -- level l, bucket b (4096 rows from the level's first
 * row), group g = row in bucket >> 4 at byte ((buckets of the levels below l) + b) * 256 + g -- and after every fused
 * step  byte != 0  <=>  some exp_avg / exp_avg_sq word of the group has a non-zero bit pattern (-0.0 counts).
 *   lnerf_moment_map_bytes  size of the map of a level table (0: not plannable).
 *   lnerf_moment_map_build  one streaming launch that computes every byte from the moments.
 *   lnerf_moment_map_bind   binds `map` to the optimiser state whose first moment is `exp_avg` (process-wide registry
 *     under a mutex; a null map unbinds).  lnerf_grid_encode_backward_adam / _adam_tail look their exp_avg up: with a
 *     binding pass 2 skips clean groups without gradient and keeps the map current; without one they behave as before.
 * The owner keeps the map valid: whatever else writes the moments (lnerf_adam_step, a copy) makes it stale -- rebuild
 * it on the same stream before the next fused call, or unbind.  Unbind before the map or the moments are freed. */
size_t lnerf_moment_map_bytes(int num_levels, const int32_t *offsets_host);
int lnerf_moment_map_build(const float *exp_avg, const float *exp_avg_sq, int num_levels, int level_dim,
                           const int32_t *offsets_host, void *map, size_t map_bytes, lnerf_stream_t stream);
int lnerf_moment_map_bind(const float *exp_avg, void *map, size_t map_bytes);
/* ---- Adam's bias corrections published once per step (additive to ABI 7).  With a device step counter every lane of
 * every Adam kernel computed  bc1 = 1 - powf(beta1, t), bc2 = 1 - powf(beta2, t), 1 / bc1, 1 / bc2  from the same three
 * numbers.  A record of LNERF_ADAM_CONSTANTS_BYTES bytes bound to the counter holds them as data:
 *   float bc1, bc2, inv_bc1, inv_bc2;  int32 tag (the step t the four belong to);  12 bytes of padding.
 *   lnerf_adam_constants_bind    binds `consts` (16-byte aligned, filled with 0xFF bytes by the owner: tag -1 = nothing
 *     published) to the counter `step_dev` for these betas (process-wide registry under a mutex, keyed by step_dev).
 *   lnerf_adam_constants_unbind  removes the binding (fine without one).  Unbind before either buffer is freed.
 * Whoever ADVANCES a bound counter -- lnerf_adam_tick, LNERF_ADAM_TICK, LNERF_TAIL_TICK in either tail form -- computes
 * the four values for the new step (the same device code every lane ran: the same bits) and stores them, then the tag.
 * Whoever READS a bound counter -- lnerf_adam_step, lnerf_adam_step_multi(_shadow), lnerf_grid_encode_backward_adam(_tail),
 * lnerf_step_tail -- reads the record with it and uses the values where tag == *step_dev; otherwise (a counter written
 * from the host, a fresh record, a call with other betas than the binding's, no binding) it computes them as before.
 * Nothing is ever read behind the counter's own words: an unbound int32[2] counter behaves as it always did. */
#define LNERF_ADAM_CONSTANTS_BYTES 32
int lnerf_adam_constants_bind(const int32_t *step_dev, float beta1, float beta2, void *consts);
int lnerf_adam_constants_unbind(const int32_t *step_dev);
int lnerf_cast_f32_to_bf16(const float *src, void *dst, int64_t n, lnerf_stream_t stream);

/* ---- iso-surface extraction (marching cubes): NeRFRenderer.export_mesh's kernel (the upstream renderer runs
 * `mcubes.marching_cubes` on the host).  Additive to ABI 7.
 *   vol [nx][ny][nz] f32, contiguous, z fastest (the layout mcubes uses); 2 <= nx, ny, nz <= LNERF_MC_MAX_DIM.
 *   Lattice point (i, j, k) sits at  x_a(i) = lo_a + (hi_a - lo_a) * i / (n_a - 1)  (f32, evaluated left to right).
 *   A point is INSIDE iff value > iso; NaN is outside.  LNERF_MC_CLOSE_BOUNDARY: a layer of outside points surrounds
 *   the lattice, so a surface that reaches the box is capped (the mesh is closed); without it the mesh is open there.
 * Tables and orientation: csrc/mc_tables.h (tools/gen_mc_tables.py): corner c = x + 2y + 4z, ambiguous faces never
 * connect their inside corners, triangles (a, b, c) have (b - a) x (c - a) pointing from inside to outside.
 * Vertices: every point of the working lattice (the lattice, plus the outside layer under CLOSE_BOUNDARY) owns its
 *   +x, +y, +z edges; a vertex exists on every edge whose ends differ in inside-ness.  Order: (owning point's linear
 *   index in the working lattice, axis x < y < z) -- shared vertices get one index, no dedup pass.  On the edge from
 *   p0 (value v0) to p0 + e_a (value v1):  t = (iso - v0) / (v1 - v0);  if 0 <= t <= 1 the vertex's axis-a coordinate
 *   is  x0 + t * (x1 - x0)  (x0, x1: the ends' coordinates), else (a NaN or outside-the-lattice end) the vertex sits
 *   exactly on the inside end; the two other coordinates are the owning point's.  f32, no fused multiply-adds.
 * Normals: world-space gradients at the two ends (central differences of vol over the ends' coordinate differences,
 *   one-sided at the lattice border), blended with the same t (or taken from the inside end), negated, normalised
 *   (0 for a zero gradient): they point from inside to outside.  `normals` may be NULL.
 * Triangles: cells in order of their corner-0 point, table order within a cell; faces [F][3] int32 vertex indices.
 *   The output is fully deterministic.  V must stay below 2^31 (int32 faces).
 * counts_dev int64[2] receives {n_verts, n_faces}.  Vertices with index >= max_verts and triangles with index >=
 * max_faces are not written (the counts are still the true ones).  Scratch: lnerf_marching_cubes_scratch_bytes()
 * (~4 bytes per working point; 16-byte aligned).  Flags:
 *   LNERF_MC_COUNT_ONLY  only the counts (and the scratch state for a following REUSE_COUNT call); outputs unused;
 *   LNERF_MC_REUSE_COUNT only the emit pass, from the scratch of an immediately preceding COUNT_ONLY call with the
 *                        same volume, lattice, iso and CLOSE_BOUNDARY (the caller sizes its buffers in between). */
#define LNERF_MC_CLOSE_BOUNDARY 1
#define LNERF_MC_COUNT_ONLY 2
#define LNERF_MC_REUSE_COUNT 4
#define LNERF_MC_MAX_DIM 1024
size_t lnerf_marching_cubes_scratch_bytes(int nx, int ny, int nz, int flags);
int lnerf_marching_cubes(const float *vol, int nx, int ny, int nz, float iso, float lo_x, float lo_y, float lo_z,
                         float hi_x, float hi_y, float hi_z, int flags, void *scratch, size_t scratch_bytes,
                         float *verts, float *normals, int64_t max_verts, int32_t *faces, int64_t max_faces,
                         int64_t *counts_dev, lnerf_stream_t stream);

/* ---- texture baking over a UV atlas: NeRFRenderer.bake_texture's kernels (csrc/uvbake.hip).  Additive to ABI 7.
 * lnerf_uv_raster: which texel of an R x R texture each face covers, and the surface point there.
 *   verts [n_verts,3] f32, faces [n_faces,3] int32 (into verts), vt [n_vt,2] f32, ft [n_faces,3] int32 (into vt);
 *   1 <= R <= LNERF_UV_MAX_RES.
 *   Texel (row i, column j) of a [C,R,R] texture has its centre at u = (j + 0.5) / R, v = 1 - (i + 0.5) / R: the
 *   convention of lnerf_texture_map_forward (grid_sample, align_corners=False, on (u, 1 - v)).  In pixel space a UV
 *   corner is X = u * R, Y = (1 - v) * R and the texel centre is p = (j + 0.5, i + 0.5).  All f32, no fused multiply-adds.
 *   E_ab(p) = (X_b - X_a) * (p_y - Y_a) - (Y_b - Y_a) * (p_x - X_a);  area = E_01(corner 2).
 *   Candidates of a face: columns max(0, floor(min X) - 1) .. min(R - 1, floor(max X) + 1), rows likewise from Y (none
 *   when that range is empty, or the area is NaN, infinite or 0).  A candidate texel is COVERED iff E_12, E_20 and E_01
 *   at p each have the sign of the area or are 0 (inclusive edges, both windings).  Where several faces cover a
 *   texel the largest face index wins.  Barycentrics b_k = E_opposite(p) / area (b0 = E_12 / area, b1 = E_20 / area,
 *   b2 = E_01 / area), surface point = b0 * P0 + b1 * P1 + b2 * P2 evaluated left to right.  Fully deterministic.
 * Outputs: texel_face [R*R] int32 (winning face, -1 = none); the P covered texels in ascending linear order (i*R + j):
 *   texel_idx [P] int32 and pos [P,3] f32 (entries at index >= max_texels are not written).
 * counts_dev int64[3]: {candidate items, faces with an index out of range, P}.  A face with an index out of range
 *   covers nothing and reads no vertex through it.  Scratch: lnerf_uv_raster_scratch_bytes() (16-byte aligned; 0 =
 *   arguments out of range).  `stages`, run in this order, each from the scratch state of the previous one (same inputs):
 *   LNERF_UV_ITEMS  the per-face candidate counts and their prefix -> counts[0], counts[1];
 *   LNERF_UV_COVER  texel_face, then counts[2]; n_items: the item total of counts[0] or any upper bound of it (one lane
 *                   per item; launches of at most 2^30 items each);
 *   LNERF_UV_EMIT   texel_idx and pos. */
#define LNERF_UV_ITEMS 1
#define LNERF_UV_COVER 2
#define LNERF_UV_EMIT 4
#define LNERF_UV_MAX_RES 8192
size_t lnerf_uv_raster_scratch_bytes(int n_faces, int R);
int lnerf_uv_raster(const float *verts, int n_verts, const int32_t *faces, const float *vt, int n_vt,
                    const int32_t *ft, int n_faces, int R, int stages, int64_t n_items, void *scratch,
                    size_t scratch_bytes, int32_t *texel_face, int32_t *texel_idx, float *pos, int64_t max_texels,
                    int64_t *counts_dev, lnerf_stream_t stream);
/* lnerf_uv_dilate: `passes` gutter rounds over texture [C,R,R] f32 and mask [R,R] uint8 (2 = covered, 1 = filled by a
 * round, 0 = empty), in place.  In a round every texel that was empty before the round and has k > 0 neighbours
 * (of its 8) that were non-empty before the round takes their mean per channel: their sum in f32 in the order
 * (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1) (row, column offsets), divided by k; its mask becomes 1.
 * Every other texel keeps its value and mask.  tmp_texture / tmp_mask: buffers of the same sizes (ping-pong). */
int lnerf_uv_dilate(float *texture, uint8_t *mask, int C, int R, int passes, float *tmp_texture, uint8_t *tmp_mask,
                    lnerf_stream_t stream);

/* ---- multi-view projection: colours surface points from K images of the surface, with a visibility test and an angle
 * weight (csrc/uvproject.hip; NeRFRenderer.bake_views, Latent-Paint's view bake).  Additive to ABI 7.
 *   pos, nrm [P,3] f32: a surface point x and its unit outward normal n (any points: the kernel knows no atlas);
 *   cams_dev: device [K,14], the record of lnerf_raster_prepare_batch (rotation rows 9, eye 3, fx, fy; camera z is
 *     negative in front);  zbuf [K,H,W]: camera z of the visible surface at each pixel centre (negative); a value >= 0
 *     marks a pixel that must not be used (background, or eroded by the host);  images [K,C,H,W], 1 <= C <= 4.
 *   1 <= K <= 65535, 2 <= H, W <= 32767, 0 < cos_min <= 1, power >= 0, slack >= 0, 0 <= P < 2^31.
 * Per point and view k, all in f32, the views in ascending k and accumulated in that order (deterministic, no atomics):
 *   1. d = eye - x, c = (n . d) / |d| (products summed left to right); rejected unless c >= cos_min.
 *   2. p = rot (x - eye), each row as fmaf(r0, x, fmaf(r1, y, r2 * z)) like lnerf_raster_prepare_batch; rejected unless
 *      p.z < 0.  X = p.x * fx / (-p.z), Y = p.y * fy / (-p.z).
 *   3. u = ((X + 1) W - 1) / 2, v = ((1 - Y) H - 1) / 2: pixel centres at integers (column u, row v), the rasteriser's
 *      convention.  j0 = floor(u), i0 = floor(v), tu = u - j0, tv = v - i0; rejected unless 0 <= j0, j0 + 1 <= W - 1,
 *      0 <= i0, i0 + 1 <= H - 1.
 *   4. rejected unless zbuf < 0 at all four taps (i0 | i0 + 1, j0 | j0 + 1): silhouette pixels mix in background.
 *   5. depth test against the NEAREST tap (tu >= 0.5 -> j0 + 1, tv >= 0.5 -> i0 + 1): accepted iff
 *      p.z >= zbuf[nearest] - bias,
 *      bias = slack * (-p.z) * 2 / min(fx W, fy H) * sqrt(max(1 - c^2, 0)) / c + 1e-4 * (-p.z)    (left to right):
 *      the depth change across `slack` pixel footprints of a surface tilted by acos c, plus a floor for head-on views.
 *   6. w = powf(c, power); colour, per channel, the bilinear sample a + tv (b - a) with a = I[i0,j0] + tu (I[i0,j0+1] -
 *      I[i0,j0]) and b the same on row i0 + 1; weight += w, count += 1, acc += w * (colour - first), `first` being the
 *      colour of the point's first accepted view.
 * Outputs: out [P,C] = first + acc / weight where weight > 0, else 0 -- the weighted mean sum(w colour) / sum(w),
 *   evaluated around the first accepted colour: differences of equal taps and of equal views are exact zeros, so a
 *   colour that all accepted views agree on comes back bit for bit; weight [P]; count [P] int32, the views accepted. */
int lnerf_uv_project_views(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                           const float *zbuf, const float *images, int C, float cos_min, float power, float slack,
                           float *out, float *weight, int32_t *count, lnerf_stream_t stream);

/* ---- exposure matching and two-band blending of a view bake (csrc/viewblend.hip; view_bake.bake_views with
 * exposure = True / blend = "bands").  Additive to ABI 7.  pos, nrm, cams_dev, zbuf, images, cos_min, power, slack as
 * lnerf_uv_project_views, and a point ACCEPTS a view by that call's steps 1-5, one device function for all
 * (csrc/view_shared.h).  No call allocates or reads back; all are capturable; every argument is checked before the first
 * launch; two calls give the same bits (numpy restatement: tests/view_blend_reference.py).
 * lnerf_view_lowpass: a masked, normalised, separable Gaussian low-pass of each view.  images, low [K,C,H,W] f32,
 *   1 <= K <= 65535, 1 <= C <= 4, 1 <= H, W <= 32767, K C H W < 2^31; a pixel is USABLE iff zbuf < 0.  taps_host: 2r + 1
 *   host floats in [0, 1], 0 <= r <= LNERF_LOWPASS_MAX_R (the host side: exp(-t^2 / (2 sigma^2)) in f64, normalised to
 *   sum 1, r = ceil(3 sigma), rounded to f32); they are copied into the launch.  All sums in f32, t ascending from -r,
 *   each term a product then an add:
 *     rows:    num(i,j) = sum_t g[t] I(i, j+t), den(i,j) = sum_t g[t]   over the taps inside the image AND usable;
 *     columns: num'(i,j) = sum_t g[t] num(i+t, j), den'(i,j) = sum_t g[t] den(i+t, j)   over the taps inside the image;
 *     low = den' > 0 ? num' / den' : 0, written at every pixel, usable or not.
 *   An unusable pixel is skipped by selection, never multiplied by 0: a NaN or inf there reaches no output.
 *   Scratch: lnerf_view_lowpass_scratch_bytes() (0 = arguments out of range; 16-byte aligned).
 * lnerf_view_overlap_stats: for every ordered pair of views, how many points both accept and what the first shows
 *   there.  low [K,C,H,W]; 1 <= K <= LNERF_STATS_MAX_K.  N [K,K] int64 and S [K,K,C] int64 must be zero on entry and are
 *   accumulated into: for every point and every ordered pair i != j of its accepted views
 *     N[i,j] += 1,   S[i,j,c] += llrintf(L_i[c] * 16777216.0f),
 *   L_i the bilinear sample of low_i at the point with step 6's nested lerps.  64-bit integer atomics only, so the
 *   sums do not depend on the order in which they land.  Domain: finite low with |value| <= 64: a term is then at most
 *   2^30 and P < 2^31 of them stay below 2^62.
 * lnerf_uv_project_views_bands: the two-band projection.  low [K,C,H,W]; gains: device [K,C] or NULL (no gain and NO
 *   multiplication: the samples keep their bits).  Any K up to 65535, the views in ascending k, no atomics.  Per
 *   accepted view: w = powf(c, power), I_k = g_k * bil(images_k), L_k = g_k * bil(low_k) per channel; weight += w,
 *   count += 1, acc += w * (L_k - Lfirst); the BEST view is the one with the largest w (strict >, so the lowest k wins
 *   an exact tie).  lowmean = Lfirst + acc / weight;  out [P,C] = I_best + (lowmean - L_best), evaluated in that order,
 *   where weight > 0, else 0: the low band is the weighted mean of the views' low bands, everything above it comes
 *   from the best view alone.  weight [P] and count [P] are exactly those of lnerf_uv_project_views; best [P] int32 is
 *   -1 where no view is accepted. */
#define LNERF_LOWPASS_MAX_R 64
#define LNERF_STATS_MAX_K 64
size_t lnerf_view_lowpass_scratch_bytes(int K, int C, int H, int W);
int lnerf_view_lowpass(const float *images, const float *zbuf, int K, int C, int H, int W, const float *taps_host, int r,
                       void *scratch, size_t scratch_bytes, float *low, lnerf_stream_t stream);
int lnerf_view_overlap_stats(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                             const float *zbuf, const float *low, int C, float cos_min, float slack, int64_t *N, int64_t *S,
                             lnerf_stream_t stream);
int lnerf_uv_project_views_bands(const float *pos, const float *nrm, int64_t P, const float *cams_dev, int K, int H, int W,
                                 const float *zbuf, const float *images, const float *low, const float *gains, int C,
                                 float cos_min, float power, float slack, float *out, float *weight, int32_t *count,
                                 int32_t *best, lnerf_stream_t stream);

/* ---- mesh decimation: rounds of independent quadric-error (Garland-Heckbert) edge collapses, NeRFRenderer.export_mesh's
 * `target_faces` (csrc/decimate.hip).  Additive to ABI 7.  Fully deterministic; the C call is synchronous (one host
 * read of the counts before round 1, one per round).
 *   verts [n_verts,3] f32, faces [n_faces,3] int32.  A face with an index outside [0, n_verts) fails the call
 *   (LNERF_ERR_INVALID_ARG) before any kernel reads through it; faces that repeat an index are dropped first.
 *   f64 and f32 arithmetic below is + - * / and sqrt only, evaluated left to right (no fused multiply-adds).
 * Quadrics (once, from the input): face quadric = w * (n0n0, n0n1, n0n2, n1n1, n1n2, n2n2, n0d, n1d, n2d, dd) in f64,
 *   m = (p1 - p0) x (p2 - p0), l = sqrt(m.m), n = m / l, d = -(n.p0), w = l * 0.5 (all ten 0 when l = 0); a vertex sums
 *   those of its faces in ascending face index (vertex -> face lists built on the device: count, scan, fill, sort).
 *   A collapse's survivor takes Q_u + Q_v.
 * A round, on the current faces:
 *   locked vertex: no faces, an edge at it not in exactly one face each way round, or faces that are not one closed
 *     fan.  Open borders and non-manifold parts therefore keep their exact positions.
 *   candidates: half-edge e = 3 f + k from faces[f][k] = u to faces[f][(k+1)%3] = v with u < v.  Invalid if u or v is
 *     locked; both have 3 faces (a tetrahedron); u and v have other than exactly 2 common neighbours (link condition);
 *     the cost is not finite or (as f32) > max_error; a face around u or v that does not hold both has normal m before
 *     and m' after the move with m != 0 and m.m' <= 0 (a flip), or m == 0 and m' != 0 (a zero-area face gaining area:
 *     its plane is in no quadric, so the move would look free).  Normals m in f64 from the f32 positions.
 *   v*: A x = -b by cofactors (c00 = a11a22 - a12a12, c01 = a02a12 - a01a22, c02 = a01a12 - a02a11, c11 = a00a22 -
 *     a02a02, c12 = a01a02 - a00a12, c22 = a00a11 - a01a01, det = a00c00 + a01c01 + a02c02, x_i = -(c_i0 b0 + c_i1 b1 +
 *     c_i2 b2) / det), rounded to f32; used iff |det| > LNERF_DECIMATE_SINGULAR_REL * tr^3 (tr = a00 + a11 + a22) and x
 *     is finite, else the cheapest of p_u, p_v, (p_u + p_v) * 0.5f (earlier wins a tie).
 *   cost(x) = (t0 x0 + t1 x1 + t2 x2) + (b0 x0 + b1 x1 + b2 x2) + c,  t_i = a_i0 x0 + a_i1 x1 + a_i2 x2 + b_i  (f64 at
 *     the f32 point; below or at 0 -> +0), rounded to f32.
 *   key = f32 cost bits << 32 | tag(e) (u64), tag = a fixed bijection of the 32-bit edge id (x *= 0x9E3779B1,
 *     x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13): costs tie often (a flat region's are all 0) and ids ordered along
 *     the lattice would leave one local minimum per region per round.
 *   selection: K1[w] = min key at w (atomic min), face key = min K1 of its corners, K2[w] = min face key at w; e
 *     collapses iff K2[u] == K2[v] == key.  No face touches the ends of two selected edges, so the checks hold together.
 *     In the round that would pass target_faces only the ceil((F - target_faces) / 2) smallest keys collapse.
 *   apply: p_u = v*, Q_u += Q_v, v -> u in every face; the two faces of each collapse go; stable compaction.
 * Stop when F <= target_faces, a round selects nothing, or after max_rounds rounds.  Then: the referenced vertices in
 *   their old order, faces in their old order, normals = the f32 sum over the vertex's faces in ascending order of
 *   (p1 - p0) x (p2 - p0), times 1.0f / sqrtf(l2) (0 for l2 = 0).
 * Outputs (capacity n_verts / n_faces; normals may be NULL): counts_dev int64[4] = {V_out, F_out, rounds, collapses}.
 * Scratch: lnerf_decimate_scratch_bytes() (0 = arguments out of range; 16-byte aligned).
 * Constants: SINGULAR_REL the solve's threshold above; DEFAULT_ROUNDS the host side's max_rounds default; MAX_FACES the
 * largest n_faces (3 n_faces half-edge ids and scan totals stay in int32). */
#define LNERF_DECIMATE_SINGULAR_REL 1e-10
#define LNERF_DECIMATE_DEFAULT_ROUNDS 128
#define LNERF_DECIMATE_MAX_FACES (1 << 28)
size_t lnerf_decimate_scratch_bytes(int n_verts, int n_faces);
int lnerf_decimate(const float *verts, int n_verts, const int32_t *faces, int n_faces, int target_faces, float max_error,
                   int max_rounds, void *scratch, size_t scratch_bytes, float *verts_out, int32_t *faces_out,
                   float *normals_out, int64_t *counts_dev, lnerf_stream_t stream);

/* ---- chart atlas: a UV map of connected, axis-projected patches, raymarching.chart_atlas's kernels (csrc/atlas.hip).
 * Additive to ABI 7.  All device arithmetic is f32 + - * / in the order written, no fused multiply-adds; the scale search
 * and the packing are host code in f64 and integers (src/uv_atlas.py).  Every result is independent of the order in
 * which the integer atomics land, so the atlas is bit-reproducible (numpy restatement: tests/atlas_reference.py).
 *   verts [n_verts,3] f32, faces [n_faces,3] int32, n_faces <= LNERF_ATLAS_MAX_FACES.
 * lnerf_atlas_buckets: for face f with corners P0, P1, P2:  m = (P1 - P0) x (P2 - P0)  (m_x = a_y b_z - a_z b_y, ...),
 *   scores (m_x, -m_x, m_y, -m_y, m_z, -m_z); b starts at 0 and becomes k whenever score_k > score_b, so the first maximum
 *   wins and m = 0 or NaN gives 0.  The unit normal then has n . axis >= 1/sqrt(3).  bucket[f] = b, label[f] = f.  A face
 *   with an index outside [0, n_verts) gets bucket -1, is counted in counts_dev int64[1] and reads nothing through the
 *   index; every later stage skips it (the host side refuses the mesh).
 *   Plane coordinates (p, q) of (x, y, z) in bucket b, p x q = axis, so a non-degenerate face is counter-clockwise:
 *     0 (+x): (y, z)   1 (-x): (z, y)   2 (+y): (z, x)   3 (-y): (x, z)   4 (+z): (x, y)   5 (-z): (y, x)
 * Links (the caller's, twin [3 n_faces] int32): half-edge 3 f + k runs from faces[f][k] to faces[f][(k+1)%3]; its twin is
 *   the one half-edge the other way round, present only if the undirected edge occurs in exactly two half-edges, one
 *   each way, and its ends differ; otherwise -1.  Open borders and non-manifold edges therefore never join charts.
 * lnerf_atlas_round: charts are the connected components of  f ~ g  iff f and g are linked and bucket[f] == bucket[g];
 *   label[f] converges to the smallest face index of f's component.  One round: hook (m = min of label[f] and the
 *   labels of f's linked same-bucket neighbours; if m < label[f]: atomicMin(label[label[f]], m), atomicMin(label[f], m),
 *   *changed_dev = 1), then LNERF_ATLAS_JUMP_HOPS steps of label[f] = label[label[f]].  changed_dev int32[1] is cleared
 *   first.  A round that leaves it 0 changed nothing and the labels are final; the host stops at
 *   LNERF_ATLAS_MAX_ROUNDS and raises.  No kernel loops on the labels beyond those fixed hops.
 * lnerf_atlas_compact: charts numbered 0 .. C-1 in ascending label order: face_chart [n_faces] (-1 for a refused face),
 *   chart_axis [capacity n_faces, C written] = the bucket, counts_dev int64[1] = C.
 * lnerf_atlas_boxes: chart_box [n_charts,4] f32 = (p_lo, p_hi, q_lo, q_hi), min / max over the corners of the chart's
 *   faces, by integer atomics on the order-preserving encoding  e = bits ^ (bits < 0 ? 0xFFFFFFFF : 0x80000000)  (so
 *   -0 < +0).  A chart without faces gets (NaN, NaN, NaN, NaN) patterns and must not be used.
 * Scale and packing (host): g = pad; ext_p = p_hi - p_lo, ext_q = q_hi - q_lo in f64; s_0 = (R - 2g - 2) / the largest
 *   extent (1 when all are 0), s_k = f32(s_0 * 0.95^k); rectangle w = 2g + 2 + floor(ext_p * s), h = 2g + 2 +
 *   floor(ext_q * s) with the ROUNDED s; charts sorted by (h desc, w desc, id asc) go on shelves left to right: a new
 *   shelf (y += shelf height, x = 0) when x + w > R, failure when w > R or y + h > R, shelf height = the largest h placed
 *   on it.  The first k that packs is taken; past k = 200 the host raises.
 * lnerf_atlas_uv: a corner at plane position (p, q) of a face in chart c with origin (ox, oy) = chart_org[c]:
 *     X = ((float)(ox + g) + 0.5f) + (p - p_lo) * s,   Y = ((float)(oy + g) + 0.5f) + (q_hi - q) * s,
 *     u = X / R,   v = 1.0f - Y / R        (the texel convention of lnerf_uv_raster)
 *   written to vt[ft[f][k]]; ft [n_faces,3] int32 is the caller's: one row of vt per distinct (chart, vertex) pair in
 *   ascending (chart, vertex) order.  Faces that share a row write the same bits.
 * lnerf_atlas_fold: a same-bucket component can still wind over itself (a helicoid).  On the packed UVs, with the
 *   pixel-space corners, candidate boxes and E_ab of lnerf_uv_raster, a texel centre is STRICTLY inside a face iff
 *   E_12, E_20 and E_01 each have the sign of the area and none is 0.  Pass A: texel_owner [R*R] int32 = the largest
 *   face index strictly covering the texel (-1 = none).  Pass B: evicted[f] = 1 for every face that strictly covers a
 *   texel it does not own, else 0.  The host makes each evicted face a chart of its own, numbered after the others
 *   in face order, and continues the shelves with their rectangles; the other faces keep their vt bits.
 *   `stages`: LNERF_UV_ITEMS (candidate counts and prefix -> counts_dev int64[1]), then LNERF_UV_COVER with n_items =
 *   that count or an upper bound.  A face with an ft index outside [0, n_vt) has no candidates.
 * Scratch sizes: the *_scratch_bytes calls (0 = arguments out of range); scratch is 16-byte aligned. */
#define LNERF_ATLAS_MAX_ROUNDS 256
#define LNERF_ATLAS_JUMP_HOPS 4
#define LNERF_ATLAS_MAX_FACES (1 << 28)
int lnerf_atlas_buckets(const float *verts, int n_verts, const int32_t *faces, int n_faces, int32_t *bucket,
                        int32_t *label, int64_t *counts_dev, lnerf_stream_t stream);
int lnerf_atlas_round(const int32_t *bucket, const int32_t *twin, int n_faces, int32_t *label, int32_t *changed_dev,
                      lnerf_stream_t stream);
size_t lnerf_atlas_compact_scratch_bytes(int n_faces);
int lnerf_atlas_compact(const int32_t *bucket, const int32_t *label, int n_faces, void *scratch, size_t scratch_bytes,
                        int32_t *face_chart, int32_t *chart_axis, int64_t *counts_dev, lnerf_stream_t stream);
size_t lnerf_atlas_boxes_scratch_bytes(int n_charts);
int lnerf_atlas_boxes(const float *verts, int n_verts, const int32_t *faces, const int32_t *bucket,
                      const int32_t *face_chart, int n_faces, int n_charts, void *scratch, size_t scratch_bytes,
                      float *chart_box, lnerf_stream_t stream);
int lnerf_atlas_uv(const float *verts, int n_verts, const int32_t *faces, const int32_t *ft, int n_faces,
                   const int32_t *face_chart, const int32_t *chart_axis, const int32_t *chart_org, const float *chart_box,
                   int n_charts, int pad, float scale, int R, float *vt, int n_vt, lnerf_stream_t stream);
size_t lnerf_atlas_fold_scratch_bytes(int n_faces, int R);
int lnerf_atlas_fold(const float *vt, int n_vt, const int32_t *ft, int n_faces, int R, int stages, int64_t n_items,
                     void *scratch, size_t scratch_bytes, int32_t *texel_owner, int32_t *evicted, int64_t *counts_dev,
                     lnerf_stream_t stream);

/* ---- mesh cleaning: connected components, a stable filter and Taubin smoothing, what NeRFRenderer.export_mesh runs
 * between marching cubes and the decimation (csrc/meshclean.hip; raymarching.mesh_components / clean_mesh / smooth_mesh).
 * Additive to ABI 7.  Device arithmetic is f32 / f64 + - * / sqrt in the order written, no fused multiply-adds; integer
 * atomics only, so every result is independent of the order in which they land and bit-reproducible (numpy restatement:
 * tests/meshclean_reference.py).  No kernel loops on anything but a bound fixed at its launch.
 *   verts [n_verts,3] f32, faces [n_faces,3] int32, n_faces <= LNERF_MESH_MAX_FACES, n_verts <= 3 LNERF_MESH_MAX_FACES.
 * Connectivity: two vertices are connected iff some face holds both (a face that repeats an index still links its
 *   distinct vertices).  A face with an index outside [0, n_verts) is skipped by every kernel of the three component
 *   calls and of the filter, which read nothing through the index (the host side refuses the mesh).
 * lnerf_mesh_components_begin: label[v] = v; counts_dev int64[1] = the number of faces with an index out of range.
 * lnerf_mesh_components_round: label[v] converges to the smallest vertex index of v's component.  One round: hook (one
 *   lane per face: m = the smallest label of its three vertices; for each corner v with m < label[v]:
 *   atomicMin(label[label[v]], m), atomicMin(label[v], m), *changed_dev = 1), then LNERF_MESH_JUMP_HOPS steps of
 *   label[v] = label[label[v]] per vertex, applied with atomicMin.  changed_dev int32[1] is cleared first.  A round that
 *   leaves it 0 changed nothing and the labels are final; the host stops at LNERF_MESH_MAX_ROUNDS and raises.
 * lnerf_mesh_components_finish: components = the roots (label[v] == v) among the REFERENCED vertices (those in at least
 *   one face), numbered 0 .. C-1 in ascending root order.  vert_comp [n_verts] (-1 for an unreferenced vertex),
 *   face_comp [n_faces] = vert_comp[faces[f][0]] (-1 for a skipped face), comp_faces [C] int32 = faces per component,
 *   comp_box [C,6] f32 = (x_lo, y_lo, z_lo, x_hi, y_hi, z_hi) over the component's vertices, by integer min / max atomics
 *   on the order-preserving encoding of lnerf_atlas_boxes (so -0 < +0).  comp_faces and comp_box have capacity
 *   min(n_verts, n_faces) rows (a component owns at least one face and one vertex), C of them written.
 *   counts_dev int64[2] = {C, referenced vertices}.
 * lnerf_mesh_filter: face_keep uint8 [n_faces], any per-face flag (a kept face with an index out of range counts as
 *   dropped).  Kept faces in their old order -> faces_out [capacity n_faces, 3], re-indexed; the vertices they reference
 *   in their old order: vert_src [capacity n_verts], vert_src[new] = old.  counts_dev int64[2] = {V_out, F_out}.
 * Keep rule of raymarching.clean_mesh (host, f64, from the f32 comp_box / comp_faces): d_a = hi_a - lo_a,
 *   diag2_c = (dx dx + dy dy) + dz dz; diag2_mesh the same from the min / max over all component boxes; a component
 *   passes iff comp_faces >= min_faces and diag2_c >= (min_diameter min_diameter) diag2_mesh; with keep_largest = k > 0
 *   only the k passing components with the most faces stay (ties to the smaller id).
 * lnerf_mesh_smooth: Taubin smoothing.  0 <= iterations <= LNERF_SMOOTH_MAX_ITER, 0 < lambda <= 1, -1.5 <= mu <= 0,
 *   anything else LNERF_ERR_INVALID_ARG.  A face with an index out of range fails the call before any kernel reads
 *   through it (one host read: the call is synchronous up to there); a face that repeats an index contributes to nothing.
 *   Incidence list of vertex v: the pairs (f, k) with faces[f][k] == v, ascending in 3 f + k (built on the device: count,
 *   scan, fill, sort).  A step with weight w reads the positions from before the step; for a vertex with n > 0
 *   incidences, per coordinate in f64: S = 0; for each incidence ascending S += p[faces[f][(k+1)%3]], then
 *   S += p[faces[f][(k+2)%3]]; mean = S / (double)(2 n); p' = (float)((double)p + (double)w * (mean - (double)p)).  A
 *   vertex without incidences keeps its position; a step with w == 0 is skipped.  One iteration = step(lambda) then
 *   step(mu) (host defaults LNERF_SMOOTH_LAMBDA, LNERF_SMOOTH_MU).  On a closed manifold mesh this is the uniform
 *   umbrella operator (every neighbour counted twice).
 *   normals_out (may be NULL), from the final positions, lnerf_decimate's definition: the f32 sum over the vertex's
 *   incident faces in ascending face order of (p1 - p0) x (p2 - p0), times 1.0f / sqrtf(l2) (0 for l2 = 0).
 *   iterations = 0 copies the vertices and still gives the normals.  verts_out [n_verts,3] must not be verts.
 * Scratch sizes: the *_scratch_bytes calls (0 = arguments out of range); scratch is 16-byte aligned. */
#define LNERF_MESH_MAX_ROUNDS 256
#define LNERF_MESH_JUMP_HOPS 4
#define LNERF_MESH_MAX_FACES (1 << 28)
#define LNERF_SMOOTH_MAX_ITER 1000
#define LNERF_SMOOTH_LAMBDA 0.5f
#define LNERF_SMOOTH_MU (-0.53f)
int lnerf_mesh_components_begin(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int64_t *counts_dev,
                                lnerf_stream_t stream);
int lnerf_mesh_components_round(const int32_t *faces, int n_verts, int n_faces, int32_t *label, int32_t *changed_dev,
                                lnerf_stream_t stream);
size_t lnerf_mesh_components_scratch_bytes(int n_verts, int n_faces);
int lnerf_mesh_components_finish(const float *verts, int n_verts, const int32_t *faces, int n_faces, const int32_t *label,
                                 void *scratch, size_t scratch_bytes, int32_t *vert_comp, int32_t *face_comp,
                                 int32_t *comp_faces, float *comp_box, int64_t *counts_dev, lnerf_stream_t stream);
size_t lnerf_mesh_filter_scratch_bytes(int n_verts, int n_faces);
int lnerf_mesh_filter(const int32_t *faces, int n_verts, int n_faces, const uint8_t *face_keep, void *scratch,
                      size_t scratch_bytes, int32_t *faces_out, int32_t *vert_src, int64_t *counts_dev,
                      lnerf_stream_t stream);
size_t lnerf_mesh_smooth_scratch_bytes(int n_verts, int n_faces);
int lnerf_mesh_smooth(const float *verts, int n_verts, const int32_t *faces, int n_faces, int iterations, float lambda,
                      float mu, void *scratch, size_t scratch_bytes, float *verts_out, float *normals_out,
                      lnerf_stream_t stream);

/* ---- Vertex gradients and edge antialiasing of the Latent-Paint renders (`optim.disp_lr`, `render.antialias`;
 * csrc/rastergrad.hip).  Additive to ABI 7; every call above is unchanged.  The geometry half of the render's backward
 * pass: each call differentiates one forward above and recomputes its terms from the same inputs.  f32, every operation
 * rounded on its own.  Shared conventions: face_idx [B*H*W], bary [B*H*W,3], face_xy [B,F,3,2] and face_z [B,F,3] are
 * what lnerf_raster_prepare_batch / lnerf_rasterize_batch wrote; the centre of pixel (i, j) is px = (2j+1)/W - 1,
 * py = 1 - (2i+1)/H; a face_idx outside [0, F) is background and nothing is read through it; 1 <= B <= 65535,
 * 1 <= H, W <= 32767, B * H * W < 2^31.  Every argument is checked before the first launch; no allocation, no
 * synchronisation, no host read-back.  The calls that ADD INTO a gradient use float atomics (their sums depend on the
 * order, within rounding); the others have one writer per element and give the same bits on every run.
 *
 * lnerf_raster_antialias_forward: image [B,H,W,C] -> out [B,H,W,C] (1 <= C <= 64; out must not be image); faces [F,3] are
 *   the mesh's vertex ids.  The depth of a pixel is d = (b0*z0 + b1*z1) + b2*z2 on its face, -inf on background; larger is
 *   nearer.  Pixel p looks at its neighbours inside the image in the order left, right, up, down, and evaluates the pair
 *   (p, n) when their face_idx differ:
 *     1. near = the pixel of larger depth, T its face; equal depths skip the pair.
 *     2. horizontal pair: the line y = py.  For the edges (0,1), (1,2), (2,0) of T with projected ends (xa,ya), (xb,yb):
 *          crosses iff (ya > py) != (yb > py);  x* = xa + (py - ya)*(xb - xa)/(yb - ya);
 *          t = (x* - x_near)/(x_far - x_near)           (x_near, x_far: the two pixel centres)
 *        the first edge in that order that crosses with 0 <= t <= 1 is taken; none: skip.  A vertical pair is the same
 *        with x and y exchanged.
 *     3. far is a face and both vertex ids of the taken edge occur in faces[far]: skip (an interior edge).
 *     4. t < 0.5: near receives (0.5 - t)*(c_far - c_near); else far receives (t - 0.5)*(c_near - c_far); c = image.
 *   out[p] = image[p] plus what lands on p, added in the neighbour order.  A pair is a function of its two pixels alone,
 *   so each pixel evaluates its own pairs and both agree: no atomics.
 * lnerf_raster_antialias_backward: grad_out [B,H,W,C] -> grad_image [B,H,W,C], OVERWRITTEN (gather form, one writer; its
 *   own buffer), through the blend weights; and grad_face_xy [B,F,3,2], ADDED INTO, through t into the two corners of the
 *   taken edge of T.  No gradient flows through the depths or through any decision.
 *
 * lnerf_raster_bary_backward: grad_bary [B*H*W,3] -> grad_face_xy, grad_face_z [B,F,3], both ADDED INTO.  The forward is
 *   lnerf_rasterize's: w0 = e0/area, w1 = e1/area, w2 = 1 - w0 - w1, q_k = w_k/z_k, b_k = q_k/(q0 + q1 + q2), with w_k
 *   recomputed from the pixel centre and the winning face (bary is not inverted).
 * lnerf_interpolate_attributes_backward_bary: grad_bary[p,k] = sum_d attr[f,k,d] * dfeat[p,d], d ascending, 0 on
 *   background; OVERWRITTEN.  attr [n_faces,3,D], 1 <= D <= 16: the half of lnerf_interpolate_attributes' backward that
 *   lnerf_interpolate_attributes_backward does not give.
 * lnerf_texture_map_backward_uv: mode 1 (bilinear) of lnerf_texture_map_forward only.  grad_uv[p] = sum_c dout[p,c] *
 *   d texture / d(u,v) at the lookup's taps, OVERWRITTEN; an axis is 0 where its clamp is active (u or v outside [0,1], or
 *   the texel position on or outside [0, R-1]) and both are 0 on background.  face_idx may be NULL (all foreground).
 * lnerf_raster_prepare_batch_backward: grad_face_xy, grad_face_z -> grad_verts [n_verts,3], OVERWRITTEN: the sum over the
 *   B views and over every face corner that references the vertex of the transpose of c = R (v - pos),
 *   ix = cx*fx/(-cz), iy = cy*fy/(-cz), z = cz.  A corner whose three incoming gradients are 0 adds nothing.
 *
 * lnerf_mesh_umbrella: the face-weighted uniform Laplacian of x [n_verts,3] and its transpose, out [n_verts,3] (not x).
 *   n_i = the number of face corners that hold vertex i.  transpose = 0:
 *     (L x)_i = x_i - (1/(2 n_i)) * sum_{faces (i,j,k)} (x_j + x_k)
 *   transpose = 1:
 *     (L^T y)_i = y_i - sum_{faces (i,j,k)} (y_j/(2 n_j) + y_k/(2 n_k))
 *   the sums over the corners i of every face; a vertex in no face gets x_i in both.  A face with an index outside
 *   [0, n_verts) counts nowhere.  n_faces = 0 copies x.  The face terms are summed with float atomics into a zeroed
 *   buffer of their own and subtracted from x in a last pass (their rounding is that of their own magnitude).  Scratch
 *   (the degrees and that buffer): lnerf_mesh_umbrella_scratch_bytes() (0 = arguments out of range; 16-byte aligned). */
int lnerf_raster_antialias_forward(const float *image, const int32_t *face_idx, const float *bary, const float *face_xy,
                                   const float *face_z, const int32_t *faces, int B, int H, int W, int C, int n_faces,
                                   float *out, lnerf_stream_t stream);
int lnerf_raster_antialias_backward(const float *grad_out, const float *image, const int32_t *face_idx,
                                    const float *bary, const float *face_xy, const float *face_z, const int32_t *faces,
                                    int B, int H, int W, int C, int n_faces, float *grad_image, float *grad_face_xy,
                                    lnerf_stream_t stream);
int lnerf_raster_bary_backward(const float *grad_bary, const int32_t *face_idx, const float *face_xy,
                               const float *face_z, int B, int H, int W, int n_faces, float *grad_face_xy,
                               float *grad_face_z, lnerf_stream_t stream);
int lnerf_interpolate_attributes_backward_bary(const int32_t *face_idx, const float *attr, const float *dfeat,
                                               int n_pixels, int D, int n_faces, float *grad_bary,
                                               lnerf_stream_t stream);
int lnerf_texture_map_backward_uv(const float *uv, const int32_t *face_idx, const float *texture, const float *dout,
                                  int n_pixels, int C, int R, float *grad_uv, lnerf_stream_t stream);
int lnerf_raster_prepare_batch_backward(const float *grad_face_xy, const float *grad_face_z, const float *verts,
                                        int n_verts, const int32_t *faces, int n_faces, const float *cams_dev, int B,
                                        float *grad_verts, lnerf_stream_t stream);
size_t lnerf_mesh_umbrella_scratch_bytes(int n_verts, int n_faces);
int lnerf_mesh_umbrella(const float *x, int n_verts, const int32_t *faces, int n_faces, int transpose, void *scratch,
                        size_t scratch_bytes, float *out, lnerf_stream_t stream);

/* ---- shaded renders (shading = "lambertian" / "textureless"): the kernels around the field (csrc/shade.hip).  Additive
 * to ABI 7.  The normal is the upstream renderer's training normal, a central finite difference of sigma at six offset
 * points; its gradient is the field's ordinary backward at 7 m points.  All arithmetic is f32 + - * / sqrt in the order
 * written here, no fused multiply-adds (numpy restatement: tests/shading_reference.py).
 *
 * lnerf_fd_points: sample i < m = min(m_host, *m_dev) (m_dev may be NULL) at x = xyzs[i] -> rows 7 i .. 7 i + 6 of pts7
 *   [7 cap, 3]: row 7 i = x; rows 7 i + 1 .. 7 i + 6 = x with ONE coordinate replaced by clamp(x_a +- eps, -bound, bound),
 *   in the order +x, -x, +y, -y, +z, -z.  m7_dev[0] = 7 m (may be NULL).  Rows >= 7 m are not touched; m_host == 0 launches
 *   nothing (m7_dev is then not written either).
 *
 * lnerf_shade_fd_forward: one wavefront per ray, rays[r] = (id, off, cnt) as in the compositing; for sample s = off + i,
 *   i < cnt, with sg = sigmas7[7 s .. 7 s + 6] (the UNSCALED densities) and albedo = rgbs7[7 s] (C channels, 1 <= C <= 4):
 *     g_a = (sg[1 + 2 a] - sg[2 + 2 a]) * inv_2eps,   s2 = (g_x g_x + g_y g_y) + g_z g_z,
 *     r = 1 / sqrt(fmax(s2, 1e-20)),   n_a = -(g_a r), a NaN component becomes 0,
 *     d = (n_x l_x + n_y l_y) + n_z l_z,   lam = ambient + (1 - ambient) * (d > 0 ? d : 0),
 *     colours[s][c] = textureless ? lam : albedo_c * lam,   sigma_c[s] = sg[0]
 *   with (l_x, l_y, l_z, ambient, textureless) = shade[min(id / rays_per_view, B - 1)] (f32 [B, 5]; l a unit vector toward
 *   the light, textureless 0 or 1).  A ray with cnt = 0 writes nothing; samples outside every span are not touched.
 *
 * lnerf_shade_fd_backward: the same launch shape; recomputes n and lam from sigmas7.  With dcol = dcolours[s], per sample
 *     dlam = textureless ? ((dcol_0 + dcol_1) + ..) : ((dcol_0 albedo_0 + dcol_1 albedo_1) + ..),
 *     dalbedo_c = textureless ? 0 : dcol_c * lam,   k = (1 - ambient) * dlam,   dn_a = d > 0 ? k * l_a : 0,
 *     q = (n_x dn_x + n_y dn_y) + n_z dn_z,   dg_a = -(r * (s2 > 1e-20 ? dn_a - n_a q : dn_a)),
 *     dsigmas7[7 s] = dsigma_c[s],   dsigmas7[7 s + 1 + 2 a] = dg_a * inv_2eps,   dsigmas7[7 s + 2 + 2 a] = -(dg_a * inv_2eps),
 *     drgbs7[7 s] = dalbedo,   drgbs7[7 s + 1 .. 7 s + 6] = 0.
 *   Every element has exactly one writer (no atomics, the same bits on every run); every row of a span is written. */
int lnerf_fd_points(const float *xyzs, float bound, float eps, int64_t m_host, const int32_t *m_dev, float *pts7,
                    int32_t *m7_dev, lnerf_stream_t stream);
int lnerf_shade_fd_forward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                           int rays_per_view, const float *shade, int B, float inv_2eps, float *sigma_c, float *colours,
                           lnerf_stream_t stream);
int lnerf_shade_fd_backward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                            int rays_per_view, const float *shade, int B, float inv_2eps, const float *dsigma_c,
                            const float *dcolours, float *dsigmas7, float *drgbs7, lnerf_stream_t stream);

/* ---- orientation regulariser of the shaded renders (Ref-NeRF's R_o, the upstream trainers' lambda_orient), fused into the
 * shade kernels (csrc/shade.hip).  Additive to ABI 7.  Per ray:  orient = sum_i w_i max(0, n_i . v)^2  -- the compositing
 * weight times the squared share of the normal that faces AWAY from the camera.  All arithmetic is f32 + - * / sqrt in the
 * order written here, no fused multiply-adds, except the weight w (expf, a 64-lane scan: tolerance-checked).  numpy
 * restatement: tests/orient_reference.py.
 *
 * lnerf_shade_fd_orient_forward: lnerf_shade_fd_forward's arguments and outputs (sigma_c and colours bit for bit), plus
 *   deltas f32 [cap, 2] = (dt, t) of the march (8-byte aligned), rays_d f32 [n_ids, 3], density_scale >= 0, T_thresh and the
 *   output orient f32 [n_ids].  For ray r with (id, off, cnt) = rays[r]:
 *     d = rays_d[id],   s_v = (d_x d_x + d_y d_y) + d_z d_z,   r_v = 1 / sqrt(fmax(s_v, 1e-20)),   v_a = d_a * r_v;
 *   per sample i < cnt, s = off + i, with n of lnerf_shade_fd_forward:
 *     c = (n_x v_x + n_y v_y) + n_z v_z,   q = c > 0 ? c : 0;
 *   w_i is THE COMPOSITING WEIGHT (lnerf_composite_rays_train_forward, above) on sigma = density_scale * sg[0].
 *   Unlike the compositing there is no early stop: behind T < T_thresh every sample still gets its sigma_c and colours
 *   (and, in the backward, its gradient rows); only w is 0.
 *     orient[id] = sum_i w_i * (q_i * q_i)   (lane partials over i = lane, lane + 64, ..; then the wave's sum; one writer).
 *   A ray with cnt = 0 writes orient[id] = 0 (and nothing else).
 *
 * lnerf_shade_fd_orient_backward: lnerf_shade_fd_backward's arguments, plus deltas, rays_d, density_scale, T_thresh as above
 *   and d_orient f32 [n_ids], the gradient w.r.t. orient.  w is DETACHED: it is recomputed as in the forward and no gradient
 *   reaches sg[0] or deltas through it.  Per sample, with go = d_orient[id]:
 *     e = go * w_i,   dn_a = (dn_a of lnerf_shade_fd_backward) + (e * (2 q)) * v_a,
 *   and the rest is lnerf_shade_fd_backward from its q = n . dn on: the projection, the seven dsigmas7 rows, the drgbs7
 *   rows.  One writer per element, no atomics, no memset, the same bits on every run.  d_orient == NULL: no gradient for
 *   the term -- the call IS lnerf_shade_fd_backward (the same kernel; deltas and rays_d are then not read). */
int lnerf_shade_fd_orient_forward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                                  int rays_per_view, const float *shade, int B, float inv_2eps, const float *deltas,
                                  const float *rays_d, float density_scale, float T_thresh, float *sigma_c, float *colours,
                                  float *orient, lnerf_stream_t stream);
int lnerf_shade_fd_orient_backward(const float *sigmas7, const float *rgbs7, int C, const int32_t *rays, int64_t N,
                                   int rays_per_view, const float *shade, int B, float inv_2eps, const float *dsigma_c,
                                   const float *dcolours, const float *deltas, const float *rays_d, float density_scale,
                                   float T_thresh, const float *d_orient, float *dsigmas7, float *drgbs7,
                                   lnerf_stream_t stream);

/* ---- distortion loss of the training renders (mip-NeRF 360's L_dist on the march's samples; optim.lambda_distortion),
 * csrc/distortion.hip.  Additive to ABI 7.  Per ray, with the compositing weights w and the samples' mid-points m:
 *   loss = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i
 * in world units of t (no normalisation to [0, 1]) -- it pulls a ray's weight into one compact interval.  All arithmetic
 * is f32 + - * in the order written here, no fused multiply-adds, except expf and the 64-lane scans (tolerance-checked).
 * numpy restatement: tests/distortion_reference.py.
 *
 * lnerf_distortion_forward: one wavefront per ray, rays[r] = (id, off, cnt) as in the compositing; sigmas f32 [cap] are
 *   the densities handed to the compositing (multiplied by density_scale already), deltas f32 [cap, 2] = (dt, t) of the
 *   march (8-byte aligned; t increases along a span, sample s covers [t, t + dt]), 0 <= T_thresh < 1.  For sample
 *   s = off + i, i < cnt, front to back, with t_0 = deltas[off][1]:
 *     w, T, e, live: THE COMPOSITING WEIGHT (lnerf_composite_rays_train_forward, above) on sigma; no early stop: behind
 *       the cut only w is 0,
 *     m = (t - t_0) + 0.5 * dt,
 *     A = sum_{j<i} w_j,   B = sum_{j<i} (w_j * m_j):  64-lane inclusive scans of w and of w * m, each taken from the
 *       previous lane (lane 0: 0) plus its scalar carry, the carries growing by lane 63's inclusive sum per chunk,
 *     u = m * A - B,
 *     loss[id] = sum_i w_i * (2 * u_i + (1.0f / 3.0f) * (w_i * dt_i))
 *   (lane partials over i = lane, lane + 64, ..; then the wave's sum; one writer), and
 *     ray_sums[id] = (A_tot, B_tot), f32 [n_ids, 2]: the two carries after the last chunk.
 *   A ray with cnt = 0 writes loss[id] = 0 and ray_sums[id] = (0, 0).  Elements of ids no ray carries are not touched.
 *
 * lnerf_distortion_backward: the same launch shape, ONE forward sweep per ray; the weights are NOT detached.  d_loss
 *   f32 [n_ids] is the gradient w.r.t. loss; loss and ray_sums are the forward's outputs.  With go = d_loss[id],
 *   G_tot = loss[id] + loss[id]  (sum_i g_i w_i = 2 L: the loss is homogeneous of degree 2 in w), and w, m, u, e, T, live
 *   recomputed as above, per sample
 *     g = 2 * ((u + u) + (B_tot - m * A_tot)) + (2.0f / 3.0f) * (w * dt)          (= dL/dw_i, from
 *         sum_{j>i} w_j = A_tot - A_i - w_i and likewise for B),
 *     P = inclusive 64-lane scan of g * w plus its scalar carry (the carry IS lane 63's P),
 *     dtau = live ? g * (T * e) - (G_tot - P) : 0                                 (= g_i T_{i+1} - sum_{j>i} g_j w_j),
 *     dsigmas[s] = (go * dt) * dtau.
 *   Every row of every span is written (zeros behind the cut); rows outside every span are not touched; a ray with
 *   cnt = 0 writes nothing.  One writer per element, no atomics, no memset, the same bits on every run.  No gradient goes
 *   to deltas.
 * Both calls refuse, before any launch: N < 0, T_thresh outside [0, 1), and for N > 0 null pointers and deltas that are
 * not 8-byte aligned. */
int lnerf_distortion_forward(const float *sigmas, const float *deltas, const int32_t *rays, int64_t N, float T_thresh,
                             float *loss, float *ray_sums, lnerf_stream_t stream);
int lnerf_distortion_backward(const float *sigmas, const float *deltas, const int32_t *rays, int64_t N, float T_thresh,
                              const float *d_loss, const float *loss, const float *ray_sums, float *dsigmas,
                              lnerf_stream_t stream);

/* ---- composited normal image of the shaded training renders and the 2D normal-smoothness stencil (the upstream
 * DreamFusion-style trainers' lambda_2d_normal_smooth; optim.lambda_normal_smooth), csrc/normal_image.hip.  Additive to
 * ABI 7.  Per ray:  normal_image = sum_i w_i n_i  -- the finite-difference normals of the samples under the compositing
 * weights; per pixel of an image: the squared differences to the right and the lower neighbour.  All arithmetic is f32
 * + - * / sqrt in the order written here, no fused multiply-adds, except expf and the 64-lane scans (tolerance-checked).
 * numpy restatement: tests/normal_image_reference.py.
 *
 * lnerf_normal_image_forward: one wavefront per ray, rays[r] = (id, off, cnt) as in the compositing; sigmas7 f32 [7 cap]
 *   are the UNSCALED densities at lnerf_fd_points' rows, deltas f32 [cap, 2] = (dt, t) of the march (8-byte aligned),
 *   density_scale >= 0, 0 <= T_thresh < 1, normal_image f32 [n_ids, 3].  For sample s = off + i, i < cnt, with
 *   sg = sigmas7[7 s .. 7 s + 6]:
 *     n of lnerf_shade_fd_forward:  g_a = (sg[1 + 2 a] - sg[2 + 2 a]) * inv_2eps,   s2 = (g_x g_x + g_y g_y) + g_z g_z,
 *       r = 1 / sqrt(fmax(s2, 1e-20)),   n_a = -(g_a r), a NaN component becomes 0;
 *     w, T, e, live: THE COMPOSITING WEIGHT (lnerf_composite_rays_train_forward, above) on sigma = density_scale * sg[0]
 *       (no early stop: behind the cut only w is 0);
 *     normal_image[id][a] = sum_i w_i * n_{i,a}   (lane partials over i = lane, lane + 64, ..; then the wave's sum; one
 *       writer).
 *   A ray with cnt = 0 writes (0, 0, 0).  Elements of ids no ray carries are not touched.
 *
 * lnerf_normal_image_backward: the same launch shape, ONE forward sweep per ray; the weights are NOT detached (upstream
 *   composites the normals with live weights).  d_normal_image f32 [n_ids, 3] is the gradient w.r.t. normal_image,
 *   normal_image the forward's output, dsigmas7 f32 [7 cap].  With dN = d_normal_image[id], N = normal_image[id], and n, s2,
 *   r, w, T, e, live recomputed as above, per sample
 *     g = (n_x dN_x + n_y dN_y) + n_z dN_z                                         (= dL/dw_i),
 *     G_tot = (N_x dN_x + N_y dN_y) + N_z dN_z                                     (= sum_i g_i w_i: N is linear in w),
 *     P = inclusive 64-lane scan of g * w plus its scalar carry (the carry IS lane 63's P),
 *     dtau = live ? g * (T * e) - (G_tot - P) : 0                                  (= g_i T_{i+1} - sum_{j>i} g_j w_j),
 *     dsigmas7[7 s] = (density_scale * dt) * dtau,
 *     dn_a = w * dN_a,   q = (n_x dn_x + n_y dn_y) + n_z dn_z,   dg_a = -(r * (s2 > 1e-20 ? dn_a - n_a q : dn_a)),
 *     dsigmas7[7 s + 1 + 2 a] = dg_a * inv_2eps,   dsigmas7[7 s + 2 + 2 a] = -(dg_a * inv_2eps)
 *   (the normalisation backward of lnerf_shade_fd_backward).  All seven rows of every span are written (behind the cut:
 *   zeros); rows outside every span are not touched; a ray with cnt = 0 writes nothing.  One writer per element, no
 *   atomics, no memset, the same bits on every run.  No gradient goes to deltas.
 *
 * lnerf_image_smooth_forward: img f32 [B, H, W, C], 1 <= C <= 4, one lane per pixel p = (b, y, x) -> loss f32 [B, H, W, 2]:
 *     loss[p][0] = x + 1 < W ? sum_c (img[b, y, x + 1, c] - img[p][c])^2 : 0,
 *     loss[p][1] = y + 1 < H ? sum_c (img[b, y + 1, x, c] - img[p][c])^2 : 0     (sums from c = 0 upward).
 * lnerf_image_smooth_backward: gather form, d_loss f32 [B, H, W, 2] -> d_img f32 [B, H, W, C]; per pixel and channel, from
 *   acc = 0 and in this order:
 *     x + 1 < W:  acc = acc - (2 * d_loss[p][0]) * (img[b, y, x + 1, c] - img[p][c])            (own-h)
 *     y + 1 < H:  acc = acc - (2 * d_loss[p][1]) * (img[b, y + 1, x, c] - img[p][c])            (own-v)
 *     x > 0:      acc = acc + (2 * d_loss[b, y, x - 1][0]) * (img[p][c] - img[b, y, x - 1, c])  (left)
 *     y > 0:      acc = acc + (2 * d_loss[b, y - 1, x][1]) * (img[p][c] - img[b, y - 1, x, c])  (up)
 *     d_img[p][c] = acc.
 *   Every element of loss / d_img is written; B, H or W = 0 launches nothing.
 * All four calls refuse, before any launch: negative sizes, T_thresh outside [0, 1), density_scale < 0, C outside 1..4, and
 * for a non-empty call null pointers and deltas that are not 8-byte aligned. */
int lnerf_normal_image_forward(const float *sigmas7, const float *deltas, const int32_t *rays, int64_t N, float inv_2eps,
                               float density_scale, float T_thresh, float *normal_image, lnerf_stream_t stream);
int lnerf_normal_image_backward(const float *sigmas7, const float *deltas, const int32_t *rays, int64_t N, float inv_2eps,
                                float density_scale, float T_thresh, const float *d_normal_image, const float *normal_image,
                                float *dsigmas7, lnerf_stream_t stream);
int lnerf_image_smooth_forward(const float *img, int B, int H, int W, int C, float *loss, lnerf_stream_t stream);
int lnerf_image_smooth_backward(const float *img, int B, int H, int W, int C, const float *d_loss, float *d_img,
                                lnerf_stream_t stream);

/* ---- Shaded Latent-Paint renders (`render.shading`; csrc/meshshade.hip): smooth vertex normals, and per pixel the
 * interpolated normal, spherical-harmonic lighting and depth, each with its transpose.  Additive to ABI 7; every call
 * above is unchanged.  The conventions of the vertex-gradient block hold: f32 throughout, every operation rounded on its
 * own in the written order; every argument is checked before the first launch; no allocation, no synchronisation, no host
 * read-back; pixel indices are 64-bit; a face_idx outside [0, F) is background and nothing is read through it;
 * 1 <= B <= 65535, 1 <= H, W <= 32767, B * H * W < 2^31, 1 <= n_faces <= LNERF_MESH_MAX_FACES, 1 <= n_verts <= (2^31-1)/3.
 * A dot product is a.b = (ax*bx + ay*by) + az*bz.  float64 restatement: tests/meshshade_reference.py.
 *
 * Vertex normals (world space, once per step for all B views).
 *   Corner table: the caller supplies it, because topology is fixed in Latent-Paint.  corner_start [V+1] and corner_list
 *   [3F] are int32; a corner id is c = 3f + k, ascending within a vertex; vertex i owns the entries corner_start[i] ..
 *   corner_start[i+1] - 1 (both clamped into [0, 3F]).  The kernel skips an entry with c outside [0, 3F) or with
 *   faces[c] != i.  A wrong table gives wrong normals but never an out-of-range access.
 *   Face normal: c_f = (v1 - v0) x (v2 - v0), l = sqrt(c.c), n_f = c_f / l.  A face with l == 0, a non-finite l, or a
 *   vertex id outside [0, V) contributes nothing.
 *   Vertex normal: s_i = sum of n_f over the vertex's corners in table order, m = sqrt(s.s), vn_i = s_i / m if m >= 1e-6,
 *   else vn_i = 0.  This is the normalised form; the fork keeps it commented out beside its mean of face normals (the
 *   unnormalised mean shortens the normal where the surface bends and so darkens creases).
 * lnerf_vertex_normals_forward: vnormals [V,3].  Gather form: one writer per vertex, identical bits on every run.
 * lnerf_vertex_normals_backward: grad_vnormals [V,3] -> grad_verts [V,3], OVERWRITTEN.  The gradient passes through both
 *   normalisations and the cross product; a zeroed vn_i or a skipped face passes nothing.  Also gather form over the
 *   corner table, with no float atomics: pass 1 writes gs_i = (g_i - vn_i (vn_i.g_i)) / m per vertex into scratch
 *   (0 where vn_i = 0); pass 2, per vertex j and per corner (f, k) of j in table order, takes dL/dn_f =
 *   (gs_v0 + gs_v1) + gs_v2, gc = (dL/dn_f - n_f (n_f.dL/dn_f)) / l, ge1 = e2 x gc, ge2 = gc x e1 (e1 = v1 - v0,
 *   e2 = v2 - v0) and adds -ge1 - ge2 (k = 0), ge1 (k = 1) or ge2 (k = 2).  One writer per vertex, identical bits on every
 *   run; it is the forward's transpose for a table that lists every corner of every face once.  Scratch (16-byte aligned):
 *   lnerf_vertex_normals_scratch_bytes(n_verts, n_faces), where 0 means arguments out of range.
 *
 * Pixel shading (one thread per pixel, 256-thread groups, no LDS).  face_idx [B*H*W], bary [B*H*W,3], face_z [B,F,3]
 * are what lnerf_raster_prepare_batch / lnerf_rasterize_batch wrote; faces [F,3]; vnormals [V,3]; lights [B,9], a device
 * array with one row per view.
 * lnerf_raster_shade_forward: outputs normal [B*H*W,3], lighting [B*H*W], depth [B*H*W].  Any output pointer may be NULL
 *   and is then skipped (all three NULL: refused).  On a foreground pixel with face f:
 *     a = (b0*vn0 + b1*vn1) + b2*vn2, where vn_k = vnormals[faces[f][k]].  A vertex id out of range makes the pixel
 *       background.
 *     m = sqrt(a.a).  n = a/m if m >= 1e-6, else n = 0.
 *     depth = -((b0*z0 + b1*z1) + b2*z2).  This is the antialias pass's d with the sign flipped, positive in front of the
 *       camera.
 *     lighting = min(max(sum_{k=0..8} lights[b,k]*Y_k(n), 1e-8), 1), summed for ascending k.
 *   The basis, with n = (x, y, z):
 *     Y0 = 0.28209479177387814          Y1 = -0.4886025119029199*y          Y2 = 0.4886025119029199*z
 *     Y3 = -0.4886025119029199*x        Y4 = 1.0925484305920792*x*y         Y5 = -1.0925484305920792*y*z
 *     Y6 = 0.94617469575755997*z*z - 0.31539156525251999                    Y7 = -1.0925484305920792*x*z
 *     Y8 = 0.5462742152960396*(x*x - y*y)
 *   (products from the left: c*x*y = (c*x)*y).  This is the nine-term real SH basis, in the order and signs of the library
 *   the fork calls.  With the fork's default lights (1,0,1, 1,0,0, 0,0,0) it reduces to 0.2821 + 0.4886 (n_z - n_x).
 *   Background pixels hold 0 in all three outputs.
 * lnerf_raster_shade_backward: grad_normal, grad_lighting, grad_depth (each may be NULL: no gradient through that output;
 *   all three NULL: refused), plus the forward's inputs.  Outputs: grad_bary [B*H*W,3], OVERWRITTEN, 0 on background;
 *   grad_vnormals [V,3] and grad_face_z [B,F,3], ADDED INTO with float atomics, as in lnerf_raster_bary_backward (their
 *   sums depend on the order, within rounding).  No gradient flows through lighting where the clamp is active (the sum
 *   below 1e-8 or above 1), through n where m < 1e-6, or through face_idx; lights gets no gradient.  All terms are
 *   recomputed from the inputs, so the forward saves nothing.  Per foreground pixel: gn = grad_normal + grad_lighting *
 *   sum_k lights[b,k] dY_k/dn;  ga = (gn - n (n.gn)) / m;  grad_bary_k = ga.vn_k - grad_depth*z_k;
 *   grad_vnormals[faces[f][k]] += ga*b_k;  grad_face_z[b,f,k] += -(grad_depth*b_k). */
int lnerf_vertex_normals_forward(const float *verts, int n_verts, const int32_t *faces, int n_faces,
                                 const int32_t *corner_start, const int32_t *corner_list, float *vnormals,
                                 lnerf_stream_t stream);
size_t lnerf_vertex_normals_scratch_bytes(int n_verts, int n_faces);
int lnerf_vertex_normals_backward(const float *grad_vnormals, const float *verts, int n_verts, const int32_t *faces,
                                  int n_faces, const int32_t *corner_start, const int32_t *corner_list, void *scratch,
                                  size_t scratch_bytes, float *grad_verts, lnerf_stream_t stream);
int lnerf_raster_shade_forward(const int32_t *face_idx, const float *bary, const float *face_z, const int32_t *faces,
                               const float *vnormals, const float *lights, int B, int H, int W, int n_faces, int n_verts,
                               float *normal, float *lighting, float *depth, lnerf_stream_t stream);
int lnerf_raster_shade_backward(const float *grad_normal, const float *grad_lighting, const float *grad_depth,
                                const int32_t *face_idx, const float *bary, const float *face_z, const int32_t *faces,
                                const float *vnormals, const float *lights, int B, int H, int W, int n_faces, int n_verts,
                                float *grad_bary, float *grad_vnormals, float *grad_face_z, lnerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LNERF_HIP_H */
