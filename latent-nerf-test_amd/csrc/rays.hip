// H1 ray generation, H2 AABB slab test, H3 Morton/bitfield, H4 occupancy-pruned march
// (training: count -> scan -> write; inference: march_rays / compact_rays).
// gfx950 only: wave64 ballot / mbcnt compaction, one wavefront per ray.  (The occupancy refresh, H10: occupancy.hip.)
#include "scan.h"

#include <math.h>
#include <string.h>

namespace lnerf {

// ------------------------------------------------------------------ H1
// pixel g of a batch of B views -> ray (origin, unit direction): camera-to-world columns are right / down / forward / eye
__device__ __forceinline__ void pixel_ray(const float *__restrict__ c2w, int H, int W, float fx, float fy, float cx,
                                          float cy, int64_t g, float o[3], float d[3]) {
    const int b = (int)(g / ((int64_t)H * W));
    const int p = (int)(g - (int64_t)b * H * W);
    const int j = p / W, i = p - j * W;
    const float *m = c2w + (int64_t)b * 16;
    const float xs = ((float)i + 0.5f - cx) / fx;
    const float ys = ((float)j + 0.5f - cy) / fy;
    const float inv = 1.0f / sqrtf(xs * xs + ys * ys + 1.0f);
    const float d0 = xs * inv, d1 = ys * inv, d2 = inv;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = d0 * m[r * 4 + 0] + d1 * m[r * 4 + 1] + d2 * m[r * 4 + 2];
        o[r] = m[r * 4 + 3];
    }
}
__global__ void __launch_bounds__(256) k_get_rays(const float *__restrict__ c2w, int B, int H, int W, float fx,
                                                  float fy, float cx, float cy, float *__restrict__ rays_o,
                                                  float *__restrict__ rays_d) {
    const int64_t total = (int64_t)B * H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        float o[3], d[3];
        pixel_ray(c2w, H, W, fx, fy, cx, cy, g, o, d);
#pragma unroll
        for (int r = 0; r < 3; ++r) { rays_o[g * 3 + r] = o[r]; rays_d[g * 3 + r] = d[r]; }
    }
}
// ray generation folded into the march's count pass (lnerf_march_rays_train_pose): camera + the buffers the rays go to
struct RayGen {
    const float *c2w;
    const float *intr;   // optional device intrinsics [B,4] = (fx, fy, cx, cy) per view: override the by-value ones, so
                         // that a replayed hipGraph can render a new camera every time (lnerf_march_rays_train_camera)
    int on, H, W;
    float fx, fy, cx, cy;
    float *ro, *rd;
};

// ------------------------------------------------------------------ H2
struct RayBox {   // axis-aligned box + minimum near distance (by value)
    float xmin, ymin, zmin, xmax, ymax, zmax, min_near;
};
__device__ __forceinline__ void ray_box(float ox, float oy, float oz, float dx, float dy, float dz, const RayBox &b,
                                        float &near, float &far) {
    const float rdx = 1.0f / dx, rdy = 1.0f / dy, rdz = 1.0f / dz;
    const float ax = (b.xmin - ox) * rdx, bx = (b.xmax - ox) * rdx;
    const float ay = (b.ymin - oy) * rdy, by = (b.ymax - oy) * rdy;
    const float az = (b.zmin - oz) * rdz, bz = (b.zmax - oz) * rdz;
    near = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    far = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    bool miss = !(far >= near);
    near = fmaxf(near, b.min_near);
    miss = miss || !(far >= near);
    if (miss) near = far = 3.4028234663852886e38f;
}
__global__ void __launch_bounds__(256) k_near_far(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                  int64_t N, RayBox box, float *__restrict__ nears,
                                                  float *__restrict__ fars) {
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        float near, far;
        ray_box(rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2], rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2],
                box, near, far);
        nears[n] = near;
        fars[n] = far;
    }
}

// ------------------------------------------------------------------ H3
__global__ void __launch_bounds__(256) k_morton3d(const int32_t *__restrict__ coords, int64_t n,
                                                  uint32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = morton3d((uint32_t)coords[i * 3], (uint32_t)coords[i * 3 + 1], (uint32_t)coords[i * 3 + 2]);
}
__global__ void __launch_bounds__(256) k_morton3d_invert(const uint32_t *__restrict__ idx, int64_t n,
                                                         int32_t *__restrict__ coords) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t v = idx[i];
        coords[i * 3] = (int32_t)compact_bits(v);
        coords[i * 3 + 1] = (int32_t)compact_bits(v >> 1);
        coords[i * 3 + 2] = (int32_t)compact_bits(v >> 2);
    }
}
// one thread per output byte; the 8 cells of a byte are two aligned float4 loads
__global__ void __launch_bounds__(256) k_packbits(const float *__restrict__ grid, int64_t n_bytes, float thresh,
                                                  const float *__restrict__ mean_dev, uint8_t *__restrict__ bits) {
    const float th = mean_dev ? fminf(thresh, *mean_dev) : thresh;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_bytes; b += (int64_t)gridDim.x * blockDim.x) {
        const float4 lo = reinterpret_cast<const float4 *>(grid)[b * 2];
        const float4 hi = reinterpret_cast<const float4 *>(grid)[b * 2 + 1];
        uint32_t v = 0;
        v |= (lo.x > th) ? 1u : 0u;
        v |= (lo.y > th) ? 2u : 0u;
        v |= (lo.z > th) ? 4u : 0u;
        v |= (lo.w > th) ? 8u : 0u;
        v |= (hi.x > th) ? 16u : 0u;
        v |= (hi.y > th) ? 32u : 0u;
        v |= (hi.z > th) ? 64u : 0u;
        v |= (hi.w > th) ? 128u : 0u;
        bits[b] = (uint8_t)v;
    }
}

// ------------------------------------------------------------------ H4 occupancy test
struct MarchParams {
    float bound;
    int cascade;
    int G;
    int max_steps;
    float dt_gamma;
    float dt_min;
    float dt_max;
    float dt_uniform;   // the step at dt_gamma = 0: clampf(0, dt_min, dt_max), which is dt_max where dt_min > dt_max
};

// x already clamped to [-bound, bound].  Op order mirrors oracle/nerf_oracle.py::march_cell_index.
__device__ __forceinline__ bool cell_occupied(float x, float y, float z, float dt, const MarchParams &P,
                                              const uint8_t *__restrict__ bitfield) {
    int level = 0;
    float mip_bound = fminf(1.0f, P.bound);
    if (P.cascade > 1) {
        const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
        int e0, e1;
        (void)frexpf(mx, &e0);
        (void)frexpf(dt * (0.5f * (float)P.G), &e1);
        e0 = min(P.cascade - 1, max(0, e0));
        e1 = min(P.cascade - 1, max(0, e1));
        level = max(e0, e1);
        mip_bound = fminf(ldexpf(1.0f, level), P.bound);
    }
    const float rb = 1.0f / mip_bound;
    const float halfG = 0.5f * (float)P.G;
    const float gm1 = (float)(P.G - 1);
    float ux = x * rb, uy = y * rb, uz = z * rb;
    ux = ux + 1.0f; uy = uy + 1.0f; uz = uz + 1.0f;
    ux = ux * halfG; uy = uy * halfG; uz = uz * halfG;
    const uint32_t nx = (uint32_t)(int)clampf(ux, 0.0f, gm1);
    const uint32_t ny = (uint32_t)(int)clampf(uy, 0.0f, gm1);
    const uint32_t nz = (uint32_t)(int)clampf(uz, 0.0f, gm1);
    const uint32_t idx = (uint32_t)level * (uint32_t)(P.G * P.G * P.G) + morton3d(nx, ny, nz);
    return (bitfield[idx >> 3] >> (idx & 7u)) & 1u;
}

// Per-ray jitter of the march start.  Either a table of values (the upstream `noises = torch.rand(N)`), or a
// counter-based generator: u = hash(ray, seed, *counter) in [0,1).  The counter lives on the device and is advanced
// by the scan pass of every call, so a replayed hipGraph draws fresh jitter without any host-side RNG state
// (torch.rand inside a captured graph costs three extra kernels per replay: measured 33 us per step).
struct MarchNoise {
    const float *values;     // [N] or null
    const int32_t *counter;  // device counter or null
    uint32_t seed;
    int bias;                // the write pass runs after the scan pass has advanced the counter: bias 1
};
__device__ __forceinline__ float march_noise(const MarchNoise &nz, int64_t n) {
    if (nz.values) return nz.values[n];
    if (!nz.counter) return 0.0f;
    return hash_unit(counter_hash((uint32_t)n, nz.seed, (uint32_t)(*nz.counter - nz.bias), 0u));
}

// ---- the training march in its parts.  k_march_train reads top to bottom: load the ray (march_ray), find its span
// (march_span), walk it (MarchWalk::chunk per 64 lattice points), record it; the capacity rule is march_dropped, the
// totals have one writer (march_write_totals).
struct MarchRays {   // where the rays come from (by value)
    const float *o, *d;          // [N,3]; with gen.on the count pass writes them (gen.ro / gen.rd are these buffers)
    const float *nears, *fars;   // [N] from lnerf_near_far_from_aabb -- or null: clip against `box` here
    RayBox box;
    RayGen gen;
};
struct MarchOut {   // where the march goes (by value)
    float *xyzs, *dirs, *deltas;   // [capacity, 3 / 3 / 2]
    int32_t *rays;                 // [N,3] = (ray, offset, count)
    int32_t *cnt;                  // scan-free form: [N] counts + [ceil(N / 4)] workgroup sums; null: k_march_scan runs
    int64_t capacity;
    int32_t *counter;              // [4] = M, live rays, dropped rays, running peak
    int32_t *noise_counter;        // the jitter generator's device counter or null
};

// The capacity rule: a ray is dropped when the samples of all rays before it (dropped or not) plus its own exceed the
// capacity.
__device__ __forceinline__ bool march_dropped(int count, long long samples_before, int64_t capacity) {
    return count > 0 && samples_before + count > capacity;
}
// The totals of a march, by the ONE thread that has them: all samples, the largest end of a kept span, kept non-empty
// rays, dropped rays.  Word 3 is the running maximum, over the marches since the caller last zeroed it, of
// M | (rays dropped ? 2^30 : 0)  -- what a training loop that sizes its sample buffers from observed marches reads back
// once in a while (NeRFRenderer.update_sample_budget): no launch, no atomics.  Advances the jitter counter: the count
// pass has drawn this call's jitter (the scan-free write pass takes it from rays[][1]; behind k_march_scan the write
// pass undoes the step: bias 1).
__device__ __forceinline__ void march_write_totals(const MarchOut &out, long long total, long long best, int live,
                                                   int drop) {
    // M: all samples when nothing was dropped, else the end of the last kept span
    const int32_t m = drop > 0 ? (int32_t)best : (int32_t)(total > out.capacity ? out.capacity : total);
    out.counter[0] = m;
    out.counter[1] = live;
    out.counter[2] = drop;
    const int32_t word = m | (drop > 0 ? (1 << 30) : 0);
    const int32_t old = out.counter[3];
    out.counter[3] = word > old ? word : old;
    if (out.noise_counter) *out.noise_counter += 1;
}
// Totals of a training march from the per-ray counts, by ONE wavefront (every lane must call it): what k_march_scan
// writes to `counter`.  64 rays per round: inclusive wave scan + running carry.
constexpr int64_t MARCH_FUSED_MAX_RAYS = 8192;   // above: the per-wavefront prefix (N^2 / 2 loads) loses to the scan kernel
__device__ __forceinline__ void march_totals(const MarchOut &out, int64_t N) {
    const int lane = lane_id();
    long long carry = 0, best = 0;
    int live = 0, drop = 0;
    for (int64_t base = 0; base < N; base += 64) {
        const int64_t i = base + lane;
        const int c = i < N ? out.cnt[i] : 0;   // (one round trip per 64 rays: this is the rare overflow path)
        const long long inc = wave_inclusive_sum_ll(c);
        const long long off = carry + inc - c;
        const bool dropped = march_dropped(c, off, out.capacity);
        if (c > 0 && !dropped) { ++live; best = off + c > best ? off + c : best; }
        drop += dropped ? 1 : 0;
        carry += __shfl(inc, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        live += __shfl_xor(live, o, 64);
        drop += __shfl_xor(drop, o, 64);
        const long long u = __shfl_xor(best, o, 64);
        best = u > best ? u : best;
    }
    if (lane == 0) march_write_totals(out, carry, best, live, drop);
}

// The ray of wavefront n and its [near, far).  The ray: generated here by the count pass of the `_pose` / `_camera`
// forms (k_get_rays' arithmetic; written out for the write pass and the caller), else read.  The span: the AABB clip of
// lnerf_near_far_from_aabb, here (one dispatch less per view, same arithmetic), or that call's table.
template <bool WRITE>
__device__ __forceinline__ void march_ray(const MarchRays &R, int64_t n, int lane, float ro[3], float rd[3], float &near,
                                          float &far) {
    const RayGen &gen = R.gen;
    if (!WRITE && gen.on) {
        float fx = gen.fx, fy = gen.fy, cx = gen.cx, cy = gen.cy;
        if (gen.intr) {   // (wave-uniform: one ray per wavefront)
            const float *k = gen.intr + (n / ((int64_t)gen.H * gen.W)) * 4;
            fx = k[0]; fy = k[1]; cx = k[2]; cy = k[3];
        }
        pixel_ray(gen.c2w, gen.H, gen.W, fx, fy, cx, cy, n, ro, rd);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { gen.ro[n * 3 + r] = ro[r]; gen.rd[n * 3 + r] = rd[r]; }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) { ro[r] = R.o[n * 3 + r]; rd[r] = R.d[n * 3 + r]; }
    }
    if (!R.nears) {
        ray_box(ro[0], ro[1], ro[2], rd[0], rd[1], rd[2], R.box, near, far);
    } else {
        near = R.nears[n]; far = R.fars[n];
    }
}

// Where a ray's samples go, how many it may write, and its jitter.
struct MarchSpan {
    int64_t offset;
    int budget;   // 0 if the ray was dropped for capacity
    float jitter;
};
// The span of ray n in the write pass of the scan-free form (N <= MARCH_FUSED_MAX_RAYS): the count pass left every
// ray's count in `cnt`, every workgroup's (4 rays') sum and number of non-empty rays in cnt[N + workgroup], and the
// ray's jitter in rays[n][1]; this wavefront sums what lies before its ray -- what the single-workgroup scan kernel
// between the two passes did, without that dispatch (7 us of launch latency for 2 us of work).  One batch of loads for
// 4096 rays.  `cnt` is never modified here, so every wavefront sees the original counts whatever the others have already
// written.  The jitter is taken out of rays[n][1] and the offset put there; the last ray's wavefront writes the totals.
__device__ __forceinline__ MarchSpan march_span(const MarchOut &out, int64_t n, int64_t N, int lane) {
    const int32_t *wg = out.cnt + N;
    const int64_t w = n >> 2;
    long long part = 0;
    int nonempty = 0;
    for (int64_t j0 = 0; j0 < w; j0 += 1024) {   // sixteen loads in flight per lane
        int v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t j = j0 + k * 64 + lane;
            v[k] = j < w ? wg[j] : 0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { part += v[k] & 0xFFFFFF; nonempty += v[k] >> 28; }
    }
    {   // the rays of this ray's own workgroup that come before it
        const int64_t i = 4 * w + lane;
        const int c = (lane < 4 && i < n) ? out.cnt[i] : 0;
        part += c;
        nonempty += c > 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        part += __shfl_xor(part, o, 64);
        nonempty += __shfl_xor(nonempty, o, 64);
    }
    const int c = out.cnt[n];
    const bool dropped = march_dropped(c, part, out.capacity);
    const MarchSpan span{dropped ? 0 : part, dropped ? 0 : c, __int_as_float(out.rays[n * 3 + 1])};
    if (lane == 0) {
        out.rays[n * 3 + 1] = (int32_t)span.offset;
        if (dropped) out.rays[n * 3 + 2] = 0;
    }
    if (n == N - 1) {   // the last ray's wavefront has the totals at hand
        if (part + c <= out.capacity) {
            if (lane == 0) march_write_totals(out, part + c, 0, nonempty + (c > 0 ? 1 : 0), 0);
        } else {
            march_totals(out, N);   // rays were dropped: the scan's bookkeeping
        }
    }
    return span;
}

// chunks of 64 lattice points whose occupancy bytes one round of the uniform-step march requests together
constexpr int MARCH_CHUNKS = 4;
// The chunk rule, once.  A wavefront has tested 64 consecutive lattice points of its ray: ballot + popcount gives the
// count (pass 1) or, with mbcnt, each sample's slot (pass 2), until the ray's budget is used up.
template <bool WRITE>
struct MarchWalk {
    int count, budget;
    int64_t offset;
    float dx, dy, dz;
    // valid: this lane's point lies before `far`; occupied: the cell of (x, y, z), the clamped point, is.  True: the
    // ray is finished.
    __device__ __forceinline__ bool chunk(const MarchOut &out, bool valid, bool occupied, float x, float y, float z,
                                          float dt, float t) {
        if (__ballot(valid) == 0ull) return true;  // lattice is monotone: nothing further is valid
        const bool occ = valid && occupied;
        const unsigned long long mask = __ballot(occ);
        const int rank = count + mbcnt(mask);
        if (WRITE && occ && rank < budget) {
            const int64_t s = offset + rank;
            // one 12-byte store per position / direction, one 8-byte store per (dt, t) pair
            *reinterpret_cast<float3 *>(out.xyzs + s * 3) = make_float3(x, y, z);
            *reinterpret_cast<float3 *>(out.dirs + s * 3) = make_float3(dx, dy, dz);
            *reinterpret_cast<float2 *>(out.deltas + s * 2) = make_float2(dt, t);
        }
        count += __popcll(mask);
        if (count < budget) return false;
        count = budget;
        return true;
    }
};

// One wavefront per ray, two passes: count (WRITE = false), then write.
template <bool WRITE, bool UNIFORM_DT>
__global__ void __launch_bounds__(256)
k_march_train(MarchRays R, int64_t N, const uint8_t *__restrict__ bitfield, MarchParams P, MarchNoise noises,
              MarchOut out) {
    const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    const int lane = lane_id();
    int count = 0;
    if (n < N) {
        float ro[3], rd[3], near, far;
        march_ray<WRITE>(R, n, lane, ro, rd, near, far);
        MarchSpan span{0, P.max_steps, 0.f};
        if (WRITE && out.cnt) span = march_span(out, n, N, lane);
        else if (WRITE) span = MarchSpan{out.rays[n * 3 + 1], out.rays[n * 3 + 2], 0.f};   // (k_march_scan's)
        if (near < far && span.budget > 0) {
            const float ox = ro[0], oy = ro[1], oz = ro[2];
            const float dx = rd[0], dy = rd[1], dz = rd[2];
            const float dt0 = clampf(near * P.dt_gamma, P.dt_min, P.dt_max);
            const float noise = (WRITE && out.cnt) ? span.jitter : march_noise(noises, n);
            if (!WRITE && out.cnt && lane == 0) out.rays[n * 3 + 1] = __float_as_int(noise);   // hand the jitter to the write pass
            const float t0 = near + dt0 * noise;
            MarchWalk<WRITE> walk{0, span.budget, span.offset, dx, dy, dz};
            if (UNIFORM_DT) {
                // Closed-form lattice: MARCH_CHUNKS chunks of 64 lattice points per round, their occupancy bytes requested together
                // -- the pass is a chain of dependent L2 round trips (one per chunk, ~16 per ray), this makes it ~16 / MARCH_CHUNKS.  Chunks
                // past the ray's end read a clamped (valid) cell and are ignored; the decisions and their order are those
                // of the one-chunk loop below.
                const float dt = P.dt_uniform;   // the one step rule at t * dt_gamma = 0
                bool done = false;
                for (int base = 0; base < (1 << 22) && !done; base += 64 * MARCH_CHUNKS) {  // bound: a non-finite `far` must not spin
                    float tj[MARCH_CHUNKS], xj[MARCH_CHUNKS], yj[MARCH_CHUNKS], zj[MARCH_CHUNKS];
                    bool vj[MARCH_CHUNKS], oj[MARCH_CHUNKS];
#pragma unroll
                    for (int j = 0; j < MARCH_CHUNKS; ++j) {
                        float tt = (float)(base + 64 * j + lane) * dt;
                        tt = tt + t0;
                        tj[j] = tt;
                        vj[j] = tt < far;
                        float x = dx * tt, y = dy * tt, z = dz * tt;
                        x = x + ox; y = y + oy; z = z + oz;
                        xj[j] = clampf(x, -P.bound, P.bound);
                        yj[j] = clampf(y, -P.bound, P.bound);
                        zj[j] = clampf(z, -P.bound, P.bound);
                    }
#pragma unroll
                    for (int j = 0; j < MARCH_CHUNKS; ++j) oj[j] = cell_occupied(xj[j], yj[j], zj[j], dt, P, bitfield);
#pragma unroll
                    for (int j = 0; j < MARCH_CHUNKS && !done; ++j)
                        done = walk.chunk(out, vj[j], oj[j], xj[j], yj[j], zj[j], dt, tj[j]);
                }
            } else {
                // The step recurrence t = t + clamp(t * dt_gamma): lane l starts at lattice point l and moves 64 points per chunk
                float t = t0;
                for (int i = 0; i < lane; ++i) t = t + clampf(t * P.dt_gamma, P.dt_min, P.dt_max);
                for (int base = 0; base < (1 << 22); base += 64) {  // bound: a non-finite `far` must not spin
                    const float dt = clampf(t * P.dt_gamma, P.dt_min, P.dt_max);
                    const bool valid = t < far;
                    float x = dx * t, y = dy * t, z = dz * t;
                    x = x + ox; y = y + oy; z = z + oz;
                    x = clampf(x, -P.bound, P.bound);
                    y = clampf(y, -P.bound, P.bound);
                    z = clampf(z, -P.bound, P.bound);
                    if (walk.chunk(out, valid, valid && cell_occupied(x, y, z, dt, P, bitfield), x, y, z, dt, t)) break;
                    for (int i = 0; i < 64; ++i) t = t + clampf(t * P.dt_gamma, P.dt_min, P.dt_max);
                }
            }
            count = walk.count;
        }
        if (!WRITE && lane == 0) {
            out.rays[n * 3] = (int32_t)n;
            if (!(out.cnt && near < far)) out.rays[n * 3 + 1] = 0;   // (scan-free form: the jitter of a marched ray sits here)
            out.rays[n * 3 + 2] = count;
            if (out.cnt) out.cnt[n] = count;
        }
    }
    if (!WRITE && out.cnt) {   // per workgroup: samples in bits [0,24) (4 rays x <= 65536 steps), non-empty rays in [28,31)
        __shared__ int s_count[4];   // (a wavefront past the last ray counts 0: every wavefront meets the barrier)
        if (lane == 0) s_count[threadIdx.x >> 6] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0, ne = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { sum += s_count[k]; ne += s_count[k] > 0 ? 1 : 0; }
            out.cnt[N + blockIdx.x] = sum | (ne << 28);
        }
    }
}

// Single-workgroup exclusive scan of the per-ray counts (N is a few thousand per view).
// Also counts live rays and drops rays that would overflow `capacity`.
// Every thread owns K = ceil(N / 1024) CONSECUTIVE rays: a local sum, ONE block-wide scan of the 1024 sums, then the
// thread walks its rays again with its base offset -- two barriers for any N (a chunk-of-1024 loop met at three barriers
// per chunk; the kernel is latency from end to end).
__global__ void __launch_bounds__(1024) k_march_scan(MarchOut out, int64_t N) {
    int32_t *__restrict__ rays = out.rays;
    __shared__ long long wave_best[16];
    const int tid = threadIdx.x;
    const int64_t K = (N + 1023) / 1024;
    const int64_t n0 = (int64_t)tid * K, n1 = (n0 + K < N) ? n0 + K : N;
    long long mine[1] = {0}, before[1], total[1];
    for (int64_t n = n0; n < n1; ++n) mine[0] += rays[n * 3 + 2];
    block_exclusive_scan<1024>(mine, before, total);
    long long off = before[0], best = 0;
    int kept[2] = {0, 0}, unused[2], sum[2];   // live rays, dropped rays
    for (int64_t n = n0; n < n1; ++n) {
        const int c = rays[n * 3 + 2];
        const bool dropped = march_dropped(c, off, out.capacity);
        rays[n * 3 + 1] = (int32_t)(dropped ? 0 : off);
        if (dropped) rays[n * 3 + 2] = 0;
        if (c > 0 && !dropped) { ++kept[0]; best = off + c; }   // (empty rays carry a meaningless offset)
        kept[1] += dropped ? 1 : 0;
        off += c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(best, o, 64);
        best = u > best ? u : best;
    }
    if (lane_id() == 0) wave_best[tid >> 6] = best;
    block_exclusive_scan<1024>(kept, unused, sum);   // (int counters: other slots than the scan above; its barrier publishes wave_best)
    if (tid == 0) {
        for (int w = 0; w < 16; ++w) best = wave_best[w] > best ? wave_best[w] : best;
        march_write_totals(out, total[0], best, sum[0], sum[1]);
    }
}

// ------------------------------------------------------------------ H4 inference
// One thread per alive ray: emit up to n_step occupied lattice samples starting at rays_t.
__global__ void __launch_bounds__(256)
k_march_rays(int64_t n_alive, int n_step, const int32_t *__restrict__ rays_alive, const float *__restrict__ rays_t,
             const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ fars,
             const uint8_t *__restrict__ bitfield, MarchParams P, float *__restrict__ xyzs, float *__restrict__ dirs,
             float *__restrict__ deltas) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_alive) return;
    const int32_t n = rays_alive[i];
    float *px = xyzs + i * n_step * 3, *pd = dirs + i * n_step * 3, *pt = deltas + i * n_step * 2;
    int step = 0;
    if (n >= 0) {
        const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
        const float dx = rays_d[n * 3], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
        const float far = fars[n];
        float t = rays_t[n];
        int guard = 0;
        while (t < far && step < n_step && guard < (1 << 22)) {
            const float dt = clampf(t * P.dt_gamma, P.dt_min, P.dt_max);
            float x = dx * t, y = dy * t, z = dz * t;
            x = x + ox; y = y + oy; z = z + oz;
            x = clampf(x, -P.bound, P.bound);
            y = clampf(y, -P.bound, P.bound);
            z = clampf(z, -P.bound, P.bound);
            if (cell_occupied(x, y, z, dt, P, bitfield)) {
                px[step * 3] = x; px[step * 3 + 1] = y; px[step * 3 + 2] = z;
                pd[step * 3] = dx; pd[step * 3 + 1] = dy; pd[step * 3 + 2] = dz;
                pt[step * 2] = dt; pt[step * 2 + 1] = t;
                ++step;
            }
            t = t + dt;
            ++guard;
        }
    }
    for (; step < n_step; ++step) {  // padding: dt = 0 contributes nothing; t < 0 marks "ray exhausted"
        px[step * 3] = 0.f; px[step * 3 + 1] = 0.f; px[step * 3 + 2] = 0.f;
        pd[step * 3] = 0.f; pd[step * 3 + 1] = 0.f; pd[step * 3 + 2] = 1.f;
        pt[step * 2] = 0.f; pt[step * 2 + 1] = -1.f;
    }
}

__global__ void __launch_bounds__(256)
k_composite_rays(int64_t n_alive, int n_step, int32_t *__restrict__ rays_alive, float *__restrict__ rays_t,
                 const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                 int C, float T_thresh, float *__restrict__ weights_sum, float *__restrict__ depth,
                 float *__restrict__ image, float *__restrict__ transmittance) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_alive) return;
    const int32_t n = rays_alive[i];
    if (n < 0) return;
    const float *sg = sigmas + i * n_step, *rg = rgbs + i * n_step * C, *dl = deltas + i * n_step * 2;
    float T = transmittance[n], ws = weights_sum[n], d = depth[n];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) acc[c] = image[n * C + c];
    float t_last = rays_t[n];
    bool alive = true;
    int step = 0;
    for (; step < n_step; ++step) {
        const float dt = dl[step * 2], t = dl[step * 2 + 1];
        if (t < 0.f) { alive = false; break; }  // march ran past `far`
        const float alpha = 1.0f - __expf(-sg[step] * dt);
        const float w = alpha * T;
        ws += w;
        d = fmaf(w, t, d);
        for (int c = 0; c < C; ++c) acc[c] = fmaf(w, rg[step * C + c], acc[c]);
        T *= 1.0f - alpha;
        t_last = t + dt;
        if (T < T_thresh) { alive = false; break; }
    }
    transmittance[n] = T;
    weights_sum[n] = ws;
    depth[n] = d;
    for (int c = 0; c < C; ++c) image[n * C + c] = acc[c];
    rays_t[n] = t_last;
    if (!alive) rays_alive[i] = -1;
}

// Live-ray compaction: keep entries >= 0, preserve order.  Single workgroup; round k of a pass is its k-th 1024
// consecutive entries, and the COMPACT_ROUNDS rounds of a pass share one block scan: two barriers per 4096 entries.
constexpr int COMPACT_ROUNDS = 4;   // (8: the scan's 8 x 16 wave sums per thread spill)
__global__ void __launch_bounds__(1024) k_compact_rays(const int32_t *__restrict__ in, int64_t n,
                                                       int32_t *__restrict__ out, int32_t *__restrict__ n_out) {
    int carry = 0;
    for (int64_t base = threadIdx.x; base < n + threadIdx.x; base += 1024 * COMPACT_ROUNDS) {   // (workgroup-uniform trip count)
        int32_t v[COMPACT_ROUNDS];
        int keep[COMPACT_ROUNDS], rank[COMPACT_ROUNDS], total[COMPACT_ROUNDS];
#pragma unroll
        for (int k = 0; k < COMPACT_ROUNDS; ++k) {
            v[k] = base + k * 1024 < n ? in[base + k * 1024] : -1;
            keep[k] = v[k] >= 0 ? 1 : 0;
        }
        block_exclusive_scan<1024>(keep, rank, total);
#pragma unroll
        for (int k = 0; k < COMPACT_ROUNDS; ++k) {
            if (keep[k]) out[carry + rank[k]] = v[k];
            carry += total[k];
        }
        __syncthreads();   // the next pass reuses the scan's slots
    }
    if (threadIdx.x == 0) *n_out = carry;
}

static MarchParams make_params(float bound, int cascade, int G, int max_steps, float dt_gamma) {
    MarchParams P;
    P.bound = bound;
    P.cascade = cascade;
    P.G = G;
    P.max_steps = max_steps;
    P.dt_gamma = dt_gamma;
    P.dt_min = (float)(2.0 * 1.7320508075688772 / (double)max_steps);
    P.dt_max = (float)(2.0 * 1.7320508075688772 * (double)(1 << (cascade - 1)) / (double)G);
    P.dt_uniform = fminf(fmaxf(0.0f, P.dt_min), P.dt_max);   // clampf's order of min and max
    return P;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_get_rays(const float *c2w, int B, int H, int W, float fx, float fy, float cx, float cy, float *rays_o,
                   float *rays_d, lnerf_stream_t stream) {
    LNERF_REQUIRE(c2w && rays_o && rays_d, "get_rays: null pointer");
    LNERF_REQUIRE(B > 0 && H > 0 && W > 0, "get_rays: B,H,W must be positive (got %d,%d,%d)", B, H, W);
    LNERF_REQUIRE(fx != 0.f && fy != 0.f, "get_rays: zero focal length");
    const int64_t total = (int64_t)B * H * W;
    hipLaunchKernelGGL(k_get_rays, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), c2w, B, H, W, fx, fy, cx, cy,
                       rays_o, rays_d);
    LNERF_CHECK_LAUNCH("get_rays");
    return LNERF_OK;
}

int lnerf_near_far_from_aabb(const float *rays_o, const float *rays_d, int64_t N, float xmin, float ymin, float zmin,
                             float xmax, float ymax, float zmax, float min_near, float *nears, float *fars,
                             lnerf_stream_t stream) {
    LNERF_REQUIRE(N >= 0, "near_far_from_aabb: negative N");
    if (N == 0) return LNERF_OK;
    LNERF_REQUIRE(rays_o && rays_d && nears && fars, "near_far_from_aabb: null pointer");
    LNERF_REQUIRE(xmin <= xmax && ymin <= ymax && zmin <= zmax, "near_far_from_aabb: inverted aabb");
    const RayBox box{xmin, ymin, zmin, xmax, ymax, zmax, min_near};
    hipLaunchKernelGGL(k_near_far, dim3(grid_for(N)), dim3(256), 0, as_stream(stream), rays_o, rays_d, N, box, nears, fars);
    LNERF_CHECK_LAUNCH("near_far_from_aabb");
    return LNERF_OK;
}

int lnerf_morton3d(const int32_t *coords, int64_t n, uint32_t *indices, lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0, "morton3d: negative n");
    if (n == 0) return LNERF_OK;
    LNERF_REQUIRE(coords && indices, "morton3d: null pointer");
    hipLaunchKernelGGL(k_morton3d, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), coords, n, indices);
    LNERF_CHECK_LAUNCH("morton3d");
    return LNERF_OK;
}

int lnerf_morton3d_invert(const uint32_t *indices, int64_t n, int32_t *coords, lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0, "morton3d_invert: negative n");
    if (n == 0) return LNERF_OK;
    LNERF_REQUIRE(coords && indices, "morton3d_invert: null pointer");
    hipLaunchKernelGGL(k_morton3d_invert, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), indices, n, coords);
    LNERF_CHECK_LAUNCH("morton3d_invert");
    return LNERF_OK;
}

int lnerf_packbits(const float *grid, int64_t n_cells, float thresh, const float *mean_dev, uint8_t *bitfield,
                   lnerf_stream_t stream) {
    LNERF_REQUIRE(n_cells >= 0 && n_cells % 8 == 0, "packbits: n_cells (%lld) must be a multiple of 8",
                  (long long)n_cells);
    if (n_cells == 0) return LNERF_OK;
    LNERF_REQUIRE(grid && bitfield, "packbits: null pointer");
    LNERF_REQUIRE(((uintptr_t)grid & 15) == 0, "packbits: grid must be 16-byte aligned");
    hipLaunchKernelGGL(k_packbits, dim3(grid_for(n_cells / 8)), dim3(256), 0, as_stream(stream), grid, n_cells / 8,
                       thresh, mean_dev, bitfield);
    LNERF_CHECK_LAUNCH("packbits");
    return LNERF_OK;
}

static int check_march_common(const char *who, float bound, int cascade, int grid_size, int max_steps, float dt_gamma) {
    LNERF_REQUIRE(bound > 0.f, "%s: bound must be > 0", who);
    LNERF_REQUIRE(cascade >= 1 && cascade <= 8, "%s: cascade must be in [1,8] (got %d)", who, cascade);
    LNERF_REQUIRE(grid_size >= 8 && grid_size <= 1024 && (grid_size & (grid_size - 1)) == 0,
                  "%s: grid_size must be a power of two in [8,1024] (got %d)", who, grid_size);
    LNERF_REQUIRE((int64_t)cascade * grid_size * grid_size * grid_size <= (int64_t)1 << 31,
                  "%s: occupancy grid too large", who);
    LNERF_REQUIRE(max_steps >= 1 && max_steps <= 65536, "%s: max_steps out of range (%d)", who, max_steps);
    LNERF_REQUIRE(dt_gamma >= 0.f, "%s: dt_gamma must be >= 0", who);
    return LNERF_OK;
}

// `clip`: R.box instead of the nears / fars tables (the forms that went through march_source)
static int march_train_impl(MarchRays R, bool clip, int64_t N, const uint8_t *bitfield, float bound, int cascade,
                            int grid_size, int max_steps, float dt_gamma, const float *noises, uint32_t noise_seed,
                            int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs, float *deltas,
                            int32_t *rays, int32_t *counter, lnerf_stream_t stream) {
    int rc = check_march_common("march_rays_train", bound, cascade, grid_size, max_steps, dt_gamma);
    if (rc) return rc;
    LNERF_REQUIRE(N >= 0 && N <= ((int64_t)1 << 24), "march_rays_train: N out of range (%lld)", (long long)N);
    LNERF_REQUIRE(capacity >= 0 && capacity <= 0x7FFFFFFFll, "march_rays_train: capacity out of range");
    LNERF_REQUIRE(counter, "march_rays_train: null counter");
    LNERF_REQUIRE(!(noises && noise_counter), "march_rays_train: give either a noise table or a noise counter");
    if (N == 0) {
        (void)hipMemsetAsync(counter, 0, 4 * sizeof(int32_t), as_stream(stream));
        return LNERF_OK;
    }
    LNERF_REQUIRE(R.o && R.d && (clip || (R.nears && R.fars)) && bitfield && rays, "march_rays_train: null pointer");
    LNERF_REQUIRE(capacity == 0 || (xyzs && dirs && deltas), "march_rays_train: null sample buffers");
    const MarchParams P = make_params(bound, cascade, grid_size, max_steps, dt_gamma);
    const dim3 block(256), grid((unsigned)div_up(N, 4));  // 4 wavefronts (rays) per workgroup
    hipStream_t s = as_stream(stream);
    MarchNoise nz{noises, noise_counter, noise_seed, 0};
    // up to MARCH_FUSED_MAX_RAYS rays: two dispatches (the write pass sums the counts before its ray itself; the counts
    // live behind the four totals in `counter`, see lnerf_march_counter_len); more: count, scan, write
    const MarchOut out{xyzs, dirs, deltas, rays, N <= MARCH_FUSED_MAX_RAYS ? counter + 4 : nullptr, capacity, counter,
                       noise_counter};
    auto pass = [&](auto uniform_dt, auto recurrence) {
        hipLaunchKernelGGL(dt_gamma == 0.f ? uniform_dt : recurrence, grid, block, 0, s, R, N, bitfield, P, nz, out);
    };
    pass(k_march_train<false, true>, k_march_train<false, false>);
    LNERF_CHECK_LAUNCH("march_rays_train(count)");
    if (!out.cnt) {
        hipLaunchKernelGGL(k_march_scan, dim3(1), dim3(1024), 0, s, out, N);
        LNERF_CHECK_LAUNCH("march_rays_train(scan)");
        nz.bias = 1;
    }
    pass(k_march_train<true, true>, k_march_train<true, false>);
    LNERF_CHECK_LAUNCH("march_rays_train(write)");
    return LNERF_OK;
}

int64_t lnerf_march_counter_len(int64_t N) { return 4 + (N >= 0 && N <= MARCH_FUSED_MAX_RAYS ? N + (N + 3) / 4 : 0); }

int lnerf_march_rays_train(const float *rays_o, const float *rays_d, const float *nears, const float *fars, int64_t N,
                           const uint8_t *bitfield, float bound, int cascade, int grid_size, int max_steps,
                           float dt_gamma, const float *noises, uint32_t noise_seed, int32_t *noise_counter,
                           int64_t capacity, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                           lnerf_stream_t stream) {
    MarchRays R{};
    R.o = rays_o; R.d = rays_d; R.nears = nears; R.fars = fars;
    return march_train_impl(R, false, N, bitfield, bound, cascade, grid_size, max_steps, dt_gamma, noises, noise_seed,
                            noise_counter, capacity, xyzs, dirs, deltas, rays, counter, stream);
}

// The ray source of the forms that clip inside the march passes, checked in the name of entry point `who`: the box and
// -- `cam`, B views -- the camera of the forms whose count pass generates the rays into cam->ro / cam->rd (`bad_camera`:
// how that form words a bad camera; intr_in_memory: it reads its intrinsics from cam->intr).
static int march_source(const char *who, MarchRays &R, float xmin, float ymin, float zmin, float xmax, float ymax,
                        float zmax, float min_near, const RayGen *cam = nullptr, int B = 0,
                        const char *bad_camera = nullptr, bool intr_in_memory = false) {
    LNERF_REQUIRE(!cam || (B >= 0 && cam->H >= 1 && cam->W >= 1 && cam->fx != 0.f && cam->fy != 0.f), "%s: %s", who,
                  bad_camera);
    LNERF_REQUIRE(xmin <= xmax && ymin <= ymax && zmin <= zmax, "%s: inverted aabb", who);
    LNERF_REQUIRE(!cam || B == 0 || (cam->c2w && (cam->intr || !intr_in_memory) && cam->ro && cam->rd),
                  "%s: null pointer", who);
    R.nears = R.fars = nullptr;
    R.box = RayBox{xmin, ymin, zmin, xmax, ymax, zmax, min_near};
    if (cam) { R.gen = *cam; R.o = cam->ro; R.d = cam->rd; }
    return LNERF_OK;
}

int lnerf_march_rays_train_aabb(const float *rays_o, const float *rays_d, float xmin, float ymin, float zmin, float xmax,
                                float ymax, float zmax, float min_near, int64_t N, const uint8_t *bitfield, float bound,
                                int cascade, int grid_size, int max_steps, float dt_gamma, const float *noises,
                                uint32_t noise_seed, int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs,
                                float *deltas, int32_t *rays, int32_t *counter, lnerf_stream_t stream) {
    MarchRays R{};
    R.o = rays_o; R.d = rays_d;
    int rc = march_source("march_rays_train_aabb", R, xmin, ymin, zmin, xmax, ymax, zmax, min_near);
    if (rc) return rc;
    return march_train_impl(R, true, N, bitfield, bound, cascade, grid_size, max_steps, dt_gamma, noises, noise_seed,
                            noise_counter, capacity, xyzs, dirs, deltas, rays, counter, stream);
}

int lnerf_march_rays_train_pose(const float *c2w, int B, int H, int W, float fx, float fy, float cx, float cy,
                                float *rays_o_out, float *rays_d_out, float xmin, float ymin, float zmin, float xmax,
                                float ymax, float zmax, float min_near, const uint8_t *bitfield, float bound, int cascade,
                                int grid_size, int max_steps, float dt_gamma, const float *noises, uint32_t noise_seed,
                                int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs, float *deltas,
                                int32_t *rays, int32_t *counter, lnerf_stream_t stream) {
    const RayGen cam{c2w, nullptr, 1, H, W, fx, fy, cx, cy, rays_o_out, rays_d_out};
    MarchRays R{};
    int rc = march_source("march_rays_train_pose", R, xmin, ymin, zmin, xmax, ymax, zmax, min_near, &cam, B, "bad camera");
    if (rc) return rc;
    return march_train_impl(R, true, (int64_t)B * H * W, bitfield, bound, cascade, grid_size, max_steps, dt_gamma, noises,
                            noise_seed, noise_counter, capacity, xyzs, dirs, deltas, rays, counter, stream);
}

int lnerf_march_rays_train_camera(const float *c2w, const float *intrinsics, int B, int H, int W, float *rays_o_out,
                                  float *rays_d_out, float xmin, float ymin, float zmin, float xmax, float ymax,
                                  float zmax, float min_near, const uint8_t *bitfield, float bound, int cascade,
                                  int grid_size, int max_steps, float dt_gamma, const float *noises, uint32_t noise_seed,
                                  int32_t *noise_counter, int64_t capacity, float *xyzs, float *dirs, float *deltas,
                                  int32_t *rays, int32_t *counter, lnerf_stream_t stream) {
    const RayGen cam{c2w, intrinsics, 1, H, W, 1.f, 1.f, 0.f, 0.f, rays_o_out, rays_d_out};   // (by-value ones: unused)
    MarchRays R{};
    int rc = march_source("march_rays_train_camera", R, xmin, ymin, zmin, xmax, ymax, zmax, min_near, &cam, B,
                          "bad image size", true);
    if (rc) return rc;
    return march_train_impl(R, true, (int64_t)B * H * W, bitfield, bound, cascade, grid_size, max_steps, dt_gamma, noises,
                            noise_seed, noise_counter, capacity, xyzs, dirs, deltas, rays, counter, stream);
}

int lnerf_march_rays(int64_t n_alive, int n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                     const float *rays_d, const float *fars, const uint8_t *bitfield, float bound, int cascade,
                     int grid_size, int max_steps, float dt_gamma, float *xyzs, float *dirs, float *deltas,
                     lnerf_stream_t stream) {
    int rc = check_march_common("march_rays", bound, cascade, grid_size, max_steps, dt_gamma);
    if (rc) return rc;
    LNERF_REQUIRE(n_alive >= 0 && n_step >= 1, "march_rays: bad n_alive/n_step");
    if (n_alive == 0) return LNERF_OK;
    LNERF_REQUIRE(rays_alive && rays_t && rays_o && rays_d && fars && bitfield && xyzs && dirs && deltas,
                  "march_rays: null pointer");
    const MarchParams P = make_params(bound, cascade, grid_size, max_steps, dt_gamma);
    hipLaunchKernelGGL(k_march_rays, dim3((unsigned)div_up(n_alive, 256)), dim3(256), 0, as_stream(stream), n_alive,
                       n_step, rays_alive, rays_t, rays_o, rays_d, fars, bitfield, P, xyzs, dirs, deltas);
    LNERF_CHECK_LAUNCH("march_rays");
    return LNERF_OK;
}

int lnerf_composite_rays(int64_t n_alive, int n_step, int32_t *rays_alive, float *rays_t, const float *sigmas,
                         const float *rgbs, const float *deltas, int C, float T_thresh, float *weights_sum,
                         float *depth, float *image, float *transmittance, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_alive >= 0 && n_step >= 1, "composite_rays: bad n_alive/n_step");
    LNERF_REQUIRE(C >= 1 && C <= 4, "composite_rays: C must be in [1,4] (got %d)", C);
    if (n_alive == 0) return LNERF_OK;
    LNERF_REQUIRE(rays_alive && rays_t && sigmas && rgbs && deltas && weights_sum && depth && image && transmittance,
                  "composite_rays: null pointer");
    hipLaunchKernelGGL(k_composite_rays, dim3((unsigned)div_up(n_alive, 256)), dim3(256), 0, as_stream(stream), n_alive,
                       n_step, rays_alive, rays_t, sigmas, rgbs, deltas, C, T_thresh, weights_sum, depth, image,
                       transmittance);
    LNERF_CHECK_LAUNCH("composite_rays");
    return LNERF_OK;
}

int lnerf_compact_rays(const int32_t *alive_in, int64_t n, int32_t *alive_out, int32_t *n_alive_dev,
                       lnerf_stream_t stream) {
    LNERF_REQUIRE(n >= 0, "compact_rays: negative n");
    LNERF_REQUIRE(n_alive_dev, "compact_rays: null n_alive_dev");
    LNERF_REQUIRE(n == 0 || (alive_in && alive_out), "compact_rays: null pointer");
    LNERF_REQUIRE(alive_in != alive_out || n == 0, "compact_rays: in-place compaction is not supported");
    hipLaunchKernelGGL(k_compact_rays, dim3(1), dim3(1024), 0, as_stream(stream), alive_in, n, alive_out, n_alive_dev);
    LNERF_CHECK_LAUNCH("compact_rays");
    return LNERF_OK;
}

}  // extern "C"
