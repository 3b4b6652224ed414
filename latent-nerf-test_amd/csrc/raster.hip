// Latent-Paint raster path (BASELINE config 5): the kaolin ops the
// reference calls in src/latent_paint/models/render.py:34-69 (prepare_vertices :39-40,56-57, rasterize
// :42-43,59-60, texture_mapping :64), rebuilt as HIP kernels.  kaolin itself is not available (un-pinned git
// HEAD, setup.sh:3), so the semantics are the documented ones restated in oracle/raster_oracle.py:
// hard z-buffer (largest camera-space z = closest), perspective-correct barycentric interpolation of
// per-face-vertex attributes, face_idx = -1 on background, texture lookup = grid_sample(align_corners=False,
// padding 'border') on (u, 1 - v).
#include "common.h"
#include "raster_shared.h"
#include "tex_shared.h"

namespace lnerf {

// cam_project (raster_shared.h) of the three corners of face f, written to slot `at` of face_z / face_xy and returned
__device__ __forceinline__ void prepare_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, int f,
                                             const Cam &cam, int64_t at, float *__restrict__ face_z,
                                             float *__restrict__ face_xy, float x[3], float y[3], float z[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *v = verts + faces[f * 3 + k] * 3;
        const CamPoint c = cam_project(cam.rec, v[0], v[1], v[2]);
        face_z[at * 3 + k] = z[k] = c.z;
        face_xy[(at * 3 + k) * 2] = x[k] = c.x;
        face_xy[(at * 3 + k) * 2 + 1] = y[k] = c.y;
    }
}

__global__ void __launch_bounds__(256)
k_raster_prepare(const float *__restrict__ verts, const int32_t *__restrict__ faces, int F, Cam cam,
                 float *__restrict__ face_z, float *__restrict__ face_xy) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float x[3], y[3], z[3];
    prepare_face(verts, faces, f, cam, f, face_z, face_xy, x, y, z);
}

// The pixel box of a face (the rule is stated in include/lnerf_hip.h): inclusive (j_lo, j_hi, i_lo, i_hi), padded by one
// pixel and clipped to the image; (0, -1, 0, -1) when the face can win no pixel.  f32, no fused multiply-adds.
struct alignas(8) Box { int16_t j_lo, j_hi, i_lo, i_hi; };

__device__ __forceinline__ Box face_box(const float x[3], const float y[3], const float z[3], int H, int W) {
    const Box empty = {0, -1, 0, -1};
    if (!(z[0] < 0.f && z[1] < 0.f && z[2] < 0.f)) return empty;   // k_rasterize rejects it: behind the camera
    if (face_area(x[0], y[0], x[1], y[1], x[2], y[2]) == 0.f) return empty;   // ... or degenerate
    const float big = 3.4028234664e38f;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) finite = finite && fabsf(x[k]) <= big && fabsf(y[k]) <= big;
    if (!finite) return Box{0, (int16_t)(W - 1), 0, (int16_t)(H - 1)};
    const float xmin = fminf(fminf(x[0], x[1]), x[2]), xmax = fmaxf(fmaxf(x[0], x[1]), x[2]);
    const float ymin = fminf(fminf(y[0], y[1]), y[2]), ymax = fmaxf(fmaxf(y[0], y[1]), y[2]);
    const float Wf = (float)W, Hf = (float)H;
    const float j_lo = fmaxf(floorf(ndc_to_col(xmin, Wf)) - 1.0f, 0.0f);
    const float j_hi = fminf(ceilf(ndc_to_col(xmax, Wf)) + 1.0f, Wf - 1.0f);
    const float i_lo = fmaxf(floorf(ndc_to_row(ymax, Hf)) - 1.0f, 0.0f);
    const float i_hi = fminf(ceilf(ndc_to_row(ymin, Hf)) + 1.0f, Hf - 1.0f);
    if (j_lo > j_hi || i_lo > i_hi) return empty;                   // wholly off the image
    return Box{(int16_t)j_lo, (int16_t)j_hi, (int16_t)i_lo, (int16_t)i_hi};
}

// B views of one mesh: blockIdx.y = view; the cameras are read from device memory
__global__ void __launch_bounds__(256)
k_raster_prepare_batch(const float *__restrict__ verts, const int32_t *__restrict__ faces, int F,
                       const float *__restrict__ cams, int H, int W, float *__restrict__ face_z,
                       float *__restrict__ face_xy, Box *__restrict__ boxes) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int b = blockIdx.y;
    const int64_t bf = (int64_t)b * F + f;
    float x[3], y[3], z[3];
    prepare_face(verts, faces, f, cam_read(cams + b * CAM_FLOATS), bf, face_z, face_xy, x, y, z);
    boxes[bf] = face_box(x, y, z, H, W);
}

constexpr int RTILE = 128;  // faces per LDS tile

// What one pixel does with one face, shared by both rasterisers: inside test, perspective-correct weights and depth (the
// two stages of raster_shared.h), and the z-buffer update (strictly closer wins, so of equal depths the lower index stays).
__device__ __forceinline__ void raster_face_test(float px, float py, float x0, float y0, float x1, float y1, float x2,
                                                 float y2, float z0, float z1, float z2, int f, float &best_z,
                                                 int &best_f, float &bw0, float &bw1, float &bw2) {
    if (!(z0 < 0.f && z1 < 0.f && z2 < 0.f)) return;  // behind the camera
    const float area = face_area(x0, y0, x1, y1, x2, y2);
    if (area == 0.f) return;
    const FaceW w = face_weights(area, px, py, x0, y0, x1, y1, x2, y2);
    if (w.w0 < 0.f || w.w1 < 0.f || w.w2 < 0.f) return;
    const FaceP p = face_perspective(w, z0, z1, z2);   // only inside the face
    if (p.z > best_z) {          // strictly closer; ties keep the lower face index
        best_z = p.z;
        best_f = f;
        bw0 = p.b0; bw1 = p.b1; bw2 = p.b2;
    }
}

// one thread per pixel; faces stream through LDS
__global__ void __launch_bounds__(256)
k_rasterize(int H, int W, const float *__restrict__ face_z, const float *__restrict__ face_xy, int F,
            int32_t *__restrict__ face_idx, float *__restrict__ bary) {
    __shared__ float s_xy[RTILE * 6];
    __shared__ float s_z[RTILE * 3];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool in = p < H * W;
    const int i = in ? p / W : 0, j = in ? p - i * W : 0;
    const Ndc c = pixel_centre(i, j, H, W);
    float best_z = -3.0e38f;
    int best_f = -1;
    float bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
    for (int f0 = 0; f0 < F; f0 += RTILE) {
        const int nf = min(RTILE, F - f0);
        __syncthreads();
        for (int k = threadIdx.x; k < nf * 6; k += 256) s_xy[k] = face_xy[(int64_t)f0 * 6 + k];
        for (int k = threadIdx.x; k < nf * 3; k += 256) s_z[k] = face_z[(int64_t)f0 * 3 + k];
        __syncthreads();
        for (int f = 0; f < nf; ++f)
            raster_face_test(c.x, c.y, s_xy[f * 6], s_xy[f * 6 + 1], s_xy[f * 6 + 2], s_xy[f * 6 + 3], s_xy[f * 6 + 4],
                             s_xy[f * 6 + 5], s_z[f * 3], s_z[f * 3 + 1], s_z[f * 3 + 2], f0 + f, best_z, best_f, bw0,
                             bw1, bw2);
    }
    if (in) {
        face_idx[p] = best_f;
        bary[p * 3] = bw0; bary[p * 3 + 1] = bw1; bary[p * 3 + 2] = bw2;
    }
}

// Tile-culled rasteriser for B views: one workgroup of NW waves per (view, TS x TS pixel tile).  The workgroup walks the
// view's faces in ascending order, 64 * NW at a time: each lane compares one face's box with the tile rectangle (8 bytes
// per face, consecutive lanes read consecutive boxes), the survivors are compacted in ascending order into an LDS queue
// of face records, and when the queue cannot take another round -- and once more at the end -- the pixels drain it with
// raster_face_test.  The tile is G = TS * TS / 64 groups of 64 pixels, and S = NW / G waves share a group: wave slice s
// takes the queue entries s, s + S, ... in ascending order, so each holds the lowest index among its own closest faces,
// and the closing merge takes the closest of the S candidates, the lower face index on an exact tie: the result of one
// ascending scan with k_rasterize's strict comparison.  No global lists, no atomics.
struct alignas(16) QFace { float x0, y0, x1, y1, x2, y2, z0, z1, z2; int f; int pad[2]; };

template <int TS, int NW>
__global__ void __launch_bounds__(64 * NW)
k_rasterize_tiles(int H, int W, const float *__restrict__ face_z, const float *__restrict__ face_xy,
                  const Box *__restrict__ boxes, int F, int32_t *__restrict__ face_idx, float *__restrict__ bary) {
    constexpr int NT = 64 * NW, G = TS * TS / 64, S = NW / G, Q = 2 * NT;
    static_assert(TS * TS % 64 == 0 && NW % G == 0, "whole waves per pixel group");
    static_assert(Q * sizeof(QFace) >= NT * 5 * sizeof(float), "the merge reuses the queue's memory");
    __shared__ QFace s_q[Q];
    __shared__ int s_cnt[2][NW];
    const int t = threadIdx.x, wave = t >> 6;
    const int slice = wave / G, pl = (wave % G) * 64 + (t & 63);   // this thread's queue slice and pixel of the tile
    const int b = blockIdx.z;
    const int tj0 = blockIdx.x * TS, ti0 = blockIdx.y * TS;
    const int j = tj0 + pl % TS, i = ti0 + pl / TS;
    const bool in = i < H && j < W;
    const Ndc c = pixel_centre(i, j, H, W);
    face_z += (int64_t)b * F * 3;
    face_xy += (int64_t)b * F * 6;
    boxes += (int64_t)b * F;
    float best_z = -3.0e38f;
    int best_f = -1;
    float bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
    int qn = 0;   // queue length: the same value in every thread

    auto drain = [&]() {
        __syncthreads();
        for (int q = slice; q < qn; q += S) {
            const QFace r = s_q[q];   // every lane of the wave reads the same record: a broadcast
            raster_face_test(c.x, c.y, r.x0, r.y0, r.x1, r.y1, r.x2, r.y2, r.z0, r.z1, r.z2, r.f, best_z, best_f, bw0,
                             bw1, bw2);
        }
        __syncthreads();
        qn = 0;
    };

    const Box none = {0, -1, 0, -1};
    Box next = t < F ? boxes[t] : none;
    int parity = 0;
    for (int f0 = 0; f0 < F; f0 += NT, parity ^= 1) {
        const Box box = next;
        const int f = f0 + t, fn = f + NT;
        next = fn < F ? boxes[fn] : none;   // in flight while this round is compacted
        if (qn + NT > Q) drain();
        const bool hit = box.j_lo <= tj0 + TS - 1 && box.j_hi >= tj0 && box.i_lo <= ti0 + TS - 1 && box.i_hi >= ti0;
        const unsigned long long m = __ballot(hit);
        int at = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        int total = __popcll(m);
        if (NW > 1) {
            if ((t & 63) == 0) s_cnt[parity][wave] = total;
            __syncthreads();
            total = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int c = s_cnt[parity][w];
                if (w < wave) at += c;
                total += c;
            }
        }
        if (hit) {
            const float *xy = face_xy + (int64_t)f * 6, *z = face_z + (int64_t)f * 3;
            QFace r;
            r.x0 = xy[0]; r.y0 = xy[1]; r.x1 = xy[2]; r.y1 = xy[3]; r.x2 = xy[4]; r.y2 = xy[5];
            r.z0 = z[0]; r.z1 = z[1]; r.z2 = z[2];
            r.f = f; r.pad[0] = 0; r.pad[1] = 0;
            s_q[at] = r;
        }
        qn += total;
    }
    drain();
    if (S > 1) {   // the slices' candidates of a pixel -> slice 0 (the drain ended with a barrier: the queue is free)
        float *mz = reinterpret_cast<float *>(s_q);
        int *mf = reinterpret_cast<int *>(mz + NT);
        float *mw = mz + 2 * NT;
        const int slot = slice * (64 * G) + pl;
        mz[slot] = best_z; mf[slot] = best_f;
        mw[slot] = bw0; mw[NT + slot] = bw1; mw[2 * NT + slot] = bw2;
        __syncthreads();
        if (slice != 0) return;
        for (int s2 = 1; s2 < S; ++s2) {
            const int o = s2 * (64 * G) + pl;
            const float z2 = mz[o];
            const int f2 = mf[o];
            if (z2 > best_z || (z2 == best_z && f2 < best_f)) {
                best_z = z2; best_f = f2;
                bw0 = mw[o]; bw1 = mw[NT + o]; bw2 = mw[2 * NT + o];
            }
        }
    }
    if (in) {
        const int64_t p = ((int64_t)b * H + i) * W + j;
        face_idx[p] = best_f;
        bary[p * 3] = bw0; bary[p * 3 + 1] = bw1; bary[p * 3 + 2] = bw2;
    }
}

// Two shapes of the kernel, chosen from the launch's size alone (measured: DESIGN.md, "Batched views on a tile-culled
// rasteriser").  Up to RASTER_SMALL_MAX_TILES 8 x 8 tiles over all views there are fewer tiles than the chip has room
// for: 8 x 8 tiles of 16 waves (each wave a sixteenth of the queue) put the most waves on every face walk and drain.
// Beyond that the tiles alone fill the chip and the box walk dominates: 16 x 16 tiles of 4 waves walk a quarter of the
// boxes per pixel.
constexpr int RASTER_SMALL_MAX_TILES = 2048;

// feat[p, :] = sum_k bary[p,k] * attr[face_idx[p], k, :]   (0 on background)
__global__ void __launch_bounds__(256)
k_interp_attr(const int32_t *__restrict__ face_idx, const float *__restrict__ bary, const float *__restrict__ attr,
              int P, int D, float *__restrict__ feat) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * D) return;
    const int p = t / D, d = t - p * D;
    const int f = face_idx[p];
    float v = 0.f;
    if (f >= 0) {
        const float *a = attr + (int64_t)f * 3 * D;
        v = fmaf(bary[p * 3], a[d], fmaf(bary[p * 3 + 1], a[D + d], bary[p * 3 + 2] * a[2 * D + d]));
    }
    feat[t] = v;
}
__global__ void __launch_bounds__(256)
k_interp_attr_bwd(const int32_t *__restrict__ face_idx, const float *__restrict__ bary,
                  const float *__restrict__ dfeat, int P, int D, float *__restrict__ dattr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * D) return;
    const int p = t / D, d = t - p * D;
    const int f = face_idx[p];
    if (f < 0) return;
    const float g = dfeat[t];
    float *a = dattr + (int64_t)f * 3 * D;
    atomicAdd(&a[d], bary[p * 3] * g);
    atomicAdd(&a[D + d], bary[p * 3 + 1] * g);
    atomicAdd(&a[2 * D + d], bary[p * 3 + 2] * g);
}

// texture lookup: tex [C,R,R]; uv [P,2]; mode 0 nearest, 1 bilinear, 2 bicubic, at the texel coordinates of tex_coords
// (tex_shared.h)
// cubic convolution weights of the 4 taps around a position with fractional part t (A = -0.75, as grid_sample)
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
    const float A = -0.75f;
    const float a = t + 1.0f, b = 1.0f - t, c = b + 1.0f;
    w[0] = ((A * a - 5.0f * A) * a + 8.0f * A) * a - 4.0f * A;
    w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    w[2] = ((A + 2.0f) * b - (A + 3.0f)) * b * b + 1.0f;
    w[3] = ((A * c - 5.0f * A) * c + 8.0f * A) * c - 4.0f * A;
}
template <bool BWD>
__global__ void __launch_bounds__(256)
k_texture_map(const float *__restrict__ uv, const int32_t *__restrict__ face_idx, float *tex, int P, int C, int R,
              int mode, float *out_or_dout) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * C) return;
    const int p = t / C, c = t - p * C;
    const bool fg = !face_idx || face_idx[p] >= 0;
    if (!fg) {
        if (!BWD) out_or_dout[t] = 0.f;
        return;
    }
    float x, y;
    tex_coords(uv[p * 2], uv[p * 2 + 1], R, mode != 2, x, y);
    float *tc = tex + (int64_t)c * R * R;
    if (mode == 0) {
        const int xi = (int)rintf(x), yi = (int)rintf(y);
        if (BWD) atomicAdd(&tc[yi * R + xi], out_or_dout[t]);
        else out_or_dout[t] = tc[yi * R + xi];
    } else if (mode == 1) {
        const BilTaps b = bil_taps(uv[p * 2], uv[p * 2 + 1], R);   // the taps the mip-mapped lookup reads per level
        if (BWD) bil_add(tc, b, out_or_dout[t]);
        else out_or_dout[t] = bil_read(tc, b);
    } else {
        const float xf = floorf(x), yf = floorf(y);
        const int xb = (int)xf - 1, yb = (int)yf - 1;
        float wx[4], wy[4];
        cubic_weights(x - xf, wx);
        cubic_weights(y - yf, wy);
        if (BWD) {
            const float g = out_or_dout[t];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int yi = min(max(yb + i, 0), R - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) atomicAdd(&tc[yi * R + min(max(xb + j, 0), R - 1)], (wy[i] * wx[j]) * g);
            }
        } else {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int yi = min(max(yb + i, 0), R - 1);
                float row = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) row = fmaf(wx[j], tc[yi * R + min(max(xb + j, 0), R - 1)], row);
                acc = fmaf(wy[i], row, acc);
            }
            out_or_dout[t] = acc;
        }
    }
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_raster_prepare(const float *verts, int n_verts, const int32_t *faces, int n_faces, const float *cam_host,
                         float *face_z, float *face_xy, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_verts > 0 && n_faces > 0, "raster_prepare: empty mesh");
    LNERF_REQUIRE(verts && faces && cam_host && face_z && face_xy, "raster_prepare: null pointer");
    LNERF_LAUNCH(k_raster_prepare, n_faces, 256, as_stream(stream), verts, faces, n_faces, cam_read(cam_host), face_z,
                 face_xy);
    LNERF_CHECK_LAUNCH("raster_prepare");
    return LNERF_OK;
}

int lnerf_rasterize(int H, int W, const float *face_z, const float *face_xy, int n_faces, int32_t *face_idx,
                    float *bary, lnerf_stream_t stream) {
    LNERF_REQUIRE(H > 0 && W > 0 && n_faces > 0, "rasterize: bad sizes");
    LNERF_REQUIRE(face_z && face_xy && face_idx && bary, "rasterize: null pointer");
    LNERF_LAUNCH(k_rasterize, (int64_t)H * W, 256, as_stream(stream), H, W, face_z, face_xy, n_faces, face_idx, bary);
    LNERF_CHECK_LAUNCH("rasterize");
    return LNERF_OK;
}

int lnerf_raster_prepare_batch(const float *verts, int n_verts, const int32_t *faces, int n_faces,
                               const float *cams_dev, int B, int H, int W, float *face_z, float *face_xy,
                               int16_t *face_box, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_verts > 0 && n_faces > 0, "raster_prepare_batch: empty mesh");
    if (int e = check_view_dims("raster_prepare_batch", B, H, W)) return e;
    LNERF_REQUIRE(verts && faces && cams_dev && face_z && face_xy && face_box, "raster_prepare_batch: null pointer");
    hipLaunchKernelGGL(k_raster_prepare_batch, dim3((unsigned)div_up(n_faces, 256), (unsigned)B), dim3(256), 0,
                       as_stream(stream), verts, faces, n_faces, cams_dev, H, W, face_z, face_xy,
                       reinterpret_cast<Box *>(face_box));
    LNERF_CHECK_LAUNCH("raster_prepare_batch");
    return LNERF_OK;
}

int lnerf_rasterize_batch(int B, int H, int W, const float *face_z, const float *face_xy, const int16_t *face_box,
                          int n_faces, int32_t *face_idx, float *bary, lnerf_stream_t stream) {
    if (int e = check_view_dims("rasterize_batch", B, H, W)) return e;
    LNERF_REQUIRE(n_faces > 0, "rasterize_batch: no faces");
    LNERF_REQUIRE(face_z && face_xy && face_box && face_idx && bary, "rasterize_batch: null pointer");
    LNERF_REQUIRE(((uintptr_t)face_box & 7) == 0, "rasterize_batch: face_box must be 8-byte aligned");
    const Box *boxes = reinterpret_cast<const Box *>(face_box);
    if ((int64_t)B * div_up(W, 8) * div_up(H, 8) <= RASTER_SMALL_MAX_TILES) {
        hipLaunchKernelGGL((k_rasterize_tiles<8, 16>), dim3((unsigned)div_up(W, 8), (unsigned)div_up(H, 8), (unsigned)B),
                           dim3(1024), 0, as_stream(stream), H, W, face_z, face_xy, boxes, n_faces, face_idx, bary);
    } else {
        hipLaunchKernelGGL((k_rasterize_tiles<16, 4>),
                           dim3((unsigned)div_up(W, 16), (unsigned)div_up(H, 16), (unsigned)B), dim3(256), 0,
                           as_stream(stream), H, W, face_z, face_xy, boxes, n_faces, face_idx, bary);
    }
    LNERF_CHECK_LAUNCH("rasterize_batch");
    return LNERF_OK;
}

int lnerf_interpolate_attributes(const int32_t *face_idx, const float *bary, const float *attr, int n_pixels, int D,
                                 float *feat, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && D >= 1 && D <= 16, "interpolate_attributes: bad sizes");
    LNERF_REQUIRE(face_idx && bary && attr && feat, "interpolate_attributes: null pointer");
    LNERF_LAUNCH(k_interp_attr, (int64_t)n_pixels * D, 256, as_stream(stream), face_idx, bary, attr, n_pixels, D, feat);
    LNERF_CHECK_LAUNCH("interpolate_attributes");
    return LNERF_OK;
}

int lnerf_interpolate_attributes_backward(const int32_t *face_idx, const float *bary, const float *dfeat,
                                          int n_pixels, int D, float *dattr, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && D >= 1 && D <= 16, "interpolate_attributes_backward: bad sizes");
    LNERF_REQUIRE(face_idx && bary && dfeat && dattr, "interpolate_attributes_backward: null pointer");
    LNERF_LAUNCH(k_interp_attr_bwd, (int64_t)n_pixels * D, 256, as_stream(stream), face_idx, bary, dfeat, n_pixels, D,
                 dattr);
    LNERF_CHECK_LAUNCH("interpolate_attributes_backward");
    return LNERF_OK;
}

int lnerf_texture_map_forward(const float *uv, const int32_t *face_idx, const float *texture, int n_pixels, int C,
                              int R, int mode, float *out, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && C >= 1 && R >= 1 && mode >= 0 && mode <= 2, "texture_map_forward: bad arguments");
    LNERF_REQUIRE(uv && texture && out, "texture_map_forward: null pointer");
    LNERF_LAUNCH(k_texture_map<false>, (int64_t)n_pixels * C, 256, as_stream(stream), uv, face_idx,
                 const_cast<float *>(texture), n_pixels, C, R, mode, out);
    LNERF_CHECK_LAUNCH("texture_map_forward");
    return LNERF_OK;
}

int lnerf_texture_map_backward(const float *uv, const int32_t *face_idx, const float *dout, int n_pixels, int C, int R,
                               int mode, float *dtexture, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && C >= 1 && R >= 1 && mode >= 0 && mode <= 2, "texture_map_backward: bad arguments");
    LNERF_REQUIRE(uv && dout && dtexture, "texture_map_backward: null pointer");
    LNERF_LAUNCH(k_texture_map<true>, (int64_t)n_pixels * C, 256, as_stream(stream), uv, face_idx, dtexture, n_pixels, C,
                 R, mode, const_cast<float *>(dout));
    LNERF_CHECK_LAUNCH("texture_map_backward");
    return LNERF_OK;
}

}  // extern "C"
