// The geometry half of the Latent-Paint backward pass ("Vertex gradients and edge antialiasing"): gradients of
// a rendered batch with respect to the projected faces and, through the projection, the vertices; the edge-antialiasing
// pass that makes a silhouette differentiable under an image loss; and the face-weighted uniform Laplacian of the
// displacement regulariser.  Everything here differentiates a forward of raster.hip / tex_shared.h and calls that forward's
// functions (raster_shared.h, tex_shared.h) for its terms; contracts: include/lnerf_hip.h.  f32, each operation rounded alone.
#include "common.h"
#include "raster_shared.h"
#include "tex_shared.h"

namespace lnerf {

// ------------------------------------------------------------------------------------------------ edge antialiasing
// What a pixel knows about itself: its face (-1 = background), its depth and its centre.
struct AAPixel {
    int f;
    float d, x, y;
};

__device__ __forceinline__ AAPixel aa_pixel(const int32_t *__restrict__ face_idx, const float *__restrict__ bary,
                                            const float *__restrict__ face_z, int b, int i, int j, int H, int W, int F) {
    const int64_t p = ((int64_t)b * H + i) * W + j;
    AAPixel r;
    const Ndc c = pixel_centre(i, j, H, W);
    r.x = c.x; r.y = c.y;
    const int f = face_idx[p];
    if (f < 0 || f >= F) {
        r.f = -1;
        r.d = -INFINITY;
        return r;
    }
    const float *z = face_z + ((int64_t)b * F + f) * 3;
    r.f = f;
    r.d = (bary[p * 3] * z[0] + bary[p * 3 + 1] * z[1]) + bary[p * 3 + 2] * z[2];
    return r;
}

// One evaluated pair: rules 1-3 of lnerf_raster_antialias_forward.  `a` and `b` are the two pixels in either order: the
// result is stated for near / far, so both pixels of a pair compute the same thing.  xy = this view's face_xy.
struct AAPair {
    bool ok;
    bool a_near;   // the near pixel is `a`
    int T, ka, kb; // near's face and the corners of the taken edge
    float t;
};

__device__ __forceinline__ AAPair aa_pair(const AAPixel &a, const AAPixel &b, bool horizontal,
                                          const float *__restrict__ xy, const int32_t *__restrict__ faces) {
    AAPair r;
    r.ok = false;
    r.a_near = a.d > b.d;
    r.T = -1; r.ka = 0; r.kb = 0; r.t = 0.f;
    if (a.f == b.f || a.d == b.d || !(a.d > b.d || b.d > a.d)) return r;   // (a NaN depth decides nothing)
    const int T = r.a_near ? a.f : b.f, far_f = r.a_near ? b.f : a.f;   // T >= 0: its depth is above -inf
    const float *c = xy + (int64_t)T * 6;
    // horizontal: the line y = line (both pixels share it); along = x.  vertical: the same with x and y exchanged.
    const float line = horizontal ? a.y : a.x;
    const float s_a = horizontal ? a.x : a.y, s_b = horizontal ? b.x : b.y;
    const float s_near = r.a_near ? s_a : s_b, s_far = r.a_near ? s_b : s_a;
    const int o_al = horizontal ? 0 : 1, o_ac = horizontal ? 1 : 0;
    int e = -1;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k2 = k == 2 ? 0 : k + 1;
        const float xa = c[k * 2 + o_al], ya = c[k * 2 + o_ac], xb = c[k2 * 2 + o_al], yb = c[k2 * 2 + o_ac];
        if ((ya > line) == (yb > line)) continue;
        const float xs = xa + (line - ya) * (xb - xa) / (yb - ya);
        const float tk = (xs - s_near) / (s_far - s_near);
        if (e < 0 && tk >= 0.f && tk <= 1.f) {
            e = k;
            t = tk;
        }
    }
    if (e < 0) return r;
    const int ka = e, kb = e == 2 ? 0 : e + 1;
    if (far_f >= 0) {   // an interior edge between mesh neighbours is no discontinuity
        const int va = faces[T * 3 + ka], vb = faces[T * 3 + kb];
        const int g0 = faces[far_f * 3], g1 = faces[far_f * 3 + 1], g2 = faces[far_f * 3 + 2];
        if ((va == g0 || va == g1 || va == g2) && (vb == g0 || vb == g1 || vb == g2)) return r;
    }
    r.ok = true;
    r.T = T; r.ka = ka; r.kb = kb; r.t = t;
    return r;
}

// the weight with which `a` receives (c_b - c_a) from the pair, and its derivative by t
__device__ __forceinline__ float aa_weight(const AAPair &r, bool for_a, float &dw_dt) {
    dw_dt = 0.f;
    if (!r.ok) return 0.f;
    const bool near = r.a_near == for_a;
    if (near && r.t < 0.5f) { dw_dt = -1.f; return 0.5f - r.t; }
    if (!near && !(r.t < 0.5f)) { dw_dt = 1.f; return r.t - 0.5f; }
    return 0.f;
}

// the neighbours of (i, j) in the fixed order left, right, up, down; false outside the image
__device__ __forceinline__ bool aa_neighbour(int n, int i, int j, int H, int W, int &ni, int &nj) {
    ni = i + (n == 2 ? -1 : n == 3 ? 1 : 0);
    nj = j + (n == 0 ? -1 : n == 1 ? 1 : 0);
    return ni >= 0 && ni < H && nj >= 0 && nj < W;
}

// one thread per pixel.  BWD: grad_image in gather form (one writer per element) and the atomics into grad_face_xy of
// the pairs this pixel RECEIVES from (every pair has at most one receiver, so each is counted once).
template <bool BWD>
__global__ void __launch_bounds__(256)
k_raster_antialias(const float *__restrict__ image, const float *__restrict__ gout, const int32_t *__restrict__ face_idx,
                   const float *__restrict__ bary, const float *__restrict__ face_xy, const float *__restrict__ face_z,
                   const int32_t *__restrict__ faces, int B, int H, int W, int C, int F, float *__restrict__ out,
                   float *__restrict__ gxy) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)B * H * W) return;
    const auto [b, i, j] = pixel_of(p, H, W);
    const float *xy = face_xy + (int64_t)b * F * 6;
    const AAPixel me = aa_pixel(face_idx, bary, face_z, b, i, j, H, W, F);
    float w_in[4], w_out[4], dw[4];   // what this pixel receives per neighbour, and what the neighbour receives from it
    int64_t q[4];
    AAPair pr[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        int ni, nj;
        w_in[n] = 0.f; w_out[n] = 0.f; dw[n] = 0.f; q[n] = -1; pr[n].ok = false;
        if (!aa_neighbour(n, i, j, H, W, ni, nj)) continue;
        q[n] = ((int64_t)b * H + ni) * W + nj;
        const AAPixel nb = aa_pixel(face_idx, bary, face_z, b, ni, nj, H, W, F);
        pr[n] = aa_pair(me, nb, n < 2, xy, faces);
        float unused;
        w_in[n] = aa_weight(pr[n], true, dw[n]);
        if (BWD) w_out[n] = aa_weight(pr[n], false, unused);
    }
    if (!BWD) {
        for (int c = 0; c < C; ++c) {
            const float mine = image[p * C + c];
            float acc = mine;
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (w_in[n] != 0.f) acc += w_in[n] * (image[q[n] * C + c] - mine);
            out[p * C + c] = acc;
        }
        return;
    }
    float dt[4] = {0.f, 0.f, 0.f, 0.f};   // dL/dt of the pairs this pixel receives from
    for (int c = 0; c < C; ++c) {
        const float g = gout[p * C + c], mine = image[p * C + c];
        float acc = g;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (q[n] < 0) continue;
            if (w_in[n] != 0.f) acc -= w_in[n] * g;
            if (w_out[n] != 0.f) acc += w_out[n] * gout[q[n] * C + c];
            if (dw[n] != 0.f) dt[n] += dw[n] * (g * (image[q[n] * C + c] - mine));
        }
        out[p * C + c] = acc;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (dw[n] == 0.f || dt[n] == 0.f) continue;
        const AAPair &r = pr[n];
        int ni, nj;
        aa_neighbour(n, i, j, H, W, ni, nj);
        const bool horizontal = n < 2;
        // the centres of near and far along the pair's axis, and the line across it
        const float mx = me.x, my = me.y;
        const auto [ox, oy] = pixel_centre(ni, nj, H, W);
        const float s_near = horizontal ? (r.a_near ? mx : ox) : (r.a_near ? my : oy);
        const float s_far = horizontal ? (r.a_near ? ox : mx) : (r.a_near ? oy : my);
        const float line = horizontal ? my : mx;   // (shared by both pixels of the pair)
        const int o_al = horizontal ? 0 : 1, o_ac = horizontal ? 1 : 0;
        const float *c = xy + (int64_t)r.T * 6;
        const float xa = c[r.ka * 2 + o_al], ya = c[r.ka * 2 + o_ac], xb = c[r.kb * 2 + o_al], yb = c[r.kb * 2 + o_ac];
        const float dxs = dt[n] / (s_far - s_near);          // dL/dx*
        const float den = yb - ya, s = (line - ya) / den;
        const float k = dxs * (xb - xa) / (den * den);
        float *g = gxy + ((int64_t)b * F + r.T) * 6;
        atomicAdd(&g[r.ka * 2 + o_al], dxs * (1.0f - s));
        atomicAdd(&g[r.kb * 2 + o_al], dxs * s);
        atomicAdd(&g[r.ka * 2 + o_ac], k * (line - yb));
        atomicAdd(&g[r.kb * 2 + o_ac], -(k * (line - ya)));
    }
}

// ------------------------------------------------------------------------------------------------ barycentrics
// One thread per pixel: the transpose of raster_face_test's weights on the winning face: both stages of raster_shared.h
// on the pixel centre and the face (bary itself is not inverted), then their derivatives.
__global__ void __launch_bounds__(256)
k_raster_bary_bwd(const float *__restrict__ gbary, const int32_t *__restrict__ face_idx,
                  const float *__restrict__ face_xy, const float *__restrict__ face_z, int B, int H, int W, int F,
                  float *__restrict__ gxy, float *__restrict__ gz) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)B * H * W) return;
    const int f = face_idx[p];
    if (f < 0 || f >= F) return;
    const float g0 = gbary[p * 3], g1 = gbary[p * 3 + 1], g2 = gbary[p * 3 + 2];
    if (g0 == 0.f && g1 == 0.f && g2 == 0.f) return;
    const auto [b, i, j] = pixel_of(p, H, W);
    const auto [px, py] = pixel_centre(i, j, H, W);
    const int64_t bf = (int64_t)b * F + f;
    const float *c = face_xy + bf * 6, *z = face_z + bf * 3;
    const float x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5];
    const float z0 = z[0], z1 = z[1], z2 = z[2];
    const FaceW w = face_weights(face_area(x0, y0, x1, y1, x2, y2), px, py, x0, y0, x1, y1, x2, y2);
    const FaceP pw = face_perspective(w, z0, z1, z2);
    const float inv = w.inv, w0 = w.w0, w1 = w.w1, q0 = pw.q0, q1 = pw.q1, q2 = pw.q2, zi = pw.z;
    // b_k = q_k / qs
    const float gb = (g0 * pw.b0 + g1 * pw.b1) + g2 * pw.b2;
    const float dq0 = (g0 - gb) * zi, dq1 = (g1 - gb) * zi, dq2 = (g2 - gb) * zi;
    // q_k = w_k / z_k
    const float dw0 = dq0 / z0, dw1 = dq1 / z1, dw2 = dq2 / z2;
    atomicAdd(&gz[bf * 3], -(dq0 * q0 / z0));
    atomicAdd(&gz[bf * 3 + 1], -(dq1 * q1 / z1));
    atomicAdd(&gz[bf * 3 + 2], -(dq2 * q2 / z2));
    // w2 = 1 - w0 - w1;  w0 = e0 / area, w1 = e1 / area
    const float a0 = dw0 - dw2, a1 = dw1 - dw2;
    const float de0 = a0 * inv, de1 = a1 * inv, da = -((a0 * w0 + a1 * w1) * inv);
    float *g = gxy + bf * 6;
    atomicAdd(&g[0], da * (y1 - y2) - de1 * (y2 - py));                       // x0
    atomicAdd(&g[1], da * (x2 - x1) + de1 * (x2 - px));                       // y0
    atomicAdd(&g[2], da * (y2 - y0) + de0 * (y2 - py));                       // x1
    atomicAdd(&g[3], -(da * (x2 - x0)) - de0 * (x2 - px));                    // y1
    atomicAdd(&g[4], (de1 * (y0 - py) - de0 * (y1 - py)) - da * (y1 - y0));   // x2
    atomicAdd(&g[5], (de0 * (x1 - px) - de1 * (x0 - px)) + da * (x1 - x0));   // y2
}

// grad_bary[p,k] = sum_d attr[f,k,d] * dfeat[p,d]: one thread per (pixel, corner), d ascending, one writer
__global__ void __launch_bounds__(256)
k_interp_attr_bwd_bary(const int32_t *__restrict__ face_idx, const float *__restrict__ attr,
                       const float *__restrict__ dfeat, int64_t P, int D, int F, float *__restrict__ gbary) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P * 3) return;
    const int64_t p = t / 3;
    const int k = (int)(t - p * 3);
    const int f = face_idx[p];
    float acc = 0.f;
    if (f >= 0 && f < F) {
        const float *a = attr + ((int64_t)f * 3 + k) * D;
        for (int d = 0; d < D; ++d) acc += a[d] * dfeat[p * D + d];
    }
    gbary[t] = acc;
}

// grad_uv of the bilinear lookup: one thread per pixel, channels ascending, one writer.  tex_coords' texel position is
// x = u R - 1/2, y = (1 - v) R - 1/2, so dx/du = R and dy/dv = -R; an axis whose clamp is active (uv outside [0, 1], or
// the position on or beyond the border texels' centres) gets 0, as grid_sample's border padding gives.
__global__ void __launch_bounds__(256)
k_texture_map_bwd_uv(const float *__restrict__ uv, const int32_t *__restrict__ face_idx, const float *__restrict__ tex,
                     const float *__restrict__ dout, int64_t P, int C, int R, float *__restrict__ guv) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float gu = 0.f, gv = 0.f;
    if (!face_idx || face_idx[p] >= 0) {
        const float u = uv[p * 2], v = uv[p * 2 + 1];
        float x, y;
        tex_coords(u, v, R, false, x, y);
        const float top = (float)(R - 1);
        const bool live_x = u >= 0.f && u <= 1.f && x > 0.f && x < top;
        const bool live_y = v >= 0.f && v <= 1.f && y > 0.f && y < top;
        if (live_x || live_y) {
            const BilTaps b = bil_taps(u, v, R);
            const float fx = b.ax, fy = b.ay;   // the fractions of the clamped position
            float sx = 0.f, sy = 0.f;
            for (int c = 0; c < C; ++c) {
                const float *tc = tex + (int64_t)c * R * R;
                const float t00 = tc[b.i00], t01 = tc[b.i01], t10 = tc[b.i10], t11 = tc[b.i11];
                const float g = dout[p * C + c];
                sx += g * ((1.0f - fy) * (t01 - t00) + fy * (t11 - t10));
                sy += g * ((1.0f - fx) * (t10 - t00) + fx * (t11 - t01));
            }
            if (live_x) gu = sx * (float)R;
            if (live_y) gv = -(sy * (float)R);
        }
    }
    guv[p * 2] = gu;
    guv[p * 2 + 1] = gv;
}

// ------------------------------------------------------------------------------------------------ projection
// One thread per (view, face): the transpose of cam_project (raster_shared.h) for its three corners, atomics into grad_verts.
// A corner whose incoming gradient is all zero adds nothing (so a face the rasteriser rejects never divides by its z here).
__global__ void __launch_bounds__(256)
k_raster_prepare_batch_bwd(const float *__restrict__ gxy, const float *__restrict__ gz, const float *__restrict__ verts,
                           int V, const int32_t *__restrict__ faces, int F, const float *__restrict__ cams,
                           float *__restrict__ gverts) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const Cam cam = cam_read(cams + blockIdx.y * CAM_FLOATS);
    const float *rot = cam.rec + CAM_ROT;
    const float fx = cam.rec[CAM_FX], fy = cam.rec[CAM_FY];
    const int64_t bf = (int64_t)blockIdx.y * F + f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float gix = gxy[(bf * 3 + k) * 2], giy = gxy[(bf * 3 + k) * 2 + 1], gcz = gz[bf * 3 + k];
        if (gix == 0.f && giy == 0.f && gcz == 0.f) continue;
        const int v = faces[f * 3 + k];
        if (v < 0 || v >= V) continue;
        const auto [cz, ix, iy] = cam_project(cam.rec, verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]);
        // ix = cx fx / (-cz), iy = cy fy / (-cz), z = cz
        const float dcx = gix * fx / (-cz), dcy = giy * fy / (-cz);
        const float dcz = gcz - (gix * ix + giy * iy) / cz;
        atomicAdd(&gverts[v * 3], (rot[0] * dcx + rot[3] * dcy) + rot[6] * dcz);
        atomicAdd(&gverts[v * 3 + 1], (rot[1] * dcx + rot[4] * dcy) + rot[7] * dcz);
        atomicAdd(&gverts[v * 3 + 2], (rot[2] * dcx + rot[5] * dcy) + rot[8] * dcz);
    }
}

// ------------------------------------------------------------------------------------------------ umbrella operator
// deg[v] = the number of face corners that hold v (faces with an index out of range count nowhere)
__device__ __forceinline__ bool face_in_range(const int32_t *__restrict__ faces, int f, int V, int v[3]) {
    v[0] = faces[f * 3]; v[1] = faces[f * 3 + 1]; v[2] = faces[f * 3 + 2];
    return v[0] >= 0 && v[0] < V && v[1] >= 0 && v[1] < V && v[2] >= 0 && v[2] < V;
}
__global__ void __launch_bounds__(256)
k_umbrella_degree(const int32_t *__restrict__ faces, int F, int V, int32_t *__restrict__ deg) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!face_in_range(faces, f, V, v)) return;
    atomicAdd(&deg[v[0]], 1); atomicAdd(&deg[v[1]], 1); atomicAdd(&deg[v[2]], 1);
}
// acc += the face terms, summed apart from x so that their rounding is that of their own (smaller) magnitude: L takes
// (x_j + x_k) / (2 n_i), its transpose y_j / (2 n_j) + y_k / (2 n_k); k_umbrella_finish then gives out = x - acc
__global__ void __launch_bounds__(256)
k_umbrella_faces(const float *__restrict__ x, const int32_t *__restrict__ faces, int F, int V,
                 const int32_t *__restrict__ deg, int transpose, float *__restrict__ acc) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!face_in_range(faces, f, V, v)) return;
    float h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = 0.5f / (float)deg[v[k]];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int kj = k == 2 ? 0 : k + 1, kl = k == 0 ? 2 : k - 1;
        const int i = v[k], j = v[kj], l = v[kl];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float term = transpose ? x[j * 3 + a] * h[kj] + x[l * 3 + a] * h[kl] : (x[j * 3 + a] + x[l * 3 + a]) * h[k];
            atomicAdd(&acc[i * 3 + a], term);
        }
    }
}
__global__ void __launch_bounds__(256)
k_umbrella_finish(const float *__restrict__ x, const float *__restrict__ acc, int n, float *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = x[t] - acc[t];
}

// scratch: deg int32 [V] (padded to 16 bytes), then acc f32 [V,3]
static size_t umbrella_deg_bytes(int V) { return (((size_t)V * sizeof(int32_t)) + 15) & ~(size_t)15; }
static size_t umbrella_scratch_bytes(int V, int F) {
    if (V < 1 || V > 0x7fffffff / 3 || F < 0 || F > LNERF_MESH_MAX_FACES) return 0;
    return umbrella_deg_bytes(V) + (((size_t)V * 3 * sizeof(float) + 15) & ~(size_t)15);
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_raster_antialias_forward(const float *image, const int32_t *face_idx, const float *bary, const float *face_xy,
                                   const float *face_z, const int32_t *faces, int B, int H, int W, int C, int n_faces,
                                   float *out, lnerf_stream_t stream) {
    if (int e = check_raster_dims("raster_antialias_forward", B, H, W, n_faces)) return e;
    LNERF_REQUIRE(C >= 1 && C <= 64, "raster_antialias_forward: C must be in [1, 64] (got %d)", C);
    LNERF_REQUIRE(image && face_idx && bary && face_xy && face_z && faces && out, "raster_antialias_forward: null pointer");
    LNERF_REQUIRE(out != image, "raster_antialias_forward: out must not be image");
    const int64_t P = (int64_t)B * H * W;
    LNERF_LAUNCH(k_raster_antialias<false>, P, 256, as_stream(stream), image, (const float *)nullptr, face_idx, bary,
                 face_xy, face_z, faces, B, H, W, C, n_faces, out, (float *)nullptr);
    LNERF_CHECK_LAUNCH("raster_antialias_forward");
    return LNERF_OK;
}

int lnerf_raster_antialias_backward(const float *grad_out, const float *image, const int32_t *face_idx,
                                    const float *bary, const float *face_xy, const float *face_z, const int32_t *faces,
                                    int B, int H, int W, int C, int n_faces, float *grad_image, float *grad_face_xy,
                                    lnerf_stream_t stream) {
    if (int e = check_raster_dims("raster_antialias_backward", B, H, W, n_faces)) return e;
    LNERF_REQUIRE(C >= 1 && C <= 64, "raster_antialias_backward: C must be in [1, 64] (got %d)", C);
    LNERF_REQUIRE(grad_out && image && face_idx && bary && face_xy && face_z && faces && grad_image && grad_face_xy,
                  "raster_antialias_backward: null pointer");
    LNERF_REQUIRE(grad_image != grad_out && grad_image != image, "raster_antialias_backward: grad_image must be its own buffer");
    const int64_t P = (int64_t)B * H * W;
    LNERF_LAUNCH(k_raster_antialias<true>, P, 256, as_stream(stream), image, grad_out, face_idx, bary, face_xy, face_z,
                 faces, B, H, W, C, n_faces, grad_image, grad_face_xy);
    LNERF_CHECK_LAUNCH("raster_antialias_backward");
    return LNERF_OK;
}

int lnerf_raster_bary_backward(const float *grad_bary, const int32_t *face_idx, const float *face_xy,
                               const float *face_z, int B, int H, int W, int n_faces, float *grad_face_xy,
                               float *grad_face_z, lnerf_stream_t stream) {
    if (int e = check_raster_dims("raster_bary_backward", B, H, W, n_faces)) return e;
    LNERF_REQUIRE(grad_bary && face_idx && face_xy && face_z && grad_face_xy && grad_face_z,
                  "raster_bary_backward: null pointer");
    LNERF_LAUNCH(k_raster_bary_bwd, (int64_t)B * H * W, 256, as_stream(stream), grad_bary, face_idx, face_xy, face_z, B,
                 H, W, n_faces, grad_face_xy, grad_face_z);
    LNERF_CHECK_LAUNCH("raster_bary_backward");
    return LNERF_OK;
}

int lnerf_interpolate_attributes_backward_bary(const int32_t *face_idx, const float *attr, const float *dfeat,
                                               int n_pixels, int D, int n_faces, float *grad_bary,
                                               lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && n_pixels <= 0x7fffffff / 16 && D >= 1 && D <= 16,
                  "interpolate_attributes_backward_bary: bad sizes");
    LNERF_REQUIRE(n_faces >= 1, "interpolate_attributes_backward_bary: n_faces must be >= 1 (got %d)", n_faces);
    LNERF_REQUIRE(face_idx && attr && dfeat && grad_bary, "interpolate_attributes_backward_bary: null pointer");
    LNERF_LAUNCH(k_interp_attr_bwd_bary, (int64_t)n_pixels * 3, 256, as_stream(stream), face_idx, attr, dfeat,
                 (int64_t)n_pixels, D, n_faces, grad_bary);
    LNERF_CHECK_LAUNCH("interpolate_attributes_backward_bary");
    return LNERF_OK;
}

int lnerf_texture_map_backward_uv(const float *uv, const int32_t *face_idx, const float *texture, const float *dout,
                                  int n_pixels, int C, int R, float *grad_uv, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_pixels > 0 && C >= 1 && R >= 1 && R <= 32768, "texture_map_backward_uv: bad arguments");
    LNERF_REQUIRE(uv && texture && dout && grad_uv, "texture_map_backward_uv: null pointer");
    LNERF_LAUNCH(k_texture_map_bwd_uv, (int64_t)n_pixels, 256, as_stream(stream), uv, face_idx, texture, dout,
                 (int64_t)n_pixels, C, R, grad_uv);
    LNERF_CHECK_LAUNCH("texture_map_backward_uv");
    return LNERF_OK;
}

int lnerf_raster_prepare_batch_backward(const float *grad_face_xy, const float *grad_face_z, const float *verts,
                                        int n_verts, const int32_t *faces, int n_faces, const float *cams_dev, int B,
                                        float *grad_verts, lnerf_stream_t stream) {
    LNERF_REQUIRE(n_verts > 0 && n_faces > 0 && n_faces <= LNERF_MESH_MAX_FACES && n_verts <= 0x7fffffff / 3,
                  "raster_prepare_batch_backward: bad mesh sizes");
    LNERF_REQUIRE(B >= 1 && B <= 65535, "raster_prepare_batch_backward: B must be in [1, 65535]");
    LNERF_REQUIRE(grad_face_xy && grad_face_z && verts && faces && cams_dev && grad_verts,
                  "raster_prepare_batch_backward: null pointer");
    hipStream_t s = as_stream(stream);
    if (!hip_ok(hipMemsetAsync(grad_verts, 0, (size_t)n_verts * 3 * sizeof(float), s), "raster_prepare_batch_backward: memset"))
        return LNERF_ERR_HIP;
    hipLaunchKernelGGL(k_raster_prepare_batch_bwd, dim3((unsigned)div_up(n_faces, 256), (unsigned)B), dim3(256), 0, s,
                       grad_face_xy, grad_face_z, verts, n_verts, faces, n_faces, cams_dev, grad_verts);
    LNERF_CHECK_LAUNCH("raster_prepare_batch_backward");
    return LNERF_OK;
}

size_t lnerf_mesh_umbrella_scratch_bytes(int n_verts, int n_faces) { return umbrella_scratch_bytes(n_verts, n_faces); }

int lnerf_mesh_umbrella(const float *x, int n_verts, const int32_t *faces, int n_faces, int transpose, void *scratch,
                        size_t scratch_bytes, float *out, lnerf_stream_t stream) {
    const size_t need = umbrella_scratch_bytes(n_verts, n_faces);
    LNERF_REQUIRE(need > 0 && n_verts <= 0x7fffffff / 3, "mesh_umbrella: n_verts (%d) or n_faces (%d) out of range", n_verts, n_faces);
    LNERF_REQUIRE(transpose == 0 || transpose == 1, "mesh_umbrella: transpose must be 0 or 1 (got %d)", transpose);
    LNERF_REQUIRE(x && out && (faces || n_faces == 0), "mesh_umbrella: null pointer");
    LNERF_REQUIRE(out != x, "mesh_umbrella: out must not be x");
    LNERF_REQUIRE(scratch && scratch_bytes >= need && ((uintptr_t)scratch & 15) == 0,
                  "mesh_umbrella: scratch must be 16-byte aligned and hold %zu bytes", need);
    hipStream_t s = as_stream(stream);
    if (n_faces == 0) {
        if (!hip_ok(hipMemcpyAsync(out, x, (size_t)n_verts * 3 * sizeof(float), hipMemcpyDeviceToDevice, s), "mesh_umbrella: copy"))
            return LNERF_ERR_HIP;
        return LNERF_OK;
    }
    int32_t *deg = static_cast<int32_t *>(scratch);
    float *acc = reinterpret_cast<float *>(static_cast<char *>(scratch) + umbrella_deg_bytes(n_verts));
    if (!hip_ok(hipMemsetAsync(scratch, 0, need, s), "mesh_umbrella: memset")) return LNERF_ERR_HIP;
    LNERF_LAUNCH(k_umbrella_degree, n_faces, 256, s, faces, n_faces, n_verts, deg);
    LNERF_LAUNCH(k_umbrella_faces, n_faces, 256, s, x, faces, n_faces, n_verts, deg, transpose, acc);
    LNERF_LAUNCH(k_umbrella_finish, (int64_t)n_verts * 3, 256, s, x, acc, n_verts * 3, out);
    LNERF_CHECK_LAUNCH("mesh_umbrella");
    return LNERF_OK;
}

}  // extern "C"
