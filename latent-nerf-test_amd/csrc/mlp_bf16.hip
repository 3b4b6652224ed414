// H7 fused sigma/latent MLP, bf16 MFMA path (v_mfma_f32_16x16x32_bf16, f32 accumulate).
//
// "Sample on the lane" formulation: every layer computes Z^T = W · X^T, i.e. A = a 16-row tile of the
// weight matrix, B = activations with the SAMPLE on the MFMA column (lane & 15).  The C/D tile of one
// layer (4 consecutive output features in the registers of a lane, its sample on the lane) is then
// directly the B operand of the next layer: no LDS, no cross-lane traffic between layers.  The k order
// inside a k-step is permuted by that reuse (slot (q, jj) of k-step s holds feature
// phi = 32 s + 16 (jj >> 2) + 4 q + (jj & 3)); the weight fragments are built once per workgroup with
// the same permutation baked in and live in LDS in fragment order (one conflict-free ds_read_b128 per
// operand).  The same trick runs the backward data chain (dA2 -> dA1 -> dX) with transposed weights.
// Only the weight gradients, which sum over SAMPLES, need a transpose.  dZ and H tiles are staged once per
// 128-sample workgroup step as [sample][feature] bf16 images in LDS -- a lane stores the packed registers it
// already holds for the MFMA B operand, 8 bytes (4 consecutive features of its sample) at a time -- and the
// operands of dW = dZ^T (x) H^T (feature on the lane, 8 consecutive SAMPLES in the registers) are read back with
// gfx950's transposing LDS read, ds_read_b64_tr_b16 (cdna_hip_programming.md T10): no per-element conversions or
// 2-byte stores.  Each of the four waves owns a 16-row slice of every dW (no cross-wave reduction).  One f32 slab per workgroup goes to
// HBM and k_mlp_reduce_slabs (mlp.hip) sums the slabs in a fixed order: deterministic gradients.
//
// Lane maps (cdna_hip_programming.md §3): A[i = l&15][k = 8 (l>>4) + jj], B[k = 8 (l>>4) + jj][j = l&15],
// C/D[i = 4 (l>>4) + reg][j = l&15].  The index algebra is replayed on the CPU by
// tests/test_mlp_bf16_layout_emulation.py.
#include "common.h"
#include "mlp_shared.h"

namespace lnerf {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// fragment slots in LDS (each slot: 64 lanes x 8 bf16 = 1 KiB)
constexpr int F_W1A = 0;    // [mt 0..3]          forward  layer 1:  W1[16mt+c][8q+jj]
constexpr int F_W2A = 4;    // [mt 0..3][s 0..1]  forward  layer 2:  W2[16mt+c][phi]
constexpr int F_W3A = 12;   // [s 0..1]           forward  layer 3:  W3[c][phi]
constexpr int F_W3T = 14;   // [mt 0..3]          backward dA2:      W3[4q+jj][16mt+c]
constexpr int F_W2T = 18;   // [mt 0..3][s 0..1]  backward dA1:      W2[phi][16mt+c]
constexpr int F_W1T = 26;   // [mt 0..1][s 0..1]  backward dX:       W1[phi][16mt+c]
constexpr int F_FWD = 14, F_ALL = 30;

constexpr int RS = 68;      // bf16 elements per row of a [128 samples][feature] staging image (64 + 4 pad: 136 B,
                            // a multiple of 8 B as the transposing read requires; 16 lanes' 8-byte stores of one
                            // column group fall on 16 different bank pairs)

__device__ __forceinline__ int phi_of(int s, int q, int jj) { return 32 * s + 16 * (jj >> 2) + 4 * q + (jj & 3); }

// Where element e of the weight-fragment image comes from: tensor 1 / 2 / 3 (= w1 / w2 / w3) and the index into it, or
// 0 for a constant zero (padding of the 16-row output tile).  ONE statement of the layout: the builder below reads
// through it, k_mlp_fragment_maps inverts it for the optimiser's fragment shadow.
__device__ __forceinline__ int frag_source(int e, int out_dim, int &idx) {
    const int f = e >> 9, l = (e >> 3) & 63, jj = e & 7;
    const int q = l >> 4, c = l & 15;
    if (f < F_W2A) {
        idx = (16 * (f - F_W1A) + c) * MLP_IN + 8 * q + jj;
        return 1;
    } else if (f < F_W3A) {
        const int mt = (f - F_W2A) >> 1, s = (f - F_W2A) & 1;
        idx = (16 * mt + c) * MLP_HID + phi_of(s, q, jj);
        return 2;
    } else if (f < F_W3T) {
        const int s = f - F_W3A;
        idx = c * MLP_HID + phi_of(s, q, jj);
        return c < out_dim ? 3 : 0;
    } else if (f < F_W2T) {
        const int mt = f - F_W3T, n = 4 * q + jj;
        idx = n * MLP_HID + 16 * mt + c;
        return (jj < 4 && n < out_dim) ? 3 : 0;
    } else if (f < F_W1T) {
        const int mt = (f - F_W2T) >> 1, s = (f - F_W2T) & 1;
        idx = phi_of(s, q, jj) * MLP_HID + 16 * mt + c;
        return 2;
    }
    const int mt = (f - F_W1T) >> 1, s = (f - F_W1T) & 1;
    idx = phi_of(s, q, jj) * MLP_IN + 16 * mt + c;
    return 1;
}

// build weight fragments cooperatively (all threads of the workgroup)
__device__ __forceinline__ void build_fragments(const MlpArgs &a, __bf16 *frag, int n_frag, int tid, int nthreads) {
    for (int e = tid; e < n_frag * 512; e += nthreads) {
        int idx;
        const int t = frag_source(e, a.out_dim, idx);
        const float v = t == 1 ? a.w1[idx] : t == 2 ? a.w2[idx] : t == 3 ? a.w3[idx] : 0.f;
        frag[e] = (__bf16)v;
    }
}

// Inverse of the layout: map_t[2 i] / map_t[2 i + 1] = the element of the fragment image that holds weight i of tensor
// t in the forward / the transposed (backward) fragments -- every weight sits in exactly one of each.  With these the
// optimiser's multi-tensor Adam launch writes the bf16 fragments itself (lnerf_adam_step_multi_shadow), and the
// per-step fragment build (one dispatch) goes away.
__global__ void __launch_bounds__(256) k_mlp_fragment_maps(int out_dim, int32_t *m1, int32_t *m2, int32_t *m3) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < F_ALL * 512; e += gridDim.x * 256) {
        int idx;
        const int t = frag_source(e, out_dim, idx);
        const int slot = (e >> 9) < F_W3T ? 0 : 1;
        int32_t *m = t == 1 ? m1 : t == 2 ? m2 : t == 3 ? m3 : nullptr;
        if (m) m[2 * idx + slot] = e;
    }
}

// The fragments of a launch, built ONCE into global memory (k_mlp_build_fragments) and copied into LDS by every
// workgroup with coalesced 16-byte loads: a workgroup building its own took 28 (forward) / 60 (backward) dependent
// scattered weight loads per thread before its first tile -- a quarter of the kernels' time at ~6 tiles per workgroup.
static_assert((size_t)F_ALL * 1024 <= MLP_FRAG_BYTES, "fragment cache");
__global__ void __launch_bounds__(256) k_mlp_build_fragments(MlpArgs a, __bf16 *out, int n_frag) {
    build_fragments(a, out, n_frag, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
// The copy is cut in two, `request` (global -> registers) and `write` (registers -> LDS), so that a kernel can put the
// requests of its first step's inputs BETWEEN them: vector loads return in issue order, the LDS writes wait for the
// fragments only, and the inputs cross the fragments' round trip, the writes and the workgroup's barrier in flight.
// Every lane loads N_FRAG * 64 / 256 rounded up times, the index clamped into the image (no branch around a load);
// the write drops what lies past the end.
template <int N_FRAG>
struct FragmentCopy {
    static constexpr int TOTAL = N_FRAG * 64, N = (TOTAL + 255) / 256;   // 16-byte words: of the image, per lane
    u32x4 r[N];
    __device__ __forceinline__ void request(const void *frag_global, int tid) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(frag_global);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int e = tid + 256 * j;
            r[j] = src[e < TOTAL ? e : TOTAL - 1];
        }
    }
    __device__ __forceinline__ void write(__bf16 *frag, int tid) const {
        u32x4 *dst = reinterpret_cast<u32x4 *>(frag);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int e = tid + 256 * j;
            if (j < TOTAL / 256 || e < TOTAL) dst[e] = r[j];
        }
    }
};
// The biases of the hidden layers travel with the fragments: raw loads by every lane (index wrapped into the 64), the
// first 64 threads write them to LDS.
struct BiasCopy {
    float b1, b2;
    __device__ __forceinline__ void request(const MlpArgs &a, int tid) {
        b1 = a.b1[tid & (MLP_HID - 1)];
        b2 = a.b2[tid & (MLP_HID - 1)];
    }
    __device__ __forceinline__ void write(float *sB1, float *sB2, int tid) const {
        if (tid < MLP_HID) { sB1[tid] = b1; sB2[tid] = b2; }
    }
};

__device__ __forceinline__ bf16x8 ld_frag(const __bf16 *frag, int f, int lane) {
    return *reinterpret_cast<const bf16x8 *>(frag + (f * 64 + lane) * 8);
}

// B fragment of X^T for one 16-sample column tile: lane (q, c) holds features 8q..8q+7 (levels 4q..4q+3)
// `m` is CLAMPED into the valid samples by the callers (no exec-masked branch around the loads): a row past the end
// reads the last sample's features, which nothing consumes -- its outputs are not stored (forward) and its upstream
// gradient is zero (backward).
// FB16 (compile time: a run-time test of a.feat_bf16 here puts two load forms on two arms inside the step loops, and the
// merge of the arms waits for everything in flight).  bf16 features are RAW loads -- four dwords that are the operand
// as they arrive; f32 features are converted where they are loaded.
template <bool FB16>
__device__ __forceinline__ bf16x8 load_x(const MlpArgs &a, int64_t m, int q) {
    if (FB16) {
        // 32-bit byte offsets from the (uniform) base: `global_load_dword v, v_off, s[base]` instead of three 64-bit
        // VALU operations per address (the launcher checks 16 * level_stride * 8 < 2^32)
        const char *f = reinterpret_cast<const char *>(a.feat);
        const uint32_t ls = (uint32_t)a.level_stride;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = *reinterpret_cast<const uint32_t *>(f + (size_t)((((uint32_t)(4 * q + k)) * ls + (uint32_t)m) << 2));
        return *reinterpret_cast<bf16x8 *>(w);
    }
    bf16x8 x;
    const float2 *f = reinterpret_cast<const float2 *>(a.feat);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 v = f[(int64_t)(4 * q + k) * a.level_stride + m];
        x[2 * k] = (__bf16)v.x;
        x[2 * k + 1] = (__bf16)v.y;
    }
    return x;
}
__device__ __forceinline__ int64_t clamp_row(int64_t m, int64_t M) { return m < M ? m : (M > 0 ? M - 1 : 0); }

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// v_cvt_pk_bf16_f32, left to the compiler: an inline-asm form hides the MFMA-result read from its hazard recogniser
__device__ __forceinline__ uint32_t cvt_pk(float lo, float hi) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}
// relu on a packed bf16 pair: the sign bit of a bf16 is the sign bit of the int16 holding it
__device__ __forceinline__ uint32_t relu_pk(uint32_t v) {
    const s16x2 z = {0, 0};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), z));
}
// 0xFFFF in every half of `act` (a relu'd pair: +0 or positive) that is non-zero: 0 - a has its sign bit set exactly
// for a in 1 .. 0x7FFF, an arithmetic shift spreads it (v_pk_sub_i16 + v_pk_ashrrev_i16; a min/sub form was turned
// into two compares, two selects and a permute per pair by the compiler)
__device__ __forceinline__ uint32_t live_pk(uint32_t act) {
    asm("" : "+v"(act));   // (opaque to the optimiser: knowing act >= 0 it rewrites the two packed ops into selects again)
    const s16x2 z = {0, 0};
    const s16x2 n = z - __builtin_bit_cast(s16x2, act);
    return __builtin_bit_cast(uint32_t, n >> 15);
}
union Pk8 {
    bf16x8 v;
    uint32_t u[4];
};
// relu + pack two C tiles (2s, 2s+1) into the B fragment of k-step s
__device__ __forceinline__ bf16x8 pack_relu(const f32x4 &lo, const f32x4 &hi) {
    Pk8 r;
    r.u[0] = relu_pk(cvt_pk(lo[0], lo[1]));
    r.u[1] = relu_pk(cvt_pk(lo[2], lo[3]));
    r.u[2] = relu_pk(cvt_pk(hi[0], hi[1]));
    r.u[3] = relu_pk(cvt_pk(hi[2], hi[3]));
    return r.v;
}
// pack d(pre-activation) = d(activation) masked by the packed activation being positive
__device__ __forceinline__ bf16x8 pack_masked(const f32x4 &lo, const f32x4 &hi, const bf16x8 &act) {
    Pk8 r, a;
    a.v = act;
    r.u[0] = cvt_pk(lo[0], lo[1]) & live_pk(a.u[0]);
    r.u[1] = cvt_pk(lo[2], lo[3]) & live_pk(a.u[1]);
    r.u[2] = cvt_pk(hi[0], hi[1]) & live_pk(a.u[2]);
    r.u[3] = cvt_pk(hi[2], hi[3]) & live_pk(a.u[3]);
    return r.v;
}

__device__ __forceinline__ f32x4 ld_bias4(const float *b, int base) {
    return (f32x4){b[base], b[base + 1], b[base + 2], b[base + 3]};
}

// Phase stamps (diagnostic builds only: -DLNERF_STAMPS, tools/mlp_stamps.py): the shader clock at the marks of ONE
// wavefront per workgroup, summed per phase into a global table.  No memory drain at a mark: what a phase waits for
// shows up in the phase that consumes it.
#ifdef LNERF_STAMPS
__device__ unsigned long long g_mlp_stamps[32];
struct Stamps {
    unsigned long long acc[16], prev;
    __device__ __forceinline__ void init() {
        for (int i = 0; i < 16; ++i) acc[i] = 0;
        prev = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void mark(int k) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[k] += now - prev;
        prev = now;
    }
    __device__ __forceinline__ void flush(int base) {
        if (threadIdx.x == 0)
            for (int i = 0; i < 16; ++i) atomicAdd(&g_mlp_stamps[base + i], acc[i]);
    }
};
#else
struct Stamps {
    __device__ __forceinline__ void init() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush(int) {}
};
#endif

// The loop-invariant operands of layers 1 and 2 that the forward keeps in registers across its steps: the twelve weight
// fragments and layer 1's biases, read from LDS ONCE in front of the step loop (the loop holds an asm volatile, behind
// which the optimiser re-reads anything it has not been handed as a value).  Layer 2's biases and layer 3's fragments
// are re-read every step: with them the kernel would not fit the 168 registers of three waves per SIMD.
struct HeldFragments {
    bf16x8 w1[4], w2[8];
    f32x4 b1[4];
    __device__ __forceinline__ void read(const __bf16 *frag, const float *sB1, int lane) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            w1[mt] = ld_frag(frag, F_W1A + mt, lane);
            b1[mt] = ld_bias4(sB1, 16 * mt + 4 * (lane >> 4));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) w2[i] = ld_frag(frag, F_W2A + i, lane);
    }
};

// shared forward: xB[T] -> h1B[2][T], h2B[2][T] (packed, relu'd; T 16-sample column tiles); weights from LDS fragments,
// or from `held` where the caller keeps them in registers
template <int T>
__device__ __forceinline__ void forward_hidden(const __bf16 *frag, const float *sB1, const float *sB2, int lane,
                                               const bf16x8 xB[T], bf16x8 h1B[2][T], bf16x8 h2B[2][T], Stamps &st,
                                               const HeldFragments *held = nullptr) {
    const int q = lane >> 4;
    f32x4 acc[4][T];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 w = held ? held->w1[mt] : ld_frag(frag, F_W1A + mt, lane);
        const f32x4 b = held ? held->b1[mt] : ld_bias4(sB1, 16 * mt + 4 * q);
#pragma unroll
        for (int t = 0; t < T; ++t) acc[mt][t] = MFMA32(w, xB[t], b);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < T; ++t) h1B[s][t] = pack_relu(acc[2 * s][t], acc[2 * s + 1][t]);
    st.mark(1);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const f32x4 b = ld_bias4(sB2, 16 * mt + 4 * q);
#pragma unroll
        for (int t = 0; t < T; ++t) acc[mt][t] = b;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 w = held ? held->w2[2 * mt + s] : ld_frag(frag, F_W2A + 2 * mt + s, lane);
#pragma unroll
            for (int t = 0; t < T; ++t) acc[mt][t] = MFMA32(w, h1B[s][t], acc[mt][t]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < T; ++t) h2B[s][t] = pack_relu(acc[2 * s][t], acc[2 * s + 1][t]);
    st.mark(2);
}

// ------------------------------------------------------------------ forward
// "These registers are needed HERE": an empty asm that reads and rewrites them.  The compiler places its wait for the
// loads that fill the first group in front of it, and what is stored from the second group is stored behind it.  Both
// step loops use it ONCE per step, behind the step's last MFMA and in front of its stores: the next step's inputs were
// requested at the top of the step and have had all of its arithmetic to arrive; the stores go out behind the wait, so
// that the wait of the NEXT step does not cover their acknowledgements too (a wave has one in-order counter for loads
// and stores).  Without it the compiler waits where a value is first touched -- at the selects behind a load, at the
// merge of two arms that load differently, at the first MFMA of the next step with vmcnt(0), i.e. for the stores.
__device__ __forceinline__ void pin_x(bf16x8 &a, bf16x8 &b) {
    u32x4 ua = __builtin_bit_cast(u32x4, a), ub = __builtin_bit_cast(u32x4, b);
    asm volatile("" : "+v"(ua), "+v"(ub));
    a = __builtin_bit_cast(bf16x8, ua);
    b = __builtin_bit_cast(bf16x8, ub);
}

// WPS: wavefronts per SIMD the register allocation aims at, 3 or 2 (mlp_fwd_wps).  Four (128 VGPRs) spilled 396 bytes
// per lane to scratch and was measured slower.  FB16 / OUT5: a.feat_bf16 and a.out_dim == 5 at compile time (the
// launcher picks): no run-time branch around a load or a store form inside the step loop.
template <int WPS, bool FB16, bool OUT5>
__global__ void __launch_bounds__(256, WPS)
k_mlp_forward_bf16(MlpArgs a, float *__restrict__ sigmas, float *__restrict__ rgbs) {
    __shared__ __attribute__((aligned(16))) __bf16 frag[F_FWD * 512];
    __shared__ float sB1[MLP_HID], sB2[MLP_HID], sB3[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
    // The prologue is ONE exposed memory round trip, not two in series (nothing else is resident that could hide one: the
    // persistent workgroups all start together).  The fragments and biases are requested first -- they need no M --, the
    // first step's inputs behind them as soon as M is there, and only then are the fragments written to LDS.
    FragmentCopy<F_FWD> fc;
    BiasCopy bc;
    const bool cached = __builtin_expect(a.frag_global != nullptr, 1);   // (a launch without the cache: the cold arm)
    if (cached) fc.request(a.frag_global, tid);
    bc.request(a, tid);
    const float b3 = a.b3[c < a.out_dim ? c : a.out_dim - 1];   // (out_dim >= 2: the launcher checks)
    __builtin_amdgcn_sched_barrier(0);
    const int64_t M = valid_count(a.m_host, a.m_dev);
    const int nrgb = a.out_dim - 1;
    // The inputs of a step -- features and positions of this wave's two 16-sample tiles -- are requested one step ahead:
    // raw loads by EVERY lane (the four q lanes of a sample read the same position) of rows clamped into the valid
    // samples, no lane predicate and no arithmetic on them until the step that consumes them.
    bf16x8 xB[2];
    Pos3 pos[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t mc = clamp_row((int64_t)blockIdx.x * 128 + w * 32 + 16 * t + c, M);
        xB[t] = load_x<FB16>(a, mc, q);
        pos[t] = load_pos(a, mc);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (cached) fc.write(frag, tid);
    else build_fragments(a, frag, F_FWD, tid, 256);
    bc.write(sB1, sB2, tid);
    if (tid < 16) sB3[tid] = tid < a.out_dim ? b3 : 0.f;
    __syncthreads();
    // (waited for HERE: a load still pending at the loop's entry makes the compiler wait at the top of every step)
    pin_x(xB[0], xB[1]);
    asm volatile("" : "+v"(pos[0].x), "+v"(pos[0].y), "+v"(pos[0].z), "+v"(pos[1].x), "+v"(pos[1].y), "+v"(pos[1].z));
    HeldFragments held;
    held.read(frag, sB1, lane);
    Stamps st;
    st.init();
    for (int64_t tile = blockIdx.x; tile * 128 < M; tile += gridDim.x) {
        const int64_t m0 = tile * 128 + w * 32;
        // this step's density blobs, from the positions that arrived during the previous step
        float blob[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) blob[t] = blob_at(a, pos[t]);
        // the next step's inputs: requested now, pinned behind this step's last MFMA
        bf16x8 xB_n[2], h1B[2][2], h2B[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t mc = clamp_row(m0 + (int64_t)gridDim.x * 128 + 16 * t + c, M);
            xB_n[t] = load_x<FB16>(a, mc, q);
            pos[t] = load_pos(a, mc);
        }
        // (the instruction scheduler may not move anything over this line: left alone it sinks the loads to the end of
        // the step, next to their wait)
        __builtin_amdgcn_sched_barrier(0);
        st.mark(0);
        forward_hidden<2>(frag, sB1, sB2, lane, xB, h1B, h2B, st, &held);
        const f32x4 b3 = ld_bias4(sB3, 4 * q);
        const bf16x8 w3a = ld_frag(frag, F_W3A, lane), w3b = ld_frag(frag, F_W3A + 1, lane);
        f32x4 o[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            o[t] = MFMA32(w3a, h2B[0][t], b3);
            o[t] = MFMA32(w3b, h2B[1][t], o[t]);
        }
        // ---- the one wait of the step: the next step's inputs, behind the last MFMA and in front of the stores
        __builtin_amdgcn_sched_barrier(0);
        pin_x(xB_n[0], xB_n[1]);
        asm volatile("" : "+v"(pos[0].x), "+v"(pos[0].y), "+v"(pos[0].z), "+v"(pos[1].x), "+v"(pos[1].y), "+v"(pos[1].z),
                          "+v"(o[0]), "+v"(o[1]));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t m = m0 + 16 * t + c;  // lane holds h[4q + r] of sample m
            if (OUT5) {
                // sigma + four latent channels: the q = 0 lane of a sample collects channel 4 from its q = 1 lane and
                // writes ONE 16-byte row (16 lanes = 256 contiguous bytes) instead of four scattered dwords -- the
                // store tail is where this kernel spends its time (tools/mlp_stamps.py)
                const float r3 = __shfl_down(o[t][0], 16, 64);
                if (q == 0 && m < M) {
                    sigmas[m] = expf(o[t][0] + blob[t]);
                    reinterpret_cast<float4 *>(rgbs)[m] = make_float4(o[t][1], o[t][2], o[t][3], r3);
                }
            } else if (m < M) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = 4 * q + r;
                    if (n == 0) sigmas[m] = expf(o[t][r] + blob[t]);
                    else if (n < a.out_dim) rgbs[m * nrgb + (n - 1)] = o[t][r];
                }
            }
        }
        st.mark(3);
        xB[0] = xB_n[0];
        xB[1] = xB_n[1];
    }
    st.flush(0);
}

// Upstream gradient of one lane (outputs 4q .. 4q+3 of its T samples), requested one step ahead of its use.
// OUT5 (sigma + four latent channels, the form that is trained): RAW registers only -- every lane loads its sample's
// dsigma, sigma and the 16-byte row of latent gradients from a row clamped into the valid samples (the four q groups
// of a sample read the same addresses: one access), with no lane predicate around any word and no select behind a
// load: a select consumes the value where it stands, i.e. the wave waits for the load it has just issued, and a word
// used under a predicate only (g.w, for q = 1) is split off its row and loaded inside the predicated block.  The
// q = 0 / q = 1 shares and d(sigma)/d(pre-activation) = sigma are applied by upstream_fragment, a step later.
// Other widths: the generic arm, predicated dword loads consumed where they are loaded.
template <int T, bool OUT5>
struct Upstream;
template <int T>
struct Upstream<T, true> { f32x4 g[T]; float ds[T], sg[T]; };
template <int T>
struct Upstream<T, false> { float v[T][4], sg[T]; };

template <int T>
__device__ __forceinline__ void load_upstream(Upstream<T, true> &u, const MlpArgs &a, const float *__restrict__ sigmas,
                                              const float *__restrict__ dsigmas, const float *__restrict__ drgbs,
                                              int64_t m0, int64_t M, int q, int c) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int64_t mc = clamp_row(m0 + 16 * t + c, M);
        u.ds[t] = dsigmas[mc];
        u.sg[t] = sigmas[mc];
        u.g[t] = reinterpret_cast<const f32x4 *>(drgbs)[mc];
    }
}
template <int T>
__device__ __forceinline__ void load_upstream(Upstream<T, false> &u, const MlpArgs &a, const float *__restrict__ sigmas,
                                              const float *__restrict__ dsigmas, const float *__restrict__ drgbs,
                                              int64_t m0, int64_t M, int q, int c) {
    const int nrgb = a.out_dim - 1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int64_t m = m0 + 16 * t + c;
        const bool in = m < M;
        u.sg[t] = 1.0f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) u.v[t][jj] = 0.f;
        if (in && q == 0) { u.v[t][0] = dsigmas[m]; u.sg[t] = sigmas[m]; }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int n = 4 * q + jj;
            if (in && n >= 1 && n < a.out_dim) u.v[t][jj] = drgbs[m * nrgb + (n - 1)];
        }
    }
}
// the B fragment of dZ3^T (slot (q, jj < 4) <-> output 4q + jj) of one column tile
__device__ __forceinline__ void upstream_fragment(const float v[4], float sg, int q, bf16x8 &d3) {
    const float v0 = q == 0 ? v[0] * trunc_exp_grad(sg) : v[0];
    Pk8 d;
    d.u[0] = cvt_pk(v0, v[1]);
    d.u[1] = cvt_pk(v[2], v[3]);
    d.u[2] = 0u;
    d.u[3] = 0u;
    d3 = d.v;
}
// (`in`: the lane's sample m0 + 16 t + c of the step that CONSUMES the values is a valid one)
template <int T>
__device__ __forceinline__ void upstream_fragment(const Upstream<T, true> &u, int t, bool in, int q, bf16x8 &d3) {
    const bool q0 = in && q == 0, q1 = in && q == 1;
    const float v[4] = {q0 ? u.ds[t] : (q1 ? u.g[t][3] : 0.f), q0 ? u.g[t][0] : 0.f, q0 ? u.g[t][1] : 0.f,
                        q0 ? u.g[t][2] : 0.f};
    upstream_fragment(v, u.sg[t], q, d3);
}
template <int T>
__device__ __forceinline__ void upstream_fragment(const Upstream<T, false> &u, int t, bool, int q, bf16x8 &d3) {
    upstream_fragment(u.v[t], u.sg[t], q, d3);
}
// the one wait of a backward step (pin_x above): the next step's features and upstream gradient, and the dX tiles that
// the stores behind it write
__device__ __forceinline__ void pin_step(bf16x8 x[2], Upstream<2, true> &u, f32x4 ax[2][2]) {
    u32x4 x0 = __builtin_bit_cast(u32x4, x[0]), x1 = __builtin_bit_cast(u32x4, x[1]);
    asm volatile("" : "+v"(x0), "+v"(x1), "+v"(u.g[0]), "+v"(u.g[1]), "+v"(u.ds[0]), "+v"(u.ds[1]), "+v"(u.sg[0]),
                      "+v"(u.sg[1]), "+v"(ax[0][0]), "+v"(ax[0][1]), "+v"(ax[1][0]), "+v"(ax[1][1]));
    x[0] = __builtin_bit_cast(bf16x8, x0);
    x[1] = __builtin_bit_cast(bf16x8, x1);
}
__device__ __forceinline__ void pin_step(bf16x8 x[2], Upstream<2, false> &u, f32x4 ax[2][2]) {
    u32x4 x0 = __builtin_bit_cast(u32x4, x[0]), x1 = __builtin_bit_cast(u32x4, x[1]);
    asm volatile("" : "+v"(x0), "+v"(x1), "+v"(u.v[0][0]), "+v"(u.v[0][1]), "+v"(u.v[0][2]), "+v"(u.v[0][3]),
                      "+v"(u.v[1][0]), "+v"(u.v[1][1]), "+v"(u.v[1][2]), "+v"(u.v[1][3]), "+v"(u.sg[0]), "+v"(u.sg[1]),
                      "+v"(ax[0][0]), "+v"(ax[0][1]), "+v"(ax[1][0]), "+v"(ax[1][1]));
    x[0] = __builtin_bit_cast(bf16x8, x0);
    x[1] = __builtin_bit_cast(bf16x8, x1);
}

// ------------------------------------------------------------------ backward
// store the two packed halves of a B fragment (elements 0..3 <-> features fa..fa+3, elements 4..7 <-> fb..fb+3 of
// this lane's sample) into row `row` of a [sample][feature] staging image: two 8-byte stores of registers the lane
// already holds
__device__ __forceinline__ void stage_pair(__bf16 *img, int row, int fa, int fb, const bf16x8 &v) {
    const uint4 u = *reinterpret_cast<const uint4 *>(&v);
    *reinterpret_cast<uint2 *>(img + row * RS + fa) = make_uint2(u.x, u.y);
    *reinterpret_cast<uint2 *>(img + row * RS + fb) = make_uint2(u.z, u.w);
}
__device__ __forceinline__ void stage_lo(__bf16 *img, int row, int fa, const bf16x8 &v) {
    const uint4 u = *reinterpret_cast<const uint4 *>(&v);
    *reinterpret_cast<uint2 *>(img + row * RS + fa) = make_uint2(u.x, u.y);
}

// MFMA operand with the FEATURE f0 + (lane & 15) on the lane and the 8 samples 32k + 8(lane >> 4) + 0..7 in the
// registers (A[i = feature][k = sample] and B[k = sample][j = feature] alike), read from a [sample][feature] image.
// ds_read_b64_tr_b16: per group of 16 lanes, lane 4a+b supplies the address of row a, columns 4b..4b+3 of a 4 x 16
// block, and lane i receives column i of the 4 rows; two of them cover the 8 samples.  EXEC is all ones here.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 ld_tr(const __bf16 *img, int k, int f0, int lane) {
    typedef s16x4 __attribute__((address_space(3))) *lds_s16x4_p;
    const int g = lane >> 4, i = lane & 15;
    const __bf16 *p = img + (32 * k + 8 * g + (i >> 2)) * RS + f0 + 4 * (i & 3);
    union {
        struct { s16x4 lo, hi; } h;
        bf16x8 v;
    } u;
    u.h.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)p);
    u.h.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(p + 4 * RS));
    return u.v;
}

// One step of a workgroup: four wavefronts x two 16-sample column tiles each = 128 samples = four k-steps of the
// weight gradients (two workgroups = eight wavefronts per CU; an eight-wave form with one tile each, half the registers
// and four wavefronts per SIMD, measured 65 us against 60: the kernel is short of LDS bandwidth and issue slots, not of
// wavefronts -- DESIGN.md).
constexpr int STEP = 128, KS = STEP / 32;

// the row of a lane's sample (tile t of wave w, column c) inside the step's images
__device__ __forceinline__ int image_row(int w, int t, int c) { return 32 * w + 16 * t + c; }
// the 64 hidden features of the wave's samples -- the packed B fragments v[k-step][tile] -- into an image
__device__ __forceinline__ void stage_hidden(__bf16 *img, int w, int q, int c, const bf16x8 v[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) stage_pair(img, image_row(w, t, c), 32 * s + 4 * q, 32 * s + 16 + 4 * q, v[s][t]);
}

// G[i] += D[:, d0 .. d0+15]^T (x) A[:, a0 + 16 i ..] for i < NC over the step's samples (D, A: [sample][feature]
// images), and B += the column sums of that D (an MFMA against the ones fragment) where `bias` (wave-uniform) says so.
// Per k-step the weights, then the bias; k ascending.
template <int NC>
__device__ __forceinline__ void accumulate(const __bf16 *imgD, int d0, const __bf16 *imgA, int a0, int lane,
                                           const bf16x8 &ones, f32x4 *G, f32x4 &B, bool bias) {
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const bf16x8 dA = ld_tr(imgD, k, d0, lane);   // A[i = row of G][k = sample]
#pragma unroll
        for (int i = 0; i < NC; ++i) G[i] = MFMA32(dA, ld_tr(imgA, k, a0 + 16 * i, lane), G[i]);   // B[k = sample][j = column]
        if (bias) B = MFMA32(dA, ones, B);
    }
}

// The weight-gradient tiles that wave w of the four holds across its steps, and who owns what: rows 16w .. 16w+15 of
// dW2 (four column tiles), of dW1 (two), of db2 and of db1; columns 16w .. 16w+15 of dW3; db3 with wave 0.  Every tile
// has one owner: no cross-wave reduction.
struct WaveGrads {
    f32x4 w2[4], w1[2], b2, b1, w3, b3;
    __device__ __forceinline__ void clear() {
        const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) w2[i] = zero4;
        w1[0] = w1[1] = b2 = b1 = w3 = b3 = zero4;
    }
    // the three accumulations of a step; D / A: the two images as their stage has written them
    __device__ __forceinline__ void add_w3(const __bf16 *dZ3, const __bf16 *H2, int w, int lane, const bf16x8 &ones) {
        accumulate<1>(dZ3, 0, H2, 16 * w, lane, ones, &w3, b3, w == 0);
    }
    __device__ __forceinline__ void add_w2(const __bf16 *dZ2, const __bf16 *H1, int w, int lane, const bf16x8 &ones) {
        accumulate<4>(dZ2, 16 * w, H1, 0, lane, ones, w2, b2, true);
    }
    __device__ __forceinline__ void add_w1(const __bf16 *dZ1, const __bf16 *X, int w, int lane, const bf16x8 &ones) {
        accumulate<2>(dZ1, 16 * w, X, 0, lane, ones, w1, b1, true);
    }
    // the wave's tiles into the workgroup's slab (layout: mlp_shared.h); C/D lane map: register rr of lane (q, c) is
    // row 4q + rr, column c of a tile
    __device__ __forceinline__ void write_slab(float *slab, int w, int q, int c) const {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int o = 16 * w + 4 * q + rr;
#pragma unroll
            for (int i = 0; i < 4; ++i) slab[MLP_SL_W2 + o * MLP_HID + 16 * i + c] = w2[i][rr];
#pragma unroll
            for (int i = 0; i < 2; ++i) slab[MLP_SL_W1 + o * MLP_IN + 16 * i + c] = w1[i][rr];
            if (c == 0) {
                slab[MLP_SL_B2 + o] = b2[rr];
                slab[MLP_SL_B1 + o] = b1[rr];
            }
            slab[MLP_SL_W3 + (4 * q + rr) * MLP_HID + 16 * w + c] = w3[rr];
            if (w == 0 && c == 0) slab[MLP_SL_B3 + 4 * q + rr] = b3[rr];
        }
    }
};

// Gradient through a layer's transposed weights: acc[mt][t] = sum over s < NS of fragment(f0 + NS mt + s) . dz[s][t],
// for MT 16-feature output tiles and both column tiles; every chain starts from zero, s ascending.
template <int MT, int NS>
__device__ __forceinline__ void through_transposed(const __bf16 *frag, int f0, int lane, const bf16x8 dz[NS][2],
                                                   f32x4 acc[MT][2]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[mt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bf16x8 wf = ld_frag(frag, f0 + NS * mt + s, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[mt][t] = MFMA32(wf, dz[s][t], acc[mt][t]);
        }
    }
}
// d(pre-activation) of a hidden layer: the gradient through the NEXT layer's transposed weights, masked by this layer's
// activation `act` being positive and packed as the B fragments of the two k-steps of the layer below
template <int NS>
__device__ __forceinline__ void hidden_grad(const __bf16 *frag, int f0, int lane, const bf16x8 dz[NS][2],
                                            const bf16x8 act[2][2], bf16x8 out[2][2]) {
    f32x4 acc[4][2];
    through_transposed<4, NS>(frag, f0, lane, dz, acc);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) out[s][t] = pack_masked(acc[2 * s][t], acc[2 * s + 1][t], act[s][t]);
}

// dX -> dfeat (level-major f32): the lane holds features 16mt + 4q + 0..3 of its samples m0 + 16t + c, i.e. levels
// 8mt + 2q and 8mt + 2q + 1: one 8-byte store per level, at 32-bit byte offsets (load_x)
__device__ __forceinline__ void store_dfeat(const MlpArgs &a, float *__restrict__ dfeat, int64_t m0, int64_t M, int q, int c,
                                            const f32x4 ax[2][2]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t m = m0 + 16 * t + c;
            if (m < M) {
                const int lv = 8 * mt + 2 * q;
                char *df = reinterpret_cast<char *>(dfeat);
                const uint32_t ls = (uint32_t)a.level_stride, o0 = (((uint32_t)lv) * ls + (uint32_t)m) << 3;
                *reinterpret_cast<float2 *>(df + (size_t)o0) = make_float2(ax[mt][t][0], ax[mt][t][1]);
                *reinterpret_cast<float2 *>(df + (size_t)(o0 + (ls << 3))) = make_float2(ax[mt][t][2], ax[mt][t][3]);
            }
        }
    }
}

// A step: recompute H1, H2 (forward_hidden); then three times "write two images, barrier, accumulate a weight gradient"
// (dW3 from dZ3 and H2, dW2 from dZ2 and H1, dW1 from dZ1 and X) with the data chain dZ3 -> dZ2 -> dZ1 -> dX in
// registers between them.  The kernel body holds what is about ORDER IN TIME -- the step-ahead loads, the barriers, the
// pin, the stamps; the arithmetic is in the parts above.
// FB16 / OUT5: a.feat_bf16 and a.out_dim == 5 at compile time, as in the forward.
template <bool FB16, bool OUT5>
__global__ void __launch_bounds__(256, 2)
k_mlp_backward_bf16(MlpArgs a, const float *__restrict__ sigmas, const float *__restrict__ dsigmas,
                    const float *__restrict__ drgbs, float *__restrict__ dfeat, float *__restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) __bf16 frag[F_ALL * 512];
    __shared__ __attribute__((aligned(16))) __bf16 imgA[STEP * RS];  // [sample][feature]: H2, then H1, then X
    __shared__ __attribute__((aligned(16))) __bf16 imgD[STEP * RS];  // [sample][feature]: dZ3, then dZ2, then dZ1
    __shared__ float sB1[MLP_HID], sB2[MLP_HID];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
    // (the prologue of the forward: fragments and biases requested, then the first step's inputs, then the LDS writes)
    FragmentCopy<F_ALL> fc;
    BiasCopy bc;
    const bool cached = __builtin_expect(a.frag_global != nullptr, 1);   // (a launch without the cache: the cold arm)
    if (cached) fc.request(a.frag_global, tid);
    bc.request(a, tid);
    __builtin_amdgcn_sched_barrier(0);
    const int64_t M = valid_count(a.m_host, a.m_dev);
    // this wave's inputs of the first step; every later step's are requested one step ahead
    const int64_t wofs = 32 * w;
    Upstream<2, OUT5> up;
    load_upstream<2>(up, a, sigmas, dsigmas, drgbs, (int64_t)blockIdx.x * STEP + wofs, M, q, c);
    bf16x8 xB[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) xB[t] = load_x<FB16>(a, clamp_row((int64_t)blockIdx.x * STEP + wofs + 16 * t + c, M), q);
    __builtin_amdgcn_sched_barrier(0);
    if (cached) fc.write(frag, tid);
    else build_fragments(a, frag, F_ALL, tid, 256);
    bc.write(sB1, sB2, tid);
    __syncthreads();
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
    WaveGrads g;
    g.clear();
    {   // (waited for HERE: a load still pending at the loop's entry makes the compiler wait at the top of every step)
        f32x4 none[2][2] = {};
        pin_step(xB, up, none);
    }
    Stamps st;
    st.init();
    for (int64_t tile = blockIdx.x; tile * STEP < M; tile += gridDim.x) {
        const int64_t m0 = tile * STEP + wofs, m1 = m0 + (int64_t)gridDim.x * STEP;
        const Upstream<2, OUT5> up_c = up;
        bf16x8 xC[2], h1B[2][2], h2B[2][2], dz3B[1][2], dz2B[2][2], dz1B[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) xC[t] = xB[t];
        // the next step's upstream gradient and features: requested now, in flight across the whole step, pinned behind
        // its last MFMA
        load_upstream<2>(up, a, sigmas, dsigmas, drgbs, m1, M, q, c);
#pragma unroll
        for (int t = 0; t < 2; ++t) xB[t] = load_x<FB16>(a, clamp_row(m1 + 16 * t + c, M), q);
        // (A step whose upstream gradient is exactly zero -- rays past their termination point, 8 % of the bench's
        // samples -- is not skipped: a branch around the step makes every accumulator live across a merge, ~130 register
        // copies per step, more than the skipped arithmetic is worth.  It flows through and produces its zeros: dfeat = +0,
        // nothing added to any weight gradient.)
#pragma unroll
        for (int t = 0; t < 2; ++t) upstream_fragment<2>(up_c, t, m0 + 16 * t + c < M, q, dz3B[0][t]);
        st.mark(4);   // next step's loads issued, dZ3 fragment
        forward_hidden<2>(frag, sB1, sB2, lane, xC, h1B, h2B, st);   // marks 1, 2
        // ================= stage 1: dW3 += dZ3^T (x) H2^T
        __syncthreads();  // previous step's readers of imgA/imgD are done
        st.mark(5);
        stage_hidden(imgA, w, q, c, h2B);
#pragma unroll
        for (int t = 0; t < 2; ++t) stage_lo(imgD, image_row(w, t, c), 4 * q, dz3B[0][t]);   // outputs 4q .. 4q+3 (columns 0..15; zero beyond out_dim)
        __syncthreads();
        st.mark(6);   // stage-1 images written + barrier
        g.add_w3(imgD, imgA, w, lane, ones);
        st.mark(7);   // dW3
        hidden_grad<1>(frag, F_W3T, lane, dz3B, h2B, dz2B);   // dZ2 = (W3^T dZ3) masked by H2 > 0
        st.mark(8);   // dA2 chain
        // ================= stage 2: dW2 += dZ2^T (x) H1^T
        __syncthreads();
        stage_hidden(imgA, w, q, c, h1B);
        stage_hidden(imgD, w, q, c, dz2B);
        __syncthreads();
        st.mark(9);   // stage-2 barrier + images + barrier
        g.add_w2(imgD, imgA, w, lane, ones);
        st.mark(10);  // dW2
        hidden_grad<2>(frag, F_W2T, lane, dz2B, h1B, dz1B);   // dZ1 = (W2^T dZ2) masked by H1 > 0
        st.mark(11);  // dA1 chain
        // ================= stage 3: dW1 += dZ1^T (x) X^T
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) stage_pair(imgA, image_row(w, t, c), 8 * q, 8 * q + 4, xC[t]);   // input features 8q .. 8q+7
        stage_hidden(imgD, w, q, c, dz1B);
        __syncthreads();
        st.mark(12);  // stage-3 barrier + images + barrier
        g.add_w1(imgD, imgA, w, lane, ones);
        st.mark(13);  // dW1
        f32x4 ax[2][2];
        through_transposed<2, 2>(frag, F_W1T, lane, dz1B, ax);   // dX = W1^T dZ1
        // ---- the one wait of the step: behind its last MFMA, in front of the dfeat stores
        __builtin_amdgcn_sched_barrier(0);
        pin_step(xB, up, ax);
        store_dfeat(a, dfeat, m0, M, q, c, ax);
        st.mark(14);  // dX + stores issued
    }

    st.flush(16);
    g.write_slab(slabs + (int64_t)blockIdx.x * MLP_SLAB, w, q, c);   // one slab per workgroup
}

}  // namespace lnerf

namespace lnerf {

#ifdef LNERF_STAMPS
int mlp_stamps_read(unsigned long long *out32) {
    unsigned long long z[32] = {0};
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_mlp_stamps), sizeof(z)) != hipSuccess) return LNERF_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mlp_stamps), z, sizeof(z)) != hipSuccess) return LNERF_ERR_HIP;
    return LNERF_OK;
}
#endif

int launch_mlp_fragment_maps(int out_dim, int32_t *m1, int32_t *m2, int32_t *m3, hipStream_t stream) {
    if (hipMemsetAsync(m1, 0xFF, (size_t)MLP_HID * MLP_IN * 2 * sizeof(int32_t), stream) != hipSuccess ||
        hipMemsetAsync(m2, 0xFF, (size_t)MLP_HID * MLP_HID * 2 * sizeof(int32_t), stream) != hipSuccess ||
        hipMemsetAsync(m3, 0xFF, (size_t)out_dim * MLP_HID * 2 * sizeof(int32_t), stream) != hipSuccess) {
        set_error("mlp_fragment_maps: hipMemsetAsync failed");
        return LNERF_ERR_HIP;
    }
    hipLaunchKernelGGL(k_mlp_fragment_maps, dim3(16), dim3(256), 0, stream, out_dim, m1, m2, m3);
    LNERF_CHECK_LAUNCH("mlp(fragment maps)");
    return LNERF_OK;
}

int launch_mlp_fragments_bf16(const MlpArgs &a, void *frag_out, bool backward_too, hipStream_t stream) {
    const int n = backward_too ? F_ALL : F_FWD;
    hipLaunchKernelGGL(k_mlp_build_fragments, dim3((unsigned)(n * 2)), dim3(256), 0, stream, a, (__bf16 *)frag_out, n);
    LNERF_CHECK_LAUNCH("mlp(fragments)");
    return LNERF_OK;
}

// (the instantiation of a launch: a.feat_bf16 and a.out_dim == 5 are compile-time arms of both kernels)
template <int WPS>
static auto forward_kernel(const MlpArgs &a) {
    return a.feat_bf16 ? (a.out_dim == 5 ? k_mlp_forward_bf16<WPS, true, true> : k_mlp_forward_bf16<WPS, true, false>)
                       : (a.out_dim == 5 ? k_mlp_forward_bf16<WPS, false, true> : k_mlp_forward_bf16<WPS, false, false>);
}
int launch_mlp_forward_bf16(const MlpArgs &a, float *sigmas, float *rgbs, int blocks, int wps, hipStream_t stream) {
    const auto k = wps >= 3 ? forward_kernel<3>(a) : forward_kernel<2>(a);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, stream, a, sigmas, rgbs);
    LNERF_CHECK_LAUNCH("mlp_forward(bf16)");
    return LNERF_OK;
}

int launch_mlp_backward_bf16(const MlpArgs &a, const float *sigmas, const float *dsigmas, const float *drgbs,
                             float *dfeat, float *slabs, int blocks, hipStream_t stream) {
    const auto k = a.feat_bf16 ? (a.out_dim == 5 ? k_mlp_backward_bf16<true, true> : k_mlp_backward_bf16<true, false>)
                               : (a.out_dim == 5 ? k_mlp_backward_bf16<false, true> : k_mlp_backward_bf16<false, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, stream, a, sigmas, dsigmas, drgbs, dfeat, slabs);
    LNERF_CHECK_LAUNCH("mlp_backward(bf16)");
    return LNERF_OK;
}

}  // namespace lnerf
