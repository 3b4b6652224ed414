// H6, pass 2 of the bucketed scatter (fixed-point LDS sums, fused Adam step of the table, the step's tail), the host-side
// driver of both passes and the C entry points of the scatter.  Gather: grid_gather.hip; pass 1: grid_bin.hip; what
// the passes share: grid_shared.h.
#include "grid_shared.h"

#include <math.h>
#include <mutex>
#include <unordered_map>

namespace lnerf {

// Pass 2.  LDS float atomics run at ~0.5 lane/clk on gfx950 while integer LDS atomics run at the
// plain-store rate (measured: profiles/README.md, "reduce_dbg"), so the tile accumulates in 64-bit
// FIXED POINT: every value is scaled by a power of two chosen from the level's bound of |value|
// (found by pass 1) so that |q| < 2^44 (12-byte records; 2^30 with the 8-byte ones, see fix_scale), which leaves
// 2^19 additions of head-room in an int64.  The scaling is exact, the integer sum is exact and
// order-independent, and the only rounding is the quantisation of each addend to 2^-45 (2^-31) of the
// level's bound plus one final conversion to f32: the result is bitwise reproducible; with the 12-byte
// records it is at least as accurate as an f32 running sum.
// records per slice workgroup of pass 2 (a bucket with fewer records is reduced by one workgroup)
constexpr int REDUCE_SLICE_RECS = 16384;

// Optional fused table update (lnerf_grid_encode_backward_adam): the workgroup of pass 2 that finishes a bucket (its
// only one, or the last slice to arrive) applies the Adam step straight from the fixed-point sum: the gradient of the
// table never travels through HBM (42 -> 26 bytes per table entry and step).
struct FusedUpdate {
    float *p, *m, *v;
    uint16_t *shadow;    // optional bf16 copy of p, refreshed in the same pass
    AdamArgs a;
    uint16_t *grad_out;  // when set: no Adam step -- every row's finished sum is WRITTEN as bf16 here instead (the wire
                         // format of the data-parallel all-reduce: no zero fill, no read-modify-write, no cast)
    uint8_t *live;       // optional MOMENT MAP (null: every row takes the step, nothing is kept): one byte per 16-row group
                         // of a bucket, at (global bucket) * LIVE_GROUPS + (row in bucket >> 4); after every fused step
                         // byte != 0 <=> some m or v word of the group has a non-zero BIT pattern
    int skip;            // with a map: a group whose byte is 0 and whose 16 gradients are all zero is left alone (0: every
                         // group takes the step, the map is only maintained)
};
// A group with m = v = +0 (all-zero bits) and g = +-0 comes out of adam_one as it went in: m' = fma(b1, +0, +-0) = +0,
// v' = +0, p' = p - (lr * 0) * rcp(0 + eps) = p bit for bit (finite lr, eps > 0: the host side checks both), and the bf16
// shadow, which equals bf16(p) already, stays valid.  Such a group needs no load and no store.  -0.0 in a moment counts
// as non-zero: the un-skipped arithmetic would turn it into +0.0.  Nothing crosses workgroups: a bucket's bytes are read
// for use, and written, only by the workgroup that finishes the bucket in that launch.
constexpr int LIVE_SHIFT = 4, LIVE_GROUPS = BK_ROWS >> LIVE_SHIFT;   // 16 rows = 128 B each of p, m, v; 256 bytes per bucket
static_assert(LIVE_GROUPS == 256, "the moment map's layout is part of the C ABI (lnerf_moment_map_bytes)");
__device__ __forceinline__ uint32_t f4_bits(const float4 &x) {
    return __float_as_uint(x.x) | __float_as_uint(x.y) | __float_as_uint(x.z) | __float_as_uint(x.w);
}

// power-of-two scale of a level's fixed-point sums: |value| < 2^(e-126) (e = biased exponent of the level's bound
// found by pass 1) is scaled by 2^(BITS+126-e), which puts every addend below 2^BITS; split so that both factors are
// normal floats.  BITS = 44 (exact 12-byte records: quantum 2^-44 of the bound, 2^19 additions of head-room in an
// int64, conversion through the 64-bit software path) or 30 (8-byte records, whose values carry 17 mantissa bits
// anyway: quantum 2^-30 of the bound, conversion with the native v_cvt_i32_f32, a third of the pass's vector work).
struct FixScale {
    float sc_a, sc_b, un_a, un_b;
};
__device__ __forceinline__ FixScale fix_scale(unsigned int gmax_bits, int bits) {
    int e = (int)(gmax_bits >> 23);
    e = e < 1 ? 1 : (e > 254 ? 254 : e);
    int k = bits + 126 - e;
    k = k > 200 ? 200 : k;
    FixScale f;
    f.sc_a = ldexpf(1.0f, k / 2); f.sc_b = ldexpf(1.0f, k - k / 2);
    f.un_a = ldexpf(1.0f, -(k / 2)); f.un_b = ldexpf(1.0f, -(k - k / 2));
    return f;
}
template <typename REC> struct FixBits { static constexpr int kBits = REC::kPacked ? 30 : 44; };
template <int BITS> __device__ __forceinline__ long long to_fixed(float x);
template <> __device__ __forceinline__ long long to_fixed<44>(float x) { return __float2ll_rn(x); }
template <> __device__ __forceinline__ long long to_fixed<30>(float x) { return (long long)__float2int_rn(x); }  // |x| < 2^30
// slices a bucket with n records is cut into (decided on the device from the actual count; the launch provides
// `smax` workgroups per bucket for the worst case)
__device__ __forceinline__ int active_slices(int n, int smax) {
    int S = (n + REDUCE_SLICE_RECS - 1) / REDUCE_SLICE_RECS;
    return S < 1 ? 1 : (S > smax ? smax : S);
}

constexpr int REDUCE_ROUNDS = 8;   // rounds of record loads in flight per lane (accumulate)
// ---- the step's TAIL: what is left of a single-GPU step besides the scatter.  In a replayed graph a dependent dispatch
// costs ~4.5 us whatever it computes, and three of them sat behind pass 2 for a few microseconds of work: the finishing
// pass of the sliced buckets (pass 2 does it itself now), the sum of the MLP's gradient slabs and the Adam step of the
// small parameters.  One SLAB BLOCK (256 threads) takes 16 parameters of the MLP: it sums their column of the gradient
// slabs in a fixed order (k_mlp_reduce_slabs' arithmetic: deterministic) and applies the Adam step straight from the sum
// -- the weight gradients never exist in memory; updated weights are mirrored into the bf16 weight fragments
// (lnerf_mlp_fragment_maps).  The LAST block of a launch to arrive advances the device step counter and leaves the
// scatter's level maxima zero for the next step (every other block has read both by then, and the arrival is a
// device-scope atomic).  The slab blocks run
//   * as EXTRA workgroups of pass 2 itself (lnerf_grid_encode_backward_adam_tail: four slab blocks per 1024-thread
//     workgroup, in front of the buckets; the step then has no launch behind pass 2 at all), or
//   * as their own launch (lnerf_step_tail: k_step_tail), where other small parameters must be stepped first.
struct SlabAdam {
    const float *slabs;
    int n_slabs, out_dim;
    float *p[6], *m[6], *v[6];        // w1, b1, w2, b2, w3, b3
    const int32_t *map[3];            // optional: fragment positions of w1, w2, w3 (two per weight)
    uint16_t *shadow;                 // the bf16 fragment image the maps point into
    float lr;
};
constexpr int TAIL_P = 16, TAIL_G = 16;   // parameters per block, slab groups (as k_mlp_reduce_slabs)

constexpr int TAIL_SLABS_PER_LANE = MLP_BWD_MAX_BLOCKS / TAIL_G;   // 32: every slab load of a lane in flight at once
constexpr int TAIL_SHARDS = 8;                                     // arrival counters (one 128-byte line each)

// One slab block: `blk` = index of the block of 16 parameters, `lt` = thread inside the block (0..255), `part` = its
// [TAIL_G][TAIL_P] floats of LDS.  `a`: the table's Adam arguments; `step_now` the device step counter when
// a.step_dev is set (requested by the caller with ONE device-scope atomic load per wave -- the last block of the launch
// to arrive rewrites it), `rec` the step's published bias corrections requested with it (adam_shared.h).  Every load
// that depends on nothing is requested first and together: the launch is a handful of dependent round trips per block.  Contains block-wide barriers at named-barrier-free places: call it with all 256
// threads of the block (the 1024-thread form synchronises the whole workgroup, see the caller).
// BATCH: slab values a lane keeps in flight (32 = all of them: the stand-alone launch; 8 inside pass 2, whose 64
// registers per lane must not spill -- the sum takes the slabs in the same order either way).
template <int BATCH, typename SYNC>
__device__ __forceinline__ void slab_block(int blk, int lt, const SlabAdam &sa, AdamArgs a, int32_t step_now,
                                           const AdamConsts &rec, float (*part)[TAIL_P], SYNC sync) {
    static_assert(TAIL_SLABS_PER_LANE % BATCH == 0, "whole batches");
    const int pi = lt & (TAIL_P - 1), sg = lt / TAIL_P;
    const int p = blk * TAIL_P + pi;
    int k = -1, i = 0;   // slab column -> (tensor, element)
    float Pw = 0.f, Mw = 0.f, Vw = 0.f;
    int2 at = make_int2(-1, -1);
    if (p < MLP_SLAB) {
        if (p < MLP_SL_B1) { k = 0; i = p - MLP_SL_W1; }
        else if (p < MLP_SL_W2) { k = 1; i = p - MLP_SL_B1; }
        else if (p < MLP_SL_B2) { k = 2; i = p - MLP_SL_W2; }
        else if (p < MLP_SL_W3) { k = 3; i = p - MLP_SL_B2; }
        else if (p < MLP_SL_B3) { if ((p - MLP_SL_W3) / MLP_HID < sa.out_dim) { k = 4; i = p - MLP_SL_W3; } }
        else { if (p - MLP_SL_B3 < sa.out_dim) { k = 5; i = p - MLP_SL_B3; } }
    }
    float vsl[BATCH];
    auto fetch = [&](int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int bsl = sg + TAIL_G * (j0 + j);
            vsl[j] = (p < MLP_SLAB && bsl < sa.n_slabs) ? sa.slabs[(int64_t)bsl * MLP_SLAB + p] : 0.f;
        }
    };
    fetch(0);
    if (sg == 0 && k >= 0) {
        Pw = sa.p[k][i]; Mw = sa.m[k][i]; Vw = sa.v[k][i];
        if (sa.shadow && !(k & 1)) at = reinterpret_cast<const int2 *>(sa.map[k >> 1])[i];
    }
    if (a.step_dev) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // (the counter has been READ: see the arrival)
        adam_bias_from(a, step_now, rec);
    } else {
        adam_bias(a);
    }
    a.zero_grad = 0;
    float sum = 0.f;   // (k_mlp_reduce_slabs' order: slabs sg, sg + 16, ...)
    for (int j0 = 0;; j0 += BATCH) {
#pragma unroll
        for (int j = 0; j < BATCH; ++j) sum += vsl[j];
        if (j0 + BATCH >= TAIL_SLABS_PER_LANE) break;
        fetch(j0 + BATCH);
    }
    part[sg][pi] = sum;
    sync();
    if (sg == 0 && k >= 0) {
        sum = part[0][pi];
#pragma unroll
        for (int g = 1; g < TAIL_G; ++g) sum += part[g][pi];
        AdamArgs am = a;
        am.lr = sa.lr;
        adam_one(Pw, sum, Mw, Vw, am);
        sa.p[k][i] = Pw; sa.m[k][i] = Mw; sa.v[k][i] = Vw;
        const uint16_t h = f32_to_bf16(Pw);   // weights (k = 0, 2, 4) are mirrored into their two fragment positions
        if (at.x >= 0) sa.shadow[at.x] = h;
        if (at.y >= 0) sa.shadow[at.y] = h;
    }
}

// arrival of a block (call from ONE thread, after the block's reads of the step counter and the level maxima have
// returned), two levels: 8 shard counters (a line each: ~600 arrivals on ONE word queue for 7 us at the memory side), the
// block that completes a shard arrives at the root, the block that completes the root is the last of the launch
__device__ __forceinline__ void tail_arrive(int32_t *arrive, int total, int block, int32_t *tick, int32_t step_now,
                                            const AdamArgs &a, unsigned int *gmax, int do_tick, int clear_gmax) {
    const int sh = block & (TAIL_SHARDS - 1);
    const int mine = (total - sh + TAIL_SHARDS - 1) / TAIL_SHARDS;   // blocks of this shard
    int32_t *cnt = arrive + (1 + sh) * CUR_STRIDE;
    if (__hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mine - 1) {
        __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int shards = total < TAIL_SHARDS ? total : TAIL_SHARDS;
        if (__hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1) {
            __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (do_tick) {
                adam_consts_publish(a, step_now + 1);   // (the next step's bias corrections, for everyone who reads the counter)
                __hip_atomic_store(&tick[0], step_now + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (clear_gmax)
                for (int l = 0; l < LNERF_MAX_LEVELS; ++l)
                    __hip_atomic_store(&gmax[l * CUR_STRIDE], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// what pass 2 does besides the buckets when it closes the step (all zero: nothing)
struct TailJob {
    SlabAdam sa;
    int blocks;            // leading workgroups of the launch that run slab blocks (four each)
    int32_t *tick;         // device step counter pair
    int do_tick, clear_gmax;
    int rev_lo, rev_hi;    // work units [rev_lo, rev_hi) are taken in DESCENDING order (0, 0: none)
};

// The once-per-step streams of the reduce pass, parameter / moment loads and their stores, are non-temporal (the bf16
// shadow the gather reads keeps the default policy; measured with the binning pass's streams: grid_shared.h).  The
// record loads keep the default policy: non-temporal, the gather gained 1.5 us more and the reduce pass lost 8.
__device__ __forceinline__ float4 ld_f4(const float4 *p) {
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_f4(float4 *p, const float4 &x) {
    nt_f4 v = {x.x, x.y, x.z, x.w};
    __builtin_nontemporal_store(v, reinterpret_cast<nt_f4 *>(p));
}

// ---- pass 2 in its parts.  k_scatter_reduce / reduce_bucket read top to bottom: which unit is this workgroup (reduce_unit),
// how is its bucket cut (the slice decision), add the records up (accumulate: sub_batch -> sub_locate -> pipelined rounds
// of add_record), request the rows' state (RowState::prefetch), hand a slice over (merge_slices), finish the rows (one of
// finish_add / finish_wire / RowState::finish / finish_adam, all through unfix).  The workgroup's LDS is at namespace scope
// so that every part names the __shared__ array ITSELF (through a pointer that had lost the LDS address space every
// ds_add_u64 became a flat atomic -- measured 0.211 -> 0.275 ms for the scatter call; tests/test_abi_cpu.py looks at the
// compiled kernels).  s_acc lives from the clear to the finisher (a slab workgroup carves its scratch out of it).
__shared__ long long s_acc[BK_ROWS * 2];                   // [feature][row]: a wave's 64 random rows spread over 32 bank pairs
template <int NW> __shared__ int s_red[NW];                 // the slice decision's record count; merge_slices' arrival value
template <int NW> __shared__ uint32_t s_bmp[NW][128];      // per wave: segment-start bitmap of a sub-batch (4096 records)
template <int NW> __shared__ uint32_t s_soff[NW][64];      // per wave: (chunk slot - flat start) of its non-empty segments
__shared__ uint32_t s_live[BK_ROWS >> 6];                  // the bucket's bytes of the moment map as they were before this step
__shared__ AdamConsts s_consts;                            // the step's published bias corrections, parked across the record loop
// The workspace as both passes and the step's tail see it (by value; built once per call on the host: scatter_ws)
struct ScatterWs {
    unsigned int *gmax;                // level maxima, CUR_STRIDE words apart (raised by pass 1)
    int32_t *items_dev;                // items of the pass 1 that filled the workspace
    int32_t *arrive, *slice_arrive;    // arrival counters: the step's tail (root + 8 shards) / one word per bucket (slices)
    uint32_t *segtab;                  // (first slot, count) per (item, bucket)
    void *recs; long long *partials;   // the items' chunks of Rec8 / Rec12; tiles of the sliced levels
};
struct ReduceOut { float *dtable; FusedUpdate fu; };   // un-fused: dtable += sums / fused: the Adam step or the wire output

// Which unit block x of the launch takes -- the ONE definition.  wg < 0: slab workgroup -1 - wg of a closing launch (they
// sit in front of the buckets); else workgroup wg of the whole table's (level, bucket, slice) units, level-major.
struct ReduceUnit { int wg, l, b, s, Smax, nb; };   // .. level, bucket, slice; slices planned per bucket, buckets of the level
template <bool FUSE>
__device__ __forceinline__ ReduceUnit reduce_unit(int block, int wg_lo, const TailJob &tj, int num_levels, const BucketMeta &bm) {
    ReduceUnit u = {};
    int unit = block - (FUSE ? tj.blocks : 0);
    // heaviest first: the un-merged fine levels carry the most records per bucket; taken in level order they ran LAST
    // and the launch's tail was its heaviest workgroups (the sliced coarse levels keep their place at the front)
    if (unit + wg_lo >= tj.rev_lo && unit + wg_lo < tj.rev_hi) unit = tj.rev_lo + (tj.rev_hi - 1 - (unit + wg_lo)) - wg_lo;
    u.wg = unit < 0 ? unit : unit + wg_lo;
    if (u.wg < 0) return u;
    while (u.l + 1 < num_levels && u.wg >= bm.wgstart[u.l + 1]) ++u.l;
    u.Smax = bm.slices[u.l];
    const int local = u.wg - bm.wgstart[u.l];
    u.b = local / u.Smax;
    u.s = local - u.b * u.Smax;
    u.nb = bm.nb[u.l];
    // Workgroups are dealt round-robin over the 8 XCDs (observed; used for speed only): on an un-sliced level whose
    // bucket count is a multiple of 8 the workgroups of one XCD take CONTIGUOUS buckets.  The segments of neighbouring
    // buckets are neighbours inside every chunk and share 128-byte lines at their seams: read by workgroups of one XCD at
    // about the same time, those lines come from that XCD's L2 the second time instead of twice through the fabric.
    if (u.Smax == 1 && (u.nb & 7) == 0) u.b = (local & 7) * (u.nb >> 3) + (local >> 3);
    return u;
}
// The accumulator's one writer.
template <typename REC> __device__ __forceinline__ void add_record(const REC &r, const FixScale &fs) {
    constexpr int FB = FixBits<REC>::kBits;
    unsigned long long *ua = reinterpret_cast<unsigned long long *>(s_acc);
    const uint32_t a0 = r.row_in_bucket();
    atomicAdd(&ua[a0], (unsigned long long)to_fixed<FB>((r.a() * fs.sc_a) * fs.sc_b));
    atomicAdd(&ua[a0 + BK_ROWS], (unsigned long long)to_fixed<FB>((r.b() * fs.sc_a) * fs.sc_b));
}

// A SUB-BATCH of a window of 64 segment entries: whole segments from lane `a` on with at most REDUCE_SUB records.  Walk the
// CONCATENATION of the segments 64 records per round: lane i of a round takes flat record f0 + i, so every lane carries a
// record whatever the segment sizes are (~32 on a hashed level, thousands on a one-bucket level).  Which segment a lane's
// record is in comes from a BITMAP of the segment starts: bit p = "flat record p is the first of its segment"; lane k
// keeps bits [64 k, 64 k + 64).  A round reads its 64 bits with two scalar readlanes; a lane's segment is the number of
// starts at or below its position (mbcnt), its record's slot one LDS read of that segment's (chunk slot - flat start) plus
// its position: ~10 instructions per round instead of a scalar walk over the 2-3 segments a round spans (~150: the pass
// was bound by instruction issue, not by HBM -- without the Adam phase it took 87 us for 240 MB).  The bitmap covers
// REDUCE_SUB = 4096 records (64 rounds).
constexpr int REDUCE_SUB = 4096;
static_assert(ITEM_RECS <= REDUCE_SUB, "a segment must fit a sub-batch");
struct SubBatch {   // bnd: one past its last lane (> a); Ts: its records; bm_lo / bm_hi: lane k keeps bits [64 k, 64 k + 64)
    int bnd, Ts, bm_lo, bm_hi, nstart;   // of the bitmap; nstart: segment starts before the next round (advanced by sub_locate)
};
// builds the bitmap and the segments' (chunk slot - flat start) of the sub-batch that starts at lane a / flat record a_base
// of the window.  e = the lane's entry, inc = the inclusive sum of the lanes' record counts, slot0 = its item's chunk slot
__device__ __forceinline__ SubBatch sub_batch(uint32_t e, int inc, int a, int a_base, uint32_t slot0, int lane,
                                              uint32_t (&bmp)[128], uint32_t (&soff)[64]) {
    SubBatch sb;
    const int c = (int)(e >> 16);                             // records of the lane's segment
    const bool in = lane >= a && inc - a_base <= REDUCE_SUB;  // (inc is monotone: a contiguous run from lane a)
    sb.bnd = a + (int)__popcll(__ballot(in));
    sb.Ts = __builtin_amdgcn_readlane(inc, sb.bnd - 1) - a_base;
    const bool seg = in && c > 0;
    const int ci = (int)mbcnt(__ballot(seg));                 // index among the non-empty segments
    const int start = inc - c - a_base;                       // flat start inside the sub-batch
    bmp[2 * lane] = 0u; bmp[2 * lane + 1] = 0u;
    if (seg) {
        atomicOr(&bmp[start >> 5], 1u << (start & 31));
        soff[ci] = slot0 + (e & 0xFFFFu) - (uint32_t)start;
    }
    // the lanes exchange data through LDS: a wave's LDS operations execute in order, but the COMPILER reasons
    // per thread -- without the fence pair a lane that set no bit "knows" its words are still zero and never
    // reads them back (measured: the read was sunk into the `if (seg)` block above)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    sb.bm_lo = (int)bmp[2 * lane]; sb.bm_hi = (int)bmp[2 * lane + 1]; sb.nstart = 0;
    return sb;
}
// record index (inside the level's region) of flat record fb + lane of the sub-batch; call with increasing fb
__device__ __forceinline__ uint32_t sub_locate(SubBatch &sb, const uint32_t (&soff)[64], int fb, int lane) {
    const int k = __builtin_amdgcn_readfirstlane(fb >> 6);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(sb.bm_lo, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(sb.bm_hi, k);
    const unsigned long long m1 = (((unsigned long long)hi << 32) | lo) >> 1;
    // starts at positions 1..lane = bits below `lane` of (M >> 1); position 0 = bit 0 of M
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
    const int j = sb.nstart + (int)(lo & 1u) - 1 + below;
    sb.nstart += __popc(lo) + __popc(hi);
    const int f = fb + lane;
    const uint32_t at = soff[j < 0 ? 0 : j] + (uint32_t)f;
    return f < sb.Ts ? at : 0u;                               // (slot 0 exists: the load is unconditional)
}

// The record loop of one wave.  The records of bucket b are the segments (first slot, count) = segtab entry of (item, b),
// one per item of pass 1, inside the items' chunks (entry of item t: tab[t * nb]).  Wave w takes items first = i0 + w,
// first + NW, ... (nmy of them): it reads 64 of its entries with one load (a WINDOW; e_first: the first one's, requested
// by the caller in front of the clear) and walks the concatenation of those segments in sub-batches, each in pipelined
// rounds of 64 records.  Built and measured on the way (profiles/r03_exp_scatter.jsonl): the segment of a lane found by a
// binary search through ds_bpermute (+12 us: the permutes share the LDS pipe with the atomics); one segment per round
// (half-empty waves: three times the instructions, 2-3x the time).
template <int RT, typename REC>
__device__ __forceinline__ void accumulate(const uint32_t *tab, int nb, int first, int nmy, uint32_t e_first, const REC *lrec,
                                           const FixScale &fs, int lane, int wave) {
    constexpr int NW = RT / 64;
    // rounds of loads in flight per lane.  A 12-byte record is three registers: five rounds in flight are what the
    // 64 registers of two resident workgroups leave room for (eight spilled 20-36 bytes per lane to scratch, whose
    // traffic shares the vector-memory queue with the very loads the loop waits for)
    constexpr int U = REC::kPacked ? REDUCE_ROUNDS : (REDUCE_ROUNDS < 5 ? REDUCE_ROUNDS : 5);
    for (int kb = 0; kb < nmy; kb += 64) {                            // (one pass for up to 64 x 16 = 1024 items)
        uint32_t e = e_first;
        if (kb > 0) e = kb + lane < nmy ? tab[(int64_t)(first + NW * (kb + lane)) * nb] : 0u;
        const int inc = wave_inclusive_sum_i((int)(e >> 16));         // the lanes' records, summed
        const int T = __builtin_amdgcn_readlane(inc, 63);
        const uint32_t slot0 = (uint32_t)(first + NW * (kb + lane)) * (uint32_t)ITEM_RECS;
        int a = 0, a_base = 0;                                        // first lane / flat start of the sub-batch (uniform)
        while (a_base < T) {
            SubBatch sb = sub_batch(e, inc, a, a_base, slot0, lane, s_bmp<NW>[wave], s_soff<NW>[wave]);
            // software pipeline over the rounds: U loads are in flight at ALL times -- a round's record is consumed
            // and its register immediately re-armed with the load of the round U ahead (a plain "issue U, consume U"
            // loop drains to zero loads in flight at the end of every batch)
            const int nr = (sb.Ts + 63) >> 6;                         // rounds (uniform)
            REC r[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nr) r[u] = lrec[sub_locate(sb, s_soff<NW>[wave], 64 * u, lane)];
            for (int rb = 0; rb < nr; rb += U) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int rd = rb + u;                            // uniform
                    if (rd < nr) {
                        pin_record(r[u]);                             // (keeps the load outside the predicated block)
                        const REC cur = r[u];
                        if (rd + U < nr) r[u] = lrec[sub_locate(sb, s_soff<NW>[wave], 64 * (rd + U), lane)];
                        if (64 * rd + lane < sb.Ts) add_record(cur, fs);
                    }
                }
            }
            a = sb.bnd;
            a_base += sb.Ts;
        }
    }
}

// Sliced bucket: every slice publishes its EXACT 64-bit partial sums as a tile of `partials`; the slice that arrives LAST
// adds the other tiles to its own sums and finishes the rows like the only workgroup of an unsliced bucket (integer sums:
// neither the slicing nor the arrival order changes a bit of the result).  The heavily loaded coarse buckets come first in
// the grid, so this happens early in the launch, under the other buckets' work -- as its own pass behind the launch it was
// a chain of dependent round trips (~9 us) at the end of the step.  Tiles travel with device-scope (write-through /
// cache-bypassing) accesses: slices run on different XCDs, whose L2s are not coherent for plain stores, and the addresses
// are the same every step.
// ORDERING -- by construction on the ISA, not by C++ memory orders (every atomic below is RELAXED):
//   writer   tile stores = `global_store_dwordx2 ... sc1` (write-through to device scope); `s_waitcnt vmcnt(0)`:
//            every store of the wave ACKNOWLEDGED, i.e. visible at device scope; workgroup barrier: true of all
//            16 waves; then ONE returning `global_atomic_add ... sc0` on the bucket's arrival word.
//   reader   (the arrival that returned S - 1) its value reaches the other waves through LDS + a barrier, so every
//            tile load is issued behind the atomic's return; tile loads = `global_load_dwordx2 ... sc1`: they
//            miss this XCD's non-coherent L2 and see the acknowledged stores.
// A release / acquire pair at agent scope would be correct by the letter and costs a `buffer_wbl2` -- a write-back
// of the XCD's whole L2 -- per workgroup: 106 -> 273 us for this pass.  tests/test_abi_cpu.py
// (test_cross_workgroup_handoffs_are_scoped_accesses) checks the compiled kernel for exactly these instructions
// and for the absence of L2 write-backs / invalidates, so a compiler that chose otherwise fails the CPU suite.
// Returns whether this workgroup arrived last (uniform): then s_acc holds the bucket's whole sums.
template <int RT>
__device__ __forceinline__ bool merge_slices(const ReduceUnit &u, int S, const BucketMeta &bm, const ScatterWs &ws, int tid) {
    unsigned long long *tiles = reinterpret_cast<unsigned long long *>(ws.partials) +
                                ((int64_t)bm.pstart[u.l] + (int64_t)u.b * u.Smax) * (BK_ROWS * 2);
    unsigned long long *pt = tiles + (int64_t)u.s * (BK_ROWS * 2);
    const unsigned long long *ul = reinterpret_cast<const unsigned long long *>(s_acc);
    for (int i = tid; i < BK_ROWS * 2; i += RT) __hip_atomic_store(&pt[i], ul[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of the tile has been written
    __syncthreads();
    int32_t *arr = ws.slice_arrive + bm.bstart[u.l] + u.b;
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == S - 1) __hip_atomic_store(arr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // clean for the next call
        s_red<RT / 64>[0] = old;
    }
    __syncthreads();
    if (s_red<RT / 64>[0] != S - 1) return false;   // uniform: an earlier arrival, somebody else finishes the bucket
    // (one tile at a time, ALL of the lane's elements of it in flight: element by element the sum was a chain of
    // 8 (S - 1) dependent round trips -- 94 us for a six-slice bucket, the longest workgroup of the launch)
    constexpr int NI = BK_ROWS * 2 / RT, NB = NI < 4 ? NI : 4;   // (four 64-bit loads in flight: no spill at 64 registers)
    for (int k0 = 0; k0 < NI; k0 += NB) {
        unsigned long long q[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) q[k] = ul[tid + (k0 + k) * RT];
        for (int s2 = 0; s2 < S; ++s2) {
            if (s2 == u.s) continue;     // uniform
            const unsigned long long *ot = tiles + (int64_t)s2 * (BK_ROWS * 2) + tid + k0 * RT;
            unsigned long long t[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) t[k] = __hip_atomic_load(&ot[k * RT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < NB; ++k) q[k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) s_acc[tid + (k0 + k) * RT] = (long long)q[k];
    }
    __syncthreads();
    return true;
}
__device__ __forceinline__ uint32_t bf16_pair(float x, float y) {
    return (uint32_t)f32_to_bf16(x) | ((uint32_t)f32_to_bf16(y) << 16);
}
// Row r's two sums back from fixed point -- the ONE conversion (scale + whether the bucket had records at all: without,
// s_acc was never cleared and the gradient is zero).
struct UnFix { FixScale fs; bool have; };
__device__ __forceinline__ float2 unfix(const UnFix &t, int r) {
    if (!t.have) return make_float2(0.f, 0.f);
    return make_float2(((float)s_acc[r] * t.fs.un_a) * t.fs.un_b, ((float)s_acc[r + BK_ROWS] * t.fs.un_a) * t.fs.un_b);
}
// The four ways to finish `rows` rows from row R0 of the table; chosen ONCE per workgroup, in reduce_bucket (uniform).
enum Finisher { FIN_ADD, FIN_WIRE, FIN_ADAM_FAST, FIN_ADAM };
// sole owner of these rows in this launch: plain read-modify-write, 8 B per lane
template <int RT> __device__ __forceinline__ void finish_add(const UnFix &t, float *dtable, int64_t R0, int rows, int tid) {
    float2 *dst = reinterpret_cast<float2 *>(dtable) + R0;
    for (int r = tid; r < rows; r += RT) {
        const float2 d = dst[r], g = unfix(t, r);
        dst[r] = make_float2(d.x + g.x, d.y + g.y);
    }
}
// gradient output in the wire format: one bf16 pair per row, WRITTEN (stale content before; zeros without records)
template <int RT> __device__ __forceinline__ void finish_wire(const UnFix &t, uint16_t *grad_out, int64_t R0, int rows, int tid) {
    uint32_t *go = reinterpret_cast<uint32_t *>(grad_out) + R0;
    for (int r = tid; r < rows; r += RT) {
        const float2 g = unfix(t, r);
        go[r] = bf16_pair(g.x, g.y);
    }
}
// The moment map's rule, the ONE definition both Adam finishers use.  PER consecutive lanes of a wave hold a group (8: a
// row pair each, 16: a row each); call both parts with the whole wave.
template <int PER> __device__ __forceinline__ uint32_t group_slice(unsigned long long ballot, int lane) {
    return (uint32_t)(ballot >> (lane & (64 - PER))) & ((1u << PER) - 1u);
}
// a group's byte as it was before this step (s_live: filled by reduce_bucket in front of a barrier; zeros without a map)
__device__ __forceinline__ uint32_t old_byte(int group) { return reinterpret_cast<const uint8_t *>(s_live)[group]; }
struct GroupStep { bool step, first; };   // the group takes the step / as a FIRST TOUCH: m = v = +0 are known, p is not loaded yet
template <int PER>
__device__ __forceinline__ GroupStep group_step(const FusedUpdate &fu, uint32_t old_byte, bool g_nonzero, int lane) {
    const bool live = !fu.live || !fu.skip || old_byte != 0u;
    const bool nz = group_slice<PER>(__ballot(g_nonzero), lane) != 0u;
    return {live || nz, !live};
}
// the group's new byte = "any non-zero bit in its new m | v" (it falls back to 0 when the moments have decayed to +0); one
// lane per group writes it, and only when it changes
template <int PER>
__device__ __forceinline__ void group_mark(uint8_t *byte_at, uint32_t old_byte, bool stepped, uint32_t mv_bits, int lane) {
    const uint32_t now = group_slice<PER>(__ballot(stepped && mv_bits != 0u), lane) != 0u ? 1u : 0u;
    if (byte_at && stepped && (lane & (PER - 1)) == 0 && now != (old_byte != 0u ? 1u : 0u)) *byte_at = (uint8_t)now;
}
// the Adam step row by row (a partial bucket, an odd first row, the last arriver of a sliced bucket); live_at: the
// bucket's first byte of the moment map
template <int RT>
__device__ __forceinline__ void finish_adam(const UnFix &t, const FusedUpdate &fu, const AdamArgs &a, int64_t R0, int rows,
                                            int tid, int64_t live_at) {
    float2 *p2 = reinterpret_cast<float2 *>(fu.p) + R0, *m2 = reinterpret_cast<float2 *>(fu.m) + R0;
    float2 *v2 = reinterpret_cast<float2 *>(fu.v) + R0;
    uint32_t *sh = fu.shadow ? reinterpret_cast<uint32_t *>(fu.shadow) + R0 : nullptr;
    uint8_t *lv = fu.live ? fu.live + live_at : nullptr;
    for (int r0 = 0; r0 < rows; r0 += RT) {   // (uniform trip count: the group rule votes across the wave)
        const int r = r0 + tid;
        const bool in = r < rows;
        const uint32_t old = in ? old_byte(r >> LIVE_SHIFT) : 0u;
        const float2 g0 = in ? unfix(t, r) : make_float2(0.f, 0.f);
        const GroupStep gs = group_step<16>(fu, old, g0.x != 0.f || g0.y != 0.f, tid & 63);
        const bool step = in && gs.step;
        uint32_t mv = 0u;
        if (step) {
            float2 Pr = p2[r], Mr = make_float2(0.f, 0.f), Vr = make_float2(0.f, 0.f), g = g0;
            if (!gs.first) { Mr = m2[r]; Vr = v2[r]; }
            adam_one(Pr.x, g.x, Mr.x, Vr.x, a);
            adam_one(Pr.y, g.y, Mr.y, Vr.y, a);
            p2[r] = Pr; m2[r] = Mr; v2[r] = Vr;
            if (sh) sh[r] = bf16_pair(Pr.x, Pr.y);
            mv = __float_as_uint(Mr.x) | __float_as_uint(Mr.y) | __float_as_uint(Vr.x) | __float_as_uint(Vr.y);
        }
        group_mark<16>(lv ? lv + (r >> LIVE_SHIFT) : nullptr, old, step, mv, tid & 63);
    }
}
// FIN_ADAM_FAST: the lane's row pairs q = tid + j RT, their parameters and moments in registers between prefetch() and
// finish().  The prefetch is issued BEHIND the record loop and IN FRONT of the barrier that ends it: a wave that is done
// with its records waits for the slowest wave anyway, and the loads travel meanwhile.  (Requested ahead of the record
// stream they were measured 35 us slower: the records queue behind them.)
template <int RT> struct RowState {
    static constexpr int NQ = (BK_ROWS / 2 + RT - 1) / RT;  // row pairs per lane
    float4 P[NQ], Mv[NQ], V[NQ];
    float4 *p4, *m4, *v4;
    __device__ __forceinline__ RowState(const FusedUpdate &fu, int64_t R0)
        : p4(reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(fu.p) + R0)),
          m4(reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(fu.m) + R0)),
          v4(reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(fu.v) + R0)) {}
    __device__ __forceinline__ void prefetch(const FusedUpdate &fu, int tid) {
        const bool all = !fu.live || !fu.skip;   // uniform
#pragma unroll
        for (int j = 0; j < NQ; ++j) {  // all of the lane's loads: six 16-byte loads in flight behind the barrier
            const int q = tid + j * RT;
            if (all || old_byte(q >> (LIVE_SHIFT - 1)) != 0u) {   // (a clean group: no load; a first touch loads p in finish())
                P[j] = ld_f4(p4 + q); Mv[j] = ld_f4(m4 + q); V[j] = ld_f4(v4 + q);
            }
        }
    }
    __device__ __forceinline__ void finish(const UnFix &t, const FusedUpdate &fu, const AdamArgs &a, int64_t R0, int tid,
                                           int64_t live_at) {
        uint2 *sh2 = fu.shadow ? reinterpret_cast<uint2 *>(reinterpret_cast<uint32_t *>(fu.shadow) + R0) : nullptr;
        uint8_t *lv = fu.live ? fu.live + live_at : nullptr;
        const int lane = tid & 63;
        // every row pair's arithmetic first, every store behind it: with the stores of one pair in front of the next
        // pair's group vote, the vote's branch made the compiler wait for those stores (s_waitcnt vmcnt(0): +10 us)
        bool step[NQ];
        uint32_t mv[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = tid + j * RT;
            float2 g0 = unfix(t, 2 * q), g1 = unfix(t, 2 * q + 1);
            const GroupStep gs = group_step<8>(fu, old_byte(q >> (LIVE_SHIFT - 1)),
                                               g0.x != 0.f || g0.y != 0.f || g1.x != 0.f || g1.y != 0.f, lane);
            step[j] = gs.step;
            mv[j] = 0u;
            if (gs.step) {
                if (gs.first) {   // (about once per group in a whole training run: a late dependent load is acceptable)
                    P[j] = ld_f4(p4 + q);
                    Mv[j] = make_float4(0.f, 0.f, 0.f, 0.f); V[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                adam_one(P[j].x, g0.x, Mv[j].x, V[j].x, a);
                adam_one(P[j].y, g0.y, Mv[j].y, V[j].y, a);
                adam_one(P[j].z, g1.x, Mv[j].z, V[j].z, a);
                adam_one(P[j].w, g1.y, Mv[j].w, V[j].w, a);
                mv[j] = f4_bits(Mv[j]) | f4_bits(V[j]);
            }
        }
        // (every load above has been consumed: free at run time.  Said through the builtin, so that the compiler's own
        // bookkeeping starts clean here -- it otherwise guards each store below against the loads of the branches above
        // with a vmcnt(2), which at run time waits for the stores in front of it)
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = tid + j * RT;
            if (step[j]) {
                st_f4(p4 + q, P[j]); st_f4(m4 + q, Mv[j]); st_f4(v4 + q, V[j]);
                if (sh2) sh2[q] = make_uint2(bf16_pair(P[j].x, P[j].y), bf16_pair(P[j].z, P[j].w));
            }
            group_mark<8>(lv ? lv + (q >> 3) : nullptr, old_byte(q >> (LIVE_SHIFT - 1)), step[j], mv[j], lane);
        }
    }
};

// One (level, bucket, slice) unit, the parts in order.  A return leaves through the kernel's end.
template <int RT, typename REC, bool FUSE>
__device__ __forceinline__ void reduce_bucket(const ReduceUnit &u, const GridMeta &meta, const BucketMeta &bm, const ScatterWs &ws,
                                              const ReduceOut &out, int32_t step_now, const AdamConsts &rec, bool have_step) {
    constexpr int NW = RT / 64;
    const int l = u.l, nb = u.nb, tid = threadIdx.x, lane = tid & 63;
    // (uniform, and known to be: everything derived from it -- the wave's items, their chunk addresses -- stays in
    // scalar registers; as a function of threadIdx it was per-lane 64-bit address arithmetic and spilled)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int I = *ws.items_dev;                       // items of the pass 1 that filled the workspace
    I = I < bm.n_items ? I : bm.n_items;
    const uint32_t *tab = ws.segtab + (int64_t)bm.bstart[l] * bm.n_items + u.b;   // entry of item t: tab[t * nb]
    // The slice decision -- the ONE place that defines `direct`.  A level whose buckets MAY be sliced (Smax > 1, uniform
    // per level) counts the bucket's records first: S slices are active, slice s takes items [i0, i1).
    int S = 1, i0 = 0, i1 = I;
    if (u.Smax > 1) {
        int cnt = 0;
        for (int t = tid; t < I; t += RT) cnt += (int)(tab[(int64_t)t * nb] >> 16);
        cnt = wave_inclusive_sum_i(cnt);
        if (lane == 63) s_red<NW>[wave] = cnt;
        __syncthreads();
        int n = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) n += s_red<NW>[k];
        S = active_slices(n, u.Smax);
        if (u.s >= S) return;    // uniform per workgroup
        i0 = (int)(((long long)I * u.s) / S);
        i1 = (int)(((long long)I * (u.s + 1)) / S);
    }
    const bool direct = S == 1;        // this workgroup sums the whole bucket: it finishes the rows itself
    // uniform.  (An active slice always has items: S > 1 means more than REDUCE_SLICE_RECS >= ITEM_RECS records, i.e.
    // at least S items.)  Whoever finishes a bucket -- its only workgroup, or the last slice to arrive -- owes a fused
    // bucket without records the Adam step (g = 0) and a wire bucket its zeros.
    const bool have = i1 > i0 || !direct;
    if (!have && !FUSE) return;
    // the bucket's 256 bytes of the moment map, word i on lane i (every wave of a bucket without records, else the first):
    // requested here, put into s_live in front of the workgroup's next barrier -- no register is held across the record loop
    const int64_t live_at = (int64_t)(bm.bstart[l] + u.b) * LIVE_GROUPS;
    uint32_t live_words = 0u;
    if (FUSE && out.fu.live && (wave == 0 || !have)) live_words = reinterpret_cast<const uint32_t *>(out.fu.live + live_at)[lane];
    // a bucket without records whose groups are all clean has no work (every wave sees all 256 bytes: uniform)
    if (FUSE && !have && out.fu.live && out.fu.skip && __ballot(live_words != 0u) == 0ull) return;
    // from the bound of |value| of the LEVEL (found by pass 1).  One device-scope atomic load: the last workgroup of a
    // closing launch to arrive ZEROES the maxima (tail_arrive) -- ordered behind this read by the arrival, but a plain
    // load the compiler might re-issue later would be a data race on paper
    const UnFix t = {fix_scale(__hip_atomic_load(&ws.gmax[l * CUR_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                               REC::kPacked ? FixBits<REC>::kBits : bm.fix_bits), have};
    RED_STAMP_INIT();
    const int row0 = u.b << BK_SHIFT;
    int rows = meta.offsets[l + 1] - meta.offsets[l] - row0;
    rows = rows < BK_ROWS ? rows : BK_ROWS;
    const int64_t R0 = (int64_t)meta.offsets[l] + row0;
    // FIN_ADAM_FAST, the usual fused case: a full bucket with an even first row, summed by this workgroup alone
    const bool pairs = direct && ((R0 | rows) & 1) == 0 && rows == BK_ROWS && (BK_ROWS / 2) % RT == 0;
    const Finisher fin = !FUSE ? FIN_ADD : out.fu.grad_out ? FIN_WIRE : pairs ? FIN_ADAM_FAST : FIN_ADAM;
    RowState<RT> rs(out.fu, R0);
    if (have) {
        const int first = i0 + wave;                                  // this wave's items: first, first + NW, ...
        const int nmy = first < i1 ? (i1 - first + NW - 1) / NW : 0;
        // (the first 64 segment entries are requested before the accumulators are cleared: one round trip hidden)
        uint32_t e_first = 0u;
        if (lane < nmy) e_first = tab[(int64_t)(first + NW * lane) * nb];
        for (int i = tid; i < BK_ROWS * 2; i += RT) s_acc[i] = 0ll;
        if (FUSE && wave == 0) s_live[lane] = live_words;
        if (FUSE && have_step && tid == 0) s_consts = rec;   // (parked: no vector register is held across the record loop)
        __syncthreads();
        step_now = __builtin_amdgcn_readfirstlane(step_now);   // (returned by now: into a scalar register for the loop)
        RED_STAMP(10);
        accumulate<RT, REC>(tab, nb, first, nmy, e_first, static_cast<const REC *>(ws.recs) + (int64_t)l * bm.n_items * ITEM_RECS,
                            t.fs, lane, wave);
        RED_STAMP(11);
        if (fin == FIN_ADAM_FAST) rs.prefetch(out.fu, tid);
        __syncthreads();
        RED_STAMP(12);
    } else {   // (FUSE: no records, but live groups whose moments decay)
        if (wave == 0) s_live[lane] = live_words;
        if (have_step && tid == 0) s_consts = rec;
        __syncthreads();
        if (fin == FIN_ADAM_FAST) rs.prefetch(out.fu, tid);
    }
    if (!direct && !merge_slices<RT>(u, S, bm, ws, tid)) return;
    AdamArgs a = out.fu.a;   // (once, in front of the choice; have_step: the closing launch, see the kernel)
    if (FUSE && have_step) adam_bias_from(a, __builtin_amdgcn_readfirstlane(step_now), s_consts);
    else if (FUSE) adam_bias(a);
    a.zero_grad = 0;
    switch (fin) {
    case FIN_ADD: finish_add<RT>(t, out.dtable, R0, rows, tid); break;
    case FIN_WIRE: finish_wire<RT>(t, out.fu.grad_out, R0, rows, tid); break;
    case FIN_ADAM: finish_adam<RT>(t, out.fu, a, R0, rows, tid, live_at); break;
    case FIN_ADAM_FAST: rs.finish(t, out.fu, a, R0, tid, live_at); RED_STAMP(13); RED_STAMP_FLUSH(); break;
    }
}

// One workgroup per (bucket, slice) unit.  (PERSISTENT workgroups striding over the units were built and measured: the
// loop keeps the three kernel-argument structs live across iterations, 77 VGPRs spill at the 64 the two-workgroups-per-CU
// occupancy allows, and the pass went from 0.211 to 0.27 ms per scatter call: profiles/r03_exp_scatter.jsonl.)
constexpr int FUSED_RT = 1024;   // threads per workgroup of the fused pass
template <int RT, typename REC, bool FUSE>
__global__ void __launch_bounds__(RT, RT / 128)
k_scatter_reduce(GridMeta meta, BucketMeta bm, ScatterWs ws, ReduceOut out, int wg_lo, TailJob tj) {
    // (closing the step: the counter is read ONCE per wave, with a device-scope atomic load, before anything else --
    // the last workgroup of the launch to arrive rewrites it)
#ifdef LNERF_STAMPS
    const unsigned long long wg_t0 = wall_clock64();
#endif
    int32_t step_now = 0;
    const bool closing = FUSE && (tj.do_tick || tj.clear_gmax || tj.blocks > 0);
    // (requested here, consumed behind the workgroup's first barrier: no stall in front of the record stream)
    if (closing && out.fu.a.step_dev) step_now = __hip_atomic_load(out.fu.a.step_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const ReduceUnit u = reduce_unit<FUSE>((int)blockIdx.x, wg_lo, tj, meta.num_levels, bm);
    // (with it the step's published bias corrections, where a record is bound to the counter: adam_shared.h.  By the
    // waves that use them: every wave of a slab workgroup, the first wave of a bucket's, which parks them in LDS)
    const bool rec_here = closing && out.fu.a.step_dev && (u.wg < 0 || __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) == 0);
    const AdamConsts rec = adam_consts_request(rec_here ? out.fu.a.consts : nullptr);
    if (u.wg < 0) {
        // a SLAB workgroup of the closing launch: RT / 256 slab blocks, their 1 KiB of LDS each carved out of the tile
        const int sub = (int)threadIdx.x >> 8, lt = (int)threadIdx.x & 255;
        float (*part)[TAIL_P] = reinterpret_cast<float (*)[TAIL_P]>(s_acc) + sub * TAIL_G;
        slab_block<8>((-1 - u.wg) * (RT / 256) + sub, lt, tj.sa, out.fu.a, step_now, rec, part, [] { __syncthreads(); });
    } else {
        reduce_bucket<RT, REC, FUSE>(u, meta, bm, ws, out, step_now, rec, closing && out.fu.a.step_dev != nullptr);
    }
#ifdef LNERF_STAMPS
    if (blockIdx.x < 4096) {   // (exit = the LAST wave's, with its stores acknowledged: the slot is free after that)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((threadIdx.x & 63) == 0) atomicMax(&g_wg_log[4 * blockIdx.x + 1], (unsigned long long)wall_clock64());
        if (threadIdx.x == 0) {
            unsigned int hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_wg_log[4 * blockIdx.x] = wg_t0;
            g_wg_log[4 * blockIdx.x + 2] = ((unsigned long long)xcc << 32) | hw;
            g_wg_log[4 * blockIdx.x + 3] = (unsigned long long)(unsigned int)(u.wg < 0 ? u.wg : u.wg - wg_lo);
        }
    }
#endif
    if (closing && (tj.do_tick || tj.clear_gmax) && threadIdx.x == 0)
        // (this wave is done.  The workgroup's other waves requested the counter as their first instruction and the
        // level maximum in front of the record loop; a workgroup's barriers wait for a wave's outstanding loads, and
        // a workgroup that leaves before its first barrier has not used either value)
        tail_arrive(ws.arrive, (int)gridDim.x, (int)blockIdx.x, tj.tick, step_now, out.fu.a, ws.gmax, tj.do_tick, tj.clear_gmax);
}

// the slab blocks + the closing arrival as a launch of their own (lnerf_step_tail)
__global__ void __launch_bounds__(256)
k_step_tail(unsigned int *__restrict__ gmax, AdamArgs a, SlabAdam sa, int32_t *__restrict__ tick,
            int32_t *__restrict__ arrive, int do_tick, int clear_gmax) {
    int32_t step_now = 0;
    if (a.step_dev) step_now = __hip_atomic_load(a.step_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const AdamConsts rec = adam_consts_request(a.step_dev ? a.consts : nullptr);
    __shared__ float part[TAIL_G][TAIL_P];
    if (sa.slabs) slab_block<TAIL_SLABS_PER_LANE>((int)blockIdx.x, (int)threadIdx.x, sa, a, step_now, rec, part, [] { __syncthreads(); });
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (do_tick || clear_gmax) {
        __syncthreads();
        if (threadIdx.x == 0) tail_arrive(arrive, (int)gridDim.x, (int)blockIdx.x, tick, step_now, a, gmax, do_tick, clear_gmax);
    }
}

// The moment map from the moments themselves (lnerf_moment_map_build): one lane per row of every bucket, 16 lanes per
// byte, every byte of the map written (rows past a level's end count as zero).
struct MapLevels { int num_levels, offsets[LNERF_MAX_LEVELS + 1], bstart[LNERF_MAX_LEVELS + 1]; };
__global__ void __launch_bounds__(256)
k_moment_map(const float2 *__restrict__ m, const float2 *__restrict__ v, MapLevels lv, uint8_t *__restrict__ map) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;   // (buckets x BK_ROWS threads: whole blocks)
    const int gb = (int)(t >> BK_SHIFT), rb = (int)(t & (BK_ROWS - 1));
    int l = 0;
    while (l + 1 < lv.num_levels && gb >= lv.bstart[l + 1]) ++l;
    const int64_t row = (int64_t)lv.offsets[l] + ((int64_t)(gb - lv.bstart[l]) << BK_SHIFT) + rb;
    uint32_t bits = 0u;
    if (row < (int64_t)lv.offsets[l + 1]) {
        const float2 a = m[row], b = v[row];
        bits = __float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(b.x) | __float_as_uint(b.y);
    }
    const uint32_t any = group_slice<16>(__ballot(bits != 0u), (int)threadIdx.x & 63);
    if ((threadIdx.x & 15) == 0) map[t >> LIVE_SHIFT] = any ? (uint8_t)1 : (uint8_t)0;
}

// Moment maps bound to a table's optimiser state (lnerf_moment_map_bind), by the exp_avg pointer: the fused entry points
// look theirs up when they fill FusedUpdate.  No binding: no map, every group takes the step.
struct BoundMap { uint8_t *map; size_t bytes; };
static std::mutex g_maps_mutex;
static std::unordered_map<const void *, BoundMap> g_maps;
// with a bound map: leave groups with zero moments and zero gradient alone (0: the map is maintained, every group steps)
int g_adam_skip = 1;
// "adam_skip" and "adam_consts" switch between two forms of the SAME result; they are not path-selecting keys
// ("adam_consts": bound records of published bias corrections are used, lnerf_adam_constants_bind -- optim.hip)
static bool set_form_switch(const char *key, int value) {
    if (strcmp(key, "adam_skip") == 0) g_adam_skip = value ? 1 : 0;
    else if (strcmp(key, "adam_consts") == 0) g_adam_consts = value ? 1 : 0;
    else return false;
    return true;
}

extern int g_mlp_fwd_blocks, g_mlp_fwd_wps, g_mlp_bwd_blocks;  // mlp.hip

// levels up to this resolution merge per-wave runs before binning (tunable: lnerf_set_tuning)
int g_compact_max_res = 512;
// gather: fetch x-adjacent vertices with one load where they are adjacent rows (2: also aligned groups of four rows)
int g_gather_pairs = 2;
// gather: levels with resolution <= this fetch a cell's vertices once per run of lanes in that cell (0 = off)
int g_gather_dedup_res = 512;
// gather: bytes of (unused) dynamic LDS per workgroup -- an EXPERIMENT knob that caps the resident wavefronts (160 KiB per CU:
// 53 KiB leaves three 256-thread workgroups = three waves per SIMD): "what would the gather cost at the occupancy of a
// kernel fused with the MLP forward?" 
int g_gather_lds_pad = 0;
// persistent workgroups of the binning pass per CU (3 fit its 44 KiB of LDS with the 8-byte records)
int g_bin_per_cu = 3;
// persistent workgroups of the binning pass (0 = 256 CUs x g_bin_per_cu); rounded down to a multiple of the level count
int g_bin_wgs = 0;
// drop contributions that are exactly zero (samples behind a ray's termination point)
int g_skip_zero = 1;
// threads per workgroup of the reduce pass (512 or 1024; two 64 KiB workgroups fit a CU either way)
int g_reduce_threads = 1024;
// level groups of the whole-frame scatter: bin(group) -> reduce(group) per group (1 = bin everything, then reduce)
int g_scatter_groups = 1;

// workspace: [header: level maxima | item count | arrival counters | unused] [segment table] [record chunks] [partial tiles]
// (the header's last region, one word per bucket from HDR_BUCKETN_OFF on, is unused: it can go with the next ABI change)
static_assert(BK_MAX_PER_LEVEL == 256 && HDR_BUCKETN_OFF <= LNERF_SCATTER_ZERO_HEAD_BYTES,
              "the counters of the header must lie inside the head a caller zeroes");
static size_t header_bytes(int n_buckets) {
    return (HDR_BUCKETN_OFF + (size_t)n_buckets * sizeof(int32_t) + 4095) / 4096 * 4096;
}

struct ScatterPlan {
    int buckets, wgs;   // buckets / pass-2 workgroups over all levels
    int ptiles;         // partial-sum tiles (sliced levels: buckets x slices)
    size_t header_bytes, seg_bytes, rec_bytes, partial_bytes;
    size_t total() const { return header_bytes + seg_bytes + rec_bytes + partial_bytes; }
};

static int fill_bucket_meta(const GridMeta &meta, int64_t m_host, BucketMeta &bm, ScatterPlan &plan) {
    int total_buckets = 0, total_wgs = 0, total_ptiles = 0;
    const int64_t n_items = m_host > 0 ? div_up(m_host, (int64_t)ITEM_SAMPLES) : 1;
    if (n_items >= (1 << 19)) return -1;   // (pass 2 addresses a level's records with 32-bit record indices)
    for (int l = 0; l < meta.num_levels; ++l) {
        const int64_t hsize = meta.offsets[l + 1] - meta.offsets[l];
        const int nb = (int)div_up(hsize, BK_ROWS);
        if (nb > BK_MAX_PER_LEVEL) return -1;
        const int64_t per_bucket = div_up(8 * m_host, nb);   // worst case under a uniform spread
        int slices = (int)((per_bucket + 65535) / 65536);    // <= ~64 Ki records per pass-2 workgroup
        if (slices < 1) slices = 1;
        if (slices > 64) slices = 64;
        bm.nb[l] = nb;
        bm.bstart[l] = total_buckets;
        bm.slices[l] = slices;
        bm.compact[l] = meta.res[l] <= g_compact_max_res ? 1 : 0;
        bm.wgstart[l] = total_wgs;
        bm.pstart[l] = slices > 1 ? total_ptiles : -1;
        if (slices > 1) total_ptiles += nb * slices;
        total_buckets += nb;
        total_wgs += nb * slices;
    }
    bm.bstart[meta.num_levels] = total_buckets;
    bm.wgstart[meta.num_levels] = total_wgs;
    bm.n_items = (int)n_items;
    // 12-byte records, exact sums: the addends of a bucket sum to at most m_host x the level's bound (the weights of a
    // sample's 8 vertices sum to 1; a merged run's bound is 64 x the largest |g| and it stands for up to 64 samples), so
    // bits + ceil(log2(m_host)) <= 62 keeps every int64 sum exact whatever the input: 44 bits up to 2^18 samples, 42 at
    // the bench's 640 Ki, 39 with eight views in a batch (the 8-byte records use 30 bits: exact below 2^32 samples)
    int lg = 1;
    while (((int64_t)1 << lg) < m_host) ++lg;
    bm.fix_bits = 62 - lg < 44 ? 62 - lg : 44;
    plan.buckets = total_buckets;
    plan.wgs = total_wgs;
    plan.ptiles = total_ptiles;
    plan.header_bytes = header_bytes(total_buckets);
    plan.seg_bytes = ((size_t)total_buckets * (size_t)n_items * sizeof(uint32_t) + 4095) / 4096 * 4096;
    // one chunk of ITEM_RECS slots per (level, item): exactly what the item's samples can emit (sized for the 12-byte
    // records; the packed ones use two thirds of it)
    plan.rec_bytes = (size_t)meta.num_levels * (size_t)n_items * ITEM_RECS * sizeof(Rec12);
    plan.partial_bytes = (size_t)total_ptiles * BK_ROWS * 2 * sizeof(long long);
    return 0;
}

// the plan of a level table known by its offsets alone (what the two size queries are given); false: not plannable
static bool plan_from_offsets(int num_levels, const int32_t *offsets_host, int64_t m_host, ScatterPlan &plan) {
    if (num_levels < 1 || num_levels > LNERF_MAX_LEVELS || !offsets_host || m_host < 0) return false;
    GridMeta meta = {};
    meta.num_levels = num_levels;
    for (int l = 0; l <= num_levels; ++l) meta.offsets[l] = offsets_host[l];
    BucketMeta bm;
    return fill_bucket_meta(meta, m_host, bm, plan) == 0;
}

// where the regions of a workspace are
static ScatterWs scatter_ws(void *workspace, const ScatterPlan &plan) {
    char *hdr = (char *)workspace, *seg = hdr + plan.header_bytes, *rec = seg + plan.seg_bytes;
    return {(unsigned int *)hdr, (int32_t *)(hdr + HDR_ITEMS_OFF), (int32_t *)(hdr + HDR_ARRIVE_OFF),
            (int32_t *)(hdr + HDR_SLICE_ARRIVE_OFF), (uint32_t *)seg, rec, (long long *)(rec + plan.rec_bytes)};
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

int lnerf_set_tuning(const char *key, int value) {
    LNERF_REQUIRE(key, "set_tuning: null key");
    if (set_form_switch(key, value)) return LNERF_OK;
    if (strcmp(key, "scatter_compact_max_res") == 0) {
        LNERF_REQUIRE(value >= 0, "set_tuning: scatter_compact_max_res must be >= 0");
        g_compact_max_res = value;
        return LNERF_OK;
    }
    if (strcmp(key, "scatter_bin_wgs") == 0) {
        LNERF_REQUIRE(value >= 0 && value <= 65535, "set_tuning: scatter_bin_wgs out of range");
        g_bin_wgs = value;
        return LNERF_OK;
    }
    if (strcmp(key, "scatter_bin_per_cu") == 0) {
        LNERF_REQUIRE(value >= 1 && value <= 4, "set_tuning: scatter_bin_per_cu must be in 1 .. 4");
        g_bin_per_cu = value;
        return LNERF_OK;
    }
    if (strcmp(key, "gather_dedup_max_res") == 0) {
        LNERF_REQUIRE(value >= 0, "set_tuning: gather_dedup_max_res must be >= 0");
        g_gather_dedup_res = value;
        return LNERF_OK;
    }
    if (strcmp(key, "gather_lds_pad") == 0) {
        LNERF_REQUIRE(value >= 0 && value <= 65536, "set_tuning: gather_lds_pad must be in [0, 65536] bytes");
        g_gather_lds_pad = value;
        return LNERF_OK;
    }
    if (strcmp(key, "gather_pair_loads") == 0) {
        LNERF_REQUIRE(value >= 0 && value <= 2, "set_tuning: gather_pair_loads must be 0, 1 or 2");
        g_gather_pairs = value;
        return LNERF_OK;
    }
    if (strcmp(key, "mlp_bwd_blocks") == 0) {
        LNERF_REQUIRE(value >= 1 && value <= 512, "set_tuning: mlp_bwd_blocks must be in 1 .. 512");
        g_mlp_bwd_blocks = value;
        return LNERF_OK;
    }
    if (strcmp(key, "mlp_fwd_wps") == 0) {
        LNERF_REQUIRE(value == 2 || value == 3, "set_tuning: mlp_fwd_wps must be 2 or 3");
        g_mlp_fwd_wps = value;
        return LNERF_OK;
    }
    if (strcmp(key, "mlp_fwd_blocks") == 0) {
        LNERF_REQUIRE(value >= 1 && value <= 65535, "set_tuning: mlp_fwd_blocks out of range");
        g_mlp_fwd_blocks = value;
        return LNERF_OK;
    }
    if (strcmp(key, "scatter_level_groups") == 0) {
        LNERF_REQUIRE(value >= 1 && value <= LNERF_MAX_LEVELS, "set_tuning: scatter_level_groups out of range");
        g_scatter_groups = value;
        return LNERF_OK;
    }
    if (strcmp(key, "scatter_skip_zero") == 0) {
        g_skip_zero = value ? 1 : 0;
        return LNERF_OK;
    }
    if (strcmp(key, "scatter_reduce_threads") == 0) {
        LNERF_REQUIRE(value == 512 || value == 1024, "set_tuning: scatter_reduce_threads must be 512 or 1024");
        g_reduce_threads = value;
        return LNERF_OK;
    }
    set_error("set_tuning: unknown key '%s'", key);
    return LNERF_ERR_INVALID_ARG;
}

#ifdef LNERF_STAMPS
// diagnostic builds only: read (and clear) the per-phase shader-clock totals of the binning pass
int lnerf_debug_wg_log(unsigned long long *out, int words) {   // reads AND clears the log
    static unsigned long long zero[4 * 4096];
    if (words > 4 * 4096) words = 4 * 4096;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_log), (size_t)words * 8) != hipSuccess) return LNERF_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wg_log), zero, sizeof(zero)) != hipSuccess) return LNERF_ERR_HIP;
    return LNERF_OK;
}
int lnerf_debug_bin_stamps(unsigned long long *out16) {   // pass 1's totals (grid_bin.hip) + pass 2's (this file); clears both
    unsigned long long z[16] = {0}, mine[16];
    if (hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_bin_stamps), sizeof(z)) != hipSuccess) return LNERF_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bin_stamps), z, sizeof(z)) != hipSuccess) return LNERF_ERR_HIP;
    const int rc = bin_stamps_read(out16);
    if (rc != LNERF_OK) return rc;
    for (int k = 0; k < 16; ++k) out16[k] += mine[k];
    return LNERF_OK;
}
#endif

size_t lnerf_grid_scatter_clear_bytes(int num_levels, const int32_t *offsets_host, int64_t m_host) {
    ScatterPlan plan;
    if (!plan_from_offsets(num_levels, offsets_host, m_host, plan)) return 0;
    return HDR_GMAX_BYTES;   // the level maxima (pass 1 raises them with atomicMax)
}

size_t lnerf_grid_encode_backward_workspace_bytes(int num_levels, const int32_t *offsets_host, int64_t m_host) {
    ScatterPlan plan;
    if (!plan_from_offsets(num_levels, offsets_host, m_host, plan)) return 0;
    return plan.total();  // header, segment table, record chunks, partial-sum tiles of the sliced levels
}

// One call of the scatter: the C ABI's common arguments in their order, then what only some entry points set.
struct ScatterCall {
    const float *xyzs; float bound; const void *dfeat; int dfeat_dtype;                                         // samples
    int num_levels, level_dim; const int32_t *offsets_host; const float *scales_host; const int32_t *res_host;  // levels
    int64_t m_host; const int32_t *m_dev; int64_t level_stride;
    float *dtable; int variant; void *workspace; size_t workspace_bytes; lnerf_stream_t stream;
    const FusedUpdate *fu = nullptr;   // set: every row's Adam step (or its bf16 wire output, fu->grad_out) is applied by the
                                       // workgroup of pass 2 that finishes its bucket; not set: dtable += scatter
    const TailJob *tail = nullptr;     // set: the launch of pass 2 closes the step
    int phases = 3;                    // 1 = pass 1 (binning, all levels), 2 = pass 2 of levels [lv_lo, lv_hi)
    int lv_lo = 0, lv_hi = -1;         // (-1: all levels)
};

static int scatter_backward(ScatterCall c) {
    // LNERF_SCATTER_CLEARED: the caller zeroed the head of the workspace (lnerf_grid_scatter_clear_bytes()) with
    // something it was launching anyway -- the fill dispatch of this call is skipped
    const bool cleared = (c.variant & LNERF_SCATTER_CLEARED) != 0;
    // (LNERF_SCATTER_DEFER_FINISH: accepted, without effect -- pass 2 finishes the sliced buckets itself)
    const int blocked = c.variant & (LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    const int variant = c.variant & ~(LNERF_SCATTER_CLEARED | LNERF_SCATTER_DEFER_FINISH | LNERF_GRID_BLOCKED | LNERF_GRID_TILED);
    const int num_levels = c.num_levels, phases = c.phases;
    const int64_t m_host = c.m_host;
    GridMeta meta;
    if (int rc = fill_meta("grid_encode_backward", meta, num_levels, c.level_dim, c.offsets_host, c.scales_host, c.res_host,
                           blocked)) return rc;
    LNERF_REQUIRE(m_host >= 0 && c.level_stride >= m_host, "grid_encode_backward: need 0 <= m_host <= level_stride");
    LNERF_REQUIRE(m_host < (1ll << 30), "grid_encode_backward: m_host must be below 2^30 samples");
    LNERF_REQUIRE(variant < 2 || m_host < (1ll << 28), "grid_encode_backward: the bucketed scatter takes m_host below 2^28");
    LNERF_REQUIRE(c.bound > 0.f, "grid_encode_backward: bound must be > 0");
    LNERF_REQUIRE(variant >= 0 && variant <= 3, "grid_encode_backward: unknown variant %d", variant);
    LNERF_REQUIRE(c.dfeat_dtype == LNERF_F32, "grid_encode_backward: dfeat must be f32");
    LNERF_REQUIRE(!c.fu || (variant >= 2 && m_host > 0), "grid_encode_backward_adam: needs variant 2/3 and m_host > 0");
    if (m_host == 0) return LNERF_OK;
    LNERF_REQUIRE(c.dtable && (!(phases & 1) || (c.xyzs && c.dfeat)), "grid_encode_backward: null pointer");
    const int lv_lo = c.lv_lo, lv_hi = c.lv_hi < 0 ? num_levels : c.lv_hi;
    LNERF_REQUIRE(lv_lo >= 0 && lv_lo <= lv_hi && lv_hi <= num_levels, "grid_encode_backward: bad level range");
    LNERF_REQUIRE(phases == 3 || variant >= 2, "grid_encode_backward: the split form needs the bucketed scatter");
    hipStream_t s = as_stream(c.stream);
    if (variant < 2) {
        launch_grid_backward_atomic(c.xyzs, c.bound, (const float *)c.dfeat, meta, m_host, c.m_dev, c.level_stride, c.dtable,
                                    variant, s);
        LNERF_CHECK_LAUNCH("grid_encode_backward");
        return LNERF_OK;
    }
    // plan -> pointers -> bin -> reduce
    BucketMeta bm;
    ScatterPlan plan;
    LNERF_REQUIRE(fill_bucket_meta(meta, m_host, bm, plan) == 0,
                  "grid_encode_backward: level too large for the bucketed scatter (use variant 0/1)");
    LNERF_REQUIRE(c.workspace && c.workspace_bytes >= plan.total(), "grid_encode_backward: workspace too small (%zu < %zu)",
                  c.workspace_bytes, plan.total());
    LNERF_REQUIRE(((uintptr_t)c.workspace & 15) == 0 && ((uintptr_t)c.dtable & 15) == 0,
                  "grid_encode_backward: workspace/dtable must be 16-byte aligned");
    const ScatterWs ws = scatter_ws(c.workspace, plan);
    const bool packed = variant == 3, whole = lv_lo == 0 && lv_hi == num_levels;
    ReduceOut out = {};
    out.dtable = c.dtable;
    if (c.fu) out.fu = *c.fu;
    TailJob tj = {};
    if (c.tail) {
        LNERF_REQUIRE(c.fu && !c.fu->grad_out && phases == 3 && whole && g_scatter_groups <= 1,
                      "grid_encode_backward: the closing form needs the fused whole-table call");
        tj = *c.tail;
        tj.blocks = tj.sa.slabs ? (int)div_up(div_up(MLP_SLAB, TAIL_P), FUSED_RT / 256) : 0;   // four slab blocks per workgroup
    }
    if ((phases & 1) && !cleared && hipMemsetAsync(ws.gmax, 0, HDR_GMAX_BYTES, s) != hipSuccess) {
        set_error("grid_encode_backward: hipMemsetAsync failed");
        return LNERF_ERR_HIP;
    }
    auto launch_bin = [&](int l0, int l1) {   // pass 1 (grid_bin.hip)
        launch_scatter_bin(packed, c.xyzs, c.bound, (const float *)c.dfeat, meta, bm, m_host, c.m_dev, c.level_stride, ws.gmax,
                           ws.items_dev, ws.segtab, ws.recs, l0, l1, s);
    };
    auto launch_reduce = [&](int l0, int l1) {   // pass 2 of levels [l0, l1)
        const int w0 = bm.wgstart[l0], w1 = bm.wgstart[l1];
        // the un-sliced levels heaviest first (whole-table launches only: a level-range launch keeps the plain order)
        tj.rev_lo = tj.rev_hi = 0;
        if (l0 == 0 && l1 == num_levels) {
            int lf = 0;
            for (int l = 0; l < num_levels; ++l) if (bm.slices[l] > 1) lf = l + 1;
            tj.rev_lo = bm.wgstart[lf];
            tj.rev_hi = bm.wgstart[num_levels];
        }
        if (w1 <= w0 && tj.blocks == 0) return;
        // (the fused pass with 512-thread workgroups: 118 us against 108, profiles/r03_exp_scatter.jsonl)
        const int rt = c.fu ? FUSED_RT : g_reduce_threads == 512 ? 512 : 1024;
        void (*const k)(GridMeta, BucketMeta, ScatterWs, ReduceOut, int, TailJob) =
            c.fu ? (packed ? k_scatter_reduce<FUSED_RT, Rec8, true> : k_scatter_reduce<FUSED_RT, Rec12, true>)
            : rt == 512 ? (packed ? k_scatter_reduce<512, Rec8, false> : k_scatter_reduce<512, Rec12, false>)
                        : (packed ? k_scatter_reduce<1024, Rec8, false> : k_scatter_reduce<1024, Rec12, false>);
        hipLaunchKernelGGL(k, dim3((unsigned)(w1 - w0 + tj.blocks)), dim3(rt), 0, s, meta, bm, ws, out, w0, tj);
    };
    // level GROUPS (whole-table calls with scatter_level_groups > 1): bin(group) -> reduce(group) -> bin(next group) ...  A
    // group's records (1/groups of the 216 MB a frame writes) are read back right behind their writes, while they still sit
    // in the 256 MiB Infinity Cache: the whole-frame form streams them out to HBM and back.  Measured slower at every group
    // count, and slower still with reduce(g) on a side stream beside bin(g + 1): default 1
    const bool grouped = phases == 3 && g_scatter_groups > 1 && whole;
    const int ng = !grouped ? 1 : g_scatter_groups < num_levels ? g_scatter_groups : num_levels;
    for (int gi = 0; gi < ng; ++gi) {
        const int l0 = (int)((int64_t)num_levels * gi / ng), l1 = (int)((int64_t)num_levels * (gi + 1) / ng);
        if (phases & 1) launch_bin(l0, l1);   // (not grouped: all levels)
        if (phases & 1) LNERF_CHECK_LAUNCH("grid_encode_backward(bin)");
        if (phases & 2) launch_reduce(grouped ? l0 : lv_lo, grouped ? l1 : lv_hi);
        if (phases & 2) LNERF_CHECK_LAUNCH("grid_encode_backward(reduce)");
    }
    return LNERF_OK;
}

int lnerf_grid_encode_backward(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                               int level_dim, const int32_t *offsets_host, const float *scales_host, const int32_t *res_host,
                               int64_t m_host, const int32_t *m_dev, int64_t level_stride, float *dtable, int variant,
                               void *workspace, size_t workspace_bytes, lnerf_stream_t stream) {
    return scatter_backward({xyzs, bound, dfeat, dfeat_dtype, num_levels, level_dim, offsets_host, scales_host, res_host,
                             m_host, m_dev, level_stride, dtable, variant, workspace, workspace_bytes, stream});
}

// the wire mode's checks and its descriptor (the Adam arguments are unused in this mode)
static int fill_wire_output(const char *who, FusedUpdate &fu, void *grad_bf16, const float *dtable_zero) {
    LNERF_REQUIRE(grad_bf16 && dtable_zero, "%s: null output", who);
    LNERF_REQUIRE((((uintptr_t)grad_bf16 | (uintptr_t)dtable_zero) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
    memset(&fu, 0, sizeof(fu));
    adam_host_args(fu.a, 0.f, 0.5f, 0.5f, 1.f, 1, nullptr, 1.f, 0);
    fu.grad_out = (uint16_t *)grad_bf16;
    return LNERF_OK;
}

int lnerf_grid_encode_backward_bf16(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                    int level_dim, const int32_t *offsets_host, const float *scales_host,
                                    const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                                    float *dtable_zero, int variant, void *workspace, size_t workspace_bytes,
                                    void *grad_bf16, lnerf_stream_t stream) {
    FusedUpdate fu;
    if (int rc = fill_wire_output("grid_encode_backward_bf16", fu, grad_bf16, dtable_zero)) return rc;
    return scatter_backward({xyzs, bound, dfeat, dfeat_dtype, num_levels, level_dim, offsets_host, scales_host, res_host,
                             m_host, m_dev, level_stride, dtable_zero, variant, workspace, workspace_bytes, stream, &fu});
}

int lnerf_grid_scatter_bin(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels, int level_dim,
                           const int32_t *offsets_host, const float *scales_host, const int32_t *res_host, int64_t m_host,
                           const int32_t *m_dev, int64_t level_stride, float *dtable_zero, int variant, void *workspace,
                           size_t workspace_bytes, lnerf_stream_t stream) {
    LNERF_REQUIRE(dtable_zero, "grid_scatter_bin: null output");
    ScatterCall c = {xyzs, bound, dfeat, dfeat_dtype, num_levels, level_dim, offsets_host, scales_host, res_host,
                     m_host, m_dev, level_stride, dtable_zero, variant, workspace, workspace_bytes, stream};
    c.phases = 1;
    return scatter_backward(c);
}

int lnerf_grid_scatter_reduce_bf16(float bound, int num_levels, int level_dim, const int32_t *offsets_host,
                                   const float *scales_host, const int32_t *res_host, int64_t m_host, int64_t level_stride,
                                   int level_lo, int level_hi, float *dtable_zero, int variant, void *workspace,
                                   size_t workspace_bytes, void *grad_bf16, lnerf_stream_t stream) {
    FusedUpdate fu;
    if (int rc = fill_wire_output("grid_scatter_reduce_bf16", fu, grad_bf16, dtable_zero)) return rc;
    ScatterCall c = {nullptr, bound, nullptr, LNERF_F32, num_levels, level_dim, offsets_host, scales_host, res_host,
                     m_host, nullptr, level_stride, dtable_zero, variant, workspace, workspace_bytes, stream, &fu};
    c.phases = 2; c.lv_lo = level_lo; c.lv_hi = level_hi;
    return scatter_backward(c);
}

// what the Adam-mode entry points check alike (behind their own checks of the step), and the kernel-side descriptor
static int fill_fused_adam(const char *who, FusedUpdate &fu, int num_levels, const int32_t *offsets_host, float *table,
                           float *exp_avg, float *exp_avg_sq, const float *dtable_zero, void *shadow_bf16, float lr, float beta1,
                           float beta2, float eps, int step, const int32_t *step_dev, float grad_scale) {
    LNERF_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: betas must be in [0,1)", who);
    LNERF_REQUIRE((((uintptr_t)table | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)dtable_zero) & 15) == 0,
                  "%s: buffers must be 16-byte aligned", who);
    LNERF_REQUIRE(!shadow_bf16 || ((uintptr_t)shadow_bf16 & 7) == 0, "%s: shadow must be 8-byte aligned", who);
    memset(&fu, 0, sizeof(fu));
    fu.p = table; fu.m = exp_avg; fu.v = exp_avg_sq; fu.shadow = (uint16_t *)shadow_bf16;
    adam_host_args(fu.a, lr, beta1, beta2, eps, step, step_dev, grad_scale, 0);
    {   // the moment map bound to this optimiser state, if any
        std::lock_guard<std::mutex> lock(g_maps_mutex);
        const auto it = g_maps.find(exp_avg);
        if (it != g_maps.end()) {
            const size_t need = lnerf_moment_map_bytes(num_levels, offsets_host);
            LNERF_REQUIRE(need > 0 && it->second.bytes >= need, "%s: the bound moment map is too small (%zu < %zu)", who,
                          it->second.bytes, need);
            fu.live = it->second.map;
        }
    }
    // (a skipped group equals a stepped one only where 0 * rcp(eps) and lr * 0 are zero: see FusedUpdate)
    fu.skip = g_adam_skip && eps > 0.f && isfinite(lr) && isfinite(grad_scale) ? 1 : 0;
    return LNERF_OK;
}

size_t lnerf_moment_map_bytes(int num_levels, const int32_t *offsets_host) {
    ScatterPlan plan;
    if (!plan_from_offsets(num_levels, offsets_host, 1, plan)) return 0;
    return (size_t)plan.buckets * LIVE_GROUPS;
}

int lnerf_moment_map_build(const float *exp_avg, const float *exp_avg_sq, int num_levels, int level_dim,
                           const int32_t *offsets_host, void *map, size_t map_bytes, lnerf_stream_t stream) {
    LNERF_REQUIRE(exp_avg && exp_avg_sq && map, "moment_map_build: null pointer");
    LNERF_REQUIRE(level_dim == 2, "moment_map_build: level_dim must be 2");
    const size_t need = lnerf_moment_map_bytes(num_levels, offsets_host);
    LNERF_REQUIRE(need > 0, "moment_map_build: bad level table");
    LNERF_REQUIRE(map_bytes >= need, "moment_map_build: map too small (%zu < %zu)", map_bytes, need);
    LNERF_REQUIRE((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 7) == 0 && ((uintptr_t)map & 15) == 0,
                  "moment_map_build: moments must be 8-byte, the map 16-byte aligned");
    MapLevels lv = {};
    lv.num_levels = num_levels;
    int buckets = 0;
    for (int l = 0; l < num_levels; ++l) {
        lv.offsets[l] = offsets_host[l];
        lv.bstart[l] = buckets;
        buckets += (int)div_up((int64_t)offsets_host[l + 1] - offsets_host[l], BK_ROWS);
    }
    lv.offsets[num_levels] = offsets_host[num_levels];
    lv.bstart[num_levels] = buckets;
    LNERF_REQUIRE((size_t)buckets * LIVE_GROUPS == need, "moment_map_build: bucket plan mismatch");
    hipLaunchKernelGGL(k_moment_map, dim3((unsigned)(buckets * (BK_ROWS / 256))), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2 *>(exp_avg), reinterpret_cast<const float2 *>(exp_avg_sq), lv, (uint8_t *)map);
    LNERF_CHECK_LAUNCH("moment_map_build");
    return LNERF_OK;
}

int lnerf_moment_map_bind(const float *exp_avg, void *map, size_t map_bytes) {
    LNERF_REQUIRE(exp_avg, "moment_map_bind: null exp_avg");
    LNERF_REQUIRE(!map || (map_bytes > 0 && map_bytes % LIVE_GROUPS == 0 && ((uintptr_t)map & 15) == 0),
                  "moment_map_bind: the map must be 16-byte aligned and whole buckets of %d bytes", LIVE_GROUPS);
    std::lock_guard<std::mutex> lock(g_maps_mutex);
    if (map) g_maps[exp_avg] = {(uint8_t *)map, map_bytes};
    else g_maps.erase(exp_avg);
    return LNERF_OK;
}

int lnerf_grid_encode_backward_adam(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                    int level_dim, const int32_t *offsets_host, const float *scales_host,
                                    const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                                    float *dtable_zero, int variant, void *workspace, size_t workspace_bytes, float *table,
                                    float *exp_avg, float *exp_avg_sq, void *shadow_bf16, float lr, float beta1, float beta2,
                                    float eps, int step, const int32_t *step_dev, float grad_scale, lnerf_stream_t stream) {
    LNERF_REQUIRE(table && exp_avg && exp_avg_sq, "grid_encode_backward_adam: null optimiser state");
    LNERF_REQUIRE(step_dev || step >= 1, "grid_encode_backward_adam: step must be >= 1 (got %d)", step);
    FusedUpdate fu;
    if (int rc = fill_fused_adam("grid_encode_backward_adam", fu, num_levels, offsets_host, table, exp_avg, exp_avg_sq, dtable_zero, shadow_bf16, lr, beta1,
                                 beta2, eps, step, step_dev, grad_scale)) return rc;
    return scatter_backward({xyzs, bound, dfeat, dfeat_dtype, num_levels, level_dim, offsets_host, scales_host, res_host,
                             m_host, m_dev, level_stride, dtable_zero, variant, workspace, workspace_bytes, stream, &fu});
}

// the MLP half of a step tail: argument checks + the kernel-side descriptor
static int fill_slab_adam(const char *who, SlabAdam &sa, const void *mlp_workspace, size_t mlp_workspace_bytes,
                          int mlp_precision, int out_dim, int64_t m_host, float *const *params_host,
                          float *const *exp_avg_host, float *const *exp_avg_sq_host, float mlp_lr,
                          const int32_t *const *maps_host) {
    memset(&sa, 0, sizeof(sa));
    LNERF_REQUIRE(out_dim >= 2 && out_dim <= 8, "%s: out_dim must be in [2,8]", who);
    LNERF_REQUIRE(mlp_precision == LNERF_F32 || mlp_precision == LNERF_BF16, "%s: bad precision tag", who);
    LNERF_REQUIRE(mlp_workspace && mlp_workspace_bytes >= lnerf_mlp_backward_workspace_bytes(out_dim),
                  "%s: MLP workspace too small", who);
    LNERF_REQUIRE(params_host && exp_avg_host && exp_avg_sq_host && m_host > 0, "%s: null MLP state", who);
    for (int k = 0; k < 6; ++k) {
        LNERF_REQUIRE(params_host[k] && exp_avg_host[k] && exp_avg_sq_host[k], "%s: null MLP tensor %d", who, k);
        sa.p[k] = params_host[k]; sa.m[k] = exp_avg_host[k]; sa.v[k] = exp_avg_sq_host[k];
    }
    if (maps_host) {
        for (int k = 0; k < 3; ++k) {
            LNERF_REQUIRE(maps_host[k] && ((uintptr_t)maps_host[k] & 7) == 0, "%s: bad fragment map %d", who, k);
            sa.map[k] = maps_host[k];
        }
        sa.shadow = (uint16_t *)const_cast<void *>(mlp_workspace);   // the fragment image heads the workspace
    }
    sa.slabs = reinterpret_cast<const float *>(static_cast<const char *>(mlp_workspace) + MLP_FRAG_BYTES);
    sa.n_slabs = lnerf_mlp_backward_slabs(m_host, mlp_precision);
    sa.out_dim = out_dim;
    sa.lr = mlp_lr;
    return LNERF_OK;
}

int lnerf_grid_encode_backward_adam_tail(const float *xyzs, float bound, const void *dfeat, int dfeat_dtype, int num_levels,
                                         int level_dim, const int32_t *offsets_host, const float *scales_host,
                                         const int32_t *res_host, int64_t m_host, const int32_t *m_dev, int64_t level_stride,
                                         float *dtable_zero, int variant, void *workspace, size_t workspace_bytes,
                                         float *table, float *exp_avg, float *exp_avg_sq, void *shadow_bf16, float lr,
                                         const void *mlp_workspace, size_t mlp_workspace_bytes, int mlp_precision,
                                         int out_dim, float *const *params_host, float *const *exp_avg_host,
                                         float *const *exp_avg_sq_host, float mlp_lr, const int32_t *const *maps_host,
                                         float beta1, float beta2, float eps, int step, int32_t *step_dev, float grad_scale,
                                         int flags, lnerf_stream_t stream) {
    LNERF_REQUIRE(table && exp_avg && exp_avg_sq, "grid_encode_backward_adam_tail: null optimiser state");
    LNERF_REQUIRE(step_dev, "grid_encode_backward_adam_tail: needs the device counter pair (int32[2])");
    LNERF_REQUIRE(m_host > 0, "grid_encode_backward_adam_tail: needs m_host > 0 (use lnerf_step_tail for an empty frame)");
    FusedUpdate fu;
    if (int rc = fill_fused_adam("grid_encode_backward_adam_tail", fu, num_levels, offsets_host, table, exp_avg, exp_avg_sq, dtable_zero, shadow_bf16, lr,
                                 beta1, beta2, eps, step, step_dev, grad_scale)) return rc;
    TailJob tj = {};
    if (mlp_workspace) {
        if (int rc = fill_slab_adam("grid_encode_backward_adam_tail", tj.sa, mlp_workspace, mlp_workspace_bytes, mlp_precision,
                                    out_dim, m_host, params_host, exp_avg_host, exp_avg_sq_host, mlp_lr, maps_host)) return rc;
    }
    tj.tick = step_dev;
    tj.do_tick = (flags & LNERF_TAIL_TICK) ? 1 : 0;
    tj.clear_gmax = (flags & LNERF_TAIL_CLEAR_SCATTER) ? 1 : 0;
    return scatter_backward({xyzs, bound, dfeat, dfeat_dtype, num_levels, level_dim, offsets_host, scales_host, res_host,
                             m_host, m_dev, level_stride, dtable_zero, variant, workspace, workspace_bytes, stream, &fu, &tj});
}

int lnerf_step_tail(int num_levels, int level_dim, const int32_t *offsets_host, const float *scales_host,
                    const int32_t *res_host, int64_t m_host, int variant, void *scatter_workspace,
                    size_t scatter_workspace_bytes, float *dtable_zero, float *table, float *exp_avg, float *exp_avg_sq,
                    void *shadow_bf16, float table_lr, const void *mlp_workspace, size_t mlp_workspace_bytes,
                    int mlp_precision, int out_dim, float *const *params_host, float *const *exp_avg_host,
                    float *const *exp_avg_sq_host, float mlp_lr, const int32_t *const *maps_host, float beta1, float beta2,
                    float eps, int step, int32_t *step_dev, float grad_scale, int flags, lnerf_stream_t stream) {
    const bool with_scatter = num_levels > 0, with_mlp = mlp_workspace != nullptr;
    LNERF_REQUIRE(with_scatter || with_mlp, "step_tail: nothing to do");
    LNERF_REQUIRE(step_dev || step >= 1, "step_tail: step must be >= 1 (got %d)", step);
    LNERF_REQUIRE(!(flags & (LNERF_TAIL_TICK | LNERF_TAIL_CLEAR_SCATTER)) || step_dev,
                  "step_tail: the tick / the clearing epilogue need the device counter pair (int32[2])");
    LNERF_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "step_tail: betas must be in [0,1)");
    AdamArgs a;   // (the table's: k_step_tail takes the step and the bias corrections from it)
    adam_host_args(a, table_lr, beta1, beta2, eps, step, step_dev, grad_scale, 0);
    ScatterWs ws = {};
    if (with_scatter) {
        GridMeta meta;
        BucketMeta bm;
        ScatterPlan plan;
        if (int rc = fill_meta("step_tail", meta, num_levels, level_dim, offsets_host, scales_host, res_host)) return rc;
        const int v = variant & 0xFF;
        LNERF_REQUIRE((v == 2 || v == 3) && m_host > 0, "step_tail: needs scatter variant 2 / 3 and m_host > 0");
        LNERF_REQUIRE(fill_bucket_meta(meta, m_host, bm, plan) == 0, "step_tail: level too large for the bucketed scatter");
        LNERF_REQUIRE(scatter_workspace && scatter_workspace_bytes >= plan.total(), "step_tail: scatter workspace too small");
        LNERF_REQUIRE(table && exp_avg && exp_avg_sq && dtable_zero, "step_tail: null optimiser state");
        LNERF_REQUIRE((((uintptr_t)table | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)scatter_workspace) & 15) == 0,
                      "step_tail: buffers must be 16-byte aligned");
        ws = scatter_ws(scatter_workspace, plan);
    }
    LNERF_REQUIRE(!(flags & (LNERF_TAIL_CLEAR_SCATTER | LNERF_TAIL_TICK)) || with_scatter,
                  "step_tail: the tick / the clearing epilogue keep their arrival counters in the scatter workspace");
    SlabAdam sa = {};
    int n_slab_blocks = 0;
    if (with_mlp) {
        if (int rc = fill_slab_adam("step_tail", sa, mlp_workspace, mlp_workspace_bytes, mlp_precision, out_dim, m_host,
                                    params_host, exp_avg_host, exp_avg_sq_host, mlp_lr, maps_host)) return rc;
        n_slab_blocks = (int)div_up(MLP_SLAB, TAIL_P);
    }
    const int do_tick = (flags & LNERF_TAIL_TICK) ? 1 : 0, clr = (flags & LNERF_TAIL_CLEAR_SCATTER) ? 1 : 0;
    // no MLP: the tick / the clearing epilogue still run -- ONE block that arrives on its own (k_step_tail's
    // `sa.slabs == nullptr` branch); a call with nothing at all to do returns without a launch
    if (n_slab_blocks == 0 && (do_tick || clr)) n_slab_blocks = 1;
    const dim3 g((unsigned)n_slab_blocks);
    if (g.x == 0) return LNERF_OK;
    hipLaunchKernelGGL(k_step_tail, g, dim3(256), 0, as_stream(stream), ws.gmax, a, sa, step_dev, ws.arrive, do_tick, clr);
    LNERF_CHECK_LAUNCH("step_tail");
    return LNERF_OK;
}

}  // extern "C"
