// GATv2 / TransformerConv edge softmax + aggregation kernels of the inference path and the
// HL-DGN attention + graph pool (hl_dgn.py:101-108).  Included by fwd.hip after plan.hpp (TargetDesc).
#pragma once
#include "plan.hpp"
#include "gemm_bf16.hpp"   // bf16 pack / unpack helpers

namespace mel {

// ------------------------------------------------------------------------------------------------
// GATv2 edge softmax + aggregation.  One wavefront per target node; the 64 lanes
// span the heads*C output channels (VPL contiguous channels per lane, so a head is C/VPL adjacent
// lanes and the per-head score reduction is a few xor-shuffles).  Sources are streamed once with an
// online softmax: out = sum_j exp(e_j - m) x_l[j] / (sum_j exp(e_j - m) + 1e-16).
// A head count that is no power of two leaves lanes over: 6 heads take 8 lanes each and lanes 48 .. 63
// carry no channels (common.hpp: head_lanes; ATT_WALK_GENERIC_48 below).
// ------------------------------------------------------------------------------------------------
enum { ATT_ROWS = 0, ATT_POOL = 1, ATT_SINGLE = 2 };

struct AttArgs {
    const float* xl;        // source rows
    int ld_l;
    const float* xr;        // target rows
    int ld_r;
    const float* att;       // [heads*C]
    const float* bias;      // [heads*C]
    const uint64_t* adj;    // [bs*N] node sets (MEL_SET_WORDS(n) words each): ATT_POOL; the row kernels read TargetDesc
    int bs, n, lanes_per_head;
    int kind;               // MEL_CONV_*
    float score_scale;      // TransformerConv: 1 / sqrt(C)
    // ATT_ROWS
    float* out;             // [rows, ldo] relu(out + bias)
    int ldo;
    const float* out_scale; // optional [rows]: row r of `out` is stored times out_scale[r] (the decision-maker mask of
                            // l_dgn.py:128 - the x_2 snapshot in xcat is taken before it, l_dgn.py:127)
    uint16_t* out_planes;   // optional (fp32 path, 4+ features per lane): the rows go out ALREADY SPLIT into bf16 planes,
                            // [rows][ldo / 16][3][16] - gemm_planes_kernel's A operand - instead of fp32 rows to `out`: the same
                            // split4() the split GEMMs apply to fp32 rows on their way into LDS
    float* xcat;            // [R, ld_cat] head input: x_1 | x_2 | x_3 (l_dgn.py:139)
    int ld_cat, hidden;
    const float* h0;        // encoder rows (packed by smask), [*, hidden]
    // ATT_POOL
    const float* obs;       // dm flag source
    int obs_stride, node_cols, aggregator;
    float* pooled;          // [bs, heads*C]
    // ATT_ROWS / ATT_SINGLE: one wavefront per target row
    const void* desc;           // [rows] per-target descriptor (TargetDesc<W>)
    const int32_t* rows_dev;    // device-side row count
    long rows_hint;             // expected rows (grid sizing only)
    int rows_cap, cat_off;
    int bf16;                   // bf16 feature path: xl / xr / out / xcat / h0 hold bf16 rows (att / bias stay fp32)
    // node-feature table mode (plan_masks.hpp): xl / xr / h0 are TABLES indexed by a node's tuple id fid[b*N + i] instead of
    // row lists indexed by packed position (null = row lists)
    const int32_t* fid;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int VPL>
struct Vec {
    float v[VPL];
};

template <int VPL>
__device__ __forceinline__ Vec<VPL> load_vec(const float* p) {
    Vec<VPL> r;
    if constexpr (VPL >= 4) {
#pragma unroll
        for (int i = 0; i < VPL / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            r.v[4 * i] = t.x, r.v[4 * i + 1] = t.y, r.v[4 * i + 2] = t.z, r.v[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPL; ++i) r.v[i] = p[i];
    }
    return r;
}

template <int VPL>
__device__ __forceinline__ void store_vec(float* p, const Vec<VPL>& r) {
    if constexpr (VPL >= 4) {
#pragma unroll
        for (int i = 0; i < VPL / 4; ++i)
            reinterpret_cast<float4*>(p)[i] = make_float4(r.v[4 * i], r.v[4 * i + 1], r.v[4 * i + 2], r.v[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < VPL; ++i) p[i] = r.v[i];
    }
}

// feature rows: fp32, or bf16 on the bf16 feature path (math stays fp32 either way).  idx in elements.
template <int VPL, bool BF>
__device__ __forceinline__ Vec<VPL> load_row(const float* base, size_t idx) {
    if constexpr (!BF) {
        return load_vec<VPL>(base + idx);
    } else {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(base) + idx;
        Vec<VPL> r;
        if constexpr (VPL >= 8) {
#pragma unroll
            for (int c = 0; c < VPL / 8; ++c) {
                const u32x4 w = reinterpret_cast<const u32x4*>(p)[c];
#pragma unroll
                for (int i = 0; i < 4; ++i) r.v[8 * c + 2 * i] = bf16_lo(w[i]), r.v[8 * c + 2 * i + 1] = bf16_hi(w[i]);
            }
        } else if constexpr (VPL == 4) {
            const u32x2 w = *reinterpret_cast<const u32x2*>(p);
            r.v[0] = bf16_lo(w[0]), r.v[1] = bf16_hi(w[0]), r.v[2] = bf16_lo(w[1]), r.v[3] = bf16_hi(w[1]);
        } else {
            static_assert(VPL == 2, "VPL");
            const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
            r.v[0] = bf16_lo(w), r.v[1] = bf16_hi(w);
        }
        return r;
    }
}

template <int VPL, bool BF>
__device__ __forceinline__ void store_row(float* base, size_t idx, const Vec<VPL>& r) {
    if constexpr (!BF) {
        store_vec<VPL>(base + idx, r);
    } else {
        uint16_t* p = reinterpret_cast<uint16_t*>(base) + idx;
        if constexpr (VPL >= 8) {
#pragma unroll
            for (int c = 0; c < VPL / 8; ++c) {
                const u32x4 w = {pack_bf16x2(r.v[8 * c], r.v[8 * c + 1]), pack_bf16x2(r.v[8 * c + 2], r.v[8 * c + 3]),
                                 pack_bf16x2(r.v[8 * c + 4], r.v[8 * c + 5]), pack_bf16x2(r.v[8 * c + 6], r.v[8 * c + 7])};
                reinterpret_cast<u32x4*>(p)[c] = w;
            }
        } else if constexpr (VPL == 4) {
            const u32x2 w = {pack_bf16x2(r.v[0], r.v[1]), pack_bf16x2(r.v[2], r.v[3])};
            *reinterpret_cast<u32x2*>(p) = w;
        } else {
            *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(r.v[0], r.v[1]);
        }
    }
}

// sum over the lanes of one head (lanes_per_head adjacent lanes).  The common case (16 lanes: C = 128,
// 8 channels per lane) is four DPP moves inside a 16-lane row; anything else falls back to shuffles.
// LPH = 16: known at compile time (no branch, no shuffle loop in the caller's step); 0: decided per call.
template <int LPH = 0>
__device__ __forceinline__ float head_sum(float s, int lanes_per_head) {
    if constexpr (LPH == 8) {           // 8 lanes per head (6 heads on 48 lanes): the first three of the moves below
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x141, 0xF, 0xF, true));  // row_half_mirror
        return s;
    }
    if (LPH == 16 || lanes_per_head == 16) {
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x141, 0xF, 0xF, true));  // row_half_mirror
        s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x140, 0xF, 0xF, true));  // row_mirror
        return s;
    }
    for (int o = lanes_per_head >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

// attention output of one target for this lane's VPL channels: relu(out + bias).  The source rows are
// streamed once with an online softmax, FOUR sources per step: their row loads, score dot products and
// per-head reductions are independent chains (the single-source form is one long dependent chain per source
// and the launch is latency bound), then one rescale per step:
//   m' = max(m, s_0..s_3); l = l e^(m-m') + sum_k e^(s_k-m'); acc = acc e^(m-m') + sum_k e^(s_k-m') row_k
// KIND = MEL_CONV_GATV2:       e = att . leaky_relu(x_r[i] + x_l[j]),          out = sum alpha x_l[j]
// KIND = MEL_CONV_TRANSFORMER: e = (q[i] . k[j]) / sqrt(C), k | v side by side, out = sum alpha v[j]
// my_fid: table mode - the tuple ids of this lane's nodes (node lane + 64 h of the target's env); a source row is then the
// table row of the source's tuple (one v_readlane) instead of its packed position in the row list.
//
// How a target's sources are walked (ATT_WALK_*).  The arithmetic of a step (attend_step) and the source order - ascending
// node id, G per step - are the same in every form, so the output bits are too (tests/test_gpu_attention_walk.py holds them
// to the bits of the walk these forms replaced, which picked its G sources off the node set in every step).
//   Every form builds the target's source list ONCE - lane k holds the row index of the k-th source - and a step takes its G
//   row indices from that register with v_readlane: no set arithmetic and no launch-uniform branch inside a step
//   GENERIC  table mode and the lanes per head decided at run time (any shape)
//   LIST_16 / TABLE_16  row-list / table mode with 16 lanes per head, both known at compile time (the headline shapes)
//   GENERIC_48  the generic walk on a wavefront of which only 48 lanes carry channels: 6 heads of 8 lanes (common.hpp:
//               head_lanes).  Lanes 48 .. 63 are IDLE: they hold zeros instead of row values, load and store nothing that is
//               addressed by channel, and still serve the source list (lane k holds the k-th source, k up to 63) and the
//               tuple ids of nodes 48 .. 63.  A head's 8 lanes never exchange anything with another head's or with idle lanes.
// (the values are part of the kernels' mangled names, which profiles and kernel traces quote: 0 was the former walk)
enum { ATT_WALK_GENERIC = 1, ATT_WALK_LIST_16 = 2, ATT_WALK_TABLE_16 = 3, ATT_WALK_GENERIC_48 = 4 };

// lanes of a wavefront that carry channels in this form (a row is LIVE * VPL channels wide)
template <int FORM>
constexpr int att_live_lanes() { return FORM == ATT_WALK_GENERIC_48 ? 48 : 64; }

// row loads / stores of the lanes that carry channels; an idle lane holds zeros and touches no memory.  On a full wavefront
// these ARE load_row / store_row / load_vec.
template <int VPL, bool BF, int LIVE>
__device__ __forceinline__ Vec<VPL> load_row_live(const float* base, size_t idx, int lane) {
    if constexpr (LIVE == 64) {
        return load_row<VPL, BF>(base, idx);
    } else {
        Vec<VPL> r;
#pragma unroll
        for (int i = 0; i < VPL; ++i) r.v[i] = 0.f;
        if (lane < LIVE) r = load_row<VPL, BF>(base, idx);
        return r;
    }
}
template <int VPL, bool BF, int LIVE>
__device__ __forceinline__ void store_row_live(float* base, size_t idx, const Vec<VPL>& r, int lane) {
    if (LIVE == 64 || lane < LIVE) store_row<VPL, BF>(base, idx, r);
}

template <int FORM>
__device__ __forceinline__ bool att_table_mode(const AttArgs& a) {
    if constexpr (FORM == ATT_WALK_TABLE_16) return true;
    else if constexpr (FORM == ATT_WALK_LIST_16) return false;
    else return a.fid != nullptr;
}

// start of source row `srow` (wave-uniform): the row loads then take a scalar base and this lane's constant offset
template <bool BF>
__device__ __forceinline__ const float* source_row(const float* base, int srow, int ld) {
    typedef const char __attribute__((address_space(1))) * global_bytes;
    global_bytes p = (global_bytes)base + (size_t)srow * ld * (BF ? 2 : 4);
    // the address stays in its SGPR pair up to the load (scalar base + 32-bit lane offset): without this the lane's offset
    // is folded into the base ahead of the loop and every row costs a 64-bit vector add and an address register pair
    asm("" : "+s"(p));
    return (const float*)p;
}

// one online-softmax step over the G source rows xl (xv: their value halves, TransformerConv); off slots weigh nothing
template <int VPL, int KIND, int G, int LPH>
__device__ __forceinline__ void attend_step(const AttArgs& a, const Vec<VPL>& xr, const Vec<VPL>& att, const Vec<VPL> (&xl)[G],
                                            const Vec<VPL> (&xv)[G], const bool (&on)[G], float& m, float& l, Vec<VPL>& acc) {
    float sc_[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        float t = 0.f;
        if constexpr (KIND == MEL_CONV_GATV2 && VPL % 2 == 0) {
            // leaky_relu(negative_slope=0.2) as max(z, 0.2 z): same value for every finite z and one op
            // fewer than compare + select; channel pairs so that add / scale / fma issue as v_pk_*_f32
            f32x2 t2 = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < VPL; i += 2) {
                const f32x2 z = f32x2{xr.v[i], xr.v[i + 1]} + f32x2{xl[k].v[i], xl[k].v[i + 1]};
                const f32x2 zs = z * 0.2f;
                const f32x2 zm = {fmaxf(z.x, zs.x), fmaxf(z.y, zs.y)};
                t2 = __builtin_elementwise_fma(f32x2{att.v[i], att.v[i + 1]}, zm, t2);
            }
            t = t2.x + t2.y;
        } else if constexpr (KIND == MEL_CONV_GATV2) {
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const float z = xr.v[i] + xl[k].v[i];
                t = fmaf(att.v[i], fmaxf(z, 0.2f * z), t);
            }
        } else {
#pragma unroll
            for (int i = 0; i < VPL; ++i) t = fmaf(xr.v[i], xl[k].v[i], t);
        }
        sc_[k] = t;
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        sc_[k] = head_sum<LPH>(sc_[k], a.lanes_per_head);
        if constexpr (KIND == MEL_CONV_TRANSFORMER) sc_[k] *= a.score_scale;
        if (!on[k]) sc_[k] = -INFINITY;
    }
    float mn = m;
#pragma unroll
    for (int k = 0; k < G; ++k) mn = fmaxf(mn, sc_[k]);
    // e^x as v_exp_f32(x log2 e): ~1e-6 relative on softmax weights that are later normalised (the libm
    // expansion was a quarter of this kernel's VALU work, and the kernel is VALU / latency bound)
    const float rs = fast_exp(m - mn);       // slot 0 is always on, so mn is finite
    float pe[G];
#pragma unroll
    for (int k = 0; k < G; ++k) pe[k] = fast_exp(sc_[k] - mn);   // exp(-inf) = 0 for the off slots
    float ps = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) ps += pe[k];
    l = l * rs + ps;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        float t = acc.v[i] * rs;
#pragma unroll
        for (int k = 0; k < G; ++k) t = fmaf(pe[k], (KIND == MEL_CONV_TRANSFORMER ? xv[k].v[i] : xl[k].v[i]), t);
        acc.v[i] = t;
    }
    m = mn;
}

template <int VPL, int KIND, bool BF, int W, int G, int FORM>
__device__ __forceinline__ Vec<VPL> attend_target(const AttArgs& a, size_t xr_row, NodeSet<W> sources,
                                                  const NodeSet<W>& smask, int soff, const Vec<VPL>& att,
                                                  const Vec<VPL>& bias, int lane, const int (&my_fid)[W]) {
    constexpr int LIVE = att_live_lanes<FORM>();
    constexpr int HC = LIVE * VPL;               // the row's real width: the TransformerConv value half starts there
    // G = sources per online-softmax step.  Row kernels: 2 - with 4 the kernel needs 112 VGPRs (four waves per SIMD), with 2 it
    // fits 96 (five): conv1 attention 24.3 -> 22.8 us, conv2 attention 13.4 -> 13.0 us, step 0.2180 -> 0.2142 ms (two A/B
    // pairs; 3: 24.1 us).  The HL-DGN pool kernel: 2 as well (MEL_ATT_GP: 39.9 -> 33.5 us; 1: 36.4, 3: 34.5).
    const Vec<VPL> xr = load_row_live<VPL, BF, LIVE>(a.xr, xr_row * a.ld_r + lane * VPL, lane);
    float m = -INFINITY, l = 0.f;
    Vec<VPL> acc;
#pragma unroll
    for (int i = 0; i < VPL; ++i) acc.v[i] = 0.f;
    constexpr int LPH = FORM == ATT_WALK_GENERIC ? 0 : FORM == ATT_WALK_GENERIC_48 ? 8 : 16;
    constexpr int CHUNK = 64 - 64 % G;           // sources per list: whole steps, one lane each (the neighbour cap keeps a
                                                 // target at 34 sources, so this loop runs once; it is here for the bound)
    NodeSet<W> left = ns_uniform(sources);       // SGPRs: the list is built by scalar instructions
    int count = ns_count(left);
    while (count > 0) {                          // TransformerConv adds no self-loop: a target may be isolated
        const int nl = min(count, CHUNK);
        // lane k: node id of the k-th source in ascending order; the lanes past the list keep node 0, whose row is
        // the valid row an off slot re-reads
        int node = 0;
        for (int k = 0; k < nl; ++k) {
            node = lane == k ? ns_lowest(left) : node;       // scalar walk of the set, one compare + select per source
            ns_clear_lowest(left);
        }
        int rowv;                                // ... and the row index of that node: its tuple id, or its packed position
        if (att_table_mode<FORM>(a)) {
            if constexpr (W == 1) rowv = __builtin_amdgcn_ds_bpermute(node << 2, my_fid[0]);
            else {
                const int lo = __builtin_amdgcn_ds_bpermute((node & 63) << 2, my_fid[0]);
                const int hi = __builtin_amdgcn_ds_bpermute((node & 63) << 2, my_fid[1]);
                rowv = node < 64 ? lo : hi;
            }
        } else {
            rowv = soff + ns_rank_below(smask, node);
        }
        for (int s0 = 0; s0 < nl; s0 += G) {
            Vec<VPL> xl[G], xv[G];
            bool on[G];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                on[k] = s0 + k < nl;             // slot 0 is always on
                const float* src = source_row<BF>(a.xl, __builtin_amdgcn_readlane(rowv, s0 + k), a.ld_l);
                xl[k] = load_row_live<VPL, BF, LIVE>(src, (unsigned)(lane * VPL), lane);
                if constexpr (KIND == MEL_CONV_TRANSFORMER) xv[k] = load_row_live<VPL, BF, LIVE>(src, (unsigned)(lane * VPL + HC), lane);
            }
            // every row load of the step is in flight before its arithmetic starts (left alone, the scheduler sinks the
            // second source's loads below the first source's score: one memory latency after the other).  Not for bf16 rows:
            // their loads are issued together anyway, and holding both rows unpacked costs 16 VGPRs and a wave per SIMD
            if constexpr (!BF) __builtin_amdgcn_sched_barrier(0);
            attend_step<VPL, KIND, G, LPH>(a, xr, att, xl, xv, on, m, l, acc);
        }
        count -= nl;
    }
    const float inv = __builtin_amdgcn_rcpf(l + 1e-16f);
    Vec<VPL> out;
#pragma unroll
    for (int i = 0; i < VPL; ++i) out.v[i] = fmaxf(acc.v[i] * inv + bias.v[i], 0.f);
    return out;
}

// row r of a [rows, K] matrix as bf16 planes (gemm_planes_kernel's A operand): this lane's VPL consecutive features
// k = lane * VPL ..; the 96 bytes of 16-k step k >> 4 hold hi | mid | lo of its 16 values
template <int VPL>
__device__ __forceinline__ void store_row_planes(uint16_t* base, int r, int K, int lane, const Vec<VPL>& o) {
    static_assert(VPL % 4 == 0, "planes need whole groups of four features per lane");
    uint16_t* row = base + (size_t)r * 3 * K;
    if constexpr (VPL % 8 == 0) {                 // eight features = half of a 16-k step: one 16-byte store per plane
#pragma unroll
        for (int i = 0; i < VPL; i += 8) {
            const int k = lane * VPL + i;
            u32x2 h0, m0, l0, h1, m1, l1;
            split4(f32x4{o.v[i], o.v[i + 1], o.v[i + 2], o.v[i + 3]}, h0, m0, l0);
            split4(f32x4{o.v[i + 4], o.v[i + 5], o.v[i + 6], o.v[i + 7]}, h1, m1, l1);
            uint16_t* d = row + (k >> 4) * 48 + (k & 15);
            *reinterpret_cast<u32x4*>(d) = u32x4{h0[0], h0[1], h1[0], h1[1]};
            *reinterpret_cast<u32x4*>(d + 16) = u32x4{m0[0], m0[1], m1[0], m1[1]};
            *reinterpret_cast<u32x4*>(d + 32) = u32x4{l0[0], l0[1], l1[0], l1[1]};
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPL; i += 4) {
            const int k = lane * VPL + i;
            u32x2 hi, mid, lo;
            split4(f32x4{o.v[i], o.v[i + 1], o.v[i + 2], o.v[i + 3]}, hi, mid, lo);
            uint16_t* d = row + (k >> 4) * 48 + (k & 15);
            *reinterpret_cast<u32x2*>(d) = hi;
            *reinterpret_cast<u32x2*>(d + 16) = mid;
            *reinterpret_cast<u32x2*>(d + 32) = lo;
        }
    }
}

template <int VPL, int LIVE = 64>
__device__ __forceinline__ Vec<VPL> load_vec_or_zero(const float* p, int lane) {
    Vec<VPL> r;
    if (p && (LIVE == 64 || lane < LIVE)) return load_vec<VPL>(p + lane * VPL);
#pragma unroll
    for (int i = 0; i < VPL; ++i) r.v[i] = 0.f;
    return r;
}

// ATT_ROWS / ATT_SINGLE: ONE WAVEFRONT PER TARGET ROW over the whole batch (envs differ a lot in how many
// targets they have - a workgroup per env leaves the launch waiting for the few crowded envs).
//   ATT_ROWS   conv1 of L-DGN: row r of the U1 list -> h1[r]; the agents' x_1 / x_2 go to the head input
//   ATT_SINGLE conv2 of L-DGN: one target per agent row (only the controlling agent's row can reach its
//              logits, l_dgn.py:135), sources = its closed neighbourhood inside U1 -> x_3
// (256, 2): with the bare bound the register allocator aims at 6 waves per SIMD and SPILLS the source-row
// pointers (88 B of scratch in front of every row load); two blocks per CU lets it keep ~100 VGPRs.
#ifdef MEL_ATT_PROF
constexpr int ATT_PROF_MODE = MEL_ATT_PROF;
#else
constexpr int ATT_PROF_MODE = -1;      // no kernel has it
#endif
// Tuning builds (-DMEL_ATT_PROF=<MODE>, kprof.hpp): cycles per sampled wave (wave 0 of every 32nd workgroup) of the rows kernel with that MODE (0 = conv1, 2 = conv2) in
// [0] prologue (row count, att / bias; the first row's descriptor is requested with them), [1] what is left to wait for the
// descriptor, [2] attend_target (row loads + scores + softmax + sum),
// [3] stores, [4] whole wave, [5] waves counted, [6] rows processed
__device__ unsigned long long g_att_prof[8];

#ifndef MEL_ATT_MINB
#define MEL_ATT_MINB 2
#endif
#ifndef MEL_ATT_G
#define MEL_ATT_G 2      // sources per online-softmax step of the row kernels (see attend_target)
#endif
#ifndef MEL_POOL_NW
#define MEL_POOL_NW 8    // waves per env of the pool kernel below 2 048 envs (16 -> 8 with two sources per step: 33.4 -> 31.6 us; 12: 35.1)
#endif
#ifndef MEL_ATT_GP
#define MEL_ATT_GP 2     // ... of the HL-DGN pool kernel (4 -> 2: pool attention 39.9 -> 33.5 us, HL-DGN 512 envs 24.4 -> 26.1 M/s)
#endif
template <int VPL, int MODE, int KIND, bool BF, int W, int FORM>
__global__ __launch_bounds__(256, MEL_ATT_MINB) void gat_attend_rows_kernel(AttArgs a) {
    const bool table = MODE == ATT_ROWS && att_table_mode<FORM>(a);
    KLaps<MODE == ATT_PROF_MODE && !BF, 8> prof;
    const auto wave_start = prof.mark();
    const int lane = lane_id();
    constexpr int LIVE = att_live_lanes<FORM>();
    // A wave takes the rows slot, slot + 4 * grid, ...: the grid is sized from the expected row count (with a quarter to spare),
    // not the worst case, so a wave has one row, seldom more (a surplus workgroup costs a global-load latency and a CU slot
    // before it can exit).  XCD-aware slots: consecutive target rows belong to one env and share their source rows, so the
    // workgroups of an XCD (block id % 8 under round-robin dispatch; the grid is a multiple of 8) hold a CONTIGUOUS range of
    // slots and the shared rows hit in that XCD's L2 instead of being fetched by all eight (measured before the remap: 54 %
    // L2 misses in this kernel).
    // the wave's number, and with it the row index and everything addressed by it, in SGPRs
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int stride = 4 * (int)gridDim.x;
    int r = (((int)blockIdx.x & 7) * ((int)gridDim.x >> 3) + ((int)blockIdx.x >> 3)) * 4 + wave;
    // The slot is known from the launch alone and the row count is a bound, not an address (the descriptors are allocated to
    // rows_cap): the wave asks for its first row's descriptor TOGETHER with the count, att and bias - one memory latency
    // instead of two in front of everything the descriptor addresses.  A slot past the count drops what it fetched.
    const TargetDesc<W>* const desc = static_cast<const TargetDesc<W>*>(a.desc);
    TargetDesc<W> d{};
    if (r < a.rows_cap) d = desc[r];                 // one 32-byte record: no chain of dependent index loads
    const int rows = min(*a.rows_dev, a.rows_cap);
    const Vec<VPL> att = load_vec_or_zero<VPL, LIVE>(a.att, lane);
    const Vec<VPL> bias = load_vec_or_zero<VPL, LIVE>(a.bias, lane);
    prof.lap(0, att.v[0], bias.v[0], ksgpr(rows));
    while (r < rows) {
        prof.mark();
        prof.lap(1, ksgpr(d.sources.w[0]), ksgpr(d.soff));
        int my_fid[W];
        MEL_W_FOR(h) my_fid[h] = 0;
        size_t xr_row = (size_t)r;
        if (table) {                                 // table mode: tuple ids of the target's env (one dependent load)
            MEL_W_FOR(h) my_fid[h] = lane + 64 * h < a.n ? a.fid[(size_t)d.env * a.n + lane + 64 * h] : 0;
            xr_row = (size_t)node_i32<W>(my_fid, d.node);
        }
        const Vec<VPL> o = attend_target<VPL, KIND, BF, W, MEL_ATT_G, FORM>(a, xr_row, d.sources, d.smask, d.soff, att, bias, lane, my_fid);
        prof.lap(2, o.v[0]);
        if constexpr (MODE == ATT_SINGLE) {
            store_row_live<VPL, BF, LIVE>(a.xcat, (size_t)r * a.ld_cat + a.cat_off + lane * VPL, o, lane);
        } else {
            Vec<VPL> om = o;
            if (a.out_scale) {
                const float dmv = a.out_scale[r];
#pragma unroll
                for (int i = 0; i < VPL; ++i) om.v[i] = o.v[i] * dmv;
            }
            bool as_rows = true;
            if constexpr (!BF && VPL % 4 == 0 && LIVE == 64) {      // (rows narrower than the wavefront go out as fp32 rows: fwd.hip)
                if (a.out_planes) store_row_planes<VPL>(a.out_planes, r, a.ldo, lane, om), as_rows = false;
            }
            if (as_rows) store_row_live<VPL, BF, LIVE>(a.out, (size_t)r * a.ldo + lane * VPL, om, lane);
            if (d.cat_row >= 0) {
                const size_t cat = (size_t)d.cat_row * a.ld_cat;
                // x_2: the controlling agent's conv1 row BEFORE the decision-maker mask (l_dgn.py:127)
                store_row_live<VPL, BF, LIVE>(a.xcat, cat + a.hidden + lane * VPL, o, lane);
                // x_1: its encoder row (l_dgn.py:122)
                const size_t h0 = (size_t)(table ? node_i32<W>(my_fid, d.node) : d.soff + ns_rank_below(d.smask, d.node)) * a.hidden;
                if constexpr (BF) {
                    uint16_t* dst = reinterpret_cast<uint16_t*>(a.xcat) + cat;
                    const uint16_t* src = reinterpret_cast<const uint16_t*>(a.h0) + h0;
                    for (int c = lane; c < a.hidden; c += 64) dst[c] = src[c];
                } else {
                    for (int c = lane; c < a.hidden; c += 64) a.xcat[cat + c] = a.h0[h0 + c];
                }
            }
        }
        prof.lap(3);
        prof.add(6, 1);
        r += stride;
        if (r < rows) d = desc[r];                   // (more rows than the grid was sized for)
    }
    prof.since(4, wave_start);
    prof.add(5, 1);
    prof.flush(g_att_prof, threadIdx.x == 0 && (blockIdx.x & 31) == 0);      // a sample: few atomics
}

// ATT_POOL (HL-DGN): one workgroup per env (every env has exactly N targets, so this is balanced):
// conv1 attention for all nodes, decision-maker mask, max / mean / add pool over the graph.
// NW wavefronts per env: at 512 envs per GPU four waves per workgroup leave a CU with 8 resident waves (two workgroups),
// too few to hide the source-row latency; eight waves (MEL_POOL_NW; six or seven targets each at N = 50) with two source rows
// per step measure best (sixteen: 33.4 us, twelve: 35.1, eight: 31.6).
template <int VPL, bool BF, int NW, int W, int FORM>
__global__ __launch_bounds__(64 * NW) void gat_attend_pool_kernel(AttArgs a) {
    const bool table = att_table_mode<FORM>(a);
    constexpr int LIVE = att_live_lanes<FORM>();
    constexpr int HC = LIVE * VPL;
    __shared__ float part[NW][HC];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const Vec<VPL> att = load_row_live<VPL, false, LIVE>(a.att, lane * VPL, lane);
    const Vec<VPL> bias = load_row_live<VPL, false, LIVE>(a.bias, lane * VPL, lane);
    const NodeSet<W> full = ns_full<W>(a.n);
    Vec<VPL> pool;
#pragma unroll
    for (int i = 0; i < VPL; ++i) pool.v[i] = (a.aggregator == MEL_AGG_MAX) ? -INFINITY : 0.f;
    int my_fid[W];                                                                    // table mode (null: rows b*N + i)
    MEL_W_FOR(h) my_fid[h] = (table && lane + 64 * h < a.n) ? a.fid[(size_t)b * a.n + lane + 64 * h] : 0;
    for (int t = wave; t < a.n; t += NW) {
        const NodeSet<W> sources = ns_load<W>(a.adj, (size_t)b * a.n + t) | ns_bit<W>(t);
        const size_t xr_row = table ? (size_t)node_i32<W>(my_fid, t) : (size_t)(b * a.n + t);
        const Vec<VPL> o = attend_target<VPL, MEL_CONV_GATV2, BF, W, MEL_ATT_GP, FORM>(a, xr_row, sources, full, b * a.n, att, bias, lane, my_fid);
        // hl_dgn.py:105-108: mask out non-decision-makers, then pool over the graph
        const float dm = a.obs[(size_t)b * a.obs_stride + t * a.node_cols + a.node_cols - 1];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const float v = o.v[i] * dm;
            pool.v[i] = (a.aggregator == MEL_AGG_MAX) ? fmaxf(pool.v[i], v) : pool.v[i] + v;
        }
    }
    if (LIVE == 64 || lane < LIVE) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) part[wave][lane * VPL + i] = pool.v[i];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < HC; c += 64 * NW) {
        float v = part[0][c];
        if (a.aggregator == MEL_AGG_MAX) {
#pragma unroll
            for (int w = 1; w < NW; ++w) v = fmaxf(v, part[w][c]);
        } else {
#pragma unroll
            for (int w = 1; w < NW; ++w) v += part[w][c];
            if (a.aggregator == MEL_AGG_MEAN) v /= (float)a.n;
        }
        if constexpr (BF) reinterpret_cast<uint16_t*>(a.pooled)[(size_t)b * HC + c] = (uint16_t)pack_bf16x2(v, 0.f);
        else a.pooled[(size_t)b * HC + c] = v;
    }
}

// The walk form of a launch (ATT_WALK_*).  The compile-time forms exist for 8 channels per lane with 16 lanes per head - hidden
// size 128 with four heads, which every configuration BASELINE quotes runs at; every other shape takes the generic list walk.
template <int V, int MODE>
static int att_walk_form(const AttArgs& a, int live) {
    if (live == 48) return ATT_WALK_GENERIC_48;     // (V 8 and 16 only: head_lanes admits nothing else on 48 lanes)
    if (V == 8 && a.lanes_per_head == 16) return (MODE != ATT_SINGLE && a.fid) ? ATT_WALK_TABLE_16 : ATT_WALK_LIST_16;
    return ATT_WALK_GENERIC;
}

template <int V, int MODE, int FORM>
static void launch_attend_form(const AttArgs& a, int grid, hipStream_t s) {
    with_flag(a.bf16, [&](auto bf) {
        constexpr bool BF = decltype(bf)::value;
        if constexpr (MODE == ATT_POOL) {
            auto launch = [&](auto nw, auto w) {        // NW waves per env, node sets of W words
                constexpr int NW = decltype(nw)::value;
                MEL_LAUNCH((gat_attend_pool_kernel<V, BF, NW, decltype(w)::value, FORM>), dim3(a.bs), dim3(64 * NW), 0, s, a);
            };
            if (a.n > 64) launch(int_c<16>{}, int_c<2>{});              // graphs of 65 .. 128 nodes: two-word node sets
            else if (a.bs >= 2048) launch(int_c<4>{}, int_c<1>{});
            else launch(int_c<MEL_POOL_NW>{}, int_c<1>{});
        } else {
            with_words(a.n, [&](auto w) {
                with_flag(a.kind == MEL_CONV_TRANSFORMER, [&](auto tconv) {
                    constexpr int KIND = decltype(tconv)::value ? MEL_CONV_TRANSFORMER : MEL_CONV_GATV2;
                    MEL_LAUNCH((gat_attend_rows_kernel<V, MODE, KIND, BF, decltype(w)::value, FORM>), dim3(grid), dim3(256), 0, s, a);
                });
            });
        }
    });
}

// V channels per lane: the launch in the walk form of its arguments - only the forms att_walk_form can name are instantiated
template <int V, int MODE>
static bool launch_attend_v(const AttArgs& a, int live, int grid, hipStream_t s) {      // false: no such instantiation
    switch (att_walk_form<V, MODE>(a, live)) {
        case ATT_WALK_LIST_16:
            if constexpr (V == 8) launch_attend_form<V, MODE, ATT_WALK_LIST_16>(a, grid, s);
            break;
        case ATT_WALK_TABLE_16:
            if constexpr (V == 8 && MODE != ATT_SINGLE) launch_attend_form<V, MODE, ATT_WALK_TABLE_16>(a, grid, s);
            break;
        case ATT_WALK_GENERIC_48:
            if constexpr (V == 8 || V == 16) launch_attend_form<V, MODE, ATT_WALK_GENERIC_48>(a, grid, s);
            else return false;
            break;
        default: launch_attend_form<V, MODE, ATT_WALK_GENERIC>(a, grid, s); break;
    }
    return true;
}

template <int MODE>
static mel_status launch_attend(AttArgs a, const HeadLanes& hl, hipStream_t s, const char* what) {
    if (!hl.ok()) return fail(MEL_ERR_UNSUPPORTED, "%s: %s", what, hl.why);
    a.lanes_per_head = hl.lanes_per_head;
    int grid = 0;                                       // the pool kernel: one workgroup per env
    if constexpr (MODE != ATT_POOL) {
        long want = ((a.rows_hint > 0 ? a.rows_hint : a.rows_cap) * 5 / 4 + 3) / 4;     // 25 % head-room, loop covers the rest
        if (want > (a.rows_cap + 3) / 4) want = (a.rows_cap + 3) / 4;
        if (want < 256) want = 256;
#ifdef MEL_ATT_GRID_CAP
        if (want > MEL_ATT_GRID_CAP) want = MEL_ATT_GRID_CAP;      // tuning: resident workgroups only, every wave loops
#endif
#ifdef MEL_ATT2_GRID_CAP
        if (MODE == ATT_SINGLE && want > MEL_ATT2_GRID_CAP) want = MEL_ATT2_GRID_CAP;
#endif
        grid = (int)((want + 7) & ~7L);                 // multiple of 8: block id % 8 = XCD
    }
    bool launched = false;
    switch (hl.vpl) {
        case 2: launched = launch_attend_v<2, MODE>(a, hl.live, grid, s); break;
        case 4: launched = launch_attend_v<4, MODE>(a, hl.live, grid, s); break;
        case 8: launched = launch_attend_v<8, MODE>(a, hl.live, grid, s); break;
        default: launched = launch_attend_v<16, MODE>(a, hl.live, grid, s); break;
    }
    if (!launched)
        return fail(MEL_ERR_UNSUPPORTED, "%s: no kernel for %d channels per lane on %d live lanes", what, hl.vpl, hl.live);
    return check_launch(what);
}

}  // namespace mel
