// The attention taps of the round loop, a translation unit of their own (the code objects of fwd.hip, env.hip and grad.hip are
// the ones they are without this feature):
//   attention_export_kernel<VPL, W>   conv2's coefficients of the inference path, read back from what the agents forward left
//                                     in its workspace (attention_export.hpp; mel_forward_attention in fwd.hip owns the layout)
//   attention_record.hpp              mel_attention_record_round / mel_attention_record_read on record_common.hpp
#include <cmath>

#include "common.hpp"
#include "attention_export.hpp"
#include "record_common.hpp"      // the trace ring, the fold over the envs and the launch geometry of the recorders
#include "attention_record.hpp"   // whom the deciding agents attend to, per round, degree and head

namespace mel {

// ------------------------------------------------------------------------------------------------
// One wavefront per agent row, the row laid over the wavefront as in attention.hpp's attend_target (a head is lanes_per_head
// adjacent lanes of VPL channels; 6 heads fill 48 lanes and the others hold zeros).  Pass 1 walks the row's sources in
// ascending node id and leaves every (source, head) score in the wave's LDS - attend_step's score expression, channel for
// channel, and head_sum's order -, pass 2 gives a lane the slots lane, lane + 64, ... of the row's [MEL_ATT_MAX_SOURCES][heads]
// block: max, sum of e^(s - max) in ascending source order, e^(s - max) / (sum + 1e-16) with the forward's exp and reciprocal.
// Latency-sized (a few sources per row, a few thousand rows): the conv kind and the live lanes are run-time values, so there are
// eight instantiations (channels per lane x words per node set).
// ------------------------------------------------------------------------------------------------
typedef float export_f32x2 __attribute__((ext_vector_type(2)));

template <int VPL> struct ExportRow {
    float v[VPL];
};

// this lane's VPL channels of a row (zeros on a lane that carries none)
template <int VPL> __device__ __forceinline__ ExportRow<VPL> export_load(const float* p, int lane, int live) {
    ExportRow<VPL> r;
#pragma unroll
    for (int i = 0; i < VPL; ++i) r.v[i] = 0.f;
    if (p && lane < live) {
        p += lane * VPL;
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
    }
    return r;
}

// this lane's share of one (target, source) score: attend_step's expression, channel for channel
template <int VPL>
__device__ __forceinline__ float export_score(int kind, const ExportRow<VPL>& xr, const ExportRow<VPL>& att, const ExportRow<VPL>& xl) {
    if (kind == MEL_CONV_GATV2) {
        export_f32x2 t2 = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < VPL; i += 2) {
            const export_f32x2 z = export_f32x2{xr.v[i], xr.v[i + 1]} + export_f32x2{xl.v[i], xl.v[i + 1]};
            const export_f32x2 zs = z * 0.2f;
            const export_f32x2 zm = {fmaxf(z.x, zs.x), fmaxf(z.y, zs.y)};
            t2 = __builtin_elementwise_fma(export_f32x2{att.v[i], att.v[i + 1]}, zm, t2);
        }
        return t2.x + t2.y;
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) t = fmaf(xr.v[i], xl.v[i], t);
    return t;
}

// sum over the lanes of one head, in head_sum's order: 16 lanes nearest partner first (its DPP moves add the same pairs),
// every other width farthest first
__device__ __forceinline__ float export_head_sum(float s, int lanes_per_head) {
    if (lanes_per_head == 16) {
        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
        return s;
    }
    for (int o = lanes_per_head >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__device__ __forceinline__ float export_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

template <int VPL, int W>
__global__ __launch_bounds__(256) void attention_export_kernel(AttExportArgs a) {
    static_assert(VPL % 2 == 0, "channel pairs");
    __shared__ float score_lds[4][MEL_ATT_MAX_SOURCES * ATT_EXPORT_MAX_HEADS];
    const int lane = lane_id();
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int r = (int)blockIdx.x * 4 + wave;
    if (r >= a.rows_cap) return;
    if (r >= min(*a.rows_dev, a.rows_cap)) return;            // rows from the live count on are not touched
    const AgentRowDesc<W> d = static_cast<const AgentRowDesc<W>*>(a.desc)[r];
    const NodeSet<W> sources = ns_uniform(d.sources), smask = ns_uniform(d.smask);
    const int soff = uniform_i32(d.soff);
    const int count = min(ns_count(sources), MEL_ATT_MAX_SOURCES);      // (the neighbour cap keeps a target at 34 sources)
    float* sc = score_lds[wave];
    const ExportRow<VPL> xr = export_load<VPL>(a.xr + (size_t)r * a.ld_r, lane, a.live);
    const ExportRow<VPL> att = export_load<VPL>(a.att, lane, a.live);
    const int head = lane / a.lanes_per_head;
    const bool writes = lane < a.live && head * a.lanes_per_head == lane;       // a head's first lane
    NodeSet<W> left = sources;
    for (int k = 0; k < count; ++k) {
        const int node = ns_lowest(left);
        ns_clear_lowest(left);
        const int srow = soff + ns_rank_below(smask, node);
        const ExportRow<VPL> xl = export_load<VPL>(a.xl + (size_t)srow * a.ld_l, lane, a.live);
        float t = export_head_sum(export_score<VPL>(a.kind, xr, att, xl), a.lanes_per_head);
        if (a.kind == MEL_CONV_TRANSFORMER) t *= a.score_scale;
        if (writes) sc[k * a.heads + head] = t;
    }
    wave_lds_handover();                                       // the scores change hands inside the wavefront
    const int slots = MEL_ATT_MAX_SOURCES * a.heads;
    float* out = a.alpha + (size_t)r * slots;
    for (int idx = lane; idx < slots; idx += 64) {
        const int k = idx / a.heads, h = idx - k * a.heads;
        float v = 0.f;                                         // slots past the source count
        if (k < count) {
            float m = -INFINITY, l = 0.f;
            for (int j = 0; j < count; ++j) m = fmaxf(m, sc[j * a.heads + h]);
            for (int j = 0; j < count; ++j) l += export_exp(sc[j * a.heads + h] - m);
            v = export_exp(sc[idx] - m) * __builtin_amdgcn_rcpf(l + 1e-16f);
        }
        out[idx] = v;
    }
    if (lane < W) a.sources[(size_t)r * W + lane] = lane == 0 ? sources.w[0] : sources.w[W - 1];
}

template <int VPL> static void launch_attention_export_v(const AttExportArgs& a, int n_nodes, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows_cap + 3) / 4));
    with_words(n_nodes, [&](auto w) { MEL_LAUNCH((attention_export_kernel<VPL, decltype(w)::value>), grid, dim3(256), 0, s, a); });
}

mel_status launch_attention_export(AttExportArgs a, const HeadLanes& hl, int n_nodes, hipStream_t s, const char* what) {
    if (!hl.ok()) return fail(MEL_ERR_UNSUPPORTED, "%s: %s", what, hl.why);
    if (a.heads > ATT_EXPORT_MAX_HEADS) return fail(MEL_ERR_UNSUPPORTED, "%s: %d heads, built for at most %d", what, a.heads, ATT_EXPORT_MAX_HEADS);
    a.lanes_per_head = hl.lanes_per_head, a.live = hl.live;
    switch (hl.vpl) {
        case 2: launch_attention_export_v<2>(a, n_nodes, s); break;
        case 4: launch_attention_export_v<4>(a, n_nodes, s); break;
        case 8: launch_attention_export_v<8>(a, n_nodes, s); break;
        default: launch_attention_export_v<16>(a, n_nodes, s); break;
    }
    return check_launch(what);
}

}  // namespace mel
