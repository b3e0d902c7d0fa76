// The node-feature table (plan_masks.hpp) in ONE pass: the workgroup that makes the encoder rows of a block of feature
// tuples also runs conv1's projections of them, so the table costs no launch of its own (it rides with the row lists in
// plan_enc_kernel, fwd.hip) where it used to cost the encoder tiles there plus a latency-bound conv1 launch behind them.
//
//     h0[m, :]        = relu(W1 relu(W0 x(m) + b0) + b1)         x(m): the 5 features of tuple m (tuple_features)
//     xl | xr [m, :]  = (Wl | Wr) h0[m, :] + (bl | br)
//
// A work item is TBL_BM = 32 rows by TBL_BN = 256 conv1 columns on four wavefronts:
//   * layer 0 (K = 5: VALU) fills the 32 x 128 block in LDS, in the A-operand layout of gemm_f32_tile;
//   * layer 1 on the exact-fp32 MFMA, one 32 x 32 block per wavefront (hidden = 128 columns); the finished rows (bias, ReLU)
//     overwrite the block in LDS and the item of column group 0 stores them to t_h0;
//   * conv1 with A read from that block, 32 x 64 per wavefront; columns [0, split_n) are lin_l -> t_xl, the rest lin_r -> t_xr.
// Every workgroup recomputes the encoder rows of its block: with r rows by c columns a work item costs (r / 64) (2 + c / 64)
// units of 64 MFMAs per wavefront, and about one item per CU is what the table's 2 000 tuples give: 32 x 256 is 3 units deep,
// 64 x 128 is 4, 64 x 64 (two items per CU) 6.
//
// The weights pass through a per-wavefront transposition stage, with no ring and no workgroup barrier.  In this shape no two
// wavefronts read the same weight row (each owns 32 rows of layer 1 and 64 of conv1), so LDS only turns coalesced row slices
// into fragment order.  A two-stage ring of 16-k stages shared by the workgroup, with one stage of look-ahead, waited for
// memory in every one of its 16 steps, and fragment-order loads straight into registers (32 cache lines per instruction) kept
// the address path busy for 15 000 cycles before the first product (both measured, NOTES.md).  So: K is 128 for both products,
// a wavefront requests its rows as whole 128-byte slices before any use - layer 1 and the first half of conv1's K at the top
// of the item, the second half when layer 1 has freed its registers (182 VGPRs; two wavefronts per SIMD, which is what the
// row lists beside it run at anyway) - and per 32-k step writes the slices to its own [64][36] stage and reads them back as
// fragments, exactly the LDS image gemm_f32_tile's staging gives.
//
// The sums are those of gemm_f32_tile bit for bit: the same instruction, accumulators from zero, the same k order (fragment
// i = 4 kt + q is what that tile's ds_read_b128 of step kt, sub-step q hands the lane), the same fp32 rows of h0 as are stored.
#pragma once
#include "gemm_f32.hpp"

namespace mel {

constexpr int TBL_BM = 32, TBL_BN = 256;
constexpr int TBL_HIDDEN = 128;                       // encoder width (both layers) = conv1's K: four wavefronts of 32 columns
constexpr int TBL_A_STRIDE = TBL_HIDDEN + 4;          // floats; rows 16 bytes apart modulo 256: conflict-free ds_read_b128
constexpr int TBL_LDS_FLOATS = TBL_BM * TBL_A_STRIDE + TBL_HIDDEN * 9 + 4 * 64 * GEMM_LDS_STRIDE;      // 58 368 bytes

struct TableArgs {
    int T = 0;                          // feature tuples (rows)
    int in_dim = 0;                     // encoder layer 0: [TBL_HIDDEN, in_dim]
    const float* enc_w = nullptr;
    const float* enc_b = nullptr;
    const float* W1 = nullptr;          // encoder layer 1: [TBL_HIDDEN, TBL_HIDDEN]
    const float* b1 = nullptr;
    const float* Wl = nullptr;          // conv1.lin_l [split_n, TBL_HIDDEN], lin_r [N - split_n, TBL_HIDDEN]
    const float* Wr = nullptr;
    const float* bl = nullptr;
    const float* br = nullptr;
    int split_n = 0, N = 0;             // split_n % 32 == 0, N % TBL_BN == 0
    float* h0 = nullptr;                // [T, TBL_HIDDEN]
    float* xl = nullptr;                // [T, split_n]
    float* xr = nullptr;                // [T, N - split_n]
};

static inline int table_items(const TableArgs& a) { return ((a.T + TBL_BM - 1) / TBL_BM) * (a.N / TBL_BN); }

#ifdef MEL_TABLE_PROF
constexpr bool TABLE_PROF = true;
#else
constexpr bool TABLE_PROF = false;
#endif
// Tuning builds (-DMEL_TABLE_PROF, kprof.hpp): cycles wave 0 of every table work item spends [0] up to the finished layer-0 block,
// [1] in layer 1's products, [2] storing its rows, [3] in conv1's products, [4] in conv1's epilogue, [5] in all, [6] items
// counted (tools/table_prof.py)
__device__ unsigned long long g_table_prof[8];

// Between the lanes that write a wavefront's own LDS stage and the lanes that read it (and back, before the next slices
// overwrite it): the LDS operations of one wavefront execute in order, so no instruction is needed - a wavefront-scope
// fence pair and a wave barrier say so to the compiler, which may then not move an access across the hand-over.
__device__ __forceinline__ void table_stage_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Work item `block` of the table: row block block / (N / 256), column group block % (N / 256) - the column group is the
// fast index, so that with workgroup ids dealt to the 8 XCDs in turn each XCD's L2 holds one or two 256-column weight slabs.
// `lds`: TBL_LDS_FLOATS floats, 16-byte aligned.  256 threads.
__device__ __forceinline__ void table_fused_tile(const TableArgs& a, const int block, float* lds) {
    const int ncg = a.N / TBL_BN;
    const int m0 = (block / ncg) * TBL_BM, cg = block % ncg;
    const int T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    KLaps<TABLE_PROF, 8> prof;
    const auto item_start = prof.mark();
    float* ablk = lds;
    float* enc = lds + TBL_BM * TBL_A_STRIDE;         // layer-0 weights as [128][9]

    // layer 0's weights first: loads return in order, and layer 0 should wait for these only
    float e0[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const int i = tid + 256 * u, k = i / 9, f = i - k * 9;
        e0[u] = 0.f;
        if (i < TBL_HIDDEN * 9) e0[u] = f == 8 ? a.enc_b[k] : (f < a.in_dim ? a.enc_w[(size_t)k * a.in_dim + f] : 0.f);
    }
    // ... and the epilogues' biases: a load issued later would make its wait cover the weight slices still in flight
    const float bias1 = a.b1 ? a.b1[wid * 32 + r] : 0.f;
    float biasc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = cg * TBL_BN + wid * 64 + j * 32 + r;
        const float* bp = n >= a.split_n ? a.br : a.bl;
        biasc[j] = bp ? bp[n >= a.split_n ? n - a.split_n : n] : 0.f;
    }
    // This wavefront's weight rows (32 of layer 1, 64 of conv1; no two wavefronts share a row), requested in whole 128-byte
    // row slices - lane l: row 8 g + l / 8, 16 bytes at k = 32 s + 4 (l % 8) - before any use: layer 1 and the first half of
    // conv1's K here, the second half once layer 1 has freed its registers
    const int lrow = lane >> 3, lk = (lane & 7) * 4;
    float* wp = enc + TBL_HIDDEN * 9 + wid * 64 * GEMM_LDS_STRIDE;      // this wavefront's own [64][36] stage
    f32x4 w1r[4][4], wcr[4][8];
    {
        const float* src = a.W1 + (size_t)(wid * 32 + lrow) * TBL_HIDDEN + lk;
#pragma unroll
        for (int sg = 0; sg < 4; ++sg)
#pragma unroll
            for (int g = 0; g < 4; ++g) w1r[sg][g] = *reinterpret_cast<const f32x4*>(src + (size_t)8 * g * TBL_HIDDEN + 32 * sg);
    }
    const float* wc_src[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int n = cg * TBL_BN + wid * 64 + 8 * g + lrow;
        wc_src[g] = (n >= a.split_n ? a.Wr + (size_t)(n - a.split_n) * TBL_HIDDEN : a.Wl + (size_t)n * TBL_HIDDEN) + lk;
    }
#pragma unroll
    for (int sg = 0; sg < 2; ++sg)
#pragma unroll
        for (int g = 0; g < 8; ++g) wcr[sg][g] = *reinterpret_cast<const f32x4*>(wc_src[g] + 32 * sg);

    // layer 0 in the producer's arithmetic (fetch_a<GEMM_MODE_ENC>): rows beyond T are clamped, never stored
#pragma unroll
    for (int u = 0; u < 5; ++u)
        if (tid + 256 * u < TBL_HIDDEN * 9) enc[tid + 256 * u] = e0[u];
    __syncthreads();
    {
        const int row = tid >> 3, kc = (tid & 7) * 4;
        float x[8];
        tuple_features(min(m0 + row, T - 1), x);
#pragma unroll
        for (int k0 = 0; k0 < TBL_HIDDEN; k0 += 32) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* w = enc + (k0 + kc + e) * 9;
                float s = w[8];
#pragma unroll
                for (int f = 0; f < 8; ++f) s = fmaf(w[f], x[f], s);
                v[e] = fmaxf(s, 0.f);
            }
            const f32x4 out = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(ablk + row * TBL_A_STRIDE + k0 + kc) = out;
        }
    }
    __syncthreads();
    prof.lap(0);

    // layer 1: 32 x 128, one 32 x 32 block per wavefront
    const float* afrag = ablk + r * TBL_A_STRIDE + 4 * h;
    f32x16 acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
    const float* wfrag = wp + r * GEMM_LDS_STRIDE + 4 * h;
    float* wslot = wp + lrow * GEMM_LDS_STRIDE + lk;
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {        // a 32-k step of gemm_f32_tile: the slices through the wavefront's stage into fragment order
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(wslot + 8 * g * GEMM_LDS_STRIDE) = w1r[sg][g];
        table_stage_handoff();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(afrag + 32 * sg + 8 * q);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(wfrag + 8 * q);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc1, 0, 0, 0);
        }
        table_stage_handoff();
    }
#pragma unroll
    for (int sg = 2; sg < 4; ++sg)
#pragma unroll
        for (int g = 0; g < 8; ++g) wcr[sg][g] = *reinterpret_cast<const f32x4*>(wc_src[g] + 32 * sg);
    prof.lap(1);
    __syncthreads();                    // every wavefront has read layer 0's rows: the finished rows replace them
    {
        const int n = wid * 32 + r;
        const float bias = bias1;
        float v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = fmaxf(acc1[e] + bias, 0.f);
#pragma unroll
        for (int e = 0; e < 16; ++e) ablk[(4 * h + (e & 3) + 8 * (e >> 2)) * TBL_A_STRIDE + n] = v[e];
        if (cg == 0) {
            float* col = a.h0 + n;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + 4 * h + (e & 3) + 8 * (e >> 2);
                if (m < T) col[(size_t)m * TBL_HIDDEN] = v[e];
            }
        }
    }
    __syncthreads();
    prof.lap(2);

    // conv1: 32 x 256, 32 x 64 per wavefront
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {
#pragma unroll
        for (int g = 0; g < 8; ++g) *reinterpret_cast<f32x4*>(wslot + 8 * g * GEMM_LDS_STRIDE) = wcr[sg][g];
        table_stage_handoff();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(afrag + 32 * sg + 8 * q);
            f32x4 bv[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const f32x4*>(wfrag + j * 32 * GEMM_LDS_STRIDE + 8 * q);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[j][kk], acc[j], 0, 0, 0);
        }
        table_stage_handoff();
    }
    prof.lap(3);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = cg * TBL_BN + wid * 64 + j * 32 + r;
        const bool hi = n >= a.split_n;                 // (wave-uniform: split_n % 32 == 0)
        const int c = hi ? n - a.split_n : n, ldy = hi ? a.N - a.split_n : a.split_n;
        const float bias = biasc[j];
        float* col = (hi ? a.xr : a.xl) + c;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + 4 * h + (e & 3) + 8 * (e >> 2);
            if (m < T) col[(size_t)m * ldy] = acc[j][e] + bias;
        }
    }
    prof.wait_vmem();
    prof.lap(4);
    prof.since(5, item_start);
    prof.add(6, 1);
    prof.flush(g_table_prof, tid == 0);
}

// the table alone (mel_feature_tables_fused)
__global__ __launch_bounds__(256, 2) void table_fused_kernel(TableArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[TBL_LDS_FLOATS];
    table_fused_tile(a, (int)blockIdx.x, lds);
}

}  // namespace mel
