// The work-item walk of the GEMM kernels: which work item does workgroup id t own.  One definition for the host (choose(),
// gemm_launch.hpp, which sizes the grid) and for every kernel (gemm_f32_tile and the seven persistent kernels).
//
//   * a problem's work items are its row tiles x column tiles x K chunks (gemm_items), ordered row panel by row panel and
//     chunk-major inside a panel, so that the items sharing an A chunk are neighbours;
//   * the ids of one problem are padded to a multiple of 8 (gemm_pad_items), the problems of a launch follow each other:
//     id % 8 - the XCD under round-robin dispatch, every grid being a multiple of 8 - then means "same XCD" in each of them;
//   * inside a problem the ids are permuted so that an A row panel stays on one XCD (xcd_panel_order).
//
// The row counts may be ragged and live on the device (GemmArgs::M_dev), so the persistent kernels build their tables from
// them (walk_tables) rather than take the host's prefix.  The tables are the KERNEL's local arrays, handed to free functions
// by reference: every index is a compile-time constant after unrolling and they stay in scalar registers.  (Gathered into one
// struct they went to scratch - 64 bytes per lane in gemm_planes_kernel - whether indexed dynamically or by select chains.)
//
// Included by gemm_f32.hpp below the definitions of GemmArgs and GemmBatch.
#pragma once

namespace mel {

// (I: int in the kernels, long where the host sums the grid of a launch)
template <class I>
__host__ __device__ constexpr I gemm_items(I rows, int N, int BM, int BN, int ksplit) {
    return ((rows + BM - 1) / BM) * (N / BN) * (ksplit > 1 ? ksplit : 1);
}
template <class I>
__host__ __device__ constexpr I gemm_pad_items(I items) { return (items + 7) & ~(I)7; }

// Only the first `active` ids of a problem have work (the dispatcher deals consecutive ids round-robin over the 8 XCDs, so they
// are spread evenly).  Inside that range ids are remapped, bijectively, so that the workgroups sharing an A row panel (same m
// tile, different n tile or K chunk) sit on one XCD's L2: XCD x takes a contiguous run of q or q + 1 items.
__device__ __forceinline__ int xcd_panel_order(int wg, int active) {
    const int q = active >> 3, r8 = active & 7, xcd = wg & 7, local = wg >> 3;
    return (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + local;
}

__device__ __forceinline__ int gemm_rows(const GemmArgs& g) { return g.M_dev ? min(*g.M_dev, g.M) : g.M; }

// Per problem: live rows, work items, and the padded prefix of the items (pre[GEMM_MAX_GROUP] = ids of the whole launch).
// SPLITK: the kernel takes GemmArgs::ksplit (a work item is one K chunk of a tile).
template <int BM, int BN, bool SPLITK>
__device__ __forceinline__ void walk_tables(const GemmBatch& batch, int (&act)[GEMM_MAX_GROUP], int (&pre)[GEMM_MAX_GROUP + 1],
                                            int (&rows)[GEMM_MAX_GROUP]) {
    pre[0] = 0;
#pragma unroll
    for (int i = 0; i < GEMM_MAX_GROUP; ++i) {
        act[i] = 0, rows[i] = 0;
        if (i < batch.count) {
            const GemmArgs& q = batch.p[i];
            rows[i] = gemm_rows(q);
            act[i] = gemm_items(rows[i], q.N, BM, BN, SPLITK ? q.ksplit : 1);
        }
        pre[i + 1] = pre[i] + gemm_pad_items(act[i]);
    }
}

// the problem id t belongs to
__device__ __forceinline__ int walk_problem(int t, const int (&pre)[GEMM_MAX_GROUP + 1]) {
    int pi = 0;
#pragma unroll
    for (int k = 1; k < GEMM_MAX_GROUP; ++k)
        if (t >= pre[k]) pi = k;
    return pi;
}

// first id with work among t, t + stride, ... (skips the per-problem padding); the launch's total when there is none
__device__ __forceinline__ int walk_next_valid(int t, int stride, const int (&act)[GEMM_MAX_GROUP],
                                               const int (&pre)[GEMM_MAX_GROUP + 1]) {
    const int total = pre[GEMM_MAX_GROUP];
    for (; t < total; t += stride) {
        const int pi = walk_problem(t, pre);
        if (t - pre[pi] < act[pi]) return t;
    }
    return total;
}

// Work item t: rows m0 .. m0 + BM - 1 (M of them live) by columns n0 .. of problem pi, K chunk ks of S.  A kernel derives its
// K steps per item and first K column from S, ks and its own K step.
struct WorkItem {
    int pi, m0, n0, M, ks, S;
};
template <int BM, int BN, bool SPLITK>
__device__ __forceinline__ WorkItem walk_item(const GemmBatch& batch, int t, const int (&act)[GEMM_MAX_GROUP],
                                              const int (&pre)[GEMM_MAX_GROUP + 1], const int (&rows)[GEMM_MAX_GROUP]) {
    const int pi = walk_problem(t, pre);
    const GemmArgs& g = batch.p[pi];
    const int nbn = g.N / BN;
    const int wg = xcd_panel_order(t - pre[pi], act[pi]);
    const int S = SPLITK && g.ksplit > 1 ? g.ksplit : 1;
    return WorkItem{pi, (wg / (nbn * S)) * BM, (wg % nbn) * BN, rows[pi], (wg / nbn) % S, S};
}

}  // namespace mel
