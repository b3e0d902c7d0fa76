// Host-side GEMM dispatch of the forward: plan_gemm decides which kernel computes a launch, on which tiles and how many
// workgroups (no side effects), launch_plan launches what it decided.  Every rule that picks a kernel lives in plan_gemm.
#pragma once
#include <cstdarg>
#include <cstdlib>
#include <type_traits>
#include "gemm_f32.hpp"
#include "gemm_bf16.hpp"
#include "gemm_split.hpp"
#include "gemm_ring.hpp"
#include "gemm_table.hpp"

namespace mel {

#ifndef MEL_PLANES_FROM
#define MEL_PLANES_FROM 129          // expected 128 x 256 work items from which conv2 runs on gemm_planes_kernel: up to 256 tiles of
                                     // 128 x 128 the older kernel has a CU per tile (32 us), beyond it doubles up (42 us at 288); this one
                                     // takes 33 us for anything up to 256 items
#endif
#ifndef MEL_SPLIT_BIG_FROM
#define MEL_SPLIT_BIG_FROM 192       // expected 128 x 128 tiles from which the split path takes gemm_split_big_kernel
#endif

// A/B switches for benchmarks and tests, read once per process: MEL_NO_PLANES_GEMM keeps conv2 off
// gemm_planes_kernel, MEL_PLANES_FROM moves the launch size from which it is taken, MEL_NO_BF16_WIDE keeps the bf16 feature
// path's large projections off gemm_bf16_wide_kernel, MEL_NO_FUSED_TABLE evaluates the node-feature table of a forward in two
// launches (encoder tiles beside the row lists, then conv1's projections) instead of inside the plan launch (gemm_table.hpp).
struct GemmTuning { bool no_planes; long planes_from; bool no_bf16_wide; bool no_fused_table; };
static const GemmTuning& gemm_tuning() {
    static const GemmTuning t{getenv("MEL_NO_PLANES_GEMM") != nullptr,
                              getenv("MEL_PLANES_FROM") ? atol(getenv("MEL_PLANES_FROM")) : (long)MEL_PLANES_FROM,
                              getenv("MEL_NO_BF16_WIDE") != nullptr, getenv("MEL_NO_FUSED_TABLE") != nullptr};
    return t;
}

enum class GemmKernel {
    NONE,               // nothing to launch (no rows)
    F32,                // gemm_f32_kernel: one workgroup per 64 x 64 or 128 x 128 tile
    F32_PERSISTENT,     // gemm_f32_persistent_kernel: a fixed grid walks the 64 x 64 (or 64 x 128) tiles
    RING,               // gemm_f32_ring_kernel (gemm_ring.hpp): specialised loader / MFMA wavefronts, 64 x 64
    BF16,               // gemm_bf16_kernel: persistent, 64 x 64, 64 x 128 or 128 x 128
    SPLIT,              // gemm_split_kernel: split-bf16 products, persistent 64 x 64
    SPLIT_BIG,          // gemm_split_big_kernel: split-bf16 products, 128 x 128
    PLANES,             // gemm_planes_kernel: split-bf16 products with both operands as plane blocks, 128 x 256
    BF16_WIDE,          // gemm_bf16_wide_kernel: bf16 rows on both sides, 128 x 256
};

struct GemmPlan {
    mel_status status = MEL_OK;     // != MEL_OK: the shape was rejected for the reason in `why`
    char why[200] = "";
    GemmKernel kernel = GemmKernel::NONE;
    int mode = GEMM_MODE_PLAIN;
    int tm = 1, tn = 1;             // F32, F32_PERSISTENT, BF16: tiles of 64 TM x 64 TN
    int ksplit = 1;                 // > 1: K is cut into this many chunks whose raw products go to planes (launch_splitk_finish)
    GemmBatch batch{};              // the problems as launched
    int grid = 0, block = 0;

    GemmPlan& reject(mel_status code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, sizeof(why), fmt, ap);
        va_end(ap);
        kernel = GemmKernel::NONE, status = code;
        return *this;
    }
};

// conv2's projection weights in gemm_planes_kernel's block layout (fwd.hip: conv2_blocks_fit)
struct PlaneBlocks {
    const float* W = nullptr;
    const float* W_hi = nullptr;
};

// What a call asks of the planner beyond the problems themselves.
struct GemmRequest {
    int mode = GEMM_MODE_PLAIN;
    int force_tile = MEL_TILE_AUTO;         // the mel_gemm_* entry points' tile codes (melissa_hip.h)
    bool group = false;                     // several problems in one launch: launch_gemm_group's rules below
    int max_ksplit = 1;                     // one problem: the planner may cut K into up to this many chunks...
    int ksplit = 0;                         // ... or exactly this many (>= 2)
    float* parts = nullptr;                 // split-K: chunk s writes its raw products to parts + s * part_stride
    long part_stride = 0;
    const PlaneBlocks* blocks = nullptr;    // group: every problem's weights as plane blocks (conv2 only)
};

// The rows a launch is expected to cover (ragged lists are sized on the device; the grid still covers M rows)
static long expected_rows(const GemmArgs& g, const long* hints, int i) {
    return (hints && hints[i] >= 0 && hints[i] <= g.M) ? hints[i] : g.M;
}

static mel_status check_gemm_shape(const GemmArgs& g, GemmPlan& p) {
    if (g.split && g.K < 128) return p.reject(MEL_ERR_UNSUPPORTED, "the split path needs K >= 128 (K=%d)", g.K).status;
    const int bk = g.bf16 ? GEMB_BK : GEMM_BK;
    if (g.K % bk != 0 || g.N % 64 != 0)
        return p.reject(MEL_ERR_UNSUPPORTED, "GEMM needs K %% %d == 0 and N %% 64 == 0 (K=%d N=%d)", bk, g.K, g.N).status;
    if (g.bf16 && (g.lda % 8 != 0 && g.A))
        return p.reject(MEL_ERR_UNSUPPORTED, "bf16 GEMM needs lda %% 8 == 0 (lda=%d)", g.lda).status;
    return MEL_OK;
}

// 128 x 128 split tiles (gemm_split_big_kernel): PLAIN mode, every N a multiple of 128
static bool split_big_fits(const GemmArgs* gs, int count, int mode) {
    if (mode != GEMM_MODE_PLAIN) return false;
    for (int i = 0; i < count; ++i) {
        const int S = gs[i].ksplit > 1 ? gs[i].ksplit : 1;
        if (gs[i].N % 128 || gs[i].K % (GEMS2_BK * S) || gs[i].K / GEMS2_BK / S < 4 || gs[i].lda % 4) return false;
    }
    return true;
}

// gemm_planes_kernel (gemm_split.hpp): A as [rows][K / 16][3][16] bf16 planes, W / W_hi as [N / 256][K / 16][256][3][16]
static bool planes_fit(const GemmArgs* gs, int count) {
    long ncols = 0;
    for (int i = 0; i < count; ++i) {
        const GemmArgs& g = gs[i];
        if (g.N % GEMP_BN || g.K % GEMS2_BK || g.K / GEMS2_BK < 4 || g.ldy % 4 || g.rscale || g.ksplit > 1) return false;
        if (g.W_hi && g.split_n % GEMP_BN) return false;
        if ((size_t)g.M * (size_t)g.K * 6 >= ((size_t)1 << 32)) return false;      // 32-bit operand offsets
        ncols += g.N;
    }
    return count >= 1 && count <= GEMM_MAX_GROUP && ncols <= GEMP_BIAS_FLOATS;
}

// gemm_bf16_wide_kernel (gemm_split.hpp): bf16 rows on both sides, 128 x 256 tiles, 64-k stages
static bool bf16_wide_fit(const GemmArgs* gs, int count) {
    long ncols = 0;
    for (int i = 0; i < count; ++i) {
        const GemmArgs& g = gs[i];
        if (!g.bf16 || !g.A || g.N % GEMP_BN || g.K % GEMW_BK || g.K / GEMW_BK < 2 || g.lda % 8 || g.rscale || g.ksplit > 1) return false;
        if (g.W_hi && g.split_n % GEMP_BN) return false;
        if ((size_t)g.M * (size_t)g.lda * 2 >= ((size_t)1 << 32) || (size_t)GEMP_BN * g.K * 2 >= ((size_t)1 << 32)) return false;
        ncols += g.N;
    }
    return count >= 1 && count <= GEMM_MAX_GROUP && ncols <= GEMP_BIAS_FLOATS;
}

// Skinny long-K problems (the dueling heads' first layer: 4 820 x 256 outputs over K = 1 152 are 304 tiles of 64 x 64 for
// 512 workgroup slots, one 36-step tile each and half of the slots empty): cut K into S chunks so that the work items
// fill the chip evenly.  Chunk s writes raw partial products to plane s of `parts`; splitk_finish_kernel sums the planes
// in order and applies scale / bias / ReLU.  Model of the launch in K steps of one workgroup: (workgroups sharing a
// CU) x (items per workgroup) x (steps per item + hand-over), over the slots of the kernel that runs the chunks:
//   fp32: the ring kernel, 64 x 64 tiles, 512 slots (two workgroups per CU), steps of 32 k, 2 steps of hand-over (the
//         hand-over buffer needs two steps between tiles);
//   split: the 128 x 128 split kernel, 512 slots (two per CU), steps of 16 k, ~4 steps of hand-over per work item - and
//          only from MEL_SPLIT_BIG_FROM work items on;
//   bf16: the one-role kernel, 64 x 64 tiles, 1 024 slots, latency bound at these sizes - items per slot x (steps per
//         item + 2), whatever the workgroups sharing a CU.
static int choose_ksplit(const GemmArgs& g, long m_hint, int max_split) {
    if (g.K < 512 || g.ldy % 4 || g.N % 64 || g.K % GEMB_BK) return 1;
    if (g.split && (g.N % 128 || g.lda % 4)) return 1;
    const bool bf = g.bf16 && !g.split;
    const int tile = g.split ? 128 : 64, KT = g.K / (g.split ? GEMS2_BK : bf ? GEMB_BK : GEMM_BK);
    const int hand_over = g.split ? 4 : 2;          // steps; also the fewest steps a chunk may have
    const long tiles = ((m_hint + tile - 1) / tile) * (g.N / tile), max_slots = bf ? 1024 : 512;
    int best = 1;
    long best_cost = 0;
    for (int S = 1; S <= max_split; ++S) {
        if (KT % S || KT / S < hand_over) continue;
        const long items = tiles * S, slots = items < max_slots ? items : max_slots, sharing = bf ? 1 : (slots + 255) / 256;
        const long cost = sharing * ((items + slots - 1) / slots) * (KT / S + hand_over);
        if (S == 1 || cost < best_cost) best = S, best_cost = cost;
    }
    return !g.split || best * tiles >= MEL_SPLIT_BIG_FROM ? best : 1;
}

// The plan of `kernel` on the problems: packs them into the batch and sizes the grid.  A kernel either runs one workgroup
// per work item (per_cu == 0) or is persistent: per_cu workgroups on each of the 256 CUs, never more than there are items.
// Every problem's items start at a multiple of 8, which keeps each tile id on its XCD (ids are dealt to the 8 XCDs in turn).
static GemmPlan& choose(GemmPlan& p, GemmKernel kernel, int mode, const GemmArgs* gs, int count, int tm = 1, int tn = 1) {
    constexpr int LDS = 160 * 1024;
    p.kernel = kernel, p.mode = mode, p.tm = tm, p.tn = tn;
    int bm = 64 * tm, bn = 64 * tn, per_cu = 0;
    bool by_ksplit = false;                 // a work item is one K chunk of a tile
    p.block = 256;
    switch (kernel) {
        case GemmKernel::F32: break;
        case GemmKernel::F32_PERSISTENT: {  // as many workgroups as the LDS of a CU holds, at most 4
            const int lds_wg = (bm + bn) * GEMM_LDS_STRIDE * 4 * 2;
            per_cu = LDS / lds_wg > 4 ? 4 : LDS / lds_wg;
            break;
        }
        case GemmKernel::RING:
            bm = RingCfg<GEMM_BK>::BM, bn = RingCfg<GEMM_BK>::BN, per_cu = RingCfg<GEMM_BK>::WG_PER_CU, by_ksplit = true;
            p.block = RingCfg<GEMM_BK>::THREADS;
            break;
        case GemmKernel::BF16: {
            const int lds_wg = (bm + bn) * GEMB_ROW * 16 * 2;
            per_cu = LDS / lds_wg > 4 ? 4 : LDS / lds_wg, by_ksplit = true;
            break;
        }
        case GemmKernel::SPLIT: per_cu = 3; break;                             // 53 KB of LDS per workgroup
        case GemmKernel::SPLIT_BIG: bm = bn = 128, per_cu = 2, by_ksplit = true; break;
        case GemmKernel::PLANES:
        case GemmKernel::BF16_WIDE: bm = 128, bn = GEMP_BN, per_cu = 1, p.block = 768; break;     // 146 KB of LDS
        case GemmKernel::NONE: return p;
    }
    GemmBatch& b = p.batch;
    b = GemmBatch{};
    b.count = count;
    long items = 0;
    for (int i = 0; i < count; ++i) {       // the ids the kernels walk (gemm_walk.hpp), for the rows the grid covers
        b.p[i] = gs[i], b.start[i] = (int)items;
        items += gemm_pad_items(gemm_items((long)gs[i].M, gs[i].N, bm, bn, by_ksplit ? gs[i].ksplit : 1));
    }
    b.start[count] = (int)items;
    p.grid = (int)(per_cu && items > 256L * per_cu ? 256L * per_cu : items);
    return p;
}

// Picks the kernel of a launch.  A call is one problem (launch_gemm: any mode, the entry points' tile codes), a group of
// PLAIN problems (launch_gemm_group) or one problem cut along K (split-K, into rq.parts).
static GemmPlan plan_gemm(const GemmArgs* gs, const long* hints, int count, const GemmRequest& rq) {
    GemmPlan p;
    if (rq.group && (count < 1 || count > GEMM_MAX_GROUP)) return p.reject(MEL_ERR_INVALID_ARG, "group of %d", count);
    GemmArgs a[GEMM_MAX_GROUP];             // the problems as they will be launched
    long big = 0, wide = 0;                 // expected 128 x 128 tiles, 128 x 256 work items
    bool n128 = true, long_k = true, ragged = false;
    for (int i = 0; i < count; ++i) {
        a[i] = gs[i];
        if (a[i].M <= 0) {
            if (rq.group) p.reject(MEL_ERR_INVALID_ARG, "empty problem in group");
            return p;
        }
        if (check_gemm_shape(a[i], p)) return p;
        const long h = expected_rows(a[i], hints, i);
        big += ((h + 127) / 128) * (a[i].N / 128);
        wide += ((h + 127) / 128) * (a[i].N / GEMP_BN);
        n128 = n128 && a[i].N % 128 == 0;
        long_k = long_k && a[i].K >= 512;
        ragged = ragged || a[i].M_dev != nullptr;
    }
    GemmArgs& g = a[0];
    const long m_hint = expected_rows(g, hints, 0);
    const int force = rq.force_tile;
    const GemmTuning& tune = gemm_tuning();

    int S = rq.ksplit;
    if (rq.max_ksplit > 1) {
        S = choose_ksplit(g, m_hint, rq.max_ksplit);
        if (g.Ws && (!g.W_hi || g.Ws_hi) && !g.split && !g.bf16) {
            // MEL_PREC_F32_AUTO (the heads' first layer): the split kernel when its work items fill the chip
            GemmArgs t = g;
            t.W = g.Ws, t.W_hi = g.W_hi ? g.Ws_hi : nullptr, t.split = 1;
            const int St = choose_ksplit(t, m_hint, rq.max_ksplit);
            const long tiles = ((m_hint + 127) / 128) * (t.N / 128);
            t.ksplit = St > 1 ? St : 0;
            if ((St > 1 || tiles >= MEL_SPLIT_BIG_FROM) && split_big_fits(&t, 1, GEMM_MODE_PLAIN)) {
                t.ksplit = 0;
                g = t, S = St;
            }
        }
    }
    if (S > 1) {
        const int bk = g.bf16 ? GEMB_BK : g.split ? GEMS2_BK : GEMM_BK;
        if ((g.K / bk) % S || !rq.parts || rq.part_stride < (long)g.M * g.N)
            return p.reject(MEL_ERR_INVALID_ARG, "bad split-K request (S=%d)", S);
        g.Y = rq.parts, g.ldy = g.N, g.ksplit = S, g.part_stride = rq.part_stride;
        p.ksplit = S;
        if (g.split) {
            if (!split_big_fits(&g, 1, GEMM_MODE_PLAIN)) return p.reject(MEL_ERR_UNSUPPORTED, "shape does not fit the 128 x 128 split tile");
            return choose(p, GemmKernel::SPLIT_BIG, GEMM_MODE_PLAIN, a, 1);
        }
        if (g.bf16) {
            g.y_f32 = 1;
            return choose(p, GemmKernel::BF16, GEMM_MODE_PLAIN, a, 1);
        }
        return choose(p, GemmKernel::RING, GEMM_MODE_PLAIN, a, 1);
    }

    if (rq.blocks && !tune.no_planes && wide >= tune.planes_from) {
        // conv2 on gemm_planes_kernel (both operands as bf16 plane blocks): large launches of the fp32-accurate paths only, a
        // launch of fewer work items than CUs stays on the 128 x 128 / 64 x 64 kernels
        GemmArgs t[GEMM_MAX_GROUP];
        bool fit = true;
        for (int i = 0; i < count; ++i) {
            t[i] = a[i];
            fit = fit && !a[i].bf16 && rq.blocks[i].W && (!a[i].W_hi || rq.blocks[i].W_hi);
            t[i].W = rq.blocks[i].W, t[i].W_hi = a[i].W_hi ? rq.blocks[i].W_hi : nullptr, t[i].split = 1;
        }
        if (fit && planes_fit(t, count)) return choose(p, GemmKernel::PLANES, GEMM_MODE_PLAIN, t, count);
    }
    if (rq.group && !g.split && !g.bf16 && big >= MEL_SPLIT_BIG_FROM) {
        // MEL_PREC_F32_AUTO: every problem carries the bf16 planes of its weights and the launch is large enough for the
        // 128 x 128 split kernel to win (conv2 in the L-DGN step: 52 against 83 us) - same fp32-accurate results
        GemmArgs t[GEMM_MAX_GROUP];
        bool alt = true;
        for (int i = 0; i < count; ++i) {
            t[i] = a[i];
            alt = alt && a[i].Ws && !a[i].split && !a[i].bf16 && (!a[i].W_hi || a[i].Ws_hi);
            t[i].W = a[i].Ws, t[i].W_hi = a[i].W_hi ? a[i].Ws_hi : nullptr, t[i].split = 1;
        }
        if (alt && split_big_fits(t, count, GEMM_MODE_PLAIN)) return choose(p, GemmKernel::SPLIT_BIG, GEMM_MODE_PLAIN, t, count);
    }
    if (rq.group)       // (whichever member comes first: the kernels below read every W of a launch in ONE format)
        for (int i = 1; i < count; ++i)
            if (!a[i].split != !g.split || !a[i].bf16 != !g.bf16) return p.reject(MEL_ERR_INVALID_ARG, "mixed precisions in one group");

    if (g.split) {      // a persistent 64 x 64 kernel for small launches, 128 x 128 tiles from MEL_SPLIT_BIG_FROM expected tiles on
        if (force == MEL_TILE_WIDE) {
            if (!planes_fit(a, count)) return p.reject(MEL_ERR_UNSUPPORTED, "shape does not fit the 128 x 256 planes kernel");
            return choose(p, GemmKernel::PLANES, GEMM_MODE_PLAIN, a, count);
        }
        if (force == MEL_TILE_128 && !split_big_fits(a, count, rq.mode))
            return p.reject(MEL_ERR_UNSUPPORTED, "shape does not fit the 128 x 128 split tile");
        const bool big_tile = force == MEL_TILE_128 || (force != MEL_TILE_64 && big >= MEL_SPLIT_BIG_FROM);
        if (big_tile && split_big_fits(a, count, rq.mode)) return choose(p, GemmKernel::SPLIT_BIG, GEMM_MODE_PLAIN, a, count);
        return choose(p, GemmKernel::SPLIT, rq.mode, a, count);
    }
    // encoder (ENC producer): a 64 x 128 tile spans the whole hidden width, so the first layer (VALU work inside the
    // A-tile producer) is evaluated once per row instead of once per 64-column tile
    // (fp32: the wide tile wins from about 20 000 rows - HL-DGN's 25 600: 24.8 -> 19.9 us - and loses below - L-DGN's
    // 16 000: 17 -> 19 us)
    const bool enc_wide = rq.mode == GEMM_MODE_ENC && force == MEL_TILE_AUTO && g.N % 128 == 0 && (g.bf16 || m_hint >= 20000);
    if (g.bf16) {       // the bf16 feature path: persistent launches for every case (ragged or not)
        if (rq.group) {
            // large launches: 128 x 256 tiles (conv2 of the bf16 feature path: 97 MB of operands through the L2 instead of 0.5 GB)
            if (!tune.no_bf16_wide && wide >= MEL_PLANES_FROM && bf16_wide_fit(a, count))
                return choose(p, GemmKernel::BF16_WIDE, GEMM_MODE_PLAIN, a, count);
            return choose(p, GemmKernel::BF16, GEMM_MODE_PLAIN, a, count);
        }
        if (force == MEL_TILE_WIDE) {
            if (rq.mode != GEMM_MODE_PLAIN || !bf16_wide_fit(a, 1))
                return p.reject(MEL_ERR_UNSUPPORTED, "shape does not fit the 128 x 256 bf16 kernel (N %% 256, K %% 64, lda %% 8)");
            return choose(p, GemmKernel::BF16_WIDE, GEMM_MODE_PLAIN, a, 1);
        }
        if (force == MEL_TILE_128 && g.N % 128 == 0) return choose(p, GemmKernel::BF16, rq.mode, a, 1, 2, 2);
        return choose(p, GemmKernel::BF16, rq.mode, a, 1, 1, enc_wide ? 2 : 1);
    }
    if (enc_wide) return choose(p, GemmKernel::F32_PERSISTENT, rq.mode, a, 1, 1, 2);
    if (force == MEL_TILE_64_RING && rq.mode == GEMM_MODE_PLAIN && g.ldy % 4 == 0 && g.K >= 64)
        return choose(p, GemmKernel::RING, GEMM_MODE_PLAIN, a, 1);
    if (force == MEL_TILE_64) return choose(p, GemmKernel::F32, rq.mode, a, 1);
    if (force >= MEL_TILE_128 && g.N % 128 == 0) {
        if (force == MEL_TILE_128) return choose(p, GemmKernel::F32, rq.mode, a, 1, 2, 2);
        if (force == MEL_TILE_64_PERSISTENT) return choose(p, GemmKernel::F32_PERSISTENT, rq.mode, a, 1);
        return p.reject(MEL_ERR_INVALID_ARG, "unknown tile %d", force);
    }
    if (ragged) {       // device-side row counts: a fixed grid walks the tiles instead of a worst-case grid exiting
        // Long-K problems (the heads' first layer, K = 1152: 36 K steps per tile) go to the specialised-wavefront kernel:
        // measured 27.4 vs 30.7 us for the head launches; at K <= 512 the one-role kernel is as fast or faster
        // (conv2 84 vs 85 us, conv1 46 vs 53 us), see NOTES.md.
        bool ring = rq.mode == GEMM_MODE_PLAIN;
        for (int i = 0; i < count; ++i) ring = ring && a[i].K >= 1024 && a[i].ldy % 4 == 0;
        return choose(p, ring ? GemmKernel::RING : GemmKernel::F32_PERSISTENT, rq.mode, a, count);
    }
    // Measured (tools/gemm_bench.py): the 64x64 tile (4x the workgroups, a quarter of the per-wave MFMA
    // chain, 4 workgroups per CU) wins or ties everywhere except long-K problems with thousands of tiles.
    if (n128 && long_k && big >= 1536) return choose(p, GemmKernel::F32, rq.mode, a, count, 2, 2);
    return choose(p, GemmKernel::F32, rq.mode, a, count);
}

using GemmKernelFn = void (*)(GemmBatch);

// The instantiation of a kernel for a call-site tag (the tag only names launches apart in traces and profiles): the
// tags listed exist, any other tag gets the first of them.
template <int FIRST, int... REST, class F>
static GemmKernelFn tagged(int tag, F kernel_of) {
    GemmKernelFn k = kernel_of(std::integral_constant<int, FIRST>{});
    (void)((tag == REST && (k = kernel_of(std::integral_constant<int, REST>{}))) || ...);
    return k;
}

static mel_status launch_plan(const GemmPlan& p, hipStream_t s, int tag, const char* what) {
    if (p.status) return fail(p.status, "%s: %s", what, p.why);
    const bool enc = p.mode == GEMM_MODE_ENC;
    GemmKernelFn k = nullptr;
    switch (p.kernel) {
        case GemmKernel::NONE: return MEL_OK;
        case GemmKernel::F32:
            if (p.tm == 2) k = enc ? gemm_f32_kernel<2, 2, 2, 2, GEMM_MODE_ENC> : gemm_f32_kernel<2, 2, 2, 2, GEMM_MODE_PLAIN>;
            else k = enc ? gemm_f32_kernel<2, 2, 1, 1, GEMM_MODE_ENC> : gemm_f32_kernel<2, 2, 1, 1, GEMM_MODE_PLAIN>;
            break;
        case GemmKernel::F32_PERSISTENT:
            if (p.tn == 2)
                k = enc ? gemm_f32_persistent_kernel<2, 2, 1, 2, GEMM_MODE_ENC> : gemm_f32_persistent_kernel<2, 2, 1, 2, GEMM_MODE_PLAIN>;
            else if (enc) k = gemm_f32_persistent_kernel<2, 2, 1, 1, GEMM_MODE_ENC>;
            else k = tagged<0, 1, 2, 3>(tag, [](auto t) -> GemmKernelFn {
                return gemm_f32_persistent_kernel<2, 2, 1, 1, GEMM_MODE_PLAIN, decltype(t)::value>; });
            break;
        case GemmKernel::RING:
            k = tagged<0, 1, 2, 3>(tag, [](auto t) -> GemmKernelFn { return gemm_f32_ring_kernel<decltype(t)::value>; });
            break;
        case GemmKernel::BF16:
            if (p.tm == 2) k = enc ? gemm_bf16_kernel<2, 2, 2, 2, GEMM_MODE_ENC> : gemm_bf16_kernel<2, 2, 2, 2, GEMM_MODE_PLAIN>;
            else if (p.tn == 2) k = enc ? gemm_bf16_kernel<2, 2, 1, 2, GEMM_MODE_ENC> : gemm_bf16_kernel<2, 2, 1, 2, GEMM_MODE_PLAIN>;
            else k = enc ? gemm_bf16_kernel<2, 2, 1, 1, GEMM_MODE_ENC> : gemm_bf16_kernel<2, 2, 1, 1, GEMM_MODE_PLAIN>;
            break;
        case GemmKernel::SPLIT:
            k = tagged<0, 1, 2, 3>(tag, [enc](auto t) -> GemmKernelFn {
                return enc ? gemm_split_kernel<GEMM_MODE_ENC, decltype(t)::value> : gemm_split_kernel<GEMM_MODE_PLAIN, decltype(t)::value>; });
            break;
        case GemmKernel::SPLIT_BIG:
            k = tagged<0, 2, 3>(tag, [](auto t) -> GemmKernelFn { return gemm_split_big_kernel<decltype(t)::value>; });
            break;
        case GemmKernel::PLANES:
            k = tagged<0, 2>(tag, [](auto t) -> GemmKernelFn { return gemm_planes_kernel<decltype(t)::value>; });
            break;
        case GemmKernel::BF16_WIDE:
            k = tagged<0, 2>(tag, [](auto t) -> GemmKernelFn { return gemm_bf16_wide_kernel<decltype(t)::value>; });
            break;
    }
    MEL_LAUNCH(k, dim3(p.grid), dim3(p.block), 0, s, p.batch);
    return check_launch(what);
}

// After a split-K plan: sums the chunks' planes in order into g.Y and applies scale / bias / ReLU (g: the problem as the
// caller gave it)
static mel_status launch_splitk_finish(const GemmArgs& g, const GemmPlan& p, long m_hint, hipStream_t s, const char* what) {
    const GemmArgs& q = p.batch.p[0];
    SplitKFinish f{q.Y, q.part_stride, q.ksplit, g.N, g.M, g.M_dev, g.bias, g.bias_hi, g.split_n, g.rscale, g.relu, g.Y, g.ldy};
    if (m_hint < 0 || m_hint > g.M) m_hint = g.M;
    long blocks = (m_hint * (g.N / 4) + 255) / 256;
    blocks = blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks;
    MEL_LAUNCH(splitk_finish_kernel, dim3((int)blocks), dim3(256), 0, s, f);
    return check_launch(what);
}

// One problem.  `m_hint` is the row count the caller expects (-1: g.M).
static mel_status launch_gemm(const GemmArgs& g, int mode, hipStream_t s, const char* what, long m_hint = -1,
                              int force_tile = MEL_TILE_AUTO, int tag = 0) {
    GemmRequest rq;
    rq.mode = mode, rq.force_tile = force_tile;
    return launch_plan(plan_gemm(&g, &m_hint, 1, rq), s, tag, what);
}

// Several PLAIN problems in one launch; hints[i] = expected rows of problem i (-1 = g.M).
static mel_status launch_gemm_group(const GemmArgs* gs, const long* hints, int count, hipStream_t s, const char* what, int tag) {
    GemmRequest rq;
    rq.group = true;
    return launch_plan(plan_gemm(gs, hints, count, rq), s, tag, what);
}

// One problem, K cut into exactly S chunks, the planes summed afterwards
static mel_status launch_gemm_splitk(const GemmArgs& g, int S, float* parts, long part_stride, hipStream_t s, const char* what) {
    GemmRequest rq;
    rq.ksplit = S, rq.parts = parts, rq.part_stride = part_stride;
    const long m_hint = -1;
    const GemmPlan p = plan_gemm(&g, &m_hint, 1, rq);
    if (mel_status st = launch_plan(p, s, 0, what)) return st;
    return p.ksplit > 1 ? launch_splitk_finish(g, p, m_hint, s, what) : MEL_OK;
}

}  // namespace mel
