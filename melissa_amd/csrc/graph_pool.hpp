// Connected random geometric graphs on the device: the training-graph dataset recipe of graph_env/env/utils/core.py:440-447
// (nx.random_geometric_graph(n, radius, seed=s) for s = first_seed, first_seed + 1, ..., keeping the connected ones), bit for
// bit what melissa_amd/env/episodes.py's packed_graph_pool computes on the host.
//
// Included by env.hip after episode_stream.hpp (it uses that file's MT19937 pieces).  Three launches per chunk of candidates:
//   graph_pool_candidate_kernel  one wavefront (a 64-thread workgroup) per candidate seed: random.Random(s) draws the 2N
//                                positions, the float64 radius rule gives the adjacency sets, a frontier search from node 0
//                                decides; an accepted candidate stages its graph in the workspace and raises its flag
//   graph_pool_scan_kernel       one workgroup: flags -> output slots in ascending seed order, starting at *count and ending
//                                at capacity; advances *count
//   graph_pool_write_kernel      one wavefront per candidate: staged graph -> its output slot
// The result depends on the seeds alone: not on the grid, the chunk size or the order in which wavefronts finish.
//
// CPython's random.Random(s) for an int 0 <= s < 2^32 (Modules/_randommodule.c: random_seed -> init_by_array with the one-word
// key [s]; s = 0 also takes a one-word key):
//   mt = init_genrand(19650218)                                           (does not depend on s: GP_INIT below)
//   i = 1; 624 times: mt[i] = (mt[i] ^ ((mt[i-1] ^ (mt[i-1] >> 30)) * 1664525)) + s + 0;     i++, wrap: mt[0] = mt[623], i = 1
//          623 times: mt[i] = (mt[i] ^ ((mt[i-1] ^ (mt[i-1] >> 30)) * 1566083941)) - i;      i++, same wrap
//   mt[0] = 0x80000000
//   random() = genrand_res53: ((a >> 5) * 2^26 + (b >> 6)) / 2^53 from two consecutive tempered outputs (mt_double)
// so loop 1 walks i = 1 .. 623 and then i = 1 once more (on top of its own first result, with mt[0] = mt[623]), and loop 2
// walks i = 2 .. 623 and then i = 1.
#pragma once

namespace mel {

constexpr int GRAPH_POOL_MAX_CANDIDATES = 1 << 30;       // per call: candidate indices and their sums stay inside int32

struct GpInit {
    uint32_t w[624];
};
constexpr GpInit gp_init_genrand(uint32_t s) {
    GpInit t{};
    t.w[0] = s;
    for (int i = 1; i < 624; ++i) t.w[i] = 1812433253u * (t.w[i - 1] ^ (t.w[i - 1] >> 30)) + (uint32_t)i;
    return t;
}
__constant__ const GpInit GP_INIT = gp_init_genrand(19650218u);

// Both seeding loops are serial and wave-uniform, so they run on the scalar unit like mt_seed: the chain lives in SGPRs, the
// table word comes from constant memory by a scalar load, lane (i - 1) % 64 of a VGPR picks word i up and 64 words go to LDS
// with one ds_write.  Loop 2 reads loop 1's words back 64 at a time (one ds_read, then v_readlane per word).
__device__ __forceinline__ void gp_seed(Mt& m, uint32_t seed, int lane) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)seed);
    uint32_t prev = GP_INIT.w[0], first = 0;
    for (int c = 0; c < 623; c += 64) {                         // lane j of chunk c: word i = c + j + 1
        int mine = 0;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) {
            const int i = c + j + 1;
            if (i < 624) prev = (GP_INIT.w[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + s;
            mine = (lane == j) ? (int)prev : mine;
        }
        if (c == 0) first = (uint32_t)__builtin_amdgcn_readlane(mine, 0);
        if (c + lane + 1 < 624) m.key[c + lane + 1] = (uint32_t)mine;
    }
    // (wrap: mt[0] = mt[623] = prev)  i = 1 again
    const uint32_t one = (first ^ ((prev ^ (prev >> 30)) * 1664525u)) + s;
    prev = one;
    __syncthreads();
    for (int c = 0; c < 623; c += 64) {
        const int old = (c + lane + 1 < 624) ? (int)m.key[c + lane + 1] : 0;
        int mine = 0;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) {
            const int i = c + j + 1;
            if (i >= 2 && i < 624)
                prev = ((uint32_t)__builtin_amdgcn_readlane(old, j) ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
            mine = (lane == j) ? (int)prev : mine;
        }
        if (c + lane + 1 >= 2 && c + lane + 1 < 624) m.key[c + lane + 1] = (uint32_t)mine;
    }
    if (lane == 0) {
        m.key[1] = (one ^ ((prev ^ (prev >> 30)) * 1566083941u)) - 1u;       // (wrap: mt[0] = mt[623])  i = 1
        m.key[0] = 0x80000000u;
    }
    m.pos = 624;
    __syncthreads();
}

struct GraphPoolArgs {
    int n, n_candidates, capacity;
    uint32_t first_seed;
    double radius_sq;
    double* pos;                // [capacity, N, 2]
    uint64_t* one_hop;          // [capacity, N, W]
    long long* seeds;           // [capacity]
    int* count;
    int* slot;                  // [n_candidates] workspace: accepted flag, then output slot or -1
    double* stage_pos;          // [n_candidates, N, 2] workspace
    uint64_t* stage_hop;        // [n_candidates, N, W] workspace
};

template <int W>
__global__ __launch_bounds__(64) void graph_pool_candidate_kernel(GraphPoolArgs a) {
    __shared__ uint32_t key[624];
    __shared__ double sx[64 * W], sy[64 * W];
    const int lane = threadIdx.x;
    const int n = a.n;
    const double r2 = a.radius_sq;
    for (int c = blockIdx.x; c < a.n_candidates; c += gridDim.x) {
        Mt m{key, 624};
        gp_seed(m, a.first_seed + (uint32_t)c, lane);
        mt_regen(m, lane);                                      // 624 words; node i takes words 4 i .. 4 i + 3 (N <= 128)
        double px[W], py[W];
        MEL_W_FOR(h) {
            const int i = lane + 64 * h;
            px[h] = py[h] = 0.0;
            if (i < n) {
                px[h] = mt_double(mt_temper(key[4 * i]), mt_temper(key[4 * i + 1]));
                py[h] = mt_double(mt_temper(key[4 * i + 2]), mt_temper(key[4 * i + 3]));
            }
            sx[i] = px[h], sy[i] = py[h];
        }
        __syncthreads();
        // Graph.from_positions: edge iff dx * dx + dy * dy <= radius ** 2 in float64 (no contraction), diagonal cleared
        NodeSet<W> row[W];
        MEL_W_FOR(h) row[h] = ns_zero<W>();
        for (int j = 0; j < n; ++j) {
            const double xj = sx[j], yj = sy[j];                // LDS broadcast
            MEL_W_FOR(h) {
                const double dx = px[h] - xj, dy = py[h] - yj;
                const double xx = dx * dx, yy = dy * dy;
                if (xx + yy <= r2 && lane + 64 * h != j && lane + 64 * h < n) row[h] |= ns_bit<W>(j);
            }
        }
        // Graph.is_connected: frontier expansion from node 0
        NodeSet<W> seen = ns_bit<W>(0), frontier = ns_bit<W>(0);
        while (ns_any(frontier)) {
            NodeSet<W> mine = ns_zero<W>();
            MEL_W_FOR(h) if (ns_mine(frontier, lane, h)) mine |= row[h];
            const NodeSet<W> nxt = ns_wave_or(mine);
            frontier = nxt & ~seen;
            seen |= nxt;
        }
        const bool ok = seen == ns_full<W>(n);
        if (ok) {
            MEL_W_FOR(h) {
                if (lane + 64 * h < n) {
                    const size_t k = (size_t)c * n + lane + 64 * h;
                    a.stage_pos[2 * k] = px[h], a.stage_pos[2 * k + 1] = py[h];
                    ns_store<W>(a.stage_hop, k, row[h]);
                }
            }
        }
        if (lane == 0) a.slot[c] = ok ? 1 : 0;
        __syncthreads();                                        // key / sx / sy are reused by the next candidate
    }
}

// flags -> slots in candidate (= seed) order.  One 1024-thread workgroup walks the flags 1024 at a time: ballot + popcount
// inside a wavefront, the 16 wavefront totals through LDS.
__global__ __launch_bounds__(1024) void graph_pool_scan_kernel(GraphPoolArgs a) {
    __shared__ int wave_total[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = *a.count;                                        // every thread reads it before thread 0 writes it (below)
    for (int c0 = 0; c0 < a.n_candidates; c0 += 1024) {
        const int c = c0 + t;
        const bool f = c < a.n_candidates && a.slot[c] != 0;
        const uint64_t ballot = __ballot(f);
        if (lane == 0) wave_total[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wave_total[w] : 0;
            total += wave_total[w];
        }
        const int at = base + before + rank_below(ballot, lane);
        if (c < a.n_candidates) a.slot[c] = (f && at < a.capacity) ? at : -1;
        base += total;
        __syncthreads();
    }
    if (t == 0) *a.count = base < a.capacity ? base : a.capacity;
}

template <int W>
__global__ __launch_bounds__(256) void graph_pool_write_kernel(GraphPoolArgs a) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.n_candidates) return;
    const int at = a.slot[c];
    if (at < 0) return;
    const int n = a.n;
    MEL_W_FOR(h) {
        if (lane + 64 * h < n) {
            const size_t src = (size_t)c * n + lane + 64 * h, dst = (size_t)at * n + lane + 64 * h;
            a.pos[2 * dst] = a.stage_pos[2 * src], a.pos[2 * dst + 1] = a.stage_pos[2 * src + 1];
            ns_store<W>(a.one_hop, dst, ns_load<W>(a.stage_hop, src));
        }
    }
    if (lane == 0) a.seeds[at] = (long long)a.first_seed + c;
}

struct GraphPoolLayout {
    int* slot;
    double* stage_pos;
    uint64_t* stage_hop;
    size_t bytes;
};
static GraphPoolLayout carve_graph_pool(int32_t n_nodes, int32_t n_candidates, void* workspace) {
    Carver c(workspace);
    GraphPoolLayout L{};
    const size_t nodes = (size_t)n_candidates * n_nodes;
    L.slot = c.take<int>((size_t)n_candidates);
    L.stage_pos = c.take<double>(2 * nodes);
    L.stage_hop = c.take<uint64_t>(nodes * MEL_SET_WORDS(n_nodes));
    L.bytes = c.off;
    return L;
}

static mel_status launch_graph_pool(int32_t n_nodes, double radius_sq, int64_t first_seed, int32_t n_candidates, int32_t capacity,
                                    double* pos, uint64_t* one_hop, int64_t* seeds, int32_t* count, void* workspace,
                                    size_t ws_bytes, hipStream_t stream) {
    if (n_nodes < 2 || n_nodes > MEL_MAX_NODES)
        return fail(MEL_ERR_INVALID_ARG, "mel_graph_pool_generate: n_nodes=%d (graphs of 2 .. %d nodes)", n_nodes, MEL_MAX_NODES);
    if (!pos || !one_hop || !seeds || !count || !workspace) return fail(MEL_ERR_INVALID_ARG, "mel_graph_pool_generate: null argument");
    if (n_candidates < 0 || n_candidates > GRAPH_POOL_MAX_CANDIDATES || capacity < 0 || !(radius_sq >= 0.0))
        return fail(MEL_ERR_INVALID_ARG, "mel_graph_pool_generate: n_candidates=%d capacity=%d radius_sq=%g", n_candidates, capacity, radius_sq);
    if (first_seed < 0 || first_seed + (int64_t)n_candidates > (1ll << 32))
        return fail(MEL_ERR_INVALID_ARG, "mel_graph_pool_generate: seeds %lld .. %lld leave [0, 2^32) (random.Random's one-word key)",
                    (long long)first_seed, (long long)first_seed + n_candidates - 1);
    if (n_candidates == 0) return MEL_OK;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(MEL_ERR_INVALID_ARG, "mel_graph_pool_generate: workspace must be 256-byte aligned");
    const GraphPoolLayout L = carve_graph_pool(n_nodes, n_candidates, workspace);
    if (ws_bytes < L.bytes) return fail(MEL_ERR_WORKSPACE, "mel_graph_pool_generate: workspace of %zu bytes, %zu needed", ws_bytes, L.bytes);
    clear_stale_error();
    GraphPoolArgs a{};
    a.n = n_nodes, a.n_candidates = n_candidates, a.capacity = capacity, a.first_seed = (uint32_t)first_seed, a.radius_sq = radius_sq;
    a.pos = pos, a.one_hop = one_hop, a.seeds = reinterpret_cast<long long*>(seeds), a.count = count;
    a.slot = L.slot, a.stage_pos = L.stage_pos, a.stage_hop = L.stage_hop;
#ifdef MEL_POOL_GRID
    const int grid = n_candidates < MEL_POOL_GRID ? n_candidates : MEL_POOL_GRID;      // tuning: fewer, longer-lived wavefronts
#else
    const int grid = n_candidates;
#endif
    const dim3 wgrid((unsigned)(((int64_t)n_candidates + 3) / 4));
    with_words(n_nodes, [&](auto w) {
        MEL_LAUNCH(graph_pool_candidate_kernel<decltype(w)::value>, dim3(grid), dim3(64), 0, stream, a);
        MEL_LAUNCH(graph_pool_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
        MEL_LAUNCH(graph_pool_write_kernel<decltype(w)::value>, wgrid, dim3(256), 0, stream, a);
    });
    return check_launch("graph_pool_generate");
}

}  // namespace mel
