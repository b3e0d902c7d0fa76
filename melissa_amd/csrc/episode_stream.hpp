// Continuous episode supply: World.reset's sampling (graph_env/env/utils/core.py:343-395) on the device, bit for bit.
//
// Included by env.hip inside namespace mel (it calls env_reset / env_store).  The launches of one refill, in stream order:
//   episode_draw_kernel    one thread per env: the env's own generator (numpy Generator(PCG64)) draws episode_seed, the
//                          graph and the scripted set for each free ring slot, in order        core.py:372,378,395
//                          (evaluation schedule, n_test > 0: the seed is read from the fixed list at the episode's list
//                          position and only the scripted set comes from the generator        core.py:351-352,395)
//   episode_keys_kernel    one LANE per new episode, for the first key_capacity of them: init_genrand of
//                          RandomState(episode_seed), that generator's first accepted randint(0, 1e9) = the movement seed
//                          (after the graph draw under the evaluation schedule), init_genrand of RandomState(movement_seed);
//                          both 624-word keys go to the stream's key scratch in HBM
//   episode_fill_kernel    one wavefront per new episode: RandomState(episode_seed) (MT19937) draws movement seed, source,
//                          interest density and the interested set (evaluation schedule: the graph first, and the density
//                          from the list position instead of a draw, core.py:357-366);
//                          the graph is copied from the packed dataset; the scripted set loses the source (:213-215)
//   episode_moves_kernel   four wavefronts per new episode (moving graphs only): RandomState(movement_seed) fills the
//                          movement offsets                                                    core.py:316-319
//   episode_snapshot_kernel one wavefront per new episode: GraphEnv.reset + World.reset run into the snapshot batch
//                          core.py:398-437 - the only launch that holds an Env<W> in registers
//   episode_publish_kernel produced[b] += new_count[b]
// A work item past key_capacity (or one whose movement seed the keys launch did not reach within MEL_KEY_DRAWS outputs) seeds
// its generators inside its own wavefront, on the scalar unit (mt_seed below).
//
// numpy algorithms restated here (numpy/random/src: pcg64.h, mt19937.c, distributions.c, legacy):
//   PCG64       state' = state * 0x2360ED051FC65DA44385DF649FCCF645 + inc (mod 2^128); out = rotr64(hi ^ lo, hi >> 58)
//               next_uint32 returns the low half of a fresh 64-bit output and keeps the high half for the next call
//   Generator.integers(0, hi) / choice(n)  (range < 2^32): Lemire's multiply-shift on next_uint32 with rejection
//   RandomState(seed)     init_genrand: key[0] = seed; key[i] = 1812433253 * (key[i-1] ^ (key[i-1] >> 30)) + i
//   RandomState.randint   masked rejection: draw & mask until <= range
//   RandomState.uniform   low + (high - low) * ((a >> 5) * 2^26 + (b >> 6)) / 2^53, a, b consecutive 32-bit outputs
//   RandomState.choice(n, k, replace=False) = permutation(n)[:k]: Fisher-Yates from the top, j = random_interval(i)
//   Generator.choice(n, k, replace=False)  (p None, n <= 10000): Floyd's algorithm - for j = n-k .. n-1 draw v in [0, j]
//               and take v, or j when v is already taken - then a Fisher-Yates shuffle of the k results, i = k-1 .. 1, each
//               one bounded draw in [0, i].  Both use the Lemire draw above (a range of 0 draws nothing).
#pragma once

namespace mel {

// ---- PCG64 (one thread) ------------------------------------------------------------------------------------------
struct Pcg64 {
    uint64_t lo, hi, inc_lo, inc_hi;
    uint32_t has32, half;
};

__device__ __forceinline__ uint64_t pcg64_next64(Pcg64& g) {
    constexpr uint64_t MH = 2549297995355413924ull, ML = 4865540595714422341ull;
    // (hi:lo) * (MH:ML) mod 2^128, then + inc
    uint64_t lo = g.lo * ML;
    uint64_t hi = __umul64hi(g.lo, ML) + g.hi * ML + g.lo * MH;
    const uint64_t lo2 = lo + g.inc_lo;
    hi = hi + g.inc_hi + (lo2 < lo ? 1ull : 0ull);
    g.lo = lo2, g.hi = hi;
    const uint64_t x = hi ^ lo2;
    const unsigned r = (unsigned)(hi >> 58);
    return (x >> r) | (x << ((64u - r) & 63u));
}
__device__ __forceinline__ uint32_t pcg64_next32(Pcg64& g) {
    if (g.has32) {
        g.has32 = 0;
        return g.half;
    }
    const uint64_t v = pcg64_next64(g);
    g.has32 = 1;
    g.half = (uint32_t)(v >> 32);
    return (uint32_t)v;
}
// uniform integer in [0, rng] (rng < 2^32 - 1): buffered_bounded_lemire_uint32
__device__ __forceinline__ uint32_t pcg64_bounded(Pcg64& g, uint32_t rng) {
    if (rng == 0) return 0;
    const uint32_t excl = rng + 1u;
    uint64_t m = (uint64_t)pcg64_next32(g) * excl;
    uint32_t left = (uint32_t)m;
    if (left < excl) {
        const uint32_t thr = (0xFFFFFFFFu - rng) % excl;
        while (left < thr) {
            m = (uint64_t)pcg64_next32(g) * excl;
            left = (uint32_t)m;
        }
    }
    return (uint32_t)(m >> 32);
}

// World._sample_scripted_agents' draw (core.py:197-212): np_random.choice(n, size=k, replace=False) as a SET.  Floyd's hash
// table is a membership test on the set itself, and the shuffle only reorders the k results: its draws are consumed, its
// data movement cannot matter to a set.  Two words always (n <= MEL_MAX_NODES = 128); k == 0 draws nothing.
__device__ __forceinline__ NodeSet<2> pcg64_choice_set(Pcg64& g, int n, int k) {
    NodeSet<2> set = ns_zero<2>();
    for (int j = n - k; j < n; ++j) {
        const int v = (int)pcg64_bounded(g, (uint32_t)j);
        set |= ns_bit<2>(ns_test(set, v) ? j : v);
    }
    for (int i = k - 1; i >= 1; --i) (void)pcg64_bounded(g, (uint32_t)i);
    return set;
}

struct StreamArgs {
    mel_episode_stream st;
    mel_graph_pool graphs;
    mel_episode_pool pool;      // ring arrays (written here)
    mel_env_batch env;          // live envs: ep_cursor
    mel_env_batch snap;         // reset snapshots, one "env" per ring slot
    int max_new, discard;
};

__global__ __launch_bounds__(256) void episode_draw_kernel(StreamArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.st.n_envs) return;
    const int K = a.st.ring;
    Pcg64 g;
    g.lo = a.st.pcg[4 * (size_t)b], g.hi = a.st.pcg[4 * (size_t)b + 1];
    g.inc_lo = a.st.pcg[4 * (size_t)b + 2], g.inc_hi = a.st.pcg[4 * (size_t)b + 3];
    g.has32 = a.st.pcg_half[2 * (size_t)b], g.half = a.st.pcg_half[2 * (size_t)b + 1];
    const uint32_t graph_rng = (uint32_t)(a.graphs.n_graphs - 1);
    const int n = a.pool.n_nodes, k_scripted = a.st.n_scripted, words = MEL_SET_WORDS(n);
    const int T = a.st.n_test;                                  // > 0: the evaluation schedule (core.py:348-370)
    for (int d = 0; d < a.discard; ++d) {                       // episodes the reference samples and throws away
        if (T == 0) {
            (void)pcg64_bounded(g, 999999999u);
            if (!a.st.fixed_graph) (void)pcg64_bounded(g, graph_rng);
        }
        if (k_scripted > 0) (void)pcg64_choice_set(g, n, k_scripted);
    }
    long long walked = 0;                                       // list entries this env has passed before episode 0
    if (T > 0) {
        walked = (long long)a.st.test_discarded[b] + a.discard;
        a.st.test_discarded[b] = (int)walked;
    }
    const int cur = a.env.scalars[(size_t)b * MEL_ENV_SCALARS + MEL_S_EP_CURSOR];
    const int first = a.st.produced[b];
    int cnt = 0;
    while (cnt < a.max_new && first + cnt <= cur + K - 2) {
        const int slot = b * K + (first + cnt) % K;
        if (T > 0) {                                                                          // core.py:351-352
            const int t = (int)(((long long)b * a.st.test_env_step + (walked + first + cnt) * a.st.test_episode_step) % T);
            a.st.draw_seed[slot] = a.st.test_seeds[t];
            a.st.draw_graph[slot] = t;                          // the fill draws the graph itself: it needs the position
        } else {
            a.st.draw_seed[slot] = pcg64_bounded(g, 999999999u);                                  // core.py:372
            a.st.draw_graph[slot] = a.st.fixed_graph ? 0 : (int)pcg64_bounded(g, graph_rng);      // core.py:377-379
        }
        if (k_scripted > 0) {                                                                 // core.py:395 (uniform branch)
            const NodeSet<2> set = pcg64_choice_set(g, n, k_scripted);
            for (int w = 0; w < words; ++w) a.st.draw_scripted[(size_t)slot * words + w] = set.w[w];
        }
        const int w = atomicAdd(a.st.work, 1);
        a.st.work[1 + w] = slot;
        ++cnt;
    }
    a.st.pcg[4 * (size_t)b] = g.lo, a.st.pcg[4 * (size_t)b + 1] = g.hi;
    a.st.pcg_half[2 * (size_t)b] = g.has32, a.st.pcg_half[2 * (size_t)b + 1] = g.half;
    a.st.new_count[b] = cnt;
}

__global__ __launch_bounds__(256) void episode_publish_kernel(StreamArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.st.n_envs) return;
    a.st.produced[b] += a.st.new_count[b];
    if (b == 0) a.st.work[0] = 0;
}

// ---- MT19937 held by one wavefront: the 624-word key in LDS, the position wave-uniform ------------------------------
struct Mt {
    uint32_t* key;      // LDS [624]
    int pos;            // wave-uniform
};

// init_genrand (mt19937_seed): a serial recurrence.  It is wave-uniform, so it is written for the SCALAR unit: the chain
// s -> 1812433253 * (s ^ (s >> 30)) + i runs in SGPRs (four dependent SALU operations per word instead of a VALU chain with
// a quarter-rate multiply), lane (i % 64) of a VGPR picks word i up with a compare + select, and 64 words go to LDS with one
// ds_write.
__device__ __forceinline__ void mt_seed(Mt& m, uint32_t seed, int lane) {
    uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)seed);
    for (int c = 0; c < 624; c += 64) {
        int mine = 0;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) {
            mine = (lane == j) ? (int)s : mine;                 // lane j keeps word c + j (s is an SGPR)
            s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)(c + j + 1);
        }
        if (c + lane < 624) m.key[c + lane] = (uint32_t)mine;
    }
    m.pos = 624;
    __syncthreads();
}

__device__ __forceinline__ uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7FFFFFFFu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
}
// mt19937_gen: key[k] = key[(k + 397) % 624] ^ twist(key[k], key[k + 1]) in place.  k < 227 reads only old words;
// 227 <= k < 454 reads new words [0, 227); 454 <= k < 623 reads new words [227, 396); k = 623 reads the NEW key[0].
__device__ __forceinline__ void mt_regen(Mt& m, int lane) {
    uint32_t v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = c * 64 + lane;
        if (k < 227) v[c] = mt_twist(m.key[k], m.key[k + 1], m.key[k + 397]);
    }
    __syncthreads();                       // every old word of phase 1 has been read (key[227] by k = 226 included)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = c * 64 + lane;
        if (k < 227) m.key[k] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = 227 + c * 64 + lane;
        if (k < 454) v[c] = mt_twist(m.key[k], m.key[k + 1], m.key[k - 227]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = 227 + c * 64 + lane;
        if (k < 454) m.key[k] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int k = 454 + c * 64 + lane;
        if (k < 623) v[c] = mt_twist(m.key[k], m.key[k + 1], m.key[k - 227]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int k = 454 + c * 64 + lane;
        if (k < 623) m.key[k] = v[c];
    }
    __syncthreads();
    if (lane == 0) m.key[623] = mt_twist(m.key[623], m.key[0], m.key[396]);
    __syncthreads();
    m.pos = 0;
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
}
// next 32-bit output, the same value in every lane (control flow stays wave-uniform: pos is uniform)
__device__ __forceinline__ uint32_t mt_next32(Mt& m, int lane) {
    if (m.pos == 624) mt_regen(m, lane);
    const uint32_t y = m.key[m.pos];                 // LDS broadcast
    m.pos += 1;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)mt_temper(y));
}
__device__ __forceinline__ double mt_double(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}
// random_interval / buffered_bounded_masked_uint32: uniform in [0, rng] by masked rejection
__device__ __forceinline__ uint32_t mt_masked(Mt& m, uint32_t rng, int lane) {
    if (rng == 0) return 0;
    uint32_t mask = rng;
    mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
    uint32_t v;
    do {
        v = mt_next32(m, lane) & mask;
    } while (v > rng);
    return v;
}

// The first MEL_HEAD_DRAWS outputs of a freshly seeded generator (m.pos == 624: no regeneration yet), tempered, lane l of t0
// holding output l and of t1 output 64 + l.  The first regeneration makes word k < 227 from the seeded words k, k + 1 and
// k + 397 alone, so the head is computed without writing the key and without a barrier, and a draw from it is a v_readlane
// with a scalar compare behind it instead of an LDS round trip per output.  A generator that is asked for more (every episode
// of 100 nodes is, hardly one of 50) regenerates for real and goes on from LDS.
constexpr int MEL_HEAD_DRAWS = 128;
struct MtHead {
    uint32_t t0, t1;
    int drawn;          // wave-uniform
};
__device__ __forceinline__ MtHead mt_head(const Mt& m, int lane) {
    MtHead h;
    h.t0 = mt_temper(mt_twist(m.key[lane], m.key[lane + 1], m.key[lane + 397]));
    h.t1 = mt_temper(mt_twist(m.key[64 + lane], m.key[65 + lane], m.key[461 + lane]));
    h.drawn = 0;
    return h;
}
__device__ __forceinline__ uint32_t mt_next32(Mt& m, MtHead& h, int lane) {
    if (h.drawn < MEL_HEAD_DRAWS) {
        const int p = h.drawn;
        h.drawn = p + 1;
        return (uint32_t)__builtin_amdgcn_readlane((int)(p < 64 ? h.t0 : h.t1), p & 63);
    }
    if (m.pos == 624 && h.drawn == MEL_HEAD_DRAWS) {        // the head is used up: outputs 128 .. 623 of this key come from LDS
        mt_regen(m, lane);
        m.pos = MEL_HEAD_DRAWS;
        h.drawn = MEL_HEAD_DRAWS + 1;
    }
    return mt_next32(m, lane);
}
__device__ __forceinline__ uint32_t mt_masked(Mt& m, MtHead& h, uint32_t rng, int lane) {
    if (rng == 0) return 0;
    uint32_t mask = rng;
    mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
    uint32_t v;
    do {
        v = mt_next32(m, h, lane) & mask;
    } while (v > rng);
    return v;
}
static_assert(MEL_HEAD_DRAWS == 128, "mt_next32 selects between two head registers");

// ---- init_genrand for 64 generators at once, one lane each ---------------------------------------------------------
// The recurrence cannot be split across words, but 64 of them run side by side: four vector instructions per word for 64
// keys, against nine scalar + vector ones per word for the single key of mt_seed.  `out` is the workgroup's block of the key
// scratch, [cnt <= 64][624] words, key-major, so that the wave which later owns a key reads it with coalesced loads: every 32
// words of the 64 keys pass through an LDS tile (row stride 33 words: both the lane-per-key writes and the lane-per-word reads
// are conflict free; 8 448 bytes, which fit beside a resident conv2 GEMM workgroup) and leave as 128-byte rows, two keys per
// store instruction.
__device__ __forceinline__ void mt_seed_lanes(uint32_t s, uint32_t* out, int cnt, uint32_t* tile, int lane) {
    const int half = lane >> 5, col = lane & 31;
    for (int c = 0; c < 624; c += 32) {
        const int len = 624 - c < 32 ? 624 - c : 32;         // 19 chunks of 32 words and one of 16
#pragma unroll 16
        for (int j = 0; j < len; ++j) {
            tile[lane * 33 + j] = s;
            s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)(c + j + 1);
        }
        __syncthreads();
        // (one row pair per trip.  Eight LDS reads in flight ahead of eight predicated stores measured WORSE on the headline:
        // the keys launch 103 us against 65, and conv2's GEMM beside it 58 us against 46 - NOTES.md)
        if (col < len)
            for (int r = half; r < cnt; r += 2) out[(size_t)r * 624 + c + col] = tile[r * 33 + col];
        __syncthreads();
    }
}

// What the keys launch leaves in work[] for item w (behind the B*K slot entries): the movement seed (< 2^30), or this mark -
// the item's wavefronts then seed in-wave and episode_fill_kernel stores the seed it draws, with the mark kept.
constexpr uint32_t MEL_SEED_IN_WAVE = 0x80000000u;
// Outputs of the episode generator the keys launch looks at per episode (the graph draw's rejections included).  The first
// regeneration gives output k from key words k, k + 1 and k + 397 alone, so this must stay below 227.
#ifndef MEL_KEY_DRAWS
#define MEL_KEY_DRAWS 8
#endif
static_assert(MEL_KEY_DRAWS >= 1 && MEL_KEY_DRAWS <= 226, "output k of the first regeneration reads key[k + 397]");

// 64 new episodes per workgroup, one lane each.
__global__ __launch_bounds__(64) void episode_keys_kernel(StreamArgs a) {
    __shared__ uint32_t tile[64 * 33];
    const int lane = threadIdx.x;
    const int n_work = a.st.work[0];
    const int n_keys = n_work < a.st.key_capacity ? n_work : a.st.key_capacity;
    const int w0 = blockIdx.x * 64;
    if (w0 >= n_keys) return;                                // (workgroup-uniform)
    const int cnt = n_keys - w0 < 64 ? n_keys - w0 : 64;
    const bool on = lane < cnt;
    const int w = w0 + lane;
    uint32_t* ep = a.st.key_scratch + (size_t)w0 * 624;
    mt_seed_lanes(on ? a.st.draw_seed[a.st.work[1 + w]] : 0u, ep, cnt, tile, lane);                 // core.py:373
    if (!a.env.dynamic_graph) return;                        // a static graph never seeds a movement generator
    // (the barrier that ends mt_seed_lanes makes the workgroup's own stores to `ep` visible to its lanes)
    uint32_t movement_seed = MEL_SEED_IN_WAVE;
    if (on) {
        const uint32_t* k = ep + (size_t)lane * 624;
        int p = 0;
        auto output = [&]() {
            const uint32_t y = mt_temper(mt_twist(k[p], k[p + 1], k[p + 397]));
            p += 1;
            return y;
        };
        bool open = true;
        const uint32_t graph_rng = (uint32_t)(a.graphs.n_graphs - 1);
        if (a.st.n_test > 0 && graph_rng != 0) {             // core.py:357 - the evaluation schedule draws the graph first
            uint32_t mask = graph_rng;
            mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
            open = false;
            while (!open && p < MEL_KEY_DRAWS) open = (output() & mask) <= graph_rng;
        }
        while (open && p < MEL_KEY_DRAWS) {                                                         // :381 / :361
            const uint32_t v = output() & 0x3FFFFFFFu;
            if (v <= 999999999u) {
                movement_seed = v;
                break;
            }
        }
        reinterpret_cast<uint32_t*>(a.st.work)[1 + a.st.n_envs * a.st.ring + w] = movement_seed;
    }
    mt_seed_lanes(movement_seed, a.st.key_scratch + ((size_t)a.st.key_capacity + w0) * 624, cnt, tile, lane);   // :382
}

// A generator whose key the keys launch seeded: 624 coalesced words from the scratch into LDS.
__device__ __forceinline__ void mt_load_key(Mt& m, const uint32_t* src, int tid, int threads) {
    for (int i = tid; i < 624; i += threads) m.key[i] = src[i];
    m.pos = 624;
    __syncthreads();
}

// One wavefront (a 64-thread workgroup) per new episode: the episode generator's draws and the pool slot.
template <int W>
__global__ __launch_bounds__(64) void episode_fill_kernel(StreamArgs a) {
    __shared__ uint32_t key[624];
    const int lane = threadIdx.x;
    const int n = a.pool.n_nodes;
    const int n_work = a.st.work[0];
    uint32_t* seeds = reinterpret_cast<uint32_t*>(a.st.work) + 1 + a.st.n_envs * a.st.ring;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int slot = a.st.work[1 + w];
        Mt m{key, 624};
        // ---- ep_rng = RandomState(episode_seed)                                                    core.py:373
        if (w < a.st.key_capacity) mt_load_key(m, a.st.key_scratch + (size_t)w * 624, lane, 64);
        else mt_seed(m, a.st.draw_seed[slot], lane);
        MtHead hd = mt_head(m, lane);
        const int T = a.st.n_test;                           // wave-uniform: > 0 = the evaluation schedule
        int g = a.st.draw_graph[slot];                       // training: the graph; evaluation: the list position
        const int t = g;
        if (T > 0) g = (int)mt_masked(m, hd, (uint32_t)(a.graphs.n_graphs - 1), lane);                  // :357 (one graph: no draw)
        const uint32_t movement_seed = mt_masked(m, hd, 999999999u, lane);                              // :381 / :361
        // (a seed the keys launch did not supply goes to the moves launch from here, marked)
        if (lane == 0 && a.env.dynamic_graph && (w >= a.st.key_capacity || seeds[w] == MEL_SEED_IN_WAVE))
            seeds[w] = movement_seed | MEL_SEED_IN_WAVE;
        const int origin = (int)mt_masked(m, hd, (uint32_t)(n - 1), lane);                              // :384 / :364
        double density = a.st.fixed_interest_density;
        if (T > 0) {                                         // :365-366 - the list index is read after it was bumped
            density = (double)(((t + 1) % T) % 10 + 1) / 10.0;
        } else if (!a.st.has_density) {                                                             // :385
            const uint32_t d0 = mt_next32(m, hd, lane);
            const uint32_t d1 = mt_next32(m, hd, lane);
            const double range = 1.0 - 0.1;
            density = 0.1 + range * mt_double(d0, d1);
        }
        const int k_int = (int)(density * (double)n);                                               // :392
        // permutation(n)[:k] (:393): the lane of node i holds arr[i]; swap(i, j) for i = n-1 .. 1, j = random_interval(i)
        int arr[W];
        MEL_W_FOR(h) arr[h] = lane + 64 * h;
        for (int i = n - 1; i >= 1; --i) {
            const int j = (int)mt_masked(m, hd, (uint32_t)i, lane);
            const int vi = node_i32<W>(arr, i), vj = node_i32<W>(arr, j);
            MEL_W_FOR(h) {
                if (lane + 64 * h == i) arr[h] = vj;
                if (lane + 64 * h == j) arr[h] = vi;
            }
        }
        NodeSet<W> mine = ns_zero<W>();
        MEL_W_FOR(h) if (lane + 64 * h < k_int) mine |= ns_bit<W>(arr[h]);
        const NodeSet<W> interested = ns_wave_or(mine);
        // ---- the pool slot
        MEL_W_FOR(h) {
            if (lane + 64 * h < n) {
                const size_t src = (size_t)g * n + lane + 64 * h, dst = (size_t)slot * n + lane + 64 * h;
                const_cast<double*>(a.pool.pos)[2 * dst] = a.graphs.pos[2 * src];
                const_cast<double*>(a.pool.pos)[2 * dst + 1] = a.graphs.pos[2 * src + 1];
                ns_store<W>(const_cast<uint64_t*>(a.pool.one_hop), dst, ns_load<W>(a.graphs.one_hop, src));
            }
        }
        if (lane == 0) {
            const_cast<int32_t*>(a.pool.origin)[slot] = origin;
            ns_store<W>(const_cast<uint64_t*>(a.pool.interested), slot, interested);
            if (a.st.n_scripted > 0)                           // the source is never scripted while ratio < 1  core.py:213-215
                ns_store<W>(const_cast<uint64_t*>(a.pool.scripted), slot, ns_load<W>(a.st.draw_scripted, slot) & ~ns_bit<W>(origin));
            else if (a.pool.scripted) ns_store<W>(const_cast<uint64_t*>(a.pool.scripted), slot, ns_zero<W>());      // scripted_agents_ratio == 0
        }
        __syncthreads();                                                  // key[] is reused by the next work item
    }
}

// mt_regen for a workgroup of 256, out of place: the three phases are 227, 227 and 170 words wide, one pass each, and with the
// new key in a buffer of its own a phase only has to wait for the new words it reads - three barriers instead of mt_regen's
// seven.  The last word (old key[623], new key[0] and key[396]) rides in the third phase.
__device__ __forceinline__ void mt_regen_wide(const uint32_t* old, uint32_t* key, int tid) {
    if (tid < 227) key[tid] = mt_twist(old[tid], old[tid + 1], old[tid + 397]);
    __syncthreads();
    if (tid < 227) key[227 + tid] = mt_twist(old[227 + tid], old[228 + tid], key[tid]);
    __syncthreads();
    if (tid < 169) key[454 + tid] = mt_twist(old[454 + tid], old[455 + tid], key[227 + tid]);
    if (tid == 169) key[623] = mt_twist(old[623], key[0], key[396]);
    __syncthreads();
}

// movement_np_random = RandomState(movement_seed): step * uniform(-1, 1), x's then y's per move        core.py:316-319,382
// Four wavefronts (a 256-thread workgroup) per new episode.
__global__ __launch_bounds__(256) void episode_moves_kernel(StreamArgs a) {
    __shared__ uint32_t keys[2][624];
    const int tid = threadIdx.x;
    const int n_work = a.st.work[0];
    const uint32_t* seeds = reinterpret_cast<const uint32_t*>(a.st.work) + 1 + a.st.n_envs * a.st.ring;
    const int total = a.pool.max_moves * 2 * a.pool.n_nodes;              // doubles; 312 per regeneration of the key
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int slot = a.st.work[1 + w];
        Mt m{keys[0], 624};
        const uint32_t seed = seeds[w];
        if (seed & MEL_SEED_IN_WAVE) mt_seed(m, seed & ~MEL_SEED_IN_WAVE, tid & 63);    // (each wave writes the same 624 words)
        else mt_load_key(m, a.st.key_scratch + ((size_t)a.st.key_capacity + w) * 624, tid, 256);
        double* out = const_cast<double*>(a.pool.moves) + (size_t)slot * total;
        int cur = 0;
        for (int base = 0; base < total; base += 312) {
            mt_regen_wide(keys[cur], keys[cur ^ 1], tid);
            cur ^= 1;
            const uint32_t* key = keys[cur];
            for (int t = tid; t < 312 && base + t < total; t += 256) {
                const double u = mt_double(mt_temper(key[2 * t]), mt_temper(key[2 * t + 1]));
                const double x = -1.0 + 2.0 * u;                          // random_uniform: low + range * u
                out[base + t] = 0.06 * x;                                 // NODES_MOVEMENT_STEP * ... (constants.py:4)
            }
        }
        __syncthreads();                                                  // key[] is reused by the next work item
    }
}

// GraphEnv.reset + World.reset for every new episode into its snapshot                               core.py:398-437
// One wavefront per new episode, after its pool slot is complete.
template <int W>
__global__ __launch_bounds__(64) void episode_snapshot_kernel(StreamArgs a) {
    const int lane = threadIdx.x;
    const int n_work = a.st.work[0];
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int slot = a.st.work[1 + w];
        Env<W> s{};
        s.skip = SKIP_NONE, s.sel = NONE;
        MEL_W_FOR(h) s.act[h] = NONE, s.cur_act[h] = NONE;
        env_reset(a.snap, a.pool, slot, s, slot, 0, lane);
        s.ep_cursor = 0;
        env_store(a.snap, slot, lane, s);
    }
}

// Pacing gate for a side stream: one wavefront polls a device counter that the main stream's kernels advance (the round
// counter of mel_env_round) until it reaches `target`, so that what follows on the side stream runs when the main stream has
// got that far - WITHOUT any event on the main stream (an event record / wait between HIP-graph replays costs the replayed
// step ~8 us on this stack).  Bounded: after timeout_us the gate opens anyway (what follows must be safe at any time; the
// episode refill is - it only ever writes ring slots no env can be using, judged from the cursors it reads).
__global__ __launch_bounds__(64) void wait_counter_kernel(const uint32_t* counter, uint32_t target, uint32_t timeout_us) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();            // 100 MHz
    const uint64_t limit = (uint64_t)timeout_us * 100ull;
    for (;;) {
        const uint32_t c = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int32_t)(c - target) >= 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit) break;
        __builtin_amdgcn_s_sleep(64);
    }
}

// The evaluation schedule's seed list (core.py:184-187): RandomState(17).randint(0, 1e9), n times.  One wavefront.
__global__ __launch_bounds__(64) void episode_test_seeds_kernel(uint32_t* out, int n) {
    __shared__ uint32_t key[624];
    const int lane = threadIdx.x;
    Mt m{key, 624};
    mt_seed(m, 17u, lane);
    for (int i = 0; i < n; ++i) {
        const uint32_t v = mt_masked(m, 999999999u, lane);
        if (lane == 0) out[i] = v;
    }
}

static mel_status launch_episode_test_seeds(uint32_t* out, int32_t n, hipStream_t stream) {
    if (!out || n < 1) return fail(MEL_ERR_INVALID_ARG, "mel_episode_test_seeds: out=%p n=%d", (void*)out, n);
    clear_stale_error();
    MEL_LAUNCH(episode_test_seeds_kernel, dim3(1), dim3(64), 0, stream, out, n);
    return check_launch("episode_test_seeds");
}

static mel_status launch_episode_refill(const mel_episode_stream* st, const mel_graph_pool* graphs,
                                        const mel_episode_pool* pool, const mel_env_batch* env, int32_t max_new,
                                        int32_t discard, hipStream_t stream) {
    if (!st || !graphs || !pool || !env) return fail(MEL_ERR_INVALID_ARG, "null argument");
    const int B = st->n_envs, K = st->ring;
    if (B != env->n_envs || K < 3) return fail(MEL_ERR_INVALID_ARG, "stream of %d envs x %d slots for %d envs (ring >= 3)", B, K, env->n_envs);
    if (!st->pcg || !st->pcg_half || !st->produced || !st->draw_seed || !st->draw_graph || !st->work || !st->new_count)
        return fail(MEL_ERR_INVALID_ARG, "episode stream has null buffers");
    if (graphs->n_nodes != env->n_nodes || graphs->n_graphs < 1 || !graphs->pos || !graphs->one_hop)
        return fail(MEL_ERR_INVALID_ARG, "graph pool of %d graphs x %d nodes for %d-node envs", graphs->n_graphs, graphs->n_nodes, env->n_nodes);
    if (st->fixed_graph && (graphs->n_graphs != 1 || env->dynamic_graph))
        return fail(MEL_ERR_UNSUPPORTED, "a fixed graph streams only when it is static (a moving fixed graph carries its positions over)");
    if (env->is_testing && st->n_test == 0)
        return fail(MEL_ERR_UNSUPPORTED, "an env in testing mode streams the evaluation schedule: set n_test and test_seeds");
    if (st->n_test != 0) {
        if (st->n_test < 0 || !env->is_testing)
            return fail(MEL_ERR_INVALID_ARG, "n_test=%d: the evaluation schedule needs n_test > 0 and an env in testing mode", st->n_test);
        if (st->fixed_graph) return fail(MEL_ERR_UNSUPPORTED, "testing mode draws its graph from the pool (core.py:355-359)");
        if (!st->test_seeds || !st->test_discarded) return fail(MEL_ERR_INVALID_ARG, "n_test=%d needs test_seeds and test_discarded", st->n_test);
        if (st->test_env_step < 0 || st->test_episode_step < 0)
            return fail(MEL_ERR_INVALID_ARG, "test_env_step=%d test_episode_step=%d", st->test_env_step, st->test_episode_step);
        if (discard > 0 && st->test_env_step != 0)
            return fail(MEL_ERR_INVALID_ARG, "discard=%d with test_env_step=%d: only the reference's walk discards episodes", discard, st->test_env_step);
    }
    // (n_scripted, not env->heuristic: a ratio without a heuristic is legal - scripted nodes then simply never act)
    if (st->n_scripted < 0 || st->n_scripted > env->n_nodes)
        return fail(MEL_ERR_INVALID_ARG, "n_scripted=%d for %d-node envs", st->n_scripted, env->n_nodes);
    if (st->n_scripted > 0 && (!st->draw_scripted || !pool->scripted))
        return fail(MEL_ERR_INVALID_ARG, "n_scripted=%d needs draw_scripted and pool->scripted", st->n_scripted);
    if (pool->n_episodes != B * K || pool->n_nodes != env->n_nodes || !pool->pos || !pool->one_hop || !pool->origin ||
        !pool->interested || (env->dynamic_graph && (!pool->moves || pool->max_moves < 1)))
        return fail(MEL_ERR_INVALID_ARG, "the ring pool must hold n_envs * ring = %d episodes", B * K);
    if (pool->produced != st->produced) return fail(MEL_ERR_INVALID_ARG, "pool->produced must be the stream's counter");
    const mel_env_batch* sn = pool->snapshot;
    if (!sn || sn->n_envs < B * K || sn->n_nodes != env->n_nodes || sn->dynamic_graph != env->dynamic_graph ||
        sn->has_local_ratio != env->has_local_ratio || !sn->pos || !sn->scalars)
        return fail(MEL_ERR_INVALID_ARG, "the ring pool needs a snapshot batch of n_envs * ring envs with the env's settings");
    if (max_new < 0 || discard < 0) return fail(MEL_ERR_INVALID_ARG, "max_new=%d discard=%d", max_new, discard);
    if (st->key_capacity < 0 || (st->key_capacity > 0 && !st->key_scratch))
        return fail(MEL_ERR_INVALID_ARG, "key_capacity=%d key_scratch=%p", st->key_capacity, (void*)st->key_scratch);
    clear_stale_error();
    StreamArgs a{};
    a.st = *st, a.graphs = *graphs, a.pool = *pool, a.env = *env, a.snap = *sn;
    a.max_new = max_new > K ? K : max_new, a.discard = discard;
    StageScope t(MEL_STAGE_ENV_RESET, stream);
    MEL_LAUNCH(episode_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, a);
    // the work-item count lives on the device: fixed grids cover or loop over it (surplus workgroups leave at once)
    const long most = (long)B * a.max_new;
    const long keys = most < st->key_capacity ? most : st->key_capacity;
    if (keys > 0) MEL_LAUNCH(episode_keys_kernel, dim3((unsigned)((keys + 63) / 64)), dim3(64), 0, stream, a);
    const long expect = (long)B * (a.max_new < 4 ? a.max_new : 4);
#ifdef MEL_FILL_GRID
    const int grid = MEL_FILL_GRID;                  // tuning: fewer, longer-lived waves in the three per-episode launches
#else
    const int grid = (int)(expect < 256 ? 256 : (expect > 4096 ? 4096 : expect));
#endif
    with_words(env->n_nodes, [&](auto w) { MEL_LAUNCH(episode_fill_kernel<decltype(w)::value>, dim3(grid), dim3(64), 0, stream, a); });
    if (env->dynamic_graph) MEL_LAUNCH(episode_moves_kernel, dim3(grid), dim3(256), 0, stream, a);
    with_words(env->n_nodes, [&](auto w) { MEL_LAUNCH(episode_snapshot_kernel<decltype(w)::value>, dim3(grid), dim3(64), 0, stream, a); });
    MEL_LAUNCH(episode_publish_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, a);
    return check_launch("episode_refill");
}

}  // namespace mel
