// Whom the deciding agents attend to, per round, recorded on the device (included by attention_record.hip on record_common.hpp; the contract
// is at mel_attention_record in melissa_hip.h).  mel_forward_attention turns what the round's forward left in its workspace into
// alpha / sources; ONE launch between that and mel_env_round - where mel_decision_record_round sits - reads them with the env's
// sets as the decisions found them: a wavefront per env books every decision of the policy into the env's own rows, by round
// index, by the deciding node's degree and by head.  No atomics, no host read, no allocation: it replays from the round loop's
// HIP graphs.  It writes nothing the round loop reads.
//
//   attention_record_kernel<W>     decision_record_kernel's frame (prologue, degree rows in LDS, the round's row in registers,
//                                  trace sink).  A decision's coefficients come in with one coalesced fetch, issued a decision
//                                  ahead.  Per decision lane h < heads walks the row's sources in ascending node id and
//                                  sums head h's eight fields in doubles; the eight values change hands through the wave's LDS
//                                  and lane l sums field l % 8 over the heads in ascending order: the head mean.
//   attention_record_read_kernel   a thread per (row, field) adds the envs in ascending order: equal inputs, equal bits.
// Every field is additions, multiplications, divisions and comparisons of doubles in a fixed order (the library is built with
// -ffp-contract=off): tests/attention_record_ref.py repeats them in NumPy bit for bit.
#pragma once

namespace mel {

template <int W>
__global__ __launch_bounds__(256) void attention_record_kernel(mel_attention_record g, mel_env_batch e, const float* __restrict__ alpha,
                                                               const uint64_t* __restrict__ sources,
                                                               const int32_t* __restrict__ row_offsets,
                                                               const uint64_t* __restrict__ live) {
    const int b = wave_env();
    if (b >= g.n_envs) return;
    const int lane = lane_id();
    const int n = e.n_nodes, H = g.n_heads;
    const int32_t* sc = e.scalars + (size_t)b * MEL_ENV_SCALARS;
    if (uniform_i32(sc[MEL_S_ERROR]) != 0) {
        if (lane == 0) g.skipped[b] += 1;
        return;
    }
    const int ep = uniform_i32(sc[MEL_S_EPISODES_DONE]), mv = uniform_i32(sc[MEL_S_NUM_MOVES]);
    if (g.quota && ep >= uniform_i32(g.quota[b])) return;            // a surplus episode of a spread evaluation
    const NodeSet<W> full = ns_full<W>(n);
    const NodeSet<W> live_in = ns_uniform(ns_load<W>(live, b)) & full;
    const uint64_t* sets = e.node_sets + (size_t)b * 8 * W;
    const NodeSet<W> scripted = ns_uniform(ns_load<W>(sets, MEL_SET_SCRIPTED));
    const NodeSet<W> has = ns_uniform(ns_load<W>(sets, MEL_SET_HAS_MESSAGE));
    const NodeSet<W> waiting = ns_uniform(ns_load<W>(sets, MEL_SET_INTERESTED)) & ~has;
    const NodeSet<W> deciding = live_in & ~scripted;
    if (!ns_any(deciding)) return;
    const int row0 = uniform_i32(row_offsets[b]);
    // every deciding node's degree, and whether its row has a source at all, in one go (lane = node)
    int deg[W];
    NodeSet<W> src_of[W], without;                                     // src_of[h]: the source set of node lane + 64 h's row
    MEL_W_FOR(h) {
        const int node = lane + 64 * h;
        const bool mine = ns_mine(deciding, lane, h);
        deg[h] = 0, src_of[h] = ns_zero<W>();
        if (mine) {
            const int d = (int)e.obs_matrix[((size_t)b * n + node) * 8 + 2];
            deg[h] = d < 0 ? 0 : (d < g.n_degrees ? d : g.n_degrees - 1);
            src_of[h] = ns_load<W>(sources, (size_t)(row0 + ns_rank_below(live_in, node))) & full;
        }
        without.w[h] = __ballot(mine && !ns_any(src_of[h]));
    }
    const bool keep_round = mv >= 0 && mv < g.max_rounds;
    double* round_row = g.by_round + ((size_t)b * g.max_rounds + (keep_round ? mv : 0)) * MEL_AR_FIELDS;
    double* degree_rows = g.by_degree + (size_t)b * g.n_degrees * MEL_AR_FIELDS;
    double* head_rows = g.by_head + (size_t)b * H * MEL_AR_FIELDS;
    double sum = (keep_round && lane < MEL_AR_FIELDS) ? round_row[lane] : 0.0;      // the round's row: read once, written once
    double head_sum8[MEL_AR_FIELDS];                                              // lane h < H: head h's row, likewise
#pragma unroll
    for (int q = 0; q < MEL_AR_FIELDS; ++q) head_sum8[q] = lane < H ? head_rows[lane * MEL_AR_FIELDS + q] : 0.0;
    // the degree rows this launch touches wait in LDS for the walk, element el = row * 8 + field with lane el % 64 from its load
    // to its store (decision_record_kernel's scheme)
    __shared__ double degree_lds[4][MEL_DR_MAX_DEGREES * MEL_AR_FIELDS];
    __shared__ double head_lds[4][MEL_AR_MAX_HEADS * MEL_AR_FIELDS];
    // A decision's coefficients - c * H consecutive floats of its alpha row - are fetched by the whole wavefront, STAGE loads
    // per lane, and wait in LDS for the walk; the NEXT decision's loads are issued before this one is booked, so the walk of
    // ~N / 6 decisions waits for one memory latency, not for one per decision and source.
    constexpr int STAGE = (MEL_ATT_MAX_SOURCES * MEL_AR_MAX_HEADS + 63) / 64;
    __shared__ float alpha_lds[4][STAGE * 64];
    float* al = alpha_lds[threadIdx.x >> 6];
    float stage[STAGE];
    auto fetch = [&](int i) {                                        // (i: wave-uniform, a deciding node)
        const float* arow = alpha + (size_t)(row0 + ns_rank_below(live_in, i)) * MEL_ATT_MAX_SOURCES * H;
        const int cH = min(ns_count(node_set<W>(src_of, i)), MEL_ATT_MAX_SOURCES) * H;
#pragma unroll
        for (int q = 0; q < STAGE; ++q) stage[q] = lane + 64 * q < cH ? arow[lane + 64 * q] : 0.f;
    };
    double* tab = degree_lds[threadIdx.x >> 6];
    double* hf = head_lds[threadIdx.x >> 6];
    NodeSet<2> my_rows = ns_zero<2>();
    MEL_W_FOR(h) if (ns_mine(deciding, lane, h)) my_rows |= ns_bit<2>(deg[h]);
    const NodeSet<2> touched = ns_uniform(ns_wave_or(my_rows));
    const int elems = g.n_degrees * MEL_AR_FIELDS;
    for (int el = lane; el < elems; el += 64)
        if (ns_test(touched, el >> 3)) tab[el] = degree_rows[el];
    const int count = ns_count(deciding);
    const int t = trace_slot(g, b);                                  // trace sink: is this env listed?
    TraceRecord tr{};
    if (t >= 0) tr = trace_open(g, t, lane, b, ep, sc[MEL_S_EPISODE], mv, count, ns_count(without));
    const int f = lane & 7;                                          // the field this lane holds of a decision's head mean
    NodeSet<W> rest = deciding;
    fetch(ns_lowest(rest));
    while (ns_any(rest)) {
        const int i = ns_lowest(rest);
        ns_clear_lowest(rest);
        const NodeSet<W> S = node_set<W>(src_of, i);
        const int c = min(ns_count(S), MEL_ATT_MAX_SOURCES);
        const int d = node_i32<W>(deg, i);
#pragma unroll
        for (int q = 0; q < STAGE; ++q) al[lane + 64 * q] = stage[q];
        if (ns_any(rest)) fetch(ns_lowest(rest));
        wave_lds_handover();
        double v0 = 1.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0, v5 = 0.0, v6 = 0.0, v7 = 0.0;     // head `lane`'s fields
        if (c > 0) {
            int informed = 0, wait = 0;
            NodeSet<W> s = S;
            for (int k = 0; k < c; ++k) {
                const int j = ns_lowest(s);
                ns_clear_lowest(s);
                const double a = lane < H ? (double)al[k * H + lane] : 0.0;
                if (j == i) v1 = a;
                else if (ns_test(has, j)) v2 += a, ++informed;
                else if (ns_test(waiting, j)) v4 += a, ++wait;
                v6 += a * a;
                v7 = a > v7 ? a : v7;
            }
            v3 = (double)informed / (double)c, v5 = (double)wait / (double)c;
        }
        if (lane < H) {
            const double vals[MEL_AR_FIELDS] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
            for (int q = 0; q < MEL_AR_FIELDS; ++q) hf[lane * MEL_AR_FIELDS + q] = vals[q], head_sum8[q] += vals[q];
        }
        wave_lds_handover();
        double s8 = 0.0;
        for (int h = 0; h < H; ++h) s8 += hf[h * MEL_AR_FIELDS + f];
        const double v = s8 / (double)H;                             // the head mean of field f
        wave_lds_handover();                                         // (the next decision overwrites hf)
        sum += v;                                                    // (lanes 0 .. 7 hold the round's row)
        if ((lane >> 3) == (d & 7)) tab[d * MEL_AR_FIELDS + f] += v;
        if (t >= 0 && lane < MEL_AR_FIELDS) g.trace_fields[(tr.rec * n + i) * MEL_AR_FIELDS + lane] = v;
    }
    for (int el = lane; el < elems; el += 64)
        if (ns_test(touched, el >> 3)) degree_rows[el] = tab[el];
    if (lane < H) {
#pragma unroll
        for (int q = 0; q < MEL_AR_FIELDS; ++q) head_rows[lane * MEL_AR_FIELDS + q] = head_sum8[q];
    }
    if (keep_round) {
        if (lane < MEL_AR_FIELDS) round_row[lane] = sum;
    } else if (lane == 0) {
        g.overflow[b] += count;
    }
    if (t >= 0) {
        MEL_W_FOR(w) if (lane == w) g.trace_sets[tr.rec * W + w] = deciding.w[w];
        for (int el = lane; el < n * MEL_AR_FIELDS; el += 64)        // (the deciding nodes' rows were written by the walk)
            if (!ns_test(deciding, el >> 3)) g.trace_fields[tr.rec * n * MEL_AR_FIELDS + el] = 0.0;
        trace_close(g, t, lane, tr);
    }
}

__global__ __launch_bounds__(256) void attention_record_read_kernel(mel_attention_record g, double* __restrict__ by_round_out,
                                                                    double* __restrict__ by_degree_out,
                                                                    double* __restrict__ by_head_out,
                                                                    long long* __restrict__ counters_out) {
    const size_t per_round = (size_t)g.max_rounds * MEL_AR_FIELDS, per_degree = (size_t)g.n_degrees * MEL_AR_FIELDS;
    const size_t per_head = (size_t)g.n_heads * MEL_AR_FIELDS;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;            // (row, field): the rounds' rows, the degrees', the heads'
    if (i < per_round) by_round_out[i] = fold_rows(g.by_round, g.n_envs, per_round, i);
    else if (i < per_round + per_degree) by_degree_out[i - per_round] = fold_rows(g.by_degree, g.n_envs, per_degree, i - per_round);
    else if (i < per_round + per_degree + per_head)
        by_head_out[i - per_round - per_degree] = fold_rows(g.by_head, g.n_envs, per_head, i - per_round - per_degree);
    if (i == 0) {
        counters_out[MEL_DRC_OVERFLOW] = fold_counter(g.overflow, g.n_envs);
        counters_out[MEL_DRC_SKIPPED] = fold_counter(g.skipped, g.n_envs);
        counters_out[2] = 0, counters_out[3] = 0;
    }
}

inline mel_status check_attention_record(const mel_attention_record* g, const char* who) {
    if (!g) return fail(MEL_ERR_INVALID_ARG, "%s: record is null", who);
    if (!g->by_round || !g->by_degree || !g->by_head || !g->overflow || !g->skipped)
        return fail(MEL_ERR_INVALID_ARG, "%s: the record has a null buffer (by_round, by_degree, by_head, overflow, skipped)", who);
    if (g->max_rounds < 1 || g->max_rounds > MEL_DR_MAX_ROUNDS || g->n_degrees < 1 || g->n_degrees > MEL_DR_MAX_DEGREES ||
        g->n_heads < 1 || g->n_heads > MEL_AR_MAX_HEADS || g->n_envs < 1 || g->n_nodes < 1 || g->n_nodes > MEL_MAX_NODES)
        return fail(MEL_ERR_INVALID_ARG, "%s: max_rounds=%d outside [1, %d], n_degrees=%d outside [1, %d], n_heads=%d outside [1, %d], n_envs=%d < 1 or n_nodes=%d outside [1, %d]",
                    who, g->max_rounds, MEL_DR_MAX_ROUNDS, g->n_degrees, MEL_DR_MAX_DEGREES, g->n_heads, MEL_AR_MAX_HEADS, g->n_envs,
                    g->n_nodes, MEL_MAX_NODES);
    return check_trace_sink(g, who, g->trace_sets && g->trace_fields);
}

}  // namespace mel

extern "C" {

mel_status mel_attention_record_round(const mel_attention_record* rec, const mel_env_batch* env, const float* alpha,
                                      const uint64_t* sources, const int32_t* row_offsets, const uint64_t* live, int32_t heads,
                                      void* stream) {
    if (mel_status st = mel::check_attention_record(rec, "mel_attention_record_round")) return st;
    if (!env) return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_round: env is null");
    if (!env->scalars || !env->node_sets || !env->obs_matrix)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_round: the env batch is not bound");
    if (env->n_envs != rec->n_envs || env->n_nodes != rec->n_nodes)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_round: the record is for %d envs of %d nodes, the env batch has %d of %d",
                         rec->n_envs, rec->n_nodes, env->n_envs, env->n_nodes);
    if (!alpha || !sources || !row_offsets || !live)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_round: null input (alpha, sources, row_offsets, live)");
    if (heads != rec->n_heads)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_round: heads=%d, the record is of %d heads", heads, rec->n_heads);
    mel::clear_stale_error();
    mel::with_env_waves(rec->n_envs, env->n_nodes, [&](auto w, dim3 grid, dim3 block) {
        MEL_LAUNCH(mel::attention_record_kernel<decltype(w)::value>, grid, block, 0, static_cast<hipStream_t>(stream), *rec, *env, alpha,
                   sources, row_offsets, live);
    });
    return mel::check_launch("mel_attention_record_round");
}

mel_status mel_attention_record_read(const mel_attention_record* rec, double* by_round_out, double* by_degree_out,
                                     double* by_head_out, int64_t* counters_out, void* stream) {
    if (mel_status st = mel::check_attention_record(rec, "mel_attention_record_read")) return st;
    if (!by_round_out || !by_degree_out || !by_head_out || !counters_out)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_attention_record_read: null output (by_round_out, by_degree_out, by_head_out, counters_out)");
    mel::clear_stale_error();
    const unsigned blocks = (unsigned)(((size_t)(rec->max_rounds + rec->n_degrees + rec->n_heads) * MEL_AR_FIELDS + 255) / 256);
    MEL_LAUNCH(mel::attention_record_read_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), *rec, by_round_out,
               by_degree_out, by_head_out, reinterpret_cast<long long*>(counters_out));
    return mel::check_launch("mel_attention_record_read");
}

}  // extern "C"
