// The policy's decisions per round, recorded on the device (included by env.hip; the contract is at mel_decision_record in
// melissa_hip.h).  The round's logits and actions live between two launches only - the forward writes them, mel_env_round consumes
// the actions and overwrites `live` - so ONE launch between the two reads them with the state the decisions were taken in: a
// wavefront per env books every decision of the policy (a member of live[b] that is not scripted) into the env's own rows, by
// round index and by the deciding node's degree.  No atomics (an env owns its rows), no host read, no allocation: it replays
// from the round loop's HIP graphs.  It writes nothing the round loop reads.
//
//   decision_record_kernel<W>      4 envs per 256-lane workgroup like env_round_kernel; a lane holds node `lane` (and lane + 64)
//                                  for the loads, lane l holds field l % 8 of a decision's row.  The decisions are walked in
//                                  ascending node id with v_readlane, one after the other: the order of the floating sums is
//                                  fixed.  The round's row is summed in registers, the touched degree rows in LDS.
//   decision_record_read_kernel    a thread per (row, field) adds the envs in ascending order: equal inputs, equal bits.
// Latency-sized launches (an env has about N / 6 decisions per round): nothing here is tuned for throughput.
#pragma once

namespace mel {

// value of node i (wave-uniform) from per-lane values v[h] = value of node lane + 64 h
template <int W> __device__ __forceinline__ float node_f32(const float (&v)[W], int i) {
    if constexpr (W == 1) return lane_f32(v[0], i);
    else return i < 64 ? lane_f32(v[0], i) : lane_f32(v[1], i - 64);
}

template <int W>
__global__ __launch_bounds__(256) void decision_record_kernel(mel_decision_record g, mel_env_batch e, const float* __restrict__ logits,
                                                              const int32_t* __restrict__ act, const int32_t* __restrict__ row_offsets,
                                                              const uint64_t* __restrict__ live) {
    const int b = wave_env();
    if (b >= g.n_envs) return;
    const int lane = lane_id();
    const int n = e.n_nodes;
    const int32_t* sc = e.scalars + (size_t)b * MEL_ENV_SCALARS;
    if (uniform_i32(sc[MEL_S_ERROR]) != 0) {
        if (lane == 0) g.skipped[b] += 1;
        return;
    }
    const int ep = uniform_i32(sc[MEL_S_EPISODES_DONE]), mv = uniform_i32(sc[MEL_S_NUM_MOVES]);
    if (g.quota && ep >= uniform_i32(g.quota[b])) return;            // a surplus episode of a spread evaluation
    const NodeSet<W> live_in = ns_uniform(ns_load<W>(live, b)) & ns_full<W>(n);
    const NodeSet<W> scripted = ns_uniform(ns_load<W>(e.node_sets + (size_t)b * 8 * W, MEL_SET_SCRIPTED));
    const NodeSet<W> taken = ns_uniform(ns_load<W>(e.sel_sets + (size_t)b * 4 * W, MEL_SEL_TAKEN_ACTION));
    const NodeSet<W> deciding = live_in & ~scripted;
    if (!ns_any(deciding)) return;
    // every deciding node's logits row, action and degree in one go (lane = node), read back with v_readlane below
    const int row0 = row_offsets ? uniform_i32(row_offsets[b]) : b;
    float q0[W], q1[W];
    int a[W], deg[W];
    NodeSet<W> relaying;
    MEL_W_FOR(h) {
        const int node = lane + 64 * h;
        const bool mine = ns_mine(deciding, lane, h);
        q0[h] = q1[h] = 0.f, a[h] = 0, deg[h] = 0;
        if (mine) {
            const size_t row = row_offsets ? (size_t)(row0 + ns_rank_below(live_in, node)) : (size_t)b;
            q0[h] = logits[row * 2], q1[h] = logits[row * 2 + 1];
            a[h] = row_offsets ? act[row] : act[(size_t)b * n + node];
            const int d = (int)e.obs_matrix[((size_t)b * n + node) * 8 + 2];
            deg[h] = d < 0 ? 0 : (d < g.n_degrees ? d : g.n_degrees - 1);
        }
        relaying.w[h] = __ballot(mine && a[h] == 1);
    }
    const bool keep_round = mv >= 0 && mv < g.max_rounds;
    double* round_row = g.by_round + ((size_t)b * g.max_rounds + (keep_round ? mv : 0)) * MEL_DR_FIELDS;
    double* degree_rows = g.by_degree + (size_t)b * g.n_degrees * MEL_DR_FIELDS;
    double sum = (keep_round && lane < MEL_DR_FIELDS) ? round_row[lane] : 0.0;      // the round's row: read once, written once
    // The degree rows this launch touches wait in LDS for the walk (a read-add-write per decision on global memory is a chain
    // of memory latencies).  Element e = row * 8 + field belongs to lane e % 64 from its load to its store - row d is added to
    // by the lanes 8 (d % 8) .. 8 (d % 8) + 7 - so no lane ever reads what another lane wrote.
    __shared__ double degree_lds[4][MEL_DR_MAX_DEGREES * MEL_DR_FIELDS];
    double* tab = degree_lds[threadIdx.x >> 6];
    NodeSet<2> my_rows = ns_zero<2>();
    MEL_W_FOR(h) if (ns_mine(deciding, lane, h)) my_rows |= ns_bit<2>(deg[h]);
    const NodeSet<2> touched = ns_uniform(ns_wave_or(my_rows));
    const int elems = g.n_degrees * MEL_DR_FIELDS;
    for (int el = lane; el < elems; el += 64)
        if (ns_test(touched, el >> 3)) tab[el] = degree_rows[el];
    const int f = lane & 7;                                              // the field this lane holds of a decision's row
    for (NodeSet<W> rest = deciding; ns_any(rest); ns_clear_lowest(rest)) {
        const int i = ns_lowest(rest);
        const float x0 = node_f32<W>(q0, i), x1 = node_f32<W>(q1, i);
        const int ai = node_i32<W>(a, i), d = node_i32<W>(deg, i);
        const float q[8] = {x0, x1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int greedy = greedy_action(q, 0.f, 0.f, 2);            // the fused selection's rule at eps = 0: ties agree
        const double gap = (double)(x1 - x0);                        // one fp32 subtraction, widened
        double v = 1.0;                                              // field 0: decisions
        v = f == 1 ? (ai == 1 ? 1.0 : 0.0) : v;
        v = f == 2 ? gap : v;
        v = f == 3 ? gap * gap : v;
        v = f == 4 ? (double)(ai == 1 ? x1 : x0) : v;
        v = f == 5 ? (double)(x1 > x0 ? x1 : x0) : v;
        v = f == 6 ? (ai != greedy ? 1.0 : 0.0) : v;
        v = f == 7 ? (ns_test(taken, i) ? 0.0 : 1.0) : v;
        sum += v;                                                    // (lanes 0 .. 7 hold the round's row)
        if ((lane >> 3) == (d & 7)) tab[d * MEL_DR_FIELDS + f] += v;
    }
    for (int el = lane; el < elems; el += 64)
        if (ns_test(touched, el >> 3)) degree_rows[el] = tab[el];
    const int count = ns_count(deciding);
    if (keep_round) {
        if (lane < MEL_DR_FIELDS) round_row[lane] = sum;
    } else if (lane == 0) {
        g.overflow[b] += count;
    }
    const int t = trace_slot(g, b);                                  // trace sink: is this env listed?
    if (t >= 0) {
        const TraceRecord tr = trace_open(g, t, lane, b, ep, sc[MEL_S_EPISODE], mv, count, ns_count(relaying));
        const size_t rec = tr.rec;
        MEL_W_FOR(w) {
            if (lane == w) g.trace_sets[rec * 2 * W + w] = deciding.w[w];
            if (lane == W + w) g.trace_sets[rec * 2 * W + W + w] = relaying.w[w];
        }
        MEL_W_FOR(h) {
            const int node = lane + 64 * h;
            if (node < n) {                                          // (q0 / q1 are 0 for a node that did not decide)
                g.trace_q[(rec * n + node) * 2] = q0[h];
                g.trace_q[(rec * n + node) * 2 + 1] = q1[h];
            }
        }
        trace_close(g, t, lane, tr);
    }
}

__global__ __launch_bounds__(256) void decision_record_read_kernel(mel_decision_record g, double* __restrict__ by_round_out,
                                                                   double* __restrict__ by_degree_out,
                                                                   long long* __restrict__ counters_out) {
    const size_t per_round = (size_t)g.max_rounds * MEL_DR_FIELDS, per_degree = (size_t)g.n_degrees * MEL_DR_FIELDS;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;            // (row, field): the rounds' rows, then the degrees'
    if (i < per_round) by_round_out[i] = fold_rows(g.by_round, g.n_envs, per_round, i);
    else if (i < per_round + per_degree) by_degree_out[i - per_round] = fold_rows(g.by_degree, g.n_envs, per_degree, i - per_round);
    if (i == 0) {
        counters_out[MEL_DRC_OVERFLOW] = fold_counter(g.overflow, g.n_envs);
        counters_out[MEL_DRC_SKIPPED] = fold_counter(g.skipped, g.n_envs);
        counters_out[2] = 0, counters_out[3] = 0;
    }
}

inline mel_status check_decision_record(const mel_decision_record* g, const char* who) {
    if (!g) return fail(MEL_ERR_INVALID_ARG, "%s: record is null", who);
    if (!g->by_round || !g->by_degree || !g->overflow || !g->skipped)
        return fail(MEL_ERR_INVALID_ARG, "%s: the record has a null buffer (by_round, by_degree, overflow, skipped)", who);
    if (g->max_rounds < 1 || g->max_rounds > MEL_DR_MAX_ROUNDS || g->n_degrees < 1 || g->n_degrees > MEL_DR_MAX_DEGREES ||
        g->n_envs < 1 || g->n_nodes < 1 || g->n_nodes > MEL_MAX_NODES)
        return fail(MEL_ERR_INVALID_ARG, "%s: max_rounds=%d outside [1, %d], n_degrees=%d outside [1, %d], n_envs=%d < 1 or n_nodes=%d outside [1, %d]",
                    who, g->max_rounds, MEL_DR_MAX_ROUNDS, g->n_degrees, MEL_DR_MAX_DEGREES, g->n_envs, g->n_nodes, MEL_MAX_NODES);
    return check_trace_sink(g, who, g->trace_sets && g->trace_q);
}

}  // namespace mel

extern "C" {

mel_status mel_decision_record_round(const mel_decision_record* rec, const mel_env_batch* env, const float* logits,
                                     const int32_t* act, const int32_t* row_offsets, const uint64_t* live, int32_t n_actions,
                                     void* stream) {
    if (mel_status st = mel::check_decision_record(rec, "mel_decision_record_round")) return st;
    if (!env) return mel::fail(MEL_ERR_INVALID_ARG, "mel_decision_record_round: env is null");
    if (!env->scalars || !env->node_sets || !env->sel_sets || !env->obs_matrix)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_decision_record_round: the env batch is not bound");
    if (env->n_envs != rec->n_envs || env->n_nodes != rec->n_nodes)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_decision_record_round: the record is for %d envs of %d nodes, the env batch has %d of %d",
                         rec->n_envs, rec->n_nodes, env->n_envs, env->n_nodes);
    if (!logits || !act || !live)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_decision_record_round: null input (logits, act, live)");
    if (n_actions != 2)
        return mel::fail(MEL_ERR_UNSUPPORTED, "mel_decision_record_round: n_actions=%d, the record is of two actions (relay is action 1)",
                         n_actions);
    mel::clear_stale_error();
    mel::with_env_waves(rec->n_envs, env->n_nodes, [&](auto w, dim3 grid, dim3 block) {
        MEL_LAUNCH(mel::decision_record_kernel<decltype(w)::value>, grid, block, 0, static_cast<hipStream_t>(stream), *rec, *env, logits,
                   act, row_offsets, live);
    });
    return mel::check_launch("mel_decision_record_round");
}

mel_status mel_decision_record_read(const mel_decision_record* rec, double* by_round_out, double* by_degree_out,
                                    int64_t* counters_out, void* stream) {
    if (mel_status st = mel::check_decision_record(rec, "mel_decision_record_read")) return st;
    if (!by_round_out || !by_degree_out || !counters_out)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_decision_record_read: null output (by_round_out, by_degree_out, counters_out)");
    mel::clear_stale_error();
    const unsigned blocks = (unsigned)(((size_t)(rec->max_rounds + rec->n_degrees) * MEL_DR_FIELDS + 255) / 256);
    MEL_LAUNCH(mel::decision_record_read_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), *rec, by_round_out,
               by_degree_out, reinterpret_cast<long long*>(counters_out));
    return mel::check_launch("mel_decision_record_read");
}

}  // extern "C"
