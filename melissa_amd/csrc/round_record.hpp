// Per-round dissemination curves and node traces of an evaluation, recorded on the device (included by env.hip; the contract is
// at mel_round_record in melissa_hip.h).  What the reference shows by drawing the graph after every world step (graph.py:350-356,
// 466-484) is sampled here by ONE launch behind every mel_env_round: a wavefront per env reads the state the round left and adds
// one sample to the env's own rows.  No atomics (an env owns its rows), no host read, no allocation: it replays from the round
// loop's HIP graphs.  What the launch can see (env_round_kernel's loop): an env's loop ends at a world step or at an episode end
// with reset, so the state is "after world step num_moves" or "the new episode's reset state, num_moves == 0".  One thing IS lost to
// a kernel that runs afterwards: when the observation right after a world step raises explicit_reset (graph.py:205-211) the episode
// ends in the launch of its last world step, and the state after that step is gone.  Its figures survive in the env batch's episode
// log (log_episode: the final observation's logger_stats and num_moves), so an env whose episode has ended looks its row up there:
// the row's figures are what `ended` books (they are what an evaluation reports for the episode), and where the row is past the
// env's last sample, the episode's final sample comes from the row too.
//
//   round_record_kernel<W>      4 envs per 256-lane workgroup like env_round_kernel; lane f < 8 holds field f of the sample.
//   round_record_read_kernel    a thread per (round, field) adds the envs in ascending order: equal inputs, equal bits.
// Latency-sized launches (about 200 B read and 128 B written per env): nothing here is tuned for throughput.
#pragma once

namespace mel {

template <int W>
__global__ __launch_bounds__(256) void round_record_kernel(mel_round_record g, mel_env_batch e) {
    const int b = wave_env();
    if (b >= g.n_envs) return;
    const int lane = lane_id();
    const int n = e.n_nodes;
    const int32_t* sc = e.scalars + (size_t)b * MEL_ENV_SCALARS;
    const int ep = uniform_i32(sc[MEL_S_EPISODES_DONE]), mv = uniform_i32(sc[MEL_S_NUM_MOVES]);
    int32_t* carry = g.seen + (size_t)b * MEL_RR_CARRY;
    const int seen_ep = uniform_i32(carry[0]), seen_mv = uniform_i32(carry[1]);
    if (ep == seen_ep && mv == seen_mv) return;                      // this state has been sampled: a second launch adds nothing
    if (uniform_i32(sc[MEL_S_ERROR]) != 0) {
        if (lane == 0) g.skipped[b] += 1;
        return;
    }
    int last_r = uniform_i32(carry[2]), last_full = uniform_i32(carry[3]);
    const size_t rows = (size_t)b * g.max_rounds;
    double* last = g.last + (size_t)b * MEL_RR_FIELDS;
    int over = 0, unlogged = 0;
    // the episode log's rows this env has not looked at yet: [log_from, log_to)
    const int log_total = uniform_i32(*e.log_cursor);
    const int log_to = log_total < 0 ? 0 : (log_total < e.log_capacity ? log_total : e.log_capacity);
    const int log_seen = uniform_i32(carry[4]);
    const int log_from = (log_seen < 0 || log_seen > log_to) ? 0 : log_seen;      // (a cursor that went back: the log was emptied)
    if (ep != seen_ep) {                                             // the previous episode ended
        if (last_r >= 0) {
            // its row: the newest of this env's (an env ends at most one episode per round launch)
            int row = -1;
            if (log_total <= e.log_capacity)                         // (a log that dropped rows may lack this one: no guess)
                for (int k = log_from + lane; k < log_to; k += 64) row = e.log_meta[(size_t)k * 3] == b ? k : row;
            for (int o = 32; o > 0; o >>= 1) {
                const int other = __shfl_xor(row, o, 64);
                row = other > row ? other : row;
            }
            row = uniform_i32(row);
            const int final_r = row >= 0 ? uniform_i32(e.log_meta[(size_t)row * 3 + 2]) : last_r;
            if (row < 0) unlogged = 1;                                // no row (the log is full): booked at its last sample
            double end_v = lane < MEL_RR_FIELDS ? last[lane] : 0.0;
            if (row >= 0) {
                // the row's figures are the logger_stats the episode's final observation carried - what an evaluation
                // reports for it (log_episode: the selected agent's slot AS STORED, stale or not)
                const double* st = e.log_stats + (size_t)row * MEL_ENV_LOGGER_STATS;
                const double n_int = st[5], cov_int = st[7];
                const int full = n_int > 0.0 && cov_int == n_int;
                double v = 1.0;
                v = lane == 1 ? (double)(int)(st[1] * (double)n + 0.5) : v;          // coverage = |has_message| / n
                v = lane == 2 ? cov_int : v;
                v = lane == 3 ? n_int : v;
                v = lane == 4 ? st[0] : v;
                v = lane == 5 ? 0.0 : v;                              // the episode is over: nobody acts
                v = lane == 6 ? st[6] : v;
                v = lane == 7 ? ((full && !last_full) ? 1.0 : 0.0) : v;
                if (final_r != last_r) {
                    // the episode's last world step ran in the launch that ended it: its final sample comes from the row
                    if (final_r >= 0 && final_r < g.max_rounds) {
                        if (lane < MEL_RR_FIELDS) g.running[(rows + final_r) * MEL_RR_FIELDS + lane] += v;
                    } else {
                        over += 1;
                    }
                    last_r = final_r;
                    end_v = v;
                } else {
                    end_v = (lane >= 1 && lane <= 4) || lane == 6 ? v : end_v;     // (fields 0, 5, 7: the last sample's)
                }
            }
            if (last_r >= 0 && last_r < g.max_rounds) {
                if (lane < MEL_RR_FIELDS) g.ended[(rows + last_r) * MEL_RR_FIELDS + lane] += end_v;
            } else {
                over += 1;
            }
        }
        last_r = -1, last_full = 0;
    }
    if (!g.quota || ep < uniform_i32(g.quota[b])) {
        const uint64_t* ns = e.node_sets + (size_t)b * 8 * W;
        const uint64_t* ss = e.sel_sets + (size_t)b * 4 * W;
        const NodeSet<W> has = ns_uniform(ns_load<W>(ns, MEL_SET_HAS_MESSAGE));
        const NodeSet<W> interested = ns_uniform(ns_load<W>(ns, MEL_SET_INTERESTED));
        const NodeSet<W> active = ns_uniform(ns_load<W>(ss, MEL_SEL_ACTIVE));
        const int msgs = uniform_i32(sc[MEL_S_WORLD_MSGS]);
        const int n_has = ns_count(has), n_int = ns_count(interested), cov_int = ns_count(has & interested);
        const double frac = n_int > 0 ? (double)cov_int / (double)n_int : 0.0;      // graph.py:158-162
        const int full = n_int > 0 && cov_int == n_int;
        double v = 1.0;                                               // lane 0: count
        v = lane == 1 ? (double)n_has : v;
        v = lane == 2 ? (double)cov_int : v;
        v = lane == 3 ? (double)n_int : v;
        v = lane == 4 ? (double)msgs : v;
        v = lane == 5 ? (double)ns_count(active) : v;
        v = lane == 6 ? frac : v;
        v = lane == 7 ? ((full && !last_full) ? 1.0 : 0.0) : v;
        if (mv < g.max_rounds) {
            if (lane < MEL_RR_FIELDS) g.running[(rows + mv) * MEL_RR_FIELDS + lane] += v;
        } else {
            over += 1;
        }
        if (lane < MEL_RR_FIELDS) last[lane] = v;
        last_r = mv, last_full = full;
        const int t = trace_slot(g, b);                              // trace sink: is this env listed?
        if (t >= 0) {
            const TraceRecord tr = trace_open(g, t, lane, b, ep, sc[MEL_S_EPISODE], mv, sc[MEL_S_ORIGIN], msgs);
            const size_t rec = tr.rec;
            const size_t node0 = (size_t)b * n;
            for (int c = lane; c < 2 * n; c += 64) g.trace_pos[rec * 2 * n + c] = e.pos[node0 * 2 + c];
            for (int c = lane; c < n * W; c += 64) g.trace_one_hop[rec * n * W + c] = e.one_hop[node0 * W + c];
            if (lane < 6 * W) {
                const int k = lane / W, w = lane % W;
                g.trace_sets[rec * 6 * W + lane] = k < 4 ? ns[k * W + w] : ss[(k == 4 ? MEL_SEL_ACTIVE : MEL_SEL_TAKEN_ACTION) * W + w];
            }
            for (int c = lane; c < n; c += 64) {
                g.trace_agent_msgs[rec * n + c] = e.agent_msgs[node0 + c];
                g.trace_received[rec * n + c] = e.received[node0 + c];
            }
            trace_close(g, t, lane, tr);
        }
    }
    if (lane == 0) {
        carry[0] = ep, carry[1] = mv, carry[2] = last_r, carry[3] = last_full, carry[4] = log_to;
        if (over) g.overflow[b] += over;
        if (unlogged) g.unlogged[b] += 1;
    }
}

__global__ __launch_bounds__(256) void round_record_read_kernel(mel_round_record g, double* __restrict__ running_out,
                                                                double* __restrict__ ended_out, long long* __restrict__ counters_out) {
    const size_t per = (size_t)g.max_rounds * MEL_RR_FIELDS;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;            // (round, field)
    if (i < per) {
        running_out[i] = fold_rows(g.running, g.n_envs, per, i);
        ended_out[i] = fold_rows(g.ended, g.n_envs, per, i);
    }
    if (i == 0) {
        counters_out[MEL_RRC_OVERFLOW] = fold_counter(g.overflow, g.n_envs);
        counters_out[MEL_RRC_SKIPPED] = fold_counter(g.skipped, g.n_envs);
        counters_out[MEL_RRC_UNLOGGED] = fold_counter(g.unlogged, g.n_envs);
    }
}

inline mel_status check_round_record(const mel_round_record* g, const char* who) {
    if (!g) return fail(MEL_ERR_INVALID_ARG, "%s: record is null", who);
    if (!g->running || !g->ended || !g->seen || !g->last || !g->overflow || !g->skipped || !g->unlogged)
        return fail(MEL_ERR_INVALID_ARG, "%s: the record has a null buffer (running, ended, seen, last, overflow, skipped, unlogged)", who);
    if (g->max_rounds < 1 || g->max_rounds > MEL_RR_MAX_ROUNDS || g->n_envs < 1 || g->n_nodes < 1 || g->n_nodes > MEL_MAX_NODES)
        return fail(MEL_ERR_INVALID_ARG, "%s: max_rounds=%d outside [1, %d], n_envs=%d < 1 or n_nodes=%d outside [1, %d]", who,
                    g->max_rounds, MEL_RR_MAX_ROUNDS, g->n_envs, g->n_nodes, MEL_MAX_NODES);
    return check_trace_sink(g, who, g->trace_pos && g->trace_one_hop && g->trace_sets && g->trace_agent_msgs && g->trace_received);
}

}  // namespace mel

extern "C" {

mel_status mel_round_record_round(const mel_round_record* rec, const mel_env_batch* env, void* stream) {
    if (mel_status st = mel::check_round_record(rec, "mel_round_record_round")) return st;
    if (!env) return mel::fail(MEL_ERR_INVALID_ARG, "mel_round_record_round: env is null");
    if (!env->scalars || !env->node_sets || !env->sel_sets || !env->pos || !env->one_hop || !env->agent_msgs || !env->received)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_round_record_round: the env batch is not bound");
    if (env->log_capacity < 1 || !env->log_cursor || !env->log_stats || !env->log_meta)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_round_record_round: the env batch has no episode log (log_capacity=%d)", env->log_capacity);
    if (env->n_envs != rec->n_envs || env->n_nodes != rec->n_nodes)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_round_record_round: the record is for %d envs of %d nodes, the env batch has %d of %d",
                         rec->n_envs, rec->n_nodes, env->n_envs, env->n_nodes);
    mel::clear_stale_error();
    mel::with_env_waves(rec->n_envs, env->n_nodes, [&](auto w, dim3 grid, dim3 block) {
        MEL_LAUNCH(mel::round_record_kernel<decltype(w)::value>, grid, block, 0, static_cast<hipStream_t>(stream), *rec, *env);
    });
    return mel::check_launch("mel_round_record_round");
}

mel_status mel_round_record_read(const mel_round_record* rec, double* running_out, double* ended_out, int64_t* counters_out,
                                 void* stream) {
    if (mel_status st = mel::check_round_record(rec, "mel_round_record_read")) return st;
    if (!running_out || !ended_out || !counters_out)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_round_record_read: null output (running_out, ended_out, counters_out)");
    mel::clear_stale_error();
    const unsigned blocks = (unsigned)(((size_t)rec->max_rounds * MEL_RR_FIELDS + 255) / 256);
    MEL_LAUNCH(mel::round_record_read_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), *rec, running_out, ended_out,
               reinterpret_cast<long long*>(counters_out));
    return mel::check_launch("mel_round_record_read");
}

}  // extern "C"
