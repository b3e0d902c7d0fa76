// What mel_round_record and mel_decision_record share (included by env.hip before round_record.hpp and decision_record.hpp; the
// contract is at mel_round_record in melissa_hip.h): the trace sink - a ring of trace_capacity records for each of up to 16
// listed envs -, the fold of the envs' rows by the read launches and the launch geometry.  Templates over the record struct G,
// which read the members the two structs name alike.  Each kernel keeps its own prologue (carry, error skip, quota: their
// order is part of each contract) and writes its own payload arrays.
#pragma once

namespace mel {

static_assert(MEL_RR_MAX_TRACE == MEL_DR_MAX_TRACE, "the two recorders share one trace sink");

// slot of env b in trace_env[], -1 when it is not listed  (n_trace <= 16: a scalar walk over the launch's own arguments)
template <typename G> __device__ __forceinline__ int trace_slot(const G& g, int b) {
    int t = -1;
    for (int k = 0; k < g.n_trace; ++k) t = g.trace_env[k] == b ? k : t;
    return t;
}

struct TraceRecord {
    long long cur;      // trace_cursor[t] as the launch found it
    size_t rec;         // t * trace_capacity + cur % trace_capacity: the record's index in every trace array
};

// Open the next record of slot t and write its header: env, episode ordinal, MEL_S_EPISODE, num_moves, two ints of the
// recorder's own, 0, 0.  The whole wavefront calls it; lanes 0 .. 7 write.
template <typename G>
__device__ __forceinline__ TraceRecord trace_open(const G& g, int t, int lane, int b, int ep, int episode, int mv, int p0, int p1) {
    const long long cur = (long long)uniform_u64((uint64_t)g.trace_cursor[t]);
    const size_t rec = (size_t)t * g.trace_capacity + (size_t)(cur % g.trace_capacity);
    if (lane < 8) {
        int m = b;
        m = lane == 1 ? ep : m;
        m = lane == 2 ? episode : m;
        m = lane == 3 ? mv : m;
        m = lane == 4 ? p0 : m;
        m = lane == 5 ? p1 : m;
        m = lane >= 6 ? 0 : m;
        g.trace_meta[rec * 8 + lane] = m;
    }
    return {cur, rec};
}

// after the payload: the record counts
template <typename G> __device__ __forceinline__ void trace_close(const G& g, int t, int lane, const TraceRecord& r) {
    if (lane == 0) g.trace_cursor[t] = r.cur + 1;
}

// The read launches: element i of the envs' rows (per_env elements each), added in ascending env order by ONE thread - equal
// inputs give equal bits - and a per-env counter summed the same way.
__device__ __forceinline__ double fold_rows(const double* rows, int n_envs, size_t per_env, size_t i) {
    double s = 0.0;
    for (int b = 0; b < n_envs; ++b) s += rows[(size_t)b * per_env + i];
    return s;
}
__device__ __forceinline__ long long fold_counter(const int64_t* per_env, int n_envs) {
    long long s = 0;
    for (int b = 0; b < n_envs; ++b) s += per_env[b];
    return s;
}

// The argument errors of the sink; payload_buffers_present: none of the recorder's own trace arrays is null.
template <typename G> inline mel_status check_trace_sink(const G* g, const char* who, bool payload_buffers_present) {
    if (g->n_trace < 0 || g->n_trace > MEL_RR_MAX_TRACE)
        return fail(MEL_ERR_INVALID_ARG, "%s: n_trace=%d outside [0, %d]", who, g->n_trace, MEL_RR_MAX_TRACE);
    if (g->n_trace > 0) {
        if (g->trace_capacity < 1) return fail(MEL_ERR_INVALID_ARG, "%s: trace_capacity=%d must be >= 1", who, g->trace_capacity);
        if (!g->trace_cursor || !g->trace_meta || !payload_buffers_present)
            return fail(MEL_ERR_INVALID_ARG, "%s: the trace sink has a null buffer", who);
        for (int k = 0; k < g->n_trace; ++k) {
            if (g->trace_env[k] < 0 || g->trace_env[k] >= g->n_envs)
                return fail(MEL_ERR_INVALID_ARG, "%s: traced env %d is outside [0, %d)", who, g->trace_env[k], g->n_envs);
            for (int j = 0; j < k; ++j)
                if (g->trace_env[j] == g->trace_env[k])
                    return fail(MEL_ERR_INVALID_ARG, "%s: env %d is traced twice", who, g->trace_env[k]);
        }
    }
    return MEL_OK;
}

// A wavefront per env, 4 envs per 256-lane workgroup like env_round_kernel: the env of this wavefront (>= n_envs in the last
// workgroup's spare waves), and the launch of such a kernel - f(w, grid, block), w the words of a node set.
__device__ __forceinline__ int wave_env() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
template <typename F> inline void with_env_waves(int n_envs, int n_nodes, F&& f) {
    const dim3 grid((unsigned)((n_envs + 3) / 4));
    with_words(n_nodes, [&](auto w) { f(w, grid, dim3(256)); });
}

}  // namespace mel
