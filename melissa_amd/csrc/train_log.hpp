// Training curves accumulated on the device (included by env.hip; the contract is at mel_train_log in melissa_hip.h).  What the
// reference hands to [3P] tianshou's logger about every 1000 env steps (l_dgn.py:203-213,237-238,260) is summed here per interval of
// env steps into a caller-owned ring of records, by launches that replay from the round loop's and the update's HIP graphs: no host
// read, no allocation, no float atomics, every sum in a fixed order.
//
//   train_log_round_kernel    ONE workgroup of 256 lanes behind every env round.  The episode log's rows arrive in atomic order, so they
//                             are scattered by env id first (LDS: rows per env and one row index, TRAIN_LOG_ENV_PASS envs per pass
//                             over the rows), then lane t folds envs t, t + 256, ... in ascending order and the lanes meet in a
//                             pairwise LDS tree: the sums do not depend on the order the rows were appended in.  An env with several
//                             rows (never in a loop that drains every round) walks them in (pool episode, row) order.
//   train_log_grad_kernel     a workgroup per MEL_TRAIN_LOG_GRAD_CHUNK elements of one gradient tensor: widen, square (exact in
//                             double), lane-strided sums, the same tree -> scratch[workgroup].
//   train_log_update_kernel   one wavefront: adds the partials (a run per lane, then the lanes in order), sqrt; loss, mean |td|,
//                             max |td|; writes the record.
// Both record writers find their slot from the env batch's decision counters (train_log_slot): the rule lives once.
// These are latency-sized launches (a few hundred rows, a million gradient elements): nothing here is tuned for throughput.
#pragma once

namespace mel {

constexpr int TRAIN_LOG_ENV_PASS = 2048;      // envs scattered per pass over the rows (a multiple of 256)

// maxima / minima in which a NaN wins and then stays (fmax / fmin would drop it, see td.hpp)
__device__ __forceinline__ void tl_max(double& m, double v) {
    if (v > m || v != v) m = v;
}
__device__ __forceinline__ void tl_min(double& m, double v) {
    if (v < m || v != v) m = v;
}

// the record of env_step's interval, cleared and renamed when the slot held another one; null while nothing is recorded.
// Called by ONE lane.
__device__ inline double* train_log_slot(const mel_train_log& g, unsigned long long env_step) {
    const unsigned long long base = *g.base;
    if (base == ~0ull || env_step < base) return nullptr;
    const long long k = (long long)((env_step - base) / (unsigned long long)g.interval);
    const int slot = (int)(k % g.capacity);
    double* rec = g.records + (size_t)slot * MEL_TRAIN_LOG_DOUBLES;
    const long long old = g.interval_id[slot];
    if (old != k) {
        if (old >= 0 && old >= *g.drained_upto) g.counters[MEL_TLC_LOST_RECORDS] += 1;
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        for (int f = 0; f < MEL_TRAIN_LOG_DOUBLES; ++f) rec[f] = 0.0;
        rec[MEL_TL_REW_MIN] = inf;
        rec[MEL_TL_REW_MAX] = rec[MEL_TL_LOSS_MAX] = rec[MEL_TL_TD_ABS_MEAN_MAX] = rec[MEL_TL_TD_ABS_MAX] = rec[MEL_TL_GRAD_NORM_MAX] = -inf;
        rec[MEL_TL_EPS_LAST] = -1.0;
        g.interval_id[slot] = k;
    }
    return rec;
}

// per-lane share of scale * sum_b decisions[b * stride] (before the scale); integers: any order gives the same sum
__device__ __forceinline__ long long train_log_decisions(const mel_train_log& g, int tid, int threads) {
    long long d = 0;
    for (int b = tid; b < g.n_envs; b += threads) d += (long long)g.decisions[(size_t)b * g.stride];
    return d;
}

enum { TLA_N, TLA_SUM, TLA_SQ, TLA_MIN, TLA_MAX, TLA_MOVES, TLA_COV, TLA_COVI, TLA_MSGS, TLA_FIELDS };

__device__ __forceinline__ void train_log_fold(double (&a)[TLA_FIELDS], const double* __restrict__ stats, const int* __restrict__ meta, int r) {
    const double* s = stats + (size_t)r * MEL_ENV_LOGGER_STATS;
    const double v = s[9];                    // episode_rewards_sum (graph.py:166-178 in dict order)
    a[TLA_N] += 1.0, a[TLA_SUM] += v, a[TLA_SQ] += v * v;
    tl_min(a[TLA_MIN], v), tl_max(a[TLA_MAX], v);
    a[TLA_MOVES] += (double)meta[(size_t)r * 3 + 2];
    a[TLA_COV] += s[1], a[TLA_COVI] += s[6], a[TLA_MSGS] += s[0];
}

__global__ __launch_bounds__(256) void train_log_round_kernel(mel_train_log g, int* __restrict__ cursor, int log_capacity,
                                                              const double* __restrict__ stats, const int* __restrict__ meta,
                                                              const float* __restrict__ eps_dev) {
    __shared__ double red[TLA_FIELDS][256];
    __shared__ long long dec[256];
    __shared__ int cnt[TRAIN_LOG_ENV_PASS], one_row[TRAIN_LOG_ENV_PASS];
    __shared__ int dup, bad;
    const int tid = threadIdx.x;
    const int total = *cursor;
    const int n = total < 0 ? 0 : (total < log_capacity ? total : log_capacity);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double a[TLA_FIELDS];
    for (int f = 0; f < TLA_FIELDS; ++f) a[f] = 0.0;
    a[TLA_MIN] = inf, a[TLA_MAX] = -inf;
    dec[tid] = train_log_decisions(g, tid, 256);
    if (tid == 0) dup = 0, bad = 0;
    for (int c0 = 0; c0 < g.n_envs && n > 0; c0 += TRAIN_LOG_ENV_PASS) {
        const int c1 = c0 + TRAIN_LOG_ENV_PASS < g.n_envs ? c0 + TRAIN_LOG_ENV_PASS : g.n_envs;
        for (int j = tid; j < TRAIN_LOG_ENV_PASS; j += 256) cnt[j] = 0, one_row[j] = -1;
        __syncthreads();
        for (int r = tid; r < n; r += 256) {
            const int b = meta[(size_t)r * 3];
            if (b >= c0 && b < c1) atomicAdd(&cnt[b - c0], 1), atomicMax(&one_row[b - c0], r);
            else if (c0 == 0 && (b < 0 || b >= g.n_envs)) atomicAdd(&bad, 1);
        }
        __syncthreads();
        for (int b = c0 + tid; b < c1; b += 256) {          // (c0 is a multiple of 256: lane t keeps envs t, t + 256, ... in order)
            const int c = cnt[b - c0];
            if (c == 1) train_log_fold(a, stats, meta, one_row[b - c0]);
            else if (c > 1) {
                atomicAdd(&dup, c - 1);
                const long long none = 0x7fffffffffffffffll;
                long long last = -none - 1;                 // key = pool episode * 2^32 + row, ascending
                for (int k = 0; k < c; ++k) {
                    long long best = none;
                    int at = -1;
                    for (int r = 0; r < n; ++r) {
                        if (meta[(size_t)r * 3] != b) continue;
                        const long long key = (long long)meta[(size_t)r * 3 + 1] * 4294967296ll + (long long)r;
                        if (key > last && key < best) best = key, at = r;
                    }
                    if (at < 0) break;
                    train_log_fold(a, stats, meta, at);
                    last = best;
                }
            }
        }
        __syncthreads();
    }
    for (int f = 0; f < TLA_FIELDS; ++f) red[f][tid] = a[f];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            dec[tid] += dec[tid + o];
            for (int f = 0; f < TLA_FIELDS; ++f) {
                if (f == TLA_MIN) tl_min(red[f][tid], red[f][tid + o]);
                else if (f == TLA_MAX) tl_max(red[f][tid], red[f][tid + o]);
                else red[f][tid] += red[f][tid + o];
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    *cursor = 0;
    const unsigned long long env_step = (unsigned long long)g.scale * (unsigned long long)dec[0];
    double* rec = train_log_slot(g, env_step);
    if (!rec) return;
    const long long lost = (long long)(total > log_capacity ? total - log_capacity : 0) + bad;
    if (lost) g.counters[MEL_TLC_LOST_EPISODES] += lost;
    if (dup) g.counters[MEL_TLC_DUPLICATE_ENV_ROWS] += dup;
    rec[MEL_TL_EPISODES] += red[TLA_N][0];
    rec[MEL_TL_REW_SUM] += red[TLA_SUM][0];
    rec[MEL_TL_REW_SQ] += red[TLA_SQ][0];
    tl_min(rec[MEL_TL_REW_MIN], red[TLA_MIN][0]);
    tl_max(rec[MEL_TL_REW_MAX], red[TLA_MAX][0]);
    rec[MEL_TL_MOVES_SUM] += red[TLA_MOVES][0];
    rec[MEL_TL_COVERAGE_SUM] += red[TLA_COV][0];
    rec[MEL_TL_COV_INTERESTED_SUM] += red[TLA_COVI][0];
    rec[MEL_TL_MESSAGES_SUM] += red[TLA_MSGS][0];
    rec[MEL_TL_ROUNDS] += 1.0;
    rec[MEL_TL_ENV_STEP_LAST] = (double)env_step;
    if (eps_dev) rec[MEL_TL_EPS_LAST] = (double)*eps_dev;
}

struct TrainLogGrads {
    const float* grad[MEL_ADAM_MAX_TENSORS];
    long long chunks[MEL_ADAM_MAX_TENSORS];
    long long numel[MEL_ADAM_MAX_TENSORS];
    int count;
};

__global__ __launch_bounds__(256) void train_log_grad_kernel(TrainLogGrads t, double* __restrict__ partial) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    long long blk = blockIdx.x;
    int i = 0;
    for (; i < t.count; ++i) {                               // (block-uniform) which tensor, which of its chunks
        if (blk < t.chunks[i]) break;
        blk -= t.chunks[i];
    }
    double s = 0.0;
    if (i < t.count) {
        const float* __restrict__ gr = t.grad[i];
        const long long lo = blk * MEL_TRAIN_LOG_GRAD_CHUNK;
        const long long hi = lo + MEL_TRAIN_LOG_GRAD_CHUNK < t.numel[i] ? lo + MEL_TRAIN_LOG_GRAD_CHUNK : t.numel[i];
        for (long long e = lo + tid; e < hi; e += 256) {
            const double v = (double)gr[e];
            s += v * v;                                      // 24-bit significand squared: exact in double
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void train_log_update_kernel(mel_train_log g, const float* __restrict__ loss, const float* __restrict__ td,
                                                              int batch, const double* __restrict__ partial, long long groups) {
    const int lane = threadIdx.x;
    long long d = train_log_decisions(g, lane, 64);
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    // the gradient's squared norm: a run of consecutive partials per lane, then the lanes in order
    const long long per = (groups + 63) / 64;
    double s = 0.0;
    for (long long k = lane * per; k < (lane + 1) * per && k < groups; ++k) s += partial[k];
    // |td|: lane-strided in double, then the lanes in order
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double a = 0.0, m = -inf;
    for (int i = lane; i < batch; i += 64) {
        const double v = fabs((double)td[i]);
        a += v;
        tl_max(m, v);
    }
    double sq = 0.0, asum = 0.0, amax = -inf;
    for (int l = 0; l < 64; ++l) {
        sq += __shfl(s, l, 64);
        asum += __shfl(a, l, 64);
        tl_max(amax, __shfl(m, l, 64));
    }
    if (lane != 0) return;
    const unsigned long long env_step = (unsigned long long)g.scale * (unsigned long long)d;
    double* rec = train_log_slot(g, env_step);
    if (!rec) return;
    const double l = (double)*loss, mean_abs = asum / (double)batch, norm = sqrt(sq);
    rec[MEL_TL_UPDATES] += 1.0;
    rec[MEL_TL_LOSS_SUM] += l;
    tl_max(rec[MEL_TL_LOSS_MAX], l);
    rec[MEL_TL_LOSS_LAST] = l;
    rec[MEL_TL_TD_ABS_SUM] += mean_abs;
    tl_max(rec[MEL_TL_TD_ABS_MEAN_MAX], mean_abs);
    tl_max(rec[MEL_TL_TD_ABS_MAX], amax);
    rec[MEL_TL_GRAD_NORM_SUM] += norm;
    tl_max(rec[MEL_TL_GRAD_NORM_MAX], norm);
    rec[MEL_TL_GRAD_NORM_LAST] = norm;
    rec[MEL_TL_ENV_STEP_LAST] = (double)env_step;
}

inline mel_status check_train_log(const mel_train_log* g, const char* who) {
    if (!g) return fail(MEL_ERR_INVALID_ARG, "%s: log is null", who);
    if (!g->records || !g->interval_id || !g->counters || !g->base || !g->drained_upto || !g->decisions)
        return fail(MEL_ERR_INVALID_ARG, "%s: the log has a null buffer (records, interval_id, counters, base, drained_upto, decisions)", who);
    if (g->capacity < 1 || g->interval < 1 || g->n_envs < 1 || g->stride < 1)
        return fail(MEL_ERR_INVALID_ARG, "%s: capacity=%d, interval=%ld, n_envs=%d, stride=%d must all be >= 1", who, g->capacity,
                    (long)g->interval, g->n_envs, g->stride);
    return MEL_OK;
}

// chunks of every tensor; -1 for a table the launches refuse
inline long long train_log_grad_chunks(const mel_adam_tensors* t, TrainLogGrads* out) {
    if (!t || t->count < 1 || t->count > MEL_ADAM_MAX_TENSORS) return -1;
    long long groups = 0;
    for (int i = 0; i < t->count; ++i) {
        if (!t->grad[i] || t->numel[i] < 0) return -1;
        const long long c = ((long long)t->numel[i] + MEL_TRAIN_LOG_GRAD_CHUNK - 1) / MEL_TRAIN_LOG_GRAD_CHUNK;
        if (out) out->grad[i] = t->grad[i], out->numel[i] = t->numel[i], out->chunks[i] = c;
        groups += c;
    }
    if (out) out->count = t->count;
    return groups;
}

}  // namespace mel

extern "C" {

size_t mel_train_log_scratch_bytes(const mel_adam_tensors* grads) {
    const long long groups = mel::train_log_grad_chunks(grads, nullptr);
    return groups < 0 ? 0 : (size_t)groups * sizeof(double);
}

mel_status mel_train_log_round(const mel_train_log* log, const mel_env_batch* env, const float* eps_dev, void* stream) {
    if (mel_status st = mel::check_train_log(log, "mel_train_log_round")) return st;
    if (!env) return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_round: env is null");
    if (env->log_capacity < 1 || !env->log_cursor || !env->log_stats || !env->log_meta)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_round: the env batch has no episode log (log_capacity=%d)", env->log_capacity);
    if (env->n_envs != log->n_envs)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_round: the log counts %d envs, the env batch has %d", log->n_envs, env->n_envs);
    mel::clear_stale_error();
    MEL_LAUNCH(mel::train_log_round_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), *log, env->log_cursor,
               env->log_capacity, env->log_stats, env->log_meta, eps_dev);
    return mel::check_launch("mel_train_log_round");
}

mel_status mel_train_log_update(const mel_train_log* log, const float* loss, const float* td, int64_t batch,
                                const mel_adam_tensors* grads, void* scratch, size_t scratch_bytes, void* stream) {
    if (mel_status st = mel::check_train_log(log, "mel_train_log_update")) return st;
    if (!loss || !td || !grads) return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_update: null pointer (loss, td or grads)");
    if (batch < 1 || batch > MEL_TD_MAX_BATCH)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_update: batch=%ld outside [1, %d]", (long)batch, MEL_TD_MAX_BATCH);
    mel::TrainLogGrads t{};
    const long long groups = mel::train_log_grad_chunks(grads, &t);
    if (groups < 0 || groups > 0x7fffffffll)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_train_log_update: 1 .. %d gradient tensors, none null, numel >= 0", MEL_ADAM_MAX_TENSORS);
    if (groups > 0 && (!scratch || scratch_bytes < (size_t)groups * sizeof(double)))
        return mel::fail(MEL_ERR_WORKSPACE, "mel_train_log_update: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : (size_t)0,
                         (size_t)groups * sizeof(double));
    mel::clear_stale_error();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (groups > 0) {
        MEL_LAUNCH(mel::train_log_grad_kernel, dim3((unsigned)groups), dim3(256), 0, s, t, static_cast<double*>(scratch));
        if (mel_status st = mel::check_launch("mel_train_log_update (gradient partials)")) return st;
    }
    MEL_LAUNCH(mel::train_log_update_kernel, dim3(1), dim3(64), 0, s, *log, loss, td, (int)batch, static_cast<const double*>(scratch),
               groups);
    return mel::check_launch("mel_train_log_update");
}

}  // extern "C"
