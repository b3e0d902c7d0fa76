// Prioritized experience replay on the device ([3P] tianshou 1.0.0 PrioritizedVectorReplayBuffer as the reference's scripts
// configure it with --prio-buffer, l_dgn.py:169-176; parity unpinned: restated from upstream's published behaviour).  Included by
// env.hip behind the uniform sampler, whose draw, n-step walk, per-sample outputs and observation copies it shares
// (replay_draw_bits / replay_emit_sample / replay_copy_obs).
//
// One priority per transition (env, slot, agent): prio [B, K, N] holds p^alpha, 0 for agents that did not act and for slots not
// yet filled, so the buffer order of upstream's prefix sums is this array's memory order.  Three launches:
//   refresh     one wavefront per record: records written since the last sample get max_prio^alpha (upstream's add(): max_prio
//               only changes in the write-back, and every write-back is preceded by a sample, so a record first seen by a sample
//               gets the max_prio it would have been added with), slots at or beyond min(cursor, K) get 0; every record's
//               priorities are summed in agent order into f64.
//   sample      one workgroup: f64 exclusive scan of the record sums in fixed order, per sample target = u * total, binary
//               search for the record, a walk over its N priorities for the agent, importance weights
//               (p^alpha / min_prio)^-beta [/ max over the batch].
//   write-back  one workgroup: prio <- (|td| + eps)^alpha, the highest sample index wins among duplicates, max_prio / min_prio.
// No float atomics: every result is a fixed-order reduction, two runs from the same state give the same bits.
#pragma once
#include <cfloat>

struct ReplayPrioSampleArgs {
    ReplaySampleArgs s;         // (s.prefix is the uniform sampler's scratch: unused here)
    mel_replay_priority pr;
    float* weight;              // [batch]
};

__global__ __launch_bounds__(256) void replay_prio_refresh_kernel(mel_round_replay rp, mel_replay_priority pr, int B, int n, int W) {
    const int lane = threadIdx.x & 63, K = rp.capacity;
    const int rec = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rec >= B * K) return;                              // (whole wavefronts)
    const int e = rec / K, k = rec - e * K;
    // written since the last sample: ring slots seen .. cursor - 1 (mod K), all K once the ring went round
    const int written = rp.cursor[e] - pr.seen[e];
    bool fresh = written >= K || written < 0;
    if (!fresh && written > 0) {
        int d = k - pr.seen[e] % K;
        d = d < 0 ? d + K : d;
        fresh = d < written;
    }
    float* p = pr.prio + (size_t)rec * n;
    float v0 = 0.f, v1 = 0.f;                              // agents lane and lane + 64
    if (k >= min(rp.cursor[e], K)) {
        // no record yet: never fresh (a cursor that went back makes the whole env "written", and acted holds stale sets here), and
        // never priority mass - the sample kernel has no filled check of its own
        if (lane < n) p[lane] = 0.f;
        if (lane + 64 < n) p[lane + 64] = 0.f;
    } else if (fresh) {
        const float init = powf(*pr.max_prio, (float)pr.alpha);
        const unsigned long long m0 = rp.acted[(size_t)rec * W];
        v0 = (m0 >> lane) & 1 ? init : 0.f;
        if (lane < n) p[lane] = v0;
        if (W == 2) {
            const unsigned long long m1 = rp.acted[(size_t)rec * W + 1];
            v1 = (m1 >> lane) & 1 ? init : 0.f;
            if (lane + 64 < n) p[lane + 64] = v1;
        }
    } else {
        v0 = lane < n ? p[lane] : 0.f;
        v1 = lane + 64 < n ? p[lane + 64] : 0.f;
    }
    double sum = 0.0;                                      // agent order, like the sample kernel's walk and a cumsum over [B, K, N]
    for (int i = 0; i < n; ++i) sum += (double)__shfl(i < 64 ? v0 : v1, i & 63);
    if (lane == 0) pr.rec_sum[rec] = sum;
}

__global__ __launch_bounds__(1024) void replay_sample_prio_kernel(ReplayPrioSampleArgs pa) {
    const ReplaySampleArgs& a = pa.s;
    const mel_replay_priority& pr = pa.pr;
    __shared__ double wave_tot[16];
    __shared__ ReplayPicks picks;
    const int tid = threadIdx.x, K = a.rp.capacity, BK = a.B * K;
    const int lane = tid & 63, wv = tid >> 6;
    // (1) exclusive scan of the record sums in a fixed order: every thread owns `per` consecutive records (serial sums), one block
    // scan over the 1 024 thread sums (shuffles inside the wave, LDS across the 16), then the thread's own prefixes
    const int per = (BK + 1023) / 1024, first = tid * per;
    double mine = 0.0;
    for (int j = 0; j < per; ++j)
        if (first + j < BK) mine += pr.rec_sum[first + j];
    double incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0.0;
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    double before = 0.0, total = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const double t = wave_tot[k];
        before += k < wv ? t : 0.0;
        total += t;
    }
    double at = before + excl;
    for (int j = 0; j < per; ++j)
        if (first + j < BK) {
            pr.prefix[first + j] = at;
            at += pr.rec_sum[first + j];
        }
    if (tid == 0) pr.prefix[BK] = total;
    __threadfence_block();
    __syncthreads();                                       // (also: wave_tot is free again for the weights' maximum)
    const unsigned long long draw = *a.counter;
    double w = 0.0;
    if (tid < a.batch) {
        int e = 0, k = 0, agent = 0;
        const bool picked = total > 0.0;
        w = 1.0;
        if (picked) {
            const unsigned long long z = replay_draw_bits(a.seed, draw, tid);
            const double target = ((double)(z >> 11) * 0x1.0p-53) * total;
            int l = 0, h = BK;                             // last record whose exclusive prefix is <= target
            while (h - l > 1) {
                const int m = (l + h) >> 1;
                if (pr.prefix[m] <= target) l = m;
                else h = m;
            }
            // (a target within rounding of a boundary: never a record without priority mass)
            while (l > 0 && !(pr.rec_sum[l] > 0.0)) --l;
            while (l < BK - 1 && !(pr.rec_sum[l] > 0.0)) ++l;
            // the first agent, in id order, whose inclusive sum exceeds what is left of the target
            const float* p = pr.prio + (size_t)l * a.n;
            const double local = target - pr.prefix[l];
            double acc = 0.0;
            int last = 0;
            agent = -1;
            for (int i = 0; i < a.n; ++i) {
                const float pi = p[i];
                if (!(pi > 0.f)) continue;
                acc += (double)pi;
                last = i;
                if (local < acc) { agent = i; break; }
            }
            if (agent < 0) agent = last;
            e = l / K, k = l - e * K;
            // upstream's simplified weight: the numerator is already p^alpha, the denominator the raw min_prio
            w = pow((double)p[agent] / (double)*pr.min_prio, -pr.beta);
        }
        replay_emit_sample(a, tid, picked, e, k, agent, picks);
    }
    // (2) batch maximum of the weights (all positive)
    double mx = w;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
    if (lane == 0) wave_tot[wv] = mx;
    __syncthreads();
    mx = wave_tot[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) mx = fmax(mx, wave_tot[k]);
    if (tid < a.batch) pa.weight[tid] = (float)(pr.weight_norm ? w / mx : w);
    replay_copy_obs(a, tid, picks);
    for (int b = tid; b < a.B; b += 1024) pr.seen[b] = a.rp.cursor[b];
    if (tid == 0) *a.counter = draw + 1;
}

__global__ __launch_bounds__(1024) void replay_prio_update_kernel(mel_replay_priority pr, int B, int K, int n, int batch,
                                                                  const long long* env, const long long* slot,
                                                                  const long long* agent, const float* td) {
    __shared__ long long key[1024];
    __shared__ float wave_max[16], wave_min[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long mine = -1;
    float p = 0.f;
    if (tid < batch) {
        const long long e = env[tid], k = slot[tid], i = agent[tid];
        p = fabsf(td[tid]) + FLT_EPSILON;                  // np.finfo(np.float32).eps
        if (e >= 0 && e < B && k >= 0 && k < K && i >= 0 && i < n) mine = (e * K + k) * n + i;
    }
    key[tid] = mine;
    __syncthreads();
    if (mine >= 0) {                                       // numpy's assignment: the last occurrence of an index wins
        bool last = true;
        for (int j = tid + 1; j < batch; ++j)
            if (key[j] == mine) { last = false; break; }
        if (last) pr.prio[mine] = powf(p, (float)pr.alpha);
    }
    float mx = tid < batch ? p : -FLT_MAX, mn = tid < batch ? p : FLT_MAX;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, d));
        mn = fminf(mn, __shfl_xor(mn, d));
    }
    if (lane == 0) wave_max[wv] = mx, wave_min[wv] = mn;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 16; ++k) mx = fmaxf(mx, wave_max[k]), mn = fminf(mn, wave_min[k]);
        *pr.max_prio = fmaxf(*pr.max_prio, mx);
        *pr.min_prio = fminf(*pr.min_prio, mn);
    }
}

static mel_status check_replay_priority(const mel_replay_priority* pr, const char* who) {
    if (!pr) return fail(MEL_ERR_INVALID_ARG, "%s: null argument", who);
    if (!pr->prio || !pr->rec_sum || !pr->prefix || !pr->seen || !pr->max_prio || !pr->min_prio)
        return fail(MEL_ERR_INVALID_ARG, "%s: incomplete priority block", who);
    if (!(pr->alpha >= 0.0)) return fail(MEL_ERR_INVALID_ARG, "%s: alpha = %g must be >= 0", who, pr->alpha);
    if (!(pr->beta >= 0.0)) return fail(MEL_ERR_INVALID_ARG, "%s: beta = %g must be >= 0", who, pr->beta);
    return MEL_OK;
}
