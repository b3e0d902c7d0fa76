// TD target and TD loss of one update, each in ONE launch (included by grad.hip).  What they replace in a captured update are
// ~20 one-line torch launches: arange / index / sub / pow / mean / the weight mul and their autograd backward nodes on the loss
// side ([3P] DQNPolicy.learn; policies/dgn.py:43-64, policies/n_dgn.py:36-66 for the sibling sums), argmax / gather / mul / add on
// the target side ([3P] DQNPolicy._target_q + compute_nstep_return).
//
//   mel_td_target   a thread per sample: best = q_target[i, argmax_a q_online[i, a]] (double DQN, the first maximum wins) or
//                   max_a q_target[i, a] (a NaN propagates, as in torch.max / torch.argmax); returns = ret + boot_w * best with the product and the sum rounded separately - the bits
//                   of the torch expression.
//   mel_td_loss     a wavefront per sample row, lanes across the row's N (siblings) and then its N * A elements:
//                     batch_q = sum_j member_j q[j, act_j]      per-lane partial (<= 2 siblings per lane), xor butterfly
//                     td = returns - batch_q,  term = weight td^2  (or Huber, delta = 1),  g = d loss / d batch_q
//                     dq[j, a] = member_j g at a = act_j, 0 elsewhere: EVERY element of the row is written, no memset launch
//                   A workgroup (16 waves) owns MEL_TD_GROUP_ROWS consecutive rows: their terms meet in LDS and wave 0 sums them
//                   with the same butterfly.  One workgroup: that sum / B is the loss.  More: the sums go to scratch[workgroup]
//                   and td_loss_finish_kernel adds them - every lane a run of consecutive workgroups, then the lanes in order.
// No float atomics, every sum in a fixed order and every product rounded on its own (__fmul_rn / __fadd_rn: the compiler contracts
// nothing into an fma): two calls on the same inputs give the same bits, whatever the optimiser does.  Nothing the host passes changes
// between two calls of an update, so both launches replay from a HIP graph.
#pragma once

namespace mel {

__global__ __launch_bounds__(256) void td_target_kernel(const float* __restrict__ q_target, const float* __restrict__ q_online,
                                                        const float* __restrict__ ret, const float* __restrict__ boot_w, int B, int A,
                                                        float* __restrict__ returns) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float* qt = q_target + (size_t)i * A;
    float best;
    if (q_online) {
        const float* qo = q_online + (size_t)i * A;
        int at = 0;
        float top = qo[0];
        for (int a = 1; a < A; ++a)
            if (qo[a] > top || (qo[a] != qo[a] && top == top)) top = qo[a], at = a;      // strict: the lowest index wins a tie;
        // a NaN counts as the maximum (the first one), as in torch.argmax
        best = qt[at];
    } else {
        best = qt[0];
        for (int a = 1; a < A; ++a)
            if (qt[a] > best || qt[a] != qt[a]) best = qt[a];      // not fmaxf: a NaN stays, as in torch.max (then no value replaces it)
    }
    returns[i] = __fadd_rn(ret[i], __fmul_rn(boot_w[i], best));      // two roundings, never an fma
}

__device__ __forceinline__ float td_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

struct TdLossArgs {
    const float* q;              // [B, N, A]
    const long long* act;        // [B, N]
    const float* member;         // [B, N] or null (every sibling counts)
    const float* returns;        // [B]
    const float* weight;         // [B] or null
    int B, N, A, huber;
    float* loss;                 // [1]
    float* td;                   // [B]
    float* dq;                   // [B, N, A]
    float* partial;              // [workgroups] when there are several
};

static_assert(MEL_TD_GROUP_ROWS == 64, "wave 0 of td_loss_kernel sums one term per lane");

__global__ __launch_bounds__(1024) void td_loss_kernel(TdLossArgs a) {
    __shared__ float term[MEL_TD_GROUP_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;              // 16 waves
    for (int r = wave; r < MEL_TD_GROUP_ROWS; r += 16) {
        const int i = blockIdx.x * MEL_TD_GROUP_ROWS + r;                    // (wave-uniform)
        if (i >= a.B) {
            if (lane == 0) term[r] = 0.f;
            continue;
        }
        const float* q = a.q + (size_t)i * a.N * a.A;
        const long long* act = a.act + (size_t)i * a.N;
        const float* member = a.member ? a.member + (size_t)i * a.N : nullptr;
        float s = 0.f;
        for (int j = lane; j < a.N; j += 64) {                               // N <= 128: at most two siblings per lane
            const long long c = act[j];
            const float m = member ? member[j] : 1.f;
            if (m != 0.f && c >= 0 && c < a.A) s = __fadd_rn(s, __fmul_rn(m, q[(size_t)j * a.A + c]));      // never an fma
        }
        const float batch_q = td_wave_sum(s);
        const float td = a.returns[i] - batch_q;
        float t, g;                                                          // the row's loss term, d (sum of terms) / d batch_q
        if (a.huber) {                                                       // huber_loss(batch_q, returns), delta = 1
            const float z = fabsf(td);
            t = z < 1.f ? __fmul_rn(__fmul_rn(0.5f, td), td) : z - 0.5f;
            g = z < 1.f ? -td : (td > 0.f ? -1.f : 1.f);
        } else {
            const float w = a.weight ? a.weight[i] : 1.f;
            t = __fmul_rn(w, __fmul_rn(td, td));
            g = __fmul_rn(__fmul_rn(-2.f, w), td);
        }
        g = g / (float)a.B;                                                  // (the mean's 1 / B)
        if (lane == 0) term[r] = t, a.td[i] = td;
        float* dq = a.dq + (size_t)i * a.N * a.A;
        for (int e = lane; e < a.N * a.A; e += 64) {
            const int j = e / a.A, c = e - j * a.A;
            const float m = member ? member[j] : 1.f;
            dq[e] = (m != 0.f && act[j] == c) ? __fmul_rn(m, g) : 0.f;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const float sum = td_wave_sum(term[lane]);                           // MEL_TD_GROUP_ROWS == 64: a term per lane
        if (lane == 0) {
            if (gridDim.x == 1) *a.loss = sum / (float)a.B;
            else a.partial[blockIdx.x] = sum;
        }
    }
}

// loss = (sum of the workgroups' partial sums) / B: lane l adds its run of consecutive partials, lane 0 adds the lanes in order
__global__ __launch_bounds__(64) void td_loss_finish_kernel(const float* __restrict__ partial, int groups, int B, float* __restrict__ loss) {
    const int lane = threadIdx.x, per = (groups + 63) / 64;
    float s = 0.f;
    for (int k = lane * per; k < (lane + 1) * per && k < groups; ++k) s += partial[k];
    float total = 0.f;
    for (int l = 0; l < 64; ++l) total += __shfl(s, l, 64);
    if (lane == 0) *loss = total / (float)B;
}

}  // namespace mel

extern "C" {

mel_status mel_td_target(const float* q_target, const float* q_online, const float* ret, const float* boot_w, int64_t batch,
                         int32_t n_actions, float* returns, void* stream) {
    if (!q_target || !ret || !boot_w || !returns) return mel::fail(MEL_ERR_INVALID_ARG, "mel_td_target: null pointer");
    if (batch < 1 || batch > MEL_TD_MAX_BATCH || n_actions < 1 || n_actions > MEL_TD_MAX_ACTIONS)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_td_target: batch=%ld outside [1, %d] or n_actions=%d outside [1, %d]", (long)batch,
                         MEL_TD_MAX_BATCH, n_actions, MEL_TD_MAX_ACTIONS);
    mel::clear_stale_error();
    MEL_LAUNCH(mel::td_target_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), q_target,
               q_online, ret, boot_w, (int)batch, n_actions, returns);
    return mel::check_launch("mel_td_target");
}

mel_status mel_td_loss(const float* q, const int64_t* act, const float* member, const float* returns, const float* weight,
                       int64_t batch, int32_t n_nodes, int32_t n_actions, int32_t huber, float* loss, float* td, float* dq,
                       void* scratch, size_t scratch_bytes, void* stream) {
    if (!q || !act || !returns || !loss || !td || !dq) return mel::fail(MEL_ERR_INVALID_ARG, "mel_td_loss: null pointer");
    if (batch < 1 || batch > MEL_TD_MAX_BATCH || n_actions < 1 || n_actions > MEL_TD_MAX_ACTIONS || n_nodes < 1 || n_nodes > MEL_MAX_NODES)
        return mel::fail(MEL_ERR_INVALID_ARG, "mel_td_loss: batch=%ld outside [1, %d], n_nodes=%d outside [1, %d] or n_actions=%d outside [1, %d]",
                         (long)batch, MEL_TD_MAX_BATCH, n_nodes, MEL_MAX_NODES, n_actions, MEL_TD_MAX_ACTIONS);
    const int groups = (int)((batch + MEL_TD_GROUP_ROWS - 1) / MEL_TD_GROUP_ROWS);
    if (groups > 1 && (!scratch || scratch_bytes < (size_t)groups * sizeof(float)))
        return mel::fail(MEL_ERR_WORKSPACE, "mel_td_loss: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : (size_t)0,
                         (size_t)groups * sizeof(float));
    mel::clear_stale_error();
    mel::TdLossArgs a{};
    a.q = q, a.act = reinterpret_cast<const long long*>(act), a.member = member, a.returns = returns, a.weight = weight;
    a.B = (int)batch, a.N = n_nodes, a.A = n_actions, a.huber = huber != 0;
    a.loss = loss, a.td = td, a.dq = dq, a.partial = static_cast<float*>(scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MEL_LAUNCH(mel::td_loss_kernel, dim3(groups), dim3(1024), 0, s, a);
    if (mel_status st = mel::check_launch("mel_td_loss")) return st;
    if (groups > 1) {
        MEL_LAUNCH(mel::td_loss_finish_kernel, dim3(1), dim3(64), 0, s, a.partial, groups, a.B, loss);
        return mel::check_launch("mel_td_loss (sum of the workgroups)");
    }
    return MEL_OK;
}

}  // extern "C"
