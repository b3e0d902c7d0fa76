/*
 * melissa_hip.h - C ABI of libmelissa_hip.so: the MI355X (gfx950) hot path of Melissa.
 *
 * The drop-in boundary.  Every pointer marked "device" is a DEVICE pointer
 * borrowed from the caller (e.g. torch.Tensor.data_ptr() of a ROCm tensor); the library never
 * allocates, frees or retains caller memory, keeps no global mutable state except a thread-local
 * error string, launches everything on the caller's HIP stream and never synchronises.  `stream`
 * is a hipStream_t passed as void* so this header needs no HIP include.
 *
 * Every entry point returns mel_status (0 = ok, negative = error, see mel_last_error()).
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   mel_ldgn_forward   -> LDGNNetwork.forward        graph_env/env/utils/networks/l_dgn.py:92-151
 *   mel_hldgn_forward  -> HLDGNNetwork.forward       graph_env/env/utils/networks/hl_dgn.py:82-119
 *   mel_dgnr_forward   -> DGNRNetwork.forward        graph_env/env/utils/networks/dgn_r.py:82-129
 *                         (both include build_pyg_batch_time, networks/common.py:6-64, and the
 *                          [3P] radius_graph / GATv2Conv / global_*_pool / tianshou MLP they call)
 *   mel_select_action  -> [3P] tianshou DQNPolicy.forward mask + argmax and exploration_noise,
 *                         called at policies/multi_agent_managers/shared_policy.py:81-91,154
 *   mel_env_reset      -> GraphEnv.reset + World.reset      graph.py:222-248, core.py:343-437
 *   mel_env_step       -> GraphEnv.step (+ World.step ...)  graph.py:303-389,402-463, core.py:225-341,
 *                         selector.py:25-48
 *   mel_env_observe    -> GraphEnv.observe / last() + [3P] PettingZooEnv.step packing
 *                         graph.py:181-216, SURVEY.md Appendix A.6
 */
#ifndef MELISSA_HIP_H
#define MELISSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t mel_status;
#define MEL_OK                 0
#define MEL_ERR_INVALID_ARG   -1   /* null pointer, bad size, N outside [1, 128] ...             */
#define MEL_ERR_SHAPE         -2   /* obs width != N*(in_dim+3)+1 (networks/common.py:24-29)      */
#define MEL_ERR_UNSUPPORTED   -3   /* layer sizes the kernels are not built for                  */
#define MEL_ERR_WORKSPACE     -4   /* ws_bytes < mel_workspace_bytes(...)                        */
#define MEL_ERR_LAUNCH        -5   /* hipGetLastError() != hipSuccess after a launch             */

/* Node sets.  A set of nodes of an N-node graph is MEL_SET_WORDS(N) consecutive uint64 words, word k holding nodes
 * 64 k .. 64 k + 63 (bit i of word k = node 64 k + i).  For N <= 64 (the sizes BASELINE quotes, 20 and 50) that is ONE
 * 64-bit mask and every layout below is exactly "one uint64 per set"; for 64 < N <= 128 (the reference CLI's third size,
 * --n-agents 100, common.py:49) every array documented as uint64 [..] of node sets gains a trailing [2]: one_hop is
 * [B, N, 2], node_sets [B, 8, 2], live [B, 2], adjacency taps [bs, N, 2] and so on.  One wavefront still steps one env;
 * a lane then holds the two nodes lane and lane + 64. */
#define MEL_MAX_NODES        128
#define MEL_SET_WORDS(n)     (((n) + 63) / 64)
#define MEL_NODE_COLS          8   /* x, y, 5 features, dm flag (graph.py:80)                    */
#define MEL_MAX_HEAD_LAYERS    6

#define MEL_MODEL_LDGN         0
#define MEL_MODEL_HLDGN        1
#define MEL_MODEL_DGNR         2   /* dgn_r.py: the L-DGN skeleton with TransformerConv layers       */

#define MEL_CONV_GATV2         0
#define MEL_CONV_TRANSFORMER   1

#define MEL_AGG_MAX            0   /* hl_dgn.py:56-60 */
#define MEL_AGG_MEAN           1
#define MEL_AGG_ADD            2

/* One torch.nn.Linear: weight [out_dim, in_dim] row-major fp32, bias [out_dim] fp32 (device). */
typedef struct mel_linear {
    const float* weight;
    const float* bias;
    int32_t in_dim;
    int32_t out_dim;
} mel_linear;

/* One attention conv layer.
 * kind MEL_CONV_GATV2 - [3P] PyG GATv2Conv: lin_l (sources) / lin_r (targets)
 *   [heads*C, in], att [1, heads, C], bias [heads*C]; negative_slope 0.2, self-loops added, eps 1e-16.
 * kind MEL_CONV_TRANSFORMER - [3P] PyG TransformerConv(root_weight=False) (A.2): lin_l = lin_key and
 *   lin_v = lin_value (sources), lin_r = lin_query (targets); score q.k/sqrt(C), NO self-loops, no output
 *   bias (att, bias NULL); lin_skip is a parameter of the module but never used. */
typedef struct mel_gatv2 {
    mel_linear lin_l;
    mel_linear lin_r;
    const float* att;
    const float* bias;
    int32_t heads;         /* a power of two (a head is 64 / heads lanes of a wavefront), or 6 (8 lanes per head, 48 of 64 live) */
    int32_t channels;      /* C, per head: 2, 4, 8 or 16 per lane of its head (6 heads: 64 or 128); else MEL_ERR_UNSUPPORTED */
    mel_linear lin_v;
    int32_t kind;
    int32_t reserved;
} mel_gatv2;

/* [3P] tianshou MLP: Linear, ReLU, ..., Linear (no activation after the last layer). */
typedef struct mel_mlp {
    mel_linear layer[MEL_MAX_HEAD_LAYERS];
    int32_t n_layers;
} mel_mlp;

/* Borrowed views of the nn.Parameter storages of LDGNNetwork / HLDGNNetwork (state_dict keys
 * encoder.model.{0,2}.*, conv1.*, conv2.* (L-DGN only), Q.model.*, V.model.*; l_dgn.py:49-86). */
typedef struct mel_weights {
    int32_t model;         /* MEL_MODEL_*                                            */
    int32_t in_dim;        /* node features fed to the encoder (5)                   */
    int32_t n_actions;     /* Q head output (2)                                      */
    int32_t dueling;       /* 1: Q/V dueling heads; 0: q_head is the single out_linear (l_dgn.py:88) */
    mel_mlp   encoder;     /* 2 layers: in_dim -> hidden -> hidden                   */
    mel_gatv2 conv1;
    mel_gatv2 conv2;       /* unused for HL-DGN                                      */
    mel_mlp   q_head;      /* latent -> ... -> n_actions                             */
    mel_mlp   v_head;      /* latent -> ... -> 1                                     */
    int32_t precision;     /* MEL_PREC_F32 (reference arithmetic, logits <= 1e-4), MEL_PREC_BF16, MEL_PREC_F32_SPLIT or MEL_PREC_F32_AUTO */
    int32_t flags;         /* MEL_FWD_PLAN_READY: the plan masks of this call were written by mel_env_round (plan_* sink);
                            * MEL_FWD_INTEGER_FEATURES: see below.  The value 4 is reserved (it once chose a former attention walk) */
    const void* prepared;  /* optional (MEL_PREC_BF16 / MEL_PREC_F32_SPLIT): device buffer filled by mel_prepare_weights for THESE
                            * weights - the forward then reads the converted projection weights from it and launches no
                            * conversion.  NULL: every call converts the fp32 parameters into its workspace (stateless). */
    const void* tables;    /* optional: device buffer filled by mel_prepare_feature_tables for THESE weights and tables_nodes
                            * nodes per graph - a forward that takes the node-feature table (MEL_FWD_INTEGER_FEATURES) then reads
                            * the encoder / conv1-projection rows of every feature tuple from it instead of evaluating them
                            * (they depend on the weights only).  NULL (the default everywhere, bench.py's headline included):
                            * the table rows are evaluated by every call. */
    int32_t tables_nodes;
    int32_t reserved;
} mel_weights;
#define MEL_FWD_PLAN_READY 1
/* MEL_FWD_INTEGER_FEATURES: the caller guarantees that the five node features of every observation row are the integers
 * GraphEnv writes for policy agents (graph.py:261-269: degree in [0, N), messages transmitted in [0, 4], last action /
 * interested / has message in {0, 1}) - true for everything mel_env_* produces when no agent is scripted.  The encoder and the conv1 projections are then functions of
 * one of N * 40 feature TUPLES: when the receptive-field row lists are at least twice that long, the forward evaluates them
 * once per tuple (table rows, on every call - nothing is kept between calls) and the conv1 attention gathers rows by tuple
 * id.  Same arithmetic per row, bit-identical logits.  A feature outside the ranges is clamped into the table and flagged
 * (mel_forward_tap kind 3).  Without the flag the general row-list path runs (arbitrary float features). */
#define MEL_FWD_INTEGER_FEATURES 2

/* Feature precision of the L-DGN / DGN-R forward (BASELINE config "bf16 feature path").  MEL_PREC_BF16: the
 * node-feature rows between layers (encoder output, lin_l / lin_r projections, conv outputs, head input and
 * hidden layers) and the weight matrices of the dense projections are bf16 (the fp32 nn.Parameters are
 * converted into the workspace by every call), contractions run on the bf16 MFMA with fp32 accumulation;
 * attention scores / softmax / aggregation, biases, the encoder's first layer, the last head layer and the
 * logits stay fp32.  Not the reference's arithmetic: expect ~1e-2 absolute on logits (tests state the bound).
 * The same holds for HL-DGN (pooled head input in bf16).  Exactly where a value is rounded to bf16 (round to nearest even):
 *   - the projection weights: encoder layer 1, lin_l / lin_r / lin_v of the convs, every hidden head layer but see below;
 *   - the first encoder layer's OUTPUT relu(W0 x + b0) (fp32 weights, fp32 fma chain over the features in order), as it
 *     becomes the bf16 operand of layer 1; then the encoder output, each conv projection (+ bias), relu(conv + bias) of
 *     conv1 BEFORE the decision-maker mask (x_2) and, separately, that fp32 value times the flag (the conv1 rows conv2
 *     reads), relu(conv2 + bias) (x_3), HL-DGN's pooled row (the mask and the max / mean / add run in fp32 on unrounded rows);
 *   - the output of a hidden head layer, EXCEPT the last hidden layer, which is stored fp32 for the fp32 tail.
 *   The standard heads (two hidden layers of 128 for Q and for V) round less: their first layer's bf16 products are kept in
 *   fp32, and bias + ReLU, the second hidden layer (on the fp32 parameters) and the tail run in fp32 in one launch.
 *   A head without a hidden layer (out_linear) is refused: MEL_ERR_UNSUPPORTED. */
#define MEL_PREC_F32  0
#define MEL_PREC_BF16 1
/* MEL_PREC_F32_SPLIT: fp32 features and fp32-accurate results, with the dense projections evaluated on the bf16 matrix
 * cores by operand splitting (x = hi + mid + lo in bf16, exactly; six of the nine partial products, each exact in
 * fp32, accumulated in fp32).  As close to the exact dot product as a native fp32 GEMM (csrc/gemm_split.hpp); the
 * reference's parity bar (logits <= 1e-4) holds with the same margin as MEL_PREC_F32. */
#define MEL_PREC_F32_SPLIT 2
/* MEL_PREC_F32_AUTO: fp32 features and fp32-accurate results like the two above, with the arithmetic chosen PER LAUNCH: the
 * large projections of a forward (conv2's lin_l + lin_r and the heads' first layer once their row lists fill the chip with
 * 128 x 128 tiles: from a few thousand rows on) take the split kernels of MEL_PREC_F32_SPLIT, everything else - small batches
 * entirely - the exact-fp32 matrix instruction of MEL_PREC_F32.  The choice depends on the expected row counts only, never on
 * the data.  Weights: the fp32 parameters plus their bf16 planes (prepared or converted per call exactly as for
 * MEL_PREC_F32_SPLIT, same buffer size).  L-DGN 50-node, 1024 envs: 0.211 -> 0.18 ms per round step. */
#define MEL_PREC_F32_AUTO 3

/* Convert the projection weights once per weight VERSION instead of once per call (bf16 feature path: bf16 copies; split
 * path: three bf16 planes per weight).  The caller owns the buffer (mel_prepared_weights_bytes; 0 for MEL_PREC_F32), calls
 * mel_prepare_weights after every change of the parameters (optimizer step, load_state_dict) and points
 * mel_weights.prepared at it; the library keeps no state. */
size_t mel_prepared_weights_bytes(const mel_weights* w);
mel_status mel_prepare_weights(const mel_weights* w, void* prepared, size_t bytes, void* stream);

/* The node-feature table of MEL_FWD_INTEGER_FEATURES (encoder row and conv1 projections of each of the n_nodes * 40 feature
 * tuples) evaluated ONCE per weight version into a caller-owned buffer, like the prepared weights above: same kernels, same
 * rows, same bits as the per-call evaluation.  Opt-in (mel_weights.tables); precision follows mel_weights.precision and,
 * for bf16 / split, needs mel_weights.prepared. */
size_t mel_feature_tables_bytes(const mel_weights* w, int32_t n_nodes);
mel_status mel_prepare_feature_tables(const mel_weights* w, int32_t n_nodes, void* tables, size_t bytes, void* stream);
/* The same table, same buffer layout and same bits, by the ONE launch in which a forward evaluates it beside its row lists
 * (a workgroup makes the encoder rows of 32 tuples, keeps them in LDS and runs 256 conv1 columns on them): the table work
 * items alone, no lists.  MEL_ERR_UNSUPPORTED where the forward keeps the two-launch form: anything but GATv2 L-DGN at
 * MEL_PREC_F32 / MEL_PREC_F32_AUTO with hidden = 128.  (MEL_NO_FUSED_TABLE in the environment, read once per process, makes
 * the FORWARD take the two-launch form for A/B runs; this entry point does not look at it.) */
mel_status mel_feature_tables_fused(const mel_weights* w, int32_t n_nodes, void* tables, size_t bytes, void* stream);

/* Bytes of scratch the forward needs for `bs` observation rows of `n_nodes`-node graphs. */
size_t mel_workspace_bytes(const mel_weights* w, int64_t bs, int32_t n_nodes);

/* obs: device fp32 [bs, obs_width] row-major, obs_width must equal n_nodes*(in_dim+3)+1;
 * logits: device fp32 [bs, n_actions].  L-DGN evaluates exactly the receptive field of the
 * controlling agent (rows of conv1/conv2 that can reach logits), which yields the same logits as the
 * full-graph evaluation of l_dgn.py:117-135. */
mel_status mel_ldgn_forward(const mel_weights* w, const float* obs, int64_t bs, int32_t n_nodes,
                            int32_t obs_width, float* logits, void* workspace, size_t ws_bytes,
                            void* stream);

/* L-DGN for a SET of controlling agents per env (the round-batched loop): within one env round every
 * active agent observes the same obs_matrix (graph.py:186-188 - rows differ only in the index column), so
 * all of a round's agents are evaluated together and the encoder / conv1 work on the union of their
 * receptive fields is shared.  obs: device fp32 [bs, obs_stride], row b = obs_matrix of env b (the index
 * column is not read; obs_stride >= n_nodes*(in_dim+3)); agent_mask: device uint64 [bs], bit i = agent i
 * is evaluated.  logits: device fp32 [rows_cap, n_actions], rows ordered by env then agent id; only the
 * first sum(popcount(agent_mask)) rows are written (rows_cap >= that sum, <= bs*n_nodes).
 * row_offsets (optional, device int32 [bs+1]): first logits row of each env, total at [bs].
 * select (optional): also write each row's action (see mel_select).
 * Each row equals mel_ldgn_forward on (obs_matrix, agent) within fp32 rounding. */
/* Optional fused action selection for mel_ldgn_forward_agents: argmax of each logits row (+ eps-greedy with
 * the same counter-based stream as mel_select_action_rows) written by the kernel that produces the logits.
 * The exploration rate is `eps`, a host value fixed when the launch is issued (and frozen into a captured HIP graph), unless
 * `eps_dev` is set: then every selection reads the rate from that device float when it RUNS (e.g. the value
 * mel_exploration_schedule wrote just before on the same stream) and `eps` is ignored - a replayed graph follows a schedule
 * without being recaptured.  The stream of draws is the same either way: eps_dev -> x selects what eps = x selects. */
typedef struct mel_select {
    int32_t*        act;       /* device int32 [rows_cap]                                          */
    float           eps;       /* exploration rate when eps_dev is NULL                            */
    uint32_t        seed;
    const uint32_t* step_dev;  /* optional device counter added to the stream position             */
    /* per-env logits (HL-DGN, mel_hldgn_forward_envs_select): every agent i in live[b] takes its action from row b,
     * act is the dense [bs, n_nodes] layout of mel_select_action_envs and the stream is keyed on
     * b * 64 * MEL_SET_WORDS(n_nodes) + i                                                                           */
    const uint64_t* live;      /* node sets [bs]; NULL: one action per logits row                   */
    int32_t         n_nodes;
    int32_t         reserved;
    const float*    eps_dev;   /* optional device float [1]: the exploration rate, read at run time */
} mel_select;

size_t mel_workspace_bytes_agents(const mel_weights* w, int64_t bs, int32_t n_nodes, int64_t rows_cap);
/* Where, inside `workspace`, a forward of these dimensions keeps its plan masks (rows_cap = 0: the single-agent / HL-DGN
 * layout of mel_workspace_bytes): out5 = {adj, live, u1, u2, cnt} (u1 / u2 / cnt NULL for HL-DGN) - the values for
 * mel_env_batch.plan_*. */
mel_status mel_plan_pointers(const mel_weights* w, int64_t bs, int32_t n_nodes, int64_t rows_cap, void* workspace,
                             void** out5);
mel_status mel_ldgn_forward_agents(const mel_weights* w, const float* obs, int64_t bs, int32_t n_nodes,
                                   int32_t obs_stride, const uint64_t* agent_mask, int64_t rows_cap,
                                   float* logits, int32_t* row_offsets, const mel_select* select,
                                   void* workspace, size_t ws_bytes, void* stream);

/* DGNRNetwork.forward (graph_env/env/utils/networks/dgn_r.py:82-129): same contracts as the two L-DGN
 * entry points above, for weights with model == MEL_MODEL_DGNR (TransformerConv layers). */
mel_status mel_dgnr_forward(const mel_weights* w, const float* obs, int64_t bs, int32_t n_nodes,
                            int32_t obs_width, float* logits, void* workspace, size_t ws_bytes,
                            void* stream);
mel_status mel_dgnr_forward_agents(const mel_weights* w, const float* obs, int64_t bs, int32_t n_nodes,
                                   int32_t obs_stride, const uint64_t* agent_mask, int64_t rows_cap,
                                   float* logits, int32_t* row_offsets, const mel_select* select,
                                   void* workspace, size_t ws_bytes, void* stream);

mel_status mel_hldgn_forward(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs,
                             int32_t n_nodes, int32_t obs_width, float* logits, void* workspace,
                             size_t ws_bytes, void* stream);

/* Tile codes of mel_gemm_f32, mel_gemm_f32_split and mel_gemm_bf16 (the `tile` argument), per entry point:
 *   MEL_TILE_AUTO            all three: the library's choice
 *   MEL_TILE_64              f32, f32_split: 64 x 64 workgroup tiles
 *   MEL_TILE_128             all three: 128 x 128 tiles (N % 128 == 0; f32 and bf16 choose automatically otherwise)
 *   MEL_TILE_WIDE            f32_split: 128 x 256 tiles with both operands as bf16 plane blocks (gemm_planes_kernel);
 *                            bf16: 128 x 256 tiles (gemm_bf16_wide_kernel)
 *   MEL_TILE_64_PERSISTENT   f32: the persistent 64 x 64 kernel of the round step's ragged launches (N % 128 == 0)
 *   MEL_TILE_64_RING         f32: the specialised-wavefront (loader / MFMA waves) 64 x 64 kernel of the heads' long-K layer
 *   + MEL_TILE_PLANES_READY  f32_split: W's bf16 planes are still in scratch from an earlier call */
#define MEL_TILE_AUTO 0
#define MEL_TILE_64 1
#define MEL_TILE_128 2
#define MEL_TILE_WIDE 3
#define MEL_TILE_64_PERSISTENT 11
#define MEL_TILE_64_RING 31
#define MEL_TILE_PLANES_READY 100

/* The dense projection used by every layer above, exposed for tests and tuning:
 *   Y[m, n] = act(sum_k A[m, k] * W[n, k] + bias[n]),  A [M, lda], W [N, K] (nn.Linear layout), Y [M, ldy],
 * all device fp32; K % 32 == 0, N % 64 == 0.  tile: MEL_TILE_AUTO, MEL_TILE_64, MEL_TILE_128, MEL_TILE_64_PERSISTENT or
 * MEL_TILE_64_RING (ldy % 4 == 0, K >= 64).
 * lda % 4 == 0 and A 16-byte aligned, for every tile code: the kernels fetch A in 16-byte pieces from A + m * lda + 4 c (the ring
 * kernel by LDS-DMA); any other lda is MEL_ERR_UNSUPPORTED.  A's columns [K, lda) and rows >= M are never read (a tile's rows
 * beyond M are clamped to row M - 1), Y's columns [N, ldy) and rows >= M never written. */
mel_status mel_gemm_f32(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                        int64_t M, int32_t N, int32_t K, int32_t relu, int32_t tile, void* stream);

/* The learn path's backward products without transposed copies of their operands: Y[m, n] = sum_k A'[m, k] W'[n, k] with
 * W' = W^T read in place (W'[n, k] = W[k * ldw + n]) and, a_t != 0, A' = A^T likewise (A'[m, k] = A[k * lda + m]).
 * dX [rows, in] = dY [rows, out] . W [out, in]:  mel_gemm_f32_t(dY, out, 0, W, in, 1, dX, in, rows, in, out);
 * dW [out, in]  = dY^T . X [rows, in]:           mel_gemm_f32_t(dY, out, 1, X, in, 1, dW, in, out, in, rows).
 * N % 64 == 0, K % 32 == 0, lda % 4 == ldw % 4 == 0, M % 4 == 0 with a_t; w_t must be 1 (the plain form is mel_gemm_f32).  Same
 * tile, K order and MFMA sequence as mel_gemm_f32's 64 x 64 kernel on transposed copies: bit-identical sums. */
mel_status mel_gemm_f32_t(const float* A, int32_t lda, int32_t a_t, const float* W, int32_t ldw, int32_t w_t, float* Y, int32_t ldy,
                          int64_t M, int32_t N, int32_t K, void* stream);

/* The same product with the contraction cut into `ksplit` equal chunks that run as independent work items and are summed in
 * chunk order afterwards: for the learn path's weight gradients dW = dY^T X, a few dozen output tiles over a contraction as
 * long as the batch has rows (one tile per workgroup would leave most of the chip idle).  K / 32 must be a multiple of
 * ksplit with at least two 32-steps per chunk; parts: device scratch of ksplit * M * N floats.  lda % 4 == 0 (16-byte LDS-DMA of
 * A) and ldy % 4 == 0 (16-byte row stores), else MEL_ERR_UNSUPPORTED. */
mel_status mel_gemm_f32_splitk(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                               int64_t M, int32_t N, int32_t K, int32_t relu, int32_t ksplit, float* parts,
                               int64_t parts_floats, void* stream);

/* The same product at MEL_PREC_F32_SPLIT (fp32 operands and results, six exact bf16 partial products per term on the bf16
 * matrix cores): W is split into bf16 planes in `scratch` first.  tile: MEL_TILE_AUTO, MEL_TILE_64, MEL_TILE_128
 * (N % 128 == 0), MEL_TILE_WIDE = 128 x 256 with BOTH operands converted to bf16 planes in scratch first (the kernel conv2's
 * projections run on in large forwards, where the conv1 attention stores its rows in that form; N % 256 == 0, N <= 1536, lda == K,
 * ldy % 4 == 0, no split-K; bit-identical to MEL_TILE_128), + MEL_TILE_PLANES_READY = W's planes are already in scratch (an earlier
 * call with the same W: benchmarks; not with MEL_TILE_WIDE); ksplit > 1: the 128 x 128 kernel's split-K (K / 16 a multiple of
 * ksplit, >= 4 steps per chunk, ldy % 4 == 0).
 * K % 32 == 0, K >= 128, N % 64 == 0, lda % 4 == 0 (every tile's kernel fetches A in 16-byte pieces; MEL_ERR_UNSUPPORTED
 * otherwise); scratch: device, >= round_up(6 N K, 256) + (ksplit > 1 ? 4 ksplit M N : 0)
 * + (tile 3 ? 6 K M : 0) bytes. */
mel_status mel_gemm_f32_split(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                              int64_t M, int32_t N, int32_t K, int32_t relu, int32_t tile, int32_t ksplit, void* scratch,
                              int64_t scratch_bytes, void* stream);

/* The same projection on the bf16 feature path: A [M, lda] and W [N, K] device bf16, bias fp32, fp32
 * accumulation, Y [M, ldy] bf16 (y_f32 = 0) or fp32 (y_f32 = 1); K % 64 == 0, N % 64 == 0, lda % 8 == 0.  tile: MEL_TILE_AUTO,
 * MEL_TILE_128, MEL_TILE_WIDE = the 128 x 256 kernel of the large launches (specialised loader / MFMA wavefronts; N % 256 == 0,
 * N <= 1536).
 * mel_convert_bf16: count (multiple of 8) fp32 values -> bf16, round to nearest even. */
mel_status mel_gemm_bf16(const void* A, int32_t lda, const void* W, const float* bias, void* Y, int32_t ldy,
                         int64_t M, int32_t N, int32_t K, int32_t relu, int32_t y_f32, int32_t tile, void* stream);
mel_status mel_convert_bf16(const float* src, void* dst, int64_t count, void* stream);

/* dst[c, r] = src[r, c] (device fp32; src [rows, ld_src >= cols], dst [cols, ld_dst >= rows]; columns r >= rows of dst are
 * left untouched, so a zero-filled dst with ld_dst = rows rounded up to 32 is a zero-padded transpose).  The learn path's
 * dense backward (policies/dgn.py:49-67, [3P] DQNPolicy.learn) runs on mel_gemm_f32, which wants both operands contiguous
 * along the contraction index:  dX = dY W = gemm(dY, W^T),  dW = dY^T X = gemm(dY^T, X^T). */
mel_status mel_transpose_f32(const float* src, int32_t ld_src, int64_t rows, int32_t cols, float* dst, int32_t ld_dst,
                             void* stream);

/* ---- learn path: attention and pool with hand-written backward ---------------------------
 * Wrapped by torch.autograd.Function in melissa_amd/networks/autograd_ops.py; all buffers device fp32, row-major,
 * rows = bs * n_nodes (row b*n + i = node i of graph b), HC = heads * channels: a head is the largest power of two of
 * lanes with heads * lanes <= 64, of 2, 4, 8 or 16 channels each - heads a power of two (HC = 128 .. 1024), or 6 heads of 64
 * or 128 channels (HC = 384 / 768; 48 live lanes, the other 16 touch no memory).  Rows are HC floats apart, no padding.
 *
 * mel_radius_graph: adj[b*n + i] = sources of target i ([3P] radius_graph on the fp32 obs positions,
 *   networks/common.py:47-48: strict <, first 33 hits, self excluded) - the mask the forward kernels build.
 * mel_gat_forward: out = relu(conv(x) + bias) given the projections (kind MEL_CONV_GATV2: xl = lin_l(x) sources,
 *   xr = lin_r(x) targets, att [HC], self-loops added, l_dgn.py:125-126; MEL_CONV_TRANSFORMER: xl = keys,
 *   xv = values, xr = queries, no self-loops, bias null, dgn_r.py:103-104).
 * mel_gat_backward: grad_out -> dxl (dxv) dxr datt dbias, all WRITTEN, all deterministic sums (the source rows' gradients are
 *   gathered target by target; d att / d bias are summed per workgroup and then over the workgroups in a fixed order: no
 *   atomics).  stats: device scratch, bs * n_nodes * heads * 4 + MEL_GAT_PARTIAL_GROUPS * 2 * HC floats.
 * mel_pool_forward / backward: hl_dgn.py:105-108, pooled[b] = max / mean / add over nodes of x * dm;
 *   arg [bs, HC] int32 = node of the first maximum (max only). */
#define MEL_GAT_PARTIAL_GROUPS 256
mel_status mel_radius_graph(const float* obs, int64_t bs, int32_t n_nodes, int32_t obs_stride, int32_t in_dim,
                            uint64_t* adj, void* stream);
mel_status mel_gat_forward(const float* xl, const float* xv, const float* xr, const float* att, const float* bias,
                           const uint64_t* adj, int64_t bs, int32_t n_nodes, int32_t heads, int32_t channels,
                           int32_t kind, float* out, void* stream);
mel_status mel_gat_backward(const float* xl, const float* xv, const float* xr, const float* att, const uint64_t* adj,
                            const float* out, const float* grad_out, int64_t bs, int32_t n_nodes, int32_t heads,
                            int32_t channels, int32_t kind, float* dxl, float* dxv, float* dxr, float* datt,
                            float* dbias, float* stats, void* stream);
/* mel_gat_attention_weights: the softmax coefficients mel_gat_forward aggregates with and then drops - what upstream's
 *   operators return under return_attention_weights=True.  alpha: device fp32 [bs * n_nodes, n_nodes, heads];
 *   alpha[b*n + i, j, h] = weight of source node j of graph b for target node i and head h:
 *     GATv2        j in adj(i) + {i} (self-loop added),  e_ij = att . leaky_relu(x_r[i] + x_l[j], 0.2)
 *     Transformer  j in adj(i),                          e_ij = q[i] . k[j] / sqrt(channels)
 *     alpha_ij = exp(e_ij - max_j e_ij) / (sum_j exp(e_ij - max_j e_ij) + 1e-16)
 *   over the forward's sources in the forward's order, with the forward's score arithmetic.  xl = sources (keys), xr = targets
 *   (queries), att [HC] (GATv2 only, else null); neither bias nor values: the coefficients do not depend on them.  EVERY element
 *   is written - 0.0f where j is not a source of i, so a target without a source has a row of zeros and the caller never clears
 *   alpha - and each exactly once (no atomics).  Takes every shape mel_gat_forward takes; bs * n_nodes^2 * heads > 2^31
 *   elements is MEL_ERR_INVALID_ARG.  No gradient flows through it. */
mel_status mel_gat_attention_weights(const float* xl, const float* xr, const float* att, const uint64_t* adj, int64_t bs,
                                     int32_t n_nodes, int32_t heads, int32_t channels, int32_t kind, float* alpha,
                                     void* stream);
mel_status mel_pool_forward(const float* x, const float* dm, int64_t bs, int32_t n_nodes, int32_t hc,
                            int32_t aggregator, float* pooled, int32_t* arg, void* stream);
mel_status mel_pool_backward(const float* grad_pooled, const float* dm, const int32_t* arg, int64_t bs,
                             int32_t n_nodes, int32_t hc, int32_t aggregator, float* dx, void* stream);

/* HL-DGN for the round-batched loop: logits depend only on the env (hl_dgn.py:108 pools over the graph and
 * ignores the controlling index), so one row per env serves all of a round's agents.  obs: device fp32
 * [bs, obs_stride], row b = obs_matrix of env b, obs_stride >= n_nodes*(in_dim+3), index column not read. */
/* mel_hldgn_forward_envs with the per-(env, agent) selection of mel_select_action_envs fused into the launch that
 * produces the logits (select->live / n_nodes / act as documented at mel_select). */
mel_status mel_hldgn_forward_envs_select(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs,
                                         int32_t n_nodes, int32_t obs_stride, float* logits, const mel_select* select,
                                         void* workspace, size_t ws_bytes, void* stream);
mel_status mel_hldgn_forward_envs(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs,
                                  int32_t n_nodes, int32_t obs_stride, float* logits, void* workspace,
                                  size_t ws_bytes, void* stream);

/* Debug/parity taps: copies of intermediates after a forward with the same workspace.
 * kind: 0 = adjacency masks uint64 [bs, n_nodes] (bit j of row i set <=> edge j -> i, radius rule),
 *       1 = head input [bs, latent], fp32 (bf16 when w->precision is MEL_PREC_BF16) (L-DGN: x_1|x_2|x_3,
 *           l_dgn.py:139; HL-DGN: pooled, hl_dgn.py:108),
 *       2 = int32 [3]: rows the L-DGN GEMMs processed (sum |U1|, sum |U2|, agent rows),
 *       3 = int32 [1 + bs]: [0] rows of the node-feature table the last forward used (0 = row-list path),
 *           [1 + b] = 1 if env b had a node feature outside the integer ranges of MEL_FWD_INTEGER_FEATURES.
 * rows_cap: 0 for a workspace used by mel_ldgn_forward / mel_hldgn_forward, else the rows_cap given to
 * mel_ldgn_forward_agents.  `out` is a device pointer with room for the requested tensor.
 *
 * Kinds MEL_TAP_H0 .. MEL_TAP_ENC0: the feature-row buffers between the stages, each copied WHOLE (the rows the workspace
 * layout gives it, live or not - rows past the live count hold whatever the workspace held) in the buffer's own element
 * type E: bf16 when w->precision is MEL_PREC_BF16, else fp32.  Row-major, leading dimension = the row width given below.
 * Row orders: "U2 rows" / "U1 rows" = the packed row lists of the plan (per env in node-id order, envs in order; live counts
 * by kind 2), "agent rows" = the logits' row order.  Caps: U2 rows bs * n_nodes; U1 rows bs * min(n_nodes, 34) for
 * rows_cap = 0, else bs * n_nodes; agent rows bs for rows_cap = 0, else rows_cap.  HL-DGN has no row lists: its rows are
 * all bs * n_nodes nodes, row b * n_nodes + i.
 *   MEL_TAP_H0   encoder output                      [U2 rows, hidden] E          (HL-DGN: [bs * n_nodes, hidden])
 *   MEL_TAP_XL1  conv1 source-side projections       [U2 rows, srcw] E: srcw = heads * C for GATv2 (lin_l), 2 heads * C for
 *                TransformerConv (key | value) and for HL-DGN (lin_l | lin_r of every node)
 *   MEL_TAP_XR1  conv1 target-side projection        [U1 rows, heads * C] E       (lin_r / query; not HL-DGN)
 *   MEL_TAP_H1   conv1 output times the decision-maker flag [U1 rows, heads * C] E (not HL-DGN; fp32 precisions: bf16 planes
 *                instead of rows where conv2 runs on the planes kernel)
 *   MEL_TAP_XL2  conv2 source-side projections       [U1 rows, srcw] E            (not HL-DGN)
 *   MEL_TAP_XR2  conv2 target-side projection        [agent rows, heads * C] E    (not HL-DGN)
 *   MEL_TAP_HQ0, MEL_TAP_HQ1  the heads' hidden ping-pong buffers, agent rows * hw * 4 BYTES each (hw = widest hidden Q layer
 *                + widest hidden V layer).  Hidden layer i writes buffer i & 1 from its start as [agent rows, q_i + v_i]
 *                (Q | V side by side), bf16 on the bf16 path EXCEPT the last hidden layer, which is fp32 (the tail reads
 *                fp32); fp32 otherwise.  The standard heads (hidden [128, 128] for Q and V) do not use them: see MEL_PREC_BF16.
 *   MEL_TAP_ENC0 first encoder layer's rows [U2 rows, K0] E, only where the encoder is wider than 256 and they live in a
 *                buffer of their own; else MEL_ERR_UNSUPPORTED, as is every kind whose buffer the model does not have.
 * These kinds are defined for the row-list path only: with MEL_FWD_INTEGER_FEATURES in w->flags they return
 * MEL_ERR_UNSUPPORTED (in table mode the first three buffers hold table rows; tests hold that path to the row lists' bits). */
#define MEL_TAP_H0   4
#define MEL_TAP_XL1  5
#define MEL_TAP_XR1  6
#define MEL_TAP_H1   7
#define MEL_TAP_XL2  8
#define MEL_TAP_XR2  9
#define MEL_TAP_HQ0  10
#define MEL_TAP_HQ1  11
#define MEL_TAP_ENC0 12
mel_status mel_forward_tap(const mel_weights* w, int32_t kind, int64_t bs, int32_t n_nodes, int64_t rows_cap,
                           const void* workspace, void* out, void* stream);

/* mel_forward_attention: the attention coefficients conv2 of the INFERENCE path aggregated with in the last
 * mel_ldgn_forward_agents / mel_dgnr_forward_agents call with the same (w, bs, n_nodes, rows_cap) and this workspace.  The
 * forward's conv2 attention keeps only the aggregate x_3; x_l2, x_r2, the conv2 target descriptors and the device-side row count
 * stay in the workspace until the next forward (nothing behind the conv2 attention writes them, in row-list and in table mode
 * alike), and ONE launch of its own - a wavefront per agent row - reads them again:
 *   alpha    device float  [rows_cap][MEL_ATT_MAX_SOURCES][heads]; slot k = the coefficient of the row's k-th source in ASCENDING
 *            node id, per head; slots from the row's source count on are written 0.  MEL_ATT_MAX_SOURCES = the neighbour cap of
 *            the radius rule (33) + the GATv2 self-loop.
 *   sources  device uint64 [rows_cap][MEL_SET_WORDS(n_nodes)]: the row's conv2 source set - GATv2: the closed neighbourhood of
 *            the agent; TransformerConv: the open one, so an isolated agent has an all-zero set and an all-zero alpha row.
 * Only the rows below the device-side agent-row count (row_offsets[bs] of the forward) are written, nothing else is touched.
 * Arithmetic, per head: the forward's sources, its score (GATv2: att . leaky_relu(x_l[j] + x_r[i], 0.2); TransformerConv:
 * q[i] . k[j] / sqrt(C)), alpha_k = e^(s_k - max s) * (1 / (sum_j e^(s_j - max s) + 1e-16)) with the forward's exp2-based exp and
 * its reciprocal, the sum taken in ascending source order (the forward streams the same terms through an online softmax, two
 * sources per step: the two agree within fp32 rounding, not bit for bit).
 * No host read, no allocation: it replays from a HIP graph.  MEL_ERR_UNSUPPORTED: HL-DGN weights (no conv2, no agent rows),
 * MEL_PREC_BF16 (bf16 rows), a head shape the attention kernels do not run.  MEL_ERR_INVALID_ARG: a null argument, bs / n_nodes
 * out of range, rows_cap outside [1, bs * n_nodes]. */
#define MEL_ATT_MAX_SOURCES 34
mel_status mel_forward_attention(const mel_weights* w, int64_t bs, int32_t n_nodes, int64_t rows_cap,
                                 const void* workspace, float* alpha, uint64_t* sources, void* stream);

/* [3P] DQNPolicy.forward + exploration_noise:
 *   q = logits + (1 - mask) * (min(logits) - max(logits) - 1)   (batch-wide min / max)
 *   act = argmax(q);  if rand_u[b] < eps: act = argmax(rand_q[b, :] + mask)
 * mask: device uint8 [bs, n_actions] or NULL; rand_u [bs], rand_q [bs, n_actions] device fp32 or NULL
 * (eps-greedy off).  act: device int32 [bs].  scratch: device, >= 8 bytes. */
mel_status mel_select_action(const float* logits, const uint8_t* mask, int64_t bs, int32_t n_actions,
                             float eps, const float* rand_u, const float* rand_q, int32_t* act,
                             void* scratch, void* stream);

/* Row-wise argmax + eps-greedy for the round-batched loop: the row count lives on the device
 * (rows_dev, may be NULL = rows_cap) and the exploration stream is a counter-based hash of
 * (seed, step + *step_dev, row) instead of host numpy draws (step_dev: optional device counter, e.g. the
 * one mel_env_round advances, so the stream moves on when the launches are replayed from a HIP graph).  logit_row (optional, device int32 [rows_cap]) maps an
 * action row to its logits row (HL-DGN: all agents of an env share the env's logits). */
mel_status mel_select_action_rows(const float* logits, const int32_t* logit_row, int64_t rows_cap,
                                  const int32_t* rows_dev, int32_t n_actions, float eps, uint32_t seed,
                                  uint32_t step, const uint32_t* step_dev, int32_t* act, void* stream);

/* Per-(env, agent) action selection from per-env logits (HL-DGN in the round loop): for every agent i in
 * live[b], act[b, i] = argmax(logits[b]) or, with probability eps, a uniformly random action (same
 * counter-based stream as mel_select_action_rows, keyed on (seed, step + *step_dev, b * 64 * MEL_SET_WORDS(n_nodes) + i)).
 * act: device int32 [bs, n_nodes] (dense layout accepted by mel_env_round when row_offsets is NULL). */
mel_status mel_select_action_envs(const float* logits, const uint64_t* live, int64_t bs, int32_t n_nodes,
                                  int32_t n_actions, float eps, uint32_t seed, const uint32_t* step_dev,
                                  int32_t* act, void* stream);

/* The exploration schedule of the reference's trainers (train_fn, l_dgn.py:225-234) evaluated ON THE DEVICE from the env
 * batch's own decision counters, so that a captured round follows it with no host involvement:
 *   env_step = scale * sum_b decisions[b * stride]                    (64-bit integer sum: deterministic)
 *   horizon  = exploration_fraction * total_steps                     (total_steps = --epoch * --step-per-epoch)
 *   eps      = max(eps_train * exp(env_step * ln(eps_final) / horizon), eps_final)      in double, rounded once to float
 * decisions: device int32, n_envs elements `stride` elements apart (the round loop passes &scalars[0][MEL_S_DECISIONS] with
 * stride MEL_ENV_SCALARS); scale: the world size (every rank collects as many decisions again).  Outputs (device):
 * eps_out float [1] (what mel_select.eps_dev points at), env_step_out uint64 [1] (optional), and - with trace_cap > 0 -
 * trace_env_step uint64 [trace_cap] / trace_eps float [trace_cap] at index *round_dev % trace_cap (round_dev: optional device
 * counter, e.g. the one mel_env_round advances; NULL = index 0).  One launch of one workgroup, no host reads, no allocation:
 * capturable (with a stage timer attached it is booked under MEL_STAGE_SELECT: that stage then holds one launch more per
 * round than in a run without a schedule).  MEL_ERR_INVALID_ARG: horizon <= 0, eps_final <= 0, eps_final > eps_train (or not finite), a null decisions /
 * eps_out, n_envs < 1, stride < 1, trace_cap > 0 without both trace arrays. */
mel_status mel_exploration_schedule(const int32_t* decisions, int32_t stride, int32_t n_envs, uint32_t scale,
                                    double eps_train, double eps_final, double exploration_fraction, double total_steps,
                                    const uint32_t* round_dev, float* eps_out, uint64_t* env_step_out, int32_t trace_cap,
                                    uint64_t* trace_env_step, float* trace_eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Environment half.  State of B independent envs lives in caller-owned device memory laid out as
 * struct-of-arrays (one wavefront steps one env, lane = node - two nodes per lane beyond 64 -, node sets as defined at
 * MEL_SET_WORDS);
 * mel_env_state_bytes() gives the size, mel_env_bind() carves the pointer table.
 * ------------------------------------------------------------------------------------------------ */
#define MEL_ENV_LOGGER_STATS  10   /* graph.py:167-177, in dict order                            */
/* doubles of one env's per-step logger_stats accumulator (mel_env_batch.step_stats): the sample count, then per key
 * the running mean, M2 (sum of squared deviations from the mean), min and max */
#define MEL_ENV_STEP_STATS_DOUBLES (1 + 4 * MEL_ENV_LOGGER_STATS)

/* node_sets[b][k] */
#define MEL_SET_HAS_MESSAGE    0   /* State.has_message                        core.py:18        */
#define MEL_SET_ORIGIN         1   /* State.message_origin                     core.py:16        */
#define MEL_SET_INTERESTED     2   /* Agent.is_interested                      core.py:71        */
#define MEL_SET_SCRIPTED       3   /* Agent.is_scripted                        core.py:69,404    */
#define MEL_SET_TRUNCATED      4   /* Agent.truncated                          graph.py:333      */
#define MEL_SET_ALIVE          5   /* keys of GraphEnv.terminations            graph.py:282-286  */
#define MEL_SET_TERMINATED     6   /* terminations[a] == True                  graph.py:334      */
#define MEL_SET_AGENTS         7   /* GraphEnv.agents (always id-ordered)      graph.py:336-341  */
/* sel_sets[b][k] */
#define MEL_SEL_ACTIVE         0   /* CustomSelector active                    selector.py:43-44 */
#define MEL_SEL_SELECTED       1   /* CustomSelector selected_round            selector.py:30    */
#define MEL_SEL_INFO_VALID     2   /* infos[a] holds logger_stats              graph.py:358      */
#define MEL_SEL_TAKEN_ACTION   3   /* State.has_taken_action                   core.py:272       */
/* scalars[b][k] */
#define MEL_S_ORIGIN           0   /* World.origin_agent                                         */
#define MEL_S_SELECTION        1   /* GraphEnv.agent_selection (-1 = False)                      */
#define MEL_S_SKIP             2   /* _skip_agent_selection (-2 = None, -1 = False)              */
#define MEL_S_NUM_MOVES        3   /* GraphEnv.num_moves                                         */
#define MEL_S_WORLD_MSGS       4   /* World.messages_transmitted                                 */
#define MEL_S_NEW_ROUND        5   /* GraphEnv.is_new_round (-1 = None, 0, 1)                    */
#define MEL_S_EPISODE          6   /* pool episode currently loaded                              */
#define MEL_S_MOVE_CURSOR      7   /* movement draws consumed this episode                       */
#define MEL_S_DECISIONS        8   /* live (non-dead) agent decisions since bind                 */
#define MEL_S_DONE_COUNT       9   /* done observations this episode (multi_agent_collector.py:261-263) */
#define MEL_S_EPISODES_DONE   10   /* episodes finished (auto-reset mode)                        */
#define MEL_S_ERROR           11   /* MEL_ENV_ERR_* bits                                         */
#define MEL_S_EP_CURSOR       12   /* episodes started (indexes the auto-reset episode table)    */
#define MEL_ENV_SCALARS       16

typedef struct mel_env_batch {
    int32_t n_envs;
    int32_t n_nodes;
    int32_t dynamic_graph;     /* core.py:256                                                    */
    int32_t has_local_ratio;   /* graph.py:376,380                                               */
    double  local_ratio;
    int32_t heuristic;         /* MEL_HEURISTIC_* run by the scripted agents (core.py:226-234)    */
    int32_t is_testing;        /* evaluation mode: scripted agents stay in the active set (graph.py:244,340) */
    double*   pos;             /* [B, N, 2] float64 positions (graph node attr "pos")            */
    uint64_t* one_hop;         /* [B, N]    Agent.one_hop_neighbours_ids as bit masks            */
    uint64_t* two_hop;         /* [B, N]    Agent.two_hop_neighbours_ids                         */
    uint64_t* node_sets;       /* [B, 8]    MEL_SET_*                                            */
    uint64_t* sel_sets;        /* [B, 4]    MEL_SEL_*                                            */
    int32_t*  scalars;         /* [B, 16]   MEL_S_*                                              */
    int32_t*  agent_msgs;      /* [B, N]    Agent.messages_transmitted                           */
    int32_t*  received;        /* [B, N]    sum(State.received_from)                             */
    int32_t*  two_hop_cover;   /* [B, N]    Agent.two_hop_cover                                  */
    int8_t*   agent_action;    /* [B, N]    Agent.action (-1 = None)                             */
    int8_t*   current_actions; /* [B, N]    GraphEnv.current_actions (-1 = None)                 */
    int8_t*   steps_taken;     /* [B, N]    Agent.steps_taken                                    */
    int8_t*   sel_steps;       /* [B, N]    CustomSelector steps                                 */
    double*   rewards;         /* [B, N]    GraphEnv.rewards                                     */
    double*   pz_rewards;      /* [B, N]    [3P] PettingZooEnv.rewards (sticky)   */
    double*   episode_rewards; /* [B]       GraphEnv.episode_rewards_sum                         */
    float*    obs_matrix;      /* [B, N, 8] GraphEnv.obs_matrix                                  */
    double*   info_stats;      /* [B, N, 10] infos[agent]['logger_stats']                        */
    /* Optional episode log (caller-owned; log_capacity 0 = off): whenever an env's episode ends inside
     * mel_env_step / mel_env_round with on-device reset, one row is appended - the `logger_stats` of the final
     * observation (graph.py:166-178: what the reference's collectors gather into `episode_info`,
     * multi_agent_collector.py:283) plus env id, episode id and num_moves.  Rows beyond the capacity are dropped
     * (the cursor keeps counting). */
    int32_t   log_capacity;
    int32_t   log_reserved;
    int32_t*  log_cursor;      /* [1]  episodes logged so far (device, atomically advanced)      */
    double*   log_stats;       /* [capacity, 10]                                                 */
    int32_t*  log_meta;        /* [capacity, 3] env, pool episode, num_moves                     */
    /* Optional forward-plan sink (mel_env_round only; all NULL = off): device pointers into the forward workspace the
     * NEXT mel_*_forward_agents / mel_hldgn_forward_envs call will use (mel_plan_pointers).  The round kernel then also
     * writes what that forward's first launch would compute from the obs it just wrote and the next active sets -
     * the fp32 radius-graph adjacency (networks/common.py:48) and, for L-DGN / DGN-R, the agent / one-hop / two-hop
     * node sets and their sizes - and the forward is called with MEL_FWD_PLAN_READY in mel_weights.flags. */
    uint64_t* plan_adj;        /* [B*N] */
    uint64_t* plan_live;       /* [B]   (NULL for HL-DGN: adjacency only) */
    uint64_t* plan_u1;         /* [B]   */
    uint64_t* plan_u2;         /* [B]   */
    int32_t*  plan_cnt;        /* [3*B] */
    /* Optional per-step logger_stats pool (caller-owned, zero-initialised; NULL = off; kept across mel_env_bind like the
     * log_* pointers): [B, MEL_ENV_STEP_STATS_DOUBLES].  The reference's collectors pool the `logger_stats` of EVERY env.step
     * of every env (multi_agent_collector.py:276,316-322).  With the pool on, every AEC sub-step mel_env_round replays
     * (live, dead and episode-ending steps alike, the fast-forwarded ones included) and every mel_env_step call with an
     * output block adds one sample to its env's accumulator: the ten values STORED in infos[agent_selection] after the
     * step (what env.last() returns, stale or not), nothing when that slot holds no logger_stats (MEL_SEL_INFO_VALID
     * clear, or no selection).  Resets, mel_env_observe and the `first` launch of mel_env_round add nothing.  Per env:
     * [0] sample count, then per key k [1 + 4k ..]: mean, M2, min, max, merged by the Chan / Welford rule (n = na + nb,
     * d = mb - ma, mean = ma + d * nb / n, M2 = M2a + M2b + d * d * na * nb / n) by the one wavefront that owns the env.
     * Count-gated: with a count of 0 the other 40 values mean nothing (an all-zero buffer is an empty pool); the first
     * sample sets mean = min = max = value, M2 = 0.  Read with mel_env_step_stats.  (It stands with the other caller-owned
     * pointers, in front of received_from, which stays the last field of the struct as it is the last one carved.) */
    double*   step_stats;
    /* State.received_from (core.py:22,276-278) as node sets: node i's set holds every node it has received the message
     * from this episode.  Carved by mel_env_bind behind every other field; read and written only when heuristic ==
     * MEL_HEURISTIC_MPR (rule core.py:236-243 is the only reader).  Empty at each reset, then set by the reset's own
     * World.step (core.py:437). */
    uint64_t* received_from;   /* [B, N]    */
} mel_env_batch;

/* An episode pool: what World.reset samples (core.py:372-394), pre-drawn on the host with the
 * reference's RNG calls and packed for the device (device pointers). */
typedef struct mel_episode_pool {
    int32_t n_episodes;
    int32_t n_nodes;
    int32_t max_moves;         /* movement offsets stored per episode                            */
    int32_t reserved;
    const double*   pos;       /* [E, N, 2] initial positions                                    */
    const uint64_t* one_hop;   /* [E, N]    initial adjacency (graph edges)                      */
    const uint64_t* interested;/* [E]                                                            */
    const int32_t*  origin;    /* [E]                                                            */
    const double*   moves;     /* [E, max_moves, 2, N] 0.06*U(-1,1): all x then all y (core.py:316-319) */
    const uint64_t* scripted;  /* [E] World.scripted_indices (core.py:197-221), or NULL = no scripted agents */
    /* Optional reset snapshots (mel_env_round only): HOST pointer to an env batch of >= n_episodes envs in which
     * mel_env_reset has been run once per episode (env e <- episode e, same dynamic_graph / local_ratio / heuristic /
     * is_testing settings).  GraphEnv.reset + World.reset are a pure function of the pre-drawn episode, so an env
     * whose episode ends loads that state instead of recomputing it (positions after the reset's move, one- / two-hop
     * masks, the source's first transmission); per-env counters and the sticky reward vector are carried over.
     * NULL: resets are computed in the round kernel. */
    const struct mel_env_batch* snapshot;
    /* Optional (device int32 [n_envs of the env batch]): how many episodes of env b the table holds so far.  An env that
     * starts episode number ep_cursor >= produced[b] sets MEL_ENV_ERR_EPISODE_UNDERRUN (the table would hand it an episode
     * it has already played: a static table that wraps, or a stream that was not refilled in time).  NULL: no check. */
    const int32_t* produced;
} mel_episode_pool;

/* bits of scalars[b][MEL_S_ERROR] */
#define MEL_ENV_ERR_MOVES_EXHAUSTED   1   /* an episode needed more than max_moves movement draws               */
#define MEL_ENV_ERR_NO_SELECTION      2   /* step with no agent selected (the reference would raise KeyError)   */
#define MEL_ENV_ERR_UNCOVERED_AGENT   4   /* mel_env_round: an agent acts that the action rows do not cover     */
#define MEL_ENV_ERR_EPISODE_UNDERRUN  8   /* see mel_episode_pool.produced                                      */

/* ------------------------------------------------------------------------------------------------
 * Continuous episode supply: World.reset's sampling (core.py:343-395) ON THE DEVICE.
 *
 * The reference draws, on every reset, an episode seed and a graph from the env's own generator
 * (np_random = Generator(PCG64), core.py:372,378) and - from RandomState(episode_seed), MT19937 - the movement seed,
 * the source, the interest density and the interested set (core.py:381-394); node movement then consumes
 * RandomState(movement_seed).uniform(-1, 1) (core.py:316-319).  mel_episode_refill performs exactly those draws, bit for
 * bit (numpy's PCG64 next_uint32 buffering + Lemire bounded integers; legacy MT19937 seeding, masked rejection
 * sampling, random_sample doubles and the Fisher-Yates shuffle of RandomState.choice(replace=False)), into a RING of
 * `ring` episode slots per env: episode j of env b lives in pool slot b*ring + j % ring.  The graph comes from a packed
 * device-resident dataset (mel_graph_pool: positions + adjacency masks of the G graphs that stand for
 * graph_topologies/training_N/*.pickle, core.py:165-175,450-452).  Each call also runs GraphEnv.reset + World.reset
 * for the new slots into the pool's snapshot batch (same code as mel_env_reset), so an ending episode loads its
 * successor's state.  With scripted agents (n_scripted > 0) the env's generator also draws World._sample_scripted_agents'
 * np_random.choice(N, n_scripted, replace=False) after the graph (core.py:197-215,395: Floyd's algorithm + the shuffle's
 * draws; the source leaves the set).
 *
 * The evaluation schedule (is_testing, core.py:182-187,348-370; n_test = num_test_episodes > 0): the episode seed is not
 * drawn but read from a fixed list, test_seeds[t] = the t-th RandomState(17).randint(0, 1e9) (mel_episode_test_seeds
 * fills it), and RandomState(test_seeds[t]) draws the graph (randint(0, n_graphs); nothing for one graph), the movement
 * seed, the source and the interested set, whose density is not drawn: (i + 1) / 10 with i = ((t + 1) % n_test) % 10.
 * Only the scripted set still comes from the env's generator.  Episode e of env b sits at list position
 *     t = (b * test_env_step + (e + discarded) * test_episode_step) % n_test
 * (0, 1): the reference's walk, every env plays the whole list from the top; (1, B): the list is spread over the B envs,
 * env b plays positions b, b + B, ...
 *
 * Not covered (use a host-sampled table): a fixed graph that moves (its positions carry over between episodes);
 * training mode with every node scripted is not playable.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mel_graph_pool {
    int32_t n_graphs;
    int32_t n_nodes;
    const double*   pos;       /* [G, N, 2] device float64 node positions ("pos" node attribute)              */
    const uint64_t* one_hop;   /* [G, N]    device adjacency masks (graph edges)                              */
} mel_graph_pool;

typedef struct mel_episode_stream {
    int32_t n_envs;            /* B                                                                            */
    int32_t ring;              /* K >= 3 episode slots per env                                                  */
    int32_t fixed_graph;       /* 1: GraphEnv(graph=...) - no graph draw (core.py:377), graphs->n_graphs == 1   */
    int32_t has_density;       /* 1: fixed_interest_density is used instead of ep_rng.uniform(0.1, 1.0) (:385) */
    double  fixed_interest_density;
    uint64_t* pcg;             /* [B, 4] device: PCG64 state lo, state hi, inc lo, inc hi of env b's np_random  */
    uint32_t* pcg_half;        /* [B, 2] device: has_uint32, uinteger (numpy buffers the upper half of a draw)  */
    int32_t*  produced;        /* [B]    device: episodes drawn into the ring so far (= mel_episode_pool.produced) */
    uint32_t* draw_seed;       /* [B, K] device scratch: episode_seed per slot (core.py:372)                    */
    int32_t*  draw_graph;      /* [B, K] device scratch: graph index per slot (core.py:378)                     */
    int32_t*  work;            /* [1 + 2*B*K] device scratch: work-item count, B*K pool slots, B*K movement seeds */
    int32_t*  new_count;       /* [B]    device scratch                                                         */
    int32_t   n_scripted;      /* scripted agents per episode: int(round(scripted_agents_ratio * N)) computed by the HOST
                                * (Python's rounding, core.py:200); 0 = none, nothing more is drawn                      */
    int32_t   reserved;
    uint64_t* draw_scripted;   /* [B, K, MEL_SET_WORDS(N)] device scratch: the drawn set per slot, source included
                                * (core.py:395); may be NULL when n_scripted == 0                                        */
    int32_t   n_test;          /* 0: training mode.  T > 0: the evaluation schedule over a list of T seeds (the env batch
                                * must be in testing mode, and fixed_graph 0); draw_graph then holds list positions        */
    int32_t   test_env_step;   /* list positions between the first episodes of env b and env b + 1                         */
    int32_t   test_episode_step; /* list positions between two consecutive episodes of one env                            */
    int32_t   reserved2;
    const uint32_t* test_seeds;/* [T] device: the seed list (mel_episode_test_seeds)                                      */
    int32_t*  test_discarded;  /* [B] device, zero at start: episodes discarded so far (they shift the walk)              */
    uint32_t* key_scratch;     /* [2, key_capacity, 624] device scratch: the MT19937 keys of RandomState(episode_seed) and
                                * RandomState(movement_seed) for the first key_capacity new episodes of a refill, seeded one
                                * lane per episode; NULL with key_capacity 0                                              */
    int32_t   key_capacity;    /* new episodes per refill whose keys fit; the ones beyond it seed inside their own
                                * wavefront (same results, a longer refill).  A steady refill draws about refill_every *
                                * B * (finished episodes per env and step), the first one B * (K - 1)                     */
    int32_t   reserved3;
} mel_episode_stream;

/* For every env b draw episodes produced[b], produced[b]+1, ... while the slot they go to is free - i.e. up to episode
 * ep_cursor[b] + ring - 2 (the episode the env is playing keeps its slot) - and at most max_new of them; fill their
 * pool slots (pos / one_hop / origin / interested / scripted / moves), run their reset into pool->snapshot, then
 * publish produced[b].  `discard` episodes are drawn and dropped first (the samplings the reference performs while an
 * env is CONSTRUCTED, so that streams line up with a reference run).  `pool` must have n_episodes == B*ring, device
 * arrays the library may WRITE, a snapshot batch of B*ring envs, and produced == stream->produced.  ep_cursor is read
 * from env->scalars.  Launches on `stream`; the caller orders it against the env launches (a refill may overlap env
 * rounds on another stream as long as no env can reach an episode >= the produced[] value of the previous refill).
 * With the evaluation schedule (st->n_test > 0) `discard` moves every env that many list positions on and draws the discarded
 * episodes' scripted sets; together with a non-zero test_env_step it is an argument error.  An env batch in testing mode with
 * n_test == 0 is MEL_ERR_UNSUPPORTED, and so is a fixed graph in testing mode. */
/* A pacing gate for `stream`: whatever is enqueued behind it runs once the device counter `counter` (e.g. the round_counter
 * mel_env_round advances on another stream) has reached `target` (wrap-around compare), or after timeout_us.  It lets the
 * episode refill follow the main stream's progress without an event on the main stream (events between HIP-graph replays
 * cost the step several microseconds on this stack); one wavefront polls with agent-scope relaxed loads and s_sleep. */
mel_status mel_wait_counter(const uint32_t* counter, uint32_t target, uint32_t timeout_us, void* stream);

mel_status mel_episode_refill(const mel_episode_stream* st, const mel_graph_pool* graphs, const mel_episode_pool* pool,
                              const mel_env_batch* env, int32_t max_new, int32_t discard, void* stream);

/* out[i] (device, n >= 1 words) = the i-th RandomState(17).randint(0, 1e9): the evaluation schedule's seed list
 * (core.py:184-187), drawn by one wavefront's MT19937. */
mel_status mel_episode_test_seeds(uint32_t* out, int32_t n, void* stream);

/* The training-graph dataset recipe (core.py:440-447) ON THE DEVICE: candidate s is nx.random_geometric_graph(n_nodes,
 * radius, seed=s) - positions from Python's random.Random(s) (MT19937 init_by_array with the one-word key [s]; x then y per
 * node), an edge iff dx*dx + dy*dy <= radius_sq in float64 - and is kept iff it is connected.  The call examines the seeds
 * first_seed .. first_seed + n_candidates - 1 and appends the accepted graphs IN ASCENDING SEED ORDER at slot *count of
 * pos [capacity, N, 2] / one_hop [capacity, N, MEL_SET_WORDS(N)] / seeds [capacity] while *count < capacity (later
 * acceptances are dropped), then advances *count (a device counter, at most capacity afterwards).  Bit for bit the arrays of
 * melissa_amd.env.episodes.packed_graph_pool; nothing depends on n_candidates or on scheduling, so a caller may cover a seed
 * range in chunks of any size.  radius_sq is the caller's radius ** 2 (a double).  Three launches on `stream`, no allocation,
 * no synchronisation; `workspace` (256-byte aligned, mel_graph_pool_workspace_bytes(n_nodes, n_candidates) bytes, 0 for
 * arguments out of range) stages the chunk's accepted graphs.  MEL_ERR_INVALID_ARG: n_nodes outside 2 .. MEL_MAX_NODES, a
 * null pointer, n_candidates outside [0, 2^30], or a seed range that leaves [0, 2^32). */
size_t mel_graph_pool_workspace_bytes(int32_t n_nodes, int32_t n_candidates);
mel_status mel_graph_pool_generate(int32_t n_nodes, double radius_sq, int64_t first_seed, int32_t n_candidates, int32_t capacity,
                                   double* pos, uint64_t* one_hop, int64_t* seeds, int32_t* count, void* workspace,
                                   size_t ws_bytes, void* stream);

/* Scripted agents (scripted_agents_ratio > 0): the deterministic heuristics of graph_env/env/utils/heuristics/.  The
 * probabilistic ones (probabilistic_gossip / _relay) draw from the process-global np.random: not offered. */
#define MEL_HEURISTIC_NONE                  0
#define MEL_HEURISTIC_SIMPLE_BROADCAST      1   /* action = 0 if has_taken_action else 1     heuristics/core.py:13-18 */
#define MEL_HEURISTIC_BROADCAST_IF_INTERESTED 2 /* action = number_interested_neighbors > 0  :45-53 */
#define MEL_HEURISTIC_SILENT                3   /* action = 0                                :56-62 */
/* OLSR multipoint relays (RFC 3626), heuristics/mpr.py:7-72.  mpr_heuristic returns a bare array where World.step reads
 * a HeuristicResult (core.py:227-234); it is read as HeuristicResult(relay_mask=mpr, action=None): every scripted agent
 * names its MPR set at every world step, a scripted node that some scripted neighbour chose forwards once, and only
 * after receiving the message from one of those neighbours (core.py:236-243).  Uses mel_env_batch.received_from. */
#define MEL_HEURISTIC_MPR                   4

/* The MPR set (MEL_HEURISTIC_MPR's selection) of every node of n_graphs undirected graphs of n_nodes <= MEL_MAX_NODES
 * nodes: one_hop device uint64 [G, N, MEL_SET_WORDS(N)] adjacency node sets (symmetric, no self loops - not checked
 * here), mpr_out the same shape.  The device function the env kernels run. */
mel_status mel_mpr_sets(const uint64_t* one_hop, int32_t n_graphs, int32_t n_nodes, uint64_t* mpr_out, void* stream);

/* Outputs of last() + [3P] PettingZooEnv packing, one row per listed env (device; any may be NULL). */
typedef struct mel_env_obs {
    float*    obs;             /* [n, 8N+1] obs_matrix flattened + controlling index (graph.py:186-188) */
    int64_t   obs_stride;      /* floats between rows (>= 8N+1)                                  */
    int32_t*  agent_id;        /* [n]                                                            */
    uint8_t*  action_mask;     /* [n, 2]    graph.py:190-192                                     */
    double*   rew;             /* [n, N]    sticky reward vector                                 */
    uint8_t*  terminated;      /* [n]                                                            */
    int32_t*  flags;           /* [n, 4]    env_step, environment_step, explicit_reset, has_stats */
    uint64_t* active_nb;       /* [n]       info['active_one_hop_neighbors'] (graph.py:198-203)  */
    double*   stats;           /* [n, 10]   info['logger_stats']                                 */
} mel_env_obs;

size_t mel_env_state_bytes(int32_t n_envs, int32_t n_nodes);
/* Carves `state` (device, mel_env_state_bytes() bytes, 256-byte aligned) into the pointer table. */
mel_status mel_env_bind(mel_env_batch* env, int32_t n_envs, int32_t n_nodes, void* state);

/* GraphEnv.reset for the envs listed in env_ids (device int32 [n], or NULL = envs 0..n-1): loads pool
 * episode episode_ids[k] (device int32 [n]), runs the forced source transmission (core.py:246,437)
 * and, if `out` is not NULL, observes.  keep_graph != 0 keeps the env's current positions/edges
 * (the reference's fixed-graph mode mutates one graph across episodes, core.py:130,303-314). */
mel_status mel_env_reset(mel_env_batch* env, const mel_episode_pool* pool, const int32_t* env_ids,
                         const int32_t* episode_ids, int64_t n, int32_t keep_graph,
                         const mel_env_obs* out, void* stream);

/* One AEC step per listed env (GraphEnv.step; action ignored when the selected agent is dead), the
 * sticky reward copy of PettingZooEnv.step, then - if `out` is not NULL - last().
 * actions: device int32 [n].  If episode_table is not NULL (device int32 [B, table_stride]) an env
 * whose observation says the episode is over (terminated and (explicit_reset or N agents reported
 * done), multi_agent_collector.py:261-264) is reset in the same launch to pool episode
 * episode_table[b, ep_cursor % table_stride] and observed again. */
mel_status mel_env_step(mel_env_batch* env, const mel_episode_pool* pool, const int32_t* actions,
                        const int32_t* env_ids, int64_t n, const mel_env_obs* out,
                        const int32_t* episode_table, int32_t table_stride, void* stream);

/* Device-resident replay of the round-batched loop (the counterpart of the per-(env, agent) sub-buffers the
 * reference collector routes transitions into, multi_agent_collector.py:229-271).  A round of env b is ONE
 * record: the obs_matrix its agents decided on, who acted, their actions, the rewards GraphEnv.rewards holds
 * after the round's world step (graph.py:373-389), who was terminated by it (graph.py:330-334) and the
 * obs_matrix every one of them observes next - i.e. the transition (obs, act, rew, done, obs_next) of each
 * acting agent i is (obs|i, act[i], rew[i], done bit i, obs_next|i).  Records of an env are consecutive ring
 * slots, so n-step returns follow an agent by walking slots while it keeps acting. */
typedef struct mel_round_replay {
    int32_t   capacity;        /* K ring slots per env                                            */
    int32_t   reserved;
    float*    obs;             /* [B, K, 8N]                                                      */
    float*    obs_next;        /* [B, K, 8N]                                                      */
    uint64_t* acted;           /* [B, K]                                                          */
    uint64_t* done;            /* [B, K]                                                          */
    int8_t*   act;             /* [B, K, N]                                                       */
    float*    rew;             /* [B, K, N]                                                       */
    int32_t*  episode;         /* [B, K] episode ordinal of the env when the round was played     */
    int32_t*  cursor;          /* [B]    rounds recorded so far (slot = cursor % K)               */
    uint64_t* active_nb;       /* [B, K, N] optional (NULL = off): info['active_one_hop_neighbors'] of each acting
                                * agent at ITS next observation (graph.py:198-203, collective_experience_collector.py:270-290),
                                * written with the world step; 0 for agents that did not act                          */
} mel_round_replay;

/* Replay sampling in one launch (the learn half's first step, l_dgn.py:246-261 -> [3P] tianshou ReplayBuffer.sample +
 * compute_nstep_return with estimation_step = n_step): `batch` (record, acting agent) pairs drawn uniformly with replacement
 * from the records the ring holds, each followed through consecutive slots while the env's episode is the same and the agent
 * keeps acting.  Outputs (device): obs / boot_obs float [batch, 8N+1] (the record's obs_matrix | agent id; the observation to
 * bootstrap from), act int64, ret float (sum_j discount[j] * rew_j), boot_w float (discount[steps], 0 when the agent
 * terminated inside the window), env / slot / agent int64.  discount: HOST float [n_step + 1] = gamma^j (copied into the launch).
 * Draws are a counter-based function of (seed, *draw_counter, sample index); the launch increments *draw_counter (device
 * uint64), so replaying it from a HIP graph keeps drawing new batches.  scratch: device int32 [n_envs * capacity + 1].
 * out->nb_sibling (optional) needs replay->active_nb, else MEL_ERR_INVALID_ARG. */
#define MEL_REPLAY_MAX_NSTEP 16
typedef struct mel_replay_batch {
    float*   obs;
    float*   boot_obs;
    int64_t* act;
    float*   ret;
    float*   boot_w;
    int64_t* env;
    int64_t* slot;
    int64_t* agent;
    uint64_t* nb_sibling;      /* [batch] optional (NULL = off): acted[rec] & (active_nb[rec, agent] | bit(agent)), the
                                * siblings N-DGN sums over (policies/n_dgn.py:36-47); needs replay->active_nb          */
} mel_replay_batch;
mel_status mel_replay_sample(const mel_round_replay* replay, int64_t n_envs, int32_t n_nodes, int32_t batch, int32_t n_step,
                             const float* discount, uint64_t seed, uint64_t* draw_counter, int32_t* scratch,
                             const mel_replay_batch* out, void* stream);

/* Prioritized experience replay over a mel_round_replay: the counterpart of [3P] tianshou 1.0.0 PrioritizedVectorReplayBuffer, which
 * every training script of the reference switches to with --prio-buffer --alpha 0.6 --beta 0.4 (common.py:52,64-65,
 * l_dgn.py:169-176).  Parity unpinned: tianshou is restated from its published behaviour.  A transition is (env, slot, agent) with
 * agent in the record's acted set; buffer order is the memory order of prio.  All pointers are caller-owned DEVICE memory:
 *   prio      float  [B, K, N]  p^alpha of every transition; 0 for agents that did not act and slots not yet filled (start: 0)
 *   rec_sum   double [B * K]    scratch: per-record sums
 *   prefix    double [B * K + 1] scratch: their exclusive prefix sums, prefix[B * K] = total
 *   seen      int32  [B]        cursor[b] at the last sample (start: 0): records written since then are initialised lazily to
 *                               max_prio^alpha by the next sample - upstream's add(), without touching mel_env_round.
 *                               Written = ring slots seen .. cursor - 1 (mod K); all of them once cursor - seen >= K, or < 0 (the
 *                               cursor went back: the ring was reset).  A slot at or beyond min(cursor, K) holds no record: it is
 *                               never initialised from its (stale) acted set, and every sample sets its priorities to 0
 *   max_prio / min_prio float scalars: largest / smallest raw p = |td| + eps written back so far (start: 1.0)
 * alpha, beta >= 0; weight_norm != 0 divides the importance weights by their maximum over the batch (upstream's default). */
typedef struct mel_replay_priority {
    float*   prio;
    double*  rec_sum;
    double*  prefix;
    int32_t* seen;
    float*   max_prio;
    float*   min_prio;
    double   alpha;
    double   beta;
    int32_t  weight_norm;
    int32_t  reserved;
} mel_replay_priority;

/* mel_replay_sample with draws proportional to priority (PrioritizedReplayBuffer.sample_indices + get_weight, then
 * compute_nstep_return): scalar = u * sum(prio), u = (splitmix64(seed, *draw_counter, sample index) >> 11) * 2^-53; the sample is
 * the first transition, in buffer order, whose inclusive prefix sum exceeds it (float64 sums).  Outputs: everything
 * mel_replay_sample writes, plus weight float [batch] (device) = (prio / min_prio)^-beta in float64 [/ max over the batch].  Two
 * launches (refresh grid-wide, then one workgroup); also sets seen[b] = cursor[b] and increments *draw_counter.  An empty replay
 * samples like mel_replay_sample (index 0, weight 1).
 * MEL_ERR_INVALID_ARG: a null argument or incomplete struct, alpha < 0, beta < 0, batch outside [1, 1024], n_step outside
 * [1, MEL_REPLAY_MAX_NSTEP], n_envs * capacity > 2^24, nb_sibling without active_nb. */
mel_status mel_replay_sample_prio(const mel_round_replay* replay, const mel_replay_priority* priority, int64_t n_envs, int32_t n_nodes,
                                  int32_t batch, int32_t n_step, const float* discount, uint64_t seed, uint64_t* draw_counter,
                                  const mel_replay_batch* out, float* weight, void* stream);

/* PrioritizedReplayBuffer.update_weight(indices, td), called by [3P] BasePolicy.post_process_fn after every update with the TD
 * error the loss left in batch.weight: p = |td| + eps in float (eps = FLT_EPSILON), prio[env, slot, agent] = powf(p, alpha) - among
 * samples that name the same transition the highest sample index wins, as numpy's assignment does -, max_prio = max(max_prio,
 * max p), min_prio = min(min_prio, min p).  env / slot / agent: device int64 [batch] (a sampled batch's), td: device float [batch].
 * One workgroup, no atomics.  Samples outside [0, B) x [0, capacity) x [0, N) are skipped.
 * MEL_ERR_INVALID_ARG: null / incomplete struct, alpha < 0, beta < 0, index arrays or td missing, batch outside [1, 1024]. */
mel_status mel_replay_update_priority(const mel_replay_priority* priority, int64_t n_envs, int32_t capacity, int32_t n_nodes,
                                      int32_t batch, const int64_t* env, const int64_t* slot, const int64_t* agent, const float* td,
                                      void* stream);

/* One Adam update of up to MEL_ADAM_MAX_TENSORS parameter tensors in one launch ([3P] torch.optim.Adam as the reference
 * configures it, l_dgn.py:207: no amsgrad, L2 weight decay): exp_avg <- lerp(exp_avg, g, 1 - beta1); exp_avg_sq <- beta2 exp_avg_sq
 * + (1 - beta2) g^2; param <- param - lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps).  All pointers
 * device fp32.  step[i]: the tensor's step counter as torch keeps it in capturable mode (device fp32 scalar, the number of updates
 * DONE: the launch uses t = *step + 1 and a second small launch stores it back) - or NULL for all tensors, then t = host_step. */
#define MEL_ADAM_MAX_TENSORS 64
typedef struct mel_adam_tensors {
    int32_t      count;
    int32_t      reserved;
    float*       param[MEL_ADAM_MAX_TENSORS];
    const float* grad[MEL_ADAM_MAX_TENSORS];
    float*       exp_avg[MEL_ADAM_MAX_TENSORS];
    float*       exp_avg_sq[MEL_ADAM_MAX_TENSORS];
    float*       step[MEL_ADAM_MAX_TENSORS];
    int64_t      numel[MEL_ADAM_MAX_TENSORS];
} mel_adam_tensors;
mel_status mel_adam_step(const mel_adam_tensors* t, float lr, float beta1, float beta2, float eps, float weight_decay,
                         double host_step, void* stream);

/* The TD target and the TD loss of one update, one launch each: what a torch formulation spends ~20 one-line launches on (index /
 * sub / pow / mean / mul and their autograd backward nodes; argmax / gather / mul / add on the target side).  All buffers device
 * fp32 unless said otherwise, row-major; no float atomics, every sum in a fixed order - two calls on the same inputs give the same
 * bits; no host value changes between two calls of an update, so both replay from a HIP graph.
 *
 * mel_td_target ([3P] DQNPolicy._target_q + compute_nstep_return as l_dgn.py:70-78 configures them: is_double, estimation_step):
 *   best_i = q_target[i, argmax_a q_online[i, a]] (double DQN; the lowest index wins a tie) or max_a q_target[i, a] when q_online is
 *   NULL; returns_i = ret_i + boot_w_i * best_i, the product and the sum rounded separately (no fused multiply-add): the bits of the
 *   torch expression.  q_target / q_online [batch, n_actions], ret / boot_w / returns [batch].
 * mel_td_loss ([3P] DQNPolicy.learn with n_nodes = 1 and member = NULL: q = logits [batch, n_actions]; policies/dgn.py:43-64 and
 *   policies/n_dgn.py:36-66 with member = the siblings summed over, [batch, n_nodes] floats, 0 = not a sibling):
 *     batch_q_i = sum_j member_ij q[i, j, act_ij]        td_i = returns_i - batch_q_i
 *     loss = mean_i weight_i td_i^2   (huber = 0; weight NULL = 1)   or   huber_loss(batch_q, returns), delta = 1, mean, weight unused
 *     dq[i, j, a] = d loss / d q[i, j, a]: -2 weight_i td_i / batch at (j, a = act_ij) of a sibling, 0 elsewhere - EVERY element is
 *     written, dq needs no memset.
 *   q / dq [batch, n_nodes, n_actions], act device int64 [batch, n_nodes] (an action outside [0, n_actions) counts as no sibling),
 *   loss [1], td [batch].  scratch: device memory of (batch + MEL_TD_GROUP_ROWS - 1) / MEL_TD_GROUP_ROWS floats - the workgroups'
 *   partial sums, added in index order by a second small launch; unused (may be NULL) when that is one.
 * MEL_ERR_INVALID_ARG: a null pointer, batch outside [1, MEL_TD_MAX_BATCH], n_actions outside [1, MEL_TD_MAX_ACTIONS], n_nodes outside
 * [1, MEL_MAX_NODES]; MEL_ERR_WORKSPACE: scratch_bytes below what the batch needs. */
#define MEL_TD_GROUP_ROWS 64
#define MEL_TD_MAX_BATCH 65536
#define MEL_TD_MAX_ACTIONS 8
mel_status mel_td_target(const float* q_target, const float* q_online, const float* ret, const float* boot_w, int64_t batch,
                         int32_t n_actions, float* returns, void* stream);
mel_status mel_td_loss(const float* q, const int64_t* act, const float* member, const float* returns, const float* weight,
                       int64_t batch, int32_t n_nodes, int32_t n_actions, int32_t huber, float* loss, float* td, float* dq,
                       void* scratch, size_t scratch_bytes, void* stream);

/* One whole env ROUND per launch for every env of the batch (round-batched loop): replays, in the
 * reference's AEC order, the dead-agent steps and one GraphEnv.step per active agent with that agent's
 * action until the world step fires or the episode ends (then the env is reset to
 * episode_table[b, ep_cursor % table_stride]).  State after the call is identical to issuing the same
 * steps one at a time through mel_env_step.
 *   actions     device int32 [rows], one per (env, active agent), ordered by env then agent id
 *   row_offsets device int32 [B+1], first action row of each env (from mel_ldgn_forward_agents); NULL =
 *               actions is the dense layout [B, N] indexed by agent id (mel_select_action_envs)
 *   live        device uint64 [B]; in: the active sets the actions belong to, out: the next round's
 *   first != 0  only publishes the current active sets (call once after mel_env_reset).
 *   round_counter (optional, device uint32): incremented once per call.
 *   replay (optional): every env that had acting agents appends one record (see mel_round_replay). */
mel_status mel_env_round(mel_env_batch* env, const mel_episode_pool* pool, const int32_t* actions,
                         const int32_t* row_offsets, uint64_t* live, const int32_t* episode_table,
                         int32_t table_stride, int32_t first, uint32_t* round_counter,
                         const mel_round_replay* replay, void* stream);

/* Reads the per-step logger_stats pool (mel_env_batch.step_stats): one workgroup merges the B per-env accumulators in a
 * fixed order (thread t folds envs t, t + 256, ... in index order, then a fixed pairwise tree), so the result is the
 * same from run to run.  out: device double [1 + 4 * MEL_ENV_LOGGER_STATS] = the sample count, then per key mean, std, max,
 * min - std = sqrt(M2 / n), the population std of SequenceSummaryStats.from_sequence (collector.py:14-30).  No sample:
 * count 0 and zeros.  reset != 0 also empties every env's accumulator in the same launch (all 41 doubles to zero: the
 * count gates the rest).  MEL_ERR_INVALID_ARG: env or out NULL, an unbound batch, step_stats == NULL. */
mel_status mel_env_step_stats(const mel_env_batch* env, double* out, int32_t reset, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training curves accumulated ON THE DEVICE (what the reference's train_agent hands to [3P] tianshou's logger, l_dgn.py:203-213,
 * 237-238,260: train/reward, train/length, train/episode, train/eps, update/loss about every 1000 env steps).  The round loop and
 * the update replay from HIP graphs and nothing in them reads the device, so the curve is summed per INTERVAL of env steps by two
 * capturable launches into a caller-owned ring of records, and the host reads the ring where it synchronises anyway (the epoch
 * boundary).  All pointers of mel_train_log are DEVICE memory:
 *   records      double [capacity][MEL_TRAIN_LOG_DOUBLES]  one record per ring slot, fields MEL_TL_*
 *   interval_id  int64  [capacity]   the interval a slot currently holds, -1 = empty (start: all -1)
 *   counters     int64  [4]          MEL_TLC_*: records overwritten before they were drained, episode rows the env's log dropped,
 *                                    second rows of one env within one drain; [3] reserved (start: 0)
 *   base         uint64 [1]          env_step of interval 0's start; UINT64_MAX = not armed
 *   drained_upto int64  [1]          the first interval the host has NOT read yet (start: 0)
 * base and drained_upto are device memory so that launches captured before the host sets them follow the values it sets later.
 * decisions / stride / n_envs / scale: the env batch's decision counters exactly as mel_exploration_schedule takes them.
 *
 * Both launches compute env_step = scale * sum_b decisions[b * stride] (64-bit integer sum).  Not armed, or env_step < base:
 * nothing is recorded and no counter moves.  Otherwise k = (env_step - base) / interval, slot = k % capacity; a slot that holds
 * another interval is first cleared to the empty record (every field 0.0 except the MEL_TL_*_MIN field +inf, the *_MAX fields
 * -inf and MEL_TL_EPS_LAST -1.0) and takes id k - and if the id it held was >= *drained_upto (not -1), counters[MEL_TLC_LOST_RECORDS]
 * is incremented.  Every field is a double; sums run in stream order, so the same launches on the same inputs give the same bits.
 * Maxima and minima use explicit compares in which a NaN wins and stays (not fmax, see mel_td_target).
 *
 * mel_train_log_round - after every mel_env_round of a training loop.  Consumes rows [0, min(*env->log_cursor, log_capacity))
 *   of the env batch's episode log (read only) and stores 0 to the cursor, armed or not.  Per interval: MEL_TL_EPISODES, the sum /
 *   sum of squares / min / max of episode_rewards_sum, the sums of num_moves, coverage, coverage_interested_fraction and
 *   total_messages_transmitted, MEL_TL_ROUNDS (+1 per call), MEL_TL_ENV_STEP_LAST and MEL_TL_EPS_LAST (*eps_dev; eps_dev NULL
 *   leaves it).  Rows land in the episode log in atomic order; the record does not depend on it: rows are scattered by env id (in LDS),
 *   lane t of one 256-lane workgroup folds envs t, t + 256, ... in ascending order and the lanes meet in a fixed pairwise tree
 *   (lane t += lane t + o, o = 128, 64 .. 1).  Cursor values beyond log_capacity add to counters[MEL_TLC_LOST_EPISODES] (so do rows
 *   whose env id is outside [0, n_envs)).  An env ends at most one episode per round; a second row of one env increments
 *   counters[MEL_TLC_DUPLICATE_ENV_ROWS] and is still folded, the env's rows in (pool episode, row) order.  One launch.
 * mel_train_log_update - once per update, directly in front of mel_adam_step, so that it sees the gradient Adam applies.
 *   loss float [1], td float [batch] (mel_td_loss's), grads: the optimizer's table (grad[i], numel[i], i < count; numel >= 0).
 *   Per interval: MEL_TL_UPDATES, sum / max / last of loss, sum and max of the update's mean_i |td_i| (lane l of one wavefront adds
 *   |td_i| for i = l, l + 64, ... in double, lane 0 adds the lanes in order, / batch), max of |td_i|, sum / max / last of the global
 *   gradient L2 norm.  The norm: every gradient widened to double and squared (exact); 256-lane workgroups sum chunks of
 *   MEL_TRAIN_LOG_GRAD_CHUNK elements (lane t its elements t, t + 256, ..., then the pairwise tree above) into scratch, and the
 *   one-wavefront launch that writes the record adds them (lane l a run of consecutive partials, lane 0 the lanes in order) and
 *   takes the square root: no float atomics, relative error <= total_numel * 2^-52.  A NaN in loss, td or a gradient reaches the
 *   record.  scratch: device, mel_train_log_scratch_bytes(grads) bytes (8 per chunk; 0 for a bad table).  Two launches.
 * Neither reads on the host nor allocates: both replay from a HIP graph.
 * MEL_ERR_INVALID_ARG: a null log / buffer / decisions / loss / td / grads, capacity < 1, interval < 1, n_envs < 1, stride < 1,
 * batch outside [1, MEL_TD_MAX_BATCH], count outside [1, MEL_ADAM_MAX_TENSORS], a null gradient or negative numel, an env batch
 * without an episode log (log_capacity < 1 or null log buffers) or with another n_envs; MEL_ERR_WORKSPACE: scratch_bytes too small. */
#define MEL_TRAIN_LOG_DOUBLES     32
#define MEL_TRAIN_LOG_GRAD_CHUNK  4096
#define MEL_TL_EPISODES            0   /* episodes ended                                   empty 0      */
#define MEL_TL_REW_SUM             1   /* sum of episode_rewards_sum                             0      */
#define MEL_TL_REW_SQ              2   /* sum of its squares                                     0      */
#define MEL_TL_REW_MIN             3   /*                                                        +inf   */
#define MEL_TL_REW_MAX             4   /*                                                        -inf   */
#define MEL_TL_MOVES_SUM           5   /* sum of num_moves                                       0      */
#define MEL_TL_COVERAGE_SUM        6   /* sum of coverage                                        0      */
#define MEL_TL_COV_INTERESTED_SUM  7   /* sum of coverage_interested_fraction                    0      */
#define MEL_TL_MESSAGES_SUM        8   /* sum of total_messages_transmitted                      0      */
#define MEL_TL_ROUNDS              9   /* round launches                                         0      */
#define MEL_TL_ENV_STEP_LAST      10   /* env_step of the last launch of either kind             0      */
#define MEL_TL_EPS_LAST           11   /* exploration rate of the last round                     -1     */
#define MEL_TL_UPDATES            12   /* update launches                                        0      */
#define MEL_TL_LOSS_SUM           13   /*                                                        0      */
#define MEL_TL_LOSS_MAX           14   /*                                                        -inf   */
#define MEL_TL_LOSS_LAST          15   /*                                                        0      */
#define MEL_TL_TD_ABS_SUM         16   /* sum over updates of mean_i |td_i|                      0      */
#define MEL_TL_TD_ABS_MEAN_MAX    17   /* max over updates of mean_i |td_i|                      -inf   */
#define MEL_TL_TD_ABS_MAX         18   /* max over updates and samples of |td_i|                 -inf   */
#define MEL_TL_GRAD_NORM_SUM      19   /*                                                        0      */
#define MEL_TL_GRAD_NORM_MAX      20   /*                                                        -inf   */
#define MEL_TL_GRAD_NORM_LAST     21   /*                                                        0      */
                                       /* 22 .. 31: padding, 0                                          */
#define MEL_TLC_LOST_RECORDS       0
#define MEL_TLC_LOST_EPISODES      1
#define MEL_TLC_DUPLICATE_ENV_ROWS 2
typedef struct mel_train_log {
    double*        records;
    int64_t*       interval_id;
    int64_t*       counters;
    uint64_t*      base;
    int64_t*       drained_upto;
    const int32_t* decisions;
    int64_t        interval;       /* env steps per record                                             */
    int32_t        capacity;       /* ring slots                                                       */
    int32_t        stride;
    int32_t        n_envs;
    uint32_t       scale;
} mel_train_log;
size_t     mel_train_log_scratch_bytes(const mel_adam_tensors* grads);
mel_status mel_train_log_round(const mel_train_log* log, const mel_env_batch* env, const float* eps_dev, void* stream);
mel_status mel_train_log_update(const mel_train_log* log, const float* loss, const float* td, int64_t batch,
                                const mel_adam_tensors* grads, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-round dissemination curves and node traces of an evaluation, recorded ON THE DEVICE: what the reference shows by drawing
 * the graph after every world step (graph.py:350-356, draw_graph :466-484).  The rounds replay from HIP graphs and nothing reads
 * the device between them, so one capturable launch behind every mel_env_round samples the state the round left.  An env's loop
 * inside mel_env_round ends at a world step or at an episode end with reset: the state a launch sees is either "after world
 * step num_moves of the current episode" or "the new episode's reset state, num_moves == 0".  When the observation right after
 * a world step raises explicit_reset (graph.py:205-211) the episode ends in the launch of its last world step and that state
 * is gone; its figures are in the env batch's episode log (mel_env_batch.log_*: final logger_stats and num_moves), which the
 * recorder therefore NEEDS: the log must be on, large enough not to drop rows (rows are only looked up, never consumed), and
 * not emptied by another launch between a round and the recorder's launch (mel_train_log_round does that: not both).
 * All pointers of mel_round_record are caller-owned DEVICE memory (B = n_envs, R = max_rounds, N = n_nodes, W = MEL_SET_WORDS(N)):
 *   running   double [B][R][MEL_RR_FIELDS]  sum of the samples env b took at round index r                       (start: 0)
 *   ended     double [B][R][MEL_RR_FIELDS]  sum of the FINAL rows of env b's ended episodes, at their last round index (start: 0)
 *   seen      int32  [B][MEL_RR_CARRY]      the env's carry: MEL_S_EPISODES_DONE and MEL_S_NUM_MOVES of the state sampled last,
 *                                           the round index of the running episode's last sample (-1: none), whether every
 *                                           interested node held the message at it, the episode-log rows looked at so far,
 *                                           one reserved                                                         (start: all -1)
 *   last      double [B][MEL_RR_FIELDS]     the running episode's last sample
 *   overflow  int64  [B]   rows not stored because their round index was >= R (a sample, or an episode's final row)  (start: 0)
 *   skipped   int64  [B]   launches that found the env with MEL_S_ERROR != 0                                     (start: 0)
 *   unlogged  int64  [B]   ended episodes whose row was not in the episode log (it was full)                     (start: 0)
 *   quota     int32  [B]   optional (NULL: no limit): episodes of env b that count
 * mel_round_record_round, per env (one wavefront, 4 envs per 256-lane workgroup, no atomics - an env owns its rows):
 *   - (episodes_done, num_moves) equal to the carry: nothing (a second launch on the same state is idempotent);
 *   - else MEL_S_ERROR != 0: skipped[b] += 1, nothing else;
 *   - else, episodes_done differs from the carry's: the previous episode has ended.  If it has a last sample, the env's newest
 *     row among the episode-log rows it has not looked at yet gives the episode's final num_moves and the logger_stats of its
 *     final observation (the selected agent's slot as stored: what an evaluation reports for the episode), as a row of fields
 *     0 .. 7 = 1, round(coverage * N), coverage_interested_count, interested_agents, total_messages_transmitted, 0 (nobody
 *     acts any more), coverage_interested_fraction, newly covered by the rule below.  Where the final num_moves is not the last
 *     sample's round, that row is the episode's final sample: added to running[b][num_moves] (it has no trace record: the node
 *     state is gone) and to ended[b][num_moves].  Otherwise ended[b][last round] takes `last` with fields 1 - 4 and 6 from the
 *     row.  So per env the ended sums of fields 4 and 6 ARE the sums of its episode-log rows, added in play order.  The episode
 *     carry is cleared.  No row (a full log): unlogged[b] += 1 and `last` is booked as it stands;
 *   - then, unless quota && episodes_done >= quota[b], ONE sample at round index r = num_moves, MEL_RR_FIELDS doubles:
 *       0 count 1;  1 |has_message|;  2 |has_message & interested|;  3 |interested|;  4 MEL_S_WORLD_MSGS;  5 |MEL_SEL_ACTIVE|;
 *       6 coverage_interested_fraction as get_info computes it (graph.py:158-162): field 2 / field 3 in one double division, 0
 *         when no node is interested;
 *       7 newly covered: 1 when every interested node (at least one) holds the message and that was not so at the episode's
 *         previous sample, else 0
 *     added to running[b][r], kept as `last`; the carry takes the state.  All fields but 6 are integers: their sums are exact in
 *     any order; field 6 is summed per env in play order.  An env past its quota still books the end of its last counted episode.
 *   - trace sink (n_trace > 0): trace_env[t] lists up to MEL_RR_MAX_TRACE distinct envs (VALUES inside the struct, checked on the
 *     host), each with a ring of trace_capacity records.  Every sample a listed env takes (stored or overflowed) also writes
 *     record trace_cursor[t] % trace_capacity and advances trace_cursor[t] (int64, start: 0).  Struct-of-arrays, record rec =
 *     t * trace_capacity + slot:
 *       trace_meta       int32  [T][cap][8]     env, episode ordinal (episodes_done), MEL_S_EPISODE, num_moves, MEL_S_ORIGIN,
 *                                               MEL_S_WORLD_MSGS, 0, 0
 *       trace_pos        double [T][cap][N][2]
 *       trace_one_hop    uint64 [T][cap][N][W]
 *       trace_sets       uint64 [T][cap][6][W]  has_message, origin, interested, scripted, MEL_SEL_ACTIVE, MEL_SEL_TAKEN_ACTION
 *       trace_agent_msgs int32  [T][cap][N]
 *       trace_received   int32  [T][cap][N]
 * mel_round_record_read: running_out / ended_out device double [R][MEL_RR_FIELDS] = the envs' rows added in ascending env order
 *   (a thread per (round, field): equal inputs give equal bits), counters_out device int64 [4] = MEL_RRC_*: the sums of overflow,
 *   skipped and unlogged, one reserved.
 * Neither reads on the host nor allocates: both replay from a HIP graph.  MEL_ERR_INVALID_ARG: a null record / buffer / env /
 * output, an env batch without an episode log, max_rounds outside [1, MEL_RR_MAX_ROUNDS], n_envs or n_nodes other than the env batch's, n_trace outside
 * [0, MEL_RR_MAX_TRACE], a traced env outside [0, n_envs) or listed twice, trace_capacity < 1 or a null trace buffer with
 * n_trace > 0. */
#define MEL_RR_FIELDS      8
#define MEL_RR_CARRY       6
#define MEL_RR_MAX_TRACE  16
#define MEL_RR_MAX_ROUNDS (1 << 20)
#define MEL_RRC_OVERFLOW   0
#define MEL_RRC_SKIPPED    1
#define MEL_RRC_UNLOGGED   2
typedef struct mel_round_record {
    double*        running;
    double*        ended;
    int32_t*       seen;
    double*        last;
    int64_t*       overflow;
    int64_t*       skipped;
    int64_t*       unlogged;
    const int32_t* quota;
    int64_t*       trace_cursor;
    int32_t*       trace_meta;
    double*        trace_pos;
    uint64_t*      trace_one_hop;
    uint64_t*      trace_sets;
    int32_t*       trace_agent_msgs;
    int32_t*       trace_received;
    int32_t        n_envs;
    int32_t        n_nodes;
    int32_t        max_rounds;
    int32_t        n_trace;
    int32_t        trace_capacity;
    int32_t        reserved;
    int32_t        trace_env[MEL_RR_MAX_TRACE];
} mel_round_record;
mel_status mel_round_record_round(const mel_round_record* rec, const mel_env_batch* env, void* stream);
mel_status mel_round_record_read(const mel_round_record* rec, double* running_out, double* ended_out, int64_t* counters_out,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * The policy's decisions per round, recorded ON THE DEVICE: which nodes the policy let relay, how sure it was, against the
 * round index and against the node's degree (the forwarding ratio per hop and per neighbourhood size of a dissemination
 * paper).  The data exists between two launches only: mel_*_forward_agents / mel_hldgn_forward_envs_select writes the round's
 * logits and actions, mel_env_round consumes the actions and overwrites `live`.  So ONE capturable launch sits BETWEEN the
 * forward and mel_env_round and reads what the forward wrote and the state the decisions were taken in.  It touches nothing
 * the round loop reads (not the episode log either: it rides with or without mel_round_record / mel_train_log).
 * All pointers of mel_decision_record are caller-owned DEVICE memory (B = n_envs, R = max_rounds, D = n_degrees, N = n_nodes,
 * W = MEL_SET_WORDS(N)):
 *   by_round   double [B][R][MEL_DR_FIELDS]  sums over the decisions env b took in a state with MEL_S_NUM_MOVES == r  (start: 0)
 *   by_degree  double [B][D][MEL_DR_FIELDS]  the same rows by the deciding node's degree, min(degree, D - 1)          (start: 0)
 *   overflow   int64  [B]   by_round rows dropped because their round index was >= R (by_degree is still booked)      (start: 0)
 *   skipped    int64  [B]   launches that found the env with MEL_S_ERROR != 0                                         (start: 0)
 *   quota      int32  [B]   optional (NULL: no limit): episodes of env b that count (mel_round_record's rule)
 * mel_decision_record_round(rec, env, logits, act, row_offsets, live, n_actions, stream): logits / act / row_offsets / live are
 * the round's forward outputs in one of the two layouts of the round loop -
 *   row_offsets != NULL (L-DGN, DGN-R): the rows of env b are row_offsets[b] .. row_offsets[b + 1], one per member of live[b]
 *     in ascending node id; logits float [rows][2], act int32 [rows];
 *   row_offsets == NULL (HL-DGN): logits row b serves every agent of live[b]; act is the dense int32 [B][N] layout;
 *   live uint64 [B][W] (members >= N are ignored).  n_actions must be 2 ("relay" is action 1), else MEL_ERR_UNSUPPORTED.
 * Per env (one wavefront, 4 envs per 256-lane workgroup, no atomics - an env owns its rows):
 *   - MEL_S_ERROR != 0: skipped[b] += 1, nothing else;
 *   - quota && MEL_S_EPISODES_DONE >= quota[b]: nothing;
 *   - the policy's decisions are the members of live[b] that are not in MEL_SET_SCRIPTED (a scripted node's action is replaced
 *     by its heuristic inside the env).  For each, in ASCENDING node id, one after the other, a row of MEL_DR_FIELDS doubles is
 *     added to by_round[b][r], r = MEL_S_NUM_MOVES, and to by_degree[b][min(degree, D - 1)], degree = column 2 of the node's
 *     obs_matrix row (q = the node's logits row, a = its action):
 *       0 decisions: 1;  1 relays: a == 1;  2 gap = q[1] - q[0], ONE fp32 subtraction, widened;  3 gap * gap in double;
 *       4 the chosen action's Q (q[1] when a == 1, else q[0]);  5 the row's larger Q (q[1] when q[1] > q[0], else q[0]);
 *       6 non-greedy: a differs from the first maximum of q, which is what the fused selection takes at eps = 0;
 *       7 first decisions: the node's MEL_SEL_TAKEN_ACTION bit is clear.
 *     The fixed order makes the floating fields reproducible bit for bit;
 *   - r >= R: the decision's by_round row is dropped and overflow[b] += 1 (per dropped row); its by_degree row is still booked;
 *   - trace sink (n_trace > 0): mel_round_record's, rule for rule (one implementation serves both: trace_env[], the rings, the
 *     cursor, the first four header ints, the argument errors; MEL_DR_MAX_TRACE == MEL_RR_MAX_TRACE).  Here a launch that booked
 *     at least one decision for a listed env writes the record; rec = t * trace_capacity + slot:
 *       trace_meta  int32  [T][cap][8]     env, episode ordinal (episodes_done), MEL_S_EPISODE, num_moves, decisions, relays, 0, 0
 *       trace_sets  uint64 [T][cap][2][W]  the deciding set, the relaying set (deciding with a == 1)
 *       trace_q     float  [T][cap][N][2]  the node's logits row; 0 for nodes that did not decide
 *     Records join mel_round_record's node traces on (env, episode ordinal, num_moves): the state sampled after round r - 1 is
 *     the state round r's decisions were taken in.
 * mel_decision_record_read: by_round_out device double [R][MEL_DR_FIELDS], by_degree_out device double [D][MEL_DR_FIELDS] = the
 *   envs' rows added in ascending env order (a thread per (row, field): equal inputs give equal bits), counters_out device
 *   int64 [4] = MEL_DRC_*: the sums of overflow and skipped, two reserved (written 0).
 * Neither reads on the host nor allocates: both replay from a HIP graph.  MEL_ERR_INVALID_ARG: a null record / buffer / env /
 * logits / act / live / output, an unbound env batch, n_envs or n_nodes other than the env batch's, max_rounds outside
 * [1, MEL_DR_MAX_ROUNDS], n_degrees outside [1, MEL_DR_MAX_DEGREES], n_trace outside [0, MEL_DR_MAX_TRACE], a traced env
 * outside [0, n_envs) or listed twice, trace_capacity < 1 or a null trace buffer with n_trace > 0. */
#define MEL_DR_FIELDS       8
#define MEL_DR_MAX_TRACE   16
#define MEL_DR_MAX_ROUNDS  (1 << 20)
#define MEL_DR_MAX_DEGREES MEL_MAX_NODES
#define MEL_DRC_OVERFLOW    0
#define MEL_DRC_SKIPPED     1
typedef struct mel_decision_record {
    double*        by_round;
    double*        by_degree;
    int64_t*       overflow;
    int64_t*       skipped;
    const int32_t* quota;
    int64_t*       trace_cursor;
    int32_t*       trace_meta;
    uint64_t*      trace_sets;
    float*         trace_q;
    int32_t        n_envs;
    int32_t        n_nodes;
    int32_t        max_rounds;
    int32_t        n_degrees;
    int32_t        n_trace;
    int32_t        trace_capacity;
    int32_t        trace_env[MEL_DR_MAX_TRACE];
} mel_decision_record;
mel_status mel_decision_record_round(const mel_decision_record* rec, const mel_env_batch* env, const float* logits,
                                     const int32_t* act, const int32_t* row_offsets, const uint64_t* live, int32_t n_actions,
                                     void* stream);
mel_status mel_decision_record_read(const mel_decision_record* rec, double* by_round_out, double* by_degree_out,
                                    int64_t* counters_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whom the deciding agents attend to, per round, recorded ON THE DEVICE: does a deciding node listen to neighbours that already
 * hold the message or to those still waiting for it, and how does that change with the round and with the node's degree.  Like
 * the decisions, the data exists between two launches only: after the forward, mel_forward_attention (above) turns what the
 * forward left in its workspace into alpha / sources; mel_env_round then overwrites the state the decision was taken in.  So
 * mel_attention_record_round sits where mel_decision_record_round sits, behind mel_forward_attention, and reads alpha, sources
 * and the env's sets as they stand at the launch.  It touches nothing the round loop reads.
 * All pointers of mel_attention_record are caller-owned DEVICE memory (B = n_envs, R = max_rounds, D = n_degrees, H = n_heads,
 * N = n_nodes, W = MEL_SET_WORDS(N)); every table is per env, double, written without atomics (an env owns its rows):
 *   by_round   double [B][R][MEL_AR_FIELDS]  per decision env b took with MEL_S_NUM_MOVES == r: the HEAD MEAN of each field  (start: 0)
 *   by_degree  double [B][D][MEL_AR_FIELDS]  the same head mean by the deciding node's degree, min(degree, D - 1)             (start: 0)
 *   by_head    double [B][H][MEL_AR_FIELDS]  the per-head values                                                              (start: 0)
 *   overflow, skipped, quota: mel_decision_record's, rule for rule.
 * mel_attention_record_round(rec, env, alpha, sources, row_offsets, live, heads, stream): alpha float [rows][MEL_ATT_MAX_SOURCES]
 *   [heads] and sources uint64 [rows][W] as mel_forward_attention writes them (members >= N of a source set are ignored),
 *   row_offsets int32 [B + 1] and live uint64 [B][W] the round's; heads must equal rec->n_heads.
 * Per env (one wavefront, 4 envs per 256-lane workgroup): the error skip, the quota, the round index MEL_S_NUM_MOVES, the degree
 * (column 2 of the node's obs_matrix row, clamped to [0, D - 1]), the overflow rule and the walk in ASCENDING node id are
 * mel_decision_record's.  A decision is a member of live[b] that is not in MEL_SET_SCRIPTED, at row row_offsets[b] + its rank in
 * live[b].  Per decision of node i and per head h, with a_k = (double)alpha[row][k][h] of the row's k-th source j_k in ascending
 * node id (k < min(|sources|, MEL_ATT_MAX_SOURCES) = c), every sum starting at 0.0 and taken in that order:
 *     0 decisions: 1
 *     1 self: a_k of j_k == i (0 where i is no source of its own: TransformerConv)
 *     2 informed: sum of a_k over j_k != i in MEL_SET_HAS_MESSAGE          3 that class's size / c
 *     4 waiting:  sum of a_k over j_k != i in MEL_SET_INTERESTED & ~MEL_SET_HAS_MESSAGE     5 that class's size / c
 *     6 sum of a_k * a_k (its reciprocal is the effective number of neighbours)             7 max a_k (0 upwards)
 *   A decision without sources (c == 0) books field 0 only.  The head mean of a field is the sum over the heads in ascending
 *   order divided by (double)heads.  Additions, multiplications, divisions and comparisons of IEEE doubles in a fixed order,
 *   no transcendental function: a NumPy restatement gives the tables bit for bit.
 *   - r >= R: the decision's by_round row is dropped and overflow[b] += 1; by_degree and by_head are still booked;
 *   - trace sink: the shared one (mel_round_record's: trace_env[], rings, cursor, header, argument errors).  A launch that booked
 *     at least one decision for a listed env writes the record:
 *       trace_meta    int32  [T][cap][8]     env, episode ordinal, MEL_S_EPISODE, num_moves, decisions, decisions without sources, 0, 0
 *       trace_sets    uint64 [T][cap][W]     the deciding set
 *       trace_fields  double [T][cap][N][MEL_AR_FIELDS]  the node's head-mean fields; 0 for nodes that did not decide
 *     Records join the other two recorders' records on (env, episode ordinal, num_moves).
 * mel_attention_record_read: by_round_out [R][8], by_degree_out [D][8], by_head_out [H][8] device doubles = the envs' rows added
 *   in ascending env order by one thread per element; counters_out device int64 [4] = MEL_DRC_* (overflow, skipped, 0, 0).
 * Neither reads on the host nor allocates: both replay from a HIP graph.  MEL_ERR_INVALID_ARG: mel_decision_record's cases, a
 * null alpha / sources / row_offsets / live / by_head, n_heads outside [1, MEL_AR_MAX_HEADS], heads != rec->n_heads. */
#define MEL_AR_FIELDS       8
#define MEL_AR_MAX_HEADS   16
typedef struct mel_attention_record {
    double*        by_round;
    double*        by_degree;
    double*        by_head;
    int64_t*       overflow;
    int64_t*       skipped;
    const int32_t* quota;
    int64_t*       trace_cursor;
    int32_t*       trace_meta;
    uint64_t*      trace_sets;
    double*        trace_fields;
    int32_t        n_envs;
    int32_t        n_nodes;
    int32_t        max_rounds;
    int32_t        n_degrees;
    int32_t        n_heads;
    int32_t        n_trace;
    int32_t        trace_capacity;
    int32_t        trace_env[MEL_DR_MAX_TRACE];
} mel_attention_record;
mel_status mel_attention_record_round(const mel_attention_record* rec, const mel_env_batch* env, const float* alpha,
                                      const uint64_t* sources, const int32_t* row_offsets, const uint64_t* live, int32_t heads,
                                      void* stream);
mel_status mel_attention_record_read(const mel_attention_record* rec, double* by_round_out, double* by_degree_out,
                                     double* by_head_out, int64_t* counters_out, void* stream);

/* last() only (mutates is_new_round exactly like GraphEnv.observe, graph.py:205-211). */
mel_status mel_env_observe(mel_env_batch* env, const int32_t* env_ids, int64_t n,
                           const mel_env_obs* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optional stage timer: while a profiler is attached to the calling thread, every launch group of the
 * entry points above is bracketed by a pair of HIP events recorded on the caller's stream
 * (measurement only - bench.py uses it for the live per-kernel roofline; nothing else in the library
 * creates events or synchronises).  mel_prof_read synchronises on the recorded events.
 * ------------------------------------------------------------------------------------------------ */
#define MEL_STAGE_PLAN          0   /* plan_masks + plan_scan + plan_lists                       */
#define MEL_STAGE_ENCODER       1   /* encoder GEMM (layer 0 fused into the A-tile producer)     */
#define MEL_STAGE_CONV1_LIN     2   /* conv1.lin_l (+ lin_r for HL-DGN, one launch)              */
#define MEL_STAGE_CONV1_LIN_R   3   /* conv1.lin_r (L-DGN one-hop rows)                          */
#define MEL_STAGE_CONV1_ATT     4   /* conv1 edge-softmax / aggregate (+ pool for HL-DGN)        */
#define MEL_STAGE_CONV2_LIN     5   /* conv2.lin_l                                               */
#define MEL_STAGE_CONV2_LIN_R   6   /* conv2.lin_r                                               */
#define MEL_STAGE_CONV2_ATT     7   /* conv2 attention for the controlling agent                 */
#define MEL_STAGE_HEAD_HIDDEN   8   /* dueling hidden layers                                     */
#define MEL_STAGE_HEAD_TAIL     9   /* last Linear + q - mean(q) + v                             */
#define MEL_STAGE_SELECT       10   /* mask + argmax + eps-greedy                                */
#define MEL_STAGE_ENV_STEP     11   /* env step (+ observe, + auto reset)                        */
#define MEL_STAGE_ENV_RESET    12
#define MEL_STAGE_ENV_OBSERVE  13
#define MEL_N_STAGES           14

void*      mel_prof_create(int32_t capacity);            /* capacity = max recorded launch groups */
void       mel_prof_destroy(void* prof);
void       mel_prof_attach(void* prof);                   /* NULL detaches                         */
void       mel_prof_reset(void* prof);
/* ms_sum / count: host arrays [MEL_N_STAGES]; returns number of records read (negative on error). */
int32_t    mel_prof_read(void* prof, double* ms_sum, int64_t* count);

const char* mel_last_error(void);
/* sizeof() of the structs of this header as the library was compiled, for binding authors to check their mirrors
 * against: which = 0 mel_linear, 1 mel_gatv2, 2 mel_mlp, 3 mel_weights, 4 mel_select, 5 mel_env_batch,
 * 6 mel_episode_pool, 7 mel_env_obs, 8 mel_round_replay, 9 mel_graph_pool, 10 mel_episode_stream, 11 mel_replay_batch, 12 mel_adam_tensors,
 * 13 mel_replay_priority, 14 mel_train_log, 15 mel_round_record, 16 mel_decision_record, 17 mel_attention_record;
 * 0 for anything else. */
size_t mel_abi_sizeof(int32_t which);
const char* mel_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MELISSA_HIP_H */
