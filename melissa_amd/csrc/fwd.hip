// L-DGN / HL-DGN forward for MI355X (gfx950): plan (obs unpack + fp32 radius adjacency + receptive
// field), fp32-MFMA row GEMMs (gemm_f32.hpp), GATv2 edge-softmax/aggregate, segmented pool, dueling
// tail, DQN action selection.  Reference semantics: networks/common.py:6-64, l_dgn.py:92-151,
// hl_dgn.py:82-119 and SURVEY.md Appendix A for the third-party operators.
#include <cmath>

#include "common.hpp"
#include "gemm_launch.hpp"
#include "plan.hpp"
#include "attention.hpp"
#include "attention_export.hpp"   // mel_forward_attention: conv2's coefficients of the last agents forward (kernel: attention_record.hip)
#include "heads.hpp"

namespace mel {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local Profiler* g_prof = nullptr;
Profiler* current_profiler() { return g_prof; }

// The row lists of a forward and the encoder rows of its node-feature table in ONE launch: the first `gemm_blocks`
// workgroups are 64 x 64 tiles of the (feature-domain) encoder GEMM, the rest run plan_lists.  The two are independent (the
// table depends on the weights only) and each is a latency-bound launch of a few hundred workgroups on its own.
// FUSED: the first workgroups are work items of the WHOLE table instead (table_fused_tile, gemm_table.hpp: encoder rows and
// conv1's projections of them), and no launch for the table follows.
template <int W, bool FUSED = false>
__global__ __launch_bounds__(256, 2) void plan_enc_kernel(PlanListsArgs pa, std::conditional_t<FUSED, TableArgs, GemmBatch> work,
                                                          int gemm_blocks) {
    if constexpr (FUSED) {
        __shared__ __attribute__((aligned(16))) float lds[TBL_LDS_FLOATS];
        if ((int)blockIdx.x < gemm_blocks) table_fused_tile(work, (int)blockIdx.x, lds);
        else plan_lists_body<W>(pa, (int)blockIdx.x - gemm_blocks);
    } else {
        if ((int)blockIdx.x < gemm_blocks) gemm_f32_tile<2, 2, 1, 1, GEMM_MODE_ENC>(work, (int)blockIdx.x);
        else plan_lists_body<W>(pa, (int)blockIdx.x - gemm_blocks);
    }
}

// HL-DGN's counterpart: its tuple ids (feature_ids) beside the encoder rows of the table, one launch instead of two
__global__ __launch_bounds__(256, 2) void fid_enc_kernel(const float* __restrict__ obs, int bs, int n, int obs_stride, int node_cols,
                                                         PlanBuffers p, int table_rows, GemmBatch batch, int gemm_blocks) {
    if ((int)blockIdx.x < gemm_blocks) gemm_f32_tile<2, 2, 1, 1, GEMM_MODE_ENC>(batch, (int)blockIdx.x);
    else feature_ids_body(obs, bs, n, obs_stride, node_cols, p, table_rows, (int)blockIdx.x - gemm_blocks);
}

// Encoder layer 0 on its own, for encoders WIDER than the GEMMs' fused producer stages (ENC_FUSED_MAX_K columns of layer-0
// weights in LDS: hidden 512).  A0[m, k] = relu(enc_b[k] + sum_f enc_w[k, f] x_f(m)) in the producer's arithmetic (fetch_a<ENC>),
// fp32 rows or - bf16 feature path - bf16 rows; the encoder's second layer then is a PLAIN GEMM on A0 (launch_encoder).
// One wavefront per row, a lane per column; rows by the device-side count where the problem has one.
constexpr int ENC_FUSED_MAX_K = 256;         // = ENC_MAX_K of the GEMM kernels
constexpr int ENC_MAX_WIDTH = 512;
__global__ __launch_bounds__(256) void encoder_layer0_kernel(GemmArgs g, float* A0, int as_bf16) {
    const int M = gemm_rows(g);
    const int lane = lane_id();
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += gridDim.x * 4) {
        float x[8];
        enc_features(g, row, x);
        for (int k = lane; k < g.K; k += 64) {
            float v = g.enc_b[k];
#pragma unroll
            for (int f = 0; f < 8; ++f)
                if (f < g.in_dim) v = fmaf(g.enc_w[(size_t)k * g.in_dim + f], x[f], v);
            v = fmaxf(v, 0.f);
            if (as_bf16) reinterpret_cast<uint16_t*>(A0)[(size_t)row * g.K + k] = (uint16_t)pack_bf16x2(v, 0.f);
            else A0[(size_t)row * g.K + k] = v;
        }
    }
}

// The encoder launch of problem g (an ENC-mode problem: obs / nid or feat_domain, enc_w, enc_b): the GEMM's fused producer
// where the encoder fits it, else layer 0 into `scratch` (g.M rows of g.K values) and a PLAIN GEMM on those rows.
static mel_status launch_encoder(GemmArgs g, float* scratch, hipStream_t s, const char* what, long m_hint = -1) {
    StageScope t(MEL_STAGE_ENCODER, s);
    if (g.K <= ENC_FUSED_MAX_K) return launch_gemm(g, GEMM_MODE_ENC, s, what, m_hint);
    if (!scratch) return fail(MEL_ERR_WORKSPACE, "%s: no scratch for the rows of an encoder %d wide", what, g.K);
    if (g.M <= 0) return MEL_OK;
    long rows = m_hint > 0 && m_hint < g.M ? m_hint : g.M;
    int grid = (int)((rows + 3) / 4);
    grid = grid < 1 ? 1 : grid > 8192 ? 8192 : grid;
    MEL_LAUNCH(encoder_layer0_kernel, dim3(grid), dim3(256), 0, s, g, scratch, g.bf16);
    if (mel_status st = check_launch(what)) return st;
    g.A = scratch, g.lda = g.K, g.arow = nullptr;
    g.obs = nullptr, g.nid = nullptr, g.feat_domain = 0;
    return launch_gemm(g, GEMM_MODE_PLAIN, s, what, m_hint);
}
static bool encoder_fuses(const mel_weights* w) { return w->encoder.layer[0].out_dim <= ENC_FUSED_MAX_K; }

// ------------------------------------------------------------------------------------------------
// workspace layout
// ------------------------------------------------------------------------------------------------
struct Dims {
    int64_t bs;        // envs / observation rows
    int n;
    int64_t rows_cap;  // most agent rows (AEC: bs; round-batched: up to bs*n)
    int64_t u1_cap;    // most conv1 targets
    int64_t u2_cap;    // most conv1 sources
};

static Dims make_dims(int64_t bs, int n, int64_t rows_cap, bool single_agent) {
    Dims d;
    d.bs = bs, d.n = n, d.rows_cap = rows_cap;
    d.u1_cap = single_agent ? bs * (n < 34 ? n : 34) : bs * n;    // |closed one-hop| <= 33 sources + self
    d.u2_cap = bs * n;
    return d;
}

struct FwdLayout {
    PlanBuffers plan;
    float* h0;      // encoder rows
    float* xl1;     // conv1 lin_l rows (HL-DGN: xl | xr in one [M, 2*HC] matrix)
    float* xr1;
    float* h1;      // conv1 output rows
    float* xl2;
    float* xr2;
    float* xcat;    // head input [rows, latent]
    float* hq[2];   // head hidden ping-pong [rows, qw + vw]
    float* hpart;   // split-K partial planes of the heads' first layer [HEAD_KSPLIT_MAX][rows, qw + vw] (fp32 path)
    float* minmax;
    float* enc0;    // encoder layer-0 rows, only for encoders wider than the GEMMs' fused producer (launch_encoder), else null
    uint16_t* wb;   // bf16 copies of the projection weights (bf16 feature path)
    size_t wb_elems;
    size_t bytes;
    size_t rows_cap;
};

// the weight matrices the dense projections read, in launch order; fp32 path: the nn.Parameter storages
// themselves, bf16 path: their bf16 copies in the workspace (refreshed by every call)
struct ProjWeights {
    const float* enc1;
    const float* c1l; const float* c1r; const float* c1v;
    const float* c2l; const float* c2r; const float* c2v;
    // conv2's matrices once more in 256-row blocks (planes only): what gemm_planes_kernel reads; null when the shape does not fit
    const float* c2l_blk; const float* c2r_blk; const float* c2v_blk;
    const float* q[MEL_MAX_HEAD_LAYERS];
    const float* v[MEL_MAX_HEAD_LAYERS];
    const ProjWeights* alt;        // MEL_PREC_F32_AUTO: the same matrices as bf16 planes (the slots above hold the fp32 ones)
};

// MEL_PREC_F32_SPLIT: the split kernels stage K in steps that need K >= 128 (check_gemm_shape).  A projection with a shorter K
// (hidden 64: the encoder's second layer and conv1; 64-wide dueling layers) keeps its fp32 matrix and runs on the exact-fp32
// kernels - the same fp32-accurate result.  resolve_projections and every launch site decide by this one rule.
// Layer i >= 1 of the Q head and of the V head share ONE launch (run_heads): the two are split together or not at all, by the
// shorter K of the pair, so that no launch ever mixes an fp32 matrix with bf16 planes.
constexpr int SPLIT_MIN_K = 128;
static int split_k(int sp, int K) { return sp && K >= SPLIT_MIN_K; }
static bool split_keeps_fp32(const mel_weights* w, const mel_linear& l) {
    if (l.in_dim < SPLIT_MIN_K) return true;
    if (!w->dueling) return false;
    for (int i = 0; i < w->q_head.n_layers && i < w->v_head.n_layers; ++i) {
        if (&l == &w->q_head.layer[i]) return w->v_head.layer[i].in_dim < SPLIT_MIN_K;
        if (&l == &w->v_head.layer[i]) return w->q_head.layer[i].in_dim < SPLIT_MIN_K;
    }
    return false;
}

static bool has_planes(const mel_weights* w) { return w->precision == MEL_PREC_F32_SPLIT || w->precision == MEL_PREC_F32_AUTO; }
static size_t lin_elems(const mel_linear& l) { return l.weight ? (size_t)l.in_dim * l.out_dim : 0; }

// visits every projection weight: f(const mel_linear&, const float** slot)
template <class F>
static void for_each_projection(const mel_weights* w, ProjWeights& pw, F f) {
    f(w->encoder.layer[1], &pw.enc1);
    f(w->conv1.lin_l, &pw.c1l), f(w->conv1.lin_r, &pw.c1r);
    if (w->conv1.kind == MEL_CONV_TRANSFORMER) f(w->conv1.lin_v, &pw.c1v);
    if (w->model != MEL_MODEL_HLDGN) {
        f(w->conv2.lin_l, &pw.c2l), f(w->conv2.lin_r, &pw.c2r);
        if (w->conv2.kind == MEL_CONV_TRANSFORMER) f(w->conv2.lin_v, &pw.c2v);
    }
    for (int i = 0; i + 1 < w->q_head.n_layers; ++i) f(w->q_head.layer[i], &pw.q[i]);
    if (w->dueling)
        for (int i = 0; i + 1 < w->v_head.n_layers; ++i) f(w->v_head.layer[i], &pw.v[i]);
}

static size_t projection_elems(const mel_weights* w) {
    ProjWeights pw{};
    size_t total = 0;
    for_each_projection(w, pw, [&](const mel_linear& l, const float**) { total += (lin_elems(l) + 7) & ~(size_t)7; });
    return total;
}

// conv2's projection weights in gemm_planes_kernel's block layout, kept beside the row-major planes (small launches stay on
// the kernels that read those): f(const mel_linear&, const float* ProjWeights::* slot)
static bool conv2_blocks_fit(const mel_weights* w) {
    return w->model != MEL_MODEL_HLDGN && w->conv2.lin_l.weight && w->conv2.lin_l.out_dim % GEMP_BN == 0 &&
           w->conv2.lin_l.in_dim % GEMS2_BK == 0 && w->conv2.lin_l.in_dim / GEMS2_BK >= 4;
}
template <class F>
static void for_each_conv2_block(const mel_weights* w, ProjWeights& pw, F f) {
    if (!conv2_blocks_fit(w)) return;
    f(w->conv2.lin_l, &pw.c2l_blk), f(w->conv2.lin_r, &pw.c2r_blk);
    if (w->conv2.kind == MEL_CONV_TRANSFORMER) f(w->conv2.lin_v, &pw.c2v_blk);
}
static size_t plane_elems(const mel_weights* w) {       // bf16 elements of all planes of a model (row-major + conv2's blocks)
    ProjWeights pw{};
    size_t total = 3 * projection_elems(w);
    for_each_conv2_block(w, pw, [&](const mel_linear& l, const float**) { total += 3 * ((lin_elems(l) + 7) & ~(size_t)7); });
    return total;
}

constexpr int HEAD_KSPLIT_MAX = 4;

static int head_hidden_width(const mel_mlp& m) {
    int w = 0;
    for (int i = 0; i + 1 < m.n_layers; ++i) w = w > m.layer[i].out_dim ? w : m.layer[i].out_dim;
    return w;
}

// What the functions below derive from the weights (validate() keeps its own arithmetic: it runs before these can be trusted)
struct NetShape {
    int K0, hidden; // widths of encoder layer 0 and of the encoder rows
    int hc;         // heads * channels: a conv's output row
    int srcw;       // a conv's source-side row: HL-DGN's lin_l | lin_r and a transformer conv's key | value lie side by side
    int latent;     // head input
    int bf, sp;     // bf16 feature path, MEL_PREC_F32_SPLIT
    bool tconv, hl;
};
static NetShape shape_of(const mel_weights* w) {
    NetShape z;
    z.K0 = w->encoder.layer[0].out_dim, z.hidden = w->encoder.layer[1].out_dim, z.hc = w->conv1.heads * w->conv1.channels;
    z.tconv = w->conv1.kind == MEL_CONV_TRANSFORMER, z.hl = w->model == MEL_MODEL_HLDGN;
    z.srcw = z.hl || z.tconv ? 2 * z.hc : z.hc, z.latent = w->q_head.layer[0].in_dim;
    z.bf = w->precision == MEL_PREC_BF16, z.sp = w->precision == MEL_PREC_F32_SPLIT;
    return z;
}

static FwdLayout carve(const mel_weights* w, const Dims& d, void* ws) {
    FwdLayout L{};
    Carver c(ws);
    const NetShape z = shape_of(w);
    const int hidden = z.hidden, hc = z.hc, srcw = z.srcw, latent = z.latent;
    const size_t M = (size_t)d.bs * d.n;
    const size_t R = (size_t)d.rows_cap;
    const size_t SW = (size_t)set_words(d.n);          // words per node set
    L.plan.adj = c.take<uint64_t>(M * SW);
    L.plan.live = c.take<uint64_t>(d.bs * SW);
    // node-feature table mode: the encoder / conv1-projection buffers must also hold the N * 40 table rows
    const size_t T = (size_t)d.n * FEATURE_TUPLES_PER_DEGREE;
    const size_t rows2 = (size_t)d.u2_cap > T ? (size_t)d.u2_cap : T, rows1 = (size_t)d.u1_cap > T ? (size_t)d.u1_cap : T;
    const size_t rowsM = M > T ? M : T;
    if (!z.hl) {
        L.plan.u1 = c.take<uint64_t>(d.bs * SW);
        L.plan.u2 = c.take<uint64_t>(d.bs * SW);
        L.plan.cnt = c.take<int32_t>(3 * d.bs);
        L.plan.offL = c.take<int32_t>(d.bs + 1);
        L.plan.off1 = c.take<int32_t>(d.bs + 1);
        L.plan.off2 = c.take<int32_t>(d.bs + 1);
        L.plan.nid2 = c.take<int32_t>(d.u2_cap);
        L.plan.arow1 = c.take<int32_t>(d.u1_cap);
        L.plan.dm1 = c.take<float>(d.u1_cap);
        L.plan.desc1 = c.take<char>((size_t)d.u1_cap * target_desc_bytes(d.n));
        L.plan.desc2 = c.take<char>(R * target_desc_bytes(d.n));
        L.plan.row_env = c.take<int32_t>(R);
        L.plan.row_agent = c.take<int32_t>(R);
        L.plan.arow_g = c.take<int32_t>(R);
        L.plan.dm_g = c.take<float>(R);
        L.h0 = c.take<float>(rows2 * hidden);
        L.xl1 = c.take<float>(rows2 * srcw);
        L.xr1 = c.take<float>(rows1 * hc);
        // (fp32 rows, or - conv2 on gemm_planes_kernel - three bf16 planes: 6 bytes per value)
        L.h1 = c.take<float>(((size_t)d.u1_cap * hc * 3 + 1) / 2);
        L.xl2 = c.take<float>((size_t)d.u1_cap * srcw);
        L.xr2 = c.take<float>(R * hc);
    } else {
        L.h0 = c.take<float>(rowsM * hidden);
        L.xl1 = c.take<float>(rowsM * srcw);
    }
    L.plan.fid = c.take<int32_t>(M);
    L.plan.fbad = c.take<int32_t>(d.bs);
    L.plan.fmeta = c.take<int32_t>(4);
    L.xcat = c.take<float>(R * latent);
    const int hw = head_hidden_width(w->q_head) + head_hidden_width(w->v_head);
    L.hq[0] = c.take<float>(R * (hw > 0 ? hw : 1));
    L.hq[1] = c.take<float>(R * (hw > 0 ? hw : 1));
    L.hpart = c.take<float>(hw > 0 ? (size_t)HEAD_KSPLIT_MAX * R * hw : 8);
    L.minmax = c.take<float>(64);
    L.wb_elems = (w->precision == MEL_PREC_BF16) ? projection_elems(w) : has_planes(w) ? plane_elems(w) : 0;
    if (w->prepared) L.wb_elems = 0;             // the caller holds the converted weights (mel_prepare_weights)
    L.wb = c.take<uint16_t>(L.wb_elems ? L.wb_elems : 8);
    // (taken last, and only for a wide encoder: every other shape keeps its layout)
    L.enc0 = encoder_fuses(w) ? nullptr
                              : c.take<float>((z.hl ? rowsM : rows2) * (size_t)z.K0);
    L.bytes = c.off;
    L.rows_cap = R;
    return L;
}

static mel_status validate(const mel_weights* w, int model, int64_t bs, int n, int obs_stride, bool index_col) {
    if (!w) return fail(MEL_ERR_INVALID_ARG, "weights pointer is null");
    if (w->model != model) return fail(MEL_ERR_INVALID_ARG, "weights are for model %d, entry point is for %d", w->model, model);
    if (bs <= 0 || bs > (1 << 24)) return fail(MEL_ERR_INVALID_ARG, "bs=%ld out of range", (long)bs);
    if (n < 1 || n > MEL_MAX_NODES) return fail(MEL_ERR_INVALID_ARG, "n_nodes=%d outside [1, %d]", n, MEL_MAX_NODES);
    if (w->in_dim < 1 || w->in_dim > 8) return fail(MEL_ERR_UNSUPPORTED, "in_dim=%d outside [1, 8]", w->in_dim);
    if (w->precision < MEL_PREC_F32 || w->precision > MEL_PREC_F32_AUTO) return fail(MEL_ERR_INVALID_ARG, "precision=%d", w->precision);
    const int expected = n * (w->in_dim + 3);
    if (index_col) {
        if (obs_stride - 1 != expected)      // networks/common.py:24-29
            return fail(MEL_ERR_SHAPE, "Expected %d feature cols for nodes, got %d", expected, obs_stride - 1);
    } else if (obs_stride < expected) {
        return fail(MEL_ERR_SHAPE, "Expected at least %d feature cols for nodes, got %d", expected, obs_stride);
    }
    if (w->encoder.n_layers != 2) return fail(MEL_ERR_UNSUPPORTED, "encoder must be a 2-layer MLP");
    const int hidden = w->encoder.layer[1].out_dim;
    if (w->encoder.layer[0].in_dim != w->in_dim || w->encoder.layer[1].in_dim != w->encoder.layer[0].out_dim)
        return fail(MEL_ERR_INVALID_ARG, "encoder layer shapes inconsistent");
    if (w->encoder.layer[0].out_dim > ENC_MAX_WIDTH)
        return fail(MEL_ERR_UNSUPPORTED, "encoder hidden width %d > %d", w->encoder.layer[0].out_dim, ENC_MAX_WIDTH);
    if (w->encoder.layer[0].out_dim % 32 || hidden % 64)
        return fail(MEL_ERR_UNSUPPORTED, "encoder widths must be multiples of 64 (got %d, %d)", w->encoder.layer[0].out_dim, hidden);
    const int hc = w->conv1.heads * w->conv1.channels;
    if (const HeadLanes hl = head_lanes(w->conv1.heads, w->conv1.channels); !hl.ok())
        return fail(MEL_ERR_UNSUPPORTED, "%d heads of %d channels: %s", w->conv1.heads, w->conv1.channels, hl.why);
    if (w->conv1.lin_l.in_dim != hidden || w->conv1.lin_l.out_dim != hc || w->conv1.lin_r.out_dim != hc)
        return fail(MEL_ERR_INVALID_ARG, "conv1 projection shapes inconsistent");
    const int want_kind = (model == MEL_MODEL_DGNR) ? MEL_CONV_TRANSFORMER : MEL_CONV_GATV2;
    if (w->conv1.kind != want_kind) return fail(MEL_ERR_INVALID_ARG, "conv1 kind %d does not fit model %d", w->conv1.kind, model);
    if (want_kind == MEL_CONV_GATV2 && (!w->conv1.att || !w->conv1.bias)) return fail(MEL_ERR_INVALID_ARG, "conv1 att/bias null");
    if (want_kind == MEL_CONV_TRANSFORMER && (w->conv1.lin_v.in_dim != hidden || w->conv1.lin_v.out_dim != hc))
        return fail(MEL_ERR_INVALID_ARG, "conv1 value projection shape inconsistent");
    int latent = hc;
    if (model != MEL_MODEL_HLDGN) {
        if (w->conv2.heads != w->conv1.heads || w->conv2.channels != w->conv1.channels || w->conv2.kind != want_kind ||
            w->conv2.lin_l.in_dim != hc || w->conv2.lin_l.out_dim != hc || w->conv2.lin_r.out_dim != hc)
            return fail(MEL_ERR_INVALID_ARG, "conv2 projection shapes inconsistent");
        if (want_kind == MEL_CONV_GATV2 && (!w->conv2.att || !w->conv2.bias)) return fail(MEL_ERR_INVALID_ARG, "conv2 att/bias null");
        if (want_kind == MEL_CONV_TRANSFORMER && (w->conv2.lin_v.in_dim != hc || w->conv2.lin_v.out_dim != hc))
            return fail(MEL_ERR_INVALID_ARG, "conv2 value projection shape inconsistent");
        latent = hidden + 2 * hc;                    // l_dgn.py:44, dgn_r.py:63
    }
    const mel_mlp* heads[2] = {&w->q_head, &w->v_head};
    for (int k = 0; k < (w->dueling ? 2 : 1); ++k) {
        const mel_mlp& m = *heads[k];
        if (m.n_layers < 1 || m.n_layers > MEL_MAX_HEAD_LAYERS) return fail(MEL_ERR_UNSUPPORTED, "dueling head depth %d", m.n_layers);
        if (m.layer[0].in_dim != latent) return fail(MEL_ERR_INVALID_ARG, "dueling head expects %d inputs, network produces %d", m.layer[0].in_dim, latent);
        for (int i = 0; i + 1 < m.n_layers; ++i)
            if (m.layer[i].out_dim % 64 || m.layer[i].in_dim % 32 || m.layer[i + 1].in_dim != m.layer[i].out_dim)
                return fail(MEL_ERR_UNSUPPORTED, "dueling hidden layer %d shape %dx%d unsupported", i, m.layer[i].out_dim, m.layer[i].in_dim);
    }
    if (w->dueling && w->q_head.n_layers != w->v_head.n_layers) return fail(MEL_ERR_UNSUPPORTED, "Q and V heads must have equal depth");
    if (w->q_head.layer[w->q_head.n_layers - 1].out_dim != w->n_actions || w->n_actions > 8 || w->n_actions < 1)
        return fail(MEL_ERR_UNSUPPORTED, "n_actions=%d outside [1, 8] or inconsistent", w->n_actions);
    if (w->dueling && w->v_head.layer[w->v_head.n_layers - 1].out_dim != 1) return fail(MEL_ERR_INVALID_ARG, "V head must end in 1 output");
    return MEL_OK;
}

// The projection weights as the GEMMs of this precision read them.  fp32: the nn.Parameter storages themselves.  bf16 /
// split: bf16 copies (planes) - taken from the caller's PREPARED buffer (mel_prepare_weights: converted once per weight
// version, nothing launched here) or, when mel_weights.prepared is null, converted into `dst` (the workspace) by one launch
// on every call, which keeps a caller that never prepares correct.  convert = false only lays the pointers out.
static mel_status resolve_projections(const mel_weights* w, uint16_t* dst, ProjWeights& pw, ProjWeights& alt, hipStream_t s,
                                      bool convert) {
    pw = ProjWeights{}, alt = ProjWeights{};
    if (w->precision == MEL_PREC_F32_SPLIT || w->precision == MEL_PREC_F32_AUTO) {
        // [rows][K / 16][3][16] bf16 planes of every projection weight; AUTO: beside the fp32 matrices themselves
        const bool both = w->precision == MEL_PREC_F32_AUTO;
        ProjWeights& planes = both ? alt : pw;
        if (both) {
            for_each_projection(w, pw, [&](const mel_linear& l, const float** slot) { *slot = l.weight; });
            pw.alt = &alt;
        }
        SplitBatch b{};
        size_t off = 0;
        int blocks = 0;
        bool bad = false;
        for_each_projection(w, planes, [&](const mel_linear& l, const float** slot) {
            const size_t cnt = lin_elems(l);
            if (!both && l.weight && split_keeps_fp32(w, l)) { *slot = l.weight; return; }     // (split_k: stays fp32)
            if (b.n >= CVT_MAX_SEG || cnt % 8 != 0 || l.in_dim % 32 != 0 || !l.weight) { bad = true; return; }
            b.src[b.n] = l.weight, b.dst[b.n] = dst + off, b.count[b.n] = (int)cnt, b.K[b.n] = l.in_dim, b.start[b.n] = blocks;
            b.rb[b.n] = 0;
            *slot = reinterpret_cast<const float*>(dst + off);
            blocks += (int)((cnt / 4 + 255) / 256);
            off += 3 * ((cnt + 7) & ~(size_t)7);
            ++b.n;
        });
        if (!bad)
            for_each_conv2_block(w, planes, [&](const mel_linear& l, const float** slot) {
                const size_t cnt = lin_elems(l);
                if (b.n >= CVT_MAX_SEG || !l.weight || l.out_dim % GEMP_BN) return;       // (the slot stays null: no planes kernel)
                b.src[b.n] = l.weight, b.dst[b.n] = dst + off, b.count[b.n] = (int)cnt, b.K[b.n] = l.in_dim, b.start[b.n] = blocks;
                b.rb[b.n] = GEMP_BN;
                *slot = reinterpret_cast<const float*>(dst + off);
                blocks += (int)((cnt / 4 + 255) / 256);
                off += 3 * ((cnt + 7) & ~(size_t)7);
                ++b.n;
            });
        if (bad && both) {                       // AUTO: shapes the split kernels cannot take simply stay on the exact-fp32 path
            alt = ProjWeights{}, pw.alt = nullptr;
            return MEL_OK;
        }
        if (bad) return fail(MEL_ERR_UNSUPPORTED, "split path: a projection weight is null or its shape is unsupported");
        if (!convert) return MEL_OK;
        b.start[b.n] = blocks;
        MEL_LAUNCH(split_weights_kernel, dim3(blocks), dim3(256), 0, s, b);
        return check_launch("weights -> bf16 planes");
    }
    if (w->precision != MEL_PREC_BF16) {
        for_each_projection(w, pw, [&](const mel_linear& l, const float** slot) { *slot = l.weight; });
        return MEL_OK;
    }
    CvtBatch b{};
    size_t off = 0;
    int blocks = 0;
    bool bad = false;
    for_each_projection(w, pw, [&](const mel_linear& l, const float** slot) {
        const size_t cnt = lin_elems(l);
        if (b.n >= CVT_MAX_SEG || cnt % 8 != 0 || !l.weight) { bad = true; return; }
        b.src[b.n] = l.weight, b.dst[b.n] = dst + off, b.count[b.n] = (int)cnt, b.start[b.n] = blocks;
        *slot = reinterpret_cast<const float*>(dst + off);
        blocks += (int)((cnt / 8 + 255) / 256);
        off += (cnt + 7) & ~(size_t)7;
        ++b.n;
    });
    if (bad) return fail(MEL_ERR_UNSUPPORTED, "bf16 path: a projection weight is null or its size is not a multiple of 8");
    if (!convert) return MEL_OK;
    b.start[b.n] = blocks;
    MEL_LAUNCH(cvt_bf16_kernel, dim3(blocks), dim3(256), 0, s, b);
    return check_launch("weights -> bf16");
}
static size_t prepared_elems(const mel_weights* w) {
    return w->precision == MEL_PREC_BF16 ? projection_elems(w) : has_planes(w) ? plane_elems(w) : 0;
}
static mel_status resolve_projections(const mel_weights* w, const FwdLayout& L, ProjWeights& pw, ProjWeights& alt, hipStream_t s) {
    if (w->prepared && w->precision != MEL_PREC_F32)
        return resolve_projections(w, static_cast<uint16_t*>(const_cast<void*>(w->prepared)), pw, alt, s, false);
    return resolve_projections(w, L.wb, pw, alt, s, true);
}

// dueling heads: hidden layers through the GEMM (Q | V stacked along n), last layer + combine in the tail.
// rows_dev (device row count) may be null.
static mel_status run_heads(const mel_weights* w, const ProjWeights& pw, const FwdLayout& L, int64_t rows,
                            const int32_t* rows_dev, long rows_hint, float* logits, hipStream_t s,
                            const mel_select* select = nullptr) {
    const int nl = w->q_head.n_layers;
    const int bf = shape_of(w).bf, sp = shape_of(w).sp;
    const float* in_q = L.xcat;
    const float* in_v = L.xcat;
    int ld_q = w->q_head.layer[0].in_dim, ld_v = ld_q;
    // The standard heads (hidden [128, 128] for Q and V, l_dgn.py:66-84 with the CLI defaults): the first layer's RAW
    // products go to fp32 planes (fp32 path: split-K, one plane per K chunk; bf16 / split paths: one plane), then
    // everything after them runs in ONE launch (head_finish_kernel: plane sum + bias + ReLU, hidden layer 1 in fp32 MFMA,
    // last layer, dueling combine, selection).
    if (nl == 3 && w->dueling && w->v_head.n_layers == 3) {
        const mel_linear& q = w->q_head.layer[0];
        const mel_linear& v = w->v_head.layer[0];
        const mel_linear& q1 = w->q_head.layer[1];
        const mel_linear& v1 = w->v_head.layer[1];
        if (q.in_dim == v.in_dim && q.out_dim == HF_W && v.out_dim == HF_W && q1.in_dim == HF_W &&
            q1.out_dim == HF_W && v1.in_dim == HF_W && v1.out_dim == HF_W && w->q_head.layer[2].out_dim <= HF_MAX_ACTIONS &&
            w->v_head.layer[2].out_dim == 1 && q1.weight && v1.weight) {
            const long ps = (long)L.rows_cap * 2 * HF_W;
            GemmArgs g;
            g.A = in_q, g.lda = ld_q, g.W = pw.q[0], g.W_hi = pw.v[0], g.split_n = q.out_dim;
            g.Y = L.hpart, g.ldy = 2 * HF_W, g.M = (int)rows, g.M_dev = rows_dev, g.N = 2 * HF_W, g.K = q.in_dim;
            g.bf16 = bf, g.split = sp, g.y_f32 = 1;
            if (pw.alt) g.Ws = pw.alt->q[0], g.Ws_hi = pw.alt->v[0];
            const long hint = rows_hint < 0 || rows_hint > rows ? rows : rows_hint;
            GemmRequest rq;     // split-K into L.hpart where the chunks fill the chip; head_finish_kernel sums the planes
            rq.max_ksplit = HEAD_KSPLIT_MAX, rq.parts = L.hpart, rq.part_stride = ps;
            const GemmPlan plan = plan_gemm(&g, &hint, 1, rq);
            const int S = plan.ksplit;
            {
                StageScope t(MEL_STAGE_HEAD_HIDDEN, s);
                if (mel_status st = launch_plan(plan, s, 3, S > 1 ? "head hidden (Q|V), split-K" : "head hidden (Q|V), raw")) return st;
            }
            StageScope t(MEL_STAGE_HEAD_TAIL, s);
            HeadFinish f{L.hpart, ps, S, (int)rows, rows_dev, q.bias, v.bias, q1, v1, w->q_head.layer[2], w->v_head.layer[2],
                         logits, select ? *select : mel_select{}, 0};
            // grid: twice the expected row count (the hint is a rough mean; a workgroup that has to loop doubles the
            // launch), surplus workgroups leave after one load
            // 16 rows per workgroup while that leaves at most one workgroup per CU, 32 beyond
            const int per = hint > 16 * 256 ? 32 : 16;
            const long need = (rows + per - 1) / per;
            const long likely = (hint + per - 1) / per;
            long blocks = rows_dev ? 2 * likely + 8 : need;
            blocks = blocks > need ? need : blocks < 1 ? 1 : blocks;
            f.likely_blocks = (int)(likely < blocks ? likely : blocks);
            if (per == 16) MEL_LAUNCH(head_finish_kernel<1>, dim3((int)blocks), dim3(512), 0, s, f);
            else MEL_LAUNCH(head_finish_kernel<2>, dim3((int)blocks), dim3(512), 0, s, f);
            return check_launch("head finish");
        }
    }
    for (int i = 0; i + 1 < nl; ++i) {
        StageScope t(MEL_STAGE_HEAD_HIDDEN, s);
        const mel_linear& q = w->q_head.layer[i];
        const mel_linear& v = w->v_head.layer[i];
        float* out = L.hq[i & 1];
        const int ldo = q.out_dim + v.out_dim;
        if (i == 0 && q.in_dim == v.in_dim) {       // shared input: one launch, weights split along n
            GemmArgs g;
            g.A = in_q, g.lda = ld_q;
            g.W = pw.q[i], g.W_hi = pw.v[i], g.bias = q.bias, g.bias_hi = v.bias, g.split_n = q.out_dim;
            g.Y = out, g.ldy = ldo, g.M = (int)rows, g.M_dev = rows_dev, g.N = ldo, g.K = q.in_dim, g.relu = 1;
            g.bf16 = bf, g.split = sp, g.y_f32 = (i + 2 == nl);       // the tail reads fp32
            // (the plane sum writes fp32: on the bf16 path only where the consumer reads fp32)
            GemmRequest rq;
            rq.max_ksplit = (bf && !g.y_f32) ? 1 : HEAD_KSPLIT_MAX, rq.parts = L.hpart, rq.part_stride = (long)L.rows_cap * ldo;
            const GemmPlan plan = plan_gemm(&g, &rows_hint, 1, rq);
            const char* what = plan.ksplit > 1 ? "head hidden (Q|V), split-K" : "head hidden (Q|V)";
            if (mel_status st = launch_plan(plan, s, 3, what)) return st;
            if (plan.ksplit > 1)
                if (mel_status st = launch_splitk_finish(g, plan, rows_hint, s, what)) return st;
        } else {
            GemmArgs g[2];
            // element offset of the V half inside a row: in elements of the buffer's type (bf16 halves the bytes)
            const bool in16 = bf, out32 = !bf || (i + 2 == nl);
            g[0].A = in_q, g[0].lda = ld_q, g[0].W = pw.q[i], g[0].bias = q.bias;
            g[0].Y = out, g[0].ldy = ldo, g[0].M = (int)rows, g[0].M_dev = rows_dev, g[0].N = q.out_dim, g[0].K = q.in_dim, g[0].relu = 1;
            g[1].A = in_v, g[1].lda = ld_v, g[1].W = pw.v[i], g[1].bias = v.bias;
            g[1].Y = out32 ? out + q.out_dim : reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(out) + q.out_dim);
            g[1].ldy = ldo, g[1].M = (int)rows, g[1].M_dev = rows_dev, g[1].N = v.out_dim, g[1].K = v.in_dim, g[1].relu = 1;
            g[0].bf16 = g[1].bf16 = bf, g[0].split = g[1].split = split_k(sp, q.in_dim < v.in_dim ? q.in_dim : v.in_dim), g[0].y_f32 = g[1].y_f32 = (bf && out32);
            (void)in16;
            const long hints[2] = {rows_hint, rows_hint};
            if (mel_status st = launch_gemm_group(g, hints, w->dueling ? 2 : 1, s, "Q + V hidden", 3)) return st;
        }
        const bool out16 = bf && !(i + 2 == nl);
        in_q = out, ld_q = ld_v = ldo;
        in_v = out16 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(out) + q.out_dim) : out + q.out_dim;
    }
    if (bf && nl < 2) return fail(MEL_ERR_UNSUPPORTED, "bf16 path needs at least one hidden layer in the heads");
    const mel_linear& ql = w->q_head.layer[nl - 1];
    const mel_linear& vl = w->v_head.layer[nl - 1];
    StageScope t(MEL_STAGE_HEAD_TAIL, s);
    MEL_LAUNCH(dueling_tail_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in_q, ld_q, ql.in_dim, in_v, ld_v,
                       vl.in_dim, ql, vl, (int)rows, rows_dev, w->dueling, logits, select ? *select : mel_select{});
    return check_launch("dueling tail");
}

// The node-feature table (plan_masks.hpp): encoder row of every feature tuple, then its conv1 projections - two launches
// into t_h0 [T, hidden], t_xl [T, srcw (HL-DGN: 2 hc, lin_l | lin_r)], t_xr [T, hc] (unused for HL-DGN).
struct FeatureTables {
    float* h0;
    float* xl;
    float* xr;
};
static size_t table_elem_bytes(const mel_weights* w) { return w->precision == MEL_PREC_BF16 ? 2 : 4; }
static FeatureTables carve_tables(const mel_weights* w, int n, void* buf, size_t* bytes) {
    const size_t T = (size_t)n * FEATURE_TUPLES_PER_DEGREE, es = table_elem_bytes(w);
    const NetShape z = shape_of(w);
    Carver c(buf);
    FeatureTables t;
    t.h0 = reinterpret_cast<float*>(c.take<char>(T * z.hidden * es));
    t.xl = reinterpret_cast<float*>(c.take<char>(T * z.srcw * es));
    t.xr = z.hl ? nullptr : reinterpret_cast<float*>(c.take<char>(T * z.hc * es));
    if (bytes) *bytes = c.off;
    return t;
}
// The shapes table_fused_tile is built for (gemm_table.hpp): GATv2 L-DGN on the exact-fp32 instruction - MEL_PREC_F32, and
// MEL_PREC_F32_AUTO, whose table launches are far too small for the split kernels.  Everything else (the bf16 feature path,
// MEL_PREC_F32_SPLIT, DGN-R's three source-side matrices, HL-DGN) keeps the two-launch form.
static bool table_fuses(const mel_weights* w) {
    const NetShape z = shape_of(w);
    return w->model == MEL_MODEL_LDGN && !z.tconv &&
           (w->precision == MEL_PREC_F32 || w->precision == MEL_PREC_F32_AUTO) && w->in_dim == 5 && w->encoder.n_layers == 2 &&
           z.K0 == TBL_HIDDEN && z.hidden == TBL_HIDDEN &&
           w->conv1.lin_l.in_dim == TBL_HIDDEN && z.hc % 32 == 0 && (2 * z.hc) % TBL_BN == 0;
}
static TableArgs fused_table_args(const mel_weights* w, const ProjWeights& pw, int n, const FeatureTables& t) {
    const int hc = shape_of(w).hc;
    TableArgs a;
    a.T = n * FEATURE_TUPLES_PER_DEGREE, a.in_dim = w->in_dim;
    a.enc_w = w->encoder.layer[0].weight, a.enc_b = w->encoder.layer[0].bias;
    a.W1 = pw.enc1, a.b1 = w->encoder.layer[1].bias;
    a.Wl = pw.c1l, a.Wr = pw.c1r, a.bl = w->conv1.lin_l.bias, a.br = w->conv1.lin_r.bias;
    a.split_n = hc, a.N = 2 * hc;
    a.h0 = t.h0, a.xl = t.xl, a.xr = t.xr;
    return a;
}

// The GEMM problems of the encoder and of conv1, each described ONCE: everything the weights and the precision decide.  The
// caller adds the rows (M, M_dev) and the gathers (nid, arow).
// The encoder, relu(W1 relu(W0 x + b0) + b1) into rows of Y (l_dgn.py:117-118): what its two problems share
static GemmArgs encoder_problem(const mel_weights* w, const NetShape& z, const float* W1, float* Y) {
    GemmArgs g;
    g.in_dim = w->in_dim, g.enc_w = w->encoder.layer[0].weight, g.enc_b = w->encoder.layer[0].bias;
    g.W = W1, g.bias = w->encoder.layer[1].bias, g.split = split_k(z.sp, z.K0);
    g.Y = Y, g.ldy = z.hidden, g.N = z.hidden, g.K = z.K0, g.relu = 1;
    return g;
}
// ... on observation rows: L-DGN's U2 rows (the caller sets nid) and every node of HL-DGN
static GemmArgs encoder_on_rows(const mel_weights* w, const ProjWeights& pw, const NetShape& z, const float* obs, int obs_stride,
                                int n, float* Y) {
    GemmArgs g = encoder_problem(w, z, pw.enc1, Y);
    g.obs = obs, g.obs_width = obs_stride, g.n_nodes = n, g.node_cols = w->in_dim + 3, g.bf16 = z.bf;
    return g;
}
// ... on the n * 40 feature tuples of the node-feature table.  bf16 feature path: the exact-fp32 tile on the fp32 weights, its
// rows stored as bf16, as a launch of its own and beside the plan - so prepared and per-call tables are identical
static GemmArgs encoder_on_tuples(const mel_weights* w, const ProjWeights& pw, const NetShape& z, int n, float* Y) {
    GemmArgs g = encoder_problem(w, z, z.bf ? w->encoder.layer[1].weight : pw.enc1, Y);
    g.feat_domain = 1, g.y_bf16 = z.bf, g.M = n * FEATURE_TUPLES_PER_DEGREE;
    return g;
}
// ... as the 64 x 64 tiles of gemm_f32_kernel, one workgroup each: the first enc.grid workgroups of plan_enc_kernel / fid_enc_kernel
static mel_status plan_encoder_beside_plan(const mel_weights* w, const ProjWeights& pw, const NetShape& z, int n, float* Y, GemmPlan& enc) {
    const GemmArgs g = encoder_on_tuples(w, pw, z, n, Y);
    GemmRequest rq;
    rq.mode = GEMM_MODE_ENC, rq.force_tile = MEL_TILE_64;
    enc = plan_gemm(&g, nullptr, 1, rq);
    return enc.status ? fail(enc.status, "encoder (feature tuples): %s", enc.why) : MEL_OK;
}
// conv1 of L-DGN / DGN-R on rows of t.h0: g[0] = lin_l for the sources (DGN-R: key | value in one problem, the weights split
// along n) into t.xl, g[1] = lin_r for the targets into t.xr
static void conv1_pair(const mel_weights* w, const ProjWeights& pw, const NetShape& z, const FeatureTables& t, GemmArgs g[2]) {
    g[0].bf16 = g[1].bf16 = z.bf, g[0].split = g[1].split = split_k(z.sp, z.hidden);
    g[0].A = t.h0, g[0].lda = z.hidden, g[0].W = pw.c1l, g[0].bias = w->conv1.lin_l.bias;
    g[0].Y = t.xl, g[0].ldy = z.srcw, g[0].N = z.srcw, g[0].K = z.hidden;
    if (z.tconv) g[0].W_hi = pw.c1v, g[0].bias_hi = w->conv1.lin_v.bias, g[0].split_n = z.hc;
    g[1].A = t.h0, g[1].lda = z.hidden, g[1].W = pw.c1r, g[1].bias = w->conv1.lin_r.bias;
    g[1].Y = t.xr, g[1].ldy = z.hc, g[1].N = z.hc, g[1].K = z.hidden;
}
// conv1 of HL-DGN: x_l | x_r of every row of t.h0 in one GEMM (weights split along n) into t.xl
static GemmArgs conv1_hl(const mel_weights* w, const ProjWeights& pw, const NetShape& z, const FeatureTables& t) {
    GemmArgs g;
    g.A = t.h0, g.lda = z.hidden, g.W = pw.c1l, g.W_hi = pw.c1r, g.bf16 = z.bf, g.split = split_k(z.sp, z.hidden);
    g.bias = w->conv1.lin_l.bias, g.bias_hi = w->conv1.lin_r.bias, g.split_n = z.hc;
    g.Y = t.xl, g.ldy = z.srcw, g.N = z.srcw, g.K = z.hidden;
    return g;
}

// A forward of env observations (integer features) takes the node-feature table (plan_masks.hpp) when it expects `rows` rows
// in its lists, much more than the n * 40 tuples ...
static bool takes_table(const mel_weights* w, int n, long rows) {
    return (w->flags & MEL_FWD_INTEGER_FEATURES) && w->in_dim == 5 && rows >= 2L * n * FEATURE_TUPLES_PER_DEGREE;
}
// ... the one the caller prepared for these weights and this n (mel_prepare_feature_tables) ...
static bool tables_prepared(const mel_weights* w, int n) { return w->tables && w->tables_nodes == n; }
// ... or its own, whose encoder rows ride in the plan launch: they and the row lists (HL-DGN: the tuple ids) are independent,
// ONE launch runs both instead of two latency-bound ones back to back (the bf16 ENC launch of 2 000 tuples alone took 15 us)
static bool encoder_rides_in_plan(const mel_weights* w, const NetShape& z, int n, bool table) {
    return table && !z.sp && !tables_prepared(w, n) && encoder_fuses(w);
}

static mel_status run_feature_tables(const mel_weights* w, const ProjWeights& pw, int n, const FeatureTables& t, hipStream_t s,
                                     bool encoder_done = false, float* enc0 = nullptr) {
    const int T = n * FEATURE_TUPLES_PER_DEGREE;
    const NetShape z = shape_of(w);
    if (!encoder_done) {
        const GemmArgs g = encoder_on_tuples(w, pw, z, n, t.h0);
        // a wide encoder without scratch of the caller's (the prepared tables): its layer-0 rows pass through t.xl, which the
        // projections below write only after the encoder has read them - where they fit
        if (!enc0 && !encoder_fuses(w)) {
            if ((size_t)z.srcw * table_elem_bytes(w) < (size_t)g.K * 4)
                return fail(MEL_ERR_UNSUPPORTED, "feature tables: an encoder %d wide needs rows of %d bytes, the table's are narrower", g.K, g.K * 4);
            enc0 = t.xl;
        }
        if (mel_status st = launch_encoder(g, enc0, s, "encoder (feature tuples)", T)) return st;
    }
    StageScope sc(MEL_STAGE_CONV1_LIN, s);
    if (z.hl) {
        GemmArgs g = conv1_hl(w, pw, z, t);
        g.M = T;
        return launch_gemm(g, GEMM_MODE_PLAIN, s, "conv1.lin_l|lin_r (feature tuples)");
    }
    GemmArgs g[2];
    conv1_pair(w, pw, z, t, g);
    g[0].M = g[1].M = T;
    const long hints[2] = {T, T};
    return launch_gemm_group(g, hints, 2, s, "conv1.lin_l + lin_r (feature tuples)", 1);
}

// L-DGN for a set of controlling agents per env (agent_mask == null: the index column names one)
static mel_status ldgn_forward_impl(const mel_weights* w, const float* obs, const Dims& d, int obs_stride,
                                    const uint64_t* agent_mask, float* logits, int32_t* row_offsets_out,
                                    const mel_select* select, void* workspace, size_t ws_bytes, hipStream_t s) {
    if (!obs || !logits || !workspace) return fail(MEL_ERR_INVALID_ARG, "null obs/logits/workspace");
    const FwdLayout L = carve(w, d, workspace);
    if (ws_bytes < L.bytes) return fail(MEL_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.bytes);
    clear_stale_error();
    const int64_t bs = d.bs;
    const int n = d.n;
    const int node_cols = w->in_dim + 3;
    const NetShape z = shape_of(w);
    const int R = (int)d.rows_cap, U1 = (int)d.u1_cap, U2 = (int)d.u2_cap;
    const int32_t* nL = L.plan.offL + bs;
    const int32_t* n1 = L.plan.off1 + bs;
    const int32_t* n2 = L.plan.off2 + bs;
    // expected sizes of the ragged row lists, for tile selection only.  Measured means on r = 0.2 disc graphs
    // (N = 50): one agent per row: |U1| ~ 0.13 N, |U2| ~ 0.25 N; a whole round (about 0.1 N active agents
    // with overlapping neighbourhoods): |U1| ~ 0.21 N, |U2| ~ 0.32 N.
    const bool single = agent_mask == nullptr;
    ProjWeights pw, pw_alt;
    if (mel_status st = resolve_projections(w, L, pw, pw_alt, s)) return st;
    // round-batched loop, measured on the bench workload (per env, N = 20 / 50): |L| = 3.1 / 4.7, |U1| = 5.8 / 10.4,
    // |U2| = 7.6 / 15.8 - linear fits below
    const long hintL = single ? bs : (n < 10 ? bs : bs * (long)(36 + n) / 18);
    const long hint1 = single ? bs * (long)(n < 8 ? n : 2 + n / 8) : (n < 10 ? bs * (long)n : bs * 2L * (18 + n) / 13);
    const long hint2 = single ? bs * (long)(n < 8 ? n : 1 + n / 4) : (n < 10 ? bs * (long)n : bs * 3L * (8 + n) / 11);
    const int T = n * FEATURE_TUPLES_PER_DEGREE;
    const bool table = takes_table(w, n, hint1 + hint2);
    // (where table_fused_tile fits, the plan launch's workgroups run conv1's projections of their encoder rows too: the whole table)
    const bool fused_enc = encoder_rides_in_plan(w, z, n, table);
    const bool fused_table = fused_enc && table_fuses(w) && !gemm_tuning().no_fused_table;
    // the encoder / conv1-projection rows the conv1 attention reads: the workspace's, unless the caller prepared tables
    FeatureTables ft{L.h0, L.xl1, L.xr1};
    if (table && tables_prepared(w, n)) ft = carve_tables(w, n, const_cast<void*>(w->tables), nullptr);
    // conv2's projections, planned HERE: on gemm_planes_kernel (both operands as bf16 planes in blocks, gemm_split.hpp) the
    // conv1 attention stores h1 already split, as that kernel's A operand.  (h1 rows are masked by the decision-maker flag,
    // l_dgn.py:128: the conv1 attention applies it as it stores them.)
    GemmArgs c2[2];
    c2[0].bf16 = c2[1].bf16 = z.bf, c2[0].split = c2[1].split = z.sp;
    c2[0].A = L.h1, c2[0].lda = z.hc;
    c2[0].W = pw.c2l, c2[0].bias = w->conv2.lin_l.bias;
    c2[0].Y = L.xl2, c2[0].ldy = z.srcw, c2[0].M = U1, c2[0].M_dev = n1, c2[0].N = z.srcw, c2[0].K = z.hc;
    if (z.tconv) c2[0].W_hi = pw.c2v, c2[0].bias_hi = w->conv2.lin_v.bias, c2[0].split_n = z.hc;
    c2[1].A = L.h1, c2[1].lda = z.hc, c2[1].arow = L.plan.arow_g;
    c2[1].W = pw.c2r, c2[1].bias = w->conv2.lin_r.bias;
    if (pw.alt) c2[0].Ws = pw.alt->c2l, c2[0].Ws_hi = z.tconv ? pw.alt->c2v : nullptr, c2[1].Ws = pw.alt->c2r;
    c2[1].Y = L.xr2, c2[1].ldy = z.hc, c2[1].M = R, c2[1].M_dev = nL, c2[1].N = z.hc, c2[1].K = z.hc;
    const long c2_hints[2] = {hint1, hintL};
    const ProjWeights* planes = z.sp ? &pw : pw.alt;
    GemmRequest c2_rq;
    c2_rq.group = true;
    PlaneBlocks c2_blocks[2];
    // (the forms of h1 the conv1 attention can store as planes: 4+ channels per lane on a full wavefront - rows of 6 heads,
    //  384 or 768 wide, stay fp32 rows, so the planner is never offered the plane blocks for them)
    const HeadLanes hl1 = head_lanes(w->conv1.heads, w->conv1.channels);
    if (planes && hl1.live == 64 && hl1.vpl >= 4) {
        c2_blocks[0] = {planes->c2l_blk, z.tconv ? planes->c2v_blk : nullptr}, c2_blocks[1] = {planes->c2r_blk, nullptr};
        c2_rq.blocks = c2_blocks;
    }
    const GemmPlan conv2 = plan_gemm(c2, c2_hints, 2, c2_rq);

    {
        StageScope t(MEL_STAGE_PLAN, s);
        if (w->flags & MEL_FWD_PLAN_READY) {       // mel_env_round's plan sink wrote the masks of this call
            if (!agent_mask) return fail(MEL_ERR_INVALID_ARG, "MEL_FWD_PLAN_READY needs the agent-set entry points");
        } else {
            if (n > 64) MEL_LAUNCH(plan_masks_kernel<2>, dim3((bs + 3) / 4), dim3(256), 0, s, obs, (int)bs, n, obs_stride, node_cols, agent_mask, L.plan, 1);
            else MEL_LAUNCH(plan_masks_kernel<1>, dim3((bs + 3) / 4), dim3(256), 0, s, obs, (int)bs, n, obs_stride, node_cols, agent_mask, L.plan, 1);
            if (mel_status st = check_launch("plan_masks")) return st;
        }
        const int inline_scan = bs <= 8192;           // beyond that the per-wave re-scan (O(bs^2 / 64) loads) loses
        if (!inline_scan) {
            MEL_LAUNCH(plan_scan_kernel, dim3(1), dim3(1024), 0, s, (int)bs, L.plan);
            if (mel_status st = check_launch("plan_scan")) return st;
        }
        const PlanListsArgs pa{obs, (int)bs, n, obs_stride, node_cols, L.plan, row_offsets_out, z.tconv ? 0 : 1, inline_scan, table ? T : 0};
        if (fused_table) {
            const TableArgs ta = fused_table_args(w, pw, n, ft);
            const int tiles = table_items(ta);
            if (n > 64) MEL_LAUNCH((plan_enc_kernel<2, true>), dim3(tiles + (int)((bs + 3) / 4)), dim3(256), 0, s, pa, ta, tiles);
            else MEL_LAUNCH((plan_enc_kernel<1, true>), dim3(tiles + (int)((bs + 3) / 4)), dim3(256), 0, s, pa, ta, tiles);
        } else if (fused_enc) {
            GemmPlan enc;
            if (mel_status st = plan_encoder_beside_plan(w, pw, z, n, L.h0, enc)) return st;
            if (n > 64) MEL_LAUNCH(plan_enc_kernel<2>, dim3(enc.grid + (int)((bs + 3) / 4)), dim3(256), 0, s, pa, enc.batch, enc.grid);
            else MEL_LAUNCH(plan_enc_kernel<1>, dim3(enc.grid + (int)((bs + 3) / 4)), dim3(256), 0, s, pa, enc.batch, enc.grid);
        } else {
            with_words(n, [&](auto w) { MEL_LAUNCH(plan_lists_kernel<decltype(w)::value>, dim3((bs + 3) / 4), dim3(256), 0, s, pa); });
        }
        if (mel_status st = check_launch("plan_lists")) return st;
    }
    if (!table) {       // encoder on the U2 rows, then conv1.lin_l on the U2 rows + lin_r on the U1 rows in one grouped launch
        GemmArgs e = encoder_on_rows(w, pw, z, obs, obs_stride, n, L.h0), g[2];
        e.nid = L.plan.nid2, e.M = U2, e.M_dev = n2;
        conv1_pair(w, pw, z, ft, g);
        g[0].M = U2, g[0].M_dev = n2, g[1].arow = L.plan.arow1, g[1].M = U1, g[1].M_dev = n1;
        const long hints[2] = {hint2, hint1};
        if (mel_status st = launch_encoder(e, L.enc0, s, "encoder", hint2)) return st;
        StageScope t(MEL_STAGE_CONV1_LIN, s);
        if (mel_status st = launch_gemm_group(g, hints, 2, s, "conv1.lin_l + lin_r", 1)) return st;
    } else if (!tables_prepared(w, n) && !fused_table) {        // (else the caller prepared the table, or the plan launch made all of it)
        if (mel_status st = run_feature_tables(w, pw, n, ft, s, /*encoder_done=*/fused_enc, L.enc0)) return st;
    }
    {   // conv1 attention for the U1 targets; also drops x_1 and x_2 of every agent into the head input
        AttArgs a{};
        a.xl = ft.xl, a.ld_l = z.srcw, a.xr = ft.xr, a.ld_r = z.hc, a.att = w->conv1.att, a.bias = w->conv1.bias;
        a.kind = w->conv1.kind, a.score_scale = 1.0f / sqrtf((float)w->conv1.channels), a.bf16 = z.bf;
        a.adj = L.plan.adj, a.bs = (int)bs, a.n = n;
        a.desc = L.plan.desc1, a.rows_dev = n1, a.rows_cap = U1, a.rows_hint = hint1;
        a.out = L.h1, a.ldo = z.hc, a.xcat = L.xcat, a.ld_cat = z.latent, a.hidden = z.hidden, a.h0 = ft.h0;
        if (conv2.kernel == GemmKernel::PLANES) a.out_planes = reinterpret_cast<uint16_t*>(L.h1);
        a.out_scale = L.plan.dm1;       // the decision-maker mask (l_dgn.py:128) is applied as h1 is stored; x_2 is taken before it
        a.fid = table ? L.plan.fid : nullptr;
        StageScope t(MEL_STAGE_CONV1_ATT, s);
        if (mel_status st = launch_attend<ATT_ROWS>(a, head_lanes(w->conv1.heads, w->conv1.channels), s, "conv1 attention")) return st;
    }
    {   // conv2.lin_l on the U1 rows + conv2.lin_r on the agent rows, one grouped launch
        StageScope t(MEL_STAGE_CONV2_LIN, s);
        if (mel_status st = launch_plan(conv2, s, 2, "conv2.lin_l + lin_r")) return st;
    }
    {   // conv2 attention, one target per agent row -> x_3
        AttArgs a{};
        a.xl = L.xl2, a.ld_l = z.srcw, a.xr = L.xr2, a.ld_r = z.hc, a.att = w->conv2.att, a.bias = w->conv2.bias;
        a.kind = w->conv2.kind, a.score_scale = 1.0f / sqrtf((float)w->conv2.channels), a.bf16 = z.bf;
        a.adj = L.plan.adj;
        a.bs = (int)bs, a.n = n;
        a.desc = L.plan.desc2, a.rows_dev = nL, a.rows_cap = R, a.rows_hint = hintL;
        a.xcat = L.xcat, a.ld_cat = z.latent, a.cat_off = z.hidden + z.hc;
        StageScope t(MEL_STAGE_CONV2_ATT, s);
        if (mel_status st = launch_attend<ATT_SINGLE>(a, head_lanes(w->conv2.heads, w->conv2.channels), s, "conv2 attention")) return st;
    }
    return run_heads(w, pw, L, R, nL, hintL, logits, s, select);
}

// the entry points of the two-convolution networks: `model` is MEL_MODEL_LDGN or MEL_MODEL_DGNR
static mel_status two_conv_forward(int model, const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_width,
                                   float* logits, void* workspace, size_t ws_bytes, void* stream) {
    if (mel_status st = validate(w, model, bs, n, obs_width, true)) return st;
    return ldgn_forward_impl(w, obs, make_dims(bs, n, bs, true), obs_width, nullptr, logits, nullptr, nullptr,
                             workspace, ws_bytes, static_cast<hipStream_t>(stream));
}
static mel_status two_conv_forward_agents(int model, const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_stride,
                                          const uint64_t* agent_mask, int64_t rows_cap, float* logits, int32_t* row_offsets, const mel_select* select,
                                          void* workspace, size_t ws_bytes, void* stream) {
    if (mel_status st = validate(w, model, bs, n, obs_stride, false)) return st;
    if (!agent_mask) return fail(MEL_ERR_INVALID_ARG, "agent_mask is null");
    if (rows_cap < 1 || rows_cap > bs * (int64_t)n) return fail(MEL_ERR_INVALID_ARG, "rows_cap=%ld outside [1, bs*n]", (long)rows_cap);
    if (select && !select->act) return fail(MEL_ERR_INVALID_ARG, "select->act is null");
    return ldgn_forward_impl(w, obs, make_dims(bs, n, rows_cap, false), obs_stride, agent_mask, logits, row_offsets,
                             select, workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

// mel_prepare_feature_tables and mel_feature_tables_fused (`one_launch`): the table into the caller's buffer
static mel_status feature_tables_entry(const mel_weights* w, int32_t n_nodes, void* tables, size_t bytes, bool one_launch, hipStream_t s) {
    if (mel_status st = validate(w, w ? w->model : 0, 1, n_nodes, n_nodes * ((w ? w->in_dim : 5) + 3), false)) return st;
    if (one_launch && !table_fuses(w))
        return fail(MEL_ERR_UNSUPPORTED, "the one-launch table is built for GATv2 L-DGN at f32 / f32-auto precision, hidden = %d", TBL_HIDDEN);
    if (!one_launch && w->in_dim != 5) return fail(MEL_ERR_UNSUPPORTED, "the node-feature table is defined for the 5 GraphEnv features");
    const size_t need = mel_feature_tables_bytes(w, n_nodes);
    if (!tables || bytes < need) return fail(MEL_ERR_WORKSPACE, "feature-table buffer %zu < %zu bytes", bytes, need);
    if (w->precision != MEL_PREC_F32 && !w->prepared)
        return fail(MEL_ERR_INVALID_ARG, "bf16 / split precision: prepare the weights first (mel_prepare_weights)");
    clear_stale_error();
    ProjWeights pw, pw_alt;
    if (mel_status st = resolve_projections(w, FwdLayout{}, pw, pw_alt, s)) return st;
    const FeatureTables t = carve_tables(w, n_nodes, tables, nullptr);
    if (!one_launch) return run_feature_tables(w, pw, n_nodes, t, s);
    const TableArgs ta = fused_table_args(w, pw, n_nodes, t);
    MEL_LAUNCH(table_fused_kernel, dim3(table_items(ta)), dim3(256), 0, s, ta);
    return check_launch("feature tables, one launch");
}

}  // namespace mel

using namespace mel;

extern "C" {

const char* mel_last_error(void) { return g_err; }
// Tuning aid (kprof.hpp, tools/kprof.py): read and zero the in-kernel cycle counters of one KprofFamily.  Returns the family's
// slot count (at most `cap` slots are copied), 0 if this build does not instrument it (-DMEL_*_PROF), -1 if there is no such family.
int32_t mel_debug_prof_read(int32_t family, unsigned long long* out, int32_t cap) {
    switch (family) {
        case KPROF_WORLD:
        case KPROF_ENV: return kprof_read_env(family, out, cap);
        case KPROF_GEMM: return kprof_read(GEMM_PROF_TAG >= 0 || SPLIT_PROF, g_gemm_prof, out, cap);
        case KPROF_SPLIT: return kprof_read(SPLIT_PROF, g_split_prof, out, cap);
        case KPROF_RING: return kprof_read(RING_PROF_TAG >= 0, g_ring_prof, out, cap);
        case KPROF_TABLE: return kprof_read(TABLE_PROF, g_table_prof, out, cap);
        case KPROF_ATT: return kprof_read(ATT_PROF_MODE >= 0, g_att_prof, out, cap);
        case KPROF_FIN: return kprof_read(FIN_PROF, g_fin_prof, out, cap);
    }
    return -1;
}
size_t mel_abi_sizeof(int32_t which) {
    switch (which) {
        case 0: return sizeof(mel_linear);
        case 1: return sizeof(mel_gatv2);
        case 2: return sizeof(mel_mlp);
        case 3: return sizeof(mel_weights);
        case 4: return sizeof(mel_select);
        case 5: return sizeof(mel_env_batch);
        case 6: return sizeof(mel_episode_pool);
        case 7: return sizeof(mel_env_obs);
        case 8: return sizeof(mel_round_replay);
        case 9: return sizeof(mel_graph_pool);
        case 10: return sizeof(mel_episode_stream);
        case 11: return sizeof(mel_replay_batch);
        case 12: return sizeof(mel_adam_tensors);
        case 13: return sizeof(mel_replay_priority);
        case 14: return sizeof(mel_train_log);
        case 15: return sizeof(mel_round_record);
        case 16: return sizeof(mel_decision_record);
        case 17: return sizeof(mel_attention_record);
        default: return 0;
    }
}
const char* mel_version(void) { return "melissa_hip 0.6 (gfx950)"; }

size_t mel_prepared_weights_bytes(const mel_weights* w) {
    if (!w || w->precision < MEL_PREC_F32 || w->precision > MEL_PREC_F32_AUTO) return 0;
    return prepared_elems(w) * sizeof(uint16_t);
}

size_t mel_feature_tables_bytes(const mel_weights* w, int32_t n_nodes) {
    if (!w || n_nodes < 1 || n_nodes > MEL_MAX_NODES || w->in_dim != 5 || w->encoder.n_layers != 2) return 0;
    size_t bytes = 0;
    (void)carve_tables(w, n_nodes, nullptr, &bytes);
    return bytes;
}

mel_status mel_prepare_feature_tables(const mel_weights* w, int32_t n_nodes, void* tables, size_t bytes, void* stream) {
    return feature_tables_entry(w, n_nodes, tables, bytes, false, static_cast<hipStream_t>(stream));
}

mel_status mel_feature_tables_fused(const mel_weights* w, int32_t n_nodes, void* tables, size_t bytes, void* stream) {
    return feature_tables_entry(w, n_nodes, tables, bytes, true, static_cast<hipStream_t>(stream));
}

mel_status mel_prepare_weights(const mel_weights* w, void* prepared, size_t bytes, void* stream) {
    if (!w) return fail(MEL_ERR_INVALID_ARG, "weights pointer is null");
    if (w->precision == MEL_PREC_F32) return MEL_OK;                 // the fp32 path reads the parameters themselves
    if (w->precision != MEL_PREC_BF16 && !has_planes(w)) return fail(MEL_ERR_INVALID_ARG, "precision=%d", w->precision);
    const size_t need = prepared_elems(w) * sizeof(uint16_t);
    if (!prepared || bytes < need) return fail(MEL_ERR_WORKSPACE, "prepared-weights buffer %zu < %zu bytes", bytes, need);
    clear_stale_error();
    ProjWeights pw, pw_alt;
    return resolve_projections(w, static_cast<uint16_t*>(prepared), pw, pw_alt, static_cast<hipStream_t>(stream), true);
}

size_t mel_workspace_bytes(const mel_weights* w, int64_t bs, int32_t n_nodes) {
    if (!w || bs <= 0 || n_nodes < 1 || n_nodes > MEL_MAX_NODES) return 0;
    return carve(w, make_dims(bs, n_nodes, bs, true), nullptr).bytes;
}

size_t mel_workspace_bytes_agents(const mel_weights* w, int64_t bs, int32_t n_nodes, int64_t rows_cap) {
    if (!w || bs <= 0 || n_nodes < 1 || n_nodes > MEL_MAX_NODES || rows_cap < 1) return 0;
    return carve(w, make_dims(bs, n_nodes, rows_cap, false), nullptr).bytes;
}

mel_status mel_ldgn_forward(const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_width,
                            float* logits, void* workspace, size_t ws_bytes, void* stream) {
    return two_conv_forward(MEL_MODEL_LDGN, w, obs, bs, n, obs_width, logits, workspace, ws_bytes, stream);
}

mel_status mel_ldgn_forward_agents(const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_stride,
                                   const uint64_t* agent_mask, int64_t rows_cap, float* logits,
                                   int32_t* row_offsets, const mel_select* select, void* workspace,
                                   size_t ws_bytes, void* stream) {
    return two_conv_forward_agents(MEL_MODEL_LDGN, w, obs, bs, n, obs_stride, agent_mask, rows_cap, logits, row_offsets, select, workspace, ws_bytes, stream);
}

mel_status mel_dgnr_forward(const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_width,
                            float* logits, void* workspace, size_t ws_bytes, void* stream) {
    return two_conv_forward(MEL_MODEL_DGNR, w, obs, bs, n, obs_width, logits, workspace, ws_bytes, stream);
}

mel_status mel_dgnr_forward_agents(const mel_weights* w, const float* obs, int64_t bs, int32_t n, int32_t obs_stride,
                                   const uint64_t* agent_mask, int64_t rows_cap, float* logits,
                                   int32_t* row_offsets, const mel_select* select, void* workspace,
                                   size_t ws_bytes, void* stream) {
    return two_conv_forward_agents(MEL_MODEL_DGNR, w, obs, bs, n, obs_stride, agent_mask, rows_cap, logits, row_offsets, select, workspace, ws_bytes, stream);
}

static mel_status hldgn_forward_impl(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs, int32_t n,
                                     int32_t obs_width, bool index_col, float* logits, void* workspace,
                                     size_t ws_bytes, void* stream, const mel_select* select = nullptr) {
    if (mel_status st = validate(w, MEL_MODEL_HLDGN, bs, n, obs_width, index_col)) return st;
    if (aggregator < MEL_AGG_MAX || aggregator > MEL_AGG_ADD) return fail(MEL_ERR_INVALID_ARG, "aggregator %d", aggregator);
    if (!obs || !logits || !workspace) return fail(MEL_ERR_INVALID_ARG, "null obs/logits/workspace");
    const Dims d = make_dims(bs, n, bs, true);
    const FwdLayout L = carve(w, d, workspace);
    if (ws_bytes < L.bytes) return fail(MEL_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    clear_stale_error();
    const int node_cols = w->in_dim + 3;
    const NetShape z = shape_of(w);
    const int hc = z.hc, bf = z.bf, M = (int)(bs * n);
    ProjWeights pw, pw_alt;
    if (mel_status st = resolve_projections(w, L, pw, pw_alt, s)) return st;
    const int T = n * FEATURE_TUPLES_PER_DEGREE;
    const bool table = takes_table(w, n, M);           // (every node is a row here)
    const bool fused_enc = encoder_rides_in_plan(w, z, n, table);
    FeatureTables ft{L.h0, L.xl1, nullptr};            // (the workspace's rows, unless the caller prepared tables)
    if (table && tables_prepared(w, n)) ft = carve_tables(w, n, const_cast<void*>(w->tables), nullptr);

    {
        StageScope t(MEL_STAGE_PLAN, s);
        // hl_dgn.py:108 pools over the whole graph: the controlling index is read (and clamped) but unused
        if (!((w->flags & MEL_FWD_PLAN_READY) && !index_col)) {      // (else: written by mel_env_round's plan sink)
            with_words(n, [&](auto w) {
                MEL_LAUNCH(plan_masks_kernel<decltype(w)::value>, dim3((bs + 3) / 4), dim3(256), 0, s, obs, (int)bs, n, obs_width, node_cols,
                           (const uint64_t*)nullptr, L.plan, index_col ? 0 : -1);
            });
            if (mel_status st = check_launch("plan_masks")) return st;
        }
        if (fused_enc) {
            GemmPlan enc;
            if (mel_status st = plan_encoder_beside_plan(w, pw, z, n, L.h0, enc)) return st;
            MEL_LAUNCH(fid_enc_kernel, dim3(enc.grid + (int)((bs + 3) / 4)), dim3(256), 0, s, obs, (int)bs, n, obs_width, node_cols, L.plan, T,
                       enc.batch, enc.grid);
        } else {
            MEL_LAUNCH(feature_ids_kernel, dim3((bs + 3) / 4), dim3(256), 0, s, obs, (int)bs, n, obs_width, node_cols, L.plan,
                       table ? T : 0);
        }
        if (mel_status st = check_launch("feature_ids")) return st;
    }
    if (!table) {       // encoder, then x_l | x_r, on every node
        GemmArgs e = encoder_on_rows(w, pw, z, obs, obs_width, n, L.h0), g = conv1_hl(w, pw, z, ft);
        e.M = g.M = M;
        if (mel_status st = launch_encoder(e, L.enc0, s, "encoder")) return st;
        StageScope t(MEL_STAGE_CONV1_LIN, s);
        if (mel_status st = launch_gemm(g, GEMM_MODE_PLAIN, s, "conv1.lin_l|lin_r")) return st;
    } else if (!tables_prepared(w, n)) {
        if (mel_status st = run_feature_tables(w, pw, n, ft, s, /*encoder_done=*/fused_enc, L.enc0)) return st;
    }
    {
        AttArgs a{};
        a.xl = ft.xl, a.ld_l = 2 * hc, a.ld_r = 2 * hc, a.bf16 = bf;
        a.xr = bf ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(ft.xl) + hc) : ft.xl + hc;
        a.att = w->conv1.att, a.bias = w->conv1.bias, a.adj = L.plan.adj, a.kind = MEL_CONV_GATV2;
        a.bs = (int)bs, a.n = n;
        a.obs = obs, a.obs_stride = obs_width, a.node_cols = node_cols, a.aggregator = aggregator;
        a.pooled = L.xcat, a.fid = table ? L.plan.fid : nullptr;
        StageScope t(MEL_STAGE_CONV1_ATT, s);
        if (mel_status st = launch_attend<ATT_POOL>(a, head_lanes(w->conv1.heads, w->conv1.channels), s, "conv1 attention + pool")) return st;
    }
    return run_heads(w, pw, L, bs, nullptr, bs, logits, s, select);
}

mel_status mel_hldgn_forward(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs, int32_t n,
                             int32_t obs_width, float* logits, void* workspace, size_t ws_bytes, void* stream) {
    return hldgn_forward_impl(w, aggregator, obs, bs, n, obs_width, true, logits, workspace, ws_bytes, stream);
}

mel_status mel_hldgn_forward_envs(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs, int32_t n,
                                  int32_t obs_stride, float* logits, void* workspace, size_t ws_bytes, void* stream) {
    return hldgn_forward_impl(w, aggregator, obs, bs, n, obs_stride, false, logits, workspace, ws_bytes, stream);
}

mel_status mel_plan_pointers(const mel_weights* w, int64_t bs, int32_t n, int64_t rows_cap, void* workspace, void** out5) {
    if (!w || !workspace || !out5 || bs <= 0 || n < 1 || n > MEL_MAX_NODES || rows_cap < 0)
        return fail(MEL_ERR_INVALID_ARG, "bad mel_plan_pointers arguments");
    const bool single = rows_cap == 0;
    const FwdLayout L = carve(w, make_dims(bs, n, single ? bs : rows_cap, single), workspace);
    const bool hl = w->model == MEL_MODEL_HLDGN;
    out5[0] = L.plan.adj, out5[1] = hl ? nullptr : (void*)L.plan.live;
    out5[2] = hl ? nullptr : (void*)L.plan.u1, out5[3] = hl ? nullptr : (void*)L.plan.u2, out5[4] = hl ? nullptr : (void*)L.plan.cnt;
    return MEL_OK;
}

mel_status mel_hldgn_forward_envs_select(const mel_weights* w, int32_t aggregator, const float* obs, int64_t bs, int32_t n,
                                         int32_t obs_stride, float* logits, const mel_select* select, void* workspace,
                                         size_t ws_bytes, void* stream) {
    if (select && select->act) {
        if (!select->live || select->n_nodes != n)
            return fail(MEL_ERR_INVALID_ARG, "per-env selection needs select->live and select->n_nodes == n_nodes");
    }
    return hldgn_forward_impl(w, aggregator, obs, bs, n, obs_stride, false, logits, workspace, ws_bytes, stream, select);
}

mel_status mel_gemm_f32(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                        int64_t M, int32_t N, int32_t K, int32_t relu, int32_t tile, void* stream) {
    if (!A || !W || !Y || M < 0 || M > (1ll << 30) || lda < K || ldy < N)
        return fail(MEL_ERR_INVALID_ARG, "bad gemm arguments");
    if (lda % 4)        // every tile code's kernel fetches A in 16-byte pieces from A + row * lda + 4 c (the ring kernel by LDS-DMA)
        return fail(MEL_ERR_UNSUPPORTED, "gemm: lda %% 4 == 0 (lda=%d)", lda);
    clear_stale_error();
    GemmArgs g;
    g.A = A, g.lda = lda, g.W = W, g.bias = bias, g.Y = Y, g.ldy = ldy, g.M = (int)M, g.N = N, g.K = K, g.relu = relu;
    return launch_gemm(g, GEMM_MODE_PLAIN, static_cast<hipStream_t>(stream), "mel_gemm_f32", -1, tile);
}

mel_status mel_gemm_f32_t(const float* A, int32_t lda, int32_t a_t, const float* W, int32_t ldw, int32_t w_t, float* Y, int32_t ldy,
                          int64_t M, int32_t N, int32_t K, void* stream) {
    if (!A || !W || !Y || M < 1 || M > (1ll << 30) || N < 64 || K < 32 || ldy < N)
        return fail(MEL_ERR_INVALID_ARG, "bad transposed-operand gemm arguments");
    if (N % 64 || K % GEMM_BK || lda % 4 || ldw % 4 || (a_t ? (M % 4 || lda < M) : lda < K) || (w_t ? ldw < N : ldw < K) || !w_t)
        return fail(MEL_ERR_UNSUPPORTED, "transposed-operand gemm: N %% 64 == 0, K %% 32 == 0, lda / ldw %% 4 == 0, M %% 4 == 0 with a "
                                         "transposed A, W transposed (the plain form is mel_gemm_f32)");
    clear_stale_error();
    GemmTArgs g{A, W, Y, lda, ldw, ldy, (int)M, N, K};
    const long grid = ((M + 63) / 64) * (N / 64);
    if (grid > (1l << 30)) return fail(MEL_ERR_INVALID_ARG, "transposed-operand gemm: too many tiles");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a_t) MEL_LAUNCH((gemm_f32_t_kernel<true, true>), dim3((int)grid), dim3(256), 0, s, g);
    else MEL_LAUNCH((gemm_f32_t_kernel<false, true>), dim3((int)grid), dim3(256), 0, s, g);
    return check_launch("mel_gemm_f32_t");
}

mel_status mel_gemm_f32_splitk(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                               int64_t M, int32_t N, int32_t K, int32_t relu, int32_t ksplit, float* parts, int64_t parts_floats,
                               void* stream) {
    if (!A || !W || !Y || !parts || M <= 0 || M > (1ll << 30) || lda < K || ldy < N)
        return fail(MEL_ERR_INVALID_ARG, "bad split-K gemm arguments");
    if (ksplit < 2 || K % GEMM_BK || (K / GEMM_BK) % ksplit || (K / GEMM_BK) / ksplit < 2 || N % 64 || lda % 4 || ldy % 4 ||
        parts_floats < (int64_t)ksplit * M * N)
        return fail(MEL_ERR_UNSUPPORTED, "split-K gemm: K / 32 = %d must split into %d chunks of >= 2 steps, N %% 64 == 0, "
                                         "lda %% 4 == 0, ldy %% 4 == 0, parts >= ksplit * M * N floats", K / GEMM_BK, ksplit);
    clear_stale_error();
    GemmArgs g;
    g.A = A, g.lda = lda, g.W = W, g.bias = bias, g.Y = Y, g.ldy = ldy, g.M = (int)M, g.N = N, g.K = K, g.relu = relu;
    return launch_gemm_splitk(g, ksplit, parts, (long)M * N, static_cast<hipStream_t>(stream), "mel_gemm_f32_splitk");
}

mel_status mel_gemm_f32_split(const float* A, int32_t lda, const float* W, const float* bias, float* Y, int32_t ldy,
                              int64_t M, int32_t N, int32_t K, int32_t relu, int32_t tile, int32_t ksplit, void* scratch,
                              int64_t scratch_bytes, void* stream) {
    if (!A || !W || !Y || !scratch || M <= 0 || M > (1ll << 30) || lda < K || ldy < N || N < 64 || K < 128)
        return fail(MEL_ERR_INVALID_ARG, "bad split-precision gemm arguments");
    const int64_t plane_bytes = ((int64_t)6 * N * K + 255) & ~255ll;
    const bool blocks = tile % MEL_TILE_PLANES_READY == MEL_TILE_WIDE;    // gemm_planes_kernel: A goes through bf16 planes in scratch as well
    const int64_t a_bytes = blocks ? M * K * 6 : 0;
    const int64_t need = plane_bytes + a_bytes + (ksplit > 1 ? (int64_t)ksplit * M * N * 4 : 0);
    // lda: both split kernels fetch A in 16-byte pieces (the 128 x 128 tile's planner falls back to the 64 x 64 kernel, which does too)
    if (K % 32 || N % 64 || lda % 4 || scratch_bytes < need)
        return fail(MEL_ERR_UNSUPPORTED, "split-precision gemm: K %% 32 == 0, N %% 64 == 0, lda %% 4 == 0, scratch >= %lld bytes",
                    (long long)need);
    clear_stale_error();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (blocks) {
        GemmArgs g;
        g.A = reinterpret_cast<const float*>(static_cast<char*>(scratch) + plane_bytes), g.lda = K;
        g.W = static_cast<const float*>(scratch), g.bias = bias, g.Y = Y, g.ldy = ldy, g.M = (int)M, g.N = N, g.K = K, g.relu = relu, g.split = 1;
        GemmRequest rq;
        rq.force_tile = MEL_TILE_WIDE;
        const GemmPlan plan = plan_gemm(&g, nullptr, 1, rq);
        if (ksplit > 1 || lda != K || M * K >= (1ll << 31) || plan.status)
            return fail(MEL_ERR_UNSUPPORTED, "split-precision gemm, 128 x 256 planes kernel: N %% 256 == 0, N <= %d, K / 16 >= 4, lda == K, "
                                             "ldy %% 4 == 0, no split-K", GEMP_BIAS_FLOATS);
        SplitBatch b{};
        b.n = 2, b.start[0] = 0;
        b.src[0] = W, b.dst[0] = static_cast<uint16_t*>(scratch), b.count[0] = N * K, b.K[0] = K, b.rb[0] = GEMP_BN;
        b.start[1] = (int)(((int64_t)N * K / 4 + 255) / 256);
        b.src[1] = A, b.dst[1] = reinterpret_cast<uint16_t*>(static_cast<char*>(scratch) + plane_bytes), b.count[1] = (int)(M * K), b.K[1] = K;
        b.rb[1] = 0;
        b.start[2] = b.start[1] + (int)((M * K / 4 + 255) / 256);
        MEL_LAUNCH(split_weights_kernel, dim3(b.start[2]), dim3(256), 0, s, b);
        if (mel_status st = check_launch("operands -> bf16 planes")) return st;
        return launch_plan(plan, s, 0, "mel_gemm_f32_split (planes)");
    }
    SplitBatch b{};
    b.n = 1, b.src[0] = W, b.dst[0] = static_cast<uint16_t*>(scratch), b.count[0] = N * K, b.K[0] = K, b.start[0] = 0;
    b.start[1] = (int)(((int64_t)N * K / 4 + 255) / 256);
    if (tile < MEL_TILE_PLANES_READY) {
        MEL_LAUNCH(split_weights_kernel, dim3(b.start[1]), dim3(256), 0, s, b);
        if (mel_status st = check_launch("weights -> bf16 planes")) return st;
    } else {
        tile -= MEL_TILE_PLANES_READY;
    }
    GemmArgs g;
    g.A = A, g.lda = lda, g.W = static_cast<const float*>(scratch), g.bias = bias, g.Y = Y, g.ldy = ldy, g.M = (int)M, g.N = N, g.K = K;
    g.relu = relu, g.split = 1;
    if (ksplit > 1)
        return launch_gemm_splitk(g, ksplit, reinterpret_cast<float*>(static_cast<char*>(scratch) + plane_bytes), (long)M * N, s,
                                  "mel_gemm_f32_split");
    return launch_gemm(g, GEMM_MODE_PLAIN, s, "mel_gemm_f32_split", -1, tile);
}

mel_status mel_radius_graph(const float* obs, int64_t bs, int32_t n, int32_t obs_stride, int32_t in_dim, uint64_t* adj,
                            void* stream) {
    if (!obs || !adj || bs < 1 || bs > (1 << 24) || n < 1 || n > MEL_MAX_NODES || in_dim < 1 || in_dim > 8 ||
        obs_stride < n * (in_dim + 3))
        return fail(MEL_ERR_INVALID_ARG, "mel_radius_graph: bad arguments");
    clear_stale_error();
    with_words(n, [&](auto w) {
        MEL_LAUNCH(radius_graph_kernel<decltype(w)::value>, dim3((bs + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), obs, (int)bs, n,
                   obs_stride, in_dim + 3, adj);
    });
    return check_launch("mel_radius_graph");
}

mel_status mel_gemm_bf16(const void* A, int32_t lda, const void* W, const float* bias, void* Y, int32_t ldy,
                         int64_t M, int32_t N, int32_t K, int32_t relu, int32_t y_f32, int32_t tile, void* stream) {
    if (!A || !W || !Y || M < 0 || M > (1ll << 30) || lda < K || ldy < N)
        return fail(MEL_ERR_INVALID_ARG, "bad gemm arguments");
    clear_stale_error();
    GemmArgs g;
    g.A = static_cast<const float*>(A), g.lda = lda, g.W = static_cast<const float*>(W), g.bias = bias;
    g.Y = static_cast<float*>(Y), g.ldy = ldy, g.M = (int)M, g.N = N, g.K = K, g.relu = relu, g.bf16 = 1, g.y_f32 = y_f32;
    return launch_gemm(g, GEMM_MODE_PLAIN, static_cast<hipStream_t>(stream), "mel_gemm_bf16", -1, tile);
}

mel_status mel_convert_bf16(const float* src, void* dst, int64_t count, void* stream) {
    if (!src || !dst || count < 0 || count % 8 != 0 || count > (1ll << 30))
        return fail(MEL_ERR_INVALID_ARG, "mel_convert_bf16: count must be a multiple of 8");
    if (count == 0) return MEL_OK;
    clear_stale_error();
    CvtBatch b{};
    b.n = 1, b.src[0] = src, b.dst[0] = static_cast<uint16_t*>(dst), b.count[0] = (int)count, b.start[0] = 0;
    b.start[1] = (int)((count / 8 + 255) / 256);
    MEL_LAUNCH(cvt_bf16_kernel, dim3(b.start[1]), dim3(256), 0, static_cast<hipStream_t>(stream), b);
    return check_launch("mel_convert_bf16");
}

mel_status mel_forward_tap(const mel_weights* w, int32_t kind, int64_t bs, int32_t n, int64_t rows_cap,
                           const void* workspace, void* out, void* stream) {
    if (!w || !workspace || !out || bs <= 0 || n < 1 || n > MEL_MAX_NODES) return fail(MEL_ERR_INVALID_ARG, "bad tap arguments");
    const bool single = rows_cap <= 0;
    const Dims d = make_dims(bs, n, single ? bs : rows_cap, single);
    const FwdLayout L = carve(w, d, const_cast<void*>(workspace));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (kind == 0)
        e = hipMemcpyAsync(out, L.plan.adj, (size_t)bs * n * set_words(n) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
    else if (kind == 1)
        e = hipMemcpyAsync(out, L.xcat, (size_t)d.rows_cap * w->q_head.layer[0].in_dim *
                           (w->precision == MEL_PREC_BF16 ? sizeof(uint16_t) : sizeof(float)), hipMemcpyDeviceToDevice, s);
    else if (kind == 2 && w->model != MEL_MODEL_HLDGN) {
        int32_t* o = static_cast<int32_t*>(out);
        e = hipMemcpyAsync(o, L.plan.off1 + bs, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o + 1, L.plan.off2 + bs, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o + 2, L.plan.offL + bs, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    } else if (kind == 3) {
        int32_t* o = static_cast<int32_t*>(out);
        e = hipMemcpyAsync(o, L.plan.fmeta, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o + 1, L.plan.fbad, (size_t)bs * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    } else if (kind >= MEL_TAP_H0 && kind <= MEL_TAP_ENC0) {
        // the feature-row buffers of the row-list path, each in its own element type, up to the rows carve() gave it
        if (w->flags & MEL_FWD_INTEGER_FEATURES)
            return fail(MEL_ERR_UNSUPPORTED, "tap kind %d is defined for the row-list path only", kind);
        const NetShape z = shape_of(w);
        const size_t es = z.bf ? sizeof(uint16_t) : sizeof(float);
        const size_t M = (size_t)bs * n, R = (size_t)d.rows_cap, U1 = (size_t)d.u1_cap, U2 = z.hl ? M : (size_t)d.u2_cap;
        const int hw = head_hidden_width(w->q_head) + head_hidden_width(w->v_head);
        const void* src = nullptr;
        size_t bytes = 0;
        switch (kind) {
            case MEL_TAP_H0: src = L.h0, bytes = U2 * z.hidden * es; break;
            case MEL_TAP_XL1: src = L.xl1, bytes = U2 * z.srcw * es; break;
            case MEL_TAP_XR1: src = L.xr1, bytes = U1 * z.hc * es; break;
            case MEL_TAP_H1: src = L.h1, bytes = U1 * z.hc * es; break;
            case MEL_TAP_XL2: src = L.xl2, bytes = U1 * z.srcw * es; break;
            case MEL_TAP_XR2: src = L.xr2, bytes = R * z.hc * es; break;
            case MEL_TAP_HQ0: src = L.hq[0], bytes = R * (hw > 0 ? hw : 1) * sizeof(float); break;
            case MEL_TAP_HQ1: src = L.hq[1], bytes = R * (hw > 0 ? hw : 1) * sizeof(float); break;
            default: src = L.enc0, bytes = U2 * z.K0 * es; break;
        }
        if (!src) return fail(MEL_ERR_UNSUPPORTED, "tap kind %d: this model / shape has no such buffer", kind);
        e = hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, s);
    } else
        return fail(MEL_ERR_INVALID_ARG, "unknown tap kind %d", kind);
    if (e != hipSuccess) return fail(MEL_ERR_LAUNCH, "tap copy: %s", hipGetErrorString(e));
    return MEL_OK;
}

// the export kernel's view of a conv2 target descriptor is TargetDesc, member for member
static_assert(sizeof(AgentRowDesc<1>) == sizeof(TargetDesc<1>) && sizeof(AgentRowDesc<2>) == sizeof(TargetDesc<2>), "AgentRowDesc");
static_assert(offsetof(AgentRowDesc<2>, smask) == offsetof(TargetDesc<2>, smask) && offsetof(AgentRowDesc<2>, soff) == offsetof(TargetDesc<2>, soff) &&
              offsetof(AgentRowDesc<1>, smask) == offsetof(TargetDesc<1>, smask) && offsetof(AgentRowDesc<1>, soff) == offsetof(TargetDesc<1>, soff),
              "AgentRowDesc");

mel_status mel_forward_attention(const mel_weights* w, int64_t bs, int32_t n, int64_t rows_cap, const void* workspace,
                                 float* alpha, uint64_t* sources, void* stream) {
    if (!w || !workspace || !alpha || !sources)
        return fail(MEL_ERR_INVALID_ARG, "mel_forward_attention: null argument (w, workspace, alpha, sources)");
    if (bs <= 0 || bs > (1 << 24) || n < 1 || n > MEL_MAX_NODES || rows_cap < 1 || rows_cap > bs * (int64_t)n)
        return fail(MEL_ERR_INVALID_ARG, "mel_forward_attention: bs=%ld, n_nodes=%d or rows_cap=%ld outside [1, bs*n]", (long)bs, n, (long)rows_cap);
    if (w->model != MEL_MODEL_LDGN && w->model != MEL_MODEL_DGNR)
        return fail(MEL_ERR_UNSUPPORTED, "mel_forward_attention: model %d has no second convolution and no agent rows", w->model);
    if (w->precision == MEL_PREC_BF16)
        return fail(MEL_ERR_UNSUPPORTED, "mel_forward_attention: bf16 feature rows are not built");
    if (w->precision < MEL_PREC_F32 || w->precision > MEL_PREC_F32_AUTO) return fail(MEL_ERR_INVALID_ARG, "precision=%d", w->precision);
    clear_stale_error();
    // Nothing the forward launches behind its conv2 attention writes x_l2 / x_r2, the conv2 descriptors or the row count (the
    // heads read xcat and write hq / hpart), in row-list and in table mode alike: conv2's buffers hold rows in both.
    const FwdLayout L = carve(w, make_dims(bs, n, rows_cap, false), const_cast<void*>(workspace));
    const NetShape z = shape_of(w);
    AttExportArgs a{};
    a.xl = L.xl2, a.ld_l = z.srcw, a.xr = L.xr2, a.ld_r = z.hc, a.att = w->conv2.kind == MEL_CONV_GATV2 ? w->conv2.att : nullptr;
    a.desc = L.plan.desc2, a.rows_dev = L.plan.offL + bs, a.rows_cap = (int)rows_cap;
    a.heads = w->conv2.heads, a.kind = w->conv2.kind, a.score_scale = 1.0f / sqrtf((float)w->conv2.channels);
    a.alpha = alpha, a.sources = sources;
    return launch_attention_export(a, head_lanes(w->conv2.heads, w->conv2.channels), n, static_cast<hipStream_t>(stream),
                                   "mel_forward_attention");
}

void* mel_prof_create(int32_t capacity) {
    if (capacity < 1) return nullptr;
    Profiler* p = new Profiler();
    p->capacity = capacity;
    p->ev = new hipEvent_t[2 * (size_t)capacity];
    p->stage = new int[capacity];
    for (int i = 0; i < 2 * capacity; ++i)
        if (hipEventCreate(&p->ev[i]) != hipSuccess) {
            for (int k = 0; k < i; ++k) (void)hipEventDestroy(p->ev[k]);
            delete[] p->ev;
            delete[] p->stage;
            delete p;
            set_error("hipEventCreate failed");
            return nullptr;
        }
    return p;
}

void mel_prof_destroy(void* prof) {
    Profiler* p = static_cast<Profiler*>(prof);
    if (!p) return;
    if (g_prof == p) g_prof = nullptr;
    for (int i = 0; i < 2 * p->capacity; ++i) (void)hipEventDestroy(p->ev[i]);
    delete[] p->ev;
    delete[] p->stage;
    delete p;
}

void mel_prof_attach(void* prof) { g_prof = static_cast<Profiler*>(prof); }

void mel_prof_reset(void* prof) {
    if (prof) static_cast<Profiler*>(prof)->count = 0;
}

int32_t mel_prof_read(void* prof, double* ms_sum, int64_t* count) {
    Profiler* p = static_cast<Profiler*>(prof);
    if (!p || !ms_sum || !count) return fail(MEL_ERR_INVALID_ARG, "bad profiler arguments");
    for (int k = 0; k < MEL_N_STAGES; ++k) ms_sum[k] = 0.0, count[k] = 0;
    for (int i = 0; i < p->count; ++i) {
        if (hipEventSynchronize(p->ev[2 * i + 1]) != hipSuccess) return fail(MEL_ERR_LAUNCH, "event sync failed");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p->ev[2 * i], p->ev[2 * i + 1]) != hipSuccess) return fail(MEL_ERR_LAUNCH, "event elapsed failed");
        const int st = p->stage[i];
        if (st >= 0 && st < MEL_N_STAGES) ms_sum[st] += ms, count[st] += 1;
    }
    return p->count;
}

mel_status mel_select_action(const float* logits, const uint8_t* mask, int64_t bs, int32_t na, float eps,
                             const float* rand_u, const float* rand_q, int32_t* act, void* scratch, void* stream) {
    if (!logits || !act || bs <= 0 || na < 1) return fail(MEL_ERR_INVALID_ARG, "bad select_action arguments");
    if (mask && !scratch) return fail(MEL_ERR_INVALID_ARG, "masking needs 8 bytes of scratch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    clear_stale_error();
    StageScope t(MEL_STAGE_SELECT, s);
    if (mask) {
        MEL_LAUNCH(minmax_kernel, dim3(1), dim3(1024), 0, s, logits, (long)bs * na, static_cast<float*>(scratch));
        if (mel_status st = check_launch("minmax")) return st;
    }
    MEL_LAUNCH(select_action_kernel, dim3((bs + 255) / 256), dim3(256), 0, s, logits, mask, (long)bs, na, eps,
                       rand_u, rand_q, static_cast<const float*>(scratch), act);
    return check_launch("select_action");
}

mel_status mel_exploration_schedule(const int32_t* decisions, int32_t stride, int32_t n_envs, uint32_t scale,
                                    double eps_train, double eps_final, double exploration_fraction, double total_steps,
                                    const uint32_t* round_dev, float* eps_out, uint64_t* env_step_out, int32_t trace_cap,
                                    uint64_t* trace_env_step, float* trace_eps, void* stream) {
    if (!decisions || !eps_out || n_envs < 1 || stride < 1) return fail(MEL_ERR_INVALID_ARG, "bad exploration_schedule arguments");
    if (trace_cap < 0 || (trace_cap > 0 && (!trace_env_step || !trace_eps)))
        return fail(MEL_ERR_INVALID_ARG, "exploration_schedule: a trace ring needs both arrays");
    const double horizon = exploration_fraction * total_steps;
    // (negated comparisons: a NaN fails them too)
    if (!(horizon > 0.0) || !std::isfinite(horizon)) return fail(MEL_ERR_INVALID_ARG, "exploration_schedule: horizon %g <= 0", horizon);
    if (!(eps_final > 0.0)) return fail(MEL_ERR_INVALID_ARG, "exploration_schedule: eps_final %g <= 0", eps_final);
    if (!(eps_final <= eps_train) || !std::isfinite(eps_train))
        return fail(MEL_ERR_INVALID_ARG, "exploration_schedule: eps_final %g > eps_train %g", eps_final, eps_train);
    hipStream_t s = static_cast<hipStream_t>(stream);
    clear_stale_error();
    StageScope t(MEL_STAGE_SELECT, s);
    MEL_LAUNCH(exploration_schedule_kernel, dim3(1), dim3(256), 0, s, decisions, (int)stride, (int)n_envs, scale, eps_train,
                       eps_final, std::log(eps_final) / horizon, round_dev, eps_out,
                       reinterpret_cast<unsigned long long*>(env_step_out), (int)trace_cap,
                       reinterpret_cast<unsigned long long*>(trace_env_step), trace_eps);
    return check_launch("exploration_schedule");
}

mel_status mel_select_action_envs(const float* logits, const uint64_t* live, int64_t bs, int32_t n, int32_t na,
                                  float eps, uint32_t seed, const uint32_t* step_dev, int32_t* act, void* stream) {
    if (!logits || !live || !act || bs <= 0 || n < 1 || n > MEL_MAX_NODES || na < 1)
        return fail(MEL_ERR_INVALID_ARG, "bad select_action_envs arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    clear_stale_error();
    StageScope t(MEL_STAGE_SELECT, s);
    MEL_LAUNCH(select_envs_kernel, dim3((bs * n + 255) / 256), dim3(256), 0, s, logits, live, (long)bs, n, na, eps,
                       seed, step_dev, act);
    return check_launch("select_action_envs");
}

mel_status mel_select_action_rows(const float* logits, const int32_t* logit_row, int64_t rows_cap,
                                  const int32_t* rows_dev, int32_t na, float eps, uint32_t seed, uint32_t step,
                                  const uint32_t* step_dev, int32_t* act, void* stream) {
    if (!logits || !act || rows_cap <= 0 || na < 1) return fail(MEL_ERR_INVALID_ARG, "bad select_action_rows arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    clear_stale_error();
    StageScope t(MEL_STAGE_SELECT, s);
    MEL_LAUNCH(select_rows_kernel, dim3((rows_cap + 255) / 256), dim3(256), 0, s, logits, logit_row, (long)rows_cap,
                       rows_dev, na, eps, seed, step, step_dev, act);
    return check_launch("select_action_rows");
}

}  // extern "C"
