// conv2's attention coefficients of the INFERENCE path: what fwd.hip (mel_forward_attention; the contract is in melissa_hip.h)
// and attention_record.hip (the kernel) share.  The forward's conv2 attention streams a target's sources through an online
// softmax and keeps only the aggregate; what it aggregated WITH is still recoverable afterwards: x_l2, x_r2, the conv2 target
// descriptors and the device-side row count stay in the workspace until the next forward (nothing behind the conv2 attention
// writes them: the heads read the head input and their own ping-pong buffers).  One launch of its own reads them again.
// The kernel lives in a translation unit of its own, so the code objects of fwd.hip, env.hip and grad.hip - every kernel the
// training and inference paths launch - are the ones they are without this feature.
#pragma once
#include "common.hpp"

namespace mel {

// A row has at most this many sources: plan_masks.hpp: radius_sources keeps the first 33 hits of the radius rule (self among
// them, then dropped), GATv2 adds the self-loop back.  The export kernel and the recorder walk min(count, this) sources; were
// the cap of radius_sources ever raised, this constant and the alpha layout have to follow it.
static_assert(MEL_ATT_MAX_SOURCES == 33 + 1, "MEL_ATT_MAX_SOURCES = the neighbour cap of radius_sources (33) + the GATv2 self-loop");
constexpr int ATT_EXPORT_MAX_HEADS = 16;      // head_lanes admits no more: 16 heads of 64 channels, 4 lanes each

// A conv2 target descriptor as the export kernel reads it: plan.hpp's TargetDesc<W>, member for member (fwd.hip, which sees
// both, holds the two to each other with static_asserts)
template <int W>
struct AgentRowDesc {
    NodeSet<W> sources; // source nodes of the target (closed neighbourhood for GATv2, open for TransformerConv)
    NodeSet<W> smask;   // node set the source rows are packed by
    int32_t soff;       // first source row of the env
    int32_t env;
    int32_t node;
    int32_t cat_row;
};

struct AttExportArgs {
    const float* xl;        // conv2 source rows [U1 rows, ld_l] (TransformerConv: key | value)
    int ld_l;
    const float* xr;        // conv2 target rows [agent rows, ld_r]
    int ld_r;
    const float* att;       // [heads*C], GATv2 only
    const void* desc;       // [rows_cap] AgentRowDesc<W> of the agent rows
    const int32_t* rows_dev;
    int rows_cap, heads, lanes_per_head, live, kind;
    float score_scale;
    float* alpha;           // [rows_cap][MEL_ATT_MAX_SOURCES][heads]
    uint64_t* sources;      // [rows_cap][W]
};

// attention_record.hip: the launch for the head shape hl (MEL_ERR_UNSUPPORTED where the attention kernels do not run it)
mel_status launch_attention_export(AttExportArgs a, const HeadLanes& hl, int n_nodes, hipStream_t s, const char* what);

}  // namespace mel
