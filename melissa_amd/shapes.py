"""Which (hidden width, head count) pairs the HIP path runs - the ONE Python restatement of the library's rule
(``validate()`` in csrc/fwd.hip, ``head_lanes`` in csrc/common.hpp), held to it by tests/test_gpu_head_shapes.py.

No torch and no library here: ``python -m melissa_amd.train`` checks its arguments with this before it starts any rank.

The networks give every head ``hidden`` channels (``GATv2Conv(hidden, hidden, heads)``), so a row is ``heads * hidden`` wide.
The attention kernels lay it over one 64-lane wavefront: a head is ``lanes_per_head`` adjacent lanes - the largest power of
two with ``heads * lanes_per_head <= 64`` - of ``hidden / lanes_per_head`` consecutive channels each (2, 4, 8 or 16: the
instantiated widths).  A power-of-two head count fills the wavefront; 6 heads fill 48 lanes (8 per head) and leave 16 idle,
which is built for 8 and 16 channels per lane (hidden 64 and 128).  Other head counts are refused.
"""
from __future__ import annotations

CHANNELS_PER_LANE = (2, 4, 8, 16)
MAX_HEAD_LAYERS = 6                 # MEL_MAX_HEAD_LAYERS (include/melissa_hip.h): Linear layers of a dueling head, the last one included
ENCODER_MAX_WIDTH = 512             # validate(): ENC_MAX_WIDTH (csrc/fwd.hip; beyond 256 the encoder's first layer is a launch of its own)


def head_lanes(heads: int, channels: int):
    """-> (lanes_per_head, live_lanes, channels_per_lane, reason): ``reason`` is None when the attention kernels run the shape."""
    if heads < 1 or heads > 64 or channels < 1:
        return 0, 0, 0, "heads outside [1, 64] or no channels"
    lanes = 1
    while heads * lanes * 2 <= 64:
        lanes *= 2
    live = heads * lanes
    if channels % lanes:
        return lanes, live, 0, (f"{channels} channels per head are no multiple of the {lanes} lanes a head gets "
                                f"(largest power of two with heads * lanes <= 64)")
    vpl = channels // lanes
    if vpl not in CHANNELS_PER_LANE:
        return lanes, live, vpl, (f"{channels} channels over {lanes} lanes per head are {vpl} channels per lane; "
                                  f"the attention kernels exist for 2, 4, 8 and 16")
    if live != 64 and not (live == 48 and lanes == 8 and vpl >= 8):
        return lanes, live, vpl, (f"{heads} heads fill {live} of 64 lanes; built are the power-of-two head counts (a full "
                                  f"wavefront) and 6 heads of 64 or 128 channels (48 live lanes)")
    return lanes, live, vpl, None


def hip_shape_supported(hidden: int, heads: int):
    """-> (True, "") when the HIP forward and learn path run networks of ``hidden`` width and ``heads`` attention heads,
    else (False, reason).  Mirrors ``validate()`` (csrc/fwd.hip) for the networks ``train.build_network`` builds."""
    hidden, heads = int(hidden), int(heads)
    if hidden < 64 or hidden % 64:
        return False, f"hidden width {hidden}: the encoder and projection GEMM tiles need a multiple of 64"
    if hidden > ENCODER_MAX_WIDTH:
        return False, f"hidden width {hidden} > {ENCODER_MAX_WIDTH}: the encoder is built for at most that many columns"
    reason = head_lanes(heads, hidden)[3]
    if reason is not None:
        return False, f"{heads} heads of {hidden} channels: {reason}"
    return True, ""


def require_hip_shape(hidden: int, heads: int) -> None:
    ok, reason = hip_shape_supported(hidden, heads)
    if not ok:
        raise ValueError(f"hidden_emb={hidden}, num_heads={heads} is not supported on the HIP path: {reason}")
