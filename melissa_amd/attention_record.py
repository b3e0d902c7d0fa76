"""Whom the deciding agents attend to, per round, recorded on the device (``mel_attention_record``, include/melissa_hip.h).

The policy is a graph-attention network and its attention coefficients are the one part a reader can interpret.
``watch --attention-out`` shows the raw coefficients of a few greedy rounds from a second, full learn-path forward; over an
evaluation of many episodes and envs the question a paper asks needs the coefficients the pruned INFERENCE launches decided
with: does a deciding node listen to neighbours that already hold the message or to those still waiting for it, and how does
that change with the round and with the node's degree.  The data exists between two launches only: after the round's forward
its workspace still holds conv2's projections, target descriptors and row count, and ``mel_env_round`` then overwrites the state
the decision was taken in.  :class:`AttentionRecorder` owns the device buffers of two capturable launches that sit in that
window (:class:`melissa_amd.collect.RoundLoop`, ``attention=``): ``mel_forward_attention`` writes the coefficients and source
sets of the round's agent rows, ``mel_attention_record_round`` books every decision of the policy by round index, by the
deciding node's degree and by head, and for a few chosen envs a ring of per-round records that join the other two recorders'
traces on (env, episode ordinal, num_moves).  Opt-in: a loop without it issues no such launch.

:func:`summarise_attention` is pure NumPy: it turns the tables into means, lifts and effective neighbour counts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .record_common import TraceRecorder, check_out_args, group_by_ordinal, save_traces

FIELDS = ("decisions", "self", "informed", "informed_share", "waiting", "waiting_share", "squares", "max")


def check_attention_args(spread: bool, attention_curves_out=None, attention_trace_out=None, trace_envs: int = 1,
                         model: "str | None" = None, feature_dtype: "str | None" = None) -> None:
    """ValueError for attention-recorder arguments that mean nothing (no torch, nothing built).  ``model`` / ``feature_dtype``:
    the names ``watch`` takes, checked only when an output is asked for."""
    if attention_curves_out is not None or attention_trace_out is not None:
        if model is not None and "hl_dgn" in str(model):
            raise ValueError(f"the attention recorder reads conv2's coefficients: model {model!r} (HL-DGN) has no second convolution")
        if feature_dtype == "bf16":
            raise ValueError("the attention recorder is not built for bf16 feature rows (feature_dtype / --dtype bf16)")
    check_out_args("attention recorder", spread, dict(attention_curves_out=attention_curves_out,
                                                      attention_trace_out=attention_trace_out),
                   attention_trace_out is not None, trace_envs)


def _figures(t: np.ndarray) -> dict:
    """Rows of sums [..., 8] -> the figures of every row; every ratio is NaN where the row holds no decision."""
    cnt = t[..., _lib.AR_DECISIONS]
    with np.errstate(divide="ignore", invalid="ignore"):
        per = lambda f: np.where(cnt > 0, t[..., f] / cnt, np.nan)
        lift = lambda a, share: np.where((cnt > 0) & (t[..., share] > 0), t[..., a] / t[..., share], np.nan)
        return dict(decisions=cnt.copy(), self_mean=per(_lib.AR_SELF), informed_mean=per(_lib.AR_INFORMED),
                    informed_share_mean=per(_lib.AR_INFORMED_SHARE), waiting_mean=per(_lib.AR_WAITING),
                    waiting_share_mean=per(_lib.AR_WAITING_SHARE), squares_mean=per(_lib.AR_SQUARES), max_mean=per(_lib.AR_MAX),
                    informed_lift=lift(_lib.AR_INFORMED, _lib.AR_INFORMED_SHARE),
                    waiting_lift=lift(_lib.AR_WAITING, _lib.AR_WAITING_SHARE),
                    effective_neighbours=np.where((cnt > 0) & (t[..., _lib.AR_SQUARES] > 0), cnt / t[..., _lib.AR_SQUARES], np.nan))


def summarise_attention(by_round, by_degree, by_head) -> dict:
    """The tables ``by_round`` float64 ``[R, 8]``, ``by_degree`` ``[D, 8]`` and ``by_head`` ``[H, 8]`` (fields :data:`FIELDS`) as
    figures.

    -> dict: ``rounds`` [R], ``degrees`` [D] (the last degree row also holds every larger degree), ``heads`` [H], and ``by_round``
    / ``by_degree`` / ``by_head``: dicts of arrays over the rows - ``decisions``; the means per decision ``self_mean``,
    ``informed_mean`` / ``waiting_mean`` (the attention the neighbours that hold the message / still wait for it got),
    ``informed_share_mean`` / ``waiting_share_mean`` (those classes' shares of the sources), ``squares_mean``, ``max_mean``; the
    lifts ``informed_lift`` = field 2 / field 3 and ``waiting_lift`` = field 4 / field 5 (1: the class gets what uniform attention
    would give it; NaN where the class was never present); ``effective_neighbours`` = 1 / mean of the sum of squares.  Every ratio
    is NaN where the row holds no decision.  ``total``: the same figures (floats) over all rows of ``by_degree``, which also
    holds the decisions of rounds past the round table."""
    tabs = [np.asarray(t, dtype=np.float64) for t in (by_round, by_degree, by_head)]
    for name, t in zip(("by_round", "by_degree", "by_head"), tabs):
        if t.ndim != 2 or t.shape[1] != _lib.AR_FIELDS:
            raise ValueError(f"summarise_attention: {name} {t.shape} must be [rows, {_lib.AR_FIELDS}]")
    by_round, by_degree, by_head = tabs
    return dict(rounds=np.arange(by_round.shape[0]), degrees=np.arange(by_degree.shape[0]), heads=np.arange(by_head.shape[0]),
                by_round=_figures(by_round), by_degree=_figures(by_degree), by_head=_figures(by_head),
                total={k: float(v) for k, v in _figures(by_degree.sum(axis=0)).items()})


def group_attention_episodes(records: list) -> list:
    """Attention records of ONE env in play order -> one dict per episode ordinal: ``env``, ``ordinal``, ``pool_episode``,
    ``rounds`` [K] (num_moves of the state the decisions were taken in), ``decisions`` / ``without_sources`` int32 [K], ``sets``
    uint64 [K, W] (the deciding set), ``fields`` float64 [K, N, 8] (the head-mean fields, 0 for nodes that did not decide)."""
    return group_by_ordinal(records, scalars={}, series=dict(decisions=4, without_sources=5), arrays=("sets", "fields"))


save_attention_traces = save_traces      # keyed as :func:`melissa_amd.round_record.save_traces` keys the node traces


class AttentionRecorder(TraceRecorder):
    """Owner of one ``mel_attention_record``, of the ``alpha`` / ``sources`` buffers ``mel_forward_attention`` fills for
    ``rows_cap`` agent rows, and of their device buffers, for the envs of ``venv`` and the network ``net`` (L-DGN or DGN-R on an
    fp32 feature path: HL-DGN has no second convolution and bf16 rows are not built - ValueError).  ``rows_cap``: the cap of the
    loop's forward (default ``env_num * N``).  ``max_rounds``, ``n_degrees``, ``trace_envs``, ``trace_capacity``, ``quota``: as
    :class:`melissa_amd.decision_record.DecisionRecorder` takes them.  Give it to :class:`melissa_amd.collect.RoundLoop`
    (``attention=``) BEFORE the loop captures its rounds: captured launches hold the pointers and the sizes."""

    group = staticmethod(group_attention_episodes)

    @staticmethod
    def trace_spec(n: int, W: int) -> dict:
        return dict(sets=((W,), "int64"), fields=((n, _lib.AR_FIELDS), "float64"))

    launches = 0             # calls of :meth:`launch`, over every instance (tests: a loop without a recorder makes none)

    def __init__(self, venv, net, rows_cap: "int | None" = None, max_rounds: "int | None" = None,
                 n_degrees: "int | None" = None, trace_envs=(), trace_capacity: int = 64, quota=None, device=None):
        import torch
        who = type(self).__name__
        if getattr(net, "_MODEL", None) == _lib.MODEL_HLDGN or not hasattr(net, "conv2"):
            raise ValueError(f"{who}: {type(net).__name__} has no second convolution and no agent rows (HL-DGN)")
        if getattr(net, "feature_dtype", "f32") == "bf16":
            raise ValueError(f"{who}: the coefficients of bf16 feature rows are not built (feature_dtype='bf16')")
        H = int(net.conv2.heads)
        if not 1 <= H <= _lib.AR_MAX_HEADS:
            raise ValueError(f"{who}: {H} heads outside [1, {_lib.AR_MAX_HEADS}]")
        D = min(int(venv.n), 64) if n_degrees is None else int(n_degrees)
        if not 1 <= D <= _lib.DR_MAX_DEGREES:
            raise ValueError(f"{who}: n_degrees={D} outside [1, {_lib.DR_MAX_DEGREES}]")
        B, n, R, dev = self._setup(venv, max_rounds, trace_envs, trace_capacity, device)
        cap = B * n if rows_cap is None else int(rows_cap)
        if not 1 <= cap <= B * n:
            raise ValueError(f"{who}: rows_cap={cap} outside [1, {B * n}]")
        self.net, self.heads, self.n_degrees, self.rows_cap = net, H, D, cap
        f64, i64 = torch.float64, torch.int64
        self.alpha = torch.zeros(cap, _lib.ATT_MAX_SOURCES, H, dtype=torch.float32, device=dev)
        self.sources = torch.zeros(cap, _lib.set_words(n), dtype=i64, device=dev)
        self.by_round = torch.zeros(B, R, _lib.AR_FIELDS, dtype=f64, device=dev)
        self.by_degree = torch.zeros(B, D, _lib.AR_FIELDS, dtype=f64, device=dev)
        self.by_head = torch.zeros(B, H, _lib.AR_FIELDS, dtype=f64, device=dev)
        self.overflow = torch.zeros(B, dtype=i64, device=dev)
        self.skipped = torch.zeros(B, dtype=i64, device=dev)
        self._out_round = torch.zeros(R, _lib.AR_FIELDS, dtype=f64, device=dev)
        self._out_degree = torch.zeros(D, _lib.AR_FIELDS, dtype=f64, device=dev)
        self._out_head = torch.zeros(H, _lib.AR_FIELDS, dtype=f64, device=dev)
        self._counters = torch.zeros(4, dtype=i64, device=dev)
        self.c = c = _lib.MelAttentionRecord()
        c.by_round, c.by_degree, c.by_head = self.by_round.data_ptr(), self.by_degree.data_ptr(), self.by_head.data_ptr()
        c.overflow, c.skipped = self.overflow.data_ptr(), self.skipped.data_ptr()
        c.n_degrees, c.n_heads = D, H
        self._bind_ring(quota)

    # ------------------------------------------------------------------ launch (capturable: no host read, no allocation)
    def launch(self, net, workspace, rows_cap: int, row_offsets, live) -> None:
        """Between the round's forward and its ``mel_env_round``, the two launches: the coefficients and source sets of the
        agent rows the forward of ``net`` just left in ``workspace`` (``rows_cap``: the forward's), then the booking with
        ``row_offsets`` int32 [B + 1] and ``live``, the round's active sets."""
        if int(rows_cap) != self.rows_cap:
            raise ValueError(f"AttentionRecorder: built for rows_cap={self.rows_cap}, the forward ran with {int(rows_cap)}")
        AttentionRecorder.launches += 1
        net.round_attention(workspace, int(self.venv.env_num), self.rows_cap, self.alpha, self.sources)
        self.launch_record(self.alpha, self.sources, row_offsets, live)

    def launch_record(self, alpha, sources, row_offsets, live) -> None:
        """The booking launch alone, on coefficients ``alpha`` fp32 [rows, 34, heads] and ``sources`` int64 [rows, W]."""
        _lib.check(_lib.load().mel_attention_record_round(
            C.byref(self.c), C.byref(self.venv.env), alpha.data_ptr(), sources.data_ptr(), row_offsets.data_ptr(),
            live.data_ptr(), self.heads, _lib.current_stream_ptr(self.device)), "mel_attention_record_round")

    # ------------------------------------------------------------------ host side
    def reset(self) -> None:
        """Zero the tables and the counters, forget every trace record."""
        for t in (self.by_round, self.by_degree, self.by_head, self.overflow, self.skipped):
            t.zero_()
        self._reset_ring()

    def tables(self):
        """-> (by_round float64 [R, 8], by_degree [D, 8], by_head [H, 8], {"overflow": int, "skipped": int}): the envs' rows added
        on the device in ascending env order; the counters are 0 in a clean run.  Synchronises."""
        import torch
        _lib.check(_lib.load().mel_attention_record_read(
            C.byref(self.c), self._out_round.data_ptr(), self._out_degree.data_ptr(), self._out_head.data_ptr(),
            self._counters.data_ptr(), _lib.current_stream_ptr(self.device)), "mel_attention_record_read")
        torch.cuda.synchronize(self.device)
        counters = self._counters.cpu().tolist()
        return (self._out_round.cpu().numpy(), self._out_degree.cpu().numpy(), self._out_head.cpu().numpy(),
                dict(overflow=int(counters[_lib.DRC_OVERFLOW]), skipped=int(counters[_lib.DRC_SKIPPED])))
