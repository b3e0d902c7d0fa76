"""The replay samplers on the MI355X over hand-built rings (tests/replay_rings.py): ``mel_replay_sample``, ``mel_replay_sample_prio``
(refresh + sample) and ``mel_replay_update_priority`` called directly, so the test owns the seed, the draw counter and the scratch.
Every sample of every batch is compared with the oracle: picks, walk outputs and observation rows exactly, ``ret`` within the
derived bound of tests/test_replay_rings.py::assert_walk_equal, weights and written priorities within the project's 1e-6.  The
rings reach past one scan chunk (1 024 records) and one scan pass (sixteen chunks), are not full, and hold stale sets in the
slots no round has written; tests/test_replay_rings.py checks without a GPU that they produce every walk ending often enough.

Each case prints the largest deviations it saw (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import replay_rings as rr
from tests.prio_oracle import EPS, PrioOracle
from tests.test_replay_rings import _ring, assert_walk_equal, load_ring, refresh_case

GUARD = 3                                                      # rows behind every output that must stay untouched
BATCHES = (1024, 1000, 1)
INT_GUARD, F_GUARD = -77, float("nan")


def _outputs(rp, batch, weight=False):
    """Output buffers of one launch with GUARD rows behind ``batch`` (NaN / -77) and the MelReplayBatch that points at them."""
    from melissa_amd import _lib
    rows, width = batch + GUARD, 8 * rp.n + 1
    out = {k: torch.full((rows, width), F_GUARD, device="cuda") for k in ("obs", "boot_obs")}
    out.update({k: torch.full((rows,), F_GUARD, device="cuda") for k in ("ret", "boot_w") + (("weight",) if weight else ())})
    out.update({k: torch.full((rows,), INT_GUARD, dtype=torch.int64, device="cuda") for k in ("act", "env", "slot", "agent")})
    if rp.active_nb is not None:
        out["nb_sibling"] = torch.full((rows, rp.W), INT_GUARD, dtype=torch.int64, device="cuda")
    b = _lib.MelReplayBatch()
    for name, t in out.items():
        if name != "weight":
            setattr(b, name, t.data_ptr())
    return out, b


def _collect(out, batch):
    """Outputs -> NumPy [batch, ...], after checking that the guard rows were not written."""
    torch.cuda.synchronize()
    got = {}
    for name, t in out.items():
        a = t.cpu().numpy()
        tail = a[batch:]
        assert np.isnan(tail).all() if a.dtype == np.float32 else (tail == INT_GUARD).all(), f"{name}: rows beyond the batch written"
        got[name] = a[:batch]
        assert not np.isnan(got[name]).any() if a.dtype == np.float32 else True, f"{name}: rows of the batch left unwritten"
    return got


def _disc(n_step):
    return (C.c_float * (n_step + 1))(*[float(x) for x in rr.discounts(n_step)])


def _stream():
    from melissa_amd import _lib
    return _lib.current_stream_ptr(torch.device("cuda"))


def sample_uniform(rp, batch, n_step, draw):
    """One ``mel_replay_sample`` launch from draw counter ``draw``.  Returns the batch and the prefix scratch [B K + 1]."""
    from melissa_amd import _lib
    BK = rp.B * rp.K
    out, b = _outputs(rp, batch)
    counter = torch.tensor([draw, INT_GUARD], dtype=torch.int64, device="cuda")
    prefix = torch.full((BK + 2,), INT_GUARD, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().mel_replay_sample(C.byref(rp.struct), rp.B, rp.n, batch, n_step, _disc(n_step), rr.SEED, counter.data_ptr(),
                                             prefix.data_ptr(), C.byref(b), _stream()), "mel_replay_sample")
    got = _collect(out, batch)
    assert counter.tolist() == [draw + 1, INT_GUARD]
    prefix = prefix.cpu().numpy()
    assert prefix[BK + 1] == INT_GUARD, "the word behind the prefix scratch was written"
    return got, prefix[:BK + 1]


class Priority:
    """A ``mel_replay_priority`` block of the test's own, every array with a guard behind it (``prio`` also in front)."""

    def __init__(self, rp, prio, seen, alpha=0.6, beta=0.4, weight_norm=1, max_prio=3.0, min_prio=0.37):
        from melissa_amd import _lib
        B, K, n = rp.B, rp.K, rp.n
        self.shape, self.margin = (B, K, n), K * n
        self.buf = torch.full(((B + 2) * K * n,), 123.0, device="cuda")
        self.prio = self.buf[self.margin:self.margin + B * K * n].view(B, K, n)
        self.prio.copy_(torch.from_numpy(np.asarray(prio, np.float32)))
        self.rec_sum = torch.full((B * K + 1,), F_GUARD, dtype=torch.float64, device="cuda")
        self.prefix = torch.full((B * K + 2,), F_GUARD, dtype=torch.float64, device="cuda")
        self.seen = torch.cat([torch.from_numpy(np.asarray(seen, np.int32)), torch.tensor([INT_GUARD], dtype=torch.int32)]).cuda()
        self.max_prio = torch.tensor([max_prio, F_GUARD], device="cuda")
        self.min_prio = torch.tensor([min_prio, F_GUARD], device="cuda")
        p = _lib.MelReplayPriority()
        p.prio, p.rec_sum, p.prefix, p.seen = self.prio.data_ptr(), self.rec_sum.data_ptr(), self.prefix.data_ptr(), self.seen.data_ptr()
        p.max_prio, p.min_prio = self.max_prio.data_ptr(), self.min_prio.data_ptr()
        p.alpha, p.beta, p.weight_norm = alpha, beta, weight_norm
        self.struct = p

    def read(self):
        """prio [B, K, n], rec_sum [B K], prefix [B K + 1], seen [B], max_prio, min_prio - after checking every guard."""
        torch.cuda.synchronize()
        B, K, n = self.shape
        buf = self.buf.cpu().numpy()
        assert (buf[:self.margin] == 123.0).all() and (buf[-self.margin:] == 123.0).all(), "prio written outside [B, K, N]"
        rec_sum, prefix, seen = self.rec_sum.cpu().numpy(), self.prefix.cpu().numpy(), self.seen.cpu().numpy()
        mx, mn = self.max_prio.cpu().numpy(), self.min_prio.cpu().numpy()
        assert np.isnan(rec_sum[-1]) and np.isnan(prefix[-1]) and seen[-1] == INT_GUARD and np.isnan(mx[1]) and np.isnan(mn[1])
        return dict(prio=self.prio.cpu().numpy(), rec_sum=rec_sum[:-1], prefix=prefix[:-1], seen=seen[:-1], max_prio=mx[0], min_prio=mn[0])


def sample_prio(rp, pr, batch, n_step, draw):
    from melissa_amd import _lib
    out, b = _outputs(rp, batch, weight=True)
    counter = torch.tensor([draw, INT_GUARD], dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().mel_replay_sample_prio(C.byref(rp.struct), C.byref(pr.struct), rp.B, rp.n, batch, n_step, _disc(n_step), rr.SEED,
                                                  counter.data_ptr(), C.byref(b), out["weight"].data_ptr(), _stream()),
               "mel_replay_sample_prio")
    got = _collect(out, batch)
    assert counter.tolist() == [draw + 1, INT_GUARD]
    return got


@pytest.mark.parametrize("name", list(rr.RING_CASES))
def test_uniform_sampler_equals_the_oracle(name):
    """Catches, among others: a scan that drops the ``run`` carry between chunks (the prefix comparison on every ring beyond 1 024
    records, and every sample behind the first chunk), a missing ``k >= filled`` mask (stale sets in unfilled slots shift every
    prefix behind them), a rank walk that starts in the wrong word (agents on both sides of 64 at N = 65 and 128), ``boot_obs``
    copied from ``slot`` instead of ``boot_slot`` (every walk longer than one step; all elements of obs_next are distinct)."""
    ring = _ring(name)
    rp = load_ring(ring, "cuda")
    want_prefix = rr.pair_prefix(ring)
    worst = 0.0
    for n_step in rr.RING_CASES[name]["n_steps"]:
        for i, batch in enumerate(BATCHES):
            draw = rr.DRAW0 + i
            got, prefix = sample_uniform(rp, batch, n_step, draw)
            np.testing.assert_array_equal(prefix, want_prefix)
            o = rr.uniform_oracle(ring, n_step, rr.discounts(n_step), rr.SEED, draw, batch)
            worst = max(worst, assert_walk_equal(ring, o, got, n_step))
            if i == 0:                                       # the same counter again: the same bits
                again, _ = sample_uniform(rp, batch, n_step, draw)
                for key in got:
                    assert got[key].tobytes() == again[key].tobytes(), key
    print(f"{name}: uniform sampler, largest ret deviation {worst:.3f} x 2^-24 x abs_sum")


@pytest.mark.parametrize("shape", [(3, 1, 1), (5, 3, 65), (9, 8, 128)])
def test_empty_ring_samples_index_zero(shape):
    """Every cursor 0, every array full of stale values: env = slot = agent = 0, ret 0, boot_w 1, act[0, 0, 0], obs[0, 0] | 0 - from
    both samplers, the prioritized one with weight 1 and every priority zeroed."""
    ring = rr.empty_ring(*shape, 2, neighbours=True)
    rp = load_ring(ring, "cuda")
    junk = np.full(shape, 0.25, np.float32)
    for batch in (1024, 1):
        o = rr.uniform_oracle(ring, 4, rr.discounts(4), rr.SEED, rr.DRAW0, batch)
        got, prefix = sample_uniform(rp, batch, 4, rr.DRAW0)
        assert (prefix == 0).all() and (got["env"] == 0).all() and (got["ret"] == 0).all() and (got["boot_w"] == 1).all()
        assert_walk_equal(ring, o, got, 4)
        for prio, seen in ((np.zeros(shape, np.float32), np.zeros(shape[0])), (junk, np.full(shape[0], 5))):
            pr = Priority(rp, prio, seen)
            got = sample_prio(rp, pr, batch, 4, rr.DRAW0)
            assert_walk_equal(ring, o, got, 4)
            assert (got["weight"] == 1).all()
            state = pr.read()
            assert (state["prio"] == 0).all() and (state["rec_sum"] == 0).all() and (state["prefix"] == 0).all() and (state["seen"] == 0).all()


@pytest.mark.parametrize("name", list(rr.RING_CASES))
def test_prioritized_sampler_picks_exactly(name):
    """Dyadic priorities (multiples of 2^-10 below 2^10, one transition at 2^9 among thousands at 2^-10, whole records without mass):
    every float64 sum is exact in any order, so the device's picks equal the cumsum + searchsorted restatement with no slack, and
    the record sums and prefix sums it leaves behind equal NumPy's."""
    ring = _ring(name)
    rp = load_ring(ring, "cuda")
    B, K, n = ring["B"], ring["K"], ring["n"]
    prio = rr.dyadic_prio(ring, 9)
    flat = prio.astype(np.float64).reshape(B * K, n)
    worst_ret = worst_w = 0.0
    for n_step in rr.RING_CASES[name]["n_steps"]:
        for i, (batch, beta, norm) in enumerate(zip(BATCHES + (1024,), (0.4, 0.4, 0.0, 0.0), (1, 0, 1, 0))):
            draw = rr.DRAW0 + i
            pr = Priority(rp, prio, ring["cursor"], beta=beta, weight_norm=norm)
            got = sample_prio(rp, pr, batch, n_step, draw)
            e, k, a = rr.prio_pick_oracle(prio, rr.SEED, draw, batch)
            assert (prio[e, k, a] > 0).all()
            o = rr.walk_oracle(ring, e, k, a, n_step, rr.discounts(n_step))
            worst_ret = max(worst_ret, assert_walk_equal(ring, o, got, n_step))
            w = (prio[e, k, a].astype(np.float64) / np.float64(np.float32(0.37))) ** -beta
            w = w / w.max() if norm else w
            if beta == 0.0:
                assert (got["weight"] == 1).all()
            worst_w = max(worst_w, float(np.abs(got["weight"] / w - 1).max()))
            np.testing.assert_allclose(got["weight"], w, rtol=1e-6)
            state = pr.read()
            np.testing.assert_array_equal(state["seen"], ring["cursor"])
            assert state["prio"].tobytes() == prio.tobytes() and state["max_prio"] == 3.0 and state["min_prio"] == np.float32(0.37)
            np.testing.assert_array_equal(state["rec_sum"], flat.sum(1))
            np.testing.assert_array_equal(state["prefix"], np.concatenate([[0.0], np.cumsum(flat.sum(1))]))
    print(f"{name}: prioritized sampler, largest ret deviation {worst_ret:.3f} x 2^-24 x abs_sum, weights {worst_w:.3e} relative")


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.6])
@pytest.mark.parametrize("K,n", [(5, 20), (5, 64), (5, 65), (5, 128), (1, 20), (1, 128)])
def test_refresh_launch_marks_exactly_the_written_slots(K, n, alpha):
    """Hand-set (seen, cursor) per env - written 0, 1, K - 1 across the wrap, exactly K, above K, below 0 - with max_prio = 3: fresh
    slots hold max_prio ** alpha at acting agents and 0 elsewhere, stale slots keep their value bit for bit, slots at or beyond
    min(cursor, K) are 0 whatever their stale acted bits say, and rec_sum is the float64 sum in agent order."""
    ring, seen, prio, want = refresh_case(K, n)
    rp = load_ring(ring, "cuda")
    pr = Priority(rp, prio, seen, alpha=alpha)
    sample_prio(rp, pr, 1, 4, rr.DRAW0)
    state = pr.read()
    got = state["prio"]
    init = {0.0: 1.0, 1.0: 3.0}.get(alpha)
    if init is None:
        np.testing.assert_allclose(got, want(3.0 ** 0.6), rtol=1e-6)
        init = np.float32(got[got != want(0.0)].flat[0])          # ... and one float32 value everywhere
    np.testing.assert_array_equal(got, want(init))
    np.testing.assert_array_equal(state["seen"], ring["cursor"])
    rec_sum = np.cumsum(got.astype(np.float64).reshape(-1, n), axis=1)[:, -1]      # sequential, agent order
    np.testing.assert_array_equal(state["rec_sum"], rec_sum)
    assert state["max_prio"] == 3.0 and state["min_prio"] == np.float32(0.37)


@pytest.mark.parametrize("batch", [1, 1000, 1024])
def test_write_back_keeps_the_highest_index_and_skips_what_is_outside(batch):
    """Duplicates in different wavefronts (samples 3 and batch - 24; three more spread over the batch): the highest index wins.
    Samples with env -1 / B, slot -1 / K, agent -1 / n change no element (their |td| lies inside the range of the valid ones, so
    max_prio / min_prio are the valid samples')."""
    from melissa_amd import _lib
    B, K, n = 6, 5, 70
    rng = np.random.RandomState(batch)
    ring = rr.build_ring(B, K, n, 3)
    rp = load_ring(ring, "cuda")
    prio0 = (rng.randint(1, 2 ** 20, (B, K, n)) * 2.0 ** -10).astype(np.float32)
    pr = Priority(rp, prio0, ring["cursor"], alpha=0.6, max_prio=1.0, min_prio=1.0)
    e, k, a = rng.randint(0, B, batch), rng.randint(0, K, batch), rng.randint(0, n, batch)
    td = (rng.uniform(0.01, 30.0, batch) * rng.choice([-1.0, 1.0], batch)).astype(np.float32)
    valid = np.ones(batch, bool)
    if batch > 1:
        td[0], td[1] = 30.5, -0.005                            # the extremes belong to valid samples
        for src, dst in ((3, batch - 24), (70, 200), (200, 650)):
            e[dst], k[dst], a[dst] = e[src], k[src], a[src]
        td[3] = 25.0
        for j, (be, bk, ba) in enumerate([(-1, 0, 0), (B, 0, 0), (0, K, 0), (0, 0, n), (2, -1, 3), (2, 3, -1), (B - 1, K, n)]):
            for at in (10 + j, batch - 10 - j):
                e[at], k[at], a[at], valid[at] = be, bk, ba, False
        keys = (e * K + k) * n + a
        last = int(np.flatnonzero(valid & (keys == keys[3]))[-1])  # (a random sample behind batch - 24 may name it once more)
        assert last >= batch - 24 and last // 64 != 3 // 64
        td[last] = 0.02
    dev = lambda x, t: torch.from_numpy(np.concatenate([x, [INT_GUARD]]).astype(t)).cuda()
    de, dk, da, dtd = dev(e, np.int64), dev(k, np.int64), dev(a, np.int64), dev(td, np.float32)
    _lib.check(_lib.load().mel_replay_update_priority(C.byref(pr.struct), B, K, n, batch, de.data_ptr(), dk.data_ptr(), da.data_ptr(),
                                                      dtd.data_ptr(), _stream()), "mel_replay_update_priority")
    state = pr.read()
    ref = PrioOracle((B, K, n), alpha=0.6)
    ref.tree = prio0.astype(np.float64).reshape(-1)
    idx = ref.flat(e[valid], k[valid], a[valid])
    ref.update_weight(idx, td[valid])                          # (numpy keeps the last of a repeated index)
    touched = np.zeros(B * K * n, bool)
    touched[idx] = True
    got = state["prio"].reshape(-1)
    assert got[~touched].tobytes() == prio0.reshape(-1)[~touched].tobytes()
    np.testing.assert_allclose(got[touched], ref.tree[touched], rtol=1e-6)
    print(f"batch {batch}: priorities {np.abs(got[touched] / ref.tree[touched] - 1).max():.3e} relative")
    p_all = np.abs(td) + EPS
    assert float(p_all.max()) == ref.max_prio or batch == 1
    assert state["max_prio"] == np.float32(ref.max_prio) and state["min_prio"] == np.float32(ref.min_prio)
    if batch > 1:
        dup = ref.flat(e[3], k[3], a[3])
        np.testing.assert_allclose(got[dup], (np.float32(0.02) + EPS) ** np.float32(0.6), rtol=1e-6)
        assert state["max_prio"] == np.float32(30.5) + EPS and state["min_prio"] == np.float32(0.005) + EPS
