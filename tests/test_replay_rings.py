"""The hand-built rings and sampler oracles of tests/replay_rings.py, checked without a GPU: the oracle's walk against
``RoundReplay._walk_host``, the properties the device tests (tests/test_gpu_replay_rings.py) rely on for each of their rings and
seeds, and ``PrioritizedRoundReplay.refresh()`` against a NumPy restatement of which slots are fresh."""
import functools

import numpy as np
import pytest
import torch

from melissa_amd.replay import PrioritizedRoundReplay, RoundReplay
from tests import replay_rings as rr


def load_ring(ring, device="cpu", cls=RoundReplay, **kw):
    """A (Prioritized)RoundReplay on ``device`` holding the ring."""
    rp = cls(ring["B"], ring["n"], ring["K"], device, neighbours="active_nb" in ring, **kw)
    for name in ("obs", "obs_next", "act", "rew", "episode", "cursor"):
        getattr(rp, name).copy_(torch.from_numpy(ring[name]))
    for name in ("acted", "done") + (("active_nb",) if "active_nb" in ring else ()):
        t = getattr(rp, name)
        t.copy_(torch.from_numpy(ring[name].view(np.int64)).reshape(t.shape))
    return rp


@functools.lru_cache(maxsize=None)
def _ring(name):
    return rr.case_ring(name)


def _all_pairs(ring):
    filled = np.minimum(ring["cursor"].astype(np.int64), ring["K"])
    live = ring["acted_bool"] & (np.arange(ring["K"])[None, :, None] < filled[:, None, None])
    return np.nonzero(live)


RET_BOUND = lambda n_step, abs_sum: (n_step + 2) * 2.0 ** -24 * abs_sum


def assert_walk_equal(ring, o, got, n_step):
    """A sampler's batch ``got`` (NumPy arrays) against the oracle batch ``o``: everything exact, ``ret`` within
    (n_step + 2) * 2^-24 * sum |disc_j rew_j| - at most one rounding per product (none when contracted to an FMA) and one per
    addition, each against a partial sum of at most abs_sum.  Returns the largest |ret - ret64| in units of 2^-24 * abs_sum."""
    obs, boot_obs = rr.batch_rows(ring, o)
    for key in ("env", "slot", "agent"):
        if key in got:
            np.testing.assert_array_equal(got[key], o[key], err_msg=key)
    np.testing.assert_array_equal(got["act"], o["act"], err_msg="act")
    assert got["boot_w"].dtype == np.float32
    np.testing.assert_array_equal(got["boot_w"], o["boot_w"], err_msg="boot_w")
    np.testing.assert_array_equal(got["obs"], obs, err_msg="obs")
    np.testing.assert_array_equal(got["boot_obs"], boot_obs, err_msg="boot_obs")
    if "nb_sibling" in o:
        np.testing.assert_array_equal(got["nb_sibling"].reshape(len(o["env"]), -1).view(np.uint64), o["nb_sibling"], err_msg="nb_sibling")
    assert got["ret"].dtype == np.float32
    err = np.abs(got["ret"].astype(np.float64) - o["ret"])
    bound = RET_BOUND(n_step, o["abs_sum"])
    worst = float((err / np.where(o["abs_sum"] > 0, 2.0 ** -24 * o["abs_sum"], 1.0)).max())
    print(f"ret: largest deviation {worst:.3f} x 2^-24 x abs_sum (bound {n_step + 2})")
    assert (err <= bound).all(), (float((err - bound).max()), worst)
    return worst


@pytest.mark.parametrize("name", list(rr.RING_CASES) + ["empty"])
def test_oracle_walk_equals_the_host_walk(name):
    ring = rr.empty_ring(5, 3, 65, 2, neighbours=True) if name == "empty" else _ring(name)
    rp = load_ring(ring)
    prp = load_ring(ring, cls=PrioritizedRoundReplay)
    for n_step in (4, 1, 16) if name == "empty" else rr.RING_CASES[name]["n_steps"]:
        o = rr.uniform_oracle(ring, n_step, rr.discounts(n_step), rr.SEED, rr.DRAW0, 1024)
        if name == "empty":
            assert (o["env"] == 0).all() and (o["ret"] == 0).all() and (o["boot_w"] == 1).all() and (o["cls"] == rr.EMPTY).all()
        else:
            assert ring["acted_bool"][o["env"], o["slot"], o["agent"]].all()
            assert (o["slot"] < np.minimum(ring["cursor"], ring["K"])[o["env"]]).all()
        for host in (rp, prp):
            got = host._walk_host(*(torch.from_numpy(o[k]) for k in ("env", "slot", "agent")), n_step, rr.GAMMA)
            assert_walk_equal(ring, o, {k: v.numpy() for k, v in got.items()}, n_step)


@pytest.mark.parametrize("name", list(rr.RING_CASES))
def test_rings_produce_what_the_device_tests_rely_on(name):
    """With the device tests' seed, draw counter and batch 1 024: every ending class the ring can produce has at least 8 samples,
    so do walks that wrap on rings that went round, samples fall into the first and the last 1 024-record chunk, and for N > 64
    into both words.  Env 0 and env B - 1 are empty on the standard rings, so there "first" and "last" are the first and last chunk
    that holds a transition (the ``-ends`` rings take the chunks of record 0 and record B K - 1); the device tests compare the whole
    prefix scratch, which covers the records behind."""
    ring, case = _ring(name), rr.RING_CASES[name]
    B, K, n = case["shape"]
    cur = ring["cursor"]
    ends = case.get("empty_ends", True)
    assert (cur[0] == 0 and cur[B - 1] == 0 and (B < 5 or cur[B // 2] == 0)) == ends
    assert set(cur.tolist()) <= {0, 1, K - 1, K, K + 1, 3 * K + 2}
    filled = np.minimum(cur, K)
    assert all((ring["rew"] != 0).all() and (ring[x] != 0).all() for x in ("obs", "obs_next"))
    for b in range(B):
        assert (ring["episode"][b, filled[b]:] == ring["episode"][b, (cur[b] - 1) % K]).all() or cur[b] == 0
        order = [t % K for t in range(cur[b] - filled[b], cur[b])]
        assert (np.diff(ring["episode"][b, order]) >= 0).all()
    if (filled < K).any() and (filled > 0).any() and K > 1:
        stale = np.arange(K)[None, :] >= filled[:, None]
        assert ring["acted_bool"][stale].any() and (ring["done_bool"][stale].any() or stale.sum() * n < 64)
    prefix = rr.pair_prefix(ring)
    assert prefix[-1] > 0
    if B * K >= 64:                                              # filled records without pairs: equal prefixes
        cnt = np.diff(prefix).reshape(B, K)
        assert ((cnt == 0) & (np.arange(K)[None, :] < filled[:, None])).any()
    e, k, a = _all_pairs(ring)
    for n_step in case["n_steps"]:
        disc = rr.discounts(n_step)
        possible = rr.walk_oracle(ring, e, k, a, n_step, disc)
        o = rr.uniform_oracle(ring, n_step, disc, rr.SEED, rr.DRAW0, 1024)
        counts = {rr.CLASSES[c]: int((o["cls"] == c).sum()) for c in sorted(set(possible["cls"].tolist()))}
        print(name, n_step, counts, "wrapped", int(o["wrapped"].sum()), "of", int(possible["wrapped"].sum()), "pairs that wrap")
        assert min(counts.values()) >= 8, counts
        if (cur > K).any() and K > 1 and n_step > 1:                # (one step never leaves its slot)
            assert int(o["wrapped"].sum()) >= 8
        if n_step == 4 and K >= 4:
            assert set(counts) == set(rr.CLASSES)
        rec = o["env"] * K + o["slot"]
        if ends:
            has = np.flatnonzero(np.diff(prefix) > 0)
            first, last = has[0] // rr.CHUNK, has[-1] // rr.CHUNK
        else:
            first, last = 0, (B * K - 1) // rr.CHUNK
        assert (rec // rr.CHUNK == first).any() and (rec // rr.CHUNK == last).any()
        if n > 64:
            assert (o["agent"] < 64).any() and (o["agent"] >= 64).any()
            assert set(rr.lanes_of(n)) <= set(o["agent"].tolist())            # both sides of the word boundary, first and last


REFRESH_K5 = [(7, 7), (7, 8), (8, 12), (4, 9), (2, 13), (9, 3), (9, 0), (0, 2), (0, 0), (3, 4), (12, 11)]
REFRESH_K1 = [(0, 0), (0, 1), (1, 1), (3, 5), (5, 1), (2, 0), (1, 2)]


def refresh_case(K, n, seed=4):
    """A ring with hand-set (seen, cursor) per env - written 0, 1, K - 1 across the wrap, exactly K, above K, below 0, with and
    without unfilled slots - dyadic junk in every priority, and the priorities a refresh must leave: the init value at the acting
    agents of fresh slots, the junk in stale slots, 0 in slots at or beyond min(cursor, K).  Returns ring, seen, prio, want(init)."""
    pairs = REFRESH_K1 if K == 1 else REFRESH_K5
    assert K in (1, 5)
    ring = rr.build_ring(len(pairs), K, n, seed, neighbours=False)
    seen = np.array([p[0] for p in pairs], np.int32)
    ring["cursor"] = np.array([p[1] for p in pairs], np.int32)
    rng = np.random.RandomState(seed)
    prio = (rng.randint(1, 2 ** 20, (len(pairs), K, n)) * 2.0 ** -10).astype(np.float32)
    fresh = rr.fresh_slots(seen, ring["cursor"], K)
    unfilled = np.arange(K)[None, :] >= np.minimum(ring["cursor"], K)[:, None]
    assert not (fresh & unfilled).any()

    def want(init):
        new = np.where(ring["acted_bool"], np.float32(init), np.float32(0))
        return np.where(unfilled[:, :, None], np.float32(0), np.where(fresh[:, :, None], new, prio))

    return ring, seen, prio, want


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.6])
@pytest.mark.parametrize("K,n", [(5, 20), (5, 64), (5, 65), (5, 128), (1, 20), (1, 128)])
def test_host_refresh_marks_exactly_the_written_slots(K, n, alpha):
    ring, seen, prio, want = refresh_case(K, n)
    rp = load_ring(ring, cls=PrioritizedRoundReplay, alpha=alpha)
    rp.seen.copy_(torch.from_numpy(seen))
    rp.prio.copy_(torch.from_numpy(prio))
    rp.max_prio.fill_(3.0)
    rp.refresh()
    got = rp.prio.numpy()
    init = {0.0: 1.0, 1.0: 3.0}.get(alpha)
    if init is None:
        init = 3.0 ** 0.6
        np.testing.assert_allclose(got, want(init), rtol=1e-6)
        init = np.float32(got[got != want(0.0)].flat[0])          # ... and one float32 value everywhere
    np.testing.assert_array_equal(got, want(init))
    assert torch.equal(rp.seen, rp.cursor)
