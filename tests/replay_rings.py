"""Hand-built replay rings and bit-for-bit oracles of the two device samplers (csrc/env.hip ``replay_sample_kernel``,
csrc/replay_prio.hpp).  NumPy and Python integers only: no torch, no library.

``build_ring`` scripts the states the round loop only produces by luck - rings that are not full, envs that never wrote, stale
sets in unfilled slots, walks that wrap from slot K - 1 to 0 and stop at the newest record, agents 63 / 64 / 127 - and
``uniform_oracle`` / ``prio_pick_oracle`` restate the documented draws (include/melissa_hip.h) so every sample can be compared
exactly."""
import numpy as np

from tests.prio_oracle import MASK64, PrioOracle, draw_u

CHUNK = 1024                                                   # records per scan chunk of the uniform sampler
CLASSES = ("full", "done", "stopped", "episode", "newest")
FULL, DONE, STOPPED, EPISODE, NEWEST, EMPTY = range(6)


SEED = (1 << 63) | 0x5DEECE66D1234567                          # sampler seed (bit 63 set) and first draw counter (past 2^32)
DRAW0 = (1 << 40) + 3
GAMMA = 0.99

# The rings the device tests sample, smallest that reach each branch: (B, K, n) -> ring seed, the n_step values, both ends empty.
# tests/test_replay_rings.py checks, without a GPU, that each of them produces what the device tests rely on.
RING_CASES = {
    "3x1x1": dict(shape=(3, 1, 1), ring_seed=1, n_steps=(4, 1)),                  # smallest ring
    "5x3x65": dict(shape=(5, 3, 65), ring_seed=1, n_steps=(4, 16)),               # K < n_step
    "9x8x128": dict(shape=(9, 8, 128), ring_seed=1, n_steps=(4, 1, 16)),          # N = 128
    "32x32x20": dict(shape=(32, 32, 20), ring_seed=1, n_steps=(4,)),              # exactly one chunk
    "41x25x20": dict(shape=(41, 25, 20), ring_seed=1, n_steps=(4,)),              # one record into the second chunk
    "41x25x20-ends": dict(shape=(41, 25, 20), ring_seed=1, n_steps=(4,), empty_ends=False),
    "37x29x128": dict(shape=(37, 29, 128), ring_seed=1, n_steps=(4,)),            # second chunk with N = 128
    "128x128x3": dict(shape=(128, 128, 3), ring_seed=1, n_steps=(4,)),            # exactly one pass of sixteen chunks
    "5x3277x3": dict(shape=(5, 3277, 3), ring_seed=1, n_steps=(4,)),              # one record into the second pass
    "5x3277x3-ends": dict(shape=(5, 3277, 3), ring_seed=1, n_steps=(4,), empty_ends=False),
    "700x25x7": dict(shape=(700, 25, 7), ring_seed=1, n_steps=(4,)),              # well into the second pass
}


def case_ring(name):
    c = RING_CASES[name]
    return build_ring(*c["shape"], c["ring_seed"], neighbours=True, empty_ends=c.get("empty_ends", True))


def discounts(n_step, gamma=GAMMA) -> np.ndarray:
    """float32 gamma^j, j = 0 .. n_step: what the host passes to the launch."""
    return np.array([gamma ** j for j in range(n_step + 1)], np.float32)


def pack_sets(bits: np.ndarray) -> np.ndarray:
    """bool [..., n] -> uint64 [..., W], bit i of word w = member 64 w + i."""
    n = bits.shape[-1]
    W = (n + 63) // 64
    out = np.zeros(bits.shape[:-1] + (W,), np.uint64)
    for i in range(n):
        out[..., i // 64] |= bits[..., i].astype(np.uint64) << np.uint64(i % 64)
    return out


def lanes_of(n: int) -> list:
    """The scripted agents: the first, the last, and both sides of the word boundary."""
    return sorted({0, n - 1} | {a for a in (63, 64) if a < n})


def build_ring(B, K, n, seed, neighbours=False, empty_ends=True):
    """Every field of ``mel_round_replay`` as NumPy arrays; node sets both as bool (``acted_bool`` [B, K, n]) and packed
    (``acted`` uint64 [B, K, W]).

    * cursors from {0, 1, K - 1, K, K + 1, 3 K + 2}; env 0, env B - 1 and (from five envs on) the middle env are empty unless
      ``empty_ends`` is off, which gives both ends 3 K + 2 rounds so that the first and the last record can be sampled;
    * slots at or beyond min(cursor, K) hold plausible garbage: random sets, the env's newest episode, non-zero values;
    * ``episode`` never decreases in write order; rings that went round keep one episode over their last four writes, so the steady
      lane's walks from K - 2 and K - 1 wrap to slot 0 and stop at the newest record;
    * the scripted lanes (``lanes_of``) are steady / done every p-th round / silent every p-th round / random, rotating over envs;
      the other agents act with probability 0.5 and are done with probability 0.1;
    * some filled records have no acting agent at all (equal prefixes for the binary search) - most of them where K is large, so
      that the few walks that wrap keep a share of the draws;
    * ``rew`` = sign * exp(U(-7, 7)); ``obs`` / ``obs_next`` hold a distinct integer in every element."""
    rng = np.random.RandomState(seed)
    W = (n + 63) // 64
    lanes = lanes_of(n)
    cursor = np.zeros(B, np.int64)
    empty = {0, B - 1} | ({B // 2} if B >= 5 else set()) if empty_ends else set()
    cycle = [3 * K + 2, K, K - 1, 3 * K + 2, K + 1, 1, 3 * K + 2, 0]
    inner = [b for b in range(B) if b not in empty]
    for j, b in enumerate(inner):
        cursor[b] = cycle[j % len(cycle)]
    if not empty_ends:
        cursor[0] = cursor[B - 1] = 3 * K + 2
    filled = np.minimum(cursor, K)

    acted = rng.rand(B, K, n) < 0.5
    done = rng.rand(B, K, n) < 0.1
    episode = np.zeros((B, K), np.int32)
    p_quiet = max(0.0, 1.0 - 48.0 / K)                         # large K: whole blocks of eight rounds in which nobody acted
    for b in range(B):
        c, f = int(cursor[b]), int(filled[b])
        ep = int(rng.randint(0, 1000))
        quiet = rng.rand(c // 8 + 1) < p_quiet
        for t in range(c - f, c):                              # write order: round t went to slot t % K
            s = t % K
            last4 = c > K and t >= c - 4
            if t > c - f and not last4 and rng.rand() < 0.2:
                ep += 1
            episode[b, s] = ep
            for li, a in enumerate(lanes):
                pat = 0 if (c == 3 * K + 2 and li == b % len(lanes)) else (b + li) % 4
                p = 2 + (b // 4) % 4
                if pat == 0:
                    acted[b, s, a], done[b, s, a] = True, False
                elif pat == 1:
                    acted[b, s, a], done[b, s, a] = True, t % p == p - 1
                elif pat == 2:
                    acted[b, s, a], done[b, s, a] = t % p != p - 1, False
                else:
                    acted[b, s, a], done[b, s, a] = rng.rand() < 0.9, rng.rand() < 0.1
            if not last4 and (quiet[t // 8] or rng.rand() < 0.08):
                acted[b, s] = False
        episode[b, f:] = ep                                    # garbage slots: the newest episode, random sets
    done &= acted | (np.arange(K)[None, :, None] >= filled[:, None, None])     # (a filled record's done set is a subset of acted)
    rew = (rng.choice([-1.0, 1.0], (B, K, n)) * np.exp(rng.uniform(-7, 7, (B, K, n)))).astype(np.float32)
    act = rng.randint(0, 4, (B, K, n)).astype(np.int8)
    idx = np.arange(B * K * 8 * n, dtype=np.int64)
    obs = (1 + idx % (2 ** 24 - 1)).astype(np.float32).reshape(B, K, 8 * n)
    obs_next = (1 + (idx + 5_000_011) % (2 ** 24 - 1)).astype(np.float32).reshape(B, K, 8 * n)
    ring = dict(B=B, K=K, n=n, W=W, cursor=cursor.astype(np.int32), obs=obs, obs_next=obs_next, acted_bool=acted, done_bool=done,
                acted=pack_sets(acted), done=pack_sets(done), act=act, rew=rew, episode=episode)
    if neighbours:
        nb = rng.rand(B, K, n, n) < 0.3
        ring.update(active_nb_bool=nb, active_nb=pack_sets(nb))
    return ring


def empty_ring(B, K, n, seed, neighbours=False):
    """``build_ring`` with every cursor at 0: all of its contents are stale."""
    ring = build_ring(B, K, n, seed, neighbours=neighbours)
    ring["cursor"] = np.zeros(B, np.int32)
    return ring


def splitmix(seed: int, draw: int, i: int) -> int:
    """The samplers' draw bits for sample ``i``: splitmix64 of seed, draw counter and sample index (Python integers)."""
    z = (seed + draw * 0x9E3779B97F4A7C15 + (i + 1) * 0xD1B54A32D192ED03) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def pair_prefix(ring) -> np.ndarray:
    """int64 [B K + 1]: exclusive prefix sums of the (record, acting agent) pair counts, unfilled slots masked; [-1] = total."""
    B, K = ring["B"], ring["K"]
    filled = np.minimum(ring["cursor"].astype(np.int64), K)
    cnt = ring["acted_bool"].sum(-1) * (np.arange(K)[None, :] < filled[:, None])
    return np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)


def walk_oracle(ring, env, slot, agent, n_step, disc_f32):
    """The n-step walk of the picked transitions, vectorised over the picks: dict of act, boot_slot, boot_w (float32), ret
    (float64 from the float32 discounts and rewards), abs_sum = sum |disc_j rew_j|, cls (FULL ... NEWEST), wrapped[, nb_sibling]."""
    K = ring["K"]
    e, k, a = (np.asarray(x, np.int64) for x in (env, slot, agent))
    cur = ring["cursor"].astype(np.int64)
    filled, newest = np.minimum(cur, K)[e], ((cur - 1) % K)[e]
    disc = np.asarray(disc_f32, np.float32)
    assert disc.dtype == np.float32 and disc.size == n_step + 1
    ep0 = ring["episode"][e, k]
    alive = np.ones(e.size, bool)
    ret, abs_sum = np.zeros(e.size, np.float64), np.zeros(e.size, np.float64)
    boot, bw = k.copy(), np.ones(e.size, np.float32)
    cls = np.full(e.size, FULL, np.int64)
    kk = k.copy()
    for j in range(n_step):
        same = ring["episode"][e, kk] == ep0
        ok = alive & same & ring["acted_bool"][e, kk, a] & (kk < filled)
        cls = np.where(alive & ~ok, np.where(same, STOPPED, EPISODE), cls)
        term = np.float64(disc[j]) * ring["rew"][e, kk, a].astype(np.float64)
        ret, abs_sum = ret + np.where(ok, term, 0.0), abs_sum + np.where(ok, np.abs(term), 0.0)
        boot, bw = np.where(ok, kk, boot), np.where(ok, disc[j + 1], bw)
        fin = ok & ring["done_bool"][e, kk, a]
        bw = np.where(fin, np.float32(0), bw).astype(np.float32)
        cls = np.where(fin, DONE, cls)
        if j < n_step - 1:
            cls = np.where(ok & ~fin & (kk == newest), NEWEST, cls)
        alive = ok & ~fin & (kk != newest)
        kk = (kk + 1) % K
    out = dict(env=e, slot=k, agent=a, act=ring["act"][e, k, a].astype(np.int64), boot_slot=boot, boot_w=bw, ret=ret,
               abs_sum=abs_sum, cls=cls, wrapped=boot < k)
    if "active_nb" in ring:
        self_bit = pack_sets(np.arange(ring["n"])[None, :] == a[:, None])
        out["nb_sibling"] = ring["acted"][e, k] & (ring["active_nb"][e, k, a] | self_bit)
    return out


def batch_rows(ring, o):
    """obs / boot_obs float32 [batch, 8 n + 1] of an oracle batch: the record's obs | agent id, obs_next[boot_slot] | agent id."""
    col = o["agent"].astype(np.float32)[:, None]
    return (np.concatenate([ring["obs"][o["env"], o["slot"]], col], 1),
            np.concatenate([ring["obs_next"][o["env"], o["boot_slot"]], col], 1))


def uniform_oracle(ring, n_step, disc_f32, seed, draw, batch):
    """``mel_replay_sample`` restated: pick = ((z >> 32) * total) >> 32 in Python integers, the record by searchsorted over the
    integer prefix sums, the agent as the rank-th member of its acted set, then the walk.  An empty ring gives index 0, ret 0,
    boot_w 1 (cls EMPTY)."""
    K = ring["K"]
    prefix = pair_prefix(ring)
    total = int(prefix[-1])
    if total == 0:
        z = np.zeros(batch, np.int64)
        out = dict(env=z, slot=z, agent=z, act=np.full(batch, int(ring["act"][0, 0, 0]), np.int64), boot_slot=z,
                   boot_w=np.ones(batch, np.float32), ret=np.zeros(batch), abs_sum=np.zeros(batch),
                   cls=np.full(batch, EMPTY, np.int64), wrapped=np.zeros(batch, bool))
        if "active_nb" in ring:
            out["nb_sibling"] = np.broadcast_to(ring["acted"][0, 0] & (ring["active_nb"][0, 0, 0] | pack_sets(np.arange(ring["n"]) == 0)),
                                                (batch, ring["W"])).copy()
        return out
    env, slot, agent = [], [], []
    for i in range(batch):
        pick = ((splitmix(seed, draw, i) >> 32) * total) >> 32
        rec = int(np.searchsorted(prefix, pick, side="right")) - 1
        rank = pick - int(prefix[rec])
        e, k = divmod(rec, K)
        env.append(e), slot.append(k), agent.append(int(np.flatnonzero(ring["acted_bool"][e, k])[rank]))
    return walk_oracle(ring, env, slot, agent, n_step, disc_f32)


def prio_pick_oracle(prio, seed, draw, batch):
    """``mel_replay_sample_prio``'s picks in float64: target = u * prio.sum(), the first transition in buffer order whose inclusive
    cumsum exceeds it.  Exact for dyadic priorities (every float64 sum is exact in any order).  Returns env, slot, agent."""
    prio = np.asarray(prio)
    _, K, n = prio.shape
    ref = PrioOracle(prio.shape)
    ref.tree = prio.astype(np.float64).reshape(-1)
    idx = ref.index_of(draw_u(seed, draw, batch) * ref.tree.sum())
    return idx // (K * n), (idx // n) % K, idx % n


def dyadic_prio(ring, seed):
    """float32 [B, K, n] priorities for the exact-pick test: multiples of 2^-10 below 2^10 on acting agents of filled slots, 0 on
    unfilled slots, non-acting agents and whole records in the middle and at both ends of the filled part; most at 2^-10, some
    larger, one at 2^9."""
    rng = np.random.RandomState(seed)
    B, K, n = ring["B"], ring["K"], ring["n"]
    filled = np.minimum(ring["cursor"].astype(np.int64), K)
    live = ring["acted_bool"] & (np.arange(K)[None, :, None] < filled[:, None, None])
    p = np.where(rng.rand(B, K, n) < 0.9, 1, rng.randint(1, 2 ** 20, (B, K, n))).astype(np.float64) * 2.0 ** -10
    p = np.where(live, p, 0.0).reshape(B * K, n)
    recs = np.flatnonzero(p.sum(1) > 0)
    if recs.size > 8:                                          # whole records without mass: both ends, a run in the middle
        mid = recs.size // 2
        p[recs[[0, -1]]] = 0.0
        p[recs[mid:mid + 3]] = 0.0
    nz = np.flatnonzero(p.reshape(-1) > 0)
    if nz.size:
        p.reshape(-1)[nz[(2 * nz.size) // 3]] = 2.0 ** 9
    out = p.reshape(B, K, n).astype(np.float32)
    assert (out.astype(np.float64) == p.reshape(B, K, n)).all() and out.max() < 2.0 ** 10
    return out


def fresh_slots(seen, cursor, K) -> np.ndarray:
    """bool [B, K]: the slots a refresh initialises.  A slot is fresh when the env wrote it since ``seen`` - slots seen ..
    cursor - 1 mod K, every slot once ``written >= K`` or ``written < 0`` (a cursor that went back: the ring was reset) - and a
    slot at or beyond min(cursor, K) never is."""
    seen, cursor = np.asarray(seen, np.int64), np.asarray(cursor, np.int64)
    fresh = np.zeros((seen.size, K), bool)
    for b, (s, c) in enumerate(zip(seen.tolist(), cursor.tolist())):
        written = c - s
        if written >= K or written < 0:
            fresh[b] = True
        else:
            fresh[b, [t % K for t in range(s, c)]] = True
        fresh[b, min(c, K):] = False
    return fresh
