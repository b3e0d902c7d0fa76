"""NumPy restatement of [3P] tianshou 1.0.0 ``PrioritizedReplayBuffer`` as the reference's scripts use it with ``--prio-buffer``
(l_dgn.py:169-176), over the transitions of a round replay.  Parity unpinned: tianshou is not installed here, the rules are
restated from its published behaviour (data/buffer/prio.py, segtree.py, policy/base.py:post_process_fn).

The tree is a flat float64 array in buffer order - (env, slot, agent) ascending, the memory order of a dense [B, K, N] array in
which agents that did not act and slots not yet filled hold 0 - and ``get_prefix_sum_idx`` is cumsum + searchsorted(side="right"):
the first transition whose inclusive prefix sum exceeds the scalar."""
import numpy as np

EPS = np.finfo(np.float32).eps
MASK64 = (1 << 64) - 1


class PrioOracle:
    def __init__(self, shape, alpha=0.6, beta=0.4, weight_norm=True):
        self.shape = tuple(shape)                                  # (B, K, N)
        self.alpha, self.beta, self.weight_norm = alpha, beta, weight_norm
        self.tree = np.zeros(int(np.prod(shape)), np.float64)
        self.max_prio = self.min_prio = 1.0

    def flat(self, env, slot, agent):
        _, K, N = self.shape
        return (np.asarray(env, np.int64) * K + np.asarray(slot, np.int64)) * N + np.asarray(agent, np.int64)

    def add(self, index):
        """init_weight: a new transition enters with max_prio ** alpha."""
        self.tree[index] = np.float32(self.max_prio) ** np.float32(self.alpha)

    def add_records(self, acted_bool, records):
        """``acted_bool`` [B, K, N]; ``records``: iterable of (env, slot) just written - their acting agents are added, the
        others of the record hold 0 (they are no transitions)."""
        _, K, N = self.shape
        for e, k in records:
            base = (e * K + k) * N
            self.tree[base:base + N] = 0.0
            self.add(base + np.nonzero(acted_bool[e, k])[0])

    def index_of(self, scalar):
        """get_prefix_sum_idx for an array of scalars in [0, tree.sum())."""
        return np.searchsorted(np.cumsum(self.tree), scalar, side="right")

    def sample_index(self, batch, rng):
        return self.index_of(rng.random(batch) * self.tree.sum())

    def get_weight(self, index):
        """(tree[index] / min_prio) ** -beta - the numerator already is p ** alpha, the denominator the raw min_prio (upstream's
        "simplified formula") - then / max over the batch (weight_norm, the default)."""
        w = (self.tree[index] / self.min_prio) ** (-self.beta)
        return w / w.max() if self.weight_norm else w

    def update_weight(self, index, td):
        p = np.abs(np.asarray(td, np.float32)) + EPS               # float32
        self.tree[np.asarray(index)] = p ** np.float32(self.alpha)  # (numpy keeps the LAST occurrence of a repeated index)
        self.max_prio = max(self.max_prio, float(p.max()))
        self.min_prio = min(self.min_prio, float(p.min()))


def draw_u(seed, draw, batch):
    """The device sampler's uniforms: splitmix64 of (seed, draw counter, sample index), u = (z >> 11) * 2^-53."""
    out = np.empty(batch, np.float64)
    for i in range(batch):
        z = (seed + draw * 0x9E3779B97F4A7C15 + (i + 1) * 0xD1B54A32D192ED03) & MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        z ^= z >> 31
        out[i] = (z >> 11) * 2.0 ** -53
    return out
