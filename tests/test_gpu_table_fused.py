"""GPU tests of the node-feature table evaluated inside the plan launch (csrc/gemm_table.hpp): a workgroup makes the encoder
rows of 32 feature tuples, keeps them in LDS and runs 256 conv1 columns on them, so a forward spends no launch on the table.
Same instruction, same k order, same fp32 encoder rows as the two-launch form (mel_prepare_feature_tables), so every bar
here is BIT-IDENTITY with that form."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})
HIDDEN, HC = 128, 512
SENTINEL = 0xA5
TAIL = 4096             # bytes behind the carved tables that must stay untouched


def env_like_obs(n, bs, seed, index_col=True):
    """Observation rows with GraphEnv's feature ranges (graph.py:261-269)."""
    rng = np.random.RandomState(seed)
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, n, size=(bs, n))           # degree
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))           # messages transmitted
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))      # last action, interested, has message
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.1)
    obs[:, -1] = rng.randint(0, n, size=bs)
    return obs if index_col else obs[:, :-1].copy()


def agent_sets(n, bs, seed):
    """A few controlling agents per env as bit patterns: int64 [bs], [bs, 2] words beyond 64 nodes."""
    rng = np.random.RandomState(seed)
    words = 1 if n <= 64 else 2
    mask = np.zeros((bs, words), dtype=np.uint64)
    for b in range(bs):
        for a in rng.choice(n, size=rng.randint(1, min(n, 6) + 1), replace=False):
            mask[b, a // 64] |= np.uint64(1) << np.uint64(a % 64)
    return mask.view(np.int64).reshape(bs) if words == 1 else mask.view(np.int64)


def make(model, n, dtype, seed=9):
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    sd = no.init_weights(model, seed=seed, random_conv_bias=True)
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator="max") if model == "hl_dgn" else {}
    net = cls(5, HIDDEN, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip", **kw)
    net.load_state_dict(sd)
    net.set_feature_dtype(dtype)
    return net


def weights_of(net):
    w = net._weights()
    net._refresh_prepared(w, torch.device("cuda"))     # f32a: the planes the struct must carry (the table does not read them)
    w.tables, w.tables_nodes = None, 0
    return w


# n = 7: T = 280, eight full blocks of 32 rows and one of 24 (four of 64 and 24); n = 20: T = 800, 25 blocks (a half block of
# the 64-row tiles); n = 50: T = 2 000, a 16-row last block; n = 100: T = 4 000, the table of plan_enc_kernel<2>
@pytest.mark.parametrize("dtype", ["f32", "f32a"])
@pytest.mark.parametrize("n", [7, 20, 50, 100])
def test_fused_tables_equal_two_launch_tables_byte_for_byte(n, dtype):
    from melissa_amd import _lib
    lib = _lib.load()
    net = make("l_dgn", n, dtype)
    w = weights_of(net)
    T = n * 40
    need = int(lib.mel_feature_tables_bytes(C.byref(w), n))
    assert need == T * (HIDDEN + 2 * HC) * 4
    stream = _lib.current_stream_ptr(torch.device("cuda"))
    bufs = []
    for fn in (lib.mel_prepare_feature_tables, lib.mel_feature_tables_fused):
        buf = torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
        _lib.check(fn(C.byref(w), n, buf.data_ptr(), need, stream), fn.__name__)
        bufs.append(buf)
    torch.cuda.synchronize()
    two, one = bufs
    assert two.data_ptr() != one.data_ptr()
    off = 0
    for name, width in (("t_h0", HIDDEN), ("t_xl", HC), ("t_xr", HC)):
        a = two[off:off + T * width * 4].view(torch.float32).view(T, width)
        b = one[off:off + T * width * 4].view(torch.float32).view(T, width)
        assert torch.isfinite(a).all(), name            # the reference rows were written (no sentinel bit patterns left)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"{name}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} words differ, first rows " \
            f"{torch.nonzero((a.view(torch.int32) != b.view(torch.int32)).any(dim=1)).flatten()[:8].tolist()}"
        off += T * width * 4
    assert off == need
    for buf in bufs:
        assert bool((buf[need:] == SENTINEL).all())
    assert torch.equal(two, one)


def test_fused_entry_point_refuses_what_the_forward_keeps_in_two_launches():
    from melissa_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream_ptr(torch.device("cuda"))
    for model, dtype in (("l_dgn", "bf16"), ("l_dgn", "f32s"), ("dgn_r", "f32"), ("hl_dgn", "f32")):
        net = make(model, 20, dtype)
        w = weights_of(net)
        need = int(lib.mel_feature_tables_bytes(C.byref(w), 20))
        buf = torch.full((need,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert lib.mel_feature_tables_fused(C.byref(w), 20, buf.data_ptr(), need, stream) == -3, (model, dtype)   # MEL_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
    net = make("l_dgn", 20, "f32")
    w = weights_of(net)
    need = int(lib.mel_feature_tables_bytes(C.byref(w), 20))
    buf = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.mel_feature_tables_fused(C.byref(w), 20, buf.data_ptr(), need - 1, stream) == -4                   # MEL_ERR_WORKSPACE


def launches_by_stage(fn):
    """Launch groups per stage (the library's stage timer, mel_prof_*) of the forwards ``fn`` issues."""
    from melissa_amd import _lib
    lib = _lib.load()
    prof = lib.mel_prof_create(64)
    lib.mel_prof_attach(prof)
    try:
        fn()
    finally:
        lib.mel_prof_attach(None)
    torch.cuda.synchronize()
    ms, cnt = (C.c_double * _lib.N_STAGES)(), (C.c_int64 * _lib.N_STAGES)()
    lib.mel_prof_read(prof, ms, cnt)
    lib.mel_prof_destroy(prof)
    return {name: int(cnt[i]) for i, name in enumerate(_lib.STAGE_NAMES)}


@pytest.mark.parametrize("dtype", ["f32", "f32a"])
@pytest.mark.parametrize("n,bs", [(7, 128), (20, 192), (100, 256)])
def test_logits_equal_the_two_launch_table(n, bs, dtype):
    """Per-call table (one launch, inside the plan launch) against the two-launch table, both entry points.  The two-launch
    form is taken in-process through ``prepared_tables = True`` (mel_prepare_feature_tables: the encoder launch, then the conv1
    launch) rather than through MEL_NO_FUSED_TABLE in a child process (the switch is read once per process): the in-process
    form needs no second program.  That the per-call forwards really evaluated their table INSIDE the plan launch is read
    off the stage timer: the table was used, and no launch was booked to the encoder or conv1_lin stages - which is where the
    two-launch form books the conv1 projections of the tuples."""
    net = make("l_dgn", n, dtype)
    obs = torch.from_numpy(env_like_obs(n, bs, 5 + n)).cuda()
    mat = torch.from_numpy(env_like_obs(n, bs, 6 + n, index_col=False)).cuda()
    am = torch.from_numpy(agent_sets(n, bs, 7 + n)).cuda()
    cap = bs * n
    with torch.no_grad():
        net.hip_forward(obs, integer_features=True)                     # (workspaces allocated before the timer is attached)
        net.hip_forward_agents(mat, am, cap, integer_features=True)
        got = {}
        stages = launches_by_stage(lambda: got.update(a=net.hip_forward(obs, integer_features=True).clone()))
        assert stages["plan"] >= 1 and stages["encoder"] == 0 and stages["conv1_lin"] == 0, stages
        fused = got["a"]
        assert int(net.hip_tap(3, bs)[0]) == 40 * n
        stages = launches_by_stage(lambda: got.update(b=net.hip_forward_agents(mat, am, cap, integer_features=True)))
        assert stages["plan"] >= 1 and stages["encoder"] == 0 and stages["conv1_lin"] == 0, stages
        fused_set, off = got["b"]
        fused_set, off = fused_set.clone(), off.clone()
        assert int(net.hip_tap(3, bs, cap)[0]) == 40 * n
        net.prepared_tables = True
        two = net.hip_forward(obs, integer_features=True).clone()
        assert net._weights().tables and int(net.hip_tap(3, bs)[0]) == 40 * n
        two_set, off2 = net.hip_forward_agents(mat, am, cap, integer_features=True)
        assert int(net.hip_tap(3, bs, cap)[0]) == 40 * n
    rows = int(off[-1])
    assert rows > 0 and torch.equal(off, off2)
    assert torch.equal(fused, two)
    assert torch.equal(fused_set[:rows], two_set[:rows])


@pytest.mark.parametrize("B", [64, 256])
def test_round_loop_graph_replay_equals_eager(B):
    """The plan launch with the table in it, captured four rounds to a graph and replayed, against eager launches.  (64 envs of
    20 nodes are below the row count from which a forward takes the table - 2 x 800 rows expected in its lists - so that case
    holds the loop itself; 256 envs take the table.)"""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    n = 20
    graphs = synthetic_graph_pool(n, 8, first_seed=5)
    net = make("l_dgn", n, "f32a")
    finals = []
    for use_graph in (True, False):
        venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=48,
                                 construct_like_reference=False)
        loop = RoundLoop(venv, DQNPolicy(net), seed=3, eps=0.05, use_graph=use_graph, graph_rounds=4)
        loop.run(12)
        torch.cuda.synchronize()
        ft = loop.feature_table()
        assert ft["bad_envs"] == 0 and ft["table_rows"] == (n * 40 if B == 256 else 0)
        finals.append((loop.logits.cpu().numpy().copy(), venv.scalars().cpu().numpy().copy(), loop.counters()))
    np.testing.assert_array_equal(finals[0][0], finals[1][0])
    np.testing.assert_array_equal(finals[0][1], finals[1][1])
    assert finals[0][2] == finals[1][2] and finals[0][2]["errors"] == 0
