"""CPU tests of the --hidden-emb / --num-heads shapes: the command-line flags of train / watch, the Python statement of the
HIP path's shape rule (melissa_amd.shapes) and the torch backend of a 6-head network against the network oracle."""
import numpy as np
import pytest
import torch

from melissa_amd.shapes import head_lanes, hip_shape_supported

# (hidden, heads) -> does the HIP path run it.  Written out here, not derived from the rule under test.
SHAPE_TABLE = {(64, 2): True, (64, 4): True, (128, 2): True, (128, 4): True, (256, 2): True, (256, 4): True, (512, 2): True,
               (64, 6): True, (128, 6): True,
               (64, 8): True, (64, 16): True, (128, 1): True, (128, 8): True, (256, 1): True, (512, 1): True,
               (16, 2): False, (16, 4): False, (16, 6): False, (32, 2): False, (32, 4): False, (32, 6): False,
               (512, 4): False, (256, 6): False}


def test_parsers_take_the_reference_flags_with_its_defaults():
    from melissa_amd import train, watch
    for parser in (train.arg_parser(), watch.arg_parser()):
        a = parser.parse_args([])
        assert (a.hidden_emb, a.num_heads, a.aggregator_function) == (128, 4, "max")          # common.py:29-30,43
        assert a.dueling_q_hidden_sizes == [128, 128] and a.dueling_v_hidden_sizes == [128, 128]    # common.py:41-42
        a = parser.parse_args(["--hidden-emb", "64", "--num-heads", "6", "--dueling-q-hidden-sizes", "64", "--dueling-v-hidden-sizes",
                               "128", "--model", "hl_dgn", "--aggregator-function", "mean"])
        assert (a.hidden_emb, a.num_heads, a.aggregator_function) == (64, 6, "mean")
        assert a.dueling_q_hidden_sizes == [64] and a.dueling_v_hidden_sizes == [128]
        assert parser.parse_args(["--dueling-q-hidden-sizes"]).dueling_q_hidden_sizes == []       # nargs='*'
    kw = train.train_kwargs(train.parse_args(["--hidden-emb", "64", "--num-heads", "6"]))
    assert (kw["hidden_emb"], kw["num_heads"], kw["aggregator_function"]) == (64, 6, "max")
    assert kw["dueling_q_hidden_sizes"] == [128, 128] and kw["dueling_v_hidden_sizes"] == [128, 128]


@pytest.mark.parametrize("argv,reason", [
    (["--num-heads", "6", "--hidden-emb", "256"], "32 channels per lane"),
    (["--hidden-emb", "32"], "multiple of 64"),
    (["--hidden-emb", "16"], "multiple of 64"),
    (["--hidden-emb", "512", "--num-heads", "4"], "32 channels per lane"),
    (["--hidden-emb", "1024", "--num-heads", "2"], "hidden width 1024"),
    (["--num-heads", "3"], "3 heads fill 48 of 64 lanes"),
    (["--model", "l_dgn", "--aggregator-function", "mean"], "HL-DGN"),
    (["--dueling-q-hidden-sizes", "100", "100"], "multiple of 64"),
    (["--dueling-q-hidden-sizes", "128"], "same depth"),
])
def test_unsupported_shapes_fail_at_argument_time_with_the_reason(argv, reason, capsys):
    from melissa_amd import train, watch
    for parse in (train.parse_args, watch.parse_args):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert e.value.code == 2
        assert reason in capsys.readouterr().err
    # the keyword form: before anything is built (no device is touched: this test runs without one)
    a = train.arg_parser().parse_args(argv)
    kw = dict(hidden_emb=a.hidden_emb, num_heads=a.num_heads, dueling_q_hidden_sizes=a.dueling_q_hidden_sizes,
              dueling_v_hidden_sizes=a.dueling_v_hidden_sizes, aggregator_function=a.aggregator_function)
    with pytest.raises(ValueError, match=reason):
        train.train(model=a.model, **kw)
    with pytest.raises(ValueError, match=reason):
        watch.watch(model=a.model, **kw)


def test_dueling_depth_rule_is_the_librarys_and_bf16_needs_a_hidden_layer(capsys):
    from melissa_amd import _lib, shapes, train, watch
    assert shapes.MAX_HEAD_LAYERS == _lib.MAX_HEAD_LAYERS
    deepest = [64] * (_lib.MAX_HEAD_LAYERS - 1)
    train.check_network_args("l_dgn", dueling_q_hidden_sizes=deepest, dueling_v_hidden_sizes=deepest)
    with pytest.raises(ValueError, match="same depth"):
        train.check_network_args("l_dgn", dueling_q_hidden_sizes=deepest + [64], dueling_v_hidden_sizes=deepest + [64])
    # no hidden layer: fine for the fp32 precisions, refused for bf16 rows where the dtype is known (watch)
    empty = ["--dueling-q-hidden-sizes", "--dueling-v-hidden-sizes"]
    assert watch.parse_args(empty + ["--dtype", "f32a"]).dueling_q_hidden_sizes == []
    with pytest.raises(SystemExit):
        watch.parse_args(empty + ["--dtype", "bf16"])
    assert "at least one hidden layer" in capsys.readouterr().err
    with pytest.raises(ValueError, match="at least one hidden layer"):
        watch.watch(dueling_q_hidden_sizes=[], dueling_v_hidden_sizes=[], feature_dtype="bf16")


@pytest.mark.parametrize("hidden,heads", sorted(SHAPE_TABLE))
def test_hip_shape_supported_against_the_table(hidden, heads):
    """tests/test_gpu_head_shapes.py::test_shape_rule_and_library_agree holds the library to the same table."""
    from melissa_amd.networks import hip_shape_supported as exported
    ok, reason = hip_shape_supported(hidden, heads)
    assert exported is hip_shape_supported
    assert isinstance(ok, bool) and (reason == "") == ok
    assert ok == SHAPE_TABLE[(hidden, heads)], reason


def test_lane_rule_of_every_supported_pair():
    seen = 0
    for hidden in (16, 32, 64, 128, 256, 512):
        for heads in range(1, 17):
            if not hip_shape_supported(hidden, heads)[0]:
                continue
            lanes, live, vpl, reason = head_lanes(heads, hidden)
            assert reason is None
            assert heads * lanes <= 64 and heads * lanes * 2 > 64 and lanes & (lanes - 1) == 0
            assert live == heads * lanes and vpl in (2, 4, 8, 16) and vpl * lanes == hidden
            assert live == 64 or (heads, live, lanes) == (6, 48, 8)        # nothing but 6 heads leaves lanes idle
            seen += 1
    assert seen >= 10
    assert head_lanes(6, 64)[:3] == (8, 48, 8) and head_lanes(6, 128)[:3] == (8, 48, 16)


def random_obs(n, bs, seed):
    rng = np.random.RandomState(seed)
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, 9, size=(bs, n))
    m[:, :, 3] = rng.randint(0, 4, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.2)
    obs[:, -1] = rng.randint(0, n, size=bs)
    return obs


@pytest.mark.parametrize("model,agg", [("l_dgn", "max"), ("dgn_r", "max"), ("hl_dgn", "max"), ("hl_dgn", "mean"), ("hl_dgn", "add")])
def test_torch_backend_of_a_six_head_network_matches_the_oracle(model, agg):
    """build_network(hidden=64, heads=6) on the torch backend (CPU) against oracle.net_oracle, edges and dense formulations
    against each other: the comparison target of the GPU tests."""
    from melissa_amd.train import build_network
    from oracle import net_oracle as no
    torch.set_num_threads(4)
    n, bs = 20, 6
    obs = random_obs(n, bs, 23)
    sd = no.init_weights(model, hidden=64, heads=6, seed=17, random_conv_bias=True)
    assert sd["conv1." + ("lin_key" if model == "dgn_r" else "lin_l") + ".weight"].shape == (384, 64)
    net = build_network(model, n, "cpu", hidden=64, heads=6, aggregator=agg)
    net.backend = "torch"
    net.load_state_dict(sd)
    fwd = {"l_dgn": no.ldgn_forward, "dgn_r": no.dgnr_forward, "hl_dgn": no.hldgn_forward}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    with torch.no_grad():
        got = net(obs)[0].numpy()
        edges = fwd(sd, obs, n, heads=6, formulation="edges", **kw).numpy()
        dense = fwd(sd, obs, n, heads=6, formulation="dense", **kw).numpy()
    np.testing.assert_allclose(edges, dense, atol=1e-5, rtol=0)
    np.testing.assert_allclose(got, edges, atol=1e-5, rtol=0)


def test_loading_a_checkpoint_of_another_shape_names_key_and_shapes(tmp_path):
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network, load_policy_weights
    path = str(tmp_path / "four_heads.pth")
    torch.save(DQNPolicy(build_network("hl_dgn", 12, "cpu", hidden=64, heads=4), target_update_freq=1).state_dict(), path)
    six = DQNPolicy(build_network("hl_dgn", 12, "cpu", hidden=64, heads=6), target_update_freq=1)
    with pytest.raises(ValueError, match=r"model\.conv1\.att is \(1, 4, 64\) in the checkpoint and \(1, 6, 64\) in the network"):
        load_policy_weights(six, path, "cpu")
    same = DQNPolicy(build_network("hl_dgn", 12, "cpu", hidden=64, heads=4), target_update_freq=1)
    load_policy_weights(same, path, "cpu")
