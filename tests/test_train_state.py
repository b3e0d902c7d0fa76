"""CPU tests of the full-state checkpoints of an epoch-mode run (melissa_amd.train_state): the command-line flags, the argument
rules, the header comparison and the atomic write.  No device is touched; tests/test_gpu_train_state.py resumes real runs."""
import os

import pytest
import torch

from melissa_amd import train, train_state


def test_parsers_take_the_state_flags_with_their_defaults():
    a = train.arg_parser().parse_args([])
    assert (a.save_state, a.stop_after_epoch, a.resume_state) == (False, None, None)
    kw = train.train_kwargs(train.parse_args([]))
    assert (kw["save_state"], kw["stop_after_epoch"], kw["resume_state"]) == (False, None, None)
    kw = train.train_kwargs(train.parse_args(["--epoch", "10", "--save-state", "--stop-after-epoch", "4", "--resume-state",
                                              "log/l_dgn/weights/run_state.pth"]))
    assert (kw["save_state"], kw["stop_after_epoch"], kw["resume_state"]) == (True, 4, "log/l_dgn/weights/run_state.pth")
    assert kw["epoch"] == 10                                   # --epoch stays the run's total
    import inspect
    sig = inspect.signature(train.train).parameters
    assert (sig["save_state"].default, sig["stop_after_epoch"].default, sig["resume_state"].default) == (False, None, None)


@pytest.mark.parametrize("argv,kwargs,reason", [
    (["--resume-state", "x.pth"], dict(resume_state="x.pth"), "needs epoch"),
    (["--resume-state", "x.pth", "--resume-path", "y.pth", "--epoch", "2"],
     dict(resume_state="x.pth", resume_path="y.pth", epoch=2), "mutually exclusive"),
    (["--stop-after-epoch", "0", "--epoch", "3"], dict(stop_after_epoch=0, epoch=3), "between 1 and epoch=3"),
    (["--stop-after-epoch", "5", "--epoch", "3"], dict(stop_after_epoch=5, epoch=3), "between 1 and epoch=3"),
    (["--stop-after-epoch", "1"], dict(stop_after_epoch=1), "needs epoch"),
    (["--save-state"], dict(save_state=True), "needs epoch"),
])
def test_meaningless_combinations_fail_at_argument_time(argv, kwargs, reason, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse_args(argv)
    assert e.value.code == 2
    assert reason in capsys.readouterr().err
    # the keyword form: before anything is built (no device is touched: this test runs without one; the files do not exist)
    with pytest.raises(ValueError, match=reason):
        train.train(model="l_dgn", **kwargs)


def header(**changes):
    h = train_state.state_header(
        model="l_dgn", n_nodes=20, envs=8, world=1, rank=0, hidden_emb=128, num_heads=4, dueling_q_hidden_sizes=(128, 128),
        dueling_v_hidden_sizes=[128, 128], aggregator_function="max", batch_size=32, n_step=4, gamma=0.99, lr=1e-3,
        target_update_freq=500, prio_buffer=False, alpha=0.6, beta=0.4, heuristic=None, scripted_agents_ratio=0.0, epoch=5,
        step_per_epoch=200, eps_train=1.0, eps_train_final=0.05, exploration_fraction=0.6, update_per_step=None,
        step_per_collect=10, replay_rounds=64, rounds_per_update=4, ring=16, seed=9, captured=True, collect_stats="episodes",
        pool_graphs=16, pool_checksum=123456789, mel_version="melissa-hip test")
    h.update(changes)
    return h


def test_header_is_every_key_in_plain_values():
    h = header()
    assert tuple(h) == train_state.HEADER_KEYS
    assert h["dueling_q_hidden_sizes"] == h["dueling_v_hidden_sizes"] == [128, 128]       # tuples and lists compare equal
    assert all(v is None or type(v) in (int, float, str, bool, list) for v in h.values())
    with pytest.raises(KeyError):
        train_state.state_header(learning_rate=1e-3)


def test_equal_headers_pass_and_a_difference_names_its_key():
    saved = dict(header(), state_epoch=3, format=1)
    train_state.check_state_header(saved, header())
    train_state.check_state_header(saved, {k: v for k, v in header().items() if not k.startswith("pool_")})     # the early check
    for key, other in (("envs", 16), ("model", "hl_dgn"), ("update_per_step", 0.1), ("pool_checksum", 987654321), ("epoch", 6)):
        with pytest.raises(ValueError, match=rf"with {key}={saved[key]!r}; this call has {key}={other!r}") as e:
            train_state.check_state_header(saved, header(**{key: other}), "run_state.pth")
        assert isinstance(e.value, train_state.StateMismatch) and "run_state.pth" in str(e.value)
    # the FIRST differing key, in header order
    with pytest.raises(ValueError, match="with model="):
        train_state.check_state_header(saved, header(seed=1, model="dgn_r"))
    with pytest.raises(ValueError, match="no ring in its header"):
        train_state.check_state_header({k: v for k, v in saved.items() if k != "ring"}, header())


def test_a_state_at_or_past_the_last_epoch_is_an_error():
    for taken_after in (3, 4):
        saved = dict(header(epoch=3), state_epoch=taken_after)
        with pytest.raises(ValueError, match=rf"after epoch {taken_after}: nothing is left of a run of epoch=3"):
            train_state.check_state_header(saved, header(epoch=3))
    train_state.check_state_header(dict(header(epoch=3), state_epoch=2), header(epoch=3))
    train_state.check_state_header(dict(header(epoch=3), state_epoch=0), header(epoch=3))


def test_rank_state_path():
    p = os.path.join("log", "l_dgn", "weights", "run_state.pth")
    assert train_state.rank_state_path(p, 0, 1) == p
    assert train_state.rank_state_path(p, 1, 2) == p[:-4] + ".rank1.pth"
    assert train_state.rank_state_path(p[:-4] + ".rank0.pth", 1, 2) == p[:-4] + ".rank1.pth"      # another rank's name was given
    assert train_state.rank_state_path(p[:-4] + ".rank0.pth", 0, 1) == p


def test_pool_identity_follows_count_and_positions():
    import numpy as np

    class G:
        def __init__(self, seed):
            self.pos = np.random.RandomState(seed).uniform(size=(20, 2))

    a = train_state.pool_identity([G(0), G(1), G(2)])
    assert a == train_state.pool_identity([G(0), G(1), G(2)]) and a["pool_graphs"] == 3 and type(a["pool_checksum"]) is int
    assert train_state.pool_identity([G(0), G(2), G(1)])["pool_checksum"] != a["pool_checksum"]
    moved = [G(0), G(1), G(2)]
    moved[1].pos[7, 0] = np.nextafter(moved[1].pos[7, 0], 2.0)                   # one position, one ulp
    assert train_state.pool_identity(moved)["pool_checksum"] != a["pool_checksum"]
    assert train_state.pool_identity([G(0), G(1)]) != a


def test_state_file_round_trip_loads_with_weights_only(tmp_path):
    path = str(tmp_path / "run_state.pth")
    state = dict(format=1, config=dict(header(), state_epoch=1), run=dict(epochs=[dict(epoch=0, eps=1.0, best=True)], best_rew=None),
                 replay=dict(cursor=torch.arange(8, dtype=torch.int32)), learner=dict(gen=torch.zeros(16, dtype=torch.uint8)))
    train_state.write_state_file(state, path)
    assert os.listdir(tmp_path) == ["run_state.pth"]
    for back in (torch.load(path, map_location="cpu", weights_only=True), train_state.load_state_file(path)):
        assert back["config"] == state["config"] and back["run"] == state["run"]
        assert torch.equal(back["replay"]["cursor"], state["replay"]["cursor"])


@pytest.mark.parametrize("failure", ["save", "replace"])
def test_a_failed_write_leaves_the_previous_file_and_no_temporary(tmp_path, monkeypatch, failure):
    path = str(tmp_path / "run_state.pth")
    train_state.write_state_file(dict(config=dict(state_epoch=1), t=torch.arange(1000)), path)
    before = open(path, "rb").read()
    real_save = torch.save

    def half_a_file(obj, f, *args, **kwargs):
        real_save(obj, f, *args, **kwargs)
        size = os.path.getsize(f)
        with open(f, "r+b") as fh:
            fh.truncate(size // 2)
        raise OSError("No space left on device")

    def never_reached(src, dst):
        assert os.path.exists(src) and os.path.dirname(src) == os.path.dirname(dst)       # same directory: the move is atomic
        raise KeyboardInterrupt

    if failure == "save":
        monkeypatch.setattr(torch, "save", half_a_file)
    else:
        monkeypatch.setattr(os, "replace", never_reached)
    with pytest.raises(OSError if failure == "save" else KeyboardInterrupt):
        train_state.write_state_file(dict(config=dict(state_epoch=2), t=torch.arange(2000)), path)
    monkeypatch.undo()
    assert open(path, "rb").read() == before
    assert os.listdir(tmp_path) == ["run_state.pth"]
    assert torch.load(path, weights_only=True)["config"] == dict(state_epoch=1)


def test_replay_safe_column_sums_are_off_by_default_and_the_same_sums():
    from melissa_amd.networks import autograd_ops as ops
    assert ops.replay_safe_column_sums() is False
    torch.manual_seed(3)
    y, b = torch.randn(37, 6, dtype=torch.float64, requires_grad=True), torch.randn(6, dtype=torch.float64, requires_grad=True)
    g = torch.randn(37, 6, dtype=torch.float64)
    try:
        for on in (False, True):
            ops.set_replay_safe_column_sums(on)
            assert ops.replay_safe_column_sums() is on
            y.grad = b.grad = None
            out = ops.add_bias(y, b)
            assert torch.equal(out, y + b)
            out.backward(g)
            assert torch.equal(y.grad, g) and torch.allclose(b.grad, g.sum(0), rtol=0, atol=1e-12)
            assert torch.allclose(ops.column_sum(g), g.sum(0), rtol=0, atol=1e-12)
    finally:
        ops.set_replay_safe_column_sums(False)
    # an argument error leaves the switch where it was
    with pytest.raises(ValueError):
        train.train(model="l_dgn", save_state=True)
    assert ops.replay_safe_column_sums() is False
