"""Host side of training in epochs: the exploration schedule's formula against the reference's own statement of it, and the
command line of ``python -m melissa_amd.train`` (the reference's names and defaults, common.py:20-39,46,54)."""
import re
from math import e, log

import pytest

from melissa_amd.collect import EpsSchedule, exploration_eps
from melissa_amd.train import arg_parser, train_kwargs

CASES = [(1.0, 0.05, 0.6, 10, 100000), (0.5, 0.01, 0.3, 2, 500)]


def reference_eps(env_step, eps_train, eps_train_final, exploration_fraction, epoch, step_per_epoch):
    """l_dgn.py:229-233, literally."""
    decay_factor = 1.0 - pow(
        e,
        (log(eps_train_final) / (exploration_fraction * epoch * step_per_epoch))
    )
    eps = max(eps_train * (1.0 - decay_factor) ** env_step, eps_train_final)
    return eps


@pytest.mark.parametrize("case", CASES, ids=["reference_defaults", "short_run"])
def test_exploration_eps_is_the_reference_expression(case):
    eps_train, eps_final, fraction, epoch, step_per_epoch = case
    horizon = fraction * epoch * step_per_epoch
    assert horizon == int(horizon)
    for env_step in (0, 1, int(horizon) // 2, int(horizon), 10 * int(horizon)):
        got = exploration_eps(env_step, *case)
        assert abs(got - reference_eps(env_step, *case)) <= 1e-12, env_step
        # the closed form the device evaluates (mel_exploration_schedule): far inside a float ulp of the reference's pow()
        closed = max(eps_train * e ** (env_step * log(eps_final) / horizon), eps_final)
        assert abs(got - closed) <= 1e-9, env_step
    assert exploration_eps(0, *case) == eps_train
    assert exploration_eps(10 * int(horizon), *case) == eps_final              # exactly, past the clamp
    assert exploration_eps(2 * int(horizon), *case) == eps_final
    # the decaying factor is eps_final at the horizon (so the floor is met there when eps_train = 1, earlier below that)
    assert exploration_eps(int(horizon * 0.8), *case) > eps_final
    assert exploration_eps(int(horizon), *case) == pytest.approx(max(eps_train * eps_final, eps_final), rel=1e-9)
    sch = EpsSchedule(eps_train, eps_final, fraction, epoch, step_per_epoch)
    assert sch.eps(int(horizon) // 2) == exploration_eps(int(horizon) // 2, *case) and sch.total_steps == epoch * step_per_epoch
    assert (sch.scale, sch.trace) == (1, 0)


def test_cli_carries_the_reference_flags_and_defaults():
    a = arg_parser().parse_args([])
    want = dict(step_per_epoch=100000, eps_train=1.0, eps_train_final=0.05, exploration_fraction=0.6, eps_test=0.001,
                test_num=100, logdir="log", resume_path=None, seed=9, lr=0.001, gamma=0.99, n_step=4, target_update_freq=500)
    for k, v in want.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    assert re.fullmatch(r"\d{6}-\d{6}", a.model_name)                            # common.py:54: the time the run starts
    b = arg_parser().parse_args(
        "--epoch 10 --step-per-epoch 500 --eps-train 0.9 --eps-train-final 0.02 --exploration-fraction 0.5 --eps-test 0.0 "
        "--test-num 7 --logdir out --model-name run1 --resume-path p.pth --seed 3 --lr 0.01 --gamma 0.9 --n-step 2 "
        "--target-update-freq 50".split())
    kw = train_kwargs(b)
    assert kw["epoch"] == 10 and kw["step_per_epoch"] == 500 and kw["eps_train"] == 0.9 and kw["eps_train_final"] == 0.02
    assert kw["exploration_fraction"] == 0.5 and kw["eps_test"] == 0.0 and kw["test_num"] == 7 and kw["logdir"] == "out"
    assert kw["model_name"] == "run1" and kw["resume_path"] == "p.pth" and kw["seed"] == 3 and kw["lr"] == 0.01
    assert kw["gamma"] == 0.9 and kw["n_step"] == 2 and kw["target_update_freq"] == 50


def test_without_epoch_the_fixed_updates_mode_is_selected():
    import inspect
    from melissa_amd.train import train
    a = arg_parser().parse_args(["--updates", "5"])
    assert a.epoch is None
    kw = train_kwargs(a)
    assert kw["epoch"] is None and kw["updates"] == 5
    params = inspect.signature(train).parameters
    assert set(kw) <= set(params) and params["epoch"].default is None          # train() itself defaults to that mode
    # the knobs train() already took keep its defaults when the flags are absent
    for k in ("seed", "lr", "gamma", "n_step", "target_update_freq"):
        assert kw[k] == params[k].default, k


def test_watch_accepts_every_model_train_saves(monkeypatch):
    import argparse
    from melissa_amd import watch
    from melissa_amd.train import MODELS
    seen = {}

    def parse_args(self, argv=None):
        seen["choices"] = next(x.choices for x in self._actions if x.dest == "model")
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse_args)
    with pytest.raises(SystemExit):
        watch.main([])
    assert set(seen["choices"]) == set(MODELS)
