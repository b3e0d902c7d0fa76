"""Host side of update pacing (``--update-per-step``): the arithmetic of :func:`melissa_amd.train.updates_owed`, the collect and
buffer sizes derived from the reference's flags, and the command line."""
import inspect
from math import floor

import numpy as np
import pytest

from melissa_amd.train import (arg_parser, parse_args, replay_rounds_for, rounds_per_collect, train, train_kwargs,
                               updates_owed)


@pytest.mark.parametrize("u", [0.1, 0.05, 1.0, 0.37, 2.5])
def test_updates_owed_is_monotone_and_never_negative(u):
    base = 137
    owed = [updates_owed(step, base, 0, u) for step in range(0, 3000, 7)]
    assert all(k >= 0 for k in owed) and all(b >= a for a, b in zip(owed, owed[1:]))
    assert updates_owed(base, base, 0, u) == 0 and updates_owed(base - 50, base, 0, u) == 0     # (a count behind the base)
    # more updates done than the count asks for (a stale count after an epoch's debt was settled): nothing, not a negative number
    assert updates_owed(base + 100, base, 10 ** 6, u) == 0
    assert isinstance(updates_owed(base + 100, base, 0, u), int)


@pytest.mark.parametrize("u", [0.1, 0.05, 1.0, 0.37, 2.5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_any_split_into_iterations_ends_at_the_cumulative_floor(u, seed):
    rng = np.random.RandomState(seed)
    base = int(rng.randint(0, 500))
    env_step, done, total_iterations = base, 0, 0
    for _ in range(400):
        env_step += int(rng.choice([0, 1, 3, 10, 160, 800]))        # iterations of very different sizes, empty ones too
        k = updates_owed(env_step, base, done, u)
        assert k >= 0
        done += k
        total_iterations += 1
        assert done == floor(u * (env_step - base))                  # ... at every iteration, so at every epoch boundary
    # the same run cut differently (one big step) owes the same total
    assert updates_owed(env_step, base, 0, u) == done


def test_reference_defaults_give_tianshous_count():
    """update_per_step 0.1, collects of exactly 10 env steps: [3P] tianshou takes round(0.1 * 10) = 1 update per collect."""
    base, done = 4321, 0
    for collect in range(1, 2001):
        k = updates_owed(base + 10 * collect, base, done, 0.1)
        assert k == round(0.1 * 10) == 1, collect
        done += k
    assert done == 2000


def test_collect_and_buffer_sizes_at_the_reference_defaults():
    assert rounds_per_collect(10, 40) == 1 and replay_rounds_for(100000, 40, 20) == 125
    assert rounds_per_collect(100, 8) == 13 and rounds_per_collect(100, 8, world=2) == 7 and rounds_per_collect(16, 8, 2) == 1
    assert rounds_per_collect(1, 256) == 1                            # never less than a round
    assert replay_rounds_for(3200, 8, 20) == 20 and replay_rounds_for(3201, 8, 20) == 21
    assert replay_rounds_for(10, 8, 20) == 8                          # never below the pre-fill


def test_cli_maps_the_pacing_flags():
    a = parse_args("--epoch 10 --update-per-step 0.1 --step-per-collect 20 --buffer-size 100000 --training-num 40".split())
    kw = train_kwargs(a)
    assert kw["update_per_step"] == 0.1 and kw["step_per_collect"] == 20 and kw["buffer_size"] == 100000 and kw["envs"] == 40
    assert kw["epoch"] == 10
    assert type(kw["update_per_step"]) is float and type(kw["step_per_collect"]) is int and type(kw["buffer_size"]) is int
    assert train_kwargs(parse_args(["--envs", "12"]))["envs"] == 12   # the project's own name still works
    # absent: pacing is off, the buffer is today's, and train() defaults to the same
    kw = train_kwargs(parse_args([]))
    assert kw["update_per_step"] is None and kw["step_per_collect"] == 10 and kw["buffer_size"] is None and kw["envs"] == 256
    params = inspect.signature(train).parameters
    assert set(kw) <= set(params)
    for k in ("update_per_step", "step_per_collect", "buffer_size"):
        assert params[k].default == kw[k], k
    assert arg_parser().parse_args([]).update_per_step is None


def test_update_per_step_without_epoch_is_rejected(capsys):
    with pytest.raises(SystemExit) as err:
        parse_args(["--update-per-step", "0.1"])
    assert err.value.code == 2 and "--epoch" in capsys.readouterr().err
    # train() says the same before it touches a device
    with pytest.raises(ValueError, match="epoch"):
        train(update_per_step=0.1)
    with pytest.raises(ValueError, match="update_per_step"):
        train(epoch=1, update_per_step=0.0)
