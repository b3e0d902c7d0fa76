"""``train(update_per_step=...)``: updates paced by the env steps collected - the cumulative-floor rule at every epoch boundary,
eagerly, from HIP graphs, for the sibling loss and on two ranks - and the collect / buffer sizes of the reference's flags."""
import os
from math import ceil, floor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 0.05
BASE = dict(model="l_dgn", n_nodes=20, envs=8, epoch=2, step_per_epoch=400, test_num=2, update_per_step=U, model_name="run",
            log=lambda line: None)
TODAY = {"rank", "world", "model", "updates", "seconds", "loss_first", "loss_last", "decisions", "episodes", "errors",
         "param_checksum", "updates_from_hip_graphs", "prio_buffer", "warmup_updates", "heuristic", "scripted_agents_ratio",
         "episode_supply", "replicas_identical", "epochs", "best_epoch", "best_rew", "best_path", "last_path", "param_checksum_start"}
PACED = {"update_per_step", "rounds_per_collect", "replay_rounds", "env_steps_per_iteration", "fused_td"}


def check_paced(out, epochs, u=U):
    ep = out["epochs"]
    assert [e["epoch"] for e in ep] == list(range(epochs + 1))
    base, done = ep[0]["env_step"], 0
    assert ep[0]["updates"] == 0 and ep[0]["update_debt"] == 0
    for e in ep[1:]:
        done += e["updates"]
        assert done == floor(u * (e["env_step"] - base)), (e["epoch"], done, e["env_step"], base)
        assert e["update_debt"] == 0 and e["overshoot"] >= 0
    assert out["updates"] == done > 0
    assert out["fused_td"] is True and out["update_per_step"] == u
    assert out["errors"] == 0 and out["replicas_identical"] and np.isfinite(out["loss_first"]) and np.isfinite(out["loss_last"])
    assert set(out) == TODAY | PACED


@pytest.fixture(scope="module")
def base_run(tmp_path_factory):
    from melissa_amd.train import train
    return train(logdir=str(tmp_path_factory.mktemp("log")), **BASE)


def test_updates_follow_the_env_steps(base_run):
    check_paced(base_run, 2)
    # the defaults: collects of 10 env steps are ceil(10 / 8 envs) = 2 rounds, the buffer is the 64 rounds it was
    assert base_run["rounds_per_collect"] == 2 and base_run["replay_rounds"] == 64
    assert base_run["updates_from_hip_graphs"] is True and base_run["warmup_updates"] == 2      # (warm-ups: outside `updates`)
    assert 0 < base_run["env_steps_per_iteration"] <= 2 * 8 * 20                                 # a round: <= envs * nodes decisions


def test_paced_updates_without_capture(tmp_path):
    from melissa_amd.train import train
    out = train(logdir=str(tmp_path), capture_updates=False, **BASE)
    check_paced(out, 2)
    assert out["updates_from_hip_graphs"] is False and out["warmup_updates"] == 0


def test_paced_sibling_loss_replays_from_graphs(tmp_path):
    """dgn_r, one epoch, the update captured although a probe watches: the learner it sees replays the fused update."""
    from melissa_amd.train import train
    seen = {}

    def probe(index, net, learner, phase):
        seen["learner"] = learner
        if phase == "before":
            seen.setdefault("indices", []).append(index)

    out = train(logdir=str(tmp_path), capture_updates=True, probe=probe, **{**BASE, "model": "dgn_r", "epoch": 1})
    check_paced(out, 1)
    learner = seen["learner"]
    assert learner.captured is not None and learner.fused_td is True and out["updates_from_hip_graphs"] is True
    assert seen["indices"] == list(range(out["updates"]))                    # every paced update, numbered in order


def test_step_per_collect_and_buffer_size(tmp_path):
    from melissa_amd.train import train
    out = train(logdir=str(tmp_path), step_per_collect=100, buffer_size=3200, **{**BASE, "epoch": 1})
    check_paced(out, 1)
    assert out["rounds_per_collect"] == ceil(100 / 8) == 13 and out["replay_rounds"] == 20
    assert out["env_steps_per_iteration"] > 13                                # (13 rounds of 8 envs: more than a decision a round)
    # many updates per iteration now: 13 rounds collect far more than 1 / U env steps
    assert out["updates"] == floor(U * (out["epochs"][1]["env_step"] - out["epochs"][0]["env_step"]))


def test_update_per_step_needs_epochs():
    from melissa_amd.train import train
    with pytest.raises(ValueError, match="epoch"):
        train(model="l_dgn", n_nodes=20, envs=8, update_per_step=U, log=lambda line: None)


def _two_rank_worker(rank, world, port, out_dir):
    import json
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from melissa_amd.train import train
    out = train(backend="gloo", logdir=os.path.join(out_dir, "log"), **{**BASE, "step_per_epoch": 300, "test_num": 1})
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    torch.distributed.destroy_process_group()


def test_two_ranks_take_the_same_paced_updates(tmp_path):
    """Two ranks on one GPU (gloo): both derive every iteration's updates from the same agreed count, so the gradient all-reduce
    pairs them one to one and the replicas stay identical."""
    import json
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [mp.get_context("spawn").Process(target=_two_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(150)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
    assert not hung, "a rank is stuck: the ranks took different numbers of updates"
    assert [p.exitcode for p in procs] == [0, 0]
    r0, r1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in range(2))
    assert (r0["world"], r1["world"]) == (2, 2)
    for a, b in zip(r0["epochs"], r1["epochs"]):
        assert (a["epoch"], a["env_step"], a["updates"], a["update_debt"]) == (b["epoch"], b["env_step"], b["updates"], 0)
    check_paced(r0, 2)
    check_paced(r1, 2)
    assert r0["updates"] == r1["updates"] and r0["param_checksum"] == r1["param_checksum"]
    assert r0["replicas_identical"] and r1["replicas_identical"]
    assert r0["rounds_per_collect"] == 1                                      # ceil(10 / (8 envs * 2 ranks))
