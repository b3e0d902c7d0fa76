"""``train(save_state=..., stop_after_epoch=..., resume_state=...)``: a run cut at an epoch boundary and continued by a second call
computes, bit for bit, what the uninterrupted run computes - the epoch records, the result and every entry of the final state file.

Every case is three calls: S, the straight run of two epochs into a logdir of its own; A, the same run stopped after epoch 1; B,
the run resumed from A's state.  The conditions that keep a case from passing trivially (the cut inside the eps decay, updates in
both epochs, a wrapped ring where the case paces) are asserted on S; ``STEPS`` holds the smallest ``step_per_epoch``, in steps of
100 from 200, at which S meets them (NOTES.md "Resuming a run" has the observed counts).

A run with any of the three arguments sums its bias gradients in the replay-safe form
(``autograd_ops.set_replay_safe_column_sums``): with torch's ``dy.sum(dim=0)`` inside the captured update, S and B ended on other
weights (param_checksum -359.4310959012896 against -362.47350602702 for ``l_dgn``) although every other entry of the state
files was equal, and S itself moved with whatever ran on the device between two replays (NOTES.md "Resuming a run")."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = dict(n_nodes=20, envs=8, test_num=2, exploration_fraction=1.0, model_name="run", log=lambda line: None)
CASES = {
    "l_dgn": dict(model="l_dgn"),
    "l_dgn_paced": dict(model="l_dgn", update_per_step=0.1, step_per_collect=10, buffer_size=8 * 20 * 8, prio_buffer=True,
                        collect_stats="steps", target_update_freq=7),
    "hl_n_dgn_r": dict(model="hl_n_dgn_r", heuristic="mpr", scripted_agents_ratio=0.5, capture_updates=False),
    "dgn_r": dict(model="dgn_r", test_envs=2),
}
STEPS = {"l_dgn": 500, "l_dgn_paced": 400, "hl_n_dgn_r": 300, "dgn_r": 500, "three_way": 300, "two_ranks": 1000}
EPS_FINAL = float(np.float32(0.05))                # eps_train_final as the device holds it: the floor the records show
SAME = ("param_checksum", "decisions", "episodes", "updates", "best_epoch", "best_rew", "loss_last")


def without_seconds(epochs):
    return [{k: v for k, v in e.items() if k != "seconds"} for e in epochs]


def differences(a, b, at="state"):
    """Where two loaded state files differ (tensors by ``torch.equal``, generator states as the byte tensors they are, scalars by
    ``==``); wall-clock seconds are not state."""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [f"{at}: keys {sorted(set(a) ^ set(b))}"] if set(a) != set(b) else []
        for k in a:
            if k in b and k != "seconds":
                out += differences(a[k], b[k], f"{at}.{k}")
        return out
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        out = [f"{at}: lengths {len(a)} and {len(b)}"] if len(a) != len(b) else []
        for i, (x, y) in enumerate(zip(a, b)):
            out += differences(x, y, f"{at}[{i}]")
        return out
    if torch.is_tensor(a) and torch.is_tensor(b):
        same = a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        return [] if same else [f"{at}: tensors differ ({tuple(a.shape)} {a.dtype} / {tuple(b.shape)} {b.dtype})"]
    return [] if type(a) is type(b) and a == b else [f"{at}: {a!r} != {b!r}"]


def load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def cut_in_two(args, root, epoch=2):
    """S, A and B of ``args`` under the directory ``root`` -> dict(S, A, B: results; a_state: A's file as loaded before B replaced
    it; a_copy: a copy of that file; s_state / b_state: the final files)."""
    from melissa_amd.train import train
    kw = dict(BASE, **args)
    S = train(epoch=epoch, save_state=True, logdir=os.path.join(root, "straight"), **kw)
    A = train(epoch=epoch, stop_after_epoch=1, save_state=True, logdir=os.path.join(root, "cut"), **kw)
    a_state = load(A["state_path"])
    a_copy = shutil.copy(A["state_path"], os.path.join(root, "after_epoch_1." + os.path.basename(A["state_path"])))
    B = train(epoch=epoch, resume_state=A["state_path"], save_state=True, logdir=os.path.join(root, "cut"), **kw)
    return dict(S=S, A=A, B=B, a_state=a_state, a_copy=a_copy, s_state=load(S["state_path"]), b_state=load(B["state_path"]))


def check_inputs(S, a_state, paced):
    """The conditions on a case's inputs, on the straight run alone (and, for the ring, on the state at the cut)."""
    ep = S["epochs"]
    print("inputs:", [(e["epoch"], e["env_step"], e["eps"], e["updates"]) for e in ep])
    assert ep[1]["eps"] > EPS_FINAL, "the cut must land inside the eps decay: raise step_per_epoch"
    assert all(e["updates"] >= 2 for e in ep[1:])
    if paced:
        cursor, K = a_state["replay"]["cursor"], a_state["config"]["replay_rounds"]
        print("ring:", int(cursor.max()), "records into", K, "slots")
        assert int(cursor.max()) > K, "the ring must have wrapped by the cut"


def check_resumed(S, B, s_state, b_state, epochs=2):
    assert [e["epoch"] for e in B["epochs"]] == list(range(epochs + 1))
    assert without_seconds(B["epochs"]) == without_seconds(S["epochs"])
    for key in SAME:
        assert B[key] == S[key], key
    assert B["errors"] == 0 and S["errors"] == 0 and B["replicas_identical"]
    assert B["param_checksum_start"] == S["param_checksum_start"] and B["param_checksum"] != B["param_checksum_start"]
    assert b_state["config"] == s_state["config"] and b_state["config"]["state_epoch"] == epochs
    assert differences(s_state, b_state) == []


def run_case(name, tmp_path_factory):
    args = dict(CASES[name], step_per_epoch=STEPS[name])
    return name, args, cut_in_two(args, str(tmp_path_factory.mktemp(name)))


@pytest.fixture(scope="module")
def first_case(tmp_path_factory):
    return run_case("l_dgn", tmp_path_factory)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, tmp_path_factory):
    return request.getfixturevalue("first_case") if request.param == "l_dgn" else run_case(request.param, tmp_path_factory)


def test_the_straight_run_meets_the_conditions_on_the_inputs(case):
    name, args, r = case
    check_inputs(r["S"], r["a_state"], paced="update_per_step" in args)


def test_resumed_run_equals_the_straight_run(case):
    name, args, r = case
    check_resumed(r["S"], r["B"], r["s_state"], r["b_state"])
    if "update_per_step" in args:
        assert all(e["update_debt"] == 0 for e in r["B"]["epochs"])
        assert r["b_state"]["replay"]["prio"].count_nonzero() > 0 and "step_stats" in r["b_state"]["venv"]
    if name == "hl_n_dgn_r":
        assert "active_nb" in r["b_state"]["replay"] and "draw_scripted" in r["b_state"]["stream"]
        assert r["B"]["updates_from_hip_graphs"] is False


def test_the_state_at_the_cut_holds_header_and_records(case):
    name, args, r = case
    A, st = r["A"], r["a_state"]
    assert os.path.basename(A["state_path"]) == "run_state.pth" and A["state_path"].startswith(os.path.dirname(A["last_path"]))
    assert [e["epoch"] for e in A["epochs"]] == [0, 1] and os.path.exists(A["last_path"])
    cfg = st["config"]
    assert (cfg["model"], cfg["envs"], cfg["n_nodes"], cfg["epoch"], cfg["state_epoch"]) == (args["model"], 8, 20, 2, 1)
    assert cfg["step_per_epoch"] == args["step_per_epoch"] and cfg["world"] == 1 and cfg["pool_graphs"] == 16
    assert cfg["captured"] is args.get("capture_updates", True)
    assert st["run"]["epochs"] == A["epochs"] and st["run"]["epochs"][1]["epoch"] == 1
    assert st["run"]["updates"] == A["updates"] == A["epochs"][1]["updates"]
    # what the straight run held at the same boundary: its own epoch-1 record
    assert without_seconds(A["epochs"]) == without_seconds(r["S"]["epochs"][:2])


def test_a_state_of_another_run_is_refused_by_name(first_case):
    from melissa_amd.train import train
    name, args, r = first_case
    with pytest.raises(ValueError, match=r"with envs=8; this call has envs=16"):
        train(epoch=2, resume_state=r["a_copy"], logdir=os.path.dirname(r["a_copy"]), **dict(BASE, **args, envs=16))
    with pytest.raises(ValueError, match=r"holds the state after epoch 2"):
        train(epoch=2, resume_state=r["B"]["state_path"], logdir=os.path.dirname(r["a_copy"]), **dict(BASE, **args))


def test_a_run_cut_twice_equals_the_straight_run(tmp_path):
    """epoch=3, stopped after 1, resumed and stopped after 2, resumed to 3: what a restore takes from the file must also be
    written back into the next file."""
    from melissa_amd.train import train
    kw = dict(BASE, **CASES["l_dgn"], step_per_epoch=STEPS["three_way"], epoch=3, save_state=True)
    S = train(logdir=str(tmp_path / "straight"), **kw)
    cut = str(tmp_path / "cut")
    A = train(stop_after_epoch=1, logdir=cut, **kw)
    check_inputs(S, load(A["state_path"]), paced=False)
    B = train(stop_after_epoch=2, resume_state=A["state_path"], logdir=cut, **kw)
    assert [e["epoch"] for e in B["epochs"]] == [0, 1, 2] and load(B["state_path"])["config"]["state_epoch"] == 2
    C = train(resume_state=B["state_path"], logdir=cut, **kw)
    check_resumed(S, C, load(S["state_path"]), load(C["state_path"]), epochs=3)


def _two_rank_worker(rank, world, port, out_dir):
    import json
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    # (one process per rank makes the three calls: the process group is initialised once)
    r = cut_in_two(dict(CASES["l_dgn"], step_per_epoch=STEPS["two_ranks"], backend="gloo"), out_dir)
    ok = differences(r["s_state"], r["b_state"])
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(S=r["S"], A=r["A"], B=r["B"], differences=ok, state_rank=r["b_state"]["config"]["rank"]), f)
    torch.distributed.destroy_process_group()


def test_two_ranks_resume_each_from_its_own_file(tmp_path):
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
    assert not hung, "a rank is stuck"
    assert [p.exitcode for p in procs] == [0, 0]
    r0, r1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in range(2))
    weights = tmp_path / "cut" / "l_dgn" / "weights"
    assert sorted(f for f in os.listdir(weights) if "state" in f) == ["run_state.rank0.pth", "run_state.rank1.pth"]
    assert r0["B"]["state_path"] == str(weights / "run_state.rank0.pth") and r1["B"]["state_path"] == str(weights / "run_state.rank1.pth")
    assert (r0["state_rank"], r1["state_rank"]) == (0, 1)
    S, B = r0["S"], r0["B"]
    print("inputs:", [(e["epoch"], e["env_step"], e["eps"], e["updates"]) for e in S["epochs"]])
    assert S["epochs"][1]["eps"] > EPS_FINAL and all(e["updates"] >= 2 for e in S["epochs"][1:])
    assert without_seconds(B["epochs"]) == without_seconds(S["epochs"]) and [e["epoch"] for e in B["epochs"]] == [0, 1, 2]
    for key in SAME:
        assert B[key] == S[key], key
    assert "test_rew" in B["epochs"][0] and "test_rew" not in r1["B"]["epochs"][0]          # rank 0's records are the run's
    for r in (r0, r1):
        assert r["differences"] == [] and r["B"]["errors"] == 0 and r["B"]["replicas_identical"] and r["B"]["world"] == 2
        assert r["B"]["param_checksum"] == r["S"]["param_checksum"] == S["param_checksum"]
    assert r1["B"]["decisions"] == r1["S"]["decisions"] != S["decisions"]                   # each rank continued its OWN envs


@pytest.mark.parametrize("rows,cols", [(640, 512), (33, 2), (1, 1), (2049, 130)])
def test_replay_safe_column_sum_is_the_column_sum(rows, cols):
    """Against float64: a float32 sum of ``rows`` terms, in any order, is within ``rows * 2^-24 * sum |x|`` of it."""
    from melissa_amd.networks import autograd_ops as ops
    dy = torch.randn(rows, cols, device="cuda", generator=torch.Generator(device="cuda").manual_seed(rows))
    want, bound = dy.double().sum(0), rows * 2.0 ** -24 * dy.double().abs().sum(0)
    try:
        ops.set_replay_safe_column_sums(True)
        got = ops.column_sum(dy)
        y, b = torch.zeros_like(dy, requires_grad=True), torch.zeros(cols, device="cuda", requires_grad=True)
        ops.add_bias(y, b).backward(dy)
    finally:
        ops.set_replay_safe_column_sums(False)
    assert got.shape == (cols,) and got.dtype == torch.float32
    assert bool(((got.double() - want).abs() <= bound).all()) and torch.equal(b.grad, got) and torch.equal(y.grad, dy)
    assert torch.equal(ops.column_sum(dy), dy.sum(dim=0))                   # off: the form every other run has always had
