"""GPU check of the two recorders on ONE round loop (csrc/record_common.hpp serves both): neither disturbs the other or the
trajectory, and their trace rings join on (env, episode ordinal, num_moves) as melissa_hip.h promises - the node trace sampled
after round r - 1 is the state round r's decisions were taken in."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from melissa_amd import _lib as L
from tests import test_gpu_decision_record as DR
from tests import test_gpu_round_record as RR

ROUNDS = 24


def play(n, B, scripted, recorder, decisions):
    """``ROUNDS`` eager rounds of the L-DGN loop from one seed, every env traced by the recorders asked for."""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.decision_record import DecisionRecorder
    from melissa_amd.round_record import RoundRecorder
    kw = dict(scripted_agents_ratio=scripted, heuristic="simple_broadcast") if scripted else {}
    venv = DR._venv(n, B, **kw)
    rec = RoundRecorder(venv, trace_envs=range(B), trace_capacity=64) if recorder else None
    dec = DecisionRecorder(venv, trace_envs=range(B), trace_capacity=64) if decisions else None
    loop = RoundLoop(venv, DR._policy("l_dgn", n), seed=3, eps=0.1, use_graph=False, recorder=rec, decisions=dec)
    loop.run(ROUNDS)
    torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0 and loop.iterations == ROUNDS
    return rec, dec


@pytest.mark.parametrize("n,B,scripted", [(12, 4, 0.0), (70, 2, 0.0), (12, 4, 0.5)])
def test_both_recorders_on_one_loop_agree_with_each_alone_and_join(n, B, scripted):
    """12 nodes x 4 envs, 70 nodes x 2 envs (two-word sets), and once with scripted nodes (outside the evaluation schedule the
    env keeps them out of the active set itself, so the deciding set must still equal it)."""
    rec, dec = play(n, B, scripted, True, True)
    # (a) bit for bit what each recorder holds when it rides alone
    RR.assert_same(RR.device_state(rec), RR.device_state(play(n, B, scripted, True, False)[0]))
    DR.assert_same(DR.device_state(dec), DR.device_state(play(n, B, scripted, False, True)[1]))
    assert rec.curves()[2] == dict(overflow=0, skipped=0, unlogged=0) and dec.tables()[2] == dict(overflow=0, skipped=0)
    nodes, lost_nodes = rec.drain_traces()
    decided, lost_decisions = dec.drain_traces()
    assert lost_nodes == 0 and lost_decisions == 0 and sorted(nodes) == sorted(decided) == list(range(B))
    joined = with_scripted = 0
    for env in range(B):
        keys = [(ep["ordinal"], int(r)) for ep in nodes[env] for r in ep["rounds"]]
        state = {(ep["ordinal"], int(r)): ep["sets"][k] for ep in nodes[env] for k, r in enumerate(ep["rounds"])}
        for ep in decided[env]:
            assert ep["env"] == env
            for k, r in enumerate(ep["rounds"]):
                # (b) exactly one node trace record of the state the decisions were taken in
                assert keys.count((ep["ordinal"], int(r))) == 1, (env, ep["ordinal"], int(r))
                sets = state[(ep["ordinal"], int(r))]
                active, is_scripted = sets[L.RR_TRACE_SETS.index("active")], sets[L.RR_TRACE_SETS.index("scripted")]
                deciding, relaying = ep["sets"][k]
                # (c) the policy decided for the active nodes that are not scripted, and relayed through some of them
                np.testing.assert_array_equal(deciding, active & ~is_scripted, err_msg=f"env {env} {ep['ordinal']} round {r}")
                assert not (relaying & ~deciding).any()
                joined, with_scripted = joined + 1, with_scripted + bool(is_scripted.any())
    assert joined > ROUNDS                               # more than one env's worth of rounds joined
    assert with_scripted == (joined if scripted else 0)  # the scripted case does have scripted nodes, in every joined state
