"""GPU test of how the attention row kernels (csrc/attention.hpp: gat_attend_rows_kernel) find their rows.  A wave's slot is
fixed by the launch, so it asks for the slot's target descriptor before it knows the device-side row count, drops it when the
slot lies past the count, and takes rows past the grid's slots in further passes.  fwd.hip sizes both attention grids from the
EXPECTED row counts, which depend on the node count and the envs alone: at (n, envs) = (50, 64) both have 1 024 slots.  One
network, one workspace, three agent sets per env:
  {3}        64 agent rows: most slots drop what they fetched;
  {0 .. 15}  1 024 agent rows: exactly the slots of the conv2 attention;
  every node 3 200 agent rows and 3 200 conv1 targets: up to four rows per wave.
The launches, their grids and every GEMM tile are the same in the three calls and a row's arithmetic does not depend on the
other rows, so an agent's logits and head input must be the same BITS in every call that has it.  (The rows' values themselves
are held to recorded bits by tests/test_gpu_attention_walk.py, which shares its network and inputs with this test.)"""
import numpy as np
import pytest
import torch

from tests.test_gpu_attention_walk import build_inputs, make, raw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", ["l_dgn", "dgn_r"])
def test_rows_below_at_and_above_the_grid(model):
    n, bs = 50, 64
    cap = bs * n
    net = make(model, n)
    mat, _ = build_inputs(n, bs, 5)
    obs = torch.from_numpy(mat.reshape(bs, n * 8)).cuda()
    logits, cat = {}, {}
    with torch.no_grad():
        for name, agents in (("one", [3]), ("sixteen", list(range(16))), ("all", list(range(n)))):
            am = torch.full((bs,), sum(1 << g for g in agents), dtype=torch.int64, device="cuda")
            out, off = net.hip_forward_agents(obs, am, cap)
            rows = bs * len(agents)
            assert int(off[-1]) == rows
            assert net.hip_tap(2, bs, cap).tolist()[2] == rows
            logits[name] = raw(out[:rows]).reshape(bs, len(agents), -1)
            cat[name] = raw(net.hip_tap(1, bs, cap)[:rows]).reshape(bs, len(agents), -1)
            assert np.isfinite(logits[name].view(np.float32)).all()
    u1_all = int(net.hip_tap(2, bs, cap)[0])
    assert u1_all == bs * n                          # every node a conv1 target: past the 1 024 slots of that grid too
    for got in (logits, cat):
        np.testing.assert_array_equal(got["one"][:, 0], got["all"][:, 3])
        np.testing.assert_array_equal(got["one"][:, 0], got["sixteen"][:, 3])
        np.testing.assert_array_equal(got["sixteen"], got["all"][:, :16])
