"""Record the 4-head logits tests/test_gpu_head_shapes.py::test_existing_shapes_keep_their_bits compares against (needs a GPU).

Run:  python tests/golden/make_head_shapes_golden.py --commit <hash>
      IN A CHECKOUT OF THE PARENT of the commit that is to be pinned, with this file and that commit's
      tests/test_gpu_head_shapes.py copied in.

The fixture holds what the code BEFORE a change computed, never what the tree under test computes: it was recorded at the last
commit whose attention kernels knew full wavefronts only, so it pins the (128 hidden, 4 heads) instantiations to their bits
from before the idle-lane instantiations were added.  Cases, inputs and the forward come from the test module (PARENT_CASES,
parent_case_logits), so recorder and test cannot drift apart.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_head_shapes as t      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of this checkout (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=t.PARENT_GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = dict(commit=np.array(commit))
    for model, agg in t.PARENT_CASES:
        out[f"{model}_{agg}"] = t.parent_case_logits(model, agg)
        print(model, agg, out[f"{model}_{agg}"].tolist(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(t.PARENT_CASES)} cases at {commit}")


if __name__ == "__main__":
    main()
