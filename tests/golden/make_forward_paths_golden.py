"""Record what tests/test_gpu_forward_paths.py compares against: logits, row offsets, table rows and launches per stage of every
forward route, at the commit BEFORE a change to the forward's host code (needs a GPU).

Run:  python tests/golden/make_forward_paths_golden.py --commit <hash>
      IN A CHECKOUT OF THE PARENT of the commit that is to be pinned, with this file and that commit's
      tests/test_gpu_forward_paths.py copied in.

The fixture holds what the code before the change computed and launched, never what the tree under test does.  Cases, inputs and
the runner come from the test module (CASES, run_case), so recorder and test cannot drift apart.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import test_gpu_forward_paths as t      # noqa: E402


def main():
    from melissa_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of this checkout (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=t.GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = dict(commit=np.array(commit), stage_names=np.array(list(_lib.STAGE_NAMES)))
    for c in t.CASES:
        got = t.run_case(c)
        for name, a in got.items():
            out[f"{c.key}/{name}"] = a
            if name.endswith("/table_rows"):
                assert int(a[0]) == c.table_rows, (c.key, name, int(a[0]))
        print(c.key, {k: v.tolist() for k, v in got.items() if k.endswith("/launches")}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(t.CASES)} cases at {commit}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
