"""Record the bits of the attention launches' outputs for tests/test_gpu_attention_walk.py (needs a GPU).

Run:  python tests/golden/make_attention_walk_golden.py --label "..."
      IN A CHECKOUT OF THE PARENT of the commit that is to be pinned, with this file and that commit's
      tests/test_gpu_attention_walk.py copied in.

The fixture holds what the code BEFORE a change computed, never what the tree under test computes.  It was first recorded at the
last commit that had the per-step source walk, with that commit's environment switch for it set (read once per process there:
every forward then took that walk; the label in the file names the switch), so it pins the list walk to the former walk's bits.
A later change that alters the forward's arithmetic on purpose records again from ITS parent, with no variable set.

Cases, inputs and the forward itself come from the test module (CASES, run_case), so recorder and test cannot drift apart.  Per
case and output array (the logits, the head input) the file keeps shape, dtype and one zlib.crc32 per row - not the outputs: a
table-mode case has thousands of rows of 1152 floats - plus the commit it was recorded at and the --label string.
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
import test_gpu_attention_walk as t      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True, help="what was recorded, e.g. the walk and the environment it ran under")
    ap.add_argument("--commit", default=None, help="the commit of this checkout (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=t.GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = dict(commit=np.array(commit), label=np.array(args.label))
    assert len({c.key for c in t.CASES}) == len(t.CASES)
    done = 0
    try:                                  # a case that fails ends the run; what was recorded before it is still written
        for c in t.CASES:
            for name, a in t.run_case(c).items():
                out[f"{c.key}/{name}/shape"] = np.array(a.shape, dtype=np.int64)
                out[f"{c.key}/{name}/dtype"] = np.array(str(a.dtype))
                out[f"{c.key}/{name}/crc"] = t.row_checksums(a)
            done += 1
            print(c.key, {name: int(out[f"{c.key}/{name}/shape"][0]) for name in t.ARRAYS}, flush=True)
    finally:
        np.savez_compressed(args.out, **out)
        print(f"{args.out}: {done} of {len(t.CASES)} cases at {commit} ({args.label}), {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
