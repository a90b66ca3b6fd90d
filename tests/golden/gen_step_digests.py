"""Writes tests/golden/step_digests.json: per case of tests/test_gpu_step_digests.py CASES, the sha256 of everything a prompt pass of 12 ids and six
token steps leave behind on this GPU (the tokens, the final logits and position, every block's cache tensors, a lookup runner's history and
state block) and of the case's inputs, with the commit, the HIP version and the device it ran on.  tests/test_gpu_step_digests.py recomputes
and compares: runners must be built, and token steps must run, to the same bytes.

    python tests/golden/gen_step_digests.py [--commit HASH] [--out FILE]

Regenerate only on a commit whose runners are the ones to hold every later one to -- never on the commit under test.  The OWQ case needs
transformers (its model is tests/test_gpu_owq_runner.py's); without it the case is left out, and the test skips it."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the tree is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "step_digests.json"))
    args = ap.parse_args()
    import pytest
    import torch
    from test_gpu_step_digests import CASES, digest
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    doc = {"commit": commit, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0), "cases": {}}
    for key in CASES:
        torch.manual_seed(0)                    # (what tests/conftest.py does in front of every test)
        try:
            doc["cases"][key] = digest(key)
        except pytest.skip.Exception as e:
            print("left out:", key, e)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
