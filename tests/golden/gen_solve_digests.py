"""Writes tests/golden/solve_digests.json: per case of tests/test_gpu_solve_digests.py CASES, the sha256 of the bytes of W_q, scale, zero, row_loss
and the info word (OWQ: W_out and choice too) that ops.gptq_quantize / ops.owq_quantize give on this GPU for that module's seeded inputs, with the
commit and the HIP version it ran on.  tests/test_gpu_solve_digests.py recomputes and compares: the three solves must keep their bits.

    python tests/golden/gen_solve_digests.py [--commit HASH] [--out FILE]

Regenerate only on a commit whose kernels are the ones to hold every later one to."""
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
    ap.add_argument("--out", default=os.path.join(HERE, "solve_digests.json"))
    args = ap.parse_args()
    import torch
    from test_gpu_solve_digests import CASES, digest, key
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    doc = {"commit": commit, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0), "cases": {}}
    for case in CASES:
        doc["cases"][key(*case)] = digest(*case)                    # (asserts that the info word is 0)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
