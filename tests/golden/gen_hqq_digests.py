"""Writes tests/golden/hqq_digests.json: per case of tests/quantize_common.py HQQ_DIGEST_CASES, the sha256 of the bytes of W_q, scale, zero and the
info block that ops.hqq_quantize gives on this GPU for the seeded ``multi_w(N, K)`` of tests/test_gpu_hqq_quantize.py, with the commit and the HIP
version it ran on.  tests/test_gpu_hqq_quantize.py recomputes and compares: the HQQ kernels must keep their bits.

    python tests/golden/gen_hqq_digests.py [--commit HASH] [--out FILE]

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
    ap.add_argument("--out", default=os.path.join(HERE, "hqq_digests.json"))
    args = ap.parse_args()
    import torch
    from amq_amd import ops
    from quantize_common import HQQ_DIGEST_CASES, hqq_digest, hqq_digest_key
    from test_gpu_hqq_quantize import multi_w
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    doc = {"commit": commit, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N, K, group, bits in HQQ_DIGEST_CASES:
        h, info = ops.hqq_quantize(multi_w(N, K).to("cuda:0"), bits, group, return_info=True)
        doc["cases"][hqq_digest_key(N, K, group, bits)] = hqq_digest(h, info)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
