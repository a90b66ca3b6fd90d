"""Writes tests/golden/runner_options.json: what the QuantLlama constructor answers to every combination of its options in
tests/test_runner_options_cpu.py GRID, as far as its option checks go -- the full message of the ValueError it raises, or "accepted" when it gets
as far as touching the device.  ``llama._prime_graph_state``, the first thing a constructor does with its device, is replaced by a function that
raises a sentinel, so nothing is built and no GPU is needed; the class switch FUSE_QKV_ATTN is set through a subclass.

    python tests/golden/gen_runner_options.py [--commit HASH] [--out FILE]

The file holds the distinct outcomes (index 0: accepted) and one letter per combination, in grid order.  Regenerate only on a commit whose
refusals are the ones to hold every later one to -- never on the commit under test."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


class _Accepted(Exception):
    pass


def _stop(dev):
    raise _Accepted()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the tree is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "runner_options.json"))
    args = ap.parse_args()
    from amq_amd import llama
    from test_runner_options_cpu import ACCEPTED, LETTERS, combinations
    llama._prime_graph_state = _stop
    classes = {False: llama.QuantLlama, True: type("Fused", (llama.QuantLlama,), {"FUSE_QKV_ATTN": True})}
    outcomes, letters = [ACCEPTED], []
    for fuse, config, kw in combinations():
        try:
            classes[fuse](config, **kw)
            raise AssertionError("a runner was built")
        except _Accepted:
            got = ACCEPTED
        except ValueError as e:
            got = str(e)
        if got not in outcomes:
            outcomes.append(got)
        letters.append(LETTERS[outcomes.index(got)])
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "outcomes": outcomes, "grid": "".join(letters)}, f, indent=1)
        f.write("\n")
    print("wrote", args.out, len(letters), "combinations,", letters.count(LETTERS[0]), "accepted,", len(outcomes) - 1, "messages")


if __name__ == "__main__":
    main()
