"""Pure-Python statement of the SAMPLED prompt-lookup step (amq_lookup.hip: decode_tail_lookup_sample_kernel; include/amq_hip.h): tests/lookup_ref.py
with every row's drawn token in the place of its arg-max, plus the rule of the draw counter.  No torch, no GPU.

Row j of a step that starts with draw counter c draws with counter c + j; the step emits drawn[0 .. n] and leaves the counter at c + n + 1, so the
token emitted at index i of the sequence is always drawn with counter i."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref  # noqa: E402

MASK64 = (1 << 64) - 1


def step(history, drafts, drawn, D, ngram_max, external=False, counter=0):
    """one sampled verify-and-propose step on the host: -> (n, new history, next drafts, new draw counter)"""
    n, new, nxt = lookup_ref.step(history, drafts, drawn, D, ngram_max, external)
    return n, new, nxt, (counter + n + 1) & MASK64


def step_brute(history, drafts, drawn, D, ngram_max, external=False, counter=0):
    """the same step restated token by token: the sequence grows by one draw at a time, each consuming one counter value, and goes on into the next
    row only while that row was run with the token just emitted"""
    seq, c, j = list(history), counter, 0
    while True:
        seq.append(drawn[j])                        # emitted index len(seq) - len(history) - 1 of this step, drawn with counter `counter + j`
        c = (c + 1) & MASK64
        if j >= D or j >= len(drafts) or drafts[j] < 0 or drafts[j] != drawn[j]:
            break
        j += 1
    return j, seq, ([-1] * D if external else lookup_ref.propose_brute(seq, D, ngram_max)), c
