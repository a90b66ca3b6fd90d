#!/usr/bin/env python3
"""Golden values for the evaluation metrics (amq_amd/evaluate.py, ops.logit_jsd), from the REAL reference on CPU.

Run only in the build container (needs /root/reference).  The reference's ``amq/utils/loss.py`` and ``amq/utils/eval.py`` are loaded by file
path under a stub ``utils`` package (importing the package itself pulls in hqq); its ``eval_loss`` / ``eval_ppl`` run with a stub accelerator
(``gather_for_metrics`` = identity) and stub models that return recorded logits as fp32, the way its FT forward does.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_evalmetrics.py

``evalmetrics.npz`` (fp16 tensors stored as their uint16 bit patterns; only inputs and recorded results):
  ids              int64 [3, 1, 12]        three token windows
  logits           fp16 bits [3, 1, 12, 500]   the scored model's logits per window
  dense            fp16 bits [3, 1, 12, 500]   the dense model's
  seqlen           12
  eval_loss        reference eval_loss(model, acc, loader, dense_logits_list, seqlen)
  eval_ppl         reference eval_ppl(model, acc, loader, seqlen)
  jsd_same_p       fp16 bits [2, 1000];  jsd_same = JSD()(p, p)  (negative: the mixture is clamped at eps)
  jsd_wide_p/q     fp16 bits [3, 100], standard deviation 8 (about two thirds of the entries clamped);  jsd_wide = JSD()(p, q)
  jsd_near_p/q     fp16 bits [2, 1000], q = p + noise of 0.05;  jsd_near = JSD()(p, q)
(every JSD value is the reference's 'batchmean' over the rows, on .float() inputs)
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference/amq/utils"
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def bits_of(t):
    import torch
    assert t.dtype == torch.float16
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    sys.dont_write_bytecode = True
    import torch
    pkg = types.ModuleType("utils")
    pkg.__path__ = []
    sys.modules["utils"] = pkg
    loss = _load("utils.loss", os.path.join(REF, "loss.py"))
    ev = _load("utils.eval", os.path.join(REF, "eval.py"))

    torch.manual_seed(20261)
    W, S, V = 3, 12, 500
    ids = torch.randint(0, V, (W, 1, S))
    logits = (torch.randn(W, 1, S, V) * 3.0).to(torch.float16)
    dense = (logits.float() + 0.3 * torch.randn(W, 1, S, V)).to(torch.float16)

    class Out:
        def __init__(self, lg):
            self.logits = lg

    class Model:
        """returns the recorded logits of the window it is called with, as fp32"""
        def __init__(self, rows):
            self.rows = rows

        def __call__(self, inputs):
            for w in range(W):
                if inputs is loader[w]:
                    return Out(self.rows[w].float())
            raise KeyError("unknown window")

    class Acc:
        def gather_for_metrics(self, x):
            return x

    loader = [ids[w] for w in range(W)]
    dense_list = torch.cat([dense[w].float() for w in range(W)], dim=0)          # what get_logits returns: [windows * B, S, V]
    out = {"ids": ids.numpy(), "logits": bits_of(logits), "dense": bits_of(dense), "seqlen": np.int32(S),
           "eval_loss": np.float64(ev.eval_loss(Model(logits), Acc(), loader, dense_list, seqlen=S)),
           "eval_ppl": np.float64(ev.eval_ppl(Model(logits), Acc(), loader, seqlen=S))}

    jsd = loss.JSD()
    p = (torch.randn(2, 1000) * 6.0).to(torch.float16)
    out["jsd_same_p"], out["jsd_same"] = bits_of(p), np.float64(jsd(p.float(), p.float()).item())
    p, q = (torch.randn(3, 100) * 8.0).to(torch.float16), (torch.randn(3, 100) * 8.0).to(torch.float16)
    out["jsd_wide_p"], out["jsd_wide_q"], out["jsd_wide"] = bits_of(p), bits_of(q), np.float64(jsd(p.float(), q.float()).item())
    p = (torch.randn(2, 1000) * 3.0).to(torch.float16)
    q = (p.float() + 0.05 * torch.randn(2, 1000)).to(torch.float16)
    out["jsd_near_p"], out["jsd_near_q"], out["jsd_near"] = bits_of(p), bits_of(q), np.float64(jsd(p.float(), q.float()).item())
    assert out["jsd_same"] < 0.0
    path = os.path.join(HERE, "evalmetrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(v) for k, v in out.items() if np.ndim(v) == 0})


if __name__ == "__main__":
    main()
