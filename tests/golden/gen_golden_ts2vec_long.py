#!/usr/bin/env python3
"""Fixture of the long-series TS2Vec encoder, made by RUNNING THE REFERENCE in the build container (see gen_golden.py for
the rules: the reference never travels, only the arrays written here are committed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ts2vec_long.py

Writes
  ts2vec_long.npz   TSEncoder forward of evaluate/ts2vec.py (:352-399, eval mode, mask 'all_true') on the seeded weights
                    of synth.make_ts2vec_state_dict(2025, input_dims=...), at lengths the LDS kernel refuses.  Per case
                    k = 0, 1, 2 with (input_dims, T, B) = (1, 137, 3), (10, 300, 3), (1, 1025, 2): x_k (B, T, input_dims)
                    with a NaN stretch in series 1, rep_k = the per-step representations at every stride_k-th step,
                    full_k = the full-series max pooling, and `cases` = the (input_dims, T, B, stride) rows.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

CASES = ((1, 137, 3, 8), (10, 300, 3, 16), (1, 1025, 2, 32))       # (input_dims, T, B, stride of the stored rep)


def main():
    torch.set_num_threads(8)
    from t2ms_amd import synth
    # the repo's own `evaluate` / `model` packages must not shadow the reference's: see gen_golden_r2.py
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for k in [k for k in sys.modules if k.split(".")[0] in ("model", "datafactory", "evaluate", "evaluation")]:
        del sys.modules[k]
    os.chdir(HERE)
    sys.path.insert(0, REF)
    from evaluate.ts2vec import TSEncoder
    assert sys.modules["evaluate.ts2vec"].__file__.startswith(REF + os.sep)
    out = {"cases": np.asarray(CASES, dtype=np.int64)}
    for k, (cin, T, B, stride) in enumerate(CASES):
        enc = TSEncoder(input_dims=cin, output_dims=100, hidden_dims=64, depth=10).eval()   # initialize_ts2vec's sizes
        print("TSEncoder load_state_dict(strict):", enc.load_state_dict(synth.make_ts2vec_state_dict(2025, input_dims=cin), strict=True))
        xs = torch.from_numpy(np.random.RandomState(80 + k).uniform(0, 1, size=(B, T, cin)).astype(np.float32))
        xs[1, T // 3:T // 3 + 5, 0] = float("nan")           # TSEncoder zeroes time steps that hold a NaN (:367-368)
        with torch.no_grad():
            rep = enc(xs.clone(), mask="all_true")
            full = torch.nn.functional.max_pool1d(rep.transpose(1, 2), kernel_size=rep.size(1)).squeeze(-1)
        assert rep.shape == (B, T, 100) and bool(torch.isfinite(rep).all())
        out[f"x_{k}"], out[f"rep_{k}"], out[f"full_{k}"] = xs.numpy(), rep[:, ::stride].numpy(), full.numpy()
    path = os.path.join(HERE, "ts2vec_long.npz")
    np.savez_compressed(path, **out)
    print(f"ts2vec_long.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
