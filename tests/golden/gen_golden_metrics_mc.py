#!/usr/bin/env python3
"""Multichannel fixture of the paired evaluation metrics (MSE / WAPE / ED / CRPS / MRR), made by RUNNING THE REFERENCE's
evaluation.py and Dataset_Construction_Pipeline/Evaluate_Datasets.py on seeded arrays (see gen_golden.py for the rules: the
reference never travels, only the arrays written here are committed).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_metrics_mc.py --reference <checkout of the reference>

Writes metrics_mc.npz: per case k of CASES = (n, L, n_series, G) the fp32 arrays `ori_k`, `gen_k` (n, L, n_series) and
`runs_k` (n, L, n_series, G), what calculate_mse / _wape / _ed (on ori, gen) and calculate_crps / _mrr (on ori, runs, with the
module global `therehold` = 0.5 as evaluation.py:299 sets it) return (`mse_k` ...), and the per-pair cosine similarities
`sims_k` (n, G).  The series are the 7- and 10-channel layout of the motion models, L just above one and two 64-step
strides of the kernels.  Rows with a purpose (ROWS): an all-zero original, a row whose runs are all negated, an exact copy
of the original at a late run index, and one generated series that is exactly constant at 0.5 -- every fp32 partial sum of
L halves is exact, so the reference's own fp32 std is exactly 0 and its `std_dev += 1e-8` branch runs; the observed values
of that series lie above, below and exactly on 0.5.

calculate_dtw is dtaidistance's dtw_ndim.distance, a third-party package that is absent where this fixture was made
(an import-time stub stands in, never called): DTW stays UNPINNED, checked against the restatement only.
G <= 16 keeps numpy's default argsort an insertion sort, i.e. stable: beyond it the reference's tie rule is undefined.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((3, 70, 7, 10), (3, 130, 10, 3))           # (n, L, n_series, G)
ROWS = {"constant": 0, "copy": 0, "zero": 1, "negated": 2}     # row 0 is ordinary but for one series and one run
COPY_RUN = {3: 2, 10: 8}                            # the run index that holds the exact copy, by G
CONST_SERIES, CONST_RUN, THRESHOLD, GRID = 1, 1, 0.5, 32.0


def make_case(n, L, S, G, seed):
    """ori, gen, runs of one case; series j of sample i is scaled by 1 + 0.5 i + 0.25 j so that no two look alike."""
    rs = np.random.RandomState(seed)
    t = np.arange(L, dtype=np.float64)[None, :, None]
    scale = 1.0 + 0.5 * np.arange(n)[:, None, None] + 0.25 * np.arange(S)[None, None, :]
    ori = scale * (0.5 + 0.3 * np.sin(t * rs.uniform(0.05, 0.5, (n, 1, S)) + rs.uniform(0, 2 * np.pi, (n, 1, S)))) + 0.05 * rs.randn(n, L, S)
    gen = ori + 0.2 * rs.randn(n, L, S)
    runs = np.stack([ori + s * scale * rs.randn(n, L, S) for s in np.linspace(0.05, 1.2, G)], axis=-1)
    ori, gen, runs = (np.round(x * GRID) / GRID for x in (ori, gen, runs))     # few mantissa bits: the file stays small
    ori, gen, runs = ori.astype(np.float32), gen.astype(np.float32), runs.astype(np.float32)
    ori[ROWS["zero"]] = 0.0
    runs[ROWS["negated"]] = -runs[ROWS["negated"]]
    r = ROWS["constant"]
    runs[r, :, CONST_SERIES, CONST_RUN] = 0.5
    ori[r, :, CONST_SERIES] = np.where(np.arange(L) % 3 == 0, 0.5, np.where(np.arange(L) % 3 == 1, 0.75, 0.25)).astype(np.float32)
    runs[ROWS["copy"], :, :, COPY_RUN[G]] = ori[ROWS["copy"]]
    return ori, gen, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ref = os.path.abspath(ap.parse_args().reference)
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    dt, dn = types.ModuleType("dtaidistance"), types.ModuleType("dtaidistance.dtw_ndim")
    dn.distance = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("dtaidistance is not installed"))
    dt.dtw_ndim = dn
    sys.modules.update({"dtaidistance": dt, "dtaidistance.dtw_ndim": dn})
    os.chdir(HERE)                                   # '' on sys.path must not resolve to a checkout of this project
    sys.path.insert(0, ref)
    import evaluation as E
    from Dataset_Construction_Pipeline.Evaluate_Datasets import cosine_similarity
    for mod in ("evaluation", "Dataset_Construction_Pipeline.Evaluate_Datasets"):
        assert sys.modules[mod].__file__.startswith(ref + os.sep), (mod, sys.modules[mod].__file__)
    E.therehold = THRESHOLD                          # module global set in __main__ (evaluation.py:299)
    out = {}
    for k, (n, L, S, G) in enumerate(CASES):
        ori, gen, runs = make_case(n, L, S, G, 5200 + k)
        const = runs[ROWS["constant"], :, CONST_SERIES, CONST_RUN]
        assert const.std() == 0 and const.mean() == np.float32(0.5), "the reference's fp32 std of the constant series must be 0"
        sims = np.asarray([[np.mean(cosine_similarity(ori[i], runs[i, :, :, g])) for g in range(G)] for i in range(n)])
        out.update({f"ori_{k}": ori, f"gen_{k}": gen, f"runs_{k}": runs, f"sims_{k}": sims,
                    f"mse_{k}": E.calculate_mse(ori, gen), f"wape_{k}": E.calculate_wape(ori, gen),
                    f"ed_{k}": E.calculate_ed(ori, gen), f"crps_{k}": E.calculate_crps(ori, runs),
                    f"mrr_{k}": E.calculate_mrr(ori, runs)})
        print(f"case {k} {(n, L, S, G)}: MSE {out[f'mse_{k}']:.6f} WAPE {out[f'wape_{k}']:.6f} ED {out[f'ed_{k}']:.6f} "
              f"CRPS {out[f'crps_{k}']:.6f} MRR {out[f'mrr_{k}']:.6f}")
    path = os.path.join(HERE, "metrics_mc.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"metrics_mc.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
