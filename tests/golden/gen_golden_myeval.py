#!/usr/bin/env python3
"""Fixture of the motion-run evaluation (t2s_eval_runs, metrics.motion_runs, myevaluation.py), made by RUNNING THE REFERENCE's
myevaluation.py on seeded clips (see gen_golden.py for the rules: the reference never travels, only the arrays written here are
committed).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_myeval.py --reference <checkout of the reference>

Writes myeval.npz.  Per case k of CASES = (C, R, lengths) and clip i: `x1_k_i` (C, T_i) the recording and `xt_k_i` (R, C, T_i)
its R samples (fp32 on a coarse grid), `n1_k_i` / `nt_k_i` what the reference's normalize() returns for them, `runs_k_i` (R, 3)
what calculate_mse / _wape / _ed return for ONE run (ori = that normalised sample, gen = the normalised recording, as the
reference's __main__ hands them over), and per case `ref_k` (K, 6): evaluate_data(..., "MSE,WAPE,ED,ACD,SD,KD") of every clip,
in that order.  Rows with a purpose (rows()): a constant channel in a recording, a constant channel in one sample, a sample that
equals its recording exactly (every metric an exact 0), and a run whose every channel is constant (its normalised sample is all
zeros: WAPE is NaN for that run and the clip's nanmean skips it).

calculate_dtw is dtaidistance's dtw_ndim.distance, a third-party package that is absent where this fixture was made (an
import-time stub stands in, never called): DTW stays UNPINNED, checked against tests/_eval_paired_ref.dtw only.  MRR and CRPS
index gen_data.shape[3] on these 3-D arrays and raise IndexError in the reference; they are not part of the fixture.

Before writing, the fp64 restatement tests/_myeval_ref.py is held to the reference's float32 results at rtol 1e-6 on every
case, so that the tests' bar of 2e-6 hides nothing."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((7, 3, (8, 63, 64, 65, 130)), (10, 10, (8, 65)))      # (C, R, lengths)
GRID = 32.0
METHODS = "MSE,WAPE,ED,ACD,SD,KD"


def rows(K, R):
    """(clip, run, channel) of the rows with a purpose, for K clips and R runs."""
    return {"const_x1": (0, None, 2), "const_sample": (1 % K, 1, 3), "copy": (2 % K, R - 1, None), "flat_run": (3 % K, 0, None)}


def make_case(C, R, lengths, seed):
    """x1 [K] (C, T_i), xt [K] (R, C, T_i); channel c is scaled by 1 + 0.5 c so that no two look alike."""
    rs = np.random.RandomState(seed)
    x1, xt = [], []
    for T in lengths:
        t = np.arange(T, dtype=np.float64)[None, :]
        scale = (1.0 + 0.5 * np.arange(C))[:, None]
        x = scale * (0.5 + 0.3 * np.sin(t * rs.uniform(0.05, 0.5, (C, 1)) + rs.uniform(0, 2 * np.pi, (C, 1)))) + 0.05 * rs.randn(C, T)
        s = np.stack([x + (0.1 + 0.1 * r) * scale * rs.randn(C, T) for r in range(R)])
        x1.append((np.round(x * GRID) / GRID).astype(np.float32))       # few mantissa bits: the file stays small
        xt.append((np.round(s * GRID) / GRID).astype(np.float32))
    w = rows(len(lengths), R)
    clip, _, c = w["const_x1"]
    x1[clip][c] = 1.25
    clip, r, c = w["const_sample"]
    xt[clip][r, c] = -0.75
    clip, r, _ = w["copy"]
    xt[clip][r] = x1[clip]
    clip, r, _ = w["flat_run"]
    xt[clip][r] = (0.5 * np.arange(C, dtype=np.float32))[:, None]
    return x1, xt


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
    import myevaluation as E
    for mod in ("myevaluation", "evaluate.feature_based_measures", "evaluate.utils"):
        assert sys.modules[mod].__file__.startswith(ref + os.sep), (mod, sys.modules[mod].__file__)
    sys.path.insert(1, os.path.dirname(HERE))        # tests/: the restatement under test
    import _myeval_ref as R
    assert R.__file__.startswith(os.path.dirname(HERE) + os.sep), R.__file__
    args = types.SimpleNamespace(method_list=METHODS, device="cpu")
    out = {}
    for k, (C, runs, lengths) in enumerate(CASES):
        x1, xt = make_case(C, runs, lengths, 7300 + k)
        table = []
        for i in range(len(lengths)):
            n1 = E.normalize(x1[i])
            nt = np.stack([E.normalize(xt[i][r]) for r in range(runs)])
            assert n1.dtype == np.float32 and nt.dtype == np.float32
            ori, gen = np.array(list(nt)), np.array([n1] * runs)          # as the reference's __main__ stacks them
            with np.errstate(all="ignore"):
                res = E.evaluate_data(args, ori, gen, i, {})[i]
                per = np.array([[E.calculate_mse(ori[r:r + 1], gen[r:r + 1]), E.calculate_wape(ori[r:r + 1], gen[r:r + 1]),
                                 E.calculate_ed(ori[r:r + 1], gen[r:r + 1])] for r in range(runs)], dtype=np.float64)
            table.append([float(res[m]) for m in METHODS.split(",")])
            out.update({f"x1_{k}_{i}": x1[i], f"xt_{k}_{i}": xt[i], f"n1_{k}_{i}": n1, f"nt_{k}_{i}": nt, f"runs_{k}_{i}": per})
        table = np.asarray(table, dtype=np.float64)
        out[f"ref_{k}"] = table
        # the restatement against the reference, before anything is written
        _, clips, per_run, norm1, normt = R.evaluate(x1, [[xt[i][r] for i in range(len(lengths))] for r in range(runs)])
        for i in range(len(lengths)):
            assert np.array_equal(norm1[i].view(np.uint32), out[f"n1_{k}_{i}"].view(np.uint32)), (k, i)
            assert np.array_equal(normt[i].view(np.uint32), out[f"nt_{k}_{i}"].view(np.uint32)), (k, i)
            np.testing.assert_allclose(per_run[i][:, :3], out[f"runs_{k}_{i}"], rtol=1e-6, atol=0, equal_nan=True)
        np.testing.assert_allclose(clips[:, :3], table[:, :3], rtol=1e-6, atol=0, equal_nan=True)
        worst = np.nanmax(np.abs(clips[:, :3] - table[:, :3]) / np.where(table[:, :3] != 0, np.abs(table[:, :3]), 1.0))
        print(f"case {k} C={C} R={runs} lengths={lengths}: restatement within {worst:.2e} of the reference")
        for i, row in enumerate(table):
            print(f"  clip {i}: " + " ".join(f"{m} {v:.6f}" for m, v in zip(METHODS.split(","), row)))
    path = os.path.join(HERE, "myeval.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"myeval.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
