#!/usr/bin/env python3
"""Compare k motion recordings with each other, as the __main__ of the reference's evaluate/metrics.py (:290-370) compares
its `merged_i.txt` files -- on the GPU, all ordered pairs as one ragged batch, no plotting.

    python tools/compare_recordings.py rec_0.npy rec_1.txt rec_2.npy [--no-normalize]

A recording is a `.npy` array (T, D), or comma-separated text with one time step per line (the fork's merged_i.txt); every
recording needs the same D, the lengths T may differ.  Each column of each recording is min-max normalised on the host
(min_max_normalize_columns, :180-187; a constant column becomes 0) unless --no-normalize is given.  Prints ONE JSON
object: `lengths` and the k x k matrices (entry [i][j] compares recording i with recording j, the diagonal is null)
  CS        correlational score (metrics.correlational_score)      SC_dist / SC_shift   sequence correlation
  DTW       DTW of unequal lengths (metrics.dtw_ragged)            MSE / WAPE           where the two lengths agree (else null)
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def load(path):
    x = np.load(path) if path.endswith(".npy") else np.loadtxt(path, delimiter=",", ndmin=2)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[0] < 1:
        sys.exit(f"compare_recordings: {path} holds an array of shape {x.shape}, expected (T, D)")
    return x


def min_max_normalize_columns(x):
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = hi - lo
    rng[rng == 0] = 1
    return (x - lo) / rng


def compare(recs, device="cuda"):
    """The matrices for a list of (T_i, D) arrays, as a dict of nested lists (None where a measure does not apply)."""
    from t2ms_amd import metrics as M
    k = len(recs)
    pairs = [(i, j) for i in range(k) for j in range(k) if i != j]
    grid = lambda: [[None] * k for _ in range(k)]
    out = {name: grid() for name in ("CS", "SC_dist", "SC_shift", "DTW", "MSE", "WAPE")}
    first, second = [recs[i] for i, _ in pairs], [recs[j] for _, j in pairs]
    _, shift, dist, _ = M.sequence_correlation(first, second, device=device)
    _, dtw = M.dtw_ragged(first, second, device=device)
    for p, (i, j) in enumerate(pairs):
        out["SC_dist"][i][j], out["SC_shift"][i][j], out["DTW"][i][j] = float(dist[p]), int(shift[p]), float(dtw[p])
        out["CS"][i][j] = M.correlational_score(recs[i], recs[j], device=device)[0] if min(len(recs[i]), len(recs[j])) >= 2 else None
        if recs[i].shape == recs[j].shape:
            mse, wape, _ = M.mse_wape(recs[i][None], recs[j][None], device=device)
            out["MSE"][i][j], out["WAPE"][i][j] = mse, wape
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="pairwise motion measures of k recordings")
    ap.add_argument("recordings", nargs="+", help=".npy (T, D) or comma-separated text files")
    ap.add_argument("--no-normalize", action="store_true", help="skip the per-column min-max normalisation")
    a = ap.parse_args(argv)
    if len(a.recordings) < 2:
        sys.exit("compare_recordings: give at least two recordings")
    import torch
    if not torch.cuda.is_available():
        sys.exit("compare_recordings: no GPU visible -- the metrics kernels run on the GPU (no CPU fallback)")
    recs = [load(p) for p in a.recordings]
    if len({r.shape[1] for r in recs}) != 1:
        sys.exit(f"compare_recordings: the recordings have {[r.shape[1] for r in recs]} columns")
    if not a.no_normalize:
        recs = [min_max_normalize_columns(r) for r in recs]
    recs = [r.astype(np.float32) for r in recs]
    result = {"recordings": a.recordings, "lengths": [int(r.shape[0]) for r in recs], "normalized": not a.no_normalize}
    result.update(compare(recs))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
