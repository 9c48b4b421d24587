#!/usr/bin/env python3
"""Fixture of the feature-based measures (MDD / ACD / SD / KD), made by RUNNING THE REFERENCE's
evaluate/feature_based_measures.py on seeded arrays (see gen_golden.py for the rules: the reference never travels, only
the arrays written here are committed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_features.py --reference <checkout of the reference>

Writes features.npz: per case k of CASES the two sets `ori_k` / `gen_k` (n, L, n_series) fp32, the four values
calculate_mdd / _acd / _sd / _kd return (`mdd_k` ...), acf_torch / skew_torch / kurtosis_torch of each set (`acf_ori_k`
(K, n_series), `skew_gen_k` (n_series) ...) and HistoLoss.compute's per-column vector `mdd_cols_k` (n_series * L,
channel-major as the reference lists it).

MDD counts values per bin, and a value ON a bin edge may fall either way under another, equally valid fp32 evaluation
order.  The fixture therefore holds no such value: `snap_off_edges` moves every value that lies within MARGIN bin widths
of an edge (computed in fp64) to a quarter-bin offset inside its own bin, never a column's min or max, and `edge_margin`
asserts the result.  tests/test_feature_metrics.py imports both for the data it draws itself.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((37, 24, 1), (33, 70, 3), (20, 130, 2))      # (n, L, n_series): K = L < 64; just over 64 lags; across a 128 tile
BINS, MARGIN = 50, 1e-3


def make_sets(n, L, S, seed):
    """ori: a smooth-plus-noise series in roughly [0, 1]; gen: ori plus a skewed heavy-tailed perturbation and an offset."""
    rs = np.random.RandomState(seed)
    t = np.arange(L, dtype=np.float64)[None, :, None]
    ori = 0.5 + 0.3 * np.sin(t * rs.uniform(0.1, 0.6, (n, 1, S)) + rs.uniform(0, 2 * np.pi, (n, 1, S))) + 0.1 * rs.randn(n, L, S)
    gen = ori + 0.15 * rs.randn(n, L, S) ** 3 + 0.05
    return ori.astype(np.float32), gen.astype(np.float32)


def _positions(ori, x):
    """Bin coordinate (x - a) / (b - a) * 50 of every value of x on its column's real range, in fp64."""
    o = ori.astype(np.float64)
    a, b = o.min(axis=0, keepdims=True), o.max(axis=0, keepdims=True)
    b = np.where(b == a, a + 1e-5, b)
    return (x.astype(np.float64) - a) / (b - a) * BINS, a, (b - a) / BINS


def _judged(ori, x, real):
    """Which values the margin applies to: real values other than a column's min / max; fake values within one bin of
    the real range."""
    pos, _, _ = _positions(ori, x)
    if real:
        return (x != ori.min(axis=0, keepdims=True)) & (x != ori.max(axis=0, keepdims=True))
    return (pos >= -1.0) & (pos <= BINS + 1.0)


def edge_margin(ori, x, real):
    """The smallest distance, in bin widths, of a judged value of x from a bin edge of its column."""
    pos, _, _ = _positions(ori, x)
    dist = np.abs(pos - np.round(pos))
    sel = _judged(ori, x, real)
    return float(dist[sel].min()) if sel.any() else float("inf")


def snap_off_edges(ori, x, real):
    """x with every judged value closer than MARGIN bin widths to an edge moved to the quarter of its bin; -> (x, moved)."""
    pos, a, delta = _positions(ori, x)
    near = (np.abs(pos - np.round(pos)) < MARGIN) & _judged(ori, x, real)
    k = np.floor(pos)
    if real:
        k = np.clip(k, 0, BINS - 1)
    out = np.where(near, a + (k + 0.25) * delta, x.astype(np.float64)).astype(np.float32)
    return out, int(near.sum())


def snapped_sets(n, L, S, seed):
    ori, gen = make_sets(n, L, S, seed)
    ori, moved_o = snap_off_edges(ori, ori, real=True)
    gen, moved_g = snap_off_edges(ori, gen, real=False)
    assert edge_margin(ori, ori, True) >= MARGIN and edge_margin(ori, gen, False) >= MARGIN
    assert (ori.max(axis=0) > ori.min(axis=0)).all(), "a constant real column"
    return ori, gen, moved_o + moved_g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ref = os.path.abspath(ap.parse_args().reference)
    sys.dont_write_bytecode = True
    import torch
    torch.set_num_threads(8)
    sys.path.insert(0, ref)
    import evaluate.feature_based_measures as F
    assert F.__file__.startswith(ref + os.sep), F.__file__
    out = {}
    for k, (n, L, S) in enumerate(CASES):
        ori, gen, moved = snapped_sets(n, L, S, 4100 + k)
        to, tg = torch.from_numpy(ori), torch.from_numpy(gen)
        K = min(64, L)
        out.update({f"ori_{k}": ori, f"gen_{k}": gen,
                    f"mdd_{k}": F.calculate_mdd(to, tg), f"acd_{k}": F.calculate_acd(to, tg),
                    f"sd_{k}": F.calculate_sd(to, tg), f"kd_{k}": F.calculate_kd(to, tg),
                    f"mdd_cols_{k}": F.HistoLoss(to, n_bins=BINS, name="marginal_distribution").compute(tg).detach().numpy()})
        for name, x in (("ori", to), ("gen", tg)):
            out[f"acf_{name}_{k}"] = F.acf_torch(x, K).numpy()
            out[f"skew_{name}_{k}"] = F.skew_torch(x).numpy()
            out[f"kurt_{name}_{k}"] = F.kurtosis_torch(x).numpy()
        print(f"case {k} {(n, L, S)}: moved {moved} values off bin edges; MDD {out[f'mdd_{k}']:.6f} ACD {out[f'acd_{k}']:.6f} "
              f"SD {out[f'sd_{k}']:.6f} KD {out[f'kd_{k}']:.6f}")
    path = os.path.join(HERE, "features.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"features.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
