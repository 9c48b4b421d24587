"""Numpy restatement of what the reference's myevaluation.py computes for one clip (include/t2s_eval_runs.h): fp32 `normalize`
exactly as numpy 2 evaluates the reference's expression on float32 arrays, then the per-run metrics in fp64 on the normalised
fp32 values.  The reference calls evaluate_data(ori = the stacked normalised SAMPLES, gen = the stacked normalised recording),
both (R, C, T), and its metric functions read axis 1 as time and axis 2 as series -- so C plays time and T plays series; with
a = a normalised sample and b = the normalised recording that is what the functions below restate.
tests/test_myeval_host.py pins this file to reference-made values (tests/golden/myeval.npz); tests/test_myeval.py judges
t2s_eval_runs by it.  DTW comes from tests/_eval_paired_ref.dtw (dtaidistance is not installed anywhere the tests run)."""
import numpy as np

import _eval_paired_ref as P

U = P.U                   # unit roundoff of fp32, 2^-24
NAMES = ("MSE", "WAPE", "ED", "DTW")


def worst(got, want):
    """Largest relative error of got against want (fp64); NaN / Inf / an exact 0 in want must be matched exactly (asserted).
    The two bars are stated in it: <= 2e-6 against reference-made values, <= 2 U resp. 3 U for the kernels."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[special], want[special], equal_nan=True), (got[special], want[special])
    if special.all():
        return 0.0
    return float(np.max(np.abs(got[~special] - want[~special]) / np.abs(want[~special])))


def same_bits(a, b):
    """Two fp32 arrays hold the same values bit for bit (NaNs by position: their payload is not part of any contract)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return bool(np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32)))


def normalize(x):
    """myevaluation.normalize on a float32 (C, T) array: min-max per channel row along time, all in float32 (1e-8 is a weak
    scalar under numpy 2).  A NaN in a row makes the whole row NaN, a constant row gives exact zeros."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
        return (x - lo) / ((hi - lo) + np.float32(1e-8))


def per_run(a, b):
    """a (R, C, T) normalised samples, b (C, T) the normalised recording -> (R, 4) fp64 [mse, wape, ed, dtw]."""
    a = np.asarray(a, dtype=np.float32)
    g = np.broadcast_to(np.asarray(b, dtype=np.float32), a.shape)
    mse, wape = P.mse_wape(a, g)          # `ori` is the sample: WAPE divides by sum |a|
    return np.stack([mse, wape, P.ed(a, g), P.dtw(a, g)], axis=1)


def per_clip(runs):
    """(R, 4) -> (4,): the reference's reductions over a clip's runs -- mean, nanmean, mean, mean."""
    runs = np.asarray(runs, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.array([runs[:, 0].mean(), P.nanmean(runs[:, 1]), runs[:, 2].mean(), runs[:, 3].mean()])


def evaluate(x1_list, xt_runs):
    """K recordings (C, T_i) and R runs of K samples -> (summary (4,), per_clip (K, 4), per_run (K, R, 4), norm1 [K], normt [K]
    each (R, C, T_i)); summary is the plain mean over clips, as the reference's summary (a NaN clip value propagates)."""
    norm1 = [normalize(x) for x in x1_list]
    normt = [np.stack([normalize(run[i]) for run in xt_runs]) for i in range(len(x1_list))]
    runs = np.stack([per_run(normt[i], norm1[i]) for i in range(len(x1_list))])
    clips = np.stack([per_clip(r) for r in runs])
    with np.errstate(invalid="ignore"):
        return clips.mean(axis=0), clips, runs, norm1, normt


def _set_stats(x):
    """acf (S, K), skewness (S,), excess kurtosis (S,) of one (n, L, S) set, K = min(64, L): the definitions
    tests/test_feature_metrics.py restates for the feature kernels (evaluate/feature_based_measures.py of the reference)."""
    x = np.asarray(x, dtype=np.float64)
    n, length, _ = x.shape
    d = x - x.mean(axis=(0, 1))
    var = (d ** 2).mean(axis=(0, 1))
    acf = np.stack([(d[:, k:] * d[:, :length - k]).mean(axis=(0, 1)) / var for k in range(min(64, length))], axis=1)
    skew = (d ** 3).mean(axis=(0, 1)) / (np.sqrt((d ** 2).sum(axis=(0, 1)) / (n * length - 1))) ** 3
    return acf, skew, (d ** 4).mean(axis=(0, 1)) / var ** 2 - 3.0


def feature_measures(ori, gen):
    """(ACD, SD, KD) of the two (R, C, T) sets as the reference's evaluate_data hands them to calculate_acd / _sd / _kd."""
    (ao, so, ko), (ag, sg, kg) = _set_stats(ori), _set_stats(gen)
    return np.array([np.sqrt(((ag - ao) ** 2).sum(axis=1)).mean(), np.abs(sg - so).mean(), np.abs(kg - ko).mean()])
