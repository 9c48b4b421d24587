"""Per-sample fp64 numpy restatements of the five paired evaluation entries of csrc/t2s_eval.hip (t2s_eval_mse_wape, _ed,
_crps, _dtw, _mrr), after the definitions at the head of that file and in include/t2s.h.  tests/test_eval_paired_host.py
pins them to the oracle and to the reference-made fixtures on the CPU; tests/test_eval_paired.py judges the kernels by them.

Every function takes ori (n, L, S) and returns fp64 arrays with one entry per sample; the runs of CRPS / MRR come as one
(n, L, S, G) array (the trailing-axis form evaluation.py stacks).  Non-finite inputs are not special-cased anywhere but in
MRR (whose contract is "0 where not finite"): whatever IEEE arithmetic and numpy's NaN-propagating minimum give is the answer.
"""
import numpy as np
from scipy.special import erfc

U = 2.0 ** -24            # unit roundoff of fp32


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def mse_wape(ori, gen):
    """(mse_i, wape_i): mean over (L, S) of (ori - gen)^2; sum |ori - gen| / sum |ori|, NaN when that sum is 0."""
    a, b = _f64(ori), _f64(gen)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = a - b
        mse = (d * d).sum(axis=1) / a.shape[1]
        ae, av = np.abs(d).sum(axis=1), np.abs(a).sum(axis=1)
        wape = np.where(av != 0, ae / np.where(av != 0, av, 1.0), np.nan)
    return mse, wape


def nanmean(v):
    """The mean over the entries that are not NaN; NaN when there is none (what out[1] of t2s_eval_mse_wape holds)."""
    v = np.asarray(v, dtype=np.float64)
    keep = ~np.isnan(v)
    return float(v[keep].sum() / keep.sum()) if keep.any() else float("nan")


def ed(ori, gen):
    """ed_i: the mean over series of the Euclidean distance over time."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = _f64(ori) - _f64(gen)
        return np.sqrt((d * d).sum(axis=1)).mean(axis=1)


def crps(ori, runs):
    """crps_i in the kernel's documented arithmetic: per (sample, series, run) the mean and the population std over time in
    fp64, each rounded ONCE to fp32, a std of exactly 0 replaced by 1e-8f; the step `obs < mean ? 0 : 1` on the fp32 values;
    Phi in fp64; mean over time of (step - Phi)^2, then over runs and series."""
    obs32 = np.asarray(ori, dtype=np.float32)
    g = _f64(runs)                                                   # (n, L, S, G)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mean64 = g.mean(axis=1)                                      # (n, S, G)
        std64 = np.sqrt(((g - mean64[:, None]) ** 2).mean(axis=1))
        mean32, std32 = mean64.astype(np.float32), std64.astype(np.float32)
        std32 = np.where(std32 == 0, np.float32(1e-8), std32).astype(np.float32)
        step = np.where(obs32[..., None] < mean32[:, None], 0.0, 1.0)                          # (n, L, S, G)
        z = (obs32.astype(np.float64)[..., None] - mean32.astype(np.float64)[:, None]) / std32.astype(np.float64)[:, None]
        cdf = 0.5 * erfc(-z * 0.70710678118654752440)
        return ((step - cdf) ** 2).mean(axis=1).mean(axis=2).mean(axis=1)


def dtw(ori, gen):
    """dtw_i: sqrt of the minimal warping-path cost with squared-Euclidean point costs (dtaidistance dtw_ndim.distance
    without window or penalty -- the recurrence of oracle.eval_dtw).  The L x L table is walked by anti-diagonals: the
    cells of one are independent, so each is one numpy expression over all samples, and the point costs are computed per
    diagonal; three diagonals are alive at a time.  Row i of a diagonal is kept at index i + 1, index 0 stays +inf."""
    a, b = _f64(ori), _f64(gen)
    n, L, _ = a.shape
    p1 = np.full((n, L + 1), np.inf)
    p2 = np.full((n, L + 1), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(2 * L - 1):
            i = np.arange(max(0, d - (L - 1)), min(d, L - 1) + 1)
            df = a[:, i] - b[:, d - i]
            c = (df * df).sum(axis=2)
            if d == 0:
                best = np.zeros((n, 1))
            else:
                best = np.minimum(p2[:, i], np.minimum(p1[:, i], p1[:, i + 1]))   # (i-1, j-1); (i-1, j); (i, j-1)
            cur = np.full((n, L + 1), np.inf)
            cur[:, i + 1] = c + best
            p2, p1 = p1, cur
        return np.sqrt(p1[:, L])


def cosine(ori, runs):
    """(n, G) fp64 similarities <ori, gen_g> / (|ori| |gen_g|) over the flattened (L, S) values, 0 where not finite."""
    a = _f64(ori).reshape(np.shape(ori)[0], -1)
    g = _f64(runs)
    g = g.reshape(g.shape[0], -1, g.shape[-1])                       # (n, L * S, G)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ab = (a[:, :, None] * g).sum(axis=1)
        den = np.sqrt((a * a).sum(axis=1))[:, None] * np.sqrt((g * g).sum(axis=1))
        s = ab / den
    return np.where(np.isfinite(s), s, 0.0)


def mrr(ori, runs, threshold=0.5):
    """(sims (n, G) fp64, score_i): the best run is searched on the similarities rounded to fp32, as the entry stores them;
    among equal similarities the largest run index wins; score_i = 1 / (g* + 1) in fp32 when sim_{g*} > threshold, else 0."""
    sims = cosine(ori, runs)
    s32 = sims.astype(np.float32)
    G = s32.shape[1]
    best = G - 1 - np.argmax(s32[:, ::-1], axis=1)
    top = s32[np.arange(s32.shape[0]), best]
    score = np.where(top > np.float32(threshold), np.float32(1.0) / (best + 1).astype(np.float32), np.float32(0.0))
    return sims, score.astype(np.float64)
