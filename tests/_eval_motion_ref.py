"""fp64 numpy restatements of the three motion entries of csrc/t2s_eval_motion.hip (t2s_eval_corr, t2s_eval_shift,
t2s_eval_dtw_ragged) in their documented arithmetic (the head of that file and include/t2s.h).
tests/test_eval_motion_host.py pins them on the CPU to tests/golden/motion_metrics.npz, which the reference's own
evaluate/metrics.py made; tests/test_eval_motion.py judges the kernels by them.

Non-finite inputs are not special-cased: whatever IEEE arithmetic gives is the answer.  The shift search runs on the
distances rounded to fp32, as the entry stores them, with the reference's left-to-right rule."""
import numpy as np

from _eval_paired_ref import U, _f64      # noqa: F401  (U: the unit roundoff of fp32, for the tests)


def corr_matrix(x):
    """(S, S) fp64: np.corrcoef(rowvar=False) of the (rows, S) view of x, restated -- channel means, centred co-moments,
    c_ij / sqrt(c_ii) / sqrt(c_jj) (two divisions), clipped to [-1, 1]; a NaN stays a NaN."""
    x = _f64(x)
    x = x.reshape(-1, x.shape[-1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - x.sum(axis=0) / x.shape[0]
        c = d.T @ d
        sd = np.sqrt(np.diag(c))
        r = c / sd[:, None]
        r = r / sd[None, :]
        return np.where(r > 1, 1.0, np.where(r < -1, -1.0, r))


def corr_score(ori, gen):
    """(score, corr (2, S, S)) in fp64: 1 - sum |C_ori - C_gen| / sum |C_ori|, NaN when that denominator is exactly 0."""
    c = np.stack([corr_matrix(ori), corr_matrix(gen)])
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.abs(c[0]).sum()
        score = np.nan if den == 0 else 1.0 - np.abs(c[0] - c[1]).sum() / den
    return float(score), c


def lengths_of(x, lens):
    return np.full(x.shape[0], x.shape[1], dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)


def shift_distances(a, b):
    """{shift: fp64 mean point distance} of ONE pair a (m, S), b (n, S), in the order the reference visits the shifts."""
    a, b = _f64(a), _f64(b)
    m, n = a.shape[0], b.shape[0]
    M = min(m, n) - 1
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(-M, M + 1):
            if s >= 0:
                ov = min(m, n - s)
                d = a[:ov] - b[s:s + ov]
            else:
                ov = min(m + s, n)
                d = a[-s:-s + ov] - b[:ov]
            out[s] = np.sqrt((d * d).sum(axis=1)).sum() / ov
    return out


def search(values32):
    """The reference's min(keys, key=...) over a sequence of fp32 values visited left to right: a later one wins only if it
    is strictly smaller (so a NaN never wins, and a NaN at the front never loses) -> its position."""
    best = 0
    for k in range(1, len(values32)):
        if values32[k] < values32[best]:
            best = k
    return best


def shift(a, b, len_a=None, len_b=None):
    """(table (n, W) fp64 with NaN where a pair has no such shift, best_shift (n,) int, min_dist (n,) fp64) for the padded
    a (n, La, S), b (n, Lb, S); the search runs on the table rounded to fp32 and min_dist is that row's fp64 value."""
    n, La, Lb = a.shape[0], a.shape[1], b.shape[1]
    la, lb = lengths_of(a, len_a), lengths_of(b, len_b)
    zero = min(La, Lb) - 1
    table = np.full((n, 2 * zero + 1), np.nan)
    best, dist = np.zeros(n, dtype=np.int64), np.zeros(n)
    for i in range(n):
        d = shift_distances(a[i, :la[i]], b[i, :lb[i]])
        keys = list(d)
        for s in keys:
            table[i, zero + s] = d[s]
        with np.errstate(invalid="ignore", over="ignore"):
            k = search(np.asarray([d[s] for s in keys]).astype(np.float32))
        best[i], dist[i] = keys[k], d[keys[k]]
    return table, best, dist


def gap(values32):
    """Relative gap between the smallest and the second smallest of the fp32 values (NaN ignored): how far the search is
    from a tie.  inf when there is one value only."""
    v = np.sort(np.asarray(values32, dtype=np.float64)[~np.isnan(values32)])
    if len(v) < 2:
        return np.inf
    return (v[1] - v[0]) / v[0] if v[0] > 0 else (np.inf if v[1] > 0 else 0.0)


def dtw_ragged(a, b, len_a=None, len_b=None):
    """dtw_i (n,) fp64: sqrt of the minimal warping-path cost with squared-Euclidean point costs on the m_i x n_i table --
    calculate_dtw(seq1, seq2) of evaluate/metrics.py.  One pair at a time, walked by anti-diagonals like
    _eval_paired_ref.dtw: row i of a diagonal sits at index i + 1, index 0 stays +inf."""
    a, b = _f64(a), _f64(b)
    la, lb = lengths_of(a, len_a), lengths_of(b, len_b)
    out = np.zeros(a.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[0]):
            m, n = int(la[k]), int(lb[k])
            x, y = a[k, :m], b[k, :n]
            p1, p2 = np.full(m + 1, np.inf), np.full(m + 1, np.inf)
            for d in range(m + n - 1):
                i = np.arange(max(0, d - (n - 1)), min(d, m - 1) + 1)
                df = x[i] - y[d - i]
                c = (df * df).sum(axis=1)
                best = np.zeros(1) if d == 0 else np.minimum(p2[i], np.minimum(p1[i], p1[i + 1]))
                cur = np.full(m + 1, np.inf)
                cur[i + 1] = c + best
                p2, p1 = p1, cur
            out[k] = np.sqrt(p1[m])
    return out


# ------------------------------------------------------------------------------------------------ shared shift cases
# Every pair on which a test compares best_shift, on the CPU or on the GPU, comes from here, so that
# tests/test_eval_motion_host.py can hold ALL of them to the condition "the search is not decided by a rounding".
def planted(seed, n, La, Lb, S, shifts, noise=0.02):
    """a (n, La, S), b (n, Lb, S) fp32: a is a sum of three sines per series, series j of pair i scaled by 1 + 0.5 i +
    0.25 j, and b[t + k] = a[t] + noise for the pair's planted shift k (both continued past their ends by the same sines)."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.15, 0.9, (3, n, 1, S))
    ph = rs.uniform(0, 2 * np.pi, (3, n, 1, S))
    amp = np.array([0.5, 0.3, 0.2])[:, None, None, None]
    scale = 1.0 + 0.5 * np.arange(n)[:, None, None] + 0.25 * np.arange(S)[None, None, :]
    ta = np.broadcast_to(np.arange(La, dtype=np.float64)[None, :, None], (n, La, 1))
    tb = np.arange(Lb, dtype=np.float64)[None, :, None] - np.asarray(shifts, dtype=np.float64)[:, None, None]
    a = scale * (amp * np.sin(w * ta[None] + ph)).sum(axis=0)
    b = scale * (amp * np.sin(w * tb[None] + ph)).sum(axis=0) + noise * rs.randn(n, Lb, S)
    return a.astype(np.float32), b.astype(np.float32)


# name: (seed, n, La, Lb, S, planted shifts, len_a or None, len_b or None)
GPU_SHIFT_CASES = {
    "ragged_10ch": (71, 5, 130, 97, 10, (3, -17, 20, -2, 0), (130, 101, 64, 65, 2), (97, 97, 63, 33, 90)),
    "one_point": (72, 1, 1, 9, 7, (4,), None, None),
    "full_130_1ch": (73, 5, 130, 130, 1, (0, 1, -1, 30, -64), None, None),
    "one_block_plus_one": (74, 1, 33, 40, 7, (5,), None, None),
    "two_points": (75, 1, 2, 5, 3, (2,), None, None),
    "longer_b": (76, 5, 63, 65, 7, (0, 2, -5, 11, 1), (63, 1, 2, 33, 63), (65, 64, 65, 64, 2)),
}


def gpu_shift_case(name):
    """a, b, len_a, len_b of GPU_SHIFT_CASES[name]; the padding behind a pair's length is filled with NaN."""
    seed, n, La, Lb, S, shifts, la, lb = GPU_SHIFT_CASES[name]
    a, b = planted(seed, n, La, Lb, S, shifts)
    la = None if la is None else np.asarray(la, dtype=np.int32)
    lb = None if lb is None else np.asarray(lb, dtype=np.int32)
    for x, ln in ((a, la), (b, lb)):
        if ln is not None:
            for i in range(n):
                x[i, ln[i]:] = np.nan
    return a, b, la, lb


def tie_case():
    """Constant sequences 0.25 against 0.625 at S = 4: every point norm is sqrt(4 * 0.375^2) = 0.75 exactly, so every
    shift's distance is 0.75 exactly and the first shift, -M, wins.  (a (2, 9, 4), b (2, 7, 4), lengths (9, 5) / (7, 7))"""
    a, b = np.full((2, 9, 4), 0.25, np.float32), np.full((2, 7, 4), 0.625, np.float32)
    return a, b, np.asarray([9, 5], np.int32), np.asarray([7, 7], np.int32)


def nan_cases():
    """Pair 0: a NaN in the only point pair of the first shift (the last point of a, m <= n) -> (-M, NaN).  Pair 1: a NaN
    in the first point of a (m <= n: the first shift's pair is a[m - 1], b[0]) is in every overlap but those of the most
    negative shifts, and is never chosen.  From the planted case, so the finite values have a clear minimum."""
    a, b = planted(77, 2, 12, 15, 3, (0, -6))
    a[0, 11] = np.nan
    a[1, 0] = np.nan
    return a, b, None, None
