"""Evaluation metrics on the GPU, computed from the arrays infer.py writes exactly as the reference's
evaluation.py defines them: MSE / WAPE (:166-206), ED (:137-150), DTW (:152-163), MRR (:21-45) and CRPS (:51-83) over
the run_0..run_k repetitions `--run_multi` writes, the TS2Vec encoder forward + FID of the C-FID metric
(:127-135,238-243; evaluate/ts2vec.py:352-399), and the set-against-set measures MDD / ACD / SD / KD of
evaluate/feature_based_measures.py (calculate_mdd :30-94, _acd :98-161, _sd :165-191, _kd :195-223), and the motion measures
of evaluate/metrics.py for recordings of unequal length: correlational_score (:112-137), sequence_correlation (:219-266)
and dtw_ragged (calculate_dtw(seq1, seq2), :139-170) on the kernels of csrc/t2s_eval_motion.hip.  motion_runs scores the runs of a motion test split as the reference's myevaluation.py does (t2s_eval_runs, csrc/t2s_eval_runs.hip; driver myevaluation.py).  `python -m t2ms_amd.metrics <generation dir>` prints them for a
directory holding x_1.npy and x_t.npy ({save_path}/generation/{backbone}_{denoiser}_{dataset}_{cfg}_{steps}/[run_k/])
and the run_* sub-directories.

C-FID end to end: evaluation.py TRAINS the TS2Vec encoder at evaluation time (initialize_ts2vec, 200 contrastive
iterations from a random initialisation, :238); `t2ms_amd.ts2vec` restates that training (torch autograd plumbing, pinned
to the reference's loss curve) and `TS2VecEncoder` here runs the forward of the trained encoder on the HIP kernel, so the
CLI prints C-FID from the .npy files alone.  (Values are comparable only for the same trained encoder / seeds.)"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

import ctypes as C

from . import _lib as L
from ._handle import HandleOwner


def mse_wape(ori, gen, device="cuda"):
    """(MSE, WAPE, per_sample (N,2)) for (N, L, n_series) arrays (or tensors) of equal shape."""
    a = torch.as_tensor(np.asarray(ori) if not torch.is_tensor(ori) else ori).float()
    b = torch.as_tensor(np.asarray(gen) if not torch.is_tensor(gen) else gen).float()
    if a.shape != b.shape or a.dim() < 2:
        raise L.T2SError(f"mse_wape: shapes {tuple(a.shape)} vs {tuple(b.shape)}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.T2SError("mse_wape: the metrics kernels run on a GPU; there is no CPU fallback")
    n = a.shape[0]
    a = a.reshape(n, -1).contiguous().to(dev)
    b = b.reshape(n, -1).contiguous().to(dev)
    per = torch.empty(n, 2, device=dev)
    out = torch.empty(2, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_mse_wape(a.data_ptr(), b.data_ptr(), per.data_ptr(), out.data_ptr(), n, a.shape[1],
                                          L.stream_ptr(dev)), "t2s_eval_mse_wape")
    o = out.cpu()
    return float(o[0]), float(o[1]), per.cpu()


def mrr(ori, gens, threshold=0.5, device="cuda"):
    """(MRR, sims (N,G), score (N,)) for ori (N, L, n_series) and the G generated arrays `gens` (a sequence of
    arrays of ori's shape, run_0 first, or one (N, L, n_series, G) array as evaluation.py:311-313 stacks them)."""
    a = torch.as_tensor(np.asarray(ori) if not torch.is_tensor(ori) else ori).float()
    if torch.is_tensor(gens) or isinstance(gens, np.ndarray):
        g = torch.as_tensor(np.asarray(gens) if not torch.is_tensor(gens) else gens).float()
        if g.dim() != a.dim() + 1 or g.shape[:-1] != a.shape:
            raise L.T2SError(f"mrr: generations {tuple(g.shape)} vs original {tuple(a.shape)}")
        g = g.movedim(-1, 0)
    else:
        g = torch.stack([torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).float() for x in gens])
        if g.shape[1:] != a.shape:
            raise L.T2SError(f"mrr: generations {tuple(g.shape[1:])} vs original {tuple(a.shape)}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.T2SError("mrr: the metrics kernels run on a GPU; there is no CPU fallback")
    n, runs = a.shape[0], g.shape[0]
    a = a.reshape(n, -1).contiguous().to(dev)
    g = g.reshape(runs, n, -1).contiguous().to(dev)
    sims = torch.empty(n, runs, device=dev)
    score = torch.empty(n, device=dev)
    out = torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_mrr(a.data_ptr(), g.data_ptr(), sims.data_ptr(), score.data_ptr(), out.data_ptr(),
                                     n, a.shape[1], runs, float(threshold), L.stream_ptr(dev)), "t2s_eval_mrr")
    return float(out.cpu()[0]), sims.cpu(), score.cpu()


def _pair(ori, gen, what):
    a = torch.as_tensor(np.asarray(ori) if not torch.is_tensor(ori) else ori).float()
    b = torch.as_tensor(np.asarray(gen) if not torch.is_tensor(gen) else gen).float()
    if a.shape != b.shape or a.dim() != 3:
        raise L.T2SError(f"{what}: expected two (N, L, n_series) arrays, got {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b


def _gpu(device, what):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.T2SError(f"{what}: the metrics kernels run on a GPU; there is no CPU fallback")
    return dev


def ed(ori, gen, device="cuda"):
    """(ED, per_sample (N,)): calculate_ed, evaluation.py:137-150."""
    a, b = _pair(ori, gen, "ed")
    dev = _gpu(device, "ed")
    a, b = a.contiguous().to(dev), b.contiguous().to(dev)
    per, out = torch.empty(a.shape[0], device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_ed(a.data_ptr(), b.data_ptr(), per.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1],
                                    a.shape[2], L.stream_ptr(dev)), "t2s_eval_ed")
    return float(out.cpu()[0]), per.cpu()


def dtw(ori, gen, device="cuda"):
    """(DTW, per_sample (N,)): calculate_dtw, evaluation.py:152-163 (dtaidistance dtw_ndim.distance)."""
    a, b = _pair(ori, gen, "dtw")
    dev = _gpu(device, "dtw")
    a, b = a.contiguous().to(dev), b.contiguous().to(dev)
    per, out = torch.empty(a.shape[0], device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_dtw(a.data_ptr(), b.data_ptr(), per.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1],
                                     a.shape[2], L.stream_ptr(dev)), "t2s_eval_dtw")
    return float(out.cpu()[0]), per.cpu()


class _Features:
    """Both sets on the device plus the workspace t2s_eval_moments / t2s_eval_mdd share: one upload serves all four."""

    def __init__(self, ori, gen, device, what):
        a, b = _pair(ori, gen, what)
        self.dev = _gpu(device, what)
        self.a, self.b = a.contiguous().to(self.dev), b.contiguous().to(self.dev)
        self.shape = tuple(int(v) for v in a.shape)
        need = L.lib().t2s_eval_features_workspace_bytes(*self.shape)
        if need == 0:
            L.check(1, "t2s_eval_features_workspace_bytes")
        self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def moments(self):
        """((ACD, SD, KD), stats): stats holds, per set (0 = ori, 1 = gen) and channel, `mean`, `var` (population),
        `skew`, `kurt` (excess), each (2, n_series), and `acf` (2, n_series, K), K = min(64, L)."""
        n, length, s = self.shape
        k = min(L.EVAL_MAX_LAG, length)
        stats, out = torch.empty(2, s, 4 + k, device=self.dev), torch.empty(3, device=self.dev)
        with torch.cuda.device(self.dev):
            L.check(L.lib().t2s_eval_moments(self.a.data_ptr(), self.b.data_ptr(), stats.data_ptr(), out.data_ptr(), n, length, s,
                                             self.ws.data_ptr(), self.ws.numel(), L.stream_ptr(self.dev)), "t2s_eval_moments")
        st = stats.cpu()
        return tuple(float(v) for v in out.cpu()), {"mean": st[:, :, 0], "var": st[:, :, 1], "skew": st[:, :, 2],
                                                    "kurt": st[:, :, 3], "acf": st[:, :, 4:]}

    def mdd(self):
        """(MDD, per_column (L, n_series))."""
        n, length, s = self.shape
        per, out = torch.empty(length, s, device=self.dev), torch.empty(1, device=self.dev)
        with torch.cuda.device(self.dev):
            L.check(L.lib().t2s_eval_mdd(self.a.data_ptr(), self.b.data_ptr(), per.data_ptr(), out.data_ptr(), n, length, s,
                                         self.ws.data_ptr(), self.ws.numel(), L.stream_ptr(self.dev)), "t2s_eval_mdd")
        return float(out.cpu()[0]), per.cpu()


def mdd(ori, gen, device="cuda"):
    """(MDD, per_column (L, n_series)): calculate_mdd, evaluate/feature_based_measures.py:30-94 -- per time step and
    channel the mean absolute difference of the two sets' 50-bin densities on the real set's range."""
    return _Features(ori, gen, device, "mdd").mdd()


def acd(ori, gen, device="cuda"):
    """(ACD, stats): calculate_acd, feature_based_measures.py:98-161 -- the distance of the two sets' autocorrelation
    functions over min(64, L) lags; stats as _Features.moments returns them."""
    (v, _, _), stats = _Features(ori, gen, device, "acd").moments()
    return v, stats


def sd(ori, gen, device="cuda"):
    """(SD, stats): calculate_sd, feature_based_measures.py:165-191 -- the difference of the two sets' skewness."""
    (_, v, _), stats = _Features(ori, gen, device, "sd").moments()
    return v, stats


def kd(ori, gen, device="cuda"):
    """(KD, stats): calculate_kd, feature_based_measures.py:195-223 -- the difference of the two sets' excess kurtosis."""
    (_, _, v), stats = _Features(ori, gen, device, "kd").moments()
    return v, stats


def feature_measures(ori, gen, device="cuda"):
    """({"MDD", "ACD", "SD", "KD"}, {"per_column", "stats"}) from one upload and one statistics pass."""
    f = _Features(ori, gen, device, "feature_measures")
    (a, s, k), stats = f.moments()
    m, per = f.mdd()
    return {"MDD": m, "ACD": a, "SD": s, "KD": k}, {"per_column": per, "stats": stats}


def _f32(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).float()


def correlational_score(ori, gen, device="cuda"):
    """(score, corr (2, S, S)): calculate_correlational_score, evaluate/metrics.py:112-137 -- 1 - sum |C_ori - C_gen| /
    sum |C_ori| of the two sets' channel correlation matrices (np.corrcoef over all rows; corr[0] = ori, corr[1] = gen).
    Takes (N, L, S) arrays, flattened to (N * L, S) as the reference does, or (rows, S) arrays; the two sets may differ
    in their number of rows.  A constant channel makes the score NaN; with S = 1 it is 1 whenever it is defined."""
    a, b = _f32(ori), _f32(gen)
    if a.dim() not in (2, 3) or b.dim() not in (2, 3):
        raise L.T2SError(f"correlational_score: expected (N, L, S) or (rows, S) arrays, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[-1] != b.shape[-1]:
        raise L.T2SError(f"correlational_score: channel counts differ, {a.shape[-1]} and {b.shape[-1]}")
    s = int(a.shape[-1])
    if not 1 <= s <= L.EVAL_CORR_MAX_SERIES:
        raise L.T2SError(f"correlational_score: S={s} is outside [1, {L.EVAL_CORR_MAX_SERIES}]")
    a, b = a.reshape(-1, s), b.reshape(-1, s)
    if a.shape[0] < 2 or b.shape[0] < 2:
        raise L.T2SError(f"correlational_score: {a.shape[0]} and {b.shape[0]} rows, a correlation needs at least 2")
    dev = _gpu(device, "correlational_score")
    a, b = a.contiguous().to(dev), b.contiguous().to(dev)
    need = L.lib().t2s_eval_corr_workspace_bytes(a.shape[0], b.shape[0], s)
    if need == 0:
        L.check(1, "t2s_eval_corr_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    corr, out = torch.empty(2, s, s, device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_corr(a.data_ptr(), b.data_ptr(), corr.data_ptr(), out.data_ptr(), a.shape[0], b.shape[0], s,
                                      ws.data_ptr(), ws.numel(), L.stream_ptr(dev)), "t2s_eval_corr")
    return float(out.cpu()[0]), corr.cpu()


def pad_ragged(seqs):
    """[(T_i, S) arrays] -> (array (n, Lmax, S) fp32 zero-padded, lengths (n,) int32)."""
    seqs = [np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.float32) for s in seqs]
    if not seqs:
        raise L.T2SError("pad_ragged: no sequence")
    seqs = [s[:, None] if s.ndim == 1 else s for s in seqs]
    if any(s.ndim != 2 or s.shape[0] < 1 for s in seqs) or len({s.shape[1] for s in seqs}) != 1:
        raise L.T2SError(f"pad_ragged: expected non-empty (T_i, S) arrays of one S, got {[tuple(s.shape) for s in seqs]}")
    out = np.zeros((len(seqs), max(s.shape[0] for s in seqs), seqs[0].shape[1]), np.float32)
    for i, s in enumerate(seqs):
        out[i, :s.shape[0]] = s
    return out, np.asarray([s.shape[0] for s in seqs], dtype=np.int32)


def _ragged(a, b, lengths, what):
    """Host side of the two ragged measures: a (n, La, S), b (n, Lb, S) (or two lists of (T_i, S) arrays) and `lengths`
    = None or (len_a, len_b), each None or n integers -> fp32 tensors and int32 length tensors (None = full length).
    Everything the kernels would clamp is refused here."""
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        if not (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))) or lengths is not None:
            raise L.T2SError(f"{what}: give two lists of (T_i, S) arrays (and no lengths), or two padded arrays")
        (a, la), (b, lb) = pad_ragged(a), pad_ragged(b)
        lengths = (la, lb)
    a, b = _f32(a), _f32(b)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[0] < 1:
        raise L.T2SError(f"{what}: expected (n, La, S) and (n, Lb, S) arrays, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[2] != b.shape[2] or a.shape[2] < 1:
        raise L.T2SError(f"{what}: channel counts differ, {a.shape[2]} and {b.shape[2]}")
    lens = []
    for x, ln, name in ((a, None if lengths is None else lengths[0], "a"), (b, None if lengths is None else lengths[1], "b")):
        cap = int(x.shape[1])
        if not 1 <= cap <= L.EVAL_MOTION_MAX_LEN:
            raise L.T2SError(f"{what}: L={cap} of {name} is outside [1, {L.EVAL_MOTION_MAX_LEN}]")
        if ln is not None:
            ln = np.asarray(ln.cpu() if torch.is_tensor(ln) else ln)
            if ln.shape != (a.shape[0],) or not np.issubdtype(ln.dtype, np.integer):
                raise L.T2SError(f"{what}: lengths of {name} must be {a.shape[0]} integers")
            if ln.min() < 1 or ln.max() > cap:
                raise L.T2SError(f"{what}: a length of {name} is outside [1, {cap}]: min {ln.min()}, max {ln.max()}")
            ln = torch.from_numpy(ln.astype(np.int32))
        lens.append(ln)
    return a, b, lens[0], lens[1]


def sequence_correlation(a, b, lengths=None, device="cuda"):
    """(mean_min_dist, best_shift (n,) int32, min_dist (n,), table (n, W)): sequence_correlation, evaluate/metrics.py:219-266,
    for every pair (a_i, b_i) -- the mean point distance at every shift -M .. M, M = min(len_a, len_b) - 1 (table, W = 2
    min(La, Lb) - 1, shift 0 in column min(La, Lb) - 1, NaN where the pair has no such shift), and the reference's
    left-to-right search for the smallest.  a (n, La, S), b (n, Lb, S) with lengths = (len_a, len_b) (each None or n
    integers), or two lists of (T_i, S) arrays."""
    a, b, la, lb = _ragged(a, b, lengths, "sequence_correlation")
    dev = _gpu(device, "sequence_correlation")
    a, b = a.contiguous().to(dev), b.contiguous().to(dev)
    la, lb = (None if v is None else v.to(dev) for v in (la, lb))
    n, w = a.shape[0], 2 * min(a.shape[1], b.shape[1]) - 1
    table, best = torch.empty(n, w, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    dist, out = torch.empty(n, device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_shift(a.data_ptr(), b.data_ptr(), None if la is None else la.data_ptr(),
                                       None if lb is None else lb.data_ptr(), table.data_ptr(), best.data_ptr(), dist.data_ptr(),
                                       out.data_ptr(), n, a.shape[1], b.shape[1], a.shape[2], L.stream_ptr(dev)), "t2s_eval_shift")
    return float(out.cpu()[0]), best.cpu(), dist.cpu(), table.cpu()


def dtw_ragged(a, b, lengths=None, device="cuda"):
    """(mean, per_sample (n,)): calculate_dtw(seq1, seq2), evaluate/metrics.py:139-170 (squared-Euclidean point costs, then
    a sqrt), for every pair of sequences of unequal length; arguments as for sequence_correlation."""
    a, b, la, lb = _ragged(a, b, lengths, "dtw_ragged")
    dev = _gpu(device, "dtw_ragged")
    a, b = a.contiguous().to(dev), b.contiguous().to(dev)
    la, lb = (None if v is None else v.to(dev) for v in (la, lb))
    per, out = torch.empty(a.shape[0], device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_dtw_ragged(a.data_ptr(), b.data_ptr(), None if la is None else la.data_ptr(),
                                            None if lb is None else lb.data_ptr(), per.data_ptr(), out.data_ptr(), a.shape[0],
                                            a.shape[1], b.shape[1], a.shape[2], L.stream_ptr(dev)), "t2s_eval_dtw_ragged")
    return float(out.cpu()[0]), per.cpu()


def pack_motion_runs(x1_list, xt_runs):
    """Host side of motion_runs: x1_list = K arrays (C, T_i), xt_runs = R lists of K arrays of the same shapes -> (x1 packed
    fp32 (C * sum T_i,), xt packed (R, C * sum T_i), lengths int32 (K,), offsets uint64 (K + 1,), C).  Everything t2s_eval_runs
    would refuse or skip is a T2SError here."""
    what = "motion_runs"

    def arr(v):
        return np.ascontiguousarray(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32))

    x1 = [arr(v) for v in x1_list]
    if not x1:
        raise L.T2SError(f"{what}: no clip")
    if any(v.ndim != 2 for v in x1):
        raise L.T2SError(f"{what}: every recording must be (C, T_i), got {[tuple(v.shape) for v in x1]}")
    chans = int(x1[0].shape[0])
    if not 1 <= chans <= L.EVAL_RUNS_MAX_CHANNELS:
        raise L.T2SError(f"{what}: C={chans} is outside [1, {L.EVAL_RUNS_MAX_CHANNELS}]")
    for i, v in enumerate(x1):
        if v.shape[0] != chans:
            raise L.T2SError(f"{what}: clip {i} has {v.shape[0]} channels, clip 0 has {chans}")
        if not 1 <= v.shape[1] <= L.EVAL_MOTION_MAX_LEN:
            raise L.T2SError(f"{what}: clip {i} has T={v.shape[1]}, outside [1, {L.EVAL_MOTION_MAX_LEN}]")
    runs = [[arr(v) for v in run] for run in xt_runs]
    if not runs:
        raise L.T2SError(f"{what}: no run")
    for r, run in enumerate(runs):
        if len(run) != len(x1):
            raise L.T2SError(f"{what}: run {r} holds {len(run)} clips, there are {len(x1)} recordings")
        for i, v in enumerate(run):
            if v.shape != x1[i].shape:
                raise L.T2SError(f"{what}: run {r} clip {i} is {tuple(v.shape)}, its recording is {tuple(x1[i].shape)}")
    lens = np.asarray([v.shape[1] for v in x1], dtype=np.int32)
    off = np.zeros(len(x1) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64))
    p1 = np.concatenate([v.reshape(-1) for v in x1])
    pt = np.stack([np.concatenate([v.reshape(-1) for v in run]) for run in runs])
    return p1, pt, lens, off, chans


def motion_runs(x1_list, xt_runs, device="cuda", detail=False):
    """The reference's myevaluation.py for every clip of a motion test split in ONE t2s_eval_runs call: x1_list = K recordings
    (C, T_i), xt_runs = R runs of K samples of the same shapes.  Per clip and run, on the min-max normalised channels
    (a = the sample, b = the recording; the reference hands the samples over as `ori` and reads the channel axis as time):
    MSE, WAPE (sum |a - b| / sum |a|, NaN when that is 0), ED (mean over t of the norm over channels) and DTW (between the C
    points a[i, :] and b[j, :]).  -> ({"MSE", "WAPE", "ED", "DTW"} the mean over clips, per_clip (K, 4) the reference's
    reductions over runs (mean, nanmean, mean, mean), per_run (K, R, 4)); detail=True adds (norm1, normt): the normalised
    planes, K arrays (C, T_i) and K arrays (R, C, T_i), views of two device tensors.  One upload, three launches, one sync."""
    p1, pt, lens, off, chans = pack_motion_runs(x1_list, xt_runs)
    dev = _gpu(device, "motion_runs")
    K, R = len(lens), pt.shape[0]
    with torch.cuda.device(dev):
        x1 = torch.from_numpy(p1).to(dev)
        xt = torch.from_numpy(pt).to(dev)
        keep, p_len, p_off, _ = L.ragged_device_tables(lens, off, off, dev)
        norm1, normt = torch.empty_like(x1), torch.empty_like(xt)
        res = torch.empty(K * R * 4 + K * 4 + 4, device=dev)          # per_run, per_clip, out: one download
        base = res.data_ptr()
        L.check(L.lib().t2s_eval_runs(x1.data_ptr(), xt.data_ptr(), p_len, p_off, base, base + 16 * K * R, base + 16 * K * (R + 1),
                                      norm1.data_ptr(), normt.data_ptr(), K, R, chans, int(lens.max()), L.stream_ptr(dev)),
                "t2s_eval_runs")
        host = res.cpu()
    del keep
    per_run, per_clip, out = host[:K * R * 4].reshape(K, R, 4), host[K * R * 4:K * (R + 1) * 4].reshape(K, 4), host[K * (R + 1) * 4:]
    summary = {name: float(out[m]) for m, name in enumerate(("MSE", "WAPE", "ED", "DTW"))}
    if not detail:
        return summary, per_clip, per_run
    o = [chans * int(v) for v in off]
    n1 = [norm1[o[i]:o[i + 1]].view(chans, int(lens[i])) for i in range(K)]
    nt = [normt[:, o[i]:o[i + 1]].reshape(R, chans, int(lens[i])) for i in range(K)]
    return summary, per_clip, per_run, n1, nt


def _runs_first(ori, gens, what):
    a = torch.as_tensor(np.asarray(ori) if not torch.is_tensor(ori) else ori).float()
    if torch.is_tensor(gens) or isinstance(gens, np.ndarray):
        g = torch.as_tensor(np.asarray(gens) if not torch.is_tensor(gens) else gens).float()
        if g.dim() != a.dim() + 1 or g.shape[:-1] != a.shape:
            raise L.T2SError(f"{what}: generations {tuple(g.shape)} vs original {tuple(a.shape)}")
        g = g.movedim(-1, 0)
    else:
        g = torch.stack([torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).float() for x in gens])
        if g.shape[1:] != a.shape:
            raise L.T2SError(f"{what}: generations {tuple(g.shape[1:])} vs original {tuple(a.shape)}")
    return a, g


def crps(ori, gens, device="cuda"):
    """(CRPS, per_sample (N,)): calculate_crps, evaluation.py:51-83; ori (N, L, n_series), `gens` the G generated arrays
    (a sequence, run_0 first, or one (N, L, n_series, G) array as evaluation.py:311-313 stacks them)."""
    a, g = _runs_first(ori, gens, "crps")
    if a.dim() != 3:
        raise L.T2SError(f"crps: ori must be (N, L, n_series), got {tuple(a.shape)}")
    dev = _gpu(device, "crps")
    a, g = a.contiguous().to(dev), g.contiguous().to(dev)
    per, out = torch.empty(a.shape[0], device=dev), torch.empty(1, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_eval_crps(a.data_ptr(), g.data_ptr(), per.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1],
                                      a.shape[2], g.shape[0], L.stream_ptr(dev)), "t2s_eval_crps")
    return float(out.cpu()[0]), per.cpu()


ENCODE_LDS_BYTES = 160 * 1024            # t2s_ts2vec_encode: three (cmax, T) fp32 planes in the LDS of one CU
ENCODE_WORKSPACE_CAP = 256 << 20         # bytes of workspace one t2s_ts2vec_encode_long call of the mirror may ask for


def _encode_path(T, cmax, path=None):
    """'lds' (t2s_ts2vec_encode, the planes in LDS) or 'gemm' (t2s_ts2vec_encode_long, the planes in a workspace) for a
    series of T steps through an encoder whose widest layer has cmax channels.  path=None keeps the LDS kernel wherever
    it fits (the same bits as before the long entry existed); 'lds' / 'gemm' force one -- 'lds' beyond its bound is
    refused by the entry itself."""
    if path not in (None, "lds", "gemm"):
        raise L.T2SError(f"TS2VecEncoder.encode: path must be None, 'lds' or 'gemm', got {path!r}")
    if path is not None:
        return path
    return "lds" if 3 * cmax * T * 4 <= ENCODE_LDS_BYTES else "gemm"


def _encode_workspace_bytes(rows, T, hidden, output_dims, depth):
    """What t2s_ts2vec_encode_workspace_bytes returns for a supported shape (csrc/t2s_ts2vec_encode.hip, enc_plan): the
    packed weights (per convolution: M tiles of 32 rows, rounded up to the group of <= 4 a wave runs, x K / 2 steps of 64
    floats) and three (rows, cmax rounded up to 32, T) fp32 planes, each part rounded up to 256 bytes."""
    def up(v, m):
        return (v + m - 1) // m * m

    def conv(ci, co, kp=0):
        tiles = (co + 31) // 32
        return up(tiles, min(tiles, 4)) * ((3 * up(ci, 2) + kp) // 2) * 64

    packed = 2 * depth * conv(hidden, hidden) + conv(hidden, output_dims) + conv(output_dims, output_dims, up(hidden, 2))
    plane = rows * up(max(hidden, output_dims), 32) * T
    return up(4 * packed, 256) + 3 * up(4 * plane, 256)


def _encode_chunks(B, T, hidden, output_dims, depth, cap=None):
    """[(row0, rows), ...] covering rows 0 .. B-1 once, in order: chunks of the most rows whose workspace stays <= cap
    (ENCODE_WORKSPACE_CAP), and of one row each if even a single row exceeds it."""
    cap = ENCODE_WORKSPACE_CAP if cap is None else cap

    def bytes_of_rows(rows):
        return _encode_workspace_bytes(rows, T, hidden, output_dims, depth)

    if B < 1:
        return []
    rows = 1
    if bytes_of_rows(B) <= cap:
        rows = B
    else:
        lo, hi = 1, B                    # bytes_of_rows(lo) <= cap or lo == 1; bytes_of_rows(hi) > cap
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if bytes_of_rows(mid) <= cap:
                lo = mid
            else:
                hi = mid
        rows = lo
    return [(r0, min(rows, B - r0)) for r0 in range(0, B, rows)]


class TS2VecEncoder(HandleOwner):
    """Forward of evaluate/ts2vec.py's TSEncoder (:352-399, eval mode, mask 'all_true') on the GPU from its state dict
    (keys input_fc.*, feature_extractor.net.<i>.conv{1,2}.conv.*, feature_extractor.net.<depth>.projector.*).  Series
    whose three activation planes fit the LDS of a CU run on t2s_ts2vec_encode, longer ones (up to 4096 steps) on
    t2s_ts2vec_encode_long with a workspace this object owns (HandleOwner._workspace)."""

    def __init__(self, state_dict, device="cuda"):
        self.device = _gpu(device, "TS2VecEncoder")
        sd = {k: torch.as_tensor(v).float().contiguous().to(self.device) for k, v in state_dict.items()}
        depth = 0
        while f"feature_extractor.net.{depth + 1}.conv1.conv.weight" in sd:
            depth += 1
        w = L.Ts2vecWeights()
        w.hidden, w.input_dims = sd["input_fc.weight"].shape
        w.depth = depth
        w.output_dims = sd[f"feature_extractor.net.{depth}.conv1.conv.weight"].shape[0]
        if depth >= L.TS2VEC_MAX_BLOCKS:
            raise L.T2SError(f"TS2VecEncoder: depth {depth} exceeds {L.TS2VEC_MAX_BLOCKS - 1}")
        w.fc_w, w.fc_b = sd["input_fc.weight"].data_ptr(), sd["input_fc.bias"].data_ptr()
        for i in range(depth + 1):
            p = f"feature_extractor.net.{i}."
            if f"{p}projector.weight" in sd and i != depth:
                raise L.T2SError("TS2VecEncoder: a projector inside the stack (unequal hidden widths) is not supported")
            w.conv1_w[i], w.conv1_b[i] = sd[p + "conv1.conv.weight"].data_ptr(), sd[p + "conv1.conv.bias"].data_ptr()
            w.conv2_w[i], w.conv2_b[i] = sd[p + "conv2.conv.weight"].data_ptr(), sd[p + "conv2.conv.bias"].data_ptr()
        p = f"feature_extractor.net.{depth}.projector."
        w.proj_w, w.proj_b = sd[p + "weight"].data_ptr(), sd[p + "bias"].data_ptr()
        self._w, self._keep = w, sd

    def _workspace_bytes(self, rows, T):
        need = L.lib().t2s_ts2vec_encode_workspace_bytes(C.byref(self._w), rows, T)
        if need == 0:
            L.check(1, "t2s_ts2vec_encode_workspace_bytes")
        return need

    def encode(self, x, encoding_window="full_series", path=None):
        """x (B, T, input_dims) -> (B, output_dims) for 'full_series' (TS2Vec.encode, ts2vec.py:236-245), or the
        per-step representations (B, T, output_dims) for encoding_window=None.  `path`: see _encode_path; on the 'gemm'
        path the batch is cut into chunks whose workspace stays under ENCODE_WORKSPACE_CAP (rows are independent, so the
        cut changes no bit)."""
        if encoding_window not in ("full_series", None):
            raise L.T2SError("TS2VecEncoder.encode: encoding_window must be 'full_series' or None")
        xs = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).float().contiguous().to(self.device)
        if xs.dim() != 3 or xs.shape[2] != self._w.input_dims:
            raise L.T2SError(f"TS2VecEncoder.encode: x must be (B, T, {self._w.input_dims}), got {tuple(xs.shape)}")
        B, T = xs.shape[0], xs.shape[1]
        cin, cout = self._w.input_dims, self._w.output_dims
        which = _encode_path(T, max(self._w.hidden, cout), path)
        full = torch.empty(B, cout, device=self.device)
        rep = torch.empty(B, T, cout, device=self.device) if encoding_window is None else None
        if which == "lds":
            with torch.cuda.device(self.device):
                L.check(L.lib().t2s_ts2vec_encode(C.byref(self._w), xs.data_ptr(), None if rep is None else rep.data_ptr(),
                                                  full.data_ptr(), B, T, L.stream_ptr(self.device)), "t2s_ts2vec_encode")
            return full if rep is None else rep
        self._workspace_bytes(B, T)      # an unsupported shape raises here, with the entry's message
        chunks = _encode_chunks(B, T, self._w.hidden, cout, self._w.depth)
        need = max(self._workspace_bytes(rows, T) for _, rows in chunks)
        with torch.cuda.device(self.device):
            ws = self._workspace(need, self.device)          # the long path's, grown on demand
            for r0, rows in chunks:
                L.check(L.lib().t2s_ts2vec_encode_long(
                    C.byref(self._w), xs.data_ptr() + 4 * r0 * T * cin,
                    None if rep is None else rep.data_ptr() + 4 * r0 * T * cout, full.data_ptr() + 4 * r0 * cout,
                    rows, T, ws.data_ptr(), ws.numel(), L.stream_ptr(self.device)), "t2s_ts2vec_encode_long")
        return full if rep is None else rep


def fid(act1, act2):
    """calculate_fid (evaluation.py:127-135) on two (N, C) activation arrays: host fp64 (a C x C matrix square root)."""
    from scipy.linalg import sqrtm
    a1 = np.asarray(act1.cpu() if torch.is_tensor(act1) else act1, dtype=np.float64)
    a2 = np.asarray(act2.cpu() if torch.is_tensor(act2) else act2, dtype=np.float64)
    mu1, s1 = a1.mean(axis=0), np.cov(a1, rowvar=False)
    mu2, s2 = a2.mean(axis=0), np.cov(a2, rowvar=False)
    covmean = sqrtm(s1.dot(s2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(np.sum((mu1 - mu2) ** 2.0) + np.trace(s1 + s2 - 2.0 * covmean))


def cfid(ori, gen, encoder: "TS2VecEncoder"):
    """C-FID as evaluation.py:238-243 computes it once the encoder exists: FID of the full-series representations of the
    original and the generated (N, L, n_series) arrays, L <= 4096 (TS2VecEncoder.encode picks the kernel by L)."""
    return fid(encoder.encode(ori), encoder.encode(gen))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        sys.exit("usage: python -m t2ms_amd.metrics <directory holding x_1.npy and x_t.npy and / or run_*/>")
    d = argv[0]
    if os.path.exists(os.path.join(d, "x_t.npy")):
        x1 = os.path.join(d, "x_1.npy")
        ori = np.load(x1 if os.path.exists(x1) else os.path.join(d, "run_0", "x_1.npy"))   # evaluation.py:285-286
        gen = np.load(os.path.join(d, "x_t.npy"))
        mse, wape, _ = mse_wape(ori, gen)
        print(f"samples {ori.shape[0]}  MSE {mse:.6f}  WAPE {wape:.6f}  ED {ed(ori, gen)[0]:.6f}  DTW {dtw(ori, gen)[0]:.6f}")
        o3 = ori if ori.ndim == 3 else ori[:, :, None]
        if o3.shape[0] >= 2 and o3.shape[1] <= 4096:
            fm, _ = feature_measures(o3, gen if gen.ndim == 3 else gen[:, :, None])
            print(f"samples {ori.shape[0]}  MDD {fm['MDD']:.6f}  ACD {fm['ACD']:.6f}  SD {fm['SD']:.6f}  KD {fm['KD']:.6f}")
        if ori.shape[0] >= 8 and os.environ.get("T2S_METRICS_CFID", "1") not in ("", "0"):
            # evaluation.py:238-243: train TS2Vec on the original series (200 contrastive iterations), encode both sets
            # with it, FID of the representations.  The encoder is trained per call from a random initialisation, as in
            # the reference, so the value varies from run to run unless torch / numpy are seeded by the caller.
            from .ts2vec import initialize_ts2vec
            o3 = ori if ori.ndim == 3 else ori[:, :, None]
            g3 = gen if gen.ndim == 3 else gen[:, :, None]
            model = initialize_ts2vec(o3.astype(np.float32), device="cuda")
            print(f"samples {ori.shape[0]}  C-FID {fid(model.encode(o3, encoding_window='full_series'), model.encode(g3, encoding_window='full_series')):.6f}"
                  f"  (TS2Vec trained {model.n_iters} iterations on the original series, engine {model.engine}: T2S_TS2VEC_FIT)")
    runs = sorted((r for r in os.listdir(d) if r.startswith("run_") and r[4:].isdigit()), key=lambda r: int(r[4:]))
    if runs:
        ori = np.load(os.path.join(d, runs[-1], "x_1.npy"))                                  # evaluation.py:304-314
        gens = [np.load(os.path.join(d, r, "x_t.npy")) for r in runs]
        m, _, _ = mrr(ori, gens)
        print(f"samples {ori.shape[0]}  runs {len(runs)}  MRR {m:.6f}  CRPS {crps(ori, gens)[0]:.6f}")


if __name__ == "__main__":
    main()
