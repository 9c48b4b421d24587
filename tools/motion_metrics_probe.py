"""Wall time of the motion measures: t2s_eval_shift, t2s_eval_dtw_ragged and t2s_eval_corr on the GPU
against the same formulas in vectorised fp64 numpy on the CPU of the same box.

    python tools/motion_metrics_probe.py [--rounds 5] [--calls 10] [--threads 16] [--out profiles/motion_metrics.json]

Shapes a user would run: 512 pairs with lengths drawn from 36 .. 192 (the fork's training lengths) at 10 channels, 64 pairs
with lengths 512 .. 1024 at 7 channels (shift and DTW each), and the score of two 2,048 x 144 x 10 sets.  GPU: the arrays
are already on the device; one round is `--calls` back-to-back calls of an entry followed by a device synchronise, host
clock, divided by the calls.  CPU: numpy with `--threads` threads, NOT the reference's code (a Python loop over shifts
resp. table cells): per pair the point distances of all (t, t') at once and every shift's sum by one bincount over t' - t;
DTW by anti-diagonals; np.corrcoef.  A warm-up round, then `--rounds` rounds in which the two sides alternate; reported
are medians and spreads (max - min), and the values of both sides.  The times are recorded, not gated: the parent commit
cannot compute these measures on the GPU at all.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def pairs(seed, n, lo, hi, s):
    import numpy as np
    rs = np.random.RandomState(seed)
    la, lb = rs.randint(lo, hi + 1, n).astype(np.int32), rs.randint(lo, hi + 1, n).astype(np.int32)
    t = np.arange(hi, dtype=np.float64)[None, :, None]
    w, ph = rs.uniform(0.02, 0.4, (n, 1, s)), rs.uniform(0, 6.28, (n, 1, s))
    a = 0.5 + 0.4 * np.sin(w * t + ph)
    b = 0.5 + 0.4 * np.sin(w * (t - rs.randint(-20, 21, n)[:, None, None]) + ph) + 0.02 * rs.randn(n, hi, s)
    return a.astype(np.float32), b.astype(np.float32), la, lb


def numpy_shift(a, b, la, lb):
    """best shift and minimal mean distance per pair, fp64, the search on fp32-rounded values as the entry does."""
    import numpy as np
    best, dist = np.zeros(len(la), np.int64), np.zeros(len(la))
    for i in range(len(la)):
        m, n = int(la[i]), int(lb[i])
        x, y = a[i, :m].astype(np.float64), b[i, :n].astype(np.float64)
        d = np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2))                 # (m, n)
        off = np.arange(n)[None, :] - np.arange(m)[:, None] + (m - 1)                    # shift + m - 1
        sums = np.bincount(off.ravel(), weights=d.ravel(), minlength=m + n - 1)
        cnt = np.bincount(off.ravel(), minlength=m + n - 1)
        M = min(m, n) - 1
        v = (sums / cnt)[m - 1 - M:m + M]
        k = int(np.argmin(v.astype(np.float32)))
        best[i], dist[i] = k - M, v[k]
    return best, dist


def numpy_dtw(a, b, la, lb):
    import numpy as np
    out = np.zeros(len(la))
    for k in range(len(la)):
        m, n = int(la[k]), int(lb[k])
        x, y = a[k, :m].astype(np.float64), b[k, :n].astype(np.float64)
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


def numpy_score(ori, gen):
    import numpy as np
    co = np.corrcoef(ori.reshape(-1, ori.shape[-1]).astype(np.float64), rowvar=False)
    cg = np.corrcoef(gen.reshape(-1, gen.shape[-1]).astype(np.float64), rowvar=False)
    return float(1 - np.abs(co - cg).sum() / np.abs(co).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_metrics.json"))
    a = ap.parse_args()
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        os.environ[var] = str(a.threads)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("motion_metrics_probe: needs a GPU (a CPU timing says nothing about the kernels)")
    from t2ms_amd import _lib as L
    from t2ms_amd import metrics as M
    torch.set_num_threads(a.threads)
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream_ptr(dev)
    result = {"device": torch.cuda.get_device_name(0), "cpu_threads": a.threads, "rounds": a.rounds, "calls_per_round": a.calls, "cells": []}

    def med(xs):
        return {"median_ms": round(1e3 * statistics.median(xs), 4), "spread_ms": round(1e3 * (max(xs) - min(xs)), 4)}

    def timed_gpu(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.calls

    def timed_cpu(fn):
        t0 = time.perf_counter()
        v = fn()
        return time.perf_counter() - t0, v

    def run(row, gpu_calls, cpu_calls):
        """gpu_calls / cpu_calls: {name: callable}; alternating rounds, round 0 is the warm-up."""
        times = {k: [] for k in list(gpu_calls) + list(cpu_calls)}
        for r in range(a.rounds + 1):
            for side in (("gpu", "cpu") if r % 2 == 0 else ("cpu", "gpu")):
                for k, fn in (gpu_calls if side == "gpu" else cpu_calls).items():
                    t = timed_gpu(fn) if side == "gpu" else timed_cpu(fn)[0]
                    if r:
                        times[k].append(t)
        row.update({k: med(v) for k, v in times.items()})
        result["cells"].append(row)
        print(json.dumps(row), flush=True)
        json.dump(result, open(a.out, "w"), indent=1)

    for n, lo, hi, s in ((512, 36, 192, 10), (64, 512, 1024, 7)):
        x, y, la, lb = pairs(n + s, n, lo, hi, s)
        dx, dy = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        dla, dlb = torch.from_numpy(la).to(dev), torch.from_numpy(lb).to(dev)
        table, best = torch.empty(n, 2 * hi - 1, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        dist, per, out = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(1, device=dev)

        def shift():
            L.check(lib.t2s_eval_shift(dx.data_ptr(), dy.data_ptr(), dla.data_ptr(), dlb.data_ptr(), table.data_ptr(), best.data_ptr(),
                                       dist.data_ptr(), out.data_ptr(), n, hi, hi, s, st), "t2s_eval_shift")

        def dtw():
            L.check(lib.t2s_eval_dtw_ragged(dx.data_ptr(), dy.data_ptr(), dla.data_ptr(), dlb.data_ptr(), per.data_ptr(), out.data_ptr(),
                                            n, hi, hi, s, st), "t2s_eval_dtw_ragged")

        shift(), dtw()
        torch.cuda.synchronize()
        cb, cd = numpy_shift(x, y, la, lb)
        cw = numpy_dtw(x, y, la, lb)
        row = {"pairs": n, "lengths": [lo, hi], "n_series": s,
               "best_shift_equal": bool(np.array_equal(best.cpu().numpy(), cb)),
               "max_rel_difference_min_dist": float(np.max(np.abs(dist.cpu().numpy() - cd) / cd)),
               "max_rel_difference_dtw": float(np.max(np.abs(per.cpu().numpy() - cw) / cw))}
        run(row, {"gpu_shift": shift, "gpu_dtw_ragged": dtw},
            {"cpu_numpy_shift": lambda: numpy_shift(x, y, la, lb), "cpu_numpy_dtw": lambda: numpy_dtw(x, y, la, lb)})
        row["cpu_over_gpu_shift"] = round(row["cpu_numpy_shift"]["median_ms"] / row["gpu_shift"]["median_ms"], 1)
        row["cpu_over_gpu_dtw"] = round(row["cpu_numpy_dtw"]["median_ms"] / row["gpu_dtw_ragged"]["median_ms"], 1)
        json.dump(result, open(a.out, "w"), indent=1)

    n, length, s = 2048, 144, 10
    rs = np.random.RandomState(3)
    mix = rs.uniform(-1, 1, (s, s)) + np.eye(s)
    ori = (rs.randn(n, length, s) @ mix).astype(np.float32)
    gen = (rs.randn(n, length, s) @ (mix + 0.3 * rs.uniform(-1, 1, (s, s)))).astype(np.float32)
    do, dg = torch.from_numpy(ori).to(dev).reshape(-1, s), torch.from_numpy(gen).to(dev).reshape(-1, s)
    ws = torch.empty(lib.t2s_eval_corr_workspace_bytes(n * length, n * length, s), dtype=torch.uint8, device=dev)
    corr, out = torch.empty(2, s, s, device=dev), torch.empty(1, device=dev)

    def score():
        L.check(lib.t2s_eval_corr(do.data_ptr(), dg.data_ptr(), corr.data_ptr(), out.data_ptr(), n * length, n * length, s, ws.data_ptr(),
                                  ws.numel(), st), "t2s_eval_corr")

    score()
    row = {"sets": [n, length, s], "score_gpu": float(out.cpu()[0]), "score_cpu_numpy": numpy_score(ori, gen),
           "score_from_numpy_arrays": M.correlational_score(ori, gen, dev)[0]}
    run(row, {"gpu_corr": score}, {"cpu_numpy_corr": lambda: numpy_score(ori, gen)})
    row["cpu_over_gpu_corr"] = round(row["cpu_numpy_corr"]["median_ms"] / row["gpu_corr"]["median_ms"], 1)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result["cells"][-1]))


if __name__ == "__main__":
    main()
