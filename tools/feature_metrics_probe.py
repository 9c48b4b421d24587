"""Wall time of the feature-based measures: t2s_eval_moments (ACD / SD / KD) and t2s_eval_mdd on
the GPU against the same formulas written in torch on the CPU.

    python tools/feature_metrics_probe.py [--shapes 2048x96x1,512x2048x1] [--rounds 7] [--out profiles/feature_metrics.json]

Per shape (n x L x n_series; seeded sinusoids with noise, the generated set skewed and shifted): a warm-up, then
`--rounds` rounds in which the GPU entries and the CPU restatement alternate.  GPU: the arrays are already on the device
(where infer.py's outputs are scored); one round is `--calls` back-to-back calls of an entry followed by a device
synchronise, host clock, divided by the calls -- and, separately, metrics.feature_measures from numpy arrays (upload, both
entries, download).  CPU: torch with `--threads` threads (16), vectorised over columns -- NOT the reference's code, whose
MDD is a Python loop over every (series, time step) and takes 0.2 - 1.5 s at these shapes; the restatement is the fairer
opponent and is checked against the GPU values here.  Reported: medians, spreads (max - min) and their ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def sets(n, length, s):
    import numpy as np
    rs = np.random.RandomState(n + 7 * length + s)
    t = np.arange(length, dtype=np.float64)[None, :, None]
    ori = 0.5 + 0.3 * np.sin(t * rs.uniform(0.1, 0.6, (n, 1, s)) + rs.uniform(0, 6.28, (n, 1, s))) + 0.1 * rs.randn(n, length, s)
    gen = ori + 0.15 * rs.randn(n, length, s) ** 3 + 0.05
    return ori.astype(np.float32), gen.astype(np.float32)


def torch_moments(ori, gen):
    """ACD, SD, KD as the C ABI defines them (include/t2s.h), fp32 torch."""
    import torch

    def stats(x):
        n, length, _ = x.shape
        d = x - x.mean((0, 1))
        var = (d * d).mean((0, 1))
        acf = torch.stack([(d[:, k:] * d[:, :length - k]).mean((0, 1)) / var for k in range(min(64, length))])
        skew = (d ** 3).mean((0, 1)) / d.std((0, 1), unbiased=True) ** 3
        return acf, skew, (d ** 4).mean((0, 1)) / var ** 2 - 3
    ao, so, ko = stats(ori)
    ag, sg, kg = stats(gen)
    return float(((ag - ao) ** 2).sum(0).sqrt().mean()), float((sg - so).abs().mean()), float((kg - ko).abs().mean())


def torch_mdd(ori, gen):
    """MDD as the C ABI defines it: one binning rule for both sets, counts by scatter_add over all columns at once."""
    import torch
    n = ori.shape[0]
    o, g = ori.reshape(n, -1), gen.reshape(n, -1)
    a, b = o.min(0).values, o.max(0).values
    b = torch.where(b == a, a + 1e-5, b)

    def counts(x):
        k = ((x - a) / (b - a) * 50).floor().clamp(0, 49).long()
        inside = ((x >= a) & (x <= b)).float()
        return torch.zeros(50, x.shape[1]).scatter_add_(0, k, inside)
    delta = (b - a) / 50
    return float(((counts(g) - counts(o)).abs() / (n * delta)).mean(0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x96x1,512x2048x1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "feature_metrics.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feature_metrics_probe: needs a GPU (a CPU timing says nothing about the kernels)")
    from t2ms_amd import _lib as L
    from t2ms_amd import metrics as M
    torch.set_num_threads(a.threads)
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "cpu_threads": a.threads, "rounds": a.rounds, "calls_per_round": a.calls,
              "shapes": []}

    def med(xs):
        return {"median_ms": round(1e3 * statistics.median(xs), 4), "spread_ms": round(1e3 * (max(xs) - min(xs)), 4)}

    for shape in a.shapes.split(","):
        n, length, s = (int(v) for v in shape.split("x"))
        ori, gen = sets(n, length, s)
        f = M._Features(ori, gen, dev, "probe")
        to, tg = torch.from_numpy(ori), torch.from_numpy(gen)
        out = torch.empty(4, device=dev)
        lib, st, ws = L.lib(), L.stream_ptr(dev), f.ws

        def gpu(entry):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                L.check(getattr(lib, entry)(f.a.data_ptr(), f.b.data_ptr(), None, out.data_ptr(), n, length, s, ws.data_ptr(),
                                            ws.numel(), st), entry)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.calls

        def wall(fn):
            t0 = time.perf_counter()
            v = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, v

        times = {k: [] for k in ("gpu_moments", "gpu_mdd", "gpu_feature_measures_from_numpy", "cpu_torch_moments", "cpu_torch_mdd")}
        values = {}
        for r in range(a.rounds + 1):                                           # round 0 warms everything up
            order = ("gpu", "cpu") if r % 2 == 0 else ("cpu", "gpu")
            now = {}
            for side in order:
                if side == "gpu":
                    now["gpu_moments"], now["gpu_mdd"] = gpu("t2s_eval_moments"), gpu("t2s_eval_mdd")
                    now["gpu_feature_measures_from_numpy"], values["gpu"] = wall(lambda: M.feature_measures(ori, gen, device=dev)[0])
                else:
                    now["cpu_torch_moments"], mo = wall(lambda: torch_moments(to, tg))
                    now["cpu_torch_mdd"], md = wall(lambda: torch_mdd(to, tg))
                    values["cpu_torch"] = {"MDD": md, "ACD": mo[0], "SD": mo[1], "KD": mo[2]}
            if r:
                for k, v in now.items():
                    times[k].append(v)
        row = {"n": n, "L": length, "n_series": s, "values": values}
        row.update({k: med(v) for k, v in times.items()})
        row["max_rel_difference_of_values"] = max(abs(values["gpu"][k] - values["cpu_torch"][k]) / abs(values["cpu_torch"][k])
                                                  for k in values["gpu"])
        row["cpu_over_gpu_moments"] = round(row["cpu_torch_moments"]["median_ms"] / row["gpu_moments"]["median_ms"], 2)
        row["cpu_over_gpu_mdd"] = round(row["cpu_torch_mdd"]["median_ms"] / row["gpu_mdd"]["median_ms"], 2)
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        json.dump(result, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
