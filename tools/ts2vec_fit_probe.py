"""TS2Vec.fit on the torch engine against the HIP engine: wall time of initialize_ts2vec.

    python tools/ts2vec_fit_probe.py [--sizes 24,512,4096] [--lengths 24,48,96] [--rounds 5] [--out profiles/ts2vec_fit.json]
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/ts2vec_fit_probe.py --trace hip --iters 20 [--trace-length 24]
    python tools/ts2vec_fit_probe.py --read-trace DIR --iters 20 [--out profiles/ts2vec_fit.json]

Timing: one process; per shape a warm-up round, then `--rounds` rounds in which the two engines alternate (which goes first
alternates too).  A round of an engine is initialize_ts2vec(X, engine=...) from fixed seeds followed by a device
synchronise, timed with the host clock: what evaluation.py pays per C-FID cell, plan drawing and uploads included.  N = 24
with L = 24 is the fixture (tests/golden/ts2vec_fit.npz); the other shapes are seeded sinusoids with noise.  Above 100,000
values fit runs 600 iterations instead of 200.  Reported: median and spread (max - min) per engine, and the ratio of the
medians.  The HIP engine is called not slower where its median is below torch's, or within the larger of the two spreads.

--trace ENGINE runs one fit of --iters iterations on 24 series of --trace-length steps and nothing else (for the profiler, in a run of its
own); --read-trace counts the kernel launches per iteration in the profiler's *_kernel_stats.csv and adds them to --out.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden", "ts2vec_fit.npz")
OURS = ("ts2vec_train_fwd_kernel", "ts2vec_loss_kernel", "ts2vec_train_bwd_kernel", "ts2vec_wgrad_kernel", "adamw_multi_kernel",
        "swa_multi_kernel")


def series(n, length):
    import numpy as np
    if (n, length) == (24, 24):
        return np.load(GOLD)["ori"].astype(np.float32)
    rs = np.random.RandomState(1000 * n + length)
    t = np.arange(length, dtype=np.float32)[None, :, None]
    x = np.sin(t * rs.uniform(0.1, 1.0, (n, 1, 1)) + rs.uniform(0, 6.28, (n, 1, 1))) + 0.3 * rs.randn(n, length, 1)
    return x.astype(np.float32)


def one_fit(x, engine, n_iters=None):
    import numpy as np
    import torch
    from t2ms_amd import ts2vec as T
    torch.manual_seed(8)
    np.random.seed(8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if n_iters is None:
        m = T.initialize_ts2vec(x, device="cuda:0", engine=engine)
    else:
        m = T.TS2Vec(input_dims=x.shape[-1], device="cuda:0", batch_size=8, lr=0.001, output_dims=100, max_train_length=3000,
                     engine=engine)
        m.fit(x, n_iters=n_iters)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m


def read_trace(directory, iters):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    calls, ours = 0, {}
    for row in csv.DictReader(open(max(files, key=os.path.getmtime))):
        n = int(row["Calls"])
        calls += n
        for k in OURS:
            if k in row["Name"]:
                ours[k] = ours.get(k, 0) + n
    return {"iters": iters, "all_kernel_launches": calls, "all_launches_per_iter": round(calls / iters, 1),
            "step_kernels": ours, "step_launches_per_iter": round(sum(ours.values()) / iters, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24,512,4096")
    ap.add_argument("--lengths", default="24,48,96")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ts2vec_fit.json"))
    ap.add_argument("--trace", choices=("torch", "hip"))
    ap.add_argument("--read-trace")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace-length", type=int, default=24)
    a = ap.parse_args()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.read_trace:
        result.setdefault("kernel_trace", {})[os.path.basename(os.path.normpath(a.read_trace))] = read_trace(a.read_trace, a.iters)
        json.dump(result, open(a.out, "w"), indent=1)
        print(json.dumps(result["kernel_trace"]))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ts2vec_fit_probe: needs a GPU (a CPU timing says nothing about either engine)")
    if a.trace:
        one_fit(series(24, a.trace_length), a.trace, n_iters=a.iters)
        return
    if a.rounds < 5:
        raise SystemExit("ts2vec_fit_probe: at least 5 rounds")
    shapes = []
    for n in (int(s) for s in a.sizes.split(",")):
        for length in (int(s) for s in a.lengths.split(",")):
            x = series(n, length)
            one_fit(x, "torch"), one_fit(x, "hip")                               # warm-up round
            times = {"torch": [], "hip": []}
            for r in range(a.rounds):
                for engine in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                    dt, m = one_fit(x, engine)
                    times[engine].append(dt)
            row = {"n_series": n, "length": length, "n_iters": m.n_iters}
            for engine, xs in times.items():
                row[engine] = {"raw_s": [round(v, 4) for v in xs], "median_s": round(statistics.median(xs), 4),
                               "spread_s": round(max(xs) - min(xs), 4)}
            row["torch_over_hip"] = round(row["torch"]["median_s"] / row["hip"]["median_s"], 2)
            row["hip_not_slower"] = bool(row["hip"]["median_s"] <= row["torch"]["median_s"] +
                                         max(row["torch"]["spread_s"], row["hip"]["spread_s"]))
            shapes.append(row)
            print(json.dumps(row), flush=True)
            result["device"] = torch.cuda.get_device_name(0)
            result["rounds"] = a.rounds
            result["shapes"] = shapes
            json.dump(result, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
