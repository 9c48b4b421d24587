#!/usr/bin/env python3
"""Seconds per evaluation of a motion test split (the reference's myevaluation.py: MSE / WAPE / ED / DTW of every clip's runs
on the min-max normalised channels), three ways on the same arrays:

    motion_runs   the one t2ms_amd.metrics.motion_runs call: one upload, t2s_eval_runs' three launches, one download
    per_clip      the same four metrics clip by clip through the existing paired entries (M.mse_wape / M.ed / M.dtw) on
                  host-normalised (R, C, T_s) arrays: per clip two uploads, four entries and four downloads
    numpy         the restatement tests/_myeval_ref.py on the host's CPU

Shape: 64 synthetic clips (myinfer.py --synthetic 64: C = 10, 30 .. 160 steps), R = 10 samples per clip.  Every way is warmed
once, then the three take turns `--rounds` times; per way the median seconds and the spread (min ... max) are reported, and
the ratios of the medians.  Recorded, not gated: nothing in the suite depends on these figures.

    python tools/myeval_probe.py [--rounds 5] [--out profiles/myeval.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

CLIPS, CHANNELS, RUNS, SEED = 64, 10, 10, 2025


def make_split():
    """The clips myinfer.py --synthetic 64 samples, and RUNS noisy copies of each in place of a model's samples."""
    from t2ms_amd import synth
    rng = np.random.RandomState(SEED)
    lengths = rng.randint(30, 161, size=CLIPS)
    x1 = [synth.make_mseries(SEED + i, 1, CHANNELS, int(n))[0].numpy() for i, n in enumerate(lengths)]
    runs = [[(x + 0.1 * (r + 1) * rng.randn(*x.shape)).astype(np.float32) for x in x1] for r in range(RUNS)]
    return x1, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be >= 3 (medians with spreads)")
    import torch

    import _myeval_ref as R
    from t2ms_amd import _lib as L
    from t2ms_amd import metrics as M
    dev = torch.device("cuda:0")
    x1, runs = make_split()

    def motion_runs():
        return M.motion_runs(x1, runs, device=dev)[1].numpy()

    def per_clip():
        rows = []
        for i, x in enumerate(x1):
            b = R.normalize(x)
            a = np.stack([R.normalize(run[i]) for run in runs])
            g = np.ascontiguousarray(np.broadcast_to(b, a.shape))
            _, _, per = M.mse_wape(a, g, device=dev)
            w = per[:, 1].numpy()
            rows.append([float(per[:, 0].mean()), float(np.nanmean(w)) if np.isfinite(w).any() else float("nan"),
                         M.ed(a, g, device=dev)[0], M.dtw(a, g, device=dev)[0]])
        return np.asarray(rows)

    def numpy_ref():
        return R.evaluate(x1, runs)[1]

    ways = {"motion_runs": motion_runs, "per_clip": per_clip, "numpy": numpy_ref}
    values = {n: f() for n, f in ways.items()}          # warm-up, and the three agree
    torch.cuda.synchronize()
    for n in ("motion_runs", "per_clip"):
        err = float(np.nanmax(np.abs(values[n] - values["numpy"]) / np.abs(values["numpy"])))
        assert err < 1e-4, (n, err)
    seconds = {n: [] for n in ways}
    for r in range(args.rounds):
        order = list(ways) if r % 2 == 0 else list(ways)[::-1]
        for n in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ways[n]()
            torch.cuda.synchronize()
            seconds[n].append(time.perf_counter() - t0)
    out = {"rounds": args.rounds, "clips": CLIPS, "channels": CHANNELS, "runs": RUNS, "lengths": "30..160",
           "device": torch.cuda.get_device_name(0), "version": L.lib().t2s_version().decode(),
           "note": "wall seconds of the whole call, host packing / normalising and transfers included; recorded, not gated",
           "seconds": {}}
    for n, t in seconds.items():
        med = statistics.median(t)
        out["seconds"][n] = {"median": round(med, 6), "min": round(min(t), 6), "max": round(max(t), 6),
                             "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2), "runs": len(t)}
    base = out["seconds"]["motion_runs"]
    out["ratio_of_medians"] = {f"{n}/motion_runs": round(out["seconds"][n]["median"] / base["median"], 3) for n in ("per_clip", "numpy")}
    # a ratio stands outside the spread when even the slowest motion_runs round beats the fastest round of the other way
    out["outside_spread"] = {f"{n}/motion_runs": bool(out["seconds"][n]["min"] > base["max"]) for n in ("per_clip", "numpy")}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
