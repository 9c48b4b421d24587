#!/usr/bin/env python3
"""Series/s of the few-step solvers against the ancestral 1000-step loop, and the cost of their update per step, INTERLEAVED
in one process on one box:

    B = 256, L = 96, T = 1000 (bench.py's workload), f32 and bf16x3:
      ancestral 1000 steps | ddim 50 | dpmpp2m 50 | dpmpp2m 20           -> series/s and the ratios against ancestral
    time per step at EQUAL S (--equal-steps, default 50): ancestral (a 50-step schedule) | ddim | dpmpp2m
      -> ms/step and the ratio against ancestral.  The table-driven update adds at most two (B,1920) fp32 streams to a step
         (the history read and write: 3.9 MB on a ~4 ms step at B = 256, under 0.1 %); the bar is <= 1 % slower than the
         ancestral step measured in the same session.

Every cell is warmed once (handle, graph capture, first replay), then the cells take turns `--rounds` times, so a drifting
clock or a neighbour on the box hits all of them alike; per cell the median and the spread (min ... max) are reported.
What is measured is speed; sample quality of these solvers on trained checkpoints has not been assessed.

    python tools/solver_probe.py [--rounds 3] [--out profiles/solvers.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench                                    # noqa: E402
from t2ms_amd import _lib as L                  # noqa: E402
from t2ms_amd import synth                      # noqa: E402
from t2ms_amd.sampler import Sampler            # noqa: E402

B, LEN, T, CFG = 256, 96, 1000, 9.0


def measure(model, vae, dev, math, cells, rounds):
    """cells: {name: (total_step, solver, sample_steps)} -> {name: figures}, the cells interleaved."""
    text = synth.make_text_embeddings(3, B).to(dev)
    samplers = {}
    for name, (total, solver, S) in cells.items():
        samplers[name] = Sampler(model, vae.decoder, "ddpm", total, CFG, B, LEN, dev, seed=1, math=math, solver=solver, sample_steps=S)
        samplers[name].run(text)
    torch.cuda.synchronize()
    times = {n: [] for n in cells}
    for _ in range(rounds):
        for name in cells:
            t0 = time.perf_counter()
            samplers[name].run_inplace()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    out = {}
    for name in cells:
        steps = samplers[name].steps
        sps = sorted(B / t for t in times[name])
        med = statistics.median(times[name])
        out[name] = {"steps": steps, "series_per_s": round(statistics.median(sps), 2), "min": round(sps[0], 2), "max": round(sps[-1], 2),
                     "spread_pct": round(100.0 * (sps[-1] - sps[0]) / statistics.median(sps), 2),
                     "ms_per_run": round(1e3 * med, 3), "ms_per_step": round(1e3 * med / steps, 4), "lanes": samplers[name].graph_lanes}
    samplers.clear()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help=">= 3 rounds of the series/s cells (the equal-S cells run 3x as many)")
    ap.add_argument("--equal-steps", type=int, default=50)
    ap.add_argument("--maths", default="f32,bf16x3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be >= 3 (medians with spreads)")
    dev = torch.device("cuda:0")
    model, vae = bench.build_models(dev)
    S = args.equal_steps
    out = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(L.LIB_PATH), "B": B, "L": LEN, "T": T, "cfg": CFG,
           "rounds": args.rounds, "equal_steps": S}
    for math in args.maths.split(","):
        speed = measure(model, vae, dev, math, {"ancestral_1000": (T, None, None), "ddim_50": (T, "ddim", 50),
                                                "dpmpp2m_50": (T, "dpmpp2m", 50), "dpmpp2m_20": (T, "dpmpp2m", 20)}, args.rounds)
        for n in speed:
            speed[n]["vs_ancestral_1000"] = round(speed[n]["series_per_s"] / speed["ancestral_1000"]["series_per_s"], 3)
        step = measure(model, vae, dev, math, {f"ancestral_{S}": (S, None, None), f"ddim_{S}": (T, "ddim", S),
                                               f"dpmpp2m_{S}": (T, "dpmpp2m", S)}, 3 * args.rounds)
        for n in step:
            step[n]["step_vs_ancestral"] = round(step[n]["ms_per_step"] / step[f"ancestral_{S}"]["ms_per_step"], 4)
        out[math] = {"series_per_s": speed, "time_per_step_equal_S": step,
                     "lms_step_within_1pct_of_ancestral": all(v["step_vs_ancestral"] <= 1.01 for v in step.values())}
        print(json.dumps({math: out[math]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
