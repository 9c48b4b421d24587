#!/usr/bin/env python3
"""Series/s of the fused sampler in the three matrix arithmetics (f32 / bf16x3 / bf16), INTERLEAVED on one box in one session:

    headline   1000-step CFG DDPM, B = 256, L = 96        (bench.py's workload)
    config3    100-step CFG rectified flow, B = 1024
    small      100-step DDPM at 1 ... 32 series            (--small; the column of tools/small_batch_probe.py)

with the lanes infer.py runs them on (automatic).  Every mode is warmed once (handle, graph capture), then the modes take
turns `--rounds` times, so a drifting clock or a neighbour on the box hits all of them alike; per mode the median and the
spread (min ... max) of its rounds are reported, and the ratios against bf16x3.

    python tools/math_probe.py [--rounds 3] [--small] [--steps-scale 1.0] [--out FILE.json]
    python tools/math_probe.py --one bf16 [--one-steps 30] [--one-lanes 1]     # the workload tools/profile_math.sh profiles

T2S_LIB=<other libt2s_hip.so> runs another build of the library (the parent commit's, for the bf16x3 baseline); a library
without T2S_MATH_BF16 is measured in its two modes.
"""
import argparse
import ctypes
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


# an older build of the library (T2S_LIB = the parent commit's) has no one-plane kernels: bind what it has
HAVE_BF16 = hasattr(ctypes.CDLL(L.LIB_PATH), "t2s_attn_fwd_bf16p")
if not HAVE_BF16:
    L.SYMBOLS.pop("t2s_attn_fwd_bf16p", None)


def measure(model, vae, dev, backbone, steps, cfg, B, maths, rounds):
    text = synth.make_text_embeddings(3, B).to(dev)
    samplers = {}
    for math in maths:
        samplers[math] = Sampler(model, vae.decoder, backbone, steps, cfg, B, 96, dev, seed=1, math=math)
        samplers[math].run(text)                 # handle, capture, first replay
    torch.cuda.synchronize()
    times = {m: [] for m in maths}
    for _ in range(rounds):
        for math in maths:
            t0 = time.perf_counter()
            samplers[math].run_inplace()
            torch.cuda.synchronize()
            times[math].append(time.perf_counter() - t0)
    out = {}
    for math in maths:
        sps = sorted(B / t for t in times[math])
        out[math] = {"series_per_s": round(statistics.median(sps), 2), "min": round(sps[0], 2), "max": round(sps[-1], 2),
                     "spread_pct": round(100.0 * (sps[-1] - sps[0]) / statistics.median(sps), 2),
                     "ms_per_step": round(1e3 * statistics.median(times[math]) / steps, 4), "lanes": samplers[math].graph_lanes}
    if "bf16x3" in out:
        for math in maths:
            out[math]["vs_bf16x3"] = round(out[math]["series_per_s"] / out["bf16x3"]["series_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="also the 1 ... 32 series column (100-step DDPM)")
    ap.add_argument("--only-small", action="store_true")
    ap.add_argument("--steps-scale", type=float, default=1.0, help="shorten the loops (a quick look; series/s is then not the headline's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--maths", default=None, help="comma-separated subset of f32,bf16x3,bf16")
    ap.add_argument("--one", default=None, metavar="MATH", help="profiling target (tools/profile_math.sh): two runs of ONE sampler in this "
                    "arithmetic, B = 256, --one-steps DDPM steps, --one-lanes lanes, nothing else")
    ap.add_argument("--one-steps", type=int, default=30)
    ap.add_argument("--one-lanes", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, vae = bench.build_models(dev)
    if args.one:
        text = synth.make_text_embeddings(3, 256).to(dev)
        s = Sampler(model, vae.decoder, "ddpm", args.one_steps, 9.0, 256, 96, dev, seed=1, math=args.one, lanes=args.one_lanes)
        s.run(text)
        s.run_inplace()
        torch.cuda.synchronize()
        return
    maths = ["f32", "bf16x3", "bf16"] if HAVE_BF16 else ["f32", "bf16x3"]
    if args.maths:
        maths = [m for m in args.maths.split(",") if m in maths]
    out = {"device": torch.cuda.get_device_name(0), "lib": L.LIB_PATH, "rounds": args.rounds, "maths": maths}
    if not args.only_small:
        out["headline_ddpm_1000_B256"] = measure(model, vae, dev, "ddpm", max(1, int(1000 * args.steps_scale)), 9.0, 256, maths, args.rounds)
        print(json.dumps({"headline_ddpm_1000_B256": out["headline_ddpm_1000_B256"]}), flush=True)
        out["config3_rf_100_B1024"] = measure(model, vae, dev, "flowmatching", max(1, int(100 * args.steps_scale)), 7.0, 1024, maths, args.rounds)
        print(json.dumps({"config3_rf_100_B1024": out["config3_rf_100_B1024"]}), flush=True)
    if args.small or args.only_small:
        out["small_ddpm_100"] = {}
        for B in (1, 2, 4, 8, 16, 32):
            out["small_ddpm_100"][f"B{B}"] = measure(model, vae, dev, "ddpm", 100, 9.0, B, maths, args.rounds)
        print(json.dumps({"small_ddpm_100": out["small_ddpm_100"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
