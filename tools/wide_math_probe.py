#!/usr/bin/env python3
"""ms per sampling step of the three matrix arithmetics at the wide latent widths (Transformer(50) / Transformer(64) after
set_wide_math(True)), and the 480-token bf16x3 / bf16 step of this build against another build of the library.  Recorded,
not gated: whether a driver default should move at the wide widths is decided from the file this writes.

    wide    whole-loop graph, 50-step DDPM, cfg 7, latents only; W 50 and 64, B 256 and 32; f32 / bf16x3 / bf16 of THIS
            library taking turns inside one process, `--rounds` times: median ms per step and the spread (max - min)
    w30     the same loop at width 30 (B 256, L 96 with the decoder), bf16x3 and bf16: one worker process per library --
            this tree's and, with --baseline-lib, the parent commit's -- taking turns `--rounds` times (one process loads one
            library).  The bf16 row kernels were re-templated on the tiles per sequence; their 480-token instantiations
            kept their instructions, so the two libraries should sit inside each other's spread.

    python tools/wide_math_probe.py [--rounds 5] [--baseline-lib /path/to/parent/libt2s_hip.so] [--out profiles/wide_math.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS, CFG = 50, 7.0
WIDE_CELLS = [(W, B) for W in (50, 64) for B in (256, 32)]
MATHS = ("f32", "bf16x3", "bf16")


def worker_wide(rounds):
    import torch
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd import _lib as L
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    dev = torch.device("cuda:0")
    res = {}
    for W, B in WIDE_CELLS:
        text = synth.make_text_embeddings(3, B).to(dev)
        xT = synth.make_wide_latents(3, B, W).to(dev)
        noise = torch.randn(STEPS, B, 64, W, generator=torch.Generator().manual_seed(3)).to(dev)
        runs = {}
        for math in MATHS:      # a model (and handle) per arithmetic: a captured graph keeps its kernels
            m = Transformer(W)
            m.load_state_dict(synth.make_dit_state_dict(2025, width=W), strict=True)
            m = m.to(dev).eval().set_wide_math(True)
            s = Sampler(m, None, "ddpm", STEPS, CFG, B, 96, dev, seed=1, math=math, loop_graph=1)
            s.run(text, x_T=xT, noise=noise, decode=False)           # handle, planes, capture, first replay
            runs[math] = s
        torch.cuda.synchronize()
        times = {math: [] for math in MATHS}
        for _ in range(rounds):
            for math, s in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.run(text, x_T=xT, noise=noise, decode=False)
                torch.cuda.synchronize()
                times[math].append((time.perf_counter() - t0) * 1e3 / STEPS)
        res[f"W{W}_B{B}"] = {math: {"ms_per_step": t, "lanes": runs[math].graph_lanes} for math, t in times.items()}
        del runs
        torch.cuda.empty_cache()
    print("WORKER " + json.dumps({"lib": os.path.basename(L.LIB_PATH), "device": torch.cuda.get_device_name(0), "cells": res}), flush=True)


def worker_w30(old_lib, inner):
    import torch
    from t2ms_amd import _lib as L
    if old_lib:                 # a build from before the wide arithmetics: bind what it exports
        L.SYMBOLS_WIDE_MATH.clear()
    import bench
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    dev = torch.device("cuda:0")
    B = 256
    text = synth.make_text_embeddings(3, B).to(dev)
    runs = {}
    for math in ("bf16x3", "bf16"):
        model, vae = bench.build_models(dev)
        s = Sampler(model, vae.decoder, "ddpm", STEPS, CFG, B, 96, dev, seed=1, math=math, loop_graph=1)
        s.run(text)
        runs[math] = s
    torch.cuda.synchronize()
    times = {math: [] for math in runs}
    for _ in range(inner):
        for math, s in runs.items():
            t0 = time.perf_counter()
            s.run_inplace()
            torch.cuda.synchronize()
            times[math].append((time.perf_counter() - t0) * 1e3 / STEPS)
    print("WORKER " + json.dumps({"lib": os.path.basename(L.LIB_PATH), "version": L.lib().t2s_version().decode(), "cells": times}), flush=True)


def run_worker(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["T2S_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + extra, env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=900).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("WORKER ")][-1]
    return json.loads(line[len("WORKER "):])


def figures(ms):
    return {"ms_per_step": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="the parent commit's libt2s_hip.so, for the 480-token comparison")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=["wide", "w30", "w30-old"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "wide":
        return worker_wide(args.rounds)
    if args.worker:
        return worker_w30(args.worker == "w30-old", 1)
    if args.rounds < 3:
        ap.error("--rounds must be >= 3 (medians with spreads)")
    wide = run_worker(["wide", "--rounds", str(args.rounds)])
    out = {"rounds": args.rounds, "loop": dict(backbone="ddpm", steps=STEPS, cfg=CFG, loop_graph=1), "device": wide["device"],
           "note": "recorded, not gated; no driver default moves on these numbers in the change that recorded them", "wide": {}}
    for cell, per in wide["cells"].items():
        row = {math: dict(figures(c["ms_per_step"]), lanes=c["lanes"]) for math, c in per.items()}
        for math in ("bf16x3", "bf16"):
            row[math]["speedup_vs_f32"] = round(row["f32"]["ms_per_step"] / row[math]["ms_per_step"], 3)
        out["wide"][cell] = row
        print(cell, {m: (r["ms_per_step"], r["spread_ms"]) for m, r in row.items()}, flush=True)
    ms = {"this": {}, "baseline": {}}
    for r in range(args.rounds):
        turns = [("this", ["w30"], os.environ.get("T2S_LIB"))]
        if args.baseline_lib:
            turns.append(("baseline", ["w30-old"], args.baseline_lib))
        for who, extra, lib in (turns if r % 2 == 0 else turns[::-1]):
            res = run_worker(extra, lib)
            for math, t in res["cells"].items():
                ms[who].setdefault(math, []).extend(t)
            print(f"round {r} {who}: " + ", ".join(f"{m} {statistics.median(t):.3f} ms" for m, t in res["cells"].items()), flush=True)
    out["w30_B256"] = {who: {math: figures(t) for math, t in per.items()} for who, per in ms.items() if per}
    if args.baseline_lib:
        for math in ms["this"]:
            a, b = out["w30_B256"]["this"][math], out["w30_B256"]["baseline"][math]
            a["vs_baseline"] = round(a["ms_per_step"] / b["ms_per_step"], 4)
            a["inside_spread"] = abs(a["ms_per_step"] - b["ms_per_step"]) <= max(a["spread_ms"], b["spread_ms"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
