#!/usr/bin/env python3
"""Series/s of the guidance interval (Sampler(guide_steps=...), t2s_sampler_set_guided_steps): classifier-free guidance on a
window of the loop, the conditional pass alone -- half the sequences -- on the other steps.  Two shapes, f32:

    headline   B = 256,  L = 96, DDPM 1000 steps, cfg 9   (bench.py's workload)
    config3    B = 1024, L = 96, rectified flow 100 steps, cfg 5, whole loop in one hipGraph per lane

each with the guided window covering 1.0 / 0.5 / 0.25 / 0 of the loop (the MIDDLE of it: (0.25, 0.75), (0.375, 0.625); where
the window sits does not change the work).  One process loads ONE library, so a round is one worker process per library:
this tree's (all windows) and, with --baseline-lib, another build's (the full window only -- it has no other), taking turns
`--rounds` times; inside a worker every cell is warmed once (handle, graph capture, first replay) and then timed in turn.  Per
cell the median series/s over the rounds and the spread (min ... max) are reported, and each window's ratio against the
baseline library's full-window run of the same session (against this library's own full window when there is no baseline).

What is measured is speed.  The guidance interval is not in the reference; sample quality on trained checkpoints has not been
assessed.

    python tools/cfg_interval_probe.py [--rounds 5] [--baseline-lib /path/to/parent/libt2s_hip.so] [--out profiles/cfg_interval.json]
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

SHAPES = {"headline": dict(backbone="ddpm", steps=1000, cfg=9.0, batch=256, loop_graph=-1),
          "config3": dict(backbone="flowmatching", steps=100, cfg=5.0, batch=1024, loop_graph=1)}
LEN = 96
WINDOWS = {"1.0": ("0", "1"), "0.5": ("0.25", "0.75"), "0.25": ("0.375", "0.625"), "0": ("0.5", "0.5")}
NEW_ENTRIES = ("t2s_sampler_set_guided_steps", "t2s_sampler_guided_steps")


def worker(full_only, inner):
    """One process, one library: seconds per run of every cell, the cells taking turns `inner` times."""
    import torch
    from t2ms_amd import _lib as L
    if full_only:                      # a build from before the guidance interval: bind what it exports
        for name in NEW_ENTRIES:
            L.SYMBOLS.pop(name, None)
    import bench
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler, guided_steps
    dev = torch.device("cuda:0")
    cells = {}
    for shape, c in SHAPES.items():
        model, vae = bench.build_models(dev)            # a handle per shape (512 / 2048 sequences)
        text = synth.make_text_embeddings(3, c["batch"]).to(dev)
        for wname, interval in WINDOWS.items():
            if full_only and wname != "1.0":
                continue
            kw = {} if full_only else dict(guide_steps=guided_steps(interval, c["steps"]))
            s = Sampler(model, vae.decoder, c["backbone"], c["steps"], c["cfg"], c["batch"], LEN, dev, seed=1, math="f32",
                        loop_graph=c["loop_graph"], **kw)
            s.run(text)
            cells[f"{shape}/{wname}"] = s
    torch.cuda.synchronize()
    times = {n: [] for n in cells}
    for _ in range(inner):
        for n, s in cells.items():
            t0 = time.perf_counter()
            s.run_inplace()
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    res = {"lib": os.path.basename(L.LIB_PATH), "version": L.lib().t2s_version().decode(), "device": torch.cuda.get_device_name(0),
           "cells": {n: {"seconds": t, "lanes": cells[n].graph_lanes, "guided": list(getattr(cells[n], "_guided", (0, cells[n].steps)))}
                     for n, t in times.items()}}
    print("WORKER " + json.dumps(res), flush=True)


def run_worker(lib, full_only, inner):
    env = dict(os.environ)
    if lib:
        env["T2S_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--inner", str(inner)] + (["--full-only"] if full_only else [])
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("WORKER ")][-1]
    return json.loads(line[len("WORKER "):])


def figures(batch, seconds):
    sps = sorted(batch / t for t in seconds)
    med = statistics.median(sps)
    return {"series_per_s": round(med, 2), "min": round(sps[0], 2), "max": round(sps[-1], 2),
            "spread_pct": round(100.0 * (sps[-1] - sps[0]) / med, 2), "runs": len(sps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="worker processes per library, taking turns")
    ap.add_argument("--inner", type=int, default=1, help="timed runs of every cell per worker")
    ap.add_argument("--baseline-lib", default=None, help="another build of libt2s_hip.so (the parent commit's): its full-window run is the 1.00")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.full_only, args.inner)
    if args.rounds < 3:
        ap.error("--rounds must be >= 3 (medians with spreads)")
    seconds = {"this": {}, "baseline": {}}
    meta = {}
    for r in range(args.rounds):
        turns = [("baseline", args.baseline_lib, True)] if args.baseline_lib else []
        turns.append(("this", os.environ.get("T2S_LIB"), False))
        for who, lib, full_only in (turns if r % 2 == 0 else turns[::-1]):
            res = run_worker(lib, full_only, args.inner)
            meta.setdefault(who, {"lib": res["lib"], "version": res["version"], "device": res["device"],
                                  "cells": {n: {"lanes": c["lanes"], "guided": c["guided"]} for n, c in res["cells"].items()}})
            for n, c in res["cells"].items():
                seconds[who].setdefault(n, []).extend(c["seconds"])
            print(f"round {r} {who}: " + ", ".join(f"{n} {SHAPES[n.split('/')[0]]['batch'] / statistics.median(c['seconds']):.1f}"
                                                   for n, c in res["cells"].items()), flush=True)
    out = {"rounds": args.rounds, "inner": args.inner, "L": LEN, "math": "f32", "shapes": SHAPES, "windows": WINDOWS,
           "note": "speed only: the guidance interval is not in the reference; quality on trained checkpoints not assessed",
           "libraries": meta, "series_per_s": {}}
    for shape, c in SHAPES.items():
        base_who = "baseline" if args.baseline_lib else "this"
        base = figures(c["batch"], seconds[base_who][f"{shape}/1.0"])
        rows = {"baseline_full_window": base} if args.baseline_lib else {}
        for wname in WINDOWS:
            f = figures(c["batch"], seconds["this"][f"{shape}/{wname}"])
            f["guided_steps"] = meta["this"]["cells"][f"{shape}/{wname}"]["guided"]
            f["vs_" + ("baseline" if args.baseline_lib else "own") + "_full_window"] = round(f["series_per_s"] / base["series_per_s"], 4)
            rows[f"window_{wname}"] = f
        out["series_per_s"][shape] = rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
