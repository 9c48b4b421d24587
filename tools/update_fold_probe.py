#!/usr/bin/env python3
"""A/B of two builds of the library on the sampler's update kernels (t2s_ddpm_step / t2s_rf_step / t2s_lms_step and the
sampling loop's update): the bits they produce and the time of a sampling step.  One process loads ONE library (T2S_LIB
selects another build, as tools/ab_libs.sh does), so a comparison is two runs per mode and a third that reads their files:

    python tools/update_fold_probe.py dump a.npz            T2S_LIB=/other/libt2s_hip.so python tools/update_fold_probe.py dump b.npz
    python tools/update_fold_probe.py compare a.npz b.npz        -> array count and the names that differ (exit 1 if any)
    python tools/update_fold_probe.py time a.json [--inner 5]    -> ms per sampling step of five cells, interleaved
    python tools/update_fold_probe.py trace                      -> one 30-step one-lane run per update (for a kernel trace)
    python tools/update_fold_probe.py summary out.json A=a1.json,a2.json,... B=b1.json,...   -> medians, spreads and the bar

dump: every stand-alone entry at B in {1, 3, 53} with and without the conditional prediction, injected and Philox noise,
and 4-step Samplers (L = 24, f32) of every solver: eager, two lanes as a whole-loop and as a one-step graph, per-row
tables, injected noise.  time: B = 256, L = 96, `ancestral` and `ddim` with 50 steps in f32 and bf16x3, and `euler` with
100 steps at B = 1024; every cell is warmed, then the cells take turns `--inner` times and the median is kept.  The bar of
`summary`: median of B <= median of A + A's own min-max spread over the processes."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SOLVER_CASES = (("ddpm", "ancestral", 4, {}), ("flowmatching", "euler", 4, {}), ("ddpm", "ddim", 60, dict(sample_steps=4, eta=0.5)),
                ("ddpm", "dpmpp2m", 60, dict(sample_steps=4)), ("flowmatching", "ab2", 4, {}))


def dump(path):
    import numpy as np
    import torch
    import bench
    from t2ms_amd import _lib as L
    from t2ms_amd import synth
    from t2ms_amd.model.backbone.DDPM import ddpm_host_tables
    from t2ms_amd.sampler import Sampler, lms_step
    dev = torch.device("cuda:0")
    out = {}
    rs = np.random.RandomState(11)
    ddpm_coef = ddpm_host_tables(1000)["coef"].to(dev)
    lms_coef = torch.tensor([[0.83, -1.7, 0.41, 0.6, 1.3, -0.9], [0.9, -0.3, 0, 0, 1.5, -0.5], [0.7, 0.2, 0.3, 0.4, 0, 0]],
                            dtype=torch.float32, device=dev)
    for B in (1, 3, 53):
        x, h, u, c, z = (torch.from_numpy(rs.randn(B, 1920).astype(np.float32)).to(dev) for _ in range(5))
        for with_c in (True, False):
            cp = c.data_ptr() if with_c else None
            xd = x.clone()
            L.check(L.lib().t2s_rf_step(xd.data_ptr(), u.data_ptr(), cp, 5.0, 0.01, B, L.stream_ptr(dev)))
            out[f"rf/B{B}/c{int(with_c)}"] = xd.cpu().numpy()
            for injected in (True, False):
                zp = z.data_ptr() if injected else None
                for t in (0, 517, 999):
                    xd = x.clone()
                    L.check(L.lib().t2s_ddpm_step(xd.data_ptr(), u.data_ptr(), cp, zp, ddpm_coef.data_ptr(), t, 9.0, 2025, 17, 7, B,
                                                  L.stream_ptr(dev)))
                    out[f"ddpm/B{B}/c{int(with_c)}/z{int(injected)}/t{t}"] = xd.cpu().numpy()
                for row in range(3):
                    xd, hd = x.clone(), h.clone()
                    lms_step(xd, hd, u, c if with_c else None, lms_coef, row, cfg=7.0, noise=z if injected else None, seed=2025,
                             stream_id=17, row0=7)
                    out[f"lms/B{B}/c{int(with_c)}/z{int(injected)}/row{row}/x"] = xd.cpu().numpy()
                    out[f"lms/B{B}/c{int(with_c)}/z{int(injected)}/row{row}/hist"] = hd.cpu().numpy()
    model, vae = bench.build_models(dev)
    text = synth.make_text_embeddings(1, 64).to(dev)
    for backbone, solver, total, kw in SOLVER_CASES:
        def make(batch, **more):
            return Sampler(model, vae.decoder, backbone, total, 5.0, batch, 24, dev, seed=7, math="f32", solver=solver, **kw, **more)

        def keep(name, res):
            out[f"sampler/{solver}/{name}/latent"] = res[0].cpu().numpy()
            out[f"sampler/{solver}/{name}/series"] = res[1].cpu().numpy()

        for loop_graph in (1, 0):
            s = make(64, loop_graph=loop_graph)
            keep(f"B64_lanes_auto_loop_graph{loop_graph}", s.run(text))
        keep("B6_eager", make(6, use_graph=False, lanes=1).run(text[:6]))
        s = make(6)
        s.set_rows(seeds=[7, 11, 7, 11, 7, 11], key_rows=[5, 0, 3, 1, 4, 2], cfg=[5.0, 5.0, 9.0, 9.0, 5.0, 9.0])
        keep("B6_set_rows", s.run(text[:6]))
        s = make(4)
        g = torch.Generator().manual_seed(3)
        x_T = torch.randn(4, 64, 30, generator=g)
        noise = torch.randn(s.steps, 4, 64, 30, generator=g) if backbone == "ddpm" else None
        keep("B4_injected", s.run(text[:4], x_T=x_T, noise=noise))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{os.path.basename(L.LIB_PATH)} ({L.LIB_PATH}): wrote {len(out)} arrays to {path}")


def compare(a, b):
    import numpy as np
    A, Bz = np.load(a), np.load(b)
    names = sorted(set(A.files) | set(Bz.files))
    differ = [n for n in names if n not in A.files or n not in Bz.files or not np.array_equal(A[n], Bz[n], equal_nan=True)]
    finite = all(bool(np.isfinite(A[n]).all()) for n in A.files)
    print(json.dumps({"arrays": len(names), "differ": len(differ), "all_finite": finite, "names_that_differ": differ[:20]}))
    return 1 if differ else 0


def _cells(dev):
    import bench
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    models = {math: bench.build_models(dev) for math in ("f32", "bf16x3")}      # the arithmetic is the model's: one model each
    cells = {"f32_euler_100_B1024": (("flowmatching", 100), dict(math="f32"), 1024)}   # (first: the largest handle)
    for math in ("f32", "bf16x3"):
        cells[f"{math}_ancestral_50_B256"] = (("ddpm", 50), dict(math=math), 256)
        cells[f"{math}_ddim_50_B256"] = (("ddpm", 1000), dict(math=math, solver="ddim", sample_steps=50), 256)
    samplers = {}
    for name, ((backbone, total), kw, B) in cells.items():
        model, vae = models[kw["math"]]
        s = Sampler(model, vae.decoder, backbone, total, 9.0, B, 96, dev, seed=1, **kw)
        s.run(synth.make_text_embeddings(3, B).to(dev))
        samplers[name] = s
    return samplers


def timing(path, inner):
    import torch
    from t2ms_amd import _lib as L
    dev = torch.device("cuda:0")
    samplers = _cells(dev)
    torch.cuda.synchronize()
    times = {n: [] for n in samplers}
    for _ in range(inner):
        for n, s in samplers.items():
            t0 = time.perf_counter()
            s.run_inplace()
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    res = {"lib": L.LIB_PATH, "inner": inner,
           "ms_per_step": {n: round(1e3 * statistics.median(t) / samplers[n].steps, 5) for n, t in times.items()}}
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


def trace():
    """One lane, 30 steps, B = 256, one update kernel per run: what a kernel trace of the update kernels needs."""
    import torch
    import bench
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    dev = torch.device("cuda:0")
    model, vae = bench.build_models(dev)
    text = synth.make_text_embeddings(3, 256).to(dev)
    for backbone, total, kw in (("ddpm", 30, {}), ("flowmatching", 30, {}), ("ddpm", 1000, dict(solver="ddim", sample_steps=30, eta=0.5))):
        Sampler(model, vae.decoder, backbone, total, 9.0, 256, 96, dev, seed=1, lanes=1, math="f32", **kw).run(text)
    torch.cuda.synchronize()


def summary(path, groups):
    runs = {k: [json.load(open(f))["ms_per_step"] for f in v.split(",")] for k, v in (g.split("=", 1) for g in groups)}
    (ka, a), (kb, b) = runs.items()
    res = {"rounds": {ka: len(a), kb: len(b)}, "cells": {}}
    for cell in a[0]:
        xa, xb = [r[cell] for r in a], [r[cell] for r in b]
        ma, mb, spread = statistics.median(xa), statistics.median(xb), max(xa) - min(xa)
        res["cells"][cell] = {f"{ka}_ms_per_step": xa, f"{kb}_ms_per_step": xb, f"{ka}_median": round(ma, 5), f"{kb}_median": round(mb, 5),
                              f"{ka}_spread": round(spread, 5), "within_bar": mb <= ma + spread}
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "compare", "time", "trace", "summary"])
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "dump":
        dump(a.paths[0])
    elif a.mode == "compare":
        sys.exit(compare(a.paths[0], a.paths[1]))
    elif a.mode == "time":
        timing(a.paths[0], a.inner)
    elif a.mode == "trace":
        trace()
    else:
        summary(a.paths[0], a.paths[1:])


if __name__ == "__main__":
    main()
