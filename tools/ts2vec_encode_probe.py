"""The long-series TS2Vec encoder (t2s_ts2vec_encode_long) against what ran before it: time per call and error against
the oracle.

    python tools/ts2vec_encode_probe.py [--rounds 5] [--calls 10] [--out profiles/ts2vec_encode.json]

(a) N = 2048, T = 96, input_dims 1: the new entry against t2s_ts2vec_encode (the LDS kernel) on the same inputs.
    Recorded only: routing at short T stays on the LDS kernel whichever wins.
(b) N = 512 at (T 300, input_dims 10) and (T 720, input_dims 1): the new entry against the eval-mode torch-op forward of
    t2ms_amd.ts2vec.TSEncoder on the GPU (all-true mask, dropout multiplier 1) followed by the max over time -- the only
    thing that ran at those lengths before.

Timing: one process, seeded weights (synth.make_ts2vec_state_dict(2025)) and uniform [0, 1) series.  Per shape a warm-up
call of each side, then `--rounds` rounds in which the two sides alternate (which goes first alternates too).  A round of a
side is `--calls` calls producing the full-series representation (what C-FID reads) followed by a device synchronise, timed
with the host clock; the workspace and the outputs are allocated before the window.  Reported per side: the per-call median
over the rounds and the spread (max - min), and each side's largest error of the per-step representations of the first 8
series against the CPU oracle, relative to max|rep|.  The new entry is called faster where its median is below the other
side's by more than both spreads.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = (("a", 2048, 96, 1, "lds"), ("b", 512, 300, 10, "torch"), ("b", 512, 720, 1, "torch"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ts2vec_encode.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ts2vec_encode_probe: needs a GPU (a CPU timing says nothing about either side)")
    if a.rounds < 5:
        raise SystemExit("ts2vec_encode_probe: at least 5 rounds")
    from oracle import t2s_oracle as O
    from t2ms_amd import _lib as L
    from t2ms_amd import metrics as M
    from t2ms_amd import synth
    from t2ms_amd.ts2vec import TSEncoder
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream_ptr(dev)
    rows = []
    for part, n, T, cin, other in SHAPES:
        sd = synth.make_ts2vec_state_dict(2025, input_dims=cin)
        enc = M.TS2VecEncoder(sd, dev)
        x = torch.from_numpy(np.random.RandomState(100 * T + cin).uniform(0, 1, size=(n, T, cin)).astype(np.float32)).to(dev)
        full = torch.empty(n, 100, device=dev)
        need = lib.t2s_ts2vec_encode_workspace_bytes(C.byref(enc._w), n, T)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        net = TSEncoder(cin, 100).to(dev).eval()
        net.load_state_dict(sd, strict=True)
        mask, one = torch.ones(n, T, dtype=torch.bool, device=dev), torch.ones(1, 1, 1, device=dev)

        def run_long(xs=x, rep=None, out=full):
            L.check(lib.t2s_ts2vec_encode_long(C.byref(enc._w), xs.data_ptr(), None if rep is None else rep.data_ptr(), out.data_ptr(),
                                               xs.shape[0], T, ws.data_ptr(), need, st), "t2s_ts2vec_encode_long")

        def run_lds(xs=x, rep=None, out=full):
            L.check(lib.t2s_ts2vec_encode(C.byref(enc._w), xs.data_ptr(), None if rep is None else rep.data_ptr(), out.data_ptr(),
                                          xs.shape[0], T, st), "t2s_ts2vec_encode")

        def run_torch(xs=x):
            with torch.no_grad():
                rep = net(xs, mask[:xs.shape[0]], one)
                return rep, rep.max(dim=1).values

        sides = {"long": run_long, other: run_lds if other == "lds" else run_torch}
        # error of each side against the oracle on the first 8 series
        with torch.no_grad():
            want = O.ts2vec_encode(sd, x[:8].cpu())[0].numpy()
        scale = float(np.abs(want).max())
        err = {}
        for name in sides:
            if name == "torch":
                got = run_torch(x[:8])[0]
            else:
                got = torch.empty(8, T, 100, device=dev)
                (run_long if name == "long" else run_lds)(x[:8], got, torch.empty(8, 100, device=dev))
            err[name] = float(np.abs(got.cpu().numpy() - want).max()) / scale
        for fn in sides.values():                                                # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for r in range(a.rounds):
            for name in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    sides[name]()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.calls)
        row = {"part": part, "n_series": n, "length": T, "input_dims": cin, "calls_per_round": a.calls, "workspace_bytes": int(need)}
        for name, xs in times.items():
            row[name] = {"raw_ms": [round(1e3 * v, 3) for v in xs], "median_ms": round(1e3 * statistics.median(xs), 3),
                         "spread_ms": round(1e3 * (max(xs) - min(xs)), 3), "max_err_over_max_rep": float(f"{err[name]:.3e}")}
        row[f"{other}_over_long"] = round(row[other]["median_ms"] / row["long"]["median_ms"], 2)
        row["long_faster_beyond_both_spreads"] = bool(row["long"]["median_ms"] + row["long"]["spread_ms"] + row[other]["spread_ms"]
                                                      < row[other]["median_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": rows}, open(a.out, "w"), indent=1)
        del x, ws, net, enc


if __name__ == "__main__":
    main()
