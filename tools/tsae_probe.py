"""The attention seq2seq codec's HIP entries (t2s_tsae_encode / t2s_tsae_generate, csrc/t2s_tsae.hip) against the torch-op path of
the same mirror (model/pretrained/TSae.py: TimeSeriesEncoder._forward_torch, TimeSeriesDecoder._generate_torch) under no_grad, on
the same GPU.

    python tools/tsae_probe.py [--rounds 5] [--out profiles/tsae.json]

Shapes: the bench-press configuration (F 10, 3 + 3 layers, d_ff 128, 8 heads) at (T 144, B 1), (T 144, B 128) and (T 36, B 128).
Both paths run the SAME module on the same resident inputs.  Timing: one process; per shape and entry a warm-up of both paths,
then `--rounds` rounds in which the two paths alternate (which goes first alternates too); a round is a fixed number of calls
between two device synchronisations, host clock (encode 200 calls; generate 10 HIP calls, 1 torch call: the torch generation
re-runs the decoder stack over the growing prefix at every step).  Reported: median and spread (max - min) of the time per call
and the ratio of the medians.  Recorded, not gated: no earlier commit runs this model.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ((144, 1), (144, 128), (36, 128))      # (T, B)
ITERS = {"encode": {"hip": 200, "torch": 200}, "generate": {"hip": 10, "torch": 1}}


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsae.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsae_probe: needs a GPU (a CPU timing says nothing about either path)")
    if a.rounds < 5:
        raise SystemExit("tsae_probe: at least 5 rounds")
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    from t2ms_amd import synth
    dev = torch.device("cuda:0")
    m = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=10, flow_dim=64, d_ff=128, num_encoder_layers=3,
                                                          num_decoder_layers=3, num_heads=8))
    m.load_state_dict(synth.make_tsae_state_dict(2025), strict=False)
    m.condition_fusion = None
    m = m.to(dev).eval()
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_round": ITERS, "shapes": []}
    for T, B in SHAPES:
        x = synth.make_tsae_series(T, B, T, 10).to(dev)
        with torch.no_grad():
            memory = m.encoder(x)
            paths = {"encode": {"hip": lambda: m.encoder(x), "torch": lambda: m.encoder._forward_torch(x)},
                     "generate": {"hip": lambda: m.decoder.generate(memory), "torch": lambda: m.decoder._generate_torch(memory)}}
            row = {"T": T, "B": B}
            for entry, fns in paths.items():
                d = float((fns["hip"]() - fns["torch"]()).abs().max())          # the two paths compute the same thing (also warms up)
                for path in ("torch", "hip"):
                    timed(fns[path], ITERS[entry][path])
                times = {"torch": [], "hip": []}
                for r in range(a.rounds):
                    for path in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                        times[path].append(timed(fns[path], ITERS[entry][path]))
                rec = {"max_abs_diff_hip_vs_torch": d}
                for path, xs in times.items():
                    rec[path] = {"raw_ms_per_call": [round(1e3 * v, 4) for v in xs], "median_ms_per_call": round(1e3 * statistics.median(xs), 4),
                                 "spread_ms_per_call": round(1e3 * (max(xs) - min(xs)), 4)}
                rec["torch_over_hip"] = round(rec["torch"]["median_ms_per_call"] / rec["hip"]["median_ms_per_call"], 2)
                # HIP is faster by more than the spread: its slowest round beats torch's fastest
                rec["hip_faster_beyond_spread"] = max(times["hip"]) < min(times["torch"])
                row[entry] = rec
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
