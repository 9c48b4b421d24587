"""The multichannel LA-VAE codec (t2s_vae_encode_mc / t2s_vae_decode_mc) against the torch-op path of the same mirror
(model/pretrained/myvqvae.py Encoder / Decoder; their _forward_autograd is the shared mirror's, t2ms_amd/model/pretrained/
_lavae.py) under no_grad, on the same GPU.

    python tools/mvae_probe.py [--batch 256] [--rounds 5] [--iters 50] [--out profiles/mvae.json]

Shapes: (C 10, L 144, W 64) -- bench press at the longest training length, two time tiles -- and (C 7, L 72, W 50), deadlift.
Both paths run the SAME module on the same resident inputs.  Timing: one process; per shape and direction a warm-up round of
both paths, then `--rounds` rounds in which the two paths alternate (which goes first alternates too); a round is `--iters`
calls between two device synchronisations, host clock.  Reported: median and spread (max - min) of the time per call and the
ratio of the medians.  Recorded, not gated: no target exists for either side.
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

SHAPES = ((10, 144, 64), (7, 72, 50))      # (channels, length, flow_dim)


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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mvae.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mvae_probe: needs a GPU (a CPU timing says nothing about either path)")
    if a.rounds < 5:
        raise SystemExit("mvae_probe: at least 5 rounds")
    from model.pretrained.myvqvae import vqvae
    from t2ms_amd import synth
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "rounds": a.rounds, "calls_per_round": a.iters, "shapes": []}
    for ch, length, W in SHAPES:
        m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256, embedding_dim=64,
                                        flow_dim=W, input_dim=ch))
        m.load_state_dict(synth.make_mvae_state_dict(2025, ch), strict=True)
        m = m.to(dev).eval()
        x = synth.make_mseries(length, a.batch, ch, length).to(dev)
        with torch.no_grad():
            z, _ = m.encoder(x)
            paths = {"encode": {"hip": lambda: m.encoder(x), "torch": lambda: m.encoder._forward_autograd(x)},
                     "decode": {"hip": lambda: m.decoder(z, length), "torch": lambda: m.decoder._forward_autograd(z, length)}}
            row = {"channels": ch, "length": length, "latent_w": W}
            for direction, fns in paths.items():
                d = float((fns["hip"]()[0] - fns["torch"]()[0]).abs().max())       # the two paths compute the same thing
                for path in ("torch", "hip"):                                       # warm-up round
                    timed(fns[path], a.iters)
                times = {"torch": [], "hip": []}
                for r in range(a.rounds):
                    for path in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                        times[path].append(timed(fns[path], a.iters))
                rec = {"max_abs_diff_hip_vs_torch": d}
                for path, xs in times.items():
                    rec[path] = {"raw_ms_per_call": [round(1e3 * v, 4) for v in xs], "median_ms_per_call": round(1e3 * statistics.median(xs), 4),
                                 "spread_ms_per_call": round(1e3 * (max(xs) - min(xs)), 4)}
                rec["torch_over_hip"] = round(rec["torch"]["median_ms_per_call"] / rec["hip"]["median_ms_per_call"], 2)
                row[direction] = rec
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
