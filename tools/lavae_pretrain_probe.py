"""One LA-VAE pre-training step (vqvae.shared_eval(..., 'train')) on the HIP path against the torch-op path of the same mirror
(DESIGN.md section 8).

    python tools/lavae_pretrain_probe.py [--lengths 24,48,96] [--batches 8,1024] [--rounds 7] [--steps 20]
                                         [--out profiles/lavae_pretrain.json]

Both paths run the SAME module, optimizer (T2SAdamW) and MSE kernels; the torch-op path is forced with
T2S_ENCODER_TORCH_AUTOGRAD=1 and T2S_DECODER_TORCH_AUTOGRAD=1 (Encoder / Decoder._forward_autograd: torch convolutions under
autograd), the HIP path is _EncodeFn / _DecodeFn (all of the shared mirror, t2ms_amd/model/pretrained/_lavae.py, which reads
the two switches in _torch_forced).  B = 8 is the reference's default batch, B = 1024 gives each of the 256 CUs
four one-workgroup series.  Timing: one process; per shape a warm-up round of both paths, then `--rounds` rounds in which the
two paths alternate (which goes first alternates too); a round is `--steps` optimisation steps on a resident batch between two
device synchronisations, host clock.  Reported: median and spread (max - min) of the time per step and the ratio of the
medians.  Recorded, not gated: the parent of this feature could not pre-train at all.
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

FORCE = ("T2S_ENCODER_TORCH_AUTOGRAD", "T2S_DECODER_TORCH_AUTOGRAD")


def run_steps(model, opt, batch, path, steps):
    import torch
    for k in FORCE:
        os.environ[k] = "1" if path == "torch" else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.shared_eval(batch, opt, "train")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="24,48,96")
    ap.add_argument("--batches", default="8,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lavae_pretrain.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lavae_pretrain_probe: needs a GPU (a CPU timing says nothing about either path)")
    if a.rounds < 5:
        raise SystemExit("lavae_pretrain_probe: at least 5 rounds")
    from model.pretrained.vqvae import vqvae
    from t2ms_amd import synth
    from t2ms_amd.train import T2SAdamW
    dev = torch.device("cuda:0")
    model = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    model.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    model = model.to(dev).train()
    opt = T2SAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": a.steps, "shapes": []}
    for length in (int(s) for s in a.lengths.split(",")):
        for B in (int(s) for s in a.batches.split(",")):
            batch = synth.make_series(length, B, length).to(dev)
            for path in ("torch", "hip"):                                         # warm-up round
                run_steps(model, opt, batch, path, a.steps)
            times = {"torch": [], "hip": []}
            for r in range(a.rounds):
                for path in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                    times[path].append(run_steps(model, opt, batch, path, a.steps))
            row = {"length": length, "batch": B}
            for path, xs in times.items():
                row[path] = {"raw_ms_per_step": [round(1e3 * v, 4) for v in xs], "median_ms_per_step": round(1e3 * statistics.median(xs), 4),
                             "spread_ms_per_step": round(1e3 * (max(xs) - min(xs)), 4)}
            row["torch_over_hip"] = round(row["torch"]["median_ms_per_step"] / row["hip"]["median_ms_per_step"], 2)
            result["shapes"].append(row)
            print(json.dumps(row), flush=True)
            json.dump(result, open(a.out, "w"), indent=1)
    for k in FORCE:
        os.environ.pop(k, None)


if __name__ == "__main__":
    main()
