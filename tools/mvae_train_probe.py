"""One pre-training step of the multichannel LA-VAE (myvqvae.vqvae.shared_eval(..., 'train')) on the HIP backward against the
torch-op path of the same mirror.

    python tools/mvae_train_probe.py [--shapes 10:144:64,7:96:50] [--batch 128] [--rounds 5] [--steps 20]
                                     [--out profiles/mvae_train.json]

A shape is channels:length:flow_dim; the defaults are the bench-press model at 4 x 36 samples and the deadlift model at
2 x 48, at the fork's batch size 128.  Both paths run the SAME module, optimizer (T2SAdamW) and torch MSE terms; the path is
chosen with T2S_MVAE_BACKWARD = hip | torch, which the mirror reads at every call: `torch` is Encoder / Decoder
._forward_autograd (torch convolutions under autograd: what the codec trained through before it had a HIP backward), `hip` is
t2s_vae_encode_mc / t2s_vae_decode_mc behind _EncodeFn / _DecodeFn with t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc
(the forwards, the nodes and the switch's reader, _torch_forced, are the shared mirror's: t2ms_amd/model/pretrained/_lavae.py).
Timing: one process; per shape a warm-up round of both paths, then `--rounds` rounds in which the two paths alternate (which
goes first alternates too); a round is `--steps` optimisation steps on a resident batch between two device synchronisations,
host clock.  Reported: median and spread (max - min) of the time per step, the ratio of the medians, and `hip_not_slower`:
the HIP median is at most the torch median plus the larger of the two spreads.  Before timing, one step of each path from the
same weights: their losses must agree to 2e-5.
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

SWITCH = "T2S_MVAE_BACKWARD"


def run_steps(model, opt, batch, path, steps):
    import torch
    os.environ[SWITCH] = path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.shared_eval(batch, opt, "train")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:144:64,7:96:50")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mvae_train.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mvae_train_probe: needs a GPU (a CPU timing says nothing about either path)")
    if a.rounds < 5:
        raise SystemExit("mvae_train_probe: at least 5 rounds")
    from model.pretrained.myvqvae import vqvae
    from t2ms_amd import synth
    from t2ms_amd.train import T2SAdamW
    dev = torch.device("cuda:0")
    before = os.environ.get(SWITCH)
    result = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps, "shapes": []}
    for ch, length, width in shapes:
        sd = synth.make_mvae_state_dict(2025, ch, 128, 3, 256)

        def fresh():
            m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256, embedding_dim=64,
                                            flow_dim=width, input_dim=ch))
            m.load_state_dict(sd, strict=True)
            m = m.to(dev).train()
            return m, T2SAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)

        batch = synth.make_mseries(length, a.batch, ch, length).to(dev)
        first = {}
        for path in ("torch", "hip"):                                             # the same step from the same weights
            os.environ[SWITCH] = path
            m, o = fresh()
            first[path] = float(m.shared_eval(batch, o, "train")[0].detach())
        if abs(first["hip"] - first["torch"]) > 2e-5 * abs(first["torch"]):
            raise SystemExit(f"mvae_train_probe: the two paths disagree on the first loss: {first}")
        model, opt = fresh()
        for path in ("torch", "hip"):                                             # warm-up round
            run_steps(model, opt, batch, path, a.steps)
        times = {"torch": [], "hip": []}
        for r in range(a.rounds):
            for path in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                times[path].append(run_steps(model, opt, batch, path, a.steps))
        row = {"channels": ch, "length": length, "flow_dim": width, "first_loss": first}
        for path, xs in times.items():
            row[path] = {"raw_ms_per_step": [round(1e3 * v, 4) for v in xs], "median_ms_per_step": round(1e3 * statistics.median(xs), 4),
                         "spread_ms_per_step": round(1e3 * (max(xs) - min(xs)), 4)}
        row["torch_over_hip"] = round(row["torch"]["median_ms_per_step"] / row["hip"]["median_ms_per_step"], 2)
        row["hip_not_slower"] = row["hip"]["median_ms_per_step"] <= row["torch"]["median_ms_per_step"] + max(
            row["hip"]["spread_ms_per_step"], row["torch"]["spread_ms_per_step"])
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        json.dump(result, open(a.out, "w"), indent=1)
    if before is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = before


if __name__ == "__main__":
    main()
