"""One `shared_eval(batch, None, optimizer, 'train')` step of the attention seq2seq codec (model/pretrained/TSae.py), AdamW
included: the opt-in HIP engine (csrc/t2s_tsae_train.hip through one autograd node) against the torch-op path of the same mirror,
on the same GPU.

    python tools/tsae_train_probe.py [--rounds 5] [--out profiles/tsae_train.json]

Shapes: the bench-press configuration (F 10, 3 + 3 layers, d_ff 128, 8 heads, dropout 0.1, training mode) at B 128 and T 144 / 36.
Two copies of one model (one per engine, each with its own torch.optim.AdamW) step on the same resident batch.  Timing: one
process; per shape a warm-up of both engines, then `--rounds` rounds in which the two alternate (which goes first alternates too);
a round is 20 steps between two device synchronisations, host clock.  Reported: median and spread (max - min) of the time per step
and the ratio of the medians.  Recorded, not gated: no earlier commit has a HIP training step for this model, and the engine is
opt-in whatever the number is.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ((144, 128), (36, 128))      # (T, B)
STEPS = 20


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsae_train.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsae_train_probe: needs a GPU (a CPU timing says nothing about either engine)")
    if a.rounds < 5:
        raise SystemExit("tsae_train_probe: at least 5 rounds")
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    from t2ms_amd import synth
    dev = torch.device("cuda:0")
    base = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=10, flow_dim=64, d_ff=128, num_encoder_layers=3,
                                                             num_decoder_layers=3, num_heads=8))
    base.load_state_dict(synth.make_tsae_state_dict(2025), strict=False)
    base.condition_fusion = None              # never read by the step: no optimizer state for its 25 M parameters
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": STEPS, "optimizer": "torch.optim.AdamW",
              "shapes": []}
    for T, B in SHAPES:
        x = synth.make_tsae_series(T, B, T, 10).to(dev)
        steps, models = {}, {}
        for engine in ("torch", "hip"):
            m = copy.deepcopy(base).to(dev).train()
            m.set_train_engine(engine)
            opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-2)
            models[engine] = m
            steps[engine] = (lambda m=m, opt=opt: m.shared_eval(x, None, opt, "train"))
        first = {e: float(steps[e]()[0].detach()) for e in steps}                       # (also warms up)
        assert models["hip"].__dict__.get("_t2s_h") is not None and models["torch"].__dict__.get("_t2s_h") is None
        for e in steps:
            timed(steps[e], STEPS)
        times = {"torch": [], "hip": []}
        for r in range(a.rounds):
            for e in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                times[e].append(timed(steps[e], STEPS))
        row = {"T": T, "B": B, "first_step_loss": first}
        for e, xs in times.items():
            row[e] = {"raw_ms_per_step": [round(1e3 * v, 4) for v in xs], "median_ms_per_step": round(1e3 * statistics.median(xs), 4),
                      "spread_ms_per_step": round(1e3 * (max(xs) - min(xs)), 4)}
        row["torch_over_hip"] = round(row["torch"]["median_ms_per_step"] / row["hip"]["median_ms_per_step"], 2)
        # HIP is faster by more than both spreads: the medians are further apart than the two spreads together
        row["hip_faster_beyond_spreads"] = (row["torch"]["median_ms_per_step"] - row["hip"]["median_ms_per_step"]
                                            > row["torch"]["spread_ms_per_step"] + row["hip"]["spread_ms_per_step"])
        row["last_step_loss"] = {e: float(steps[e]()[0].detach()) for e in steps}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
