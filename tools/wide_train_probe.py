"""One training step of the wide-latent DiT (mytrain.py's step: forward, MSE, backward, AdamW) on the HIP path against torch
autograd through the plain-torch restatement of the same network, on the same GPU.

    python tools/wide_train_probe.py [--widths 50,64] [--batch 128] [--rounds 5] [--steps 10] [--out profiles/wide_train.json]
    python tools/wide_train_probe.py --ab480 PARENT_TREE [--rounds 5]      # the 480-token step, another checkout against this one

Wide step.  HIP: Transformer(W).set_trainable(True) under autograd, t2ms_amd.train.mse_loss, T2SAdamW.  torch: the
restatement tests/_wide_train_ref.py (the network the wide gradient tests differentiate) with the oracle's attention on
F.scaled_dot_product_attention -- the branch timm takes in the reference --, F.mse_loss, torch.optim.AdamW; same weights, same
resident batch.  One process; a warm-up round of both paths, then `--rounds` rounds in which the two alternate (which goes
first alternates too); a round is `--steps` optimisation steps between two device synchronisations, host clock.  Reported
per width: median and spread (max - min) of the time per step and the ratio of the medians.  Before timing, the two paths'
first losses from the same weights must agree to 2e-5.  Recorded, not gated.

--ab480.  `tools/bench_train.py --steps 20 --warmup 3` (f32 and bf16 legs) of the tree given and of this tree, each run a
fresh process, alternating, `--rounds` rounds: median and spread of ms_per_step per tree and leg, and `not_slower`: this
tree's median exceeds the other's by no more than the larger of the two spreads.  Goes under "step_480" of the same file.
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def _stats(xs):
    return {"raw_ms_per_step": [round(v, 4) for v in xs], "median_ms_per_step": round(statistics.median(xs), 4),
            "spread_ms_per_step": round(max(xs) - min(xs), 4)}


def _load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def ab480(a):
    """bench_train.py of two trees, fresh processes, alternating."""
    trees = {"parent": os.path.abspath(a.ab480), "branch": REPO}
    times = {(t, d): [] for t in trees for d in ("f32", "bf16")}
    for r in range(a.rounds):
        for tree in (("parent", "branch") if r % 2 == 0 else ("branch", "parent")):
            for dtype in ("f32", "bf16"):
                cmd = [sys.executable, os.path.join(trees[tree], "tools", "bench_train.py"), "--steps", "20", "--warmup", "3", "--dtype", dtype]
                p = subprocess.run(cmd, capture_output=True, text=True, cwd=trees[tree], timeout=600)
                if p.returncode != 0:
                    raise SystemExit(f"wide_train_probe: {' '.join(cmd)} failed ({p.returncode}):\n{p.stdout[-1000:]}{p.stderr[-3000:]}")
                row = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                times[(tree, dtype)].append(float(row["ms_per_step"]))
                print(f"round {r} {tree} {dtype}: {row['ms_per_step']:.4f} ms/step", flush=True)
    out = {"command": "tools/bench_train.py --steps 20 --warmup 3 --dtype <leg>", "rounds": a.rounds}
    for dtype in ("f32", "bf16"):
        p, b = _stats(times[("parent", dtype)]), _stats(times[("branch", dtype)])
        out[dtype] = {"parent": p, "branch": b,
                      "not_slower": b["median_ms_per_step"] <= p["median_ms_per_step"] + max(p["spread_ms_per_step"], b["spread_ms_per_step"])}
    return out


def wide(a):
    import torch
    import torch.nn.functional as F

    import _wide_train_ref as R
    from model.denoiser.mytransformer import Transformer
    from oracle import t2s_oracle as O
    from t2ms_amd import synth
    from t2ms_amd.train import T2SAdamW, mse_loss
    if not torch.cuda.is_available():
        raise SystemExit("wide_train_probe: needs a GPU (a CPU timing says nothing about either path)")
    dev = torch.device("cuda:0")
    O.set_attention_impl("sdpa")
    rows = []
    for W in [int(w) for w in a.widths.split(",")]:
        B = a.batch
        x = synth.make_wide_latents(7100 + W, B, W).to(dev)
        target = synth.make_wide_latents(7200 + W, B, W).to(dev)
        text = synth.make_text_embeddings(71, B).to(dev)
        t = (torch.arange(B, device=dev) % 100).float() / 100.0

        def fresh_hip():
            m = Transformer(W).set_trainable(True)
            m.load_state_dict(R.state_dict(W), strict=True)
            m = m.to(dev).train()
            return m, T2SAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)

        def fresh_torch():
            sd = {k: v.to(dev).requires_grad_(not k.startswith(R.NOGRAD)) for k, v in R.state_dict(W).items()}
            return sd, torch.optim.AdamW([v for v in sd.values() if v.requires_grad], lr=1e-4, weight_decay=0.0)

        def hip_step(m, opt):
            opt.zero_grad()
            loss = mse_loss(m(input=x, t=t, text_input=text), target)
            loss.backward()
            opt.step()
            return loss

        def torch_step(sd, opt):
            opt.zero_grad()
            loss = F.mse_loss(R.forward(sd, x, t, text), target)
            loss.backward()
            opt.step()
            return loss

        paths = {"hip": (hip_step, fresh_hip()), "torch": (torch_step, fresh_torch())}
        first = {k: float(step(*state).detach()) for k, (step, state) in paths.items()}
        if abs(first["hip"] - first["torch"]) > 2e-5 * abs(first["torch"]):
            raise SystemExit(f"wide_train_probe: the two paths disagree on the first loss: {first}")

        def run(k):
            step, state = paths[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(*state)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / a.steps

        for k in paths:
            run(k)
        times = {"hip": [], "torch": []}
        for r in range(a.rounds):
            for k in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
                times[k].append(run(k))
        row = {"flow_dim": W, "tokens": 16 * W, "batch": B, "first_loss": first, "hip": _stats(times["hip"]), "torch": _stats(times["torch"])}
        row["torch_over_hip"] = round(row["torch"]["median_ms_per_step"] / row["hip"]["median_ms_per_step"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del paths
        torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": a.steps, "widths": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="50,64")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ab480", default="", help="another checkout (built) to run tools/bench_train.py against this one")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_train.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("wide_train_probe: at least 5 rounds")
    result = _load(a.out)
    if a.ab480:
        result["step_480"] = ab480(a)
    else:
        result["wide_step"] = wide(a)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
