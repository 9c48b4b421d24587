"""One bf16 training step of the wide-latent DiT (mytrain.py --bf16: forward, MSE, backward, AdamW) against the PARENT
build's fp32 wide step and against torch autograd under autocast(bfloat16), on the same GPU.

    python tools/wide_train_bf16_probe.py --baseline-lib PARENT/t2ms_amd/libt2s_hip.so [--variant-lib OTHER.so]
                                          [--widths 50,64 | --widths ""  (the 480-token legs only)] [--batch 128] [--batch480 1152] [--rounds 5] [--steps 10]
                                          [--out profiles/wide_train_bf16.json]

Method of tools/wide_train_probe.py: a warm-up round, then `--rounds` rounds in which the paths alternate (the order turns
round by round); a round is `--steps` optimisation steps between two device synchronisations, host clock; reported are the
median and the spread (max - min) of the time per step.  A library is chosen when a process loads it (T2S_LIB), so every
build runs in a WORKER process of its own, all alive for the whole probe and idle while another is timed:

  branch    this tree's library: the wide bf16 step, the wide fp32 step, the 480-token f32 / bf16 steps, the torch path
  baseline  --baseline-lib, the parent commit's build: the wide fp32 step, the 480-token f32 / bf16 steps
  variant   --variant-lib (optional), another build of this tree (e.g. t2s_attn_bf16.hip with WW = 8): the wide bf16 step

Written: (a) "wide_step" per width -- bf16 (branch) against fp32 (baseline build) and against torch autocast, `faster`: the
bf16 median is below the fp32 one by more than the two spreads together; (b) "step_480" -- f32 and bf16 of branch and
baseline, `not_slower`: the branch median exceeds the baseline's by no more than the larger spread; (c) "attention_share" --
the attention classes' part of the wide bf16 step's kernel time (t2s_dit_timing_*).  Recorded, not gated.
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


# ------------------------------------------------------------------------------------------------ worker
def worker(a):
    """Reads one JSON command per line on stdin, answers one JSON line on stdout."""
    import ctypes as C

    import torch
    import torch.nn.functional as F

    import _wide_train_ref as R
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd import _lib as L
    from t2ms_amd import synth
    from t2ms_amd.train import T2SAdamW, mse_loss
    if a.old_abi:                                  # the parent build has no t2s_wide_train_bf16.h entries; the fp32 paths never call them
        L.SYMBOLS_WIDE_TRAIN_BF16.clear()
    dev = torch.device("cuda:0")
    paths = {}

    def data(W, B):
        if W == 30:
            x, target = synth.make_latents(7100, B).to(dev), synth.make_latents(7200, B).to(dev)
        else:
            x, target = synth.make_wide_latents(7100 + W, B, W).to(dev), synth.make_wide_latents(7200 + W, B, W).to(dev)
        return x, target, synth.make_text_embeddings(71, B).to(dev), (torch.arange(B, device=dev) % 100).float() / 100.0

    def make(kind, W, B):
        x, target, text, t = data(W, B)
        if kind == "torch_autocast":
            sd = {k: v.to(dev).requires_grad_(not k.startswith(R.NOGRAD)) for k, v in R.state_dict(W).items()}
            opt = torch.optim.AdamW([v for v in sd.values() if v.requires_grad], lr=1e-4, weight_decay=0.0)

            def step():
                opt.zero_grad()
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    pred = R.forward(sd, x, t, text)
                loss = F.mse_loss(pred.float(), target)
                loss.backward()
                opt.step()
                return loss
            return step, None
        m = Transformer(W).set_trainable(True)
        if kind == "bf16":
            if W != 30:
                m.set_wide_train_bf16(True)
            m.set_train_dtype("bf16")
        m.load_state_dict(R.state_dict(W), strict=True)
        m = m.to(dev).train()
        opt = T2SAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)

        def step():
            opt.zero_grad()
            loss = mse_loss(m(input=x, t=t, text_input=text), target)
            loss.backward()
            opt.step()
            return loss
        return step, m

    for line in sys.stdin:
        cmd = json.loads(line)
        key = (cmd.get("kind"), cmd.get("W"), cmd.get("B"))
        if cmd["op"] == "make":
            from oracle import t2s_oracle as O
            O.set_attention_impl("sdpa")
            paths[key] = make(*key)
            loss = float(paths[key][0]().detach())
            torch.cuda.synchronize()
            out = {"first_loss": loss}
        elif cmd["op"] == "run":
            step = paths[key][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(cmd["steps"]):
                step()
            torch.cuda.synchronize()
            out = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / cmd["steps"]}
        elif cmd["op"] == "classes":               # HIP-event time per launch class over `steps` steps (t2s_dit_timing_*)
            step, m = paths[key]
            h = m.t2s_handle(dev, 1)
            L.check(L.lib().t2s_dit_timing_begin(h))
            for _ in range(cmd["steps"]):
                step()
            buf = (C.c_double * 18)()
            L.check(L.lib().t2s_dit_timing_end_ex(h, buf, 9))
            names = {3: "gemm", 4: "attn_fwd", 5: "attn_bwd", 6: "wgrad", 7: "elementwise", 8: "tail"}
            out = {"ms_per_step": {n: buf[2 * i] / cmd["steps"] for i, n in names.items()}}
        elif cmd["op"] == "drop":
            paths.pop(key, None)
            torch.cuda.empty_cache()
            out = {}
        else:
            break
        print(json.dumps(out), flush=True)


class Worker:
    def __init__(self, name, lib, old_abi=False):
        env = dict(os.environ)
        if lib:
            env["T2S_LIB"] = os.path.abspath(lib)
        self.name = name
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"] + (["--old-abi"] if old_abi else []),
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=REPO)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        while True:                                # (anything a library prints on the way is not an answer)
            line = self.p.stdout.readline()
            if not line:
                raise SystemExit(f"wide_train_bf16_probe: worker {self.name} ended ({self.p.poll()}) on {cmd}")
            if line.startswith("{"):
                return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def alternate(legs, rounds, steps):
    """legs: {label: (worker, kind, W, B)} -> {label: stats}; one warm-up round, then `rounds` in turning order."""
    labels = list(legs)
    times = {k: [] for k in labels}
    for r in range(-1, rounds):
        order = labels[r % len(labels):] + labels[:r % len(labels)] if r >= 0 else labels
        for k in order:
            w, kind, W, B = legs[k]
            ms = w.ask(op="run", kind=kind, W=W, B=B, steps=steps)["ms_per_step"]
            if r >= 0:
                times[k].append(ms)
                print(f"round {r} {k}: {ms:.3f} ms/step", flush=True)
    return {k: _stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--old-abi", dest="old_abi", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--baseline-lib", default="", help="libt2s_hip.so of the parent commit's build")
    ap.add_argument("--variant-lib", default="", help="another build of this tree's library to A/B the wide bf16 step against")
    ap.add_argument("--variant-name", default="variant")
    ap.add_argument("--widths", default="50,64")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batch480", type=int, default=1152)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-480", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_train_bf16.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.rounds < 5:
        raise SystemExit("wide_train_bf16_probe: at least 5 rounds")
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = json.load(f)
    branch = Worker("branch", "")
    base = Worker("baseline", a.baseline_lib, old_abi=True) if a.baseline_lib else None
    var = Worker(a.variant_name, a.variant_lib) if a.variant_lib else None
    try:
        import torch
        result.update(device=torch.cuda.get_device_name(0), rounds=a.rounds, steps_per_round=a.steps)
        rows = []
        for W in [int(w) for w in a.widths.split(",") if w]:
            B = a.batch
            legs = {"bf16": (branch, "bf16", W, B)}
            first = {"bf16": branch.ask(op="make", kind="bf16", W=W, B=B)["first_loss"]}
            if base:
                legs["f32_parent"] = (base, "f32", W, B)
                first["f32_parent"] = base.ask(op="make", kind="f32", W=W, B=B)["first_loss"]
            if var:
                legs[a.variant_name] = (var, "bf16", W, B)
                first[a.variant_name] = var.ask(op="make", kind="bf16", W=W, B=B)["first_loss"]
            if not a.skip_torch:
                legs["torch_autocast"] = (branch, "torch_autocast", W, B)
                first["torch_autocast"] = branch.ask(op="make", kind="torch_autocast", W=W, B=B)["first_loss"]
            row = {"flow_dim": W, "tokens": 16 * W, "batch": B, "first_loss": first}
            row.update(alternate(legs, a.rounds, a.steps))
            for k in legs:
                if k != "bf16":
                    row[k + "_over_bf16"] = round(row[k]["median_ms_per_step"] / row["bf16"]["median_ms_per_step"], 3)
            if base:
                row["faster_than_parent_f32"] = (row["bf16"]["median_ms_per_step"] + row["bf16"]["spread_ms_per_step"] +
                                                 row["f32_parent"]["spread_ms_per_step"] < row["f32_parent"]["median_ms_per_step"])
            cls = branch.ask(op="classes", kind="bf16", W=W, B=B, steps=3)["ms_per_step"]
            total = sum(cls.values())
            row["kernel_classes_ms_per_step"] = {k: round(v, 4) for k, v in cls.items()}
            row["attention_share"] = round((cls["attn_fwd"] + cls["attn_bwd"]) / total, 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            for w, kind in ((branch, "bf16"), (branch, "torch_autocast"), (base, "f32"), (var, "bf16")):
                if w:
                    w.ask(op="drop", kind=kind, W=W, B=B)
        if rows:
            result["wide_step"] = rows
        if base and not a.skip_480:
            B, legs = a.batch480, {}
            builds = [("parent", base), ("branch", branch)] + ([(a.variant_name, var)] if var else [])
            for dtype in ("f32", "bf16"):
                for name, w in builds:
                    w.ask(op="make", kind=dtype, W=30, B=B)
                    legs[f"{dtype}_{name}"] = (w, dtype, 30, B)
            st = alternate(legs, a.rounds, a.steps)
            out = {"batch": B}
            for dtype in ("f32", "bf16"):
                p, b = st[f"{dtype}_parent"], st[f"{dtype}_branch"]
                out[dtype] = {"parent": p, "branch": b,
                              "not_slower": b["median_ms_per_step"] <= p["median_ms_per_step"] + max(p["spread_ms_per_step"], b["spread_ms_per_step"])}
                if var:
                    out[dtype][a.variant_name] = st[f"{dtype}_{a.variant_name}"]
            result["step_480"] = out
            print(json.dumps(out), flush=True)
    finally:
        for w in (branch, base, var):
            if w:
                w.close()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
