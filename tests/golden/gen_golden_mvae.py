#!/usr/bin/env python3
"""Generate tests/golden/mvae.npz by RUNNING THE REFERENCE's multichannel codec (model/pretrained/myvqvae.py, imported
unmodified) on the CPU.  Run with the reference checkout at hand:

    MKL_CBWR=COMPATIBLE,STRICT PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mvae.py --reference DIR

(MKL_CBWR: see gen_golden.py.)  The reference never travels: only the arrays written below are committed.  Weights and
inputs are regenerated from seeds by ``t2ms_amd.synth``, so the file holds OUTPUTS only, plus -- as one JSON string under
"plan" -- the weight configurations, the list of recorded cases and the state-dict key names and shapes of the reference
module.  tests/test_mvae.py reads the plan back, so the generator and the tests cannot disagree about a case.

Per case (cfg, W, L, B): z (B,64,W), before / after (B,64,L//4), rec (B,C,L) of the encode -> decode round trip, and
recr (B,C,L), the decode of an N(0,1) latent.  stride 1 stores everything in full; stride s > 1 stores z, before and after
at every s-th position plus their fp64 row sums (every position enters), rec / recr in full -- as vae_long.npz does.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

# weight configurations: hidden 128, embedding_dim 64 throughout ("c7": the deadlift model, "c10": bench press)
CFGS = {
    "c7": dict(channels=7, n_res=3, res_hidden=256, seed=2025),
    "c10": dict(channels=10, n_res=3, res_hidden=256, seed=2026),
    "c1": dict(channels=1, n_res=3, res_hidden=256, seed=2027),
    "c16": dict(channels=16, n_res=3, res_hidden=256, seed=2028),
    "c7r1": dict(channels=7, n_res=1, res_hidden=128, seed=2029),
    "c7r0": dict(channels=7, n_res=0, res_hidden=256, seed=2030),
}


def plan_cases():
    cases = []
    for cfg, W in (("c7", 50), ("c10", 64)):                     # the parity grid
        for B in (1, 3):
            for L in (36, 100, 128):
                cases.append(dict(cfg=cfg, W=W, L=L, B=B, stride=1 if B == 1 else 3))
    for L in (9, 37, 101):                                       # lengths that are no multiple of 4
        cases.append(dict(cfg="c7", W=30, L=L, B=1, stride=1))
    for L in (144, 263):                                         # time tiles (L//4 = 36, 65); 5 is coprime with the tile cores
        cases.append(dict(cfg="c10", W=64, L=L, B=1, stride=5))
    cases.append(dict(cfg="c16", W=2, L=8, B=1, stride=1))        # edges
    cases.append(dict(cfg="c1", W=1, L=24, B=1, stride=1))
    cases.append(dict(cfg="c7r1", W=30, L=50, B=1, stride=1))     # other stacks
    cases.append(dict(cfg="c7r0", W=30, L=50, B=1, stride=1))
    return cases


def case_key(c):
    return f"{c['cfg']}_W{c['W']}_L{c['L']}_B{c['B']}"


def case_inputs(synth, c, channels):
    """(x (B,C,L), random latent (B,64,W)) of a case: functions of the case alone."""
    s = 1000 * channels + 7 * c["B"] + c["W"] + c["L"]
    return synth.make_mseries(s, c["B"], channels, c["L"]), synth.make_wide_latents(s, c["B"], c["W"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (Bill9125/T2MS)")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    torch.set_num_threads(8)
    from t2ms_amd import synth
    # the repo's own `model/` package would shadow the reference's: take the repo off the path once synth is imported
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for k in [k for k in sys.modules if k.split(".")[0] == "model"]:
        del sys.modules[k]
    os.chdir(HERE)
    sys.path.insert(0, ref)
    from model.pretrained.myvqvae import vqvae
    assert sys.modules["model.pretrained.myvqvae"].__file__.startswith(ref + os.sep), sys.modules["model.pretrained.myvqvae"].__file__

    models = {}

    def model(cfg, W):
        if (cfg, W) not in models:
            k = CFGS[cfg]
            ns = types.SimpleNamespace(block_hidden_size=128, num_residual_layers=k["n_res"], res_hidden_size=k["res_hidden"],
                                       embedding_dim=64, flow_dim=W, input_dim=k["channels"])
            m = vqvae(ns).eval()
            m.load_state_dict(synth.make_mvae_state_dict(k["seed"], k["channels"], 128, k["n_res"], k["res_hidden"]), strict=True)
            models[(cfg, W)] = m
        return models[(cfg, W)]

    out, cases = {}, plan_cases()
    with torch.no_grad():
        for c in cases:
            m, key, st = model(c["cfg"], c["W"]), case_key(c), c["stride"]
            x, zr = case_inputs(synth, c, CFGS[c["cfg"]]["channels"])
            z, before = m.encoder(x)
            rec, after = m.decoder(z, c["L"])
            recr, _ = m.decoder(zr, c["L"])
            assert rec.shape == x.shape and torch.equal(m(x), rec)
            out[f"rec_{key}"], out[f"recr_{key}"] = rec, recr
            for name, t in (("z", z), ("before", before), ("after", after)):
                out[f"{name}_{key}"] = t[:, :, ::st].contiguous()
                if st > 1:
                    out[f"{name}_rowsum_{key}"] = t.double().sum(dim=2)
    ref_sd = model("c7", 50).state_dict()
    plan = dict(cfgs=CFGS, cases=cases, state_dict_c7={k: list(v.shape) for k, v in ref_sd.items()})
    arrs = {k: v.numpy() for k, v in out.items()}
    arrs["plan"] = np.asarray(json.dumps(plan))
    path = os.path.join(args.out, "mvae.npz")
    np.savez_compressed(path, **arrs)
    print(f"mvae.npz  {os.path.getsize(path) / 1024:.1f} KiB, {len(cases)} cases")


if __name__ == "__main__":
    main()
