#!/usr/bin/env python3
"""Generate tests/golden/wide_dit.npz by RUNNING THE REFERENCE's wide-latent denoiser (model/denoiser/mytransformer.py,
imported unmodified; its timm dependency supplied by gen_golden._install_timm_stub, see there) on the CPU:

    MKL_CBWR=COMPATIBLE,STRICT PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_wide.py --reference DIR

(MKL_CBWR: see gen_golden.py.)

The reference never travels: only the arrays written below are committed.  Weights and inputs are regenerated from seeds
(``t2ms_amd.synth`` and the functions below, which tests/test_wide_dit.py imports), so the file holds OUTPUTS only, plus --
as one JSON string under "plan" -- the cases, the reference module's state-dict key names and shapes at dim 50 and 64, and,
per case, the deviation of the reference's fp32 result from an fp64 run of itself on the same fp32 time embedding (what
the fixture is good for).

Forward cases (W, B): conditional forward with integer t, unconditional forward, conditional forward with float t, and the
``post_mlp_3`` hook tap (output of the last block) of row 0 at every 7th token.
Chains (W 50, B 2): a 3-step CFG DDPM chain with injected noise and a 3-step CFG flow chain, recorded as gen_golden.py
records chains.npz, with the reference's DDPM / RectifiedFlow classes around mytransformer.Transformer(50).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

WEIGHT_SEED = 2025
FORWARD_CASES = [dict(W=50, B=3), dict(W=64, B=2), dict(W=64, B=1)]
CHAIN = dict(W=50, B=2, steps=3, cfg=7.0, weight_seed=31337, gain=0.7)
TAP_STRIDE = 7


def case_key(c):
    return f"W{c['W']}_B{c['B']}"


def forward_inputs(synth, c):
    """(x (B,64,W), text (B,128), integer t (B,), float t (B,)) of a forward case: functions of the case alone."""
    s = 4000 + 10 * c["W"] + c["B"]
    t_long = torch.tensor([999, 500, 3][:c["B"]])
    t_float = torch.tensor([0.0, 0.25, 0.99][:c["B"]])
    return synth.make_wide_latents(s, c["B"], c["W"]), synth.make_text_embeddings(s, c["B"]), t_long, t_float


def chain_inputs(synth):
    """(x_T (B,64,W), text (B,128), noise (steps,B,64,W)) of the two chains."""
    c = CHAIN
    noise = np.random.RandomState(199).randn(c["steps"], c["B"], 64, c["W"]).astype(np.float32)
    return synth.make_wide_latents(31337, c["B"], c["W"]), synth.make_text_embeddings(31337, c["B"]), torch.from_numpy(noise)


def wide_state_dict(synth, width, seed=WEIGHT_SEED, **kw):
    return synth.make_dit_state_dict(seed, width=width, **kw)


class _Widen(torch.nn.Module):
    """fp32 module, fp64 result"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, *a):
        return self.inner(*a).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (Bill9125/T2MS)")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    torch.set_num_threads(8)
    from t2ms_amd import synth
    sys.path.insert(0, HERE)
    import gen_golden
    gen_golden._install_timm_stub()
    # the repo's own `model/` package would shadow the reference's: take the repo off the path once synth is imported
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") not in (REPO, HERE)]
    for k in [k for k in sys.modules if k.split(".")[0] == "model"]:
        del sys.modules[k]
    os.chdir(HERE)
    sys.path.insert(0, ref)
    from model.backbone.DDPM import DDPM
    from model.backbone.rectified_flow import RectifiedFlow
    from model.denoiser.mytransformer import Transformer
    for mod in ("model.backbone.DDPM", "model.backbone.rectified_flow", "model.denoiser.mytransformer"):
        assert sys.modules[mod].__file__.startswith(ref + os.sep), (mod, sys.modules[mod].__file__)

    def model(width, sd):
        m = Transformer(width).eval()
        m.load_state_dict(sd, strict=True)
        return m

    out, dev64, keys = {}, {}, {}
    with torch.no_grad():
        for c in FORWARD_CASES:
            key = case_key(c)
            sd = wide_state_dict(synth, c["W"])
            m = model(c["W"], sd)
            keys[str(c["W"])] = {k: list(v.shape) for k, v in m.state_dict().items()}
            # the fp64 run of the reference itself.  Its time embedding stays the fp32 module's (widened): sin / cos of
            # 100 t / f at t = 999 move by 1e-3 with the fp32 rounding of their ARGUMENT alone, which is the reference's
            # definition of the embedding (the kernels evaluate the same fp32 argument), not arithmetic error of the network
            m64 = model(c["W"], sd).double()
            m64.time_emb = _Widen(m.time_emb)
            x, text, t_long, t_float = forward_inputs(synth, c)
            taps = {}
            hook = m.layers[3].register_forward_hook(lambda mod, a, o: taps.__setitem__("t", o.detach().clone()))
            y_c = m(input=x, t=t_long, text_input=text)
            hook.remove()
            y_u = m(input=x, t=t_long, text_input=None)
            y_f = m(input=x, t=t_float, text_input=text)
            out[f"cond_{key}"], out[f"uncond_{key}"], out[f"cond_float_{key}"] = y_c, y_u, y_f
            out[f"tap_post_mlp_3_{key}"] = taps["t"][:1, ::TAP_STRIDE].contiguous()
            d = [float((y_c.double() - m64(input=x.double(), t=t_long, text_input=text.double())).abs().max()),
                 float((y_u.double() - m64(input=x.double(), t=t_long, text_input=None)).abs().max()),
                 float((y_f.double() - m64(input=x.double(), t=t_float, text_input=text.double())).abs().max())]
            dev64[key] = dict(cond=d[0], uncond=d[1], cond_float=d[2], rms=float(y_c.pow(2).mean().sqrt()),
                              absmax=float(y_c.abs().max()))
            print(key, dev64[key])
        # the chains, as gen_golden.py section (7)
        c = CHAIN
        m = model(c["W"], wide_state_dict(synth, c["W"], c["weight_seed"], gain=c["gain"]))
        xT, text, noises = chain_inputs(synth)
        steps, cfg, B = c["steps"], c["cfg"], c["B"]
        ddpm, rf = DDPM(steps, "cpu"), RectifiedFlow()
        x = xT.clone()
        for j in range(steps):
            tt = torch.full((B,), steps - 1 - j, dtype=torch.long)
            u = m(input=x, t=tt, text_input=None)
            cc = m(input=x, t=tt, text_input=text)
            pred = u + cfg * (cc - u)
            alpha_bar = ddpm.alpha_bar[tt].reshape(-1, 1, 1)
            alpha = ddpm.alpha[tt].reshape(-1, 1, 1)
            mean = 1 / (alpha ** 0.5) * (x - (1 - alpha) / (1 - alpha_bar) ** .5 * pred)
            x = mean + (ddpm.sigma2[tt].reshape(-1, 1, 1) ** .5) * noises[j]     # p_sample with the draw injected
        out["chain_ddpm_latent"] = x.clone()
        x = xT.clone()
        for j in range(steps):
            tt = torch.round(torch.full((B,), j * 1.0 / steps) * steps) / steps
            u = m(input=x, t=tt, text_input=None)
            cc = m(input=x, t=tt, text_input=text)
            x = rf.euler(x, u + cfg * (cc - u), 1.0 / steps)
        out["chain_rf_latent"] = x.clone()
    plan = dict(weight_seed=WEIGHT_SEED, forward_cases=FORWARD_CASES, chain=CHAIN, tap_stride=TAP_STRIDE,
                state_dict=keys, fp32_vs_fp64=dev64)
    arrs = {k: v.numpy() for k, v in out.items()}
    arrs["plan"] = np.asarray(json.dumps(plan))
    path = os.path.join(args.out, "wide_dit.npz")
    np.savez_compressed(path, **arrs)
    print(f"wide_dit.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
