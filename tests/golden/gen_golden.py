#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE in the build container.

Run once, here, with /root/reference mounted:

    MKL_CBWR=COMPATIBLE,STRICT PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden.py

ddpm.npz, time_emb.npz, init_seeded.npz and vae_long.npz were recorded with MKL_CBWR=COMPATIBLE,STRICT: MKL's
reproducible branch, which tests/conftest.py pins so that the bit-exact comparisons hold on any x86 host (MKL's
default branch depends on the CPU vendor).  The other files were recorded on the default branch; their tests
compare at tolerances that hold on either.

The reference never travels: only the arrays written below are committed.
Weights/inputs are regenerated from seeds by ``t2ms_amd.synth`` so the
fixtures hold outputs only.

What executes reference code:
  * model/backbone/DDPM.py, rectified_flow.py, model/pretrained/vqvae.py,
    model/denoiser/mlp.py -- imported unmodified.
  * model/denoiser/transformer.py -- imported unmodified, but its third-party
    dependency ``timm`` (timm==1.0.11, requirements.txt:9) is not installed and
    not on disk, so ``timm.models.vision_transformer.{Attention,Mlp}`` are
    supplied by the two small classes below, which restate the published
    timm 1.0.11 forward.  Everything AROUND those two calls (patchify, pos-emb,
    time-emb, adaLN wiring, gating, final LN, unpatchify) is the real
    reference.  Parity at the timm boundary itself is therefore UNPINNED (see
    oracle/t2s_oracle.py header and DESIGN.md).
"""
import os
import sys
import types
import argparse

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, REPO)


# ---- timm stand-in (published timm 1.0.11 semantics), gen-time only ----------
class _Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, **_):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        x = F.scaled_dot_product_attention(q, k, v)
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class _Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0, **_):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


def _install_timm_stub():
    timm = types.ModuleType("timm")
    models = types.ModuleType("timm.models")
    vt = types.ModuleType("timm.models.vision_transformer")
    vt.Attention, vt.Mlp, vt.PatchEmbed = _Attention, _Mlp, object
    timm.models, models.vision_transformer = models, vt
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.vision_transformer": vt})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_num_threads(8)
    torch.manual_seed(0)

    from t2ms_amd import synth  # seeds -> weights/inputs (shared with the tests)

    _install_timm_stub()
    # The repo's own `model/` (the drop-in mirrors) is a REGULAR package and shadows the reference's namespace package
    # `model` under any sys.path order: take the repo off the path now that t2ms_amd.synth is imported, and assert
    # below that what got imported IS the reference.
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for k in [k for k in sys.modules if k.split(".")[0] == "model"]:
        del sys.modules[k]
    os.chdir(HERE)
    sys.path.insert(0, REF)
    from model.backbone.DDPM import DDPM
    from model.backbone.rectified_flow import RectifiedFlow
    from model.denoiser.transformer import Transformer, TimeEmbedding, get_sinusoidal_positional_embeddings
    from model.denoiser.mlp import MLP
    from model.pretrained.vqvae import vqvae
    for mod in ("model.backbone.DDPM", "model.backbone.rectified_flow", "model.denoiser.transformer", "model.denoiser.mlp",
                "model.pretrained.vqvae"):
        assert sys.modules[mod].__file__.startswith(REF + os.sep), (mod, sys.modules[mod].__file__)

    def save(name, **arrs):
        arrs = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")

    rs = np.random.RandomState(77)

    # (1) DDPM tables + q_sample / p_sample with injected eps --------------------------------
    out = {}
    for T in (50, 1000):
        d = DDPM(T, "cpu")
        out[f"beta_{T}"], out[f"alpha_{T}"], out[f"alpha_bar_{T}"] = d.beta, d.alpha, d.alpha_bar
    d = DDPM(1000, "cpu")
    x0 = torch.from_numpy(rs.randn(4, 64, 30).astype(np.float32))
    eps = torch.from_numpy(rs.randn(4, 64, 30).astype(np.float32))
    eh = torch.from_numpy(rs.randn(4, 64, 30).astype(np.float32))
    t = torch.tensor([0, 1, 500, 999])
    xq, _ = d.q_sample(x0, t, eps)
    # p_sample draws torch.randn internally: inject by seeding the global generator
    torch.manual_seed(1234)
    xp = d.p_sample(x0, eh, t)
    torch.manual_seed(1234)
    noise = torch.randn(x0.shape)
    save("ddpm", x0=x0, eps=eps, eps_hat=eh, t=t, q_sample=xq, p_sample=xp, p_noise=noise, **out)

    # (2) rectified flow -------------------------------------------------------------------
    rf = RectifiedFlow()
    x1 = torch.from_numpy(rs.randn(4, 64, 30).astype(np.float32))
    v = torch.from_numpy(rs.randn(4, 64, 30).astype(np.float32))
    tf = torch.tensor([0.0, 0.37, 0.5, 1.0])
    torch.manual_seed(4321)
    xt, x0f = rf.create_flow(x1, tf)
    save("rf", x1=x1, v=v, t=tf, euler=rf.euler(x1, v, 1.0 / 100), x_t=xt, x_0=x0f)

    # (3) time embedding + positional embedding -------------------------------------------
    te = TimeEmbedding(128)
    tl = torch.tensor([0, 1, 7, 999])
    tfl = torch.tensor([0.0, 0.37, 1.0])
    save("time_emb", t_long=tl, emb_long=te(tl), t_float=tfl, emb_float=te(tfl),
         pos_embed=get_sinusoidal_positional_embeddings(480, 128))

    # (4) DiT forward, cond + uncond, with per-block taps ----------------------------------
    sd = synth.make_dit_state_dict(2025)
    model = Transformer().eval()
    missing = model.load_state_dict(sd, strict=True)
    print("DiT load_state_dict(strict):", missing)
    assert torch.equal(model.pos_embed, sd["pos_embed"])
    x = synth.make_latents(2025, 4)
    text = synth.make_text_embeddings(2025, 4)
    taps = {}
    hooks = []
    for i, layer in enumerate(model.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"post_mlp_{i}", o.detach())))
    with torch.no_grad():
        t_l = torch.tensor([999, 500, 3, 0])
        y_c = model(input=x, t=t_l, text_input=text)
        tap_c = {k: v[:1, ::7].clone() for k, v in taps.items()}   # sample 0, every 7th token
        y_u = model(input=x, t=t_l, text_input=None)
        t_f = torch.tensor([0.0, 0.25, 0.5, 0.99])
        y_cf = model(input=x, t=t_f, text_input=text)
    for h in hooks:
        h.remove()
    save("dit_forward", t_long=t_l, cond=y_c, uncond=y_u, t_float=t_f, cond_float=y_cf,
         **{"tap_" + k: v for k, v in tap_c.items()})

    # (5) standalone attention: qkv -> out (timm-boundary restatement; UNPINNED) -----------
    att = model.layers[0].attn
    xa = torch.from_numpy(np.random.RandomState(4242).randn(2, 480, 128).astype(np.float32))
    with torch.no_grad():
        ya = att(xa)
        ym = model.layers[0].mlp(xa)
    # input is regenerated in the test from RandomState(4242); outputs stored at token stride 5
    save("timm_boundary", attn_out=ya[:, ::5], mlp_out=ym[:, ::5])

    # (6) LA-VAE encode/decode for L in {24,48,96}, B in {1,5} -------------------------------
    vsd = synth.make_vae_state_dict(2025)
    ns = types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64)
    vae = vqvae(ns).eval()
    print("VAE load_state_dict(strict):", vae.load_state_dict(vsd, strict=True))
    out = {}
    with torch.no_grad():
        for L in (24, 48, 96):
            for B in (1, 5):
                xs = synth.make_series(100 + L + B, B, L)
                z, before = vae.encoder(xs)
                rec, after = vae.decoder(z, length=L)
                out[f"z_{L}_{B}"], out[f"before_{L}_{B}"] = z, before
                out[f"rec_{L}_{B}"], out[f"after_{L}_{B}"] = rec, after
                zr = synth.make_latents(300 + L, B)
                rec2, _ = vae.decoder(zr, length=L)
                out[f"rec_rand_{L}_{B}"] = rec2
    save("vae", **out)

    # (7) short chains: 20-step DDPM and 20-step RF, cfg 7, B=4 ------------------------------
    sdc = synth.make_dit_state_dict(31337, gain=0.7)
    model.load_state_dict(sdc, strict=True)
    xT = synth.make_latents(31337, 4)
    text = synth.make_text_embeddings(31337, 4)
    steps, cfg = 20, 7.0
    ddpm = DDPM(steps, "cpu")
    noises = torch.from_numpy(np.random.RandomState(99).randn(steps, 4, 64, 30).astype(np.float32))
    with torch.no_grad():
        x = xT.clone()
        for j in range(steps):
            tt = torch.full((4,), steps - 1 - j, dtype=torch.long)
            u = model(input=x, t=tt, text_input=None)
            c = model(input=x, t=tt, text_input=text)
            pred = u + cfg * (c - u)
            # ddpm.p_sample with the draw injected: re-seed so torch.randn == noises[j]
            alpha_bar = ddpm.alpha_bar[tt].reshape(-1, 1, 1)
            alpha = ddpm.alpha[tt].reshape(-1, 1, 1)
            mean = 1 / (alpha ** 0.5) * (x - (1 - alpha) / (1 - alpha_bar) ** .5 * pred)
            x_manual = mean + (ddpm.sigma2[tt].reshape(-1, 1, 1) ** .5) * noises[j]
            x = x_manual
        x_ddpm = x.clone()
        rec_ddpm, _ = vae.decoder(x_ddpm, length=96)
        x = xT.clone()
        for j in range(steps):
            tt = torch.round(torch.full((4,), j * 1.0 / steps) * steps) / steps
            u = model(input=x, t=tt, text_input=None)
            c = model(input=x, t=tt, text_input=text)
            x = rf.euler(x, u + cfg * (c - u), 1.0 / steps)
        x_rf = x.clone()
        rec_rf, _ = vae.decoder(x_rf, length=96)
    save("chains", ddpm_latent=x_ddpm, ddpm_series=rec_ddpm, rf_latent=x_rf, rf_series=rec_rf)

    # (8) MLP denoiser on (4,64,6) -------------------------------------------------------------
    msd = synth.make_mlp_state_dict(2025)
    mlp = MLP().eval()
    print("MLP load_state_dict(strict):", mlp.load_state_dict(msd, strict=True))
    xm = torch.from_numpy(np.random.RandomState(5).randn(4, 64, 6).astype(np.float32))
    with torch.no_grad():
        ym_c = mlp(xm, torch.tensor([49, 20, 1, 0]), synth.make_text_embeddings(5, 4))
        ym_u = mlp(xm, torch.tensor([49, 20, 1, 0]), None)
    save("mlp_denoiser", x=xm, cond=ym_c, uncond=ym_u)

    # (9) one training step (loss + per-parameter grad norms), fp32 reference -----------------
    model.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    model.train()
    d100 = DDPM(100, "cpu")
    x1 = synth.make_latents(555, 4)
    tt = torch.tensor([3, 50, 77, 99])
    eps = synth.make_latents(556, 4)
    xt, _ = d100.q_sample(x1, tt, eps)
    pred = model(input=xt, t=tt, text_input=synth.make_text_embeddings(555, 4))
    loss = d100.loss(pred, eps)
    loss.backward()
    gn = {k.replace(".", "__"): p.grad.norm() for k, p in model.named_parameters() if p.grad is not None}
    g_qkv0 = model.layers[0].attn.qkv.weight.grad[::16, ::8].clone()
    save("train_step", loss=loss.detach(), grad_qkv0_sample=g_qkv0, **{"gn_" + k: v for k, v in gn.items()})
    print("params with grad:", len(gn), "total numel:",
          sum(p.numel() for p in model.parameters() if p.grad is not None))


if __name__ == "__main__":
    main()
