"""The HIP backward of the multichannel LA-VAE codec: t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc (csrc/t2s_vae.hip,
one scaffold with the single-channel entries), the autograd nodes of model.pretrained.myvqvae behind them, and the motion path of
pretrain_lavae.py.

Reference: CPU fp32 autograd through the restatement of the codec in tests/test_mvae.py (_ref_encode / _ref_decode), weights from
synth.make_mvae_state_dict with the configurations of tests/golden/mvae.npz's plan, inputs from synth.make_mseries /
make_wide_latents.  Bars: every gradient tensor within GRAD_TOL = 2e-4 of its own largest magnitude (the project's bar for the
exact-fp32 weight-gradient GEMMs), losses to rtol 2e-5.  On the shapes below fp32 and fp64 autograd of the restatement agree to
<= 7.4e-7 of each tensor's largest and 6e-8 on the loss, and no gradient tensor is identically zero, so the reference sits about
270 times inside the bar.
"""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from t2ms_amd import _lib as L
from t2ms_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mvae import _ref_decode, _ref_encode  # noqa: E402  (the restatement)

pytestmark = pytest.mark.gpu

GRAD_TOL, LOSS_RTOL = 2e-4, 2e-5
E_INVALID = -1
NEW_ENTRIES = ("t2s_vae_encode_backward_mc", "t2s_vae_decode_backward_mc")

# (cfg, W, L, B)
SHAPES = [("c7", 50, 36, 3),       # baseline
          ("c7", 50, 37, 2),       # L % 4 = 1: the transposed final resampling
          ("c7", 50, 39, 2),       # odd L/2
          ("c7r1", 30, 50, 2),     # res_hidden 128, one layer, L % 4 = 2
          ("c10", 64, 128, 2),     # the largest TB = 32 series, latent wider than the tile
          ("c10", 64, 144, 2),     # TB = 48
          ("c7", 50, 192, 2),      # the upper bound
          ("c16", 2, 8, 2),        # most channels, shortest series
          ("c1", 1, 24, 1)]        # one channel, width 1


@pytest.fixture(scope="module")
def plan(golden_dir):
    with np.load(os.path.join(golden_dir, "mvae.npz")) as f:
        return json.loads(str(f["plan"]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _state_dict(plan, cfg):
    k = plan["cfgs"][cfg]
    return synth.make_mvae_state_dict(k["seed"], k["channels"], 128, k["n_res"], k["res_hidden"])


def _inputs(plan, cfg, W, Ln, B):
    ch = plan["cfgs"][cfg]["channels"]
    s = 1000 * ch + 7 * B + W + Ln
    return synth.make_mseries(s, B, ch, Ln), synth.make_wide_latents(s, B, W)


def _upstream(plan, cfg, W, Ln, B):
    """Seeded N(0,1) output gradients: dz (B,64,W), dbefore / dafter (B,64,L//4), drecon (B,C,L)."""
    ch = plan["cfgs"][cfg]["channels"]
    rs = np.random.RandomState(77 + 1000 * ch + 7 * B + W + Ln)
    mk = lambda *shape: torch.from_numpy(rs.randn(*shape).astype(np.float32))  # noqa: E731
    return {"dz": mk(B, 64, W), "dbefore": mk(B, 64, Ln // 4), "drecon": mk(B, ch, Ln), "dafter": mk(B, 64, Ln // 4)}


def _model(plan, cfg, W):
    from model.pretrained.myvqvae import vqvae
    k = plan["cfgs"][cfg]
    m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=k["n_res"], res_hidden_size=k["res_hidden"],
                                    embedding_dim=64, flow_dim=W, input_dim=k["channels"]))
    m.load_state_dict(_state_dict(plan, cfg), strict=True)
    return m


_GPU_MODELS, _REF = {}, {}


def _gpu_model(plan, dev, cfg, W):
    """A shared model for the tests that do not change weights (requires_grad flags are left as built: all trainable)."""
    if (cfg, W) not in _GPU_MODELS:
        _GPU_MODELS[(cfg, W)] = _model(plan, cfg, W).to(dev)
    return _GPU_MODELS[(cfg, W)]


def _ref_kernel_grads(plan, cfg, W, Ln, B, aux):
    """CPU autograd of the restatement under the linear losses <z, dz> (+ <before, dbefore>) and <rec, drecon> (+ <after,
    dafter>) on the decode of the N(0,1) latent: name -> gradient, plus 'dz' of the decoder.  Computed once per case."""
    key = (cfg, W, Ln, B, aux)
    if key not in _REF:
        sd = {k: v.clone().requires_grad_(True) for k, v in _state_dict(plan, cfg).items()}
        x, zr = _inputs(plan, cfg, W, Ln, B)
        up = _upstream(plan, cfg, W, Ln, B)
        zr = zr.clone().requires_grad_(True)
        z, before = _ref_encode(sd, x, W)
        rec, after = _ref_decode(sd, zr, Ln)
        loss = (z * up["dz"]).sum() + (rec * up["drecon"]).sum()
        if aux:
            loss = loss + (before * up["dbefore"]).sum() + (after * up["dafter"]).sum()
        loss.backward()
        out = {k: v.grad for k, v in sd.items()}
        out["dz"] = zr.grad
        _REF[key] = out
    return _REF[key]


def _check(name, got, want, tag=""):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name
    big = float(want.abs().max())
    d = float((got - want).abs().max())
    print(f"  {tag}{name}: max|d| = {d:.3e}, largest {big:.3e}, ratio {d / big if big else float('inf'):.2e} (bar {GRAD_TOL:.0e})")
    assert big > 0 and d < GRAD_TOL * big, (tag, name, d, big)


def _grad_struct(codec, struct, fill=float("nan")):
    """A gradient struct over fresh tensors (pre-filled: an entry must overwrite every one) -> (struct, {param name: tensor})."""
    params = codec._grad_params()
    names = {id(p): n for n, p in codec.named_parameters()}
    tensors = [torch.full_like(p, fill, dtype=torch.float32) for p in params]
    g, ptrs, n = struct(), iter(t.data_ptr() for t in tensors), len(codec._residual_stack._layers)
    for name, ctype in struct._fields_:
        if ctype is C.c_void_p:
            setattr(g, name, next(ptrs))
        else:
            getattr(g, name)[:n] = [next(ptrs) for _ in range(n)]
    return g, {names[id(p)]: t for p, t in zip(params, tensors)}


def _enc_backward(m, dev, x, dz, dbefore, W, entry="t2s_vae_encode_backward_mc"):
    g, out = _grad_struct(m.encoder, L.VaeEncGrads)
    B, Ln = x.shape[0], x.shape[-1]
    args = [m.encoder._handle(dev), x.data_ptr(), dz.data_ptr(), None if dbefore is None else dbefore.data_ptr(), C.byref(g), B, Ln]
    args += [W] if entry.endswith("_mc") else []
    L.check(getattr(L.lib(), entry)(*args, L.stream_ptr(dev)), entry)
    torch.cuda.synchronize()
    return out


def _dec_backward(m, dev, z, drecon, dafter, Ln, want_dz=True, entry="t2s_vae_decode_backward_mc"):
    g, out = _grad_struct(m.decoder, L.VaeDecGrads)
    dz = torch.full_like(z, float("nan")) if want_dz else None
    L.check(getattr(L.lib(), entry)(m.decoder._handle(dev), z.data_ptr(), drecon.data_ptr(), None if dafter is None else dafter.data_ptr(),
                                    C.byref(g), None if dz is None else dz.data_ptr(), z.shape[0], Ln, z.shape[2], L.stream_ptr(dev)), entry)
    torch.cuda.synchronize()
    return out, dz


# ------------------------------------------------------------------------------------------------ 1. kernels against autograd
@pytest.mark.parametrize("aux", [True, False], ids=["aux", "noaux"])
@pytest.mark.parametrize("cfg,W,Ln,B", SHAPES)
def test_kernels_against_autograd(plan, dev, cfg, W, Ln, B, aux):
    """Both entries called directly: every field of the two gradient structs and the decoder's dz against CPU autograd, with
    dbefore / dafter given and NULL."""
    m = _gpu_model(plan, dev, cfg, W)
    x, zr = (t.to(dev) for t in _inputs(plan, cfg, W, Ln, B))
    up = {k: v.to(dev) for k, v in _upstream(plan, cfg, W, Ln, B).items()}
    ref = _ref_kernel_grads(plan, cfg, W, Ln, B, aux)
    tag = f"{cfg} W{W} L{Ln} B{B} {'aux' if aux else 'noaux'} "
    enc = _enc_backward(m, dev, x, up["dz"], up["dbefore"] if aux else None, W)
    assert len(enc) == 8 + 2 * plan["cfgs"][cfg]["n_res"]
    for n, t in enc.items():
        _check("encoder." + n, t, ref["encoder." + n], tag)
    dec, dz = _dec_backward(m, dev, zr, up["drecon"], up["dafter"] if aux else None, Ln)
    assert len(dec) == 6 + 2 * plan["cfgs"][cfg]["n_res"]
    for n, t in dec.items():
        _check("decoder." + n, t, ref["decoder." + n], tag)
    _check("dz", dz, ref["dz"], tag)


def test_decoder_without_dz(plan, dev):
    """dz = NULL: the parameter gradients of the call that computes it, bit for bit."""
    cfg, W, Ln, B = SHAPES[0]
    m = _gpu_model(plan, dev, cfg, W)
    zr = _inputs(plan, cfg, W, Ln, B)[1].to(dev)
    up = {k: v.to(dev) for k, v in _upstream(plan, cfg, W, Ln, B).items()}
    with_dz, dz = _dec_backward(m, dev, zr, up["drecon"], up["dafter"], Ln)
    without, none = _dec_backward(m, dev, zr, up["drecon"], up["dafter"], Ln, want_dz=False)
    assert none is None and dz is not None
    ref = _ref_kernel_grads(plan, cfg, W, Ln, B, True)
    for n in with_dz:
        assert torch.equal(with_dz[n], without[n]), n
        _check("decoder." + n, without[n], ref["decoder." + n], "dz NULL ")


# ------------------------------------------------------------------------------------------------ 2. one codec
def test_one_channel_is_the_single_channel_backward(plan, dev):
    """A channels = 1 multichannel handle and a single-channel handle on the same weights (L 24, W 30, B 2): the _mc entries
    give the gradients of t2s_vae_encode_backward / t2s_vae_decode_backward bit for bit."""
    from model.pretrained.vqvae import vqvae as vqvae1
    m = _gpu_model(plan, dev, "c1", 30)
    k = plan["cfgs"]["c1"]
    s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=k["n_res"], res_hidden_size=k["res_hidden"],
                                     embedding_dim=64))
    s.load_state_dict(_state_dict(plan, "c1"), strict=True)
    s = s.to(dev)
    x, zr = (t.to(dev) for t in _inputs(plan, "c1", 30, 24, 2))
    up = {k_: v.to(dev) for k_, v in _upstream(plan, "c1", 30, 24, 2).items()}
    for aux in (True, False):
        db, da = (up["dbefore"], up["dafter"]) if aux else (None, None)
        a = _enc_backward(m, dev, x, up["dz"], db, 30)
        b = _enc_backward(s, dev, x[:, 0, :].contiguous(), up["dz"], db, 30, entry="t2s_vae_encode_backward")
        assert set(a) == set(b)
        for n in a:
            assert bool(torch.isfinite(a[n]).all()) and torch.equal(a[n], b[n]), ("encoder", n, aux)
        a, dza = _dec_backward(m, dev, zr, up["drecon"], da, 24)
        b, dzb = _dec_backward(s, dev, zr, up["drecon"][:, 0, :].contiguous(), da, 24, entry="t2s_vae_decode_backward")
        for n in a:
            assert bool(torch.isfinite(a[n]).all()) and torch.equal(a[n], b[n]), ("decoder", n, aux)
        assert torch.equal(dza, dzb)


# ------------------------------------------------------------------------------------------------ 3. determinism and growth
def test_determinism_and_row_block_growth(plan, dev):
    """Two calls give equal bits; B = 2, then B = 6 (the row blocks grow), then B = 2 again gives the B = 2 bits, and the B = 6
    call that grew them gives the bits of a B = 6 call on a fresh handle.  (Accuracy is test_kernels_against_autograd's: this
    B = 6 batch has a residual-layer pre-activation of 4e-9, inside the fp32 summation noise of 2e-8, where the ReLU's
    gradient is not defined to fp32 -- no bar applies to it.)"""
    m = _model(plan, "c7", 50).to(dev)          # its own handles: the row blocks start empty
    runs = {}
    for B in (2, 6):
        x, zr = (t.to(dev) for t in _inputs(plan, "c7", 50, 36, B))
        up = {k: v.to(dev) for k, v in _upstream(plan, "c7", 50, 36, B).items()}
        runs[B] = (x, zr, up)

    def both(B, model=m):
        x, zr, up = runs[B]
        enc = _enc_backward(model, dev, x, up["dz"], up["dbefore"], 50)
        dec, dz = _dec_backward(model, dev, zr, up["drecon"], up["dafter"], 36)
        return {**{"e." + n: t for n, t in enc.items()}, **{"d." + n: t for n, t in dec.items()}, "dz": dz}

    first, again = both(2), both(2)
    for n in first:
        assert bool(torch.isfinite(first[n]).all()) and torch.equal(first[n], again[n]), n
    ref = _ref_kernel_grads(plan, "c7", 50, 36, 2, True)
    _check("encoder._conv_1.weight", first["e._conv_1.weight"], ref["encoder._conv_1.weight"], "B 2 ")
    _check("decoder._conv_trans_2.weight", first["d._conv_trans_2.weight"], ref["decoder._conv_trans_2.weight"], "B 2 ")
    grown, fresh = both(6), both(6, _model(plan, "c7", 50).to(dev))
    for n in grown:
        assert bool(torch.isfinite(grown[n]).all()) and torch.equal(grown[n], fresh[n]), n
    back = both(2)
    for n in first:
        assert torch.equal(first[n], back[n]), n


@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_mirror_grows_row_blocks_under_the_device_lock(plan, dev, side, monkeypatch):
    """Through the mirror, a backward that grows the row blocks (rows or series beyond what the handle holds) takes the
    device's lock, and only such a backward: the spy and the shapes of test_backward_grows_its_row_blocks_under_the_device_lock."""
    import gc
    gc.collect()
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "hip")
    entries, real = [0], L.device_lock

    def counting(device):
        entries[0] += 1
        return real(device)

    monkeypatch.setattr(L, "device_lock", counting)
    codec = getattr(_model(plan, "c7", 50).to(dev), side)

    def backward_entries(B, Ln):
        codec.zero_grad(set_to_none=True)
        if side == "encoder":
            z, before = codec(synth.make_mseries(40 + B + Ln, B, 7, Ln).to(dev))
            loss, node = z.sum() + before.sum(), z
        else:
            rec, after = codec(synth.make_wide_latents(40 + B + Ln, B, 50).to(dev), length=Ln)
            loss, node = rec.sum() + after.sum(), after
        assert type(node.grad_fn).__name__ == ("_EncodeFnBackward" if side == "encoder" else "_DecodeFnBackward")
        n0 = entries[0]
        loss.backward()
        n1 = entries[0]
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in codec.parameters())
        return n1 - n0

    assert backward_entries(2, 8) >= 1
    assert backward_entries(2, 8) == 0
    assert backward_entries(3, 8) == 1
    assert backward_entries(1, 16) == 0


# ------------------------------------------------------------------------------------------------ 4. the public class
class _CountingLib:
    """L.lib() with a call counter on the two new entries."""

    def __init__(self, real):
        self._real, self.calls = real, {n: 0 for n in NEW_ENTRIES}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in NEW_ENTRIES:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counting_lib(monkeypatch):
    spy = _CountingLib(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    return spy


def _ref_train_step(plan, cfg, W, x):
    sd = {k: v.clone().requires_grad_(True) for k, v in _state_dict(plan, cfg).items()}
    z, before = _ref_encode(sd, x, W)
    rec, after = _ref_decode(sd, z, x.shape[-1])
    recon = F.mse_loss(rec, x)
    loss = recon + F.mse_loss(before, after)
    loss.backward()
    return sd, float(loss.detach()), float(recon.detach()), rec.detach()


@pytest.mark.parametrize("cfg,W,Ln,B", [("c7", 50, 36, 3), ("c7", 50, 39, 2), ("c10", 64, 144, 2)])
def test_training_step_through_the_public_class(plan, dev, cfg, W, Ln, B, monkeypatch, counting_lib):
    """vqvae.shared_eval(x, T2SAdamW, 'train') under T2S_MVAE_BACKWARD=hip: the tuple's shapes, the loss and the reconstruction
    error, every p.grad, the parameters moved -- and both new entries were called (this does not pass on the torch-op path)."""
    from t2ms_amd.train import T2SAdamW
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "hip")
    m = _model(plan, cfg, W).to(dev).train()
    x = _inputs(plan, cfg, W, Ln, B)[0]
    ch = plan["cfgs"][cfg]["channels"]
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss, recon_error, data_recon, z = m.shared_eval(x.to(dev), T2SAdamW(m.parameters(), lr=1e-3), "train")
    assert counting_lib.calls == {n: 1 for n in NEW_ENTRIES}
    assert loss.dim() == 0 and recon_error.dim() == 0 and tuple(data_recon.shape) == (B, ch, Ln) and tuple(z.shape) == (B, 64, W)
    sd, ref_loss, ref_recon, ref_rec = _ref_train_step(plan, cfg, W, x)
    loss, recon_error = float(loss.detach()), float(recon_error.detach())
    print(f"  {cfg} W{W} L{Ln} B{B}: loss {loss:.8f} (ref {ref_loss:.8f}), recon error {recon_error:.8f} (ref {ref_recon:.8f})")
    assert abs(loss - ref_loss) < LOSS_RTOL * abs(ref_loss) and abs(recon_error - ref_recon) < LOSS_RTOL * abs(ref_recon)
    assert float((data_recon.detach().cpu() - ref_rec).abs().max()) < 1e-5
    params = dict(m.named_parameters())
    assert set(params) == set(sd)
    for k, p in params.items():
        assert p.grad is not None, k
        _check(k, p.grad, sd[k].grad, f"{cfg} L{Ln} ")
        assert not torch.equal(p.detach(), start[k]), k


def test_trainable_encoder_frozen_decoder(plan, dev, monkeypatch, counting_lib):
    """The DiT-training arrangement (a trainable encoder, everything else frozen) under torch losses on z and on the frozen
    decoder's reconstruction: the frozen gradients are None, the encoder's within the bar; `before` is unused (dbefore NULL)."""
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "hip")
    cfg, W, Ln, B = "c7", 50, 36, 3
    m = _model(plan, cfg, W).to(dev).train()
    m.decoder.requires_grad_(False)
    m.encoder._conv_3.bias.requires_grad_(False)
    x, target = _inputs(plan, cfg, W, Ln, B)
    z, _ = m.encoder(x.to(dev))
    rec, _ = m.decoder(z, length=Ln)
    assert type(z.grad_fn).__name__ == "_EncodeFnBackward" and type(rec.grad_fn).__name__ == "_DecodeFnBackward"
    loss = F.mse_loss(z, target.to(dev)) + F.mse_loss(rec, x.to(dev))
    loss.backward()
    assert counting_lib.calls == {n: 1 for n in NEW_ENTRIES}
    sd = {k: v.clone().requires_grad_(True) for k, v in _state_dict(plan, cfg).items()}
    zr, _ = _ref_encode(sd, x, W)
    recr, _ = _ref_decode(sd, zr, Ln)
    ref_loss = F.mse_loss(zr, target) + F.mse_loss(recr, x)
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < LOSS_RTOL * abs(float(ref_loss.detach()))
    for k, p in m.named_parameters():
        if k.startswith("decoder.") or k == "encoder._conv_3.bias":
            assert p.grad is None, k
        else:
            _check(k, p.grad, sd[k].grad, "frozen decoder ")


# ------------------------------------------------------------------------------------------------ 5. fallbacks
@pytest.mark.parametrize("cfg,Ln", [("c7", 196), ("c7r0", 36)])
def test_uncovered_shapes_keep_the_torch_op_path(plan, dev, cfg, Ln, monkeypatch, counting_lib):
    """L = 196 (> 192) and a stack without layers, with grad: _forward_autograd, no call of the new entries, the same bar."""
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "hip")
    W, B = 50, 2
    m = _model(plan, cfg, W).to(dev).train()
    x = _inputs(plan, cfg, W, Ln, B)[0]
    z, before = m.encoder(x.to(dev))
    rec, after = m.decoder(z, length=Ln)
    assert "Fn" not in type(z.grad_fn).__name__ and "Fn" not in type(rec.grad_fn).__name__
    loss = F.mse_loss(rec, x.to(dev)) + F.mse_loss(before, after)
    loss.backward()
    assert counting_lib.calls == {n: 0 for n in NEW_ENTRIES}
    sd, ref_loss, _, _ = _ref_train_step(plan, cfg, W, x)
    assert abs(float(loss.detach()) - ref_loss) < LOSS_RTOL * abs(ref_loss)
    for k, p in m.named_parameters():
        _check(k, p.grad, sd[k].grad, f"{cfg} L{Ln} torch ops ")


def test_switch_to_torch_never_calls_the_new_entries(plan, dev, monkeypatch, counting_lib):
    from t2ms_amd.train import T2SAdamW
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "torch")
    m = _model(plan, "c7", 50).to(dev).train()
    x = _inputs(plan, "c7", 50, 36, 3)[0]
    loss, *_ = m.shared_eval(x.to(dev), T2SAdamW(m.parameters(), lr=1e-3), "train")
    assert counting_lib.calls == {n: 0 for n in NEW_ENTRIES}
    _, ref_loss, _, _ = _ref_train_step(plan, "c7", 50, x)
    assert abs(float(loss.detach()) - ref_loss) < LOSS_RTOL * abs(ref_loss)
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "cuda")
    with pytest.raises(L.T2SError, match="T2S_MVAE_BACKWARD"):
        m.encoder(x.to(dev))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(plan, dev):
    """Every refusal of the two entries: T2S_E_INVALID, its key words, the outputs untouched."""
    from model.pretrained.myvqvae import vqvae
    from model.pretrained.vqvae import vqvae as vqvae1
    lib, st = L.lib(), L.stream_ptr(dev)
    m = _gpu_model(plan, dev, "c7", 50)
    x, zr = (t.to(dev) for t in _inputs(plan, "c7", 50, 36, 2))
    up = {k: v.to(dev) for k, v in _upstream(plan, "c7", 50, 36, 2).items()}
    sentinel = 7.0
    ge, enc_out = _grad_struct(m.encoder, L.VaeEncGrads, sentinel)
    gd, dec_out = _grad_struct(m.decoder, L.VaeDecGrads, sentinel)
    dz_out = torch.full((2, 64, 50), sentinel, device=dev)
    he, hd = m.encoder._handle(dev), m.decoder._handle(dev)

    def enc(h=he, g=ge, B=2, Ln=36, W=50, xp=x.data_ptr(), dzp=up["dz"].data_ptr()):
        return lib.t2s_vae_encode_backward_mc(h, xp, dzp, None, C.byref(g) if g is not None else None, B, Ln, W, st)

    def dec(h=hd, g=gd, B=2, Ln=36, W=50, zp=zr.data_ptr(), drp=up["drecon"].data_ptr()):
        return lib.t2s_vae_decode_backward_mc(h, zp, drp, None, C.byref(g) if g is not None else None, dz_out.data_ptr(), B, Ln, W, st)

    def refused(rc, *words):
        msg = lib.t2s_last_error()
        assert rc == E_INVALID and all(w in msg for w in words), (rc, msg, words)

    # a single-channel handle, naming the single-channel entry
    s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64)).to(dev)
    refused(enc(h=s.encoder._handle(dev)), b"t2s_vae_encode_backward_mc", b"single-channel", b"t2s_vae_encode_backward")
    refused(dec(h=s.decoder._handle(dev)), b"t2s_vae_decode_backward_mc", b"single-channel", b"t2s_vae_decode_backward")
    # length, latent width, batch
    for Ln in (7, 193, 196):
        refused(enc(Ln=Ln), b"L=%d" % Ln, b"unsupported")
        refused(dec(Ln=Ln), b"L=%d" % Ln, b"unsupported")
    for W in (0, 65, -3):
        refused(enc(W=W), b"latent width %d" % W)
        refused(dec(W=W), b"latent width %d" % W)
    for B in (0, -2):
        refused(enc(B=B), b"B=%d" % B)
        refused(dec(B=B), b"B=%d" % B)
    # a handle without the needed weights
    refused(enc(h=hd), b"without encoder weights")
    refused(dec(h=he), b"without decoder weights")
    # no residual layer; hidden other than 128; res_hidden no multiple of 128  (an emb other than 64 never gets a handle:
    # t2s_vae_create_mc refuses it)
    r0 = _gpu_model(plan, dev, "c7r0", 50)
    refused(enc(h=r0.encoder._handle(dev)), b"n_res=0")
    refused(dec(h=r0.decoder._handle(dev)), b"n_res=0")
    for hidden, rh, word in ((64, 128, b"hidden=64"), (128, 64, b"res_hidden=64"), (128, 192, b"res_hidden=192")):
        odd = vqvae(types.SimpleNamespace(block_hidden_size=hidden, num_residual_layers=1, res_hidden_size=rh, embedding_dim=64,
                                          flow_dim=50, input_dim=7)).to(dev)
        refused(enc(h=odd.encoder._handle(dev)), word, b"unsupported")
        refused(dec(h=odd.decoder._handle(dev)), word, b"unsupported")
    w, keep = m.encoder._weights_struct()
    w.emb = 32
    ptr = C.c_void_p()
    assert lib.t2s_vae_create_mc(C.byref(w), 7, C.byref(ptr)) == E_INVALID and b"embedding_dim=32" in lib.t2s_last_error() and not ptr.value
    del keep
    # NULL arguments and NULL gradient pointers
    refused(enc(g=None), b"NULL")
    refused(dec(g=None), b"NULL")
    refused(enc(xp=None), b"NULL")
    refused(dec(drp=None), b"NULL")
    for struct, codec, call, field in ((L.VaeEncGrads, m.encoder, enc, "prevq_b"), (L.VaeDecGrads, m.decoder, dec, "ct2_w")):
        g, _ = _grad_struct(codec, struct, sentinel)
        setattr(g, field, None)
        refused(call(g=g), b"NULL gradient pointer")
        g, _ = _grad_struct(codec, struct, sentinel)
        g.stack_conv1_w[2] = None
        refused(call(g=g), b"NULL gradient pointer", b"residual layer 2")
    torch.cuda.synchronize()
    for t in list(enc_out.values()) + list(dec_out.values()) + [dz_out]:
        assert bool((t == sentinel).all())
    # valid calls still work
    assert enc() == 0 and dec() == 0
    torch.cuda.synchronize()
    ref = _ref_kernel_grads(plan, "c7", 50, 36, 2, False)
    _check("encoder._conv_1.weight", enc_out["_conv_1.weight"], ref["encoder._conv_1.weight"], "after refusals ")
    _check("dz", dz_out, ref["dz"], "after refusals ")


# ------------------------------------------------------------------------------------------------ 7. the driver
DRIVER_ARGV = ["--input_dim", "7", "--flow_dim", "50", "--synthetic", "12", "--split_base_num", "12", "--batch_size", "6",
               "--num_training_updates", "4"]


@pytest.fixture(scope="module")
def driver_run(dev, tmp_path_factory):
    """ONE run of pretrain_lavae.py's pretrain() on the motion path; batches and start weights recorded at `pretrain_step`."""
    import pretrain_lavae as drv
    root = tmp_path_factory.mktemp("mvae")
    calls, keep, real = [], {}, drv.pretrain_step

    def spy(model, opt, batch):
        if not calls:
            keep["sd0"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            keep["model"] = model
        calls.append(batch.detach().cpu().clone())
        return real(model, opt, batch)

    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(root)
        mp.setenv("T2S_MVAE_BACKWARD", "hip")
        mp.setattr(drv, "pretrain_step", spy)
        counter = _CountingLib(L.lib())
        mp.setattr(L, "lib", lambda: counter)
        args = drv.get_args(DRIVER_ARGV + ["--save_path", str(root / "saved")])
        losses = drv.pretrain(args)
    return types.SimpleNamespace(args=args, losses=losses, calls=calls, sd0=keep["sd0"], model=keep["model"],
                                 save_dir=drv.save_dir_of(args), hip_calls=counter.calls)


def test_driver_steps_equal_the_restatement(driver_run):
    """12 rows per group in batches of 6 are 2 batch indices, epochs = int(4 / 2 + 0.5) = 2, one step per length group (12, 24,
    48): 12 steps.  The recorded batches replayed through the CPU restatement with torch.optim.AdamW(1e-3, wd 1e-2) reproduce
    the losses within 2e-5 max(1, |ref|), the bar of test_pretrain_driver_steps_equal_the_oracle."""
    r = driver_run
    assert len(r.losses) == len(r.calls) == 12
    assert [tuple(c.shape) for c in r.calls] == [(6, 7, 12), (6, 7, 24), (6, 7, 48)] * 4
    assert r.hip_calls == {n: 12 for n in NEW_ENTRIES}
    sd = {k: v.clone().requires_grad_(True) for k, v in r.sd0.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, weight_decay=1e-2)
    want = []
    for x in r.calls:
        opt.zero_grad()
        z, before = _ref_encode(sd, x, 50)
        rec, after = _ref_decode(sd, z, x.shape[-1])
        loss = F.mse_loss(rec, x) + F.mse_loss(before, after)
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    print("  driver losses", r.losses, "\n  restatement losses", want)
    for a, b in zip(r.losses, want):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (r.losses, want)


def test_driver_files(driver_run, dev):
    """final_model.pth is a whole-module pickle naming model.pretrained.myvqvae; loaded, it encodes and decodes bit for bit as
    the in-memory model, and its decoder carries the latent width a Sampler checks."""
    r = driver_run
    path = os.path.join(r.save_dir, "final_model.pth")
    assert os.path.exists(path) and os.path.exists(os.path.join(r.save_dir, "model_epoch_0.pth"))
    raw = open(path, "rb").read()
    assert b"model.pretrained.myvqvae" in raw and b"t2ms_amd" not in raw
    from model.pretrained.myvqvae import vqvae
    loaded = torch.load(path, map_location="cpu", weights_only=False)
    assert type(loaded) is vqvae and loaded.decoder.flow_dim == 50 and loaded.encoder.flow_dim == 50
    loaded = loaded.to(dev)
    x = synth.make_mseries(5, 4, 7, 24).to(dev)
    with torch.no_grad():
        za, ba = r.model.encoder(x)
        zb, bb = loaded.encoder(x)
        ra, aa = r.model.decoder(za, length=24)
        rb, ab = loaded.decoder(zb, length=24)
    for a, b in ((za, zb), (ba, bb), (ra, rb), (aa, ab)):
        assert torch.equal(a, b)
    lines = dict(ln.split(": ") for ln in open(os.path.join(r.save_dir, "metrics.txt")).read().strip().splitlines())
    assert set(lines) == {"MAE", "RMSE"} and all(np.isfinite(float(v)) and float(v) >= 0 for v in lines.values())
