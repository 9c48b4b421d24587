"""LA-VAE pre-training on the GPU: t2s_vae_decode_backward behind Decoder.forward, vqvae.shared_eval(..., 'train') and the
pretrain_lavae.py driver, against torch autograd on the CPU through the oracle (oracle.t2s_oracle.vae_encode / vae_decode with
synth.make_vae_state_dict(2025) and synth.make_series).  Needs an MI355X.

Bars (those of the encoder backward and the DiT in tests/test_hip_train.py): a gradient tensor agrees within 2e-4 of the
reference tensor's largest gradient, a loss within rtol 2e-5, forward outputs within 1e-5."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import t2s_oracle as O
from t2ms_amd import synth

pytestmark = pytest.mark.gpu

HP = dict(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64)
GRAD_TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _vae(dev, sd=None):
    from model.pretrained.vqvae import vqvae
    v = vqvae(types.SimpleNamespace(**HP))
    v.load_state_dict(sd if sd is not None else synth.make_vae_state_dict(2025), strict=True)
    return v.to(dev)


def _leaf_sd(scale=1.0, prefixes=("encoder.", "decoder.")):
    return {k: (v * (scale if k.startswith(prefixes) else 1.0)).clone().requires_grad_(k.startswith(prefixes))
            for k, v in synth.make_vae_state_dict(2025).items()}


def _check_grads(named_got, ref_sd, prefix="", tol=GRAD_TOL):
    """Every tensor within `tol` of its reference's largest gradient; returns the worst ratio error / (tol * scale)."""
    worst = 0.0
    for n, got in named_got.items():
        ref = ref_sd[prefix + n].grad
        assert ref is not None and got is not None, n
        assert got.shape == ref.shape, n
        scale = float(ref.abs().max())
        assert scale > 0, n
        err = float((got.detach().cpu() - ref).abs().max())
        print(f"  grad {prefix + n}: max err {err:.3e}  scale {scale:.3e}  ({err / scale:.2e} of scale)")
        assert err < tol * scale, (prefix + n, err, scale)
        worst = max(worst, err / (tol * scale))
    return worst


@pytest.mark.parametrize("Ls,B,W", [(8, 3, 30), (24, 5, 30), (24, 2, 6), (48, 2, 30), (96, 3, 30), (128, 1, 30)])
def test_decoder_backward_kernel_vs_oracle_autograd(dev, Ls, B, W):
    """t2s_vae_decode_backward (vqvae.py:97-105 backwards) on its own: loss = <recon, G> + <after, H> with random G, H and a
    latent that asks for a gradient.  The 10 decoder.* gradients and dz against autograd through the oracle, the forward
    outputs, bit-reproducibility from run to run, and fresh weights after an in-place update without a new handle.  The cases
    cover T = L/4 = 2, an identity interpolation (W = L/4 = 6), a full 32-position tile and the B == 1 squeeze."""
    xs = synth.make_series(700 + Ls, B, Ls)
    rs = np.random.RandomState(Ls + W)
    G = torch.from_numpy(rs.randn(B, Ls).astype(np.float32))
    Hh = torch.from_numpy(rs.randn(B, 64, Ls // 4).astype(np.float32))
    with torch.no_grad():
        z30, before = O.vae_encode(synth.make_vae_state_dict(2025), xs)
    z0 = (z30 if W == 30 else before).clone()
    assert z0.shape == (B, 64, W)

    def oracle(scale):
        vsd = _leaf_sd(scale, ("decoder.",))
        zr = z0.clone().requires_grad_(True)
        rec, after = O.vae_decode(vsd, zr, Ls)
        assert rec.shape == ((B, Ls) if B > 1 else (Ls,))
        ((rec.reshape(B, Ls) * G).sum() + (after * Hh).sum()).backward()
        return vsd, zr, rec.detach(), after.detach()

    vsd, zr, rec_ref, after_ref = oracle(1.0)
    dec = _vae(dev).decoder

    def run():
        dec.zero_grad(set_to_none=True)
        z = z0.to(dev).requires_grad_(True)
        rec, after = dec(z, length=Ls)
        ((rec.reshape(B, Ls) * G.to(dev)).sum() + (after * Hh.to(dev)).sum()).backward()
        return rec, after, z.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in dec.named_parameters()}

    rec, after, dz1, g1 = run()
    assert type(after.grad_fn).__name__ == "_DecodeFnBackward"
    assert rec.shape == rec_ref.shape
    assert float((rec.detach().cpu() - rec_ref).abs().max()) < 1e-5
    assert float((after.detach().cpu() - after_ref).abs().max()) < 1e-5
    assert len(g1) == 10
    _check_grads(g1, vsd, "decoder.")
    zs = float(zr.grad.abs().max())
    assert zs > 0 and float((dz1.cpu() - zr.grad).abs().max()) < GRAD_TOL * zs, (float((dz1.cpu() - zr.grad).abs().max()), zs)
    _, _, dz2, g2 = run()
    assert torch.equal(dz1, dz2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n                                 # fixed summation order
    # an optimizer-style in-place update: same handle, new contents
    h_before = dec.__dict__["_t2s_h"]
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(1.01)
    rec3, _, dz3, g3 = run()
    assert dec.__dict__["_t2s_h"] is h_before
    vsd3, zr3, rec3_ref, _ = oracle(1.01)
    assert float((rec3.detach().cpu() - rec3_ref).abs().max()) < 1e-5
    _check_grads(g3, vsd3, "decoder.")
    assert float((dz3.cpu() - zr3.grad).abs().max()) < GRAD_TOL * float(zr3.grad.abs().max())


@pytest.mark.parametrize("Ls,B", [(24, 5), (96, 3)])
def test_encoder_decoder_chain_gradients(dev, Ls, B):
    """Encoder -> decoder with loss = <recon, G> + <after, H> + <before, K> + <z, J>: all 22 gradients.  The latent gradient
    the decoder kernel returns flows into t2s_vae_encode_backward together with dbefore -- the reconstruction term of the
    pre-training loss alone would hide it (the round trip 30 <-> L/4 is nearly the identity)."""
    xs = synth.make_series(800 + Ls, B, Ls)
    rs = np.random.RandomState(1000 + Ls)
    G, Hh, K, J = (torch.from_numpy(rs.randn(*s).astype(np.float32))
                   for s in ((B, Ls), (B, 64, Ls // 4), (B, 64, Ls // 4), (B, 64, 30)))
    vsd = _leaf_sd()
    z_r, before_r = O.vae_encode(vsd, xs)
    rec_r, after_r = O.vae_decode(vsd, z_r, Ls)
    ((rec_r * G).sum() + (after_r * Hh).sum() + (before_r * K).sum() + (z_r * J).sum()).backward()
    v = _vae(dev)
    z, before = v.encoder(xs.to(dev))
    rec, after = v.decoder(z, length=Ls)
    assert type(z.grad_fn).__name__ == "_EncodeFnBackward" and type(after.grad_fn).__name__ == "_DecodeFnBackward"
    ((rec * G.to(dev)).sum() + (after * Hh.to(dev)).sum() + (before * K.to(dev)).sum() + (z * J.to(dev)).sum()).backward()
    got = {n: p.grad for n, p in v.named_parameters()}
    assert len(got) == 22
    _check_grads(got, vsd)


def _round_tol(p, lr):
    """fp32 rounding of one AdamW update p <- p (1 - lr wd) - lr m^ / (sqrt(v^) + eps): a handful of roundings at the size
    of the parameter and of the update (|update| <= lr on the first step): 4 ulp of each."""
    return 4 * 1.2e-7 * (p.abs() + lr)


@pytest.mark.parametrize("Ls,B", [(24, 5), (96, 3), (8, 1)])
def test_shared_eval_train_step_vs_oracle(dev, Ls, B):
    """vqvae.shared_eval(batch, T2SAdamW, 'train') (vqvae.py:118-127): loss and recon_error (rtol 2e-5), p.grad of all 22
    tensors (2e-4 of the tensor's largest), and the parameters after the step against torch.optim.AdamW(lr 1e-3, wd 1e-2)
    on the oracle's gradients.

    The last comparison, per element: the first AdamW step moves a parameter by lr g / (|g| + eps), whose slope in g is
    eps / (|g| + eps)^2 -- so a gradient error of dg (allowed: 2e-4 of the tensor's largest gradient) may move the update by
    lr dg eps / (|g| + eps)^2, at most 2 lr (a sign flip of a gradient that is itself within dg of zero); on top, 4 ulp of
    rounding at the size of the parameter and of the update (_round_tol).  The test prints the measured deviation next to
    this tolerance.  Measured on an MI355X: gradients within 1.2e-6 of each tensor's largest (bar 2e-4), parameter
    deviations up to 1.1e-6 absolute, the worst element at 0.77 of its tolerance."""
    from t2ms_amd.train import T2SAdamW
    lr, wd, eps = 1e-3, 1e-2, 1e-8
    xs = synth.make_series(900 + Ls, B, Ls)
    vsd = _leaf_sd()
    z_r, before_r = O.vae_encode(vsd, xs)
    rec_r, after_r = O.vae_decode(vsd, z_r, Ls)
    recon_ref = F.mse_loss(rec_r.reshape(B, Ls), xs)
    loss_ref = recon_ref + F.mse_loss(before_r, after_r)
    loss_ref.backward()
    p0 = {k: v.detach().clone() for k, v in vsd.items()}
    ref_opt = torch.optim.AdamW(list(vsd.values()), lr=lr, weight_decay=wd, eps=eps)
    grads_ref = {k: v.grad.clone() for k, v in vsd.items()}
    ref_opt.step()

    v = _vae(dev)
    opt = T2SAdamW(v.parameters(), lr=lr, weight_decay=wd)
    loss, recon_error, data_recon, z = v.shared_eval(xs.to(dev), opt, "train")
    assert data_recon.shape == ((B, Ls) if B > 1 else (Ls,)) and z.shape == (B, 64, 30)
    print(f"  loss {loss.item():.8f} ref {loss_ref.item():.8f}   recon_error {recon_error.item():.8f} ref {recon_ref.item():.8f}")
    np.testing.assert_allclose(loss.item(), loss_ref.item(), rtol=2e-5)
    np.testing.assert_allclose(recon_error.item(), recon_ref.item(), rtol=2e-5)
    assert float((data_recon.reshape(B, Ls).cpu() - rec_r.detach().reshape(B, Ls)).abs().max()) < 1e-5
    got = {n: p.grad for n, p in v.named_parameters()}
    assert len(got) == 22
    _check_grads(got, vsd)
    for n, p in v.named_parameters():
        g = grads_ref[n]
        dg = GRAD_TOL * float(g.abs().max())
        tol = torch.clamp(lr * dg * eps / (g.abs() + eps) ** 2, max=2 * lr) + _round_tol(p0[n], lr)
        dev_ = (p.detach().cpu() - vsd[n].detach()).abs()
        ratio = float((dev_ / tol).max())
        print(f"  param {n}: max deviation {float(dev_.max()):.3e}, worst element at {ratio:.3f} of its tolerance "
              f"(tolerances {float(tol.min()):.2e} .. {float(tol.max()):.2e})")
        assert ratio < 1.0, (n, ratio)
        assert float((p.detach().cpu() - p0[n]).abs().max()) > 0, n        # the step moved it


DRIVER_ARGV = ["--dataset_name", "ETTh1_24", "--synthetic", "24", "--batch_size", "6", "--num_training_updates", "6", "--split_train"]


@pytest.fixture(scope="module")
def driver_run(dev, tmp_path_factory):
    """ONE run of pretrain_lavae.py's pretrain() shared by the driver tests: the batches and the start weights are recorded
    at its `pretrain_step` calls."""
    import pretrain_lavae as drv
    root = tmp_path_factory.mktemp("lavae")
    calls, keep, real = [], {}, drv.pretrain_step

    def spy(model, opt, batch):
        if not calls:
            keep["sd0"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            keep["model"] = model
        calls.append(batch.detach().cpu().clone())
        return real(model, opt, batch)

    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(root)
        mp.setattr(drv, "pretrain_step", spy)
        args = drv.get_args(DRIVER_ARGV + ["--save_path", str(root / "saved")])
        losses = drv.pretrain(args)
    return types.SimpleNamespace(args=args, losses=losses, calls=calls, sd0=keep["sd0"], model=keep["model"],
                                 save_dir=drv.save_dir_of(args))


def test_pretrain_driver_steps_equal_the_oracle(driver_run):
    """pretrain_lavae.py itself against the CPU oracle: the recorded batches replayed through the oracle under autograd with
    torch.optim.AdamW(lr 1e-3, wd 1e-2) must give the driver's losses within 2e-5 max(1, |ref|) (the bar of
    test_train_driver_first_steps_equal_the_oracle; fp32 and fp64 CPU runs of these steps differ by <= 6.5e-7 relative), and
    the sixth loss must be below the first.  (24 rows in batches of 6 are 4 steps per epoch, and the reference's
    epochs = int(updates / len(loader) + 0.5) = 2: the run makes 8 steps, all of which are compared.)"""
    r = driver_run
    assert len(r.losses) == len(r.calls) >= 6 and all(tuple(c.shape) == (6, 24) for c in r.calls)
    sd = {k: v.clone().requires_grad_(True) for k, v in r.sd0.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, weight_decay=1e-2)
    want = []
    for x in r.calls:
        opt.zero_grad()
        z, before = O.vae_encode(sd, x)
        rec, after = O.vae_decode(sd, z, x.shape[-1])
        loss = F.mse_loss(rec, x) + F.mse_loss(before, after)
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    print("  driver losses", r.losses, "\n  oracle losses", want)
    for a, b in zip(r.losses, want):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (r.losses, want)
    assert r.losses[5] < r.losses[0]


def test_pretrain_driver_files(driver_run, dev):
    """final_model.pth under dataset{X}_epoch6/ is a whole-module pickle naming the reference's module path; loaded, it
    encodes and decodes bit for bit as the in-memory model; metrics.txt holds finite MAE and RMSE."""
    r = driver_run
    assert os.path.basename(os.path.normpath(r.save_dir)) == "datasetETTh1_24_epoch6"
    path = os.path.join(r.save_dir, "final_model.pth")
    assert os.path.exists(path) and os.path.exists(os.path.join(r.save_dir, "model_epoch_0.pth"))
    raw = open(path, "rb").read()
    assert b"model.pretrained.vqvae" in raw and b"t2ms_amd" not in raw
    from model.pretrained.vqvae import vqvae
    loaded = torch.load(path, map_location="cpu", weights_only=False)
    assert type(loaded) is vqvae
    loaded = loaded.to(dev)
    x = synth.make_series(5, 4, 24).to(dev)
    with torch.no_grad():
        za, ba = r.model.encoder(x)
        zb, bb = loaded.encoder(x)
        ra, aa = r.model.decoder(za, length=24)
        rb, ab = loaded.decoder(zb, length=24)
    for a, b in ((za, zb), (ba, bb), (ra, rb), (aa, ab)):
        assert torch.equal(a, b)
    lines = dict(ln.split(": ") for ln in open(os.path.join(r.save_dir, "metrics.txt")).read().strip().splitlines())
    assert set(lines) == {"MAE", "RMSE"} and all(np.isfinite(float(v)) and float(v) >= 0 for v in lines.values())


def test_decoder_backward_refuses_what_it_does_not_cover(dev):
    """A non-default LA-VAE shape: the C entry refuses it loudly, the mirror keeps the labelled torch-op path and gives finite
    gradients; a frozen decoder under no_grad saves nothing."""
    from model.pretrained.vqvae import vqvae
    from t2ms_amd import _lib as L
    v = vqvae(types.SimpleNamespace(block_hidden_size=16, num_residual_layers=2, res_hidden_size=32, embedding_dim=64)).to(dev)
    z = synth.make_latents(3, 2).to(dev).requires_grad_(True)
    rec, after = v.decoder(z, length=24)
    assert rec.requires_grad and type(after.grad_fn).__name__ != "_DecodeFnBackward"
    (rec.sum() + after.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in v.decoder.parameters())
    assert z.grad is not None and torch.isfinite(z.grad).all()
    h = v.decoder._handle(dev)
    g = L.VaeDecGrads()
    drecon = torch.zeros(2, 24, device=dev)
    rc = L.lib().t2s_vae_decode_backward(h, z.detach().data_ptr(), drecon.data_ptr(), None, C.byref(g), None, 2, 24, 30, None)
    assert rc == -1 and "unsupported" in L.lib().t2s_last_error().decode()
    # the default shape, frozen / under no_grad: today's call, no graph
    vd = _vae(dev)
    with torch.no_grad():
        r0, a0 = vd.decoder(z.detach(), length=24)
    assert r0.grad_fn is None and a0.grad_fn is None and not r0.requires_grad
    for p in vd.decoder.parameters():
        p.requires_grad = False
    r1, a1 = vd.decoder(z.detach(), length=24)
    assert r1.grad_fn is None and a1.grad_fn is None and torch.equal(r0, r1) and torch.equal(a0, a1)
    # and the C entry's range checks on the default shape
    hd = vd.decoder._handle(dev)
    for Lbad, Wbad in ((4, 30), (132, 30), (26, 30), (24, 33), (24, 0)):
        rc = L.lib().t2s_vae_decode_backward(hd, z.detach().data_ptr(), drecon.data_ptr(), None, C.byref(g), None, 2, Lbad, Wbad, None)
        assert rc == -1 and "unsupported" in L.lib().t2s_last_error().decode(), (Lbad, Wbad)


@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_backward_grows_its_row_blocks_under_the_device_lock(dev, side, monkeypatch):
    """Both backwards free / allocate their row blocks when B * L/4 or B exceeds what the handle holds (vae_grow_rows), which
    must not run inside another thread's stream capture: the mirror takes the device's lock around exactly those calls, in
    both directions.  Counted: the entries of L.device_lock during backward() alone (the forward has built the handle
    before).  Shapes: rows 4 / series 2 first, the same again, series 3 (rows 6), then rows 4 <= 6 with series 1 <= 3."""
    import gc
    from t2ms_amd import _lib as L
    gc.collect()                       # no finalizer of an earlier test's handle (destroy_locked) inside the counts
    entries, real = [0], L.device_lock

    def counting(device):
        entries[0] += 1
        return real(device)

    monkeypatch.setattr(L, "device_lock", counting)
    v = _vae(dev)
    codec = getattr(v, side)

    def backward_entries(B, Ls):
        codec.zero_grad(set_to_none=True)
        if side == "encoder":
            z, before = codec(synth.make_series(40 + B + Ls, B, Ls).to(dev))
            loss, node = z.sum() + before.sum(), z
        else:
            rec, after = codec(synth.make_latents(40 + B + Ls, B).to(dev), length=Ls)
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


def test_zero_residual_layers_take_the_torch_op_path(dev):
    """A residual stack without layers has no res_hidden; the library is told 1, which the backward entries refuse
    ("unsupported").  The mirror must therefore not choose the HIP pair for it: the labelled torch-op forwards run under
    autograd, as for every other shape the kernels do not cover, and backward() gives finite, non-zero gradients."""
    from model.pretrained.vqvae import vqvae
    torch.manual_seed(5)
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=0, res_hidden_size=256, embedding_dim=64)).to(dev)
    x = synth.make_series(77, 1, 8).to(dev)
    z, before = v.encoder(x)
    rec, after = v.decoder(z, length=8)
    assert z.requires_grad and type(z.grad_fn).__name__ != "_EncodeFnBackward"
    assert after.requires_grad and type(after.grad_fn).__name__ != "_DecodeFnBackward"
    (rec.sum() + after.sum() + before.sum()).backward()
    ps = dict(v.named_parameters())
    assert len(ps) == 14
    for n, p in ps.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
