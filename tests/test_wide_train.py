"""Training the wide-latent DiT on the GPU (Transformer(50) / Transformer(64) with set_trainable(True): the fp32 HIP step at
800 / 1024 tokens) against fp64 torch autograd through the plain-torch restatement of the reference's network
(tests/_wide_train_ref.py, anchored to the reference's own outputs by tests/test_wide_train_host.py), and the mytrain.py
driver.  Needs an MI355X.

Bars: those of tests/test_hip_train.py -- pred within 1e-4, loss rtol 1e-5, each of the 48 gradient tensors within 2e-4 of
its absmax + 1e-9.  fp32 autograd through the restatement deviates from fp64 by at most 1.4e-6 of a tensor's absmax at these
widths (tests/test_wide_train_host.py, profiles/wide_train_errors.md): far below a quarter of 2e-4, so the bar stands."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _wide_train_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_TOL, LOSS_RTOL, GRAD_REL, GRAD_ABS = 1e-4, 1e-5, 2e-4, 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, W, trainable=True):
    from model.denoiser.mytransformer import Transformer
    m = Transformer(W)
    m.load_state_dict(R.state_dict(W), strict=True)
    if trainable:
        assert m.set_trainable(True) is m
    return m.to(dev).train()


def _step(m, dev, x, t, text, target, input_grad=False):
    """forward, MSE, backward on the HIP path -> (pred, loss, input gradient or None); parameter gradients in p.grad."""
    from t2ms_amd.train import mse_loss
    xin = x.to(dev).requires_grad_(input_grad)
    pred = m(input=xin, t=t.to(dev), text_input=None if text is None else text.to(dev))
    loss = mse_loss(pred, target.to(dev))
    loss.backward()
    return pred.detach().cpu(), loss.item(), (xin.grad.cpu() if input_grad else None)


def _check(m, dev, W, B, with_text, input_grad=False):
    x, t, text, target, pred_ref, loss_ref, g_ref, dx_ref = R.batch_case(W, B, with_text, torch.float64, input_grad)
    pred, loss, dx = _step(m, dev, x, t, text, target, input_grad)
    assert tuple(pred.shape) == (B, 64, W)
    e_pred = float((pred.double() - pred_ref).abs().max())
    worst, checked = 0.0, 0
    for name, p in m.named_parameters():
        if name.startswith("unpatch") or name == "pos_embed":
            assert p.grad is None, name
            continue
        ref = g_ref[name]
        scale = float(ref.abs().max()) + 1e-12
        err = float((p.grad.detach().cpu().double() - ref).abs().max())
        worst = max(worst, err / scale)
        assert err < GRAD_REL * scale + GRAD_ABS, (name, err, scale)
        checked += 1
    print(f"wide_train_errors | HIP vs fp64 autograd | W{W} B{B} text={with_text} | pred {e_pred:.3e} | loss rel "
          f"{abs(loss - float(loss_ref)) / float(loss_ref):.3e} | worst gradient tensor {worst:.3e} of absmax")
    assert checked == 48
    assert e_pred < PRED_TOL
    np.testing.assert_allclose(loss, float(loss_ref), rtol=LOSS_RTOL)
    if input_grad:
        err = float((dx.double() - dx_ref).abs().max())
        print(f"wide_train_errors | HIP vs fp64 autograd | W{W} B{B} | dx {err / float(dx_ref.abs().max()):.3e} of absmax")
        assert tuple(dx.shape) == (B, 64, W)
        assert err < GRAD_REL * float(dx_ref.abs().max()) + GRAD_ABS


# B = 1: a one-row adaLN weight gradient, a single patchify group; B = 5: a partial second patchify group, partial tail
# workgroups (tests/test_hip_train.py names them).  W 50, B 3: 2,400 rows, a partial 64-row GEMM tile, 25 key blocks.
@pytest.mark.parametrize("with_text", [True, False], ids=["text", "notext"])
@pytest.mark.parametrize("W,B", [(50, 3), (64, 1), (64, 5)])
def test_wide_backward_matches_fp64_autograd(dev, W, B, with_text):
    _check(_model(dev, W), dev, W, B, with_text)


def test_wide_input_gradient_matches_fp64_autograd(dev):
    _check(_model(dev, 64), dev, 64, 2, True, input_grad=True)


def test_wide_backward_when_the_batch_shrinks_and_grows(dev):
    """B = 5, then 1, then 3 on ONE model: the workspace laid out for the larger batch serves the smaller ones."""
    m = _model(dev, 64)
    for B in (5, 1, 3):
        m.zero_grad()
        _check(m, dev, 64, B, True)


def _grad_bits(m):
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_two_wide_backward_runs_are_bit_equal(dev):
    x, t, text, target = R.batch_inputs(50, 3, True)
    runs = []
    for _ in range(2):
        m = _model(dev, 50)
        pred, loss, dx = _step(m, dev, x, t, text, target, input_grad=True)
        runs.append((pred, loss, dx, _grad_bits(m)))
    (pa, la, da, ga), (pb, lb, db, gb) = runs
    assert torch.equal(pa, pb) and la == lb and torch.equal(da, db) and len(ga) == 48
    for k in ga:
        assert torch.isfinite(ga[k]).all() and torch.equal(ga[k], gb[k]), k


def test_the_switch_changes_nothing_at_width_30(dev):
    x, t, text, target = synth.make_latents(71, 3), torch.tensor([5, 50, 99]), synth.make_text_embeddings(71, 3), synth.make_latents(72, 3)
    out = []
    for on in (False, True):
        m = _model(dev, 30, trainable=on)
        pred, loss, _ = _step(m, dev, x, t, text, target)
        out.append((pred, loss, _grad_bits(m)))
    (pa, la, ga), (pb, lb, gb) = out
    assert torch.equal(pa, pb) and la == lb and len(ga) == 48
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def _refused(rc, *words):
    msg = L.lib().t2s_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def test_wide_handles_refuse_without_the_switch_and_refuse_bf16_with_it(dev):
    """The C entries called directly on a Transformer(64) handle: without t2s_dit_set_trainable every training entry answers
    what it always did ("latent width 30"); with it T2S_TRAIN_F32 is taken and T2S_TRAIN_BF16 refused; switching it off
    restores the refusals.  The mirror: set_train_dtype("bf16") raises, a model without set_trainable raises under grad."""
    lib = L.lib()
    m = _model(dev, 64, trainable=False)
    x = synth.make_wide_latents(1, 1, 64).to(dev)
    with torch.cuda.device(dev):
        st = L.stream_ptr(dev)
        w, keep, _ = m._weights_struct(dev)
        h = m.t2s_handle(dev, 2)
        temb, out = torch.zeros(1, 128, device=dev), torch.empty(1, 64, 64, device=dev)

        def all_refuse():
            _refused(lib.t2s_dit_set_train_dtype(h, L.TRAIN_F32), b"latent width 30")
            _refused(lib.t2s_dit_train_forward(h, C.byref(w), x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, st), b"latent width 30")
            _refused(lib.t2s_dit_train_backward(h, out.data_ptr(), C.byref(L.DitGrads()), 1, st), b"latent width 30")
            _refused(lib.t2s_dit_train_input_grad(h, out.data_ptr(), 1, st), b"latent width 30")

        all_refuse()
        assert lib.t2s_dit_set_trainable(h, 1) == 0
        _refused(lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16), b"T2S_TRAIN_F32 only", b"64")
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_F32) == 0
        assert lib.t2s_dit_train_forward(h, C.byref(w), x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, st) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert lib.t2s_dit_set_trainable(h, 0) == 0
        all_refuse()
        assert lib.t2s_dit_set_trainable(None, 1) == -1
    with pytest.raises(L.T2SError, match="train in 'f32' only"):
        m.set_train_dtype("bf16")
    with pytest.raises(L.T2SError, match="training runs at dim 30"):
        m(input=x.requires_grad_(True), t=torch.zeros(1, device=dev), text_input=None)
    del keep


# ------------------------------------------------------------------------------------------------ the driver
def test_mytrain_synthetic_run_checkpoint_sample_and_resume(dev, tmp_path, monkeypatch):
    """mytrain.py on synthetic deadlift clips (800 tokens): 2 epochs x 3 length groups = 6 steps, finite losses, changed
    parameters, model_1.pth with the reference's keys; myinfer.py samples from that checkpoint; --checkpoint_path resumes at
    epoch 2 with the optimiser's step counts carried on."""
    import myinfer
    import mytrain
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "res")
    base = ["--dataset_name", "deadlift", "--random_init", "--synthetic", "8", "--batch_size", "8", "--save_path", save]
    args = mytrain.get_args(base + ["--epochs", "2", "--max_steps", "6"])
    mytrain.seed_everything(args.general_seed)
    losses = mytrain.train(args)
    assert len(losses) == 2 and np.isfinite(losses).all()
    path = os.path.join(save, "checkpoints", "flowmatching_DiT_deadlift_Caption_explain_no_barbell_20000", "model_1.pth")
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "loss_list", "model", "optimizer"] and ck["epoch"] == 1 and ck["loss_list"] == losses
    sd0 = R.state_dict(50, seed=args.general_seed)
    changed = [k for k in sd0 if not k.startswith(("pos_embed", "unpatch.")) and not torch.equal(ck["model"][k], sd0[k])]
    assert len(changed) == 48
    assert any(k.startswith("encoder.") for k in ck["model"])
    steps = {int(s["step"]) for s in ck["optimizer"]["state"].values()}
    assert steps == {6}
    # myinfer.py from that checkpoint (the codec from the path the drivers share)
    vae_path = mytrain.get_args(base).pretrainedvae_path
    os.makedirs(os.path.dirname(vae_path), exist_ok=True)
    torch.save(synth.make_mvae_state_dict(args.general_seed, args.input_dim, args.block_hidden_size, args.num_residual_layers,
                                          args.res_hidden_size), vae_path)
    out = myinfer.main(["--dataset_name", "deadlift", "--checkpoint_id", "1", "--synthetic", "4", "--total_step", "3", "--save_path", save])
    assert len(out) == 1 and len(out[0]["clips"]) == 4 and np.isfinite(out[0]["mean_mse"])
    # resume
    args3 = mytrain.get_args(base + ["--epochs", "3", "--checkpoint_path", path])
    losses3 = mytrain.train(args3)
    assert losses3[:2] == losses and len(losses3) == 3 and np.isfinite(losses3[2])
    ck3 = torch.load(os.path.join(os.path.dirname(path), "model_2.pth"), map_location="cpu")
    assert ck3["epoch"] == 2 and {int(s["step"]) for s in ck3["optimizer"]["state"].values()} == {9}


def test_mytrain_first_step_equals_the_restatement(dev, tmp_path, monkeypatch):
    """mytrain.py on tests/golden/motion_ds/benchpress (1024 tokens): the loss of the first optimisation step is what the
    restatement gives in fp64 on the x_t, t draws, CFG coin and target the driver used (captured at the model's forward and
    at the loss)."""
    import mytrain
    from model.denoiser.mytransformer import Transformer
    monkeypatch.chdir(tmp_path)
    seen = {}
    fwd, mse = Transformer.forward, mytrain.mse_loss

    def spy_forward(self, input, t, text_input):
        if "x_t" not in seen and torch.is_grad_enabled():
            seen.update(x_t=input.detach().cpu(), t=t.detach().cpu(), text=None if text_input is None else text_input.detach().cpu(),
                        sd={k: v.detach().cpu().clone() for k, v in self.state_dict().items() if not k.startswith("encoder.")})
        return fwd(self, input, t, text_input)

    def spy_mse(a, b):
        out = mse(a, b)
        if "target" not in seen:
            seen.update(target=b.detach().cpu(), loss=float(out.detach()))
        return out

    monkeypatch.setattr(Transformer, "forward", spy_forward)
    monkeypatch.setattr(mytrain, "mse_loss", spy_mse)
    losses = mytrain.main(["--dataset_root", os.path.join(REPO, "tests", "golden", "motion_ds"), "--dataset_name", "benchpress",
                           "--random_init", "--epochs", "1", "--batch_size", "8", "--save_path", str(tmp_path / "res")])
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert tuple(seen["x_t"].shape[1:]) == (64, 64) and seen["x_t"].shape[0] >= 1
    temb = R.time_embedding(seen["t"], torch.float32).double()
    sd = {k: v.double() for k, v in seen["sd"].items()}
    pred = R.forward(sd, seen["x_t"].double(), seen["t"], None if seen["text"] is None else seen["text"].double(), temb=temb)
    want = float(torch.nn.functional.mse_loss(pred, seen["target"].double()))
    print(f"wide_train_errors | mytrain.py first step | loss {seen['loss']:.8f} | restatement {want:.8f} | rel "
          f"{abs(seen['loss'] - want) / want:.3e} | text dropped: {seen['text'] is None}")
    np.testing.assert_allclose(seen["loss"], want, rtol=1e-5)


@pytest.mark.parametrize("backbone,frozen", [("flowmatching", False), ("ddpm", True)], ids=["flow-encoder-trains", "ddpm-frozen"])
def test_mytrain_backbones_and_the_unfrozen_encoder(dev, tmp_path, monkeypatch, backbone, frozen):
    """`--usepretrainedvae ""` trains the codec's encoder through the denoiser's input gradient (every encoder tensor moves,
    the decoder is not part of the model); the frozen default leaves it bit for bit; both backbones give finite losses."""
    import mytrain
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset_name", "deadlift", "--random_init", "--synthetic", "4", "--batch_size", "4", "--epochs", "1", "--backbone", backbone,
            "--save_path", str(tmp_path / "res")] + ([] if frozen else ["--usepretrainedvae", ""])
    args = mytrain.get_args(argv)
    mytrain.seed_everything(args.general_seed)
    losses = mytrain.train(args)
    assert len(losses) == 1 and np.isfinite(losses[0])
    vsd = synth.make_mvae_state_dict(args.general_seed, args.input_dim, args.block_hidden_size, args.num_residual_layers, args.res_hidden_size)
    enc = {k: v.detach().cpu() for k, v in args.model.state_dict().items() if k.startswith("encoder.")}
    assert enc and all(torch.isfinite(v).all() for v in enc.values())
    moved = [k for k, v in enc.items() if not torch.equal(v, vsd[k])]
    if frozen:
        assert moved == []
    else:       # first and last layer certainly, and most of what lies between
        assert "encoder._conv_1.weight" in moved and "encoder._pre_vq_conv.weight" in moved and len(moved) > len(enc) // 2, moved
