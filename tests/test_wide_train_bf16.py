"""The bf16 mixed-precision training step of the wide-latent DiT on the GPU (Transformer(50) / Transformer(64) with
set_trainable(True).set_wide_train_bf16(True).set_train_dtype("bf16"): the HIP step of train.py --bf16 at 800 / 1024 tokens)
against fp64 torch autograd through the plain-torch restatement of the reference's network (tests/_wide_train_ref.py), and the
mytrain.py --bf16 driver.  Needs an MI355X.

Bars: those of the 480-token bf16 step (tests/test_hip_train.py::test_bf16_backward_close_to_fp32_oracle) -- per gradient
tensor relative L2 error < 1e-2 and cosine > 0.9999, prediction relative L2 < 5e-3, loss rtol 2e-3 -- over the same 48
trainable tensors.  Next to each figure the tests print what torch.autocast(bfloat16) autograd through the same restatement
deviates by on the CPU: context for profiles/wide_train_bf16_errors.md, not a bar."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _wide_train_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_REL, LOSS_RTOL, GRAD_REL, GRAD_COS = 5e-3, 2e-3, 1e-2, 0.9999
GUARD_REL = 1e-5               # a bf16 step differs from the fp32 step by more than this in some block weight


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, W, bf16=True, seed=R.WEIGHT_SEED):
    from model.denoiser.mytransformer import Transformer
    m = Transformer(W)
    m.load_state_dict(R.state_dict(W, seed=seed), strict=True)
    m.set_trainable(True)
    if bf16:
        assert m.set_wide_train_bf16(True) is m and m.set_train_dtype("bf16") is m
    return m.to(dev).train()


def _step(m, dev, x, t, text, target):
    """forward, MSE, backward on the HIP path -> (pred, loss); parameter gradients in p.grad."""
    from t2ms_amd.train import mse_loss
    pred = m(input=x.to(dev), t=t.to(dev), text_input=None if text is None else text.to(dev))
    loss = mse_loss(pred, target.to(dev))
    loss.backward()
    return pred.detach().cpu(), loss.item()


def _grads(m):
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


_AUTOCAST = {}


def _autocast_case(W, B, with_text):
    """torch.autocast(bfloat16) autograd through the restatement on the CPU: (pred, loss, {key: grad}), once per case."""
    key = (W, B, with_text)
    if key not in _AUTOCAST:
        x, t, text, target = R.batch_inputs(W, B, with_text)
        sd = {k: v.detach().clone().requires_grad_(not k.startswith(R.NOGRAD)) for k, v in R.state_dict(W).items()}
        temb = R.time_embedding(t, torch.float32)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            pred = R.forward(sd, x, t, text, temb=temb)
        loss = F.mse_loss(pred.float(), target)
        loss.backward()
        _AUTOCAST[key] = (pred.detach().float(), float(loss), {k: v.grad for k, v in sd.items() if v.grad is not None})
    return _AUTOCAST[key]


@pytest.mark.parametrize("with_text", [True, False], ids=["text", "notext"])
@pytest.mark.parametrize("W,B", [(50, 1), (50, 2), (64, 1), (64, 2)])
def test_wide_bf16_backward_close_to_fp64_autograd(dev, W, B, with_text):
    x, t, text, target, pred_ref, loss_ref, g_ref, _ = R.batch_case(W, B, with_text, torch.float64)
    ac_pred, ac_loss, ac_g = _autocast_case(W, B, with_text)
    m = _model(dev, W)
    pred, loss = _step(m, dev, x, t, text, target)
    assert tuple(pred.shape) == (B, 64, W)
    tag = f"wide_train_bf16_errors | step W{W} B{B} text={with_text}"
    print(f"{tag} | pred rel L2 {_rel(pred, pred_ref):.3e} (autocast {_rel(ac_pred, pred_ref):.3e}) | loss rel "
          f"{abs(loss - float(loss_ref)) / float(loss_ref):.3e} (autocast {abs(ac_loss - float(loss_ref)) / float(loss_ref):.3e})")
    got = _grads(m)
    checked, bad = 0, []
    worst = {"rel": ("", 0.0, 0.0), "cos": ("", 1.0, 1.0)}
    for name, p in m.named_parameters():
        if name.startswith("unpatch") or name == "pos_embed":
            assert p.grad is None, name
            continue
        ref = g_ref[name]
        assert torch.isfinite(got[name]).all(), name
        rel, cos = _rel(got[name], ref), _cos(got[name], ref)
        ac_rel, ac_cos = _rel(ac_g[name], ref), _cos(ac_g[name], ref)
        if rel > worst["rel"][1]:
            worst["rel"] = (name, rel, ac_rel)
        if cos < worst["cos"][1]:
            worst["cos"] = (name, cos, ac_cos)
        if not (rel < GRAD_REL and cos > GRAD_COS):
            bad.append((name, rel, cos))
        checked += 1
    print(f"{tag} | worst gradient rel L2 {worst['rel'][1]:.3e} (autocast {worst['rel'][2]:.3e}) {worst['rel'][0]} | lowest cosine "
          f"{worst['cos'][1]:.7f} (autocast {worst['cos'][2]:.7f}) {worst['cos'][0]}")
    assert checked == 48
    assert not bad, bad
    assert _rel(pred, pred_ref) < PRED_REL
    np.testing.assert_allclose(loss, float(loss_ref), rtol=LOSS_RTOL)
    # dispatch guard: the same handle's fp32 step gives other gradients (a run that fell back to fp32 would pass the bars)
    m.set_train_dtype("f32")
    m.zero_grad()
    pred32, _ = _step(m, dev, x, t, text, target)
    g32 = _grads(m)
    assert float((pred32.double() - pred_ref).abs().max()) < 1e-4          # (the fp32 step's own bar)
    block_w = [n for n in got if n.startswith("layers.") and n.endswith(("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight"))]
    assert len(block_w) == 16
    apart = max(_rel(got[n], g32[n]) for n in block_w)
    print(f"{tag} | bf16 step vs fp32 step, block weights: largest rel L2 {apart:.3e}")
    assert apart > GUARD_REL


def test_switching_back_gives_the_fp32_bits_and_the_old_refusals(dev):
    """set_train_dtype("f32") after a bf16 step on the same handle: the bits of a model that never left fp32.
    set_wide_train_bf16(False): the mirror's refusal is back, and the handle answers T2S_TRAIN_BF16 with the old message."""
    W, B = 50, 2
    x, t, text, target = R.batch_inputs(W, B, True)
    m = _model(dev, W)
    _step(m, dev, x, t, text, target)
    hid = m.t2s_handle_id()
    m.set_train_dtype("f32")
    m.zero_grad()
    pred_a, loss_a = _step(m, dev, x, t, text, target)
    assert m.t2s_handle_id() == hid
    ga = _grads(m)
    fresh = _model(dev, W, bf16=False)
    pred_b, loss_b = _step(fresh, dev, x, t, text, target)
    gb = _grads(fresh)
    assert torch.equal(pred_a, pred_b) and loss_a == loss_b and len(ga) == 48
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # back to bf16, then the switch off: the model is on f32, the refusal is back
    m.set_train_dtype("bf16")
    assert m.set_wide_train_bf16(False) is m and m.__dict__["_t2s_train_dtype"] == "f32"
    with pytest.raises(L.T2SError, match="train in 'f32' only"):
        m.set_train_dtype("bf16")
    m.zero_grad()
    pred_c, loss_c = _step(m, dev, x, t, text, target)
    assert torch.equal(pred_c, pred_b) and loss_c == loss_b
    with torch.cuda.device(dev):
        h = m.t2s_handle(dev, B)
        assert L.lib().t2s_dit_set_train_dtype(h, L.TRAIN_BF16) == -1
        assert L.lib().t2s_last_error() == (b"t2s_dit_set_train_dtype: a handle of latent width 50 trains in T2S_TRAIN_F32 only "
                                            b"(T2S_TRAIN_BF16 exists at width 30)")


def test_the_two_switches_in_either_order_on_a_handle(dev):
    """The C entries on a Transformer(64) handle: t2s_dit_set_wide_train_bf16 before or after t2s_dit_set_trainable, with
    `trainable` off the answer stays "latent width 30"; switching the bf16 opt-in off while on T2S_TRAIN_BF16 puts the
    handle back on T2S_TRAIN_F32 (its next forward gives the fp32 forward's bits); NULL handle; width 30 is a no-op."""
    lib = L.lib()
    from model.denoiser.mytransformer import Transformer
    m = Transformer(64)
    m.load_state_dict(R.state_dict(64), strict=True)
    m = m.to(dev)
    x = synth.make_wide_latents(1, 1, 64).to(dev)
    old_bf16 = (b"t2s_dit_set_train_dtype: a handle of latent width 64 trains in T2S_TRAIN_F32 only "
                b"(T2S_TRAIN_BF16 exists at width 30)")
    old_width = b"t2s_dit_set_train_dtype: training runs at latent width 30 only, this handle has 64"
    with torch.cuda.device(dev):
        st = L.stream_ptr(dev)
        w, keep, _ = m._weights_struct(dev)
        h = m.t2s_handle(dev, 2)
        temb = torch.zeros(1, 128, device=dev)

        def fwd():
            out = torch.full((1, 64, 64), float("nan"), device=dev)
            assert lib.t2s_dit_train_forward(h, C.byref(w), x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, st) == 0
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            return out.cpu()

        # bf16 switch first, `trainable` still off: "latent width 30", for either dtype
        assert lib.t2s_dit_set_wide_train_bf16(h, 1) == 0
        for dt in (L.TRAIN_BF16, L.TRAIN_F32):
            assert lib.t2s_dit_set_train_dtype(h, dt) == -1 and lib.t2s_last_error() == old_width
        assert lib.t2s_dit_set_trainable(h, 1) == 0
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_F32) == 0
        out32 = fwd()
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) == 0
        out16 = fwd()
        assert not torch.equal(out16, out32) and float((out16 - out32).norm() / out32.norm()) < 5e-3
        # off while on BF16: back on F32 without being told
        assert lib.t2s_dit_set_wide_train_bf16(h, 0) == 0
        assert torch.equal(fwd(), out32)
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) == -1 and lib.t2s_last_error() == old_bf16
        # the other order: trainable (already on), then the bf16 switch
        assert lib.t2s_dit_set_wide_train_bf16(h, 1) == 0 and lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) == 0
        assert torch.equal(fwd(), out16)
        # trainable off under it: the old answer
        assert lib.t2s_dit_set_trainable(h, 0) == 0
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) == -1 and lib.t2s_last_error() == old_width
        out = torch.empty(1, 64, 64, device=dev)
        assert lib.t2s_dit_train_forward(h, C.byref(w), x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, st) == -1
        assert b"latent width 30" in lib.t2s_last_error()
        assert lib.t2s_dit_set_wide_train_bf16(h, 0) == 0
        assert lib.t2s_dit_set_wide_train_bf16(None, 1) == -1 and b"t2s_dit_set_wide_train_bf16" in lib.t2s_last_error()
        m30 = Transformer(30).to(dev)
        h30 = m30.t2s_handle(dev, 1)
        assert lib.t2s_dit_set_wide_train_bf16(h30, 0) == 0 and lib.t2s_dit_set_train_dtype(h30, L.TRAIN_BF16) == 0
    del keep


def test_two_wide_bf16_steps_are_bit_equal(dev):
    x, t, text, target = R.batch_inputs(50, 2, True)
    runs = []
    for _ in range(2):
        m = _model(dev, 50)
        pred, loss = _step(m, dev, x, t, text, target)
        runs.append((pred, loss, _grads(m)))
    (pa, la, ga), (pb, lb, gb) = runs
    assert torch.equal(pa, pb) and la == lb and len(ga) == 48
    for k in ga:
        assert torch.isfinite(ga[k]).all() and torch.equal(ga[k], gb[k]), k


def test_wide_bf16_training_reduces_loss(dev):
    """Twelve AdamW steps at W 50, B 8 (tests/test_hip_train.py::test_bf16_training_reduces_loss at 800 tokens)."""
    from model.backbone.DDPM import DDPM
    from t2ms_amd.train import T2SAdamW
    m = _model(dev, 50, seed=9)
    opt = T2SAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.0)
    ddpm = DDPM(100, dev)
    x1 = synth.make_wide_latents(1, 8, 50).to(dev) * 0.5
    text = synth.make_text_embeddings(1, 8).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    losses = []
    for it in range(12):
        t = torch.randint(0, 100, (8,), generator=g).to(dev)
        eps = torch.randn(8, 64, 50, generator=g).to(dev)
        xt, _ = ddpm.q_sample(x1, t, eps)
        opt.zero_grad()
        loss = ddpm.loss(m(input=xt, t=t, text_input=text), eps)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"wide_train_bf16_errors | 12 AdamW steps W50 B8 | first three {np.mean(losses[:3]):.5f} | last three {np.mean(losses[-3:]):.5f}")
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3])


def test_mytrain_bf16_run_checkpoint_sample_and_fp32_resume(dev, tmp_path, monkeypatch, capsys):
    """mytrain.py --bf16 on synthetic deadlift clips (800 tokens): 3 steps, finite loss, every trainable tensor changed, a
    checkpoint of fp32 tensors that myinfer.py samples from and that a run WITHOUT --bf16 resumes in fp32."""
    import myinfer
    import mytrain
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "res")
    base = ["--dataset_name", "deadlift", "--random_init", "--synthetic", "8", "--batch_size", "8", "--save_path", save]
    args = mytrain.get_args(base + ["--epochs", "2", "--max_steps", "3", "--bf16"])      # (stops in epoch 0, which is checkpointed)
    mytrain.seed_everything(args.general_seed)
    losses = mytrain.train(args)
    assert "bf16 mixed precision" in capsys.readouterr().out
    assert len(losses) == 1 and np.isfinite(losses).all()
    assert args.model.__dict__["_t2s_train_dtype"] == "bf16" and args.model.__dict__["_t2s_wide_train_bf16"] is True
    path = os.path.join(save, "checkpoints", "flowmatching_DiT_deadlift_Caption_explain_no_barbell_20000", "model_0.pth")
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "loss_list", "model", "optimizer"] and ck["epoch"] == 0 and ck["loss_list"] == losses
    assert all(v.dtype == torch.float32 for v in ck["model"].values() if v.is_floating_point())
    sd0 = R.state_dict(50, seed=args.general_seed)
    changed = [k for k in sd0 if not k.startswith(("pos_embed", "unpatch.")) and not torch.equal(ck["model"][k], sd0[k])]
    assert len(changed) == 48
    assert all(torch.isfinite(ck["model"][k]).all() for k in sd0)
    assert {int(s["step"]) for s in ck["optimizer"]["state"].values()} == {3}
    vae_path = mytrain.get_args(base).pretrainedvae_path
    os.makedirs(os.path.dirname(vae_path), exist_ok=True)
    torch.save(synth.make_mvae_state_dict(args.general_seed, args.input_dim, args.block_hidden_size, args.num_residual_layers,
                                          args.res_hidden_size), vae_path)
    out = myinfer.main(["--dataset_name", "deadlift", "--checkpoint_id", "0", "--synthetic", "4", "--total_step", "3", "--save_path", save])
    assert len(out) == 1 and len(out[0]["clips"]) == 4 and np.isfinite(out[0]["mean_mse"])
    # resumed without --bf16: fp32 from the same file
    args2 = mytrain.get_args(base + ["--epochs", "2", "--checkpoint_path", path])
    losses2 = mytrain.train(args2)
    assert "Training arithmetic: fp32" in capsys.readouterr().out
    assert args2.model.__dict__.get("_t2s_train_dtype", "f32") == "f32" and "_t2s_wide_train_bf16" not in args2.model.__dict__
    assert losses2[:1] == losses and len(losses2) == 2 and np.isfinite(losses2[1])
    ck2 = torch.load(os.path.join(os.path.dirname(path), "model_1.pth"), map_location="cpu")
    assert ck2["epoch"] == 1 and {int(s["step"]) for s in ck2["optimizer"]["state"].values()} == {6}
