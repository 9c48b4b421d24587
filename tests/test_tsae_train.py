"""The TSae training kernels (csrc/t2s_tsae_train.hip) on the GPU: t2s_tsae_train_forward / _backward against fp64 autograd of
the restatement in tests/_tsae_train_ref.py on the SAME dropout masks (rebuilt on the host from the Philox rule) and the library's
own positional table; bitwise properties; t2s_tsae_update_weights; the mirror's opt-in HIP engine; the refusals; the driver.

Measured on one MI355X (worst |error| / bar per case, forward | loss rtol | worst gradient tensor): profiles/tsae_train_errors.md.
"""
import copy
import ctypes as C
import os
import subprocess
import sys
import types

import pytest
import torch

import _tsae_handle as TH
import _tsae_train_ref as TR
from t2ms_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = TH.DEV
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k(c):
    return dict(n_features=c.n_features, d_ff=c.d_ff, heads=c.heads, n_enc=c.n_enc, n_dec=c.n_dec)


def _grads_struct(c, names):
    """A t2s_tsae_grads over fresh tensors: ({name: tensor}, struct)."""
    sd = TR.state_dict(c)
    out = {n: torch.full(sd[n].shape, float("nan"), device=DEV) for n in names}
    g = L.TsaeWeights()

    def attn(dst, prefix):
        dst.in_proj_w, dst.in_proj_b = out[prefix + ".in_proj_weight"].data_ptr(), out[prefix + ".in_proj_bias"].data_ptr()
        dst.out_proj_w, dst.out_proj_b = out[prefix + ".out_proj.weight"].data_ptr(), out[prefix + ".out_proj.bias"].data_ptr()

    def wb(dst, field, name):
        setattr(dst, field + "_w", out[name + ".weight"].data_ptr())
        setattr(dst, field + "_b", out[name + ".bias"].data_ptr())

    wb(g, "value_embedding", "encoder.value_embedding"), wb(g, "embedding_ln", "encoder.embedding_ln")
    wb(g, "input_projection", "decoder.input_projection"), wb(g, "output_projection", "decoder.output_projection")
    for i in range(c.n_enc):
        p = f"encoder.transformer_encoder.layers.{i}"
        attn(g.enc[i].self_attn, p + ".self_attn")
        for n in ("linear1", "linear2", "norm1", "norm2"):
            wb(g.enc[i], n, f"{p}.{n}")
    for i in range(c.n_dec):
        p = f"decoder.transformer_decoder.layers.{i}"
        attn(g.dec[i].self_attn, p + ".self_attn"), attn(g.dec[i].multihead_attn, p + ".multihead_attn")
        for n in ("linear1", "linear2", "norm1", "norm2", "norm3"):
            wb(g.dec[i], n, f"{p}.{n}")
    return out, g


class Trainer:
    """A two-sided handle on a case's weights with the training entries as methods."""

    def __init__(self, c, sd=None):
        self.c, self.h = c, TH.Handle(_k(c), TR.state_dict(c) if sd is None else sd)
        assert self.h.rc == 0, L.lib().t2s_last_error()

    def ws(self, B, T):
        n = int(L.lib().t2s_tsae_train_workspace_bytes(self.h.ptr, B, T))
        assert n > 0, L.lib().t2s_last_error()
        return torch.empty(n, dtype=torch.uint8, device=DEV)

    def forward_rc(self, x, pred, B, T, p, seed, ws, ws_bytes=None, ptr=None):
        return L.lib().t2s_tsae_train_forward(self.h.ptr if ptr is None else ptr, x.data_ptr() if x is not None else None,
                                              pred.data_ptr() if pred is not None else None, B, T, p, seed,
                                              ws.data_ptr() if ws is not None else None, ws.numel() if ws_bytes is None else ws_bytes,
                                              L.stream_ptr(DEV))

    def forward(self, x, p, seed, ws):
        B, T, F_ = x.shape
        pred = torch.empty(B, T, F_, device=DEV)
        L.check(self.forward_rc(x, pred, B, T, p, seed, ws), "t2s_tsae_train_forward")
        return pred

    def backward_rc(self, x, d_pred, g, B, T, p, seed, ws, ws_bytes=None):
        return L.lib().t2s_tsae_train_backward(self.h.ptr, x.data_ptr() if x is not None else None,
                                               d_pred.data_ptr() if d_pred is not None else None, C.byref(g) if g is not None else None,
                                               B, T, p, seed, ws.data_ptr() if ws is not None else None,
                                               ws.numel() if ws_bytes is None else ws_bytes, L.stream_ptr(DEV))

    def backward(self, x, d_pred, p, seed, ws):
        B, T, _ = x.shape
        out, g = _grads_struct(self.c, TR.taking_part(TR.state_dict(self.c)))
        L.check(self.backward_rc(x, d_pred, g, B, T, p, seed, ws), "t2s_tsae_train_backward")
        return out

    def step(self, x, p, seed):
        """(prediction, loss, grads) with d_prediction the MSE gradient."""
        ws = self.ws(x.shape[0], x.shape[1])
        pred = self.forward(x, p, seed, ws)
        d_pred = (2.0 / pred.numel()) * (pred - x)
        grads = self.backward(x, d_pred.contiguous(), p, seed, ws)
        torch.cuda.synchronize()
        return pred, float(torch.mean((pred.double() - x.double()) ** 2)), grads


_RUNS = {}


def _run(c):
    """The case on the GPU and in fp64 on the library's own table, once: (trainer, hip (pred, loss, grads), reference)."""
    if c not in _RUNS:
        t = Trainer(c)
        hip = t.step(TR.series(c).to(DEV), c.p, TR.case_seed(c))
        ref = TR.reference(c, pe=t.h.positional(c.T).double(), key="library table")
        _RUNS[c] = (t, hip, ref)
    return _RUNS[c]


@pytest.mark.parametrize("c", TR.CASES, ids=TR.IDS)
def test_forward(c):
    t, (pred, _, _), (ref, _, _) = _run(c)
    bar = TR.FWD_BAR * max(1.0, float(ref.abs().max()))
    err = float((pred.cpu().double() - ref).abs().max())
    print(f"\ncase {c.name}: forward max|err| {err:.3e} = {err / bar:.3f} of the bar {bar:.3e}")
    assert err <= bar
    if c.p == 0.0:
        x = TR.series(c).to(DEV)
        two = t.h.decode(t.h.encode(x), x)
        err2 = float((pred - two).abs().max())
        print(f"case {c.name}: against encode + decode {err2:.3e}")
        assert err2 <= bar


@pytest.mark.parametrize("c", TR.CASES, ids=TR.IDS)
def test_backward(c):
    _, (_, loss, grads), (_, ref_loss, ref) = _run(c)
    print(f"\ncase {c.name}: loss {loss:.9f} vs fp64 {float(ref_loss):.9f} (rtol {abs(loss - float(ref_loss)) / float(ref_loss):.2e})")
    worst, worst_name = 0.0, None
    for name, g64 in ref.items():
        top = float(g64.abs().max())
        err = float((grads[name].cpu().double() - g64).abs().max())
        if top == 0.0:       # structurally zero (case D, T = 1: a softmax over one key passes no gradient to its scores, no row
            #                  reaches the shifted input projection): nothing but zeros will do
            assert c.T == 1, name
            assert err == 0.0, name
            continue
        assert top >= TR.MIN_GRAD, (name, top)
        if err / (TR.GRAD_BAR * top) > worst:
            worst, worst_name = err / (TR.GRAD_BAR * top), name
    print(f"case {c.name}: worst gradient tensor {worst_name}: {worst:.4f} of its bar ({len(ref)} tensors)")
    assert worst <= 1.0, worst_name
    assert abs(loss - float(ref_loss)) <= TR.LOSS_RTOL * float(ref_loss)


def test_repeats_bit_for_bit():
    c = TR.BY_NAME["B"]
    t, (pred, _, grads), _ = _run(c)
    pred2, _, grads2 = t.step(TR.series(c).to(DEV), c.p, TR.case_seed(c))
    assert torch.equal(pred, pred2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


def test_a_series_does_not_depend_on_the_batch():
    c = TR.BY_NAME["A"]
    t, (pred, _, _), _ = _run(c)
    x = TR.series(c).to(DEV)
    alone = t.forward(x[1:2].contiguous(), 0.0, 5, t.ws(1, c.T))
    assert torch.equal(alone[0], pred[1])


def test_the_seed_matters_only_with_dropout():
    for name, differs in (("B", True), ("A", False)):
        c = TR.BY_NAME[name]
        t, (pred, _, _), _ = _run(c)
        other = t.forward(TR.series(c).to(DEV), c.p, TR.case_seed(c) + 1, t.ws(c.B, c.T))
        assert torch.equal(pred, other) != differs


def test_update_weights_equals_a_fresh_handle():
    c = TR.BY_NAME["C"]
    sd = {k: v.clone().to(DEV) for k, v in TR.state_dict(c).items()}
    t = Trainer(c, sd)              # TH.Handle keeps `sd`'s tensors as they are on the device: t.h.keep
    x = TR.series(c).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    for k in TR.taking_part(sd):
        t.h.keep[k].add_(0.05 * torch.randn(t.h.keep[k].shape, device=DEV, generator=g))
    L.check(L.lib().t2s_tsae_update_weights(t.h.ptr, C.byref(t.h.w), L.stream_ptr(DEV)), "t2s_tsae_update_weights")
    fresh = Trainer(c, {k: v.clone() for k, v in t.h.keep.items()})
    mem_a, mem_b = t.h.encode(x), fresh.h.encode(x)
    assert torch.equal(mem_a, mem_b)
    assert torch.equal(t.h.decode(mem_a, x), fresh.h.decode(mem_b, x))
    assert torch.equal(t.forward(x, c.p, 9, t.ws(c.B, c.T)), fresh.forward(x, c.p, 9, fresh.ws(c.B, c.T)))
    bad = L.TsaeWeights.from_buffer_copy(t.h.w)
    bad.d_ff = 128
    assert L.lib().t2s_tsae_update_weights(t.h.ptr, C.byref(bad), L.stream_ptr(DEV)) != 0
    assert b"not the handle's" in L.lib().t2s_last_error()


# ---- the mirror -------------------------------------------------------------------------------------------------------------
def _model(c, p=None):
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    torch.manual_seed(3)
    m = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=c.n_features, flow_dim=64, d_ff=c.d_ff, num_heads=c.heads,
                                                          num_encoder_layers=c.n_enc, num_decoder_layers=c.n_dec))
    m.load_state_dict(TR.state_dict(c), strict=False)
    if p is not None:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = p
            elif isinstance(mod, torch.nn.MultiheadAttention):
                mod.dropout = p
    return m.to(DEV).train()


def test_mirror_three_steps_against_the_torch_engine():
    """AdamW's update u = m / (sqrt(v) + eps) moves by at most delta / (|g| + eps) when a gradient element moves by delta, and
    never by more than 2 (a sign flip of an element that is rounding noise, the in_proj K bias): three steps at rate lr put the
    parameters within 3 lr min(2, GRAD_BAR max|g| / (|g| + eps)) of each other, |g| the element's smallest gradient of the run."""
    c, lr, eps = TR.BY_NAME["B"], 1e-3, 1e-8
    x = TR.series(c).to(DEV)
    hip = _model(c, 0.0)
    ref = copy.deepcopy(hip)
    hip.set_train_engine("hip"), ref.set_train_engine("torch")
    losses, gmin, gmax = {}, {}, {}
    for name, m in (("hip", hip), ("torch", ref)):
        opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=1e-2, eps=eps)
        losses[name] = []
        for _ in range(3):
            loss, _ = m.shared_eval(x, None, opt, "train")
            losses[name].append(float(loss.detach()))
            if name == "torch":
                for k, prm in m.named_parameters():
                    if prm.grad is not None:
                        a = prm.grad.abs()
                        gmin[k] = a if k not in gmin else torch.minimum(gmin[k], a)
                        gmax[k] = max(gmax.get(k, 0.0), float(a.max()))
    assert hip.__dict__.get("_t2s_h") is not None and ref.__dict__.get("_t2s_h") is None       # the engines that ran
    print("\nlosses", losses)
    for a, b in zip(losses["hip"], losses["torch"]):
        assert abs(a - b) <= 1e-4 * abs(b)
    pr = dict(ref.named_parameters())
    worst = 0.0
    for k, prm in hip.named_parameters():
        if k not in gmin:
            continue
        tol = 3 * lr * torch.clamp(TR.GRAD_BAR * gmax[k] / (gmin[k] + eps), max=2.0)
        ratio = float(((prm.detach() - pr[k].detach()).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, k
    print(f"parameters after three steps: worst {worst:.4f} of the bound")


def test_mirror_keeps_its_handle_and_refreshes_it():
    c = TR.BY_NAME["C"]
    m = _model(c, 0.0)
    m.set_train_engine("hip")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    x = TR.series(c).to(DEV)
    m.shared_eval(x, None, opt, "train")
    uid = m.__dict__["_t2s_h"].uid
    _, recon = m.shared_eval(x, None, opt, "train")          # after opt.step(): t2s_tsae_update_weights, the same handle
    assert m.__dict__["_t2s_h"].uid == uid
    fresh = Trainer(c, {k: v.detach().clone() for k, v in m.state_dict().items()})
    # `recon` was computed BEFORE the second optimizer step: recompute on the parameters as they are now, both ways
    pred = m._train_forward_hip(x).detach()
    assert m.__dict__["_t2s_h"].uid == uid
    assert torch.equal(pred, fresh.forward(x, 0.0, 1, fresh.ws(c.B, c.T)))


def test_mirror_dropout_loss_is_the_restatements():
    c = TR.BY_NAME["B"]
    m = _model(c)
    m.set_train_engine("hip")
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items() if not k.startswith("condition_fusion.")}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    x = TR.series(c)
    torch.manual_seed(77)
    loss, _ = m.shared_eval(x.to(DEV), None, opt, "train")
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    masks = TR.build_masks(seed, 0.1, c.B, c.d_ff, c.n_enc, c.n_dec, c.heads, c.T)
    _, ref_loss, _ = TR.loss_and_grads(sd64, x, c.heads, masks, 0.1)
    loss = float(loss.detach())
    print(f"\nhip step loss {loss:.8f}, restatement on the rebuilt masks {float(ref_loss):.8f}")
    assert abs(loss - float(ref_loss)) <= TR.LOSS_RTOL * float(ref_loss)


def test_mirror_uncovered_length_takes_torch_ops():
    c = TR.BY_NAME["C"]
    m = _model(c)
    m.set_train_engine("hip")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    x = torch.rand(1, 193, c.n_features, device=DEV)
    loss, recon = m.shared_eval(x, None, opt, "train")
    assert torch.isfinite(loss) and recon.shape == x.shape and m.__dict__.get("_t2s_h") is None


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = TR.BY_NAME["C"]
    t = Trainer(c)
    x = TR.series(c).to(DEV)
    B, T = c.B, c.T
    ws = t.ws(B, T)
    pred = torch.full((B, T, c.n_features), 7.0, device=DEV)
    names = TR.taking_part(TR.state_dict(c))
    out, g = _grads_struct(c, names)
    d_pred = torch.zeros_like(pred)

    def refused(rc, text):
        assert rc != 0 and text in L.lib().t2s_last_error().decode(), L.lib().t2s_last_error()

    big = t.ws(B, 192)
    for bad_T in (0, 193):
        refused(t.forward_rc(x, pred, B, bad_T, 0.1, 1, big), f"T={bad_T}")
        refused(t.backward_rc(x, d_pred, g, B, bad_T, 0.1, 1, big), f"T={bad_T}")
    for bad_B in (0, 65536):
        refused(t.forward_rc(x, pred, bad_B, T, 0.1, 1, ws), f"B={bad_B}")
        refused(t.backward_rc(x, d_pred, g, bad_B, T, 0.1, 1, ws), f"B={bad_B}")
    for bad_p in (-0.1, 1.0, float("nan")):
        refused(t.forward_rc(x, pred, B, T, bad_p, 1, ws), "p_drop")
        refused(t.backward_rc(x, d_pred, g, B, T, bad_p, 1, ws), "p_drop")
    refused(t.forward_rc(None, pred, B, T, 0.1, 1, ws), "NULL")
    refused(t.forward_rc(x, None, B, T, 0.1, 1, ws), "NULL")
    refused(t.forward_rc(x, pred, B, T, 0.1, 1, None, ws_bytes=ws.numel()), "workspace is NULL")
    refused(t.forward_rc(x, pred, B, T, 0.1, 1, ws, ptr=C.c_void_p()), "handle is NULL")
    refused(t.backward_rc(None, d_pred, g, B, T, 0.1, 1, ws), "NULL")
    refused(t.backward_rc(x, None, g, B, T, 0.1, 1, ws), "NULL")
    refused(t.backward_rc(x, d_pred, None, B, T, 0.1, 1, ws), "NULL")
    refused(t.forward_rc(x, pred, B, T, 0.1, 1, ws, ws_bytes=ws.numel() - 1), "too small")
    refused(t.backward_rc(x, d_pred, g, B, T, 0.1, 1, ws, ws_bytes=ws.numel() - 1), "too small")
    hole = L.TsaeWeights.from_buffer_copy(g)
    hole.dec[0].multihead_attn.in_proj_b = None
    refused(t.backward_rc(x, d_pred, hole, B, T, 0.1, 1, ws), "gradient pointer is NULL")
    for one_sided in (TH.Handle(_k(c), TR.state_dict(c), dec=False), TH.Handle(_k(c), TR.state_dict(c), enc=False)):
        refused(t.forward_rc(x, pred, B, T, 0.1, 1, ws, ptr=one_sided.ptr), "two-sided")
        assert L.lib().t2s_tsae_train_workspace_bytes(one_sided.ptr, B, T) == 0
    assert L.lib().t2s_tsae_train_workspace_bytes(t.h.ptr, B, 193) == 0
    torch.cuda.synchronize()
    assert float(pred.min()) == 7.0 == float(pred.max())                   # nothing was launched
    assert all(bool(torch.isnan(v).all()) for v in out.values())


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def test_driver_trains_and_saves(tmp_path):
    model_flags = ["--input_dim", "4", "--flow_dim", "64", "--d_ff", "64", "--num_encoder_layers", "1", "--num_decoder_layers", "1",
                   "--num_heads", "8"]
    cmd = [sys.executable, os.path.join(REPO, "pretrain_tsae.py"), "--synthetic", "8", "--split_base_num", "12", "--pretrained_epc", "6",
           "--train_engine", "hip", "--batch_size", "4", "--dataset_name", "synth", "--save_path", str(tmp_path)] + model_flags
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    losses = [float(line.split("loss")[1].split()[0]) for line in run.stdout.splitlines() if line.startswith("epoch") and "loss" in line]
    assert losses and all(l == l and abs(l) < float("inf") for l in losses), run.stdout
    assert "train engine: hip" in run.stdout
    path = tmp_path / "12_synth_epoch6" / "final_model.pth"
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert "decoder.output_projection.weight" in sd
    rec = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tsae_reconstruct.py"), "--state_dict", str(path), "--synthetic", "2",
                          "--out", str(tmp_path / "rec")] + model_flags, capture_output=True, text=True, timeout=300)
    assert rec.returncode == 0 and '"finite": true' in rec.stdout, rec.stdout + rec.stderr
