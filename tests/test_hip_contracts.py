"""Contracts of the C ABI and of the class-API mirror that round 5 closed at their cause:
sizes behind the raw weight pointers, the handle-free time embedding, the stateless MSE reduction, and the limits of the
class-API pairing (torch.inference_mode(), writes torch cannot see).  Needs a real MI355X (`pytest -m gpu`)."""
import os
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _model(dev, seed=31337, gain=0.7):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(seed, gain=gain), strict=True)
    return m.to(dev).eval()


# ------------------------------------------------------------------------------------------------ sizes behind raw pointers
def test_undersized_weight_is_an_error_code_not_a_fault(dev):
    """include/t2s.h t2s_dit_weights_check: the ABI carries no sizes, so an undersized tensor must come back as
    T2S_E_INVALID naming the state-dict key -- by the caller's own float count, and (what t2s_dit_create / _update_weights
    check by themselves) by the extent of the device allocation the pointer lies in.  Round 4's fault was exactly this: a
    480 x 128 dummy behind the (768,128) adaLN matrix."""
    m = _model(dev)
    w, keep, _ = m._weights_struct(dev)
    lib = L.lib()
    counts = [t.numel() for t in keep[:9]] + [64] + [t.numel() for t in keep[9:]]
    arr = (C.c_uint64 * L.DIT_N_TENSORS)(*counts)
    assert lib.t2s_dit_weights_check(C.byref(w), arr, L.DIT_N_TENSORS) == 0
    # (1) the caller's count says the adaLN matrix of block 2 holds 480 x 128 floats
    i_ada = 10 + 10 * 2 + 8
    bad = list(counts)
    bad[i_ada] = 480 * 128
    rc = lib.t2s_dit_weights_check(C.byref(w), (C.c_uint64 * L.DIT_N_TENSORS)(*bad), L.DIT_N_TENSORS)
    msg = lib.t2s_last_error().decode()
    assert rc == -1 and "layers.2.adaLN_modulation.1.weight" in msg and "98304" in msg, (rc, msg)
    assert lib.t2s_dit_weights_check(C.byref(w), arr, 49) == -1                  # wrong table length
    # (2) no counts at all: a pointer whose ALLOCATION ends too early.  A private hipMalloc of exactly 480 x 128 floats
    # (torch's caching allocator would hide the end of a small tensor inside a 2 MB segment -- the reason round 4's fault
    # came and went).
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), 480 * 128 * 4) == 0
    try:
        w2 = L.DitWeights.from_buffer_copy(w)
        w2.blk[2].ada_w = small.value
        rc = lib.t2s_dit_weights_check(C.byref(w2), None, 0)
        msg = lib.t2s_last_error().decode()
        assert rc == -1 and "layers.2.adaLN_modulation.1.weight" in msg and "allocation ends" in msg, (rc, msg)
        out = C.c_void_p()
        assert lib.t2s_dit_create(C.byref(w2), 2, C.byref(out)) == -1 and not out.value       # refused before any kernel ran
        h = m.t2s_handle(dev, 2)
        assert lib.t2s_dit_update_weights(h, C.byref(w2), None) == -1
        w2.blk[2].ada_w = None
        assert lib.t2s_dit_weights_check(C.byref(w2), None, 0) == -1 and "is NULL" in lib.t2s_last_error().decode()
    finally:
        hip.hipFree(small)
    torch.cuda.synchronize()
    # the handle still works
    x = synth.make_latents(1, 2).to(dev)
    t = torch.tensor([3, 4], device=dev)
    with torch.no_grad():
        assert float((m(input=x, t=t, text_input=None).cpu() - O.dit_forward(synth.make_dit_state_dict(31337, gain=0.7), x.cpu(), t.cpu(), None)).abs().max()) < 1e-4


def test_refused_handle_growth_leaves_no_freed_handle_behind(dev):
    """Growing the handle frees the old one before it builds the new one (_handle.HandleOwner._owned_handle).  A build the
    library refuses -- max_seqs > 65536, before any allocation -- must leave the model without a handle, not with the freed
    one: the next forward builds a fresh handle and computes the same bits."""
    m = _model(dev)
    m.t2s_handle(dev, 4)
    x, t = synth.make_latents(1, 2).to(dev), torch.tensor([3, 4], device=dev)
    text = synth.make_text_embeddings(1, 2).to(dev)
    with torch.no_grad():
        want = m(input=x, t=t, text_input=text).clone()
    uid = m.t2s_handle_id()
    assert uid is not None and m.__dict__["_t2s_h"].max_seqs == 4
    with pytest.raises(L.T2SError, match="max_seqs=70000 out of range"):
        m.t2s_handle(dev, 70000)
    assert m.t2s_handle_id() is None and "_t2s_h" not in m.__dict__ and "_t2s_stamp" not in m.__dict__
    with torch.no_grad():
        got = m(input=x, t=t, text_input=text)
    assert torch.equal(got, want)
    assert m.t2s_handle_id() not in (None, uid)


def test_vae_weights_extent_is_checked_too(dev):
    """t2s_vae_create / _update_weights derive every tensor's size from the hyper-parameters in the struct: a tensor whose
    device allocation ends before that many floats is T2S_E_INVALID, not an out-of-bounds copy."""
    import types
    from model.pretrained.vqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64)).to(dev)
    w, keep = v.encoder._weights_struct()
    lib = L.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), 1024) == 0
    try:
        good = C.c_void_p()
        assert lib.t2s_vae_create(C.byref(w), C.byref(good)) == 0
        w2 = L.VaeWeights.from_buffer_copy(w)
        w2.enc_conv3_w = small.value                      # (128,128,3) floats expected
        out = C.c_void_p()
        assert lib.t2s_vae_create(C.byref(w2), C.byref(out)) == -1 and not out.value
        assert "allocation ends" in lib.t2s_last_error().decode()
        assert lib.t2s_vae_update_weights(good, C.byref(w2), None) == -1
        w3 = L.VaeWeights.from_buffer_copy(w)
        w3.hidden = 64                                    # hyper-parameters that are not the handle's
        assert lib.t2s_vae_update_weights(good, C.byref(w3), None) == -1
        assert lib.t2s_vae_update_weights(good, C.byref(w), None) == 0
        lib.t2s_vae_destroy(good)
    finally:
        torch.cuda.synchronize()
        hip.hipFree(small)
    del keep


def test_mirror_refuses_an_undersized_parameter(dev):
    """The mirror hands every parameter's numel() over with the pointers: a parameter re-assigned to a smaller tensor is a
    T2SError with its state-dict key, before anything is packed."""
    m = _model(dev)
    m.layers[1].mlp.fc1.weight = torch.nn.Parameter(torch.zeros(128, 128, device=dev))      # (256,128) expected
    with pytest.raises(L.T2SError, match=r"layers\.1\.mlp\.fc1\.weight holds 16384 floats"):
        m.t2s_handle(dev, 2)


def test_time_embedding_needs_no_handle(dev, golden_dir):
    """t2s_time_embedding_freqs: the module TimeEmbedding is parameter-free (transformer.py:25-40) -- no scratch t2s_dit with
    dummy weights behind it any more.  Same bits as the handle's entry, golden values of the reference."""
    import os
    from model.denoiser.transformer import TimeEmbedding
    g = np.load(os.path.join(golden_dir, "time_emb.npz"))
    te = TimeEmbedding(128)
    assert float((te(torch.from_numpy(g["t_long"]).to(dev)).cpu() - torch.from_numpy(g["emb_long"])).abs().max()) < 1e-5
    assert float((te(torch.from_numpy(g["t_float"]).to(dev)).cpu() - torch.from_numpy(g["emb_float"])).abs().max()) < 1e-5
    m = _model(dev)
    t = torch.arange(1000, device=dev).float()
    via_handle = torch.empty(1000, 128, device=dev)
    L.check(L.lib().t2s_time_embedding(m.t2s_handle(dev, 2), t.data_ptr(), via_handle.data_ptr(), 1000, L.stream_ptr(dev)))
    assert torch.equal(te(t), via_handle)
    import model.denoiser.transformer as T
    assert not hasattr(T, "_scratch_handle")


# ------------------------------------------------------------------------------------------------ stateless MSE
def test_mse_is_stateless_two_streams_and_two_threads(dev):
    """t2s_mse_ws keeps its partial sums in the CALLER's scratch (until round 5: one __device__ array per device, so two
    overlapping calls raced silently).  Many calls in flight on two streams from two threads, each with its own scratch,
    all give the single-call bits; t2s_mse (library-lent scratch per stream) gives the same bits; both equal the oracle."""
    from t2ms_amd.train import mse_loss
    rs = np.random.RandomState(5)
    sizes = (1152 * 1920, 4 * 1920 + 3, 7)
    pairs = [(torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev), torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev))
             for n in sizes]
    single = [mse_loss(a, b).clone() for a, b in pairs]
    torch.cuda.synchronize()
    for (a, b), s in zip(pairs, single):
        ref = float(O.mse_loss(a.cpu(), b.cpu()))
        assert abs(float(s) - ref) <= 2e-6 * max(1.0, abs(ref))
        lent = torch.empty((), device=dev)
        L.check(L.lib().t2s_mse(a.data_ptr(), b.data_ptr(), lent.data_ptr(), a.numel(), L.stream_ptr(dev)))
        assert torch.equal(lent, s)
    results, errors = {}, []

    def worker(k):
        try:
            st = torch.cuda.Stream(dev)
            outs = []
            with torch.cuda.stream(st):
                for rep in range(40):
                    a, b = pairs[(rep + k) % len(pairs)]
                    outs.append(((rep + k) % len(pairs), mse_loss(a, b)))
            st.synchronize()
            results[k] = outs
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for k in range(2):
        for i, out in results[k]:
            assert torch.equal(out, single[i]), (k, i)


# ------------------------------------------------------------------------------------------------ paired evaluation entries
def test_eval_entries_refuse_bad_arguments_with_their_name(dev):
    """t2s_eval_mse_wape / _mrr / _ed / _crps / _dtw check their arguments before any launch: a NULL array or an empty
    extent is T2S_E_INVALID with a message that names the entry, and the outputs are not written (the full table of
    refusals is tests/test_eval_paired.py's)."""
    lib, st = L.lib(), L.stream_ptr(dev)
    x = torch.rand(2, 8, 2, device=dev)
    out = torch.full((8,), -7.0, device=dev)
    p, o = x.data_ptr(), out.data_ptr()
    calls = {"t2s_eval_mse_wape": (lambda a, n: lib.t2s_eval_mse_wape(a, p, o, o + 16, n, 16, st)),
             "t2s_eval_mrr": (lambda a, n: lib.t2s_eval_mrr(a, p, o, o + 8, o + 16, n, 16, 1, 0.5, st)),
             "t2s_eval_ed": (lambda a, n: lib.t2s_eval_ed(a, p, o, o + 16, n, 8, 2, st)),
             "t2s_eval_crps": (lambda a, n: lib.t2s_eval_crps(a, p, o, o + 16, n, 8, 2, 1, st)),
             "t2s_eval_dtw": (lambda a, n: lib.t2s_eval_dtw(a, p, o, o + 16, n, 8, 2, st))}
    for name, call in calls.items():
        for a, n in ((None, 2), (p, 0), (p, -1)):
            assert call(a, n) == -1 and lib.t2s_last_error().decode().startswith(name + ":"), (name, a, n)
    assert lib.t2s_eval_dtw(p, p, o, o + 16, 1, 4097, 1, st) == -1 and "4096" in lib.t2s_last_error().decode()
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all()


# ------------------------------------------------------------------------------------------------ class-API pairing limits
def _ref_loop(m, x0, emb, steps, cfg, pairing):
    m.set_pairing(pairing)
    x, outs = x0.clone(), []
    for j in range(steps):
        t = torch.full((x.shape[0],), 9 - j, dtype=torch.long, device=x.device)
        u = m(input=x, t=t, text_input=None)
        c = m(input=x, t=t, text_input=emb)
        outs.append((u, c))
        x = x + 0.1 * (u + cfg * (c - u))
    return outs


def test_class_api_loop_under_inference_mode(dev):
    """tensors created under torch.inference_mode() have no version counter (`._version` raises), and
    the pairing logic read it on every call.  The reference-style loop under inference_mode now runs as plain forwards
    (nothing to speculate on) and gives the no_grad loop's bits."""
    m = _model(dev)
    x0, emb = synth.make_latents(9, 3).to(dev), synth.make_text_embeddings(3, 3).to(dev)
    with torch.no_grad():
        want = _ref_loop(m, x0, emb, 4, 2.0, pairing=True)
    with torch.inference_mode():
        xi, ei = x0.clone(), emb.clone()            # inference tensors
        assert xi.is_inference()
        got = _ref_loop(m, xi, ei, 4, 2.0, pairing=True)
        assert m.__dict__["_t2s_pair"]["stash"] is None and not m.__dict__["_t2s_pair"]["armed"]
    for (u, c), (gu, gc) in zip(want, got):
        assert torch.equal(u, gu) and torch.equal(c, gc)
    # a model BUILT under inference_mode (parameters without version counters) re-packs every call instead of caching
    with torch.inference_mode():
        mi = _model(dev)
        got = _ref_loop(mi, x0.clone(), emb.clone(), 2, 2.0, pairing=True)
    for (u, c), (gu, gc) in zip(want, got):
        assert torch.equal(u, gu) and torch.equal(c, gc)


def test_raw_pointer_write_between_the_pair_needs_pairing_off(dev):
    """the pairing is speculation on tensor IDENTITY; a write through a raw pointer (here this
    library's own in-place t2s_rf_step, called through ctypes on x_t between the text-free and the conditional call) does not
    bump torch's version counter.  With set_pairing(False) -- or T2S_NO_PAIRING=1 -- every call is a plain forward: the
    conditional output is computed from the UPDATED x_t, bit for bit what a fresh model gives and within 1e-4 of the oracle.
    (With pairing on, the same sequence hands out the stale half: shown here so the documented limit is a tested fact.)"""
    sd = synth.make_dit_state_dict(31337, gain=0.7)
    m, fresh = _model(dev), _model(dev)
    fresh.set_pairing(False)
    B = 4
    emb = synth.make_text_embeddings(3, B).to(dev)
    t = torch.full((B,), 5, dtype=torch.long, device=dev)
    v = synth.make_latents(4, B).to(dev)

    def raw_update(x):          # x <- x + v * 0.25 through the C ABI: torch sees no write
        ver = x._version
        L.check(L.lib().t2s_rf_step(x.data_ptr(), v.data_ptr(), None, 0.0, 0.25, B, L.stream_ptr(dev)), "t2s_rf_step")
        assert x._version == ver

    with torch.no_grad():
        for pairing in (False, True):
            m.set_pairing(pairing)
            x = synth.make_latents(9, B).to(dev)
            for _ in range(2):                                   # show the pattern twice: arms the speculation when it is on
                m(input=x, t=t, text_input=None)
                m(input=x, t=t, text_input=emb)
            u = m(input=x, t=t, text_input=None)
            assert (m.__dict__["_t2s_pair"]["stash"] is not None) == pairing
            x_before = x.clone()
            raw_update(x)
            c = m(input=x, t=t, text_input=emb)
            want_new = fresh(input=x, t=t, text_input=emb)
            want_old = fresh(input=x_before, t=t, text_input=emb)
            assert torch.equal(u, fresh(input=x_before, t=t, text_input=None))
            if pairing:
                assert torch.equal(c, want_old) and not torch.equal(c, want_new)      # the documented limit
            else:
                assert torch.equal(c, want_new)
                ref = O.dit_forward(sd, x.cpu(), t.cpu(), emb.cpu())
                assert float((c.cpu() - ref).abs().max()) < 1e-4


def test_env_opt_out_and_math_switch_between_the_pair(dev, monkeypatch):
    """T2S_NO_PAIRING=1 is the environment form of set_pairing(False); a set_math() between the two calls of a pair drops
    the stash (the conditional half must come from the arithmetic now selected)."""
    m, fresh = _model(dev), _model(dev)
    fresh.set_pairing(False)
    B = 2
    x, emb = synth.make_latents(9, B).to(dev), synth.make_text_embeddings(3, B).to(dev)
    t = torch.full((B,), 5, dtype=torch.long, device=dev)
    with torch.no_grad():
        for _ in range(2):
            m(input=x, t=t, text_input=None)
            m(input=x, t=t, text_input=emb)
        m(input=x, t=t, text_input=None)
        assert m.__dict__["_t2s_pair"]["stash"] is not None
        m.set_math("bf16x3")
        c = m(input=x, t=t, text_input=emb)
        fresh.set_math("bf16x3")
        assert torch.equal(c, fresh(input=x, t=t, text_input=emb))
        m.set_math("f32")
        fresh.set_math("f32")
        monkeypatch.setenv("T2S_NO_PAIRING", "1")
        for _ in range(3):
            u = m(input=x, t=t, text_input=None)
            assert m.__dict__["_t2s_pair"]["stash"] is None and not m.__dict__["_t2s_pair"]["armed"]
            c = m(input=x, t=t, text_input=emb)
        assert torch.equal(u, fresh(input=x, t=t, text_input=None)) and torch.equal(c, fresh(input=x, t=t, text_input=emb))


# ------------------------------------------------------------------------------------------------ the shipped default arithmetic
def test_infer_driver_at_its_shipped_default_math(dev, tmp_path, monkeypatch):
    """The suite pins T2S_DEFAULT_MATH=f32 (tests/conftest.py) so the headline kernels stay covered; THIS test removes the pin
    and runs infer.py exactly as a user gets it: the run reports bf16x3 (round 5: the drivers' default, profiles/r05_accuracy.md),
    its four files equal the oracle's restatement of infer.py:65-123 within the same 1e-4 as the f32 run, and `--math f32` on the
    same rows gives the exact-MFMA bits of the pinned suite (both arithmetics fp32-accurate: the two runs differ by < 1e-4)."""
    import os
    import infer as drv
    from datafactory.dataset import SyntheticT2SDataset
    monkeypatch.delenv("T2S_DEFAULT_MATH", raising=False)
    monkeypatch.chdir(tmp_path)
    seed, L_, n_ds, bs, steps, cfg = 21, 48, 11, 2, 6, 9.0
    outs = {}
    for tag, extra in (("default", []), ("f32", ["--math", "f32"])):
        save = str(tmp_path / tag)
        a = drv.main(["--dataset_name", f"ETTh1_{L_}", "--backbone", "ddpm", "--denoiser", "DiT", "--total_step", str(steps), "--cfg_scale",
                      str(cfg), "--batch_size", str(bs), "--save_path", save, "--synthetic", str(n_ds), "--random_init", "--seed", str(seed),
                      "--no_figs"] + extra)
        assert a.math == ("bf16x3" if tag == "default" else "f32")
        out = os.path.join(save, "generation", f"ddpm_DiT_ETTh1_{L_}_{cfg}_{steps}")
        outs[tag] = {f: np.load(os.path.join(out, f + ".npy")) for f in ("x_1", "x_t", "x_t_latent_dec_array", "x_t_latent_enc_array")}
    x1 = outs["default"]["x_1"][:, :, 0]
    n = (n_ds // bs) * bs
    ds = SyntheticT2SDataset(n_ds, L_)
    rows = [int(np.argmin(np.abs(ds.samples - x1[i][None]).sum(axis=1))) for i in range(n)]
    text = torch.from_numpy(ds.embedding[rows]).float()
    sd, vsd = synth.make_dit_state_dict(seed), synth.make_vae_state_dict(seed)
    with torch.no_grad():
        x_T = torch.from_numpy(O.device_normal(seed, 0xFFFFFFFF, 0, n)).view(n, 64, 30)
        noises = [torch.from_numpy(O.device_normal(seed, j, 0, n)).view(n, 64, 30) for j in range(steps)]
        ref = O.sample_ddpm(sd, x_T, text, steps, cfg, noises)
        series, _ = O.vae_decode(vsd, ref, L_)
    scale = max(1.0, float(ref.abs().max()))
    for tag in ("default", "f32"):
        assert np.array_equal(outs[tag]["x_1"], outs["default"]["x_1"])                      # the same rows in the same order
        assert float(np.abs(outs[tag]["x_t_latent_dec_array"] - ref.numpy()).max()) < 1e-4 * scale, tag
        assert float(np.abs(outs[tag]["x_t"][:, :, 0] - series.reshape(n, L_).numpy()).max()) < 1e-4 * scale, tag
    assert not np.array_equal(outs["default"]["x_t_latent_dec_array"], outs["f32"]["x_t_latent_dec_array"])   # two arithmetics...
    assert float(np.abs(outs["default"]["x_t_latent_dec_array"] - outs["f32"]["x_t_latent_dec_array"]).max()) < 1e-4 * scale   # ...one accuracy


# ------------------------------------------------------------------------------------------------ patchify in the prologue
_PATCH_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r})
from t2ms_amd import synth
from model.denoiser.transformer import Transformer
dev = torch.device("cuda", 0)
m = Transformer(); m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True); m = m.to(dev).eval()
out = {{}}
for math in ("f32", "bf16x3"):
    m.set_math(math)
    for B in (3, 40):
        x = synth.make_latents(5, B).to(dev); t = torch.arange(B, device=dev) % 50
        text = synth.make_text_embeddings(9, B).to(dev)
        with torch.no_grad():
            out[f"{{math}}_{{B}}_c"] = m(input=x, t=t, text_input=text).cpu().numpy()
            out[f"{{math}}_{{B}}_u"] = m(input=x, t=t, text_input=None).cpu().numpy()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("var,values", [("T2S_PATCHIFY_KERNEL", ("0", "1")), ("T2S_ATTN_PARTS", ("2", "4")),
                                        ("T2S_ATTN_PERSIST_MIN", ("1", "100000")), ("T2S_ROWS16_MAX_SEQS", ("0", "100000"))])
def test_scheduling_switches_do_not_change_a_bit(dev, tmp_path, var, values):
    """Switches that only choose a launch FORM, each read once per process (hence child processes), must not change a bit in either
    arithmetic at a 16-token and a 32-token size:
      T2S_PATCHIFY_KERNEL  block 0's tokens from the prologue of the <qkv only> row kernel (32-token f32, 16-token f32 and -- round
                           5 -- bf16x3) or from the stand-alone patchify_kernel (same helpers);
      T2S_ATTN_PARTS       two or four workgroups per head in the small-launch attention kernel (one or two query tiles per wave);
      T2S_ATTN_PERSIST_MIN the persistent attention kernel from one head on / never (f32);
      T2S_ROWS16_MAX_SEQS  the 16-token row kernels never / always (f32)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "switch_ab.py"
    script.write_text(_PATCH_SCRIPT.format(repo=repo))
    outs = []
    for flag in values:
        dst = str(tmp_path / f"out_{flag}.npz")
        env = dict(os.environ, **{var: flag})
        subprocess.run([sys.executable, str(script), dst], check=True, env=env, cwd=repo, timeout=300)
        outs.append(np.load(dst))
    assert set(outs[0].files) == set(outs[1].files) and len(outs[0].files) == 8
    for k in outs[0].files:
        assert np.array_equal(outs[0][k], outs[1][k]), (var, k)
