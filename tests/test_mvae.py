"""The multichannel LA-VAE codec of the T2MS motion models (reference model/pretrained/myvqvae.py): the mirrors
model.pretrained.myvqvae, the C entries t2s_vae_create_mc / _channels / _encode_mc / _decode_mc, and the sampler's (B,C,L) decode.

Reference: tests/golden/mvae.npz, recorded from the reference module by tests/golden/gen_golden_mvae.py (outputs only; weights
and inputs come from t2ms_amd.synth seeds, the plan of configurations and cases travels inside the file).  Shapes the file does
not hold are compared with `_ref_encode` / `_ref_decode` below, a torch-functional restatement of the two forwards that a CPU
test pins to the file.

Bars: the project's LA-VAE bar of test_vae_golden, max |d| < 1e-5 (outputs are 0.02 .. 0.2 large; the reference's own fp32 run
differs from its fp64 run by <= 6.9e-7 on these shapes, a wrong tap moves a value by O(0.1)); 2e-5 for the decode of an N(0,1)
latent; gradients of the torch-op training path within 2e-4 of each tensor's largest (tests/test_lavae_pretrain_gpu.py).
"""
import ctypes as C
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from t2ms_amd import _lib as L
from t2ms_amd import synth

TOL, TOL_RAND, GRAD_TOL = 1e-5, 2e-5, 2e-4
NAMES = ("z", "before", "after", "rec", "recr")


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "mvae.npz")) as f:
        g = {k: f[k] for k in f.files}
    g["plan"] = json.loads(str(g["plan"]))
    return g


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ shared with the generator
def _key(cfg, W, Ln, B):
    return f"{cfg}_W{W}_L{Ln}_B{B}"


def _state_dict(gold, cfg):
    k = gold["plan"]["cfgs"][cfg]
    return synth.make_mvae_state_dict(k["seed"], k["channels"], 128, k["n_res"], k["res_hidden"])


def _inputs(gold, cfg, W, Ln, B):
    ch = gold["plan"]["cfgs"][cfg]["channels"]
    s = 1000 * ch + 7 * B + W + Ln
    return synth.make_mseries(s, B, ch, Ln), synth.make_wide_latents(s, B, W)


def _model(gold, cfg, W):
    from model.pretrained.myvqvae import vqvae
    k = gold["plan"]["cfgs"][cfg]
    m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=k["n_res"], res_hidden_size=k["res_hidden"],
                                    embedding_dim=64, flow_dim=W, input_dim=k["channels"]))
    m.load_state_dict(_state_dict(gold, cfg), strict=True)
    return m.eval()


# ------------------------------------------------------------------------------------------------ the restatement
def _ref_stack(sd, p, h):
    i = 0
    while f"{p}._residual_stack._layers.{i}._block.1.weight" in sd:
        h = F.relu(h)            # nn.ReLU(True) mutates the block input: the skip carries relu(x)
        m = F.relu(F.conv1d(h, sd[f"{p}._residual_stack._layers.{i}._block.1.weight"], None, 1, 1))
        h = h + F.conv1d(m, sd[f"{p}._residual_stack._layers.{i}._block.3.weight"], None)
        i += 1
    return F.relu(h)


def _ref_encode(sd, x, W):
    h = F.relu(F.conv1d(x, sd["encoder._conv_1.weight"], sd["encoder._conv_1.bias"], 2, 1))
    h = F.relu(F.conv1d(h, sd["encoder._conv_2.weight"], sd["encoder._conv_2.bias"], 2, 1))
    h = F.conv1d(h, sd["encoder._conv_3.weight"], sd["encoder._conv_3.bias"], 1, 1)
    before = F.conv1d(_ref_stack(sd, "encoder", h), sd["encoder._pre_vq_conv.weight"], sd["encoder._pre_vq_conv.bias"])
    return F.interpolate(before, size=W, mode="linear", align_corners=True), before


def _ref_decode(sd, z, length):
    after = F.interpolate(z, size=int(length / 4), mode="linear", align_corners=True)
    h = F.conv1d(after, sd["decoder._conv_1.weight"], sd["decoder._conv_1.bias"], 1, 1)
    h = _ref_stack(sd, "decoder", h)
    h = F.relu(F.conv_transpose1d(h, sd["decoder._conv_trans_1.weight"], sd["decoder._conv_trans_1.bias"], 2, 1))
    h = F.conv_transpose1d(h, sd["decoder._conv_trans_2.weight"], sd["decoder._conv_trans_2.bias"], 2, 1)
    return F.interpolate(h, size=length, mode="linear", align_corners=True), after


_REF_CACHE = {}


def _ref_case(gold, cfg, W, Ln, B):
    """The five outputs of a case from the restatement (CPU, computed once per case)."""
    k = _key(cfg, W, Ln, B)
    if k not in _REF_CACHE:
        sd = _state_dict(gold, cfg)
        x, zr = _inputs(gold, cfg, W, Ln, B)
        with torch.no_grad():
            z, before = _ref_encode(sd, x, W)
            rec, after = _ref_decode(sd, z, Ln)
            recr, _ = _ref_decode(sd, zr, Ln)
        _REF_CACHE[k] = {n: t.numpy() for n, t in zip(NAMES, (z, before, after, rec, recr))}
    return _REF_CACHE[k]


def _maxdiff(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def _check_recorded(gold, case, got, tol, tol_rand, tol_sum):
    """`got` (name -> full array) against what the file holds of the case: full arrays, or strided slices + fp64 row sums."""
    k, st = _key(case["cfg"], case["W"], case["L"], case["B"]), case["stride"]
    for n in NAMES:
        a = got[n].detach().cpu().numpy() if torch.is_tensor(got[n]) else got[n]
        bar = tol_rand if n == "recr" else tol
        if n in ("rec", "recr") or st == 1:
            d = _maxdiff(a, gold[f"{n}_{k}"])
        else:
            d = _maxdiff(np.ascontiguousarray(a[:, :, ::st]), gold[f"{n}_{k}"])
            ds = float(np.abs(a.astype(np.float64).sum(2) - gold[f"{n}_rowsum_{k}"]).max())
            print(f"{k} {n} row sums: {ds:.3e} (bar {tol_sum * a.shape[2]:.1e})")
            assert ds < tol_sum * a.shape[2], (k, n, ds)
        print(f"{k} {n}: max|d| = {d:.3e} (bar {bar:.0e})")
        assert d < bar, (k, n, d)


# ------------------------------------------------------------------------------------------------ CPU tests
def test_restatement_matches_the_reference_fixture(gold):
    """_ref_encode / _ref_decode (the same torch ops as myvqvae.py:49-61,76-86) reproduce every recorded case: 1e-6, the bar of
    tests/test_oracle_golden.py for the single-channel codec (fp32 conv summation order may differ with the thread count)."""
    assert len(gold["plan"]["cases"]) == 21
    for case in gold["plan"]["cases"]:
        ref = _ref_case(gold, case["cfg"], case["W"], case["L"], case["B"])
        ch = gold["plan"]["cfgs"][case["cfg"]]["channels"]
        assert ref["rec"].shape == (case["B"], ch, case["L"]) and ref["z"].shape == (case["B"], 64, case["W"])
        _check_recorded(gold, case, ref, 1e-6, 1e-6, 1e-6)


def test_mirror_state_dict_keys_and_shapes(gold):
    """The mirror's state dict has the reference module's keys, order and shapes (recorded for the deadlift configuration),
    and synth.make_mvae_state_dict loads strictly for every configuration."""
    want = gold["plan"]["state_dict_c7"]
    have = {k: list(v.shape) for k, v in _model(gold, "c7", 50).state_dict().items()}
    assert list(have) == list(want) and have == want
    assert have["encoder._conv_1.weight"] == [64, 7, 4] and have["decoder._conv_trans_2.weight"] == [64, 7, 4]
    for cfg in gold["plan"]["cfgs"]:
        _model(gold, cfg, 30)


def test_pickle_round_trip_resolves_through_the_reference_path(gold):
    import model.pretrained.myvqvae as M
    m = _model(gold, "c10", 64)
    blob = pickle.dumps(m)
    assert b"model.pretrained.myvqvae" in blob and b"t2ms_amd" not in blob
    m2 = pickle.loads(blob)
    assert type(m2) is M.vqvae and type(m2.encoder) is M.Encoder and m2.encoder.flow_dim == 64
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    for cls in (M.Residual, M.ResidualStack, M.Encoder, M.Decoder, M.vqvae):
        assert cls.__module__ == "model.pretrained.myvqvae"


def test_cpu_tensor_raises(gold):
    m = _model(gold, "c7", 30)
    x, zr = _inputs(gold, "c7", 30, 36, 1)
    with torch.no_grad():
        with pytest.raises(L.T2SError):
            m.encoder(x)
        with pytest.raises(L.T2SError):
            m.decoder(zr, 36)
    # custom_loss is plain torch (myvqvae.py:144-156)
    a, b = torch.rand(2, 7, 9), torch.rand(2, 7, 9)
    want = F.smooth_l1_loss(a, b) + 0.1 * F.smooth_l1_loss(a[..., 1:] - a[..., :-1], b[..., 1:] - b[..., :-1])
    assert torch.equal(m.custom_loss(a, b), want)


def test_lib_declares_the_new_symbols():
    I, VP = C.c_int, C.c_void_p
    assert L.SYMBOLS["t2s_vae_create_mc"] == (I, [C.POINTER(L.VaeWeights), I, C.POINTER(VP)])
    assert L.SYMBOLS["t2s_vae_channels"] == (I, [VP])
    for n in ("t2s_vae_encode_mc", "t2s_vae_decode_mc"):
        assert L.SYMBOLS[n] == (I, [VP, VP, VP, VP, I, I, I, VP])
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2s.h")).read()
    for n in ("t2s_vae_create_mc", "t2s_vae_channels", "t2s_vae_encode_mc", "t2s_vae_decode_mc"):
        assert f"int {n}(" in header


# ------------------------------------------------------------------------------------------------ GPU tests
_GPU_MODELS = {}


def _gpu_model(gold, dev, cfg, W):
    if (cfg, W) not in _GPU_MODELS:
        _GPU_MODELS[(cfg, W)] = _model(gold, cfg, W).to(dev)
    return _GPU_MODELS[(cfg, W)]


def _gpu_case(gold, dev, cfg, W, Ln, B):
    m = _gpu_model(gold, dev, cfg, W)
    x, zr = _inputs(gold, cfg, W, Ln, B)
    ch = gold["plan"]["cfgs"][cfg]["channels"]
    with torch.no_grad():
        z, before = m.encoder(x.to(dev))
        rec, after = m.decoder(z, Ln)
        recr, after_r = m.decoder(zr.to(dev), Ln)
        assert torch.equal(m(x.to(dev)), rec)
    assert tuple(z.shape) == (B, 64, W) and tuple(before.shape) == (B, 64, Ln // 4) == tuple(after.shape)
    assert tuple(rec.shape) == (B, ch, Ln) == tuple(recr.shape)           # never squeezed: (1,C,L) at B = 1, (B,1,L) at C = 1
    return dict(zip(NAMES, (z, before, after, rec, recr)))


def _check_vs_restatement(gold, got, cfg, W, Ln, B):
    ref = _ref_case(gold, cfg, W, Ln, B)
    for n in NAMES:
        d, bar = _maxdiff(got[n], ref[n]), (TOL_RAND if n == "recr" else TOL)
        print(f"{_key(cfg, W, Ln, B)} {n} vs restatement: max|d| = {d:.3e} (bar {bar:.0e})")
        assert d < bar, (cfg, W, Ln, B, n, d)


def _recorded(gold, cfg, W, Ln, B):
    for case in gold["plan"]["cases"]:
        if (case["cfg"], case["W"], case["L"], case["B"]) == (cfg, W, Ln, B):
            return case
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Ln", [36, 100, 128])
@pytest.mark.parametrize("cfg,W", [("c7", 50), ("c10", 64)])
def test_parity_with_the_reference_fixture(gold, dev, cfg, W, Ln, B):
    """z, before, after, recon and the decode of an N(0,1) latent against the REFERENCE run (1e-5; 2e-5 for the random
    latent; fp64 row sums within 1e-5 per position where the file holds strided slices)."""
    case = _recorded(gold, cfg, W, Ln, B)
    assert case is not None
    _check_recorded(gold, case, _gpu_case(gold, dev, cfg, W, Ln, B), TOL, TOL_RAND, TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("Ln", [9, 37, 50, 101, 103])
def test_lengths_that_are_no_multiple_of_4(gold, dev, Ln):
    """Odd lengths: the floor lengths of the two stride-2 convolutions (their last taps are real samples) and the final
    resampling 4 (L//4) -> L, against the restatement, and against the reference run where recorded (9, 37, 101)."""
    got = _gpu_case(gold, dev, "c7", 30, Ln, 2)
    _check_vs_restatement(gold, got, "c7", 30, Ln, 2)
    case = _recorded(gold, "c7", 30, Ln, 1)
    assert (case is not None) == (Ln in (9, 37, 101))
    if case is not None:
        _check_recorded(gold, case, _gpu_case(gold, dev, "c7", 30, Ln, 1), TOL, TOL_RAND, TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,W,Ln", [("c10", 64, 144), ("c10", 64, 263), ("c7r1", 30, 263), ("c7r0", 30, 263)])
def test_time_tiles(gold, dev, cfg, W, Ln):
    """L//4 > 32 runs in time tiles with recomputed halos: 144 -> 36 positions (two tiles each way), 263 -> 65 (three ragged
    tiles and the final resampling across their seams); stacks of 3, 1 and 0 layers have halos, hence cores, of their own.
    Against the restatement at B = 2 and the reference run (B = 1, strided + row sums) where recorded."""
    _check_vs_restatement(gold, _gpu_case(gold, dev, cfg, W, Ln, 2), cfg, W, Ln, 2)
    case = _recorded(gold, cfg, W, Ln, 1)
    assert (case is not None) == (cfg == "c10")
    if case is not None:
        _check_recorded(gold, case, _gpu_case(gold, dev, cfg, W, Ln, 1), TOL, TOL_RAND, TOL)


@pytest.mark.gpu
def test_tiled_encode_needs_the_before_buffer(gold, dev):
    m = _gpu_model(gold, dev, "c10", 64)
    x = _inputs(gold, "c10", 64, 144, 2)[0].to(dev)
    z = torch.empty(2, 64, 64, device=dev)
    h = m.encoder._handle(dev)
    rc = L.lib().t2s_vae_encode_mc(h, x.data_ptr(), z.data_ptr(), None, 2, 144, 64, L.stream_ptr(dev))
    assert rc != 0 and b"before" in L.lib().t2s_last_error()
    # one tile (L//4 <= 32) does not need it, and gives the z of the call that writes it
    x = _inputs(gold, "c10", 64, 128, 2)[0].to(dev)
    L.check(L.lib().t2s_vae_encode_mc(h, x.data_ptr(), z.data_ptr(), None, 2, 128, 64, L.stream_ptr(dev)))
    with torch.no_grad():
        assert torch.equal(z, m.encoder(x)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,W,Ln", [("c1", 1, 24), ("c16", 2, 8), ("c16", 64, 8), ("c1", 64, 50), ("c7", 1, 8), ("c7", 2, 37),
                                      ("c7r1", 30, 50), ("c7r0", 30, 50)])
def test_width_and_channel_edges(gold, dev, cfg, W, Ln):
    """W in {1, 2, 64}, C in {1, 16}, L = 8 (two positions at L/4), and the 1- and 0-layer stacks."""
    _check_vs_restatement(gold, _gpu_case(gold, dev, cfg, W, Ln, 2), cfg, W, Ln, 2)
    case = _recorded(gold, cfg, W, Ln, 1)
    if case is not None:
        _check_recorded(gold, case, _gpu_case(gold, dev, cfg, W, Ln, 1), TOL, TOL_RAND, TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("Ln", [24, 96])
def test_one_channel_agrees_with_the_single_channel_entries(gold, dev, Ln):
    """C = 1, W = 30: the _mc entries against t2s_vae_encode / t2s_vae_decode on the same weights, bit for bit -- both families
    of entries launch the same kernels (the single-channel codec is C = 1), and the interpolation tap's rounding is pinned."""
    from model.pretrained.vqvae import vqvae as vqvae1
    m = _gpu_model(gold, dev, "c1", 30)
    k = gold["plan"]["cfgs"]["c1"]
    s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=k["n_res"], res_hidden_size=k["res_hidden"],
                                     embedding_dim=64))
    s.load_state_dict(_state_dict(gold, "c1"), strict=True)
    s = s.to(dev).eval()
    x = _inputs(gold, "c1", 30, Ln, 3)[0].to(dev)
    with torch.no_grad():
        z, before = m.encoder(x)
        rec, after = m.decoder(z, Ln)
        z1, before1 = s.encoder(x[:, 0, :])
        rec1, after1 = s.decoder(z1, Ln)
    assert tuple(rec.shape) == (3, 1, Ln) and tuple(rec1.shape) == (3, Ln)
    for n, a, b in (("z", z, z1), ("before", before, before1), ("after", after, after1), ("rec", rec[:, 0, :], rec1)):
        d = _maxdiff(a, b)
        print(f"C=1 L={Ln} {n}: mc vs single-channel max|d| = {d:.3e}")
        assert torch.equal(a, b), (n, d)


def _single_channel_model(dev):
    if "single" not in _GPU_MODELS:
        from model.pretrained.vqvae import vqvae as vqvae1
        s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
        s.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
        _GPU_MODELS["single"] = s.to(dev).eval()
    return _GPU_MODELS["single"]


def _interp_cpu(t, size):
    return F.interpolate(t.cpu(), size=size, mode="linear", align_corners=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,W,Ln", [(1, 30, 24), (1, 30, 96), (1, 30, 136), (7, 64, 36), (7, 1, 24), (7, 50, 263)])
def test_decode_after_is_torch_interpolation_bit_for_bit(gold, dev, ch, W, Ln):
    """`after` of a decode is pure interpolation of the latent: torch.equal with F.interpolate(align_corners=True) on the CPU,
    whose rounding sequence the tap restates (t2s_vae.hip, InterpTap).  Single-channel entries at W 30 -- L 136 is two decoder
    tiles, the windowed form -- and the multichannel ones at C 7 with W in {64, 1, 50}; B = 2."""
    if ch == 1:
        m, z = _single_channel_model(dev), synth.make_latents(Ln, 2)
    else:
        m, z = _gpu_model(gold, dev, "c7", W), synth.make_wide_latents(Ln, 2, W)
    assert tuple(z.shape) == (2, 64, W)
    with torch.no_grad():
        _, after = m.decoder(z.to(dev), Ln)
    want = _interp_cpu(z, Ln // 4)
    print(f"C={ch} W={W} L={Ln} after vs torch CPU: max|d| = {_maxdiff(after, want):.3e}")
    assert torch.equal(after.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,W,Ln", [(1, 30, 24), (1, 30, 128), (1, 30, 136), (7, 64, 36), (7, 2, 37), (7, 50, 263)])
def test_encode_z_is_torch_interpolation_of_before_bit_for_bit(gold, dev, ch, W, Ln):
    """z of an encode is the interpolation of the `before` the same call wrote: torch.equal with F.interpolate on the CPU.
    Single-channel: L 128 is the largest series the encode kernel finishes itself, 136 runs in tiles and vae_interp_rows_kernel
    finishes it from the whole row -- so a tiled and a fused latent are the same function of `before`.  Multichannel C 7: one
    tile with W 64 and W 2 (L 37: floor lengths) and three ragged tiles at L 263; B = 2."""
    if ch == 1:
        m, x = _single_channel_model(dev), synth.make_series(Ln, 2, Ln)
    else:
        m, x = _gpu_model(gold, dev, "c7", W), synth.make_mseries(Ln, 2, 7, Ln)
    with torch.no_grad():
        z, before = m.encoder(x.to(dev))
    assert tuple(z.shape) == (2, 64, W) and tuple(before.shape) == (2, 64, Ln // 4)
    want = _interp_cpu(before, W)
    print(f"C={ch} W={W} L={Ln} z vs torch CPU interpolation of before: max|d| = {_maxdiff(z, want):.3e}")
    assert torch.equal(z.cpu(), want)


@pytest.mark.gpu
def test_refusals(gold, dev):
    """Wrong-kind handles in both directions, C = 0 / 17, W = 65, L = 7, an undersized enc_conv1_w: an error code and a message
    each, before any launch; a valid call works afterwards."""
    from model.pretrained.vqvae import vqvae as vqvae1
    lib, st = L.lib(), L.stream_ptr(dev)
    m = _gpu_model(gold, dev, "c7", 30)
    s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    s.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    s = s.to(dev).eval()
    x, zr = (t.to(dev) for t in _inputs(gold, "c7", 30, 36, 2))
    x1 = synth.make_series(3, 2, 36).to(dev)
    with torch.no_grad():
        want_z, _ = m.encoder(x)
        want_rec, _ = m.decoder(zr, 36)
    he, hd = m.encoder._handle(dev), m.decoder._handle(dev)
    h1e, h1d = s.encoder._handle(dev), s.decoder._handle(dev)
    assert lib.t2s_vae_channels(he) == 7 and lib.t2s_vae_channels(hd) == 7
    assert lib.t2s_vae_channels(h1e) == 0 and lib.t2s_vae_channels(h1d) == 0 and lib.t2s_vae_channels(None) == 0
    z = torch.empty(2, 64, 64, device=dev)
    before = torch.empty(2, 64, 9, device=dev)
    rec = torch.empty(2, 7, 36, device=dev)
    grads = torch.zeros(1 << 20, device=dev)

    def refused(rc, *words):
        msg = lib.t2s_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    # a multichannel handle in the single-channel entries
    refused(lib.t2s_vae_encode(he, x.data_ptr(), z.data_ptr(), before.data_ptr(), 2, 36, st), b"t2s_vae_encode_mc")
    refused(lib.t2s_vae_decode(hd, zr.data_ptr(), rec.data_ptr(), None, 2, 36, st), b"t2s_vae_decode_mc")
    refused(lib.t2s_vae_decode_w(hd, zr.data_ptr(), rec.data_ptr(), None, 2, 36, 30, st), b"t2s_vae_decode_mc")
    ge, gd = L.VaeEncGrads(), L.VaeDecGrads()
    for g in (ge, gd):                      # (never reached: the handle's kind is checked first)
        for name, ctype in g._fields_:
            if ctype is C.c_void_p:
                setattr(g, name, grads.data_ptr())
            else:
                getattr(g, name)[:4] = [grads.data_ptr()] * 4
    refused(lib.t2s_vae_encode_backward(he, x.data_ptr(), z.data_ptr(), None, C.byref(ge), 2, 36, st), b"t2s_vae_encode_mc")
    refused(lib.t2s_vae_decode_backward(hd, zr.data_ptr(), rec.data_ptr(), None, C.byref(gd), None, 2, 36, 30, st), b"t2s_vae_decode_mc")
    # a single-channel handle in the multichannel entries
    refused(lib.t2s_vae_encode_mc(h1e, x1.data_ptr(), z.data_ptr(), before.data_ptr(), 2, 36, 30, st), b"single-channel", b"t2s_vae_encode")
    refused(lib.t2s_vae_decode_mc(h1d, zr.data_ptr(), rec.data_ptr(), None, 2, 36, 30, st), b"single-channel", b"t2s_vae_decode")
    # latent width, length, batch
    refused(lib.t2s_vae_encode_mc(he, x.data_ptr(), z.data_ptr(), before.data_ptr(), 2, 36, 65, st), b"latent width 65")
    refused(lib.t2s_vae_decode_mc(hd, zr.data_ptr(), rec.data_ptr(), None, 2, 36, 65, st), b"latent width 65")
    refused(lib.t2s_vae_encode_mc(he, x.data_ptr(), z.data_ptr(), before.data_ptr(), 2, 36, 0, st), b"latent width 0")
    refused(lib.t2s_vae_encode_mc(he, x.data_ptr(), z.data_ptr(), before.data_ptr(), 2, 7, 30, st), b"L=7")
    refused(lib.t2s_vae_decode_mc(hd, zr.data_ptr(), rec.data_ptr(), None, 2, 7, 30, st), b"L=7")
    refused(lib.t2s_vae_decode_mc(hd, zr.data_ptr(), rec.data_ptr(), None, 0, 36, 30, st), b"B=0")
    # channel counts at create
    w, keep = m.encoder._weights_struct()
    for ch in (0, 17, -1):
        ptr = C.c_void_p()
        refused(lib.t2s_vae_create_mc(C.byref(w), ch, C.byref(ptr)), b"channels=%d" % ch)
        assert not ptr.value
    # an enc_conv1_w that holds one channel where the handle is asked for seven: a private hipMalloc (torch's caching
    # allocator would hide the end of a small tensor inside a 2 MB segment)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 64 * 1 * 4 * 4) == 0
    try:
        good = w.enc_conv1_w
        w.enc_conv1_w = short.value
        ptr = C.c_void_p()
        refused(lib.t2s_vae_create_mc(C.byref(w), 7, C.byref(ptr)), b"t2s_vae_create_mc", b"allocation ends")
        assert not ptr.value
        refused(lib.t2s_vae_update_weights(he, C.byref(w), st), b"allocation ends")
        w.enc_conv1_w = good
    finally:
        hip.hipFree(short)
    del keep
    # valid calls still work, with the same bits
    with torch.no_grad():
        assert torch.equal(m.encoder(x)[0], want_z) and torch.equal(m.decoder(zr, 36)[0], want_rec)
        s.decoder(s.encoder(x1)[0], 36)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_weight_refresh_without_a_new_handle(gold, dev):
    """An in-place change of encoder._conv_1.weight / decoder._conv_trans_2.bias reaches the next forward through
    t2s_vae_update_weights (which copies the C-dependent sizes): same C handle, new values."""
    m = _model(gold, "c10", 64).to(dev)
    x = _inputs(gold, "c10", 64, 50, 2)[0].to(dev)
    sd = {k: v.clone() for k, v in _state_dict(gold, "c10").items()}
    with torch.no_grad():
        z0, _ = m.encoder(x)
        rec0, _ = m.decoder(z0, 50)
        he, hd = m.encoder.__dict__["_t2s_h"], m.decoder.__dict__["_t2s_h"]
        m.encoder._conv_1.weight[:, 9, :] *= -1.5             # the LAST channel: beyond a single-channel copy's extent
        m.decoder._conv_trans_2.bias[9] += 0.25
        z1, _ = m.encoder(x)
        rec1, _ = m.decoder(z0, 50)
    assert m.encoder.__dict__["_t2s_h"] is he and m.decoder.__dict__["_t2s_h"] is hd
    sd["encoder._conv_1.weight"][:, 9, :] *= -1.5
    sd["decoder._conv_trans_2.bias"][9] += 0.25
    with torch.no_grad():
        z_ref, _ = _ref_encode(sd, x.cpu(), 64)
        rec_ref, _ = _ref_decode(sd, z0.cpu(), 50)
    assert _maxdiff(z1, z_ref) < TOL and _maxdiff(rec1, rec_ref) < TOL
    assert _maxdiff(z1, z0) > 1e-3 and abs(_maxdiff(rec1[:, 9], rec0[:, 9]) - 0.25) < 1e-6 and torch.equal(rec1[:, :9], rec0[:, :9])


@pytest.fixture(scope="module")
def chain(dev):
    """The synthetic DiT and inputs of tests/test_hip_parity.py _chain_setup, and a single-channel decoder."""
    from model.denoiser.transformer import Transformer
    from model.pretrained.vqvae import vqvae as vqvae1
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    s = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    s.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    noises = torch.from_numpy(np.random.RandomState(99).randn(20, 4, 64, 30).astype(np.float32))
    return m.to(dev).eval(), s.to(dev).eval(), synth.make_latents(31337, 4), synth.make_text_embeddings(31337, 4), noises


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("Ln", [36, 37])
@pytest.mark.parametrize("backbone", ["flowmatching", "ddpm"])
def test_sampler_decodes_channels(gold, dev, chain, backbone, Ln, use_graph):
    """The fused sampler with a multichannel decoder (C 7, W 30): the hot loop is untouched -- the latent is array_equal to the
    one of the same sampler built with the single-channel decoder -- and the series is array_equal to the mirror's
    decoder(latent, L), (B,7,L); the trace is (steps,7,L)."""
    from t2ms_amd.sampler import Sampler
    dit, single, xT, text, noises = chain
    mc = _gpu_model(gold, dev, "c7", 30)
    noise = noises[:3] if backbone == "ddpm" else None
    s = Sampler(dit, mc.decoder, backbone, 3, 7.0, 4, Ln, dev, use_graph=use_graph)
    lat, series, _ = s.run(text, x_T=xT, noise=noise, decode=True)
    s1 = Sampler(dit, single.decoder, backbone, 3, 7.0, 4, 36, dev, use_graph=use_graph)
    lat1, series1, _ = s1.run(text, x_T=xT, noise=noise, decode=True)
    assert tuple(series.shape) == (4, 7, Ln) and tuple(series1.shape) == (4, 36)
    assert np.array_equal(lat.cpu().numpy(), lat1.cpu().numpy())
    with torch.no_grad():
        want, _ = mc.decoder(lat, Ln)
    assert np.array_equal(series.cpu().numpy(), want.cpu().numpy())
    lat2, _, tr = s.run(text, x_T=xT, noise=noise, decode=False, trace=True)
    assert tuple(tr.shape) == (3, 7, Ln) and np.array_equal(lat2.cpu().numpy(), lat.cpu().numpy())
    assert np.array_equal(tr[-1].cpu().numpy(), want[0].cpu().numpy())       # the last trace row: row 0 of the final latent


@pytest.mark.gpu
def test_sampler_length_rule_follows_the_decoder(gold, dev, chain):
    from t2ms_amd.sampler import Sampler
    dit, single, *_ = chain
    with pytest.raises(L.T2SError, match="length=37"):
        Sampler(dit, single.decoder, "flowmatching", 3, 7.0, 4, 37, dev)
    with pytest.raises(L.T2SError, match="length=7"):
        Sampler(dit, _gpu_model(gold, dev, "c7", 30).decoder, "flowmatching", 3, 7.0, 4, 7, dev)


@pytest.mark.gpu
def test_torch_op_training_step(gold, dev):
    """vqvae.shared_eval(batch, T2SAdamW, 'train') at C 7, L 36, B 3 runs the torch-op forwards under autograd (no HIP backward
    for C channels): the tuple has the reference's shapes, every parameter gets a finite gradient within 2e-4 of the
    tensor's largest against CPU autograd of the restatement, and the optimizer moved the parameters."""
    from t2ms_amd.train import T2SAdamW
    m = _model(gold, "c7", 50).to(dev).train()
    x = _inputs(gold, "c7", 50, 36, 3)[0]
    before_step = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss, recon_error, data_recon, z = m.shared_eval(x.to(dev), T2SAdamW(m.parameters(), lr=1e-3), "train")
    assert loss.dim() == 0 and recon_error.dim() == 0 and tuple(data_recon.shape) == (3, 7, 36) and tuple(z.shape) == (3, 64, 50)
    sd = {k: v.clone().requires_grad_(True) for k, v in _state_dict(gold, "c7").items()}
    zr, before = _ref_encode(sd, x, 50)
    rec, after = _ref_decode(sd, zr, 36)
    ref_recon = F.mse_loss(rec, x)
    ref_loss = ref_recon + F.mse_loss(before, after)
    ref_loss.backward()
    loss, recon_error, ref_loss_v, ref_recon_v = (float(t.detach()) for t in (loss, recon_error, ref_loss, ref_recon))
    assert abs(loss - ref_loss_v) < 2e-5 * abs(ref_loss_v) and abs(recon_error - ref_recon_v) < 2e-5 * abs(ref_recon_v)
    params = dict(m.named_parameters())
    assert set(params) == set(sd)
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        big = float(sd[k].grad.abs().max())
        d = _maxdiff(p.grad, sd[k].grad)
        assert big > 0 and d < GRAD_TOL * big, (k, d, big)
        assert not torch.equal(p.detach(), before_step[k]), k
    # 'val' runs the HIP forwards under no_grad and returns the same shapes
    m.eval()
    loss_v, rec_v, data_v, z_v = m.shared_eval(x.to(dev), None, "val")
    assert tuple(data_v.shape) == (3, 7, 36) and tuple(z_v.shape) == (3, 64, 50) and not data_v.requires_grad
