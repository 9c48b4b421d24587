"""The wide-latent DiT on the GPU (the T2MS motion models: latent width 50 / 64, 800 / 1024 tokens, f32 arithmetic): the packed
attention at the wide token counts against fp64, the forward / chains against the reference's own mytransformer.py
(tests/golden/wide_dit.npz, gen_golden_wide.py), the bitwise properties of the 480-token path carried over, and the
refusals."""
import ctypes as C
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's bar for the 480-token forward at the same weight family and output scale (test_hip_parity.py)
ATTN_TOL = 2e-5     # ... and for its f32 attention against fp64

_spec = importlib.util.spec_from_file_location("gen_golden_wide", os.path.join(os.path.dirname(__file__), "golden", "gen_golden_wide.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = {k: v for k, v in np.load(os.path.join(golden_dir, "wide_dit.npz")).items()}
    g["plan"] = json.loads(str(g["plan"]))
    return g


def _wide_model(dev, width, seed=2025, **kw):
    from model.denoiser.mytransformer import Transformer
    m = Transformer(width)
    m.load_state_dict(synth.make_dit_state_dict(seed, width=width, **kw), strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def models(dev):
    return {W: _wide_model(dev, W) for W in (50, 64)}


@pytest.fixture(scope="module")
def chain(dev):
    """The fixture's chain set-up: Transformer(50) with the chain weights, x_T, text, injected noise (B 2, 3 steps)."""
    c = gen.CHAIN
    m = _wide_model(dev, c["W"], c["weight_seed"], gain=c["gain"])
    xT, text, noise = gen.chain_inputs(synth)
    return m, xT.to(dev), text.to(dev), noise.to(dev)


def _maxdiff(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


# ------------------------------------------------------------------------------------------------ 1. attention
def _pack_frag(x):
    """(BH,N,32) -> fragment-major (include/t2s.h, t2s_attn_fwd_packed_n): P[((tile*4 + g)*64 + 32h + i)*4 + e] = X[32 tile + i][8g + 4h + e]."""
    BH, N, _ = x.shape
    return x.reshape(BH, N // 32, 32, 4, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous()


def _pack_vT(v):
    """(BH,N,32) -> transposed fragment-major: vT[((tile*4 + g)*64 + 32h + d)*4 + e] = V[32 tile + 8g + 4h + e][d]."""
    BH, N, _ = v.shape
    return v.reshape(BH, N // 32, 4, 2, 4, 32).permute(0, 1, 2, 3, 5, 4).contiguous()


def _unpack_o(od, n_seq, N):
    """o: [tile = seq * N/32 + t][G = head*4 + g][h][i][e] = O[seq][head][32 t + i][8g + 4h + e]"""
    return od.cpu().reshape(n_seq, N // 32, 4, 4, 2, 32, 4).permute(0, 2, 1, 5, 3, 4, 6).reshape(n_seq * 4, N, 32)


def _attn_n(dev, q, k, v, n_seq, N):
    qd, kd, vd = _pack_frag(q).to(dev), _pack_frag(k).to(dev), _pack_vT(v).to(dev)
    od = torch.full((n_seq * N * 128,), float("nan"), device=dev)
    L.check(L.lib().t2s_attn_fwd_packed_n(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), n_seq, N, L.stream_ptr(dev)),
            "t2s_attn_fwd_packed_n")
    return _unpack_o(od, n_seq, N)


def _ref_attn(q, k, v):
    return (torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()).float()


@pytest.mark.parametrize("N,n_seq,kind", [(800, 1, "plain"), (800, 3, "plain"), (1024, 1, "plain"), (1024, 3, "plain"),
                                          (800, 1, "late"), (1024, 1, "late"), (800, 3, "block0")])
def test_packed_attention_wide_vs_fp64(dev, N, n_seq, kind):
    """plain: N(0,1) operands with the spikes of the 480-token test (early and late re-scales).  late: scores are small
    everywhere (|s| of a few units in the exp2 domain) except for three keys of the LAST key block, each aligned with one
    query and scaled to a dot product of 270 -- 2^68 in the exp2 domain, more than 2^60 above that query's running reference,
    so the sticky reference is renewed in the last block.  block0: the same three keys in block 0 only -- the first reference
    is the largest score, everything after it underflows against it.  Three sequences are 12 heads: not a multiple of the 8 heads a workgroup group covers."""
    rs = np.random.RandomState(N + 10 * n_seq + len(kind))
    BH = n_seq * 4
    q, k, v = (torch.from_numpy(rs.randn(BH, N, 32).astype(np.float32)) for _ in range(3))
    if kind == "plain":
        q = q * 2.0
        k[:, N - 147] = q[:, 100] * 2.5
        k[:, 5] = q[:, N - 1] * 2.0
        k[:, N - 1] = q[:, 0] * 2.0
        k[:, N - 70] = q[:, 200] * 6.0
    else:
        q, k = q * 0.25, k * 0.25
        base = N - 32 if kind == "late" else 0
        for key, query in ((base + 3, 100), (base + 17, N - 1), (base + 31, 33)):
            k[:, key] = q[:, query] * (270.0 / q[:, query].pow(2).sum(-1, keepdim=True))     # q . k = 270
        s2 = (q[:, 100] * k[:, base + 3]).sum(-1) * (32 ** -0.5 * 1.4426950408889634)
        assert float(s2.min()) > 68.0          # log2-domain score of the aligned pair; the queries' other scores are a few units
    o = _attn_n(dev, q, k, v, n_seq, N)
    assert bool(torch.isfinite(o).all())
    err = _maxdiff(o, _ref_attn(q, k, v))
    print(f"attention N={N} n_seq={n_seq} {kind}: max abs err {err:.3e}")
    assert err < ATTN_TOL


def test_packed_attention_n_480_is_the_480_kernel(dev):
    rs = np.random.RandomState(5)
    n_seq = 3
    q, k, v = (torch.from_numpy(rs.randn(n_seq * 4, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 410] = q[:, 200] * 12.0
    qd, kd, vd = _pack_frag(q).to(dev), _pack_frag(k).to(dev), _pack_vT(v).to(dev)
    a, b = torch.empty(n_seq * 480 * 128, device=dev), torch.empty(n_seq * 480 * 128, device=dev)
    L.check(L.lib().t2s_attn_fwd_packed(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), a.data_ptr(), n_seq, L.stream_ptr(dev)))
    L.check(L.lib().t2s_attn_fwd_packed_n(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), b.data_ptr(), n_seq, 480, L.stream_ptr(dev)))
    assert torch.equal(a, b)
    assert _maxdiff(_unpack_o(b, n_seq, 480), _ref_attn(q, k, v)) < ATTN_TOL


# ------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("case", gen.FORWARD_CASES, ids=gen.case_key)
def test_forward_against_the_reference_fixture(gold, dev, models, case):
    """Bar: TOL = 1e-4 max abs, the bar of the 480-token forward; the reference's own fp32 result is 1.0e-6 to 1.7e-6 from an
    fp64 run of itself (recorded by the generator per case).  Were a case's recorded deviation above 2.5e-5, its bar would be four times
    that deviation.  B 3 at W 50 is 2,400 rows: a partial 64-row tile."""
    key, W, B = gen.case_key(case), case["W"], case["B"]
    m = models[W]
    x, text, t_long, t_float = (a.to(dev) for a in gen.forward_inputs(synth, case))
    with torch.no_grad():
        yc = m(input=x, t=t_long, text_input=text)
        stream = torch.empty(B, 16 * W, 128, device=dev)
        L.check(L.lib().t2s_dit_read_stream(m.t2s_handle(dev, B), stream.data_ptr(), B, L.stream_ptr(dev)))
        yu = m(input=x, t=t_long, text_input=None)
        yf = m(input=x, t=t_float, text_input=text)
    assert tuple(yc.shape) == (B, 64, W)
    rec = gold["plan"]["fp32_vs_fp64"][key]
    for name, got in (("cond", yc), ("uncond", yu), ("cond_float", yf)):
        bar = TOL if rec[name] <= 2.5e-5 else 4.0 * rec[name]
        err = _maxdiff(got, gold[f"{name}_{key}"])
        print(f"{key} {name}: max abs err {err:.3e} (reference fp32 vs fp64 {rec[name]:.2e}, bar {bar:.1e})")
        assert err < bar, (key, name)
    err = _maxdiff(stream[:1, ::gold["plan"]["tap_stride"]], gold[f"tap_post_mlp_3_{key}"])
    print(f"{key} post_mlp_3 tap: max abs err {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------------ 3. CFG passes
def test_cfg_pass_equals_two_forwards_bitwise_at_w64(dev, models):
    m, B, W = models[64], 2, 64
    x = synth.make_wide_latents(77, B, W).to(dev)
    text = synth.make_text_embeddings(77, B).to(dev)
    t = torch.full((B,), 421, dtype=torch.long, device=dev)
    lib, st = L.lib(), L.stream_ptr(dev)
    with torch.no_grad():
        yu, yc = m(input=x, t=t, text_input=None), m(input=x, t=t, text_input=text)
        h = m.t2s_handle(dev, 2 * B)
        temb = m.time_emb(t[:1])
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        L.check(lib.t2s_dit_forward_cfg(h, x.data_ptr(), temb.data_ptr(), text.data_ptr(), ou.data_ptr(), oc.data_ptr(), B, st))
        assert torch.equal(ou, yu) and torch.equal(oc, yc)
        # per-row t and a row permutation through _cfg_rows: rows are batch-invariant
        t2 = torch.tensor([900, 17], device=dev)
        yu2, yc2 = m(input=x, t=t2, text_input=None), m(input=x, t=t2, text_input=text)
        perm = torch.tensor([1, 0], device=dev)
        xp, tp, tembp = x[perm].contiguous(), text[perm].contiguous(), m.time_emb(t2[perm])
        L.check(lib.t2s_dit_forward_cfg_rows(h, xp.data_ptr(), tembp.data_ptr(), B, tp.data_ptr(), ou.data_ptr(), oc.data_ptr(), B, st))
    assert torch.equal(ou, yu2[perm]) and torch.equal(oc, yc2[perm])


# ------------------------------------------------------------------------------------------------ 4. width 30 through the new door
def test_create_w_30_is_create(dev):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    m = m.to(dev).eval()
    B = 3
    x, text = synth.make_latents(5, B).to(dev), synth.make_text_embeddings(5, B).to(dev)
    temb = m.time_emb(torch.tensor([999, 4, 250], device=dev))
    lib, st = L.lib(), L.stream_ptr(dev)
    w, keep, _ = m._weights_struct(dev)
    outs = []
    with torch.cuda.device(dev):
        for create in (lambda p: lib.t2s_dit_create(C.byref(w), B, C.byref(p)), lambda p: lib.t2s_dit_create_w(C.byref(w), 30, B, C.byref(p))):
            p = C.c_void_p()
            L.check(create(p), "create")
            try:
                assert lib.t2s_dit_latent_w(p) == 30 and lib.t2s_dit_max_seqs(p) == B
                out = torch.empty(B, 64, 30, device=dev)
                L.check(lib.t2s_dit_forward(p, x.data_ptr(), temb.data_ptr(), B, text.data_ptr(), out.data_ptr(), B, st))
                torch.cuda.synchronize(dev)
                outs.append(out)
            finally:
                lib.t2s_dit_destroy(p)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    del keep


# ------------------------------------------------------------------------------------------------ 5. sampler
def _mc_decoder(dev, width, channels=7):
    from model.pretrained.myvqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256, embedding_dim=64,
                                    flow_dim=width, input_dim=channels))
    v.load_state_dict(synth.make_mvae_state_dict(2025, channels, 128, 3, 256), strict=True)
    return v.to(dev).eval()


@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_chains_against_the_reference_fixture_and_their_bitwise_forms(gold, dev, chain, backbone):
    """The fixture's two 3-step CFG chains at W 50, B 2 (eager) within TOL = 1e-4 max abs (latents of absmax 4-5); the
    one-step graph, the whole-loop graph and two lanes at B 4 (the batch twice) give the same bits; with the 7-channel decoder
    at L 37 the series is t2s_vae_decode_mc of the returned latent, and so is the last row of trace0 (every row of a trace
    against the state it decodes: test_lms_sampler_equals_the_eager_class_api_loop_at_w64)."""
    from t2ms_amd.sampler import Sampler
    m, xT, text, noise = chain
    c = gen.CHAIN
    W, B, steps = c["W"], c["B"], c["steps"]
    want = gold["chain_ddpm_latent" if backbone == "ddpm" else "chain_rf_latent"]
    nz = noise if backbone == "ddpm" else None
    dec = _mc_decoder(dev, W).decoder
    s = Sampler(m, dec, backbone, steps, c["cfg"], B, 37, dev, use_graph=False)
    assert s.math == "f32" and s.width == W
    lat, series, _ = s.run(text, x_T=xT, noise=nz)
    err = _maxdiff(lat, want)
    print(f"{backbone} chain W={W}: max abs err {err:.3e} (latent absmax {float(np.abs(want).max()):.2f})")
    assert err < TOL
    with torch.no_grad():
        dec_want, _ = dec(lat, 37)
    assert tuple(series.shape) == (B, 7, 37) and torch.equal(series, dec_want)
    lat_t, _, tr = s.run(text, x_T=xT, noise=nz, decode=False, trace=True)
    assert tuple(tr.shape) == (steps, 7, 37) and torch.equal(lat_t, lat) and torch.equal(tr[-1], dec_want[0])
    for kw in (dict(loop_graph=0), dict(loop_graph=1)):
        g = Sampler(m, dec, backbone, steps, c["cfg"], B, 37, dev, use_graph=True, **kw)
        lat_g, series_g, _ = g.run(text, x_T=xT, noise=nz)
        assert g.graph_lanes == 1 and torch.equal(lat_g, lat) and torch.equal(series_g, series), kw
    x4, text4 = torch.cat([xT, xT]), torch.cat([text, text])
    nz4 = None if nz is None else torch.cat([nz, nz], dim=1)
    s4 = Sampler(m, None, backbone, steps, c["cfg"], 2 * B, 37, dev, use_graph=True, lanes=2)
    lat4, _, _ = s4.run(text4, x_T=x4, noise=nz4, decode=False)
    assert s4.graph_lanes == 2 and torch.equal(lat4[:B], lat) and torch.equal(lat4[B:], lat)


def test_lms_sampler_equals_the_eager_class_api_loop_at_w64(dev, models):
    """dpmpp2m, S = 3 of T = 100, W 64, B 2: the fused loop against model(...) twice per step and t2s_lms_step, bit for bit.
    The eager loop has every intermediate state, so EVERY row of trace0 (10-channel decoder, L 37) is compared with
    t2s_vae_decode_mc of row 0 of the state it decodes.  (A shorter run of the sampler does not reproduce an intermediate
    state: the coefficients and dt of every update depend on the number of steps.)"""
    from t2ms_amd.sampler import Sampler, lms_step, solver_tables
    m, B, W, cfg = models[64], 2, 64, 5.0
    xT = synth.make_wide_latents(9, B, W).to(dev)
    text = synth.make_text_embeddings(9, B).to(dev)
    dec = _mc_decoder(dev, W, channels=10).decoder
    s = Sampler(m, dec, "ddpm", 100, cfg, B, 37, dev, use_graph=True, solver="dpmpp2m", sample_steps=3)
    lat, _, _ = s.run(text, x_T=xT, decode=False)
    assert s.steps == 3 and tuple(lat.shape) == (B, 64, W) and bool(torch.isfinite(lat).all())
    lat_t, _, tr = s.run(text, x_T=xT, decode=False, trace=True)
    assert tuple(tr.shape) == (3, 10, 37) and torch.equal(lat_t, lat)
    tvals, coef = solver_tables("ddpm", "dpmpp2m", 100, 3, 0.0)
    coef_d = coef.to(dev)
    m.set_pairing(False)            # lms_step writes x in place through a raw pointer (Transformer.set_pairing)
    try:
        x, hist = xT.clone(), torch.zeros_like(xT)
        with torch.no_grad():
            for j in range(3):
                t = torch.full((B,), float(tvals[j]), device=dev)
                u, c = m(input=x, t=t, text_input=None), m(input=x, t=t, text_input=text)
                lms_step(x, hist, u, c, coef_d, j, cfg=cfg)
                assert torch.equal(tr[j], dec(x[:1], 37)[0][0]), f"trace row {j}"
    finally:
        m.set_pairing(True)
    assert torch.equal(x, lat)


# ------------------------------------------------------------------------------------------------ 6. Philox
def test_draw_xT_at_w64_is_the_oracle_stream(dev, models):
    from t2ms_amd.sampler import Sampler
    s = Sampler(models[64], None, "ddpm", 3, 7.0, 3, 40, dev, use_graph=False, seed=2025, row0=5)
    x = s.draw_xT()
    assert tuple(x.shape) == (3, 64, 64)
    ref = O.device_normal(2025, 0xFFFFFFFF, 5, 3, row_elems=4096)
    assert _maxdiff(x.reshape(3, 4096), ref) < 1e-5      # the bar of the 1920-wide draw (test_hip_parity.py)


# ------------------------------------------------------------------------------------------------ 7. refusals
def _refused(rc, *needles):
    msg = L.lib().t2s_last_error()
    assert rc != 0 and len(msg) > 0, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals(dev, models):
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd.sampler import Sampler
    lib, st = L.lib(), L.stream_ptr(dev)
    m64 = models[64]
    w, keep, _ = m64._weights_struct(dev)
    with torch.cuda.device(dev):
        p = C.c_void_p()
        _refused(lib.t2s_dit_create_w(C.byref(w), 40, 4, C.byref(p)), b"latent_w=40")
        assert not p.value
        # a 480-row pos_embed offered at width 64: refused with its state-dict key in the message
        m30 = Transformer(30)
        m30.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
        m30 = m30.to(dev).eval()
        w30, keep30, _ = m30._weights_struct(dev)
        counts = [t.numel() for t in keep30[:9]] + [64] + [t.numel() for t in keep30[9:]]
        _refused(lib.t2s_dit_weights_check_w(C.byref(w30), 64, (C.c_uint64 * L.DIT_N_TENSORS)(*counts), L.DIT_N_TENSORS), b"pos_embed")
        assert lib.t2s_dit_weights_check_w(C.byref(w30), 30, (C.c_uint64 * L.DIT_N_TENSORS)(*counts), L.DIT_N_TENSORS) == 0
        # ... and by t2s_dit_create_w itself, which has no counts: a private hipMalloc of exactly 480 x 128 floats (torch's caching
        # allocator would hide the end of the tensor inside a larger segment), as tests/test_hip_contracts.py does it
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        small = C.c_void_p()
        assert hip.hipMalloc(C.byref(small), 480 * 128 * 4) == 0
        try:
            keep_pos, w30.pos_embed = w30.pos_embed, small.value
            p = C.c_void_p()
            _refused(lib.t2s_dit_create_w(C.byref(w30), 64, 4, C.byref(p)), b"pos_embed", b"allocation ends")
            assert not p.value
            w30.pos_embed = keep_pos
        finally:
            hip.hipFree(small)
        h = m64.t2s_handle(dev, 4)
        assert lib.t2s_dit_latent_w(h) == 64
        for math in (L.MATH_CODES["bf16x3"], L.MATH_CODES["bf16"]):
            _refused(lib.t2s_dit_set_math(h, math), b"latent width 64")
        _refused(lib.t2s_dit_set_train_dtype(h, L.TRAIN_F32), b"latent width 30")
        x = synth.make_wide_latents(1, 1, 64).to(dev)
        temb, out = torch.zeros(1, 128, device=dev), torch.empty(1, 64, 64, device=dev)
        _refused(lib.t2s_dit_train_forward(h, C.byref(w), x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, st), b"latent width 30")
        _refused(lib.t2s_dit_train_backward(h, out.data_ptr(), C.byref(L.DitGrads()), 1, st), b"latent width 30")
        _refused(lib.t2s_dit_train_input_grad(h, out.data_ptr(), 1, st), b"latent width 30")
    with pytest.raises(L.T2SError, match="f32"):
        m64.set_math("bf16x3")
    with pytest.raises(L.T2SError, match="training runs at dim 30"):
        m64(input=x.requires_grad_(True), t=torch.zeros(1, device=dev), text_input=None)
    # a single-channel decoder at W 64: refused by the Sampler, and by t2s_sampler_create itself before any allocation
    from model.pretrained.vqvae import vqvae
    single = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    single.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    single = single.to(dev).eval()
    with pytest.raises(L.T2SError, match="multichannel"):
        Sampler(m64, single.decoder, "flowmatching", 3, 7.0, 2, 36, dev)
    tv = (C.c_float * 3)(0.0, 1 / 3, 2 / 3)
    cfg = L.SampleConfig()
    cfg.mode, cfg.steps, cfg.cfg_scale, cfg.batch, cfg.length = L.MODE_RF, 3, 7.0, 2, 36
    cfg.t_values = C.cast(tv, C.c_void_p).value
    with torch.cuda.device(dev):
        sp = C.c_void_p()
        _refused(lib.t2s_sampler_create(m64.t2s_handle(dev, 4), single.decoder._handle(dev), C.byref(cfg), C.byref(sp)), b"multichannel")
        assert not sp.value
        cfg.mode = L.MODE_LMS
        lms_coef = (C.c_float * 18)(*([1.0, 0.0, 0.0, 0.0, 0.0, 0.0] * 3))
        _refused(lib.t2s_sampler_create_lms(m64.t2s_handle(dev, 4), single.decoder._handle(dev), C.byref(cfg),
                                            C.cast(lms_coef, C.c_void_p), C.byref(sp)), b"multichannel")
        assert not sp.value
    # a codec trained at another latent width
    with pytest.raises(L.T2SError, match="flow_dim 50"):
        Sampler(m64, _mc_decoder(dev, 50).decoder, "flowmatching", 3, 7.0, 2, 36, dev)
    del keep
