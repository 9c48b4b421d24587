"""bf16x3 and bf16 inference of the wide-latent DiT on the GPU (Transformer(50) / Transformer(64) after set_wide_math(True);
include/t2s_wide_math.h): the wide attention kernel alone against fp64 in both plane counts, its persistent walk bit for bit,
the forward against the reference fixture / the f32 path / the autocast bar, the bitwise structure of the 480-token modes
carried over, the chains, the ragged sampler and the driver, and the refusals that stay.

Bars.  bf16x3 attention: max 2e-5, rms 1e-6 against the fp64 softmax (what t2s_attn_fwd_x3 is held to).  bf16 attention:
2^-8 max|v| per head against the fp64 exp2-softmax of the operands as the kernel rounds them (derived in
tests/test_math_bf16.py).  bf16x3 forward: the fixture rule of tests/test_wide_dit.py and 2e-5 to the f32 path.  bf16 forward:
the restatement under torch.autocast(bfloat16), rms <= 1.05 x per case, max <= 1.25 x pooled (tests/_wide_math_ref.py)."""
import ctypes as C
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

import _wide_math_ref as WM
import _wide_train_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4            # tests/test_wide_dit.py: the forward and the chains against the reference fixture
X3_VS_F32 = 2e-5      # tests/test_hip_parity.py::test_dit_forward_bf16x3_matches_f32_path
MODES = ("bf16x3", "bf16")
ENTRY = {"bf16x3": "t2s_attn_fwd_x3_n", "bf16": "t2s_attn_fwd_bf16p_n"}

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
    return m.to(dev).eval().set_wide_math(True)


@pytest.fixture(scope="module")
def models(dev):
    """One opted-in model per width; every test leaves it on f32."""
    return {W: _wide_model(dev, W) for W in (50, 64)}


def _maxdiff(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ attention alone
def _attn(dev, mode, q, k, v, N=None):
    """t2s_attn_fwd_x3_n / _bf16p_n on plain (BH,N,32) tensors (CPU or device) -> device tensor"""
    qd, kd, vd = q.to(dev).contiguous(), k.to(dev).contiguous(), v.to(dev).contiguous()
    od = torch.full_like(qd, float("nan"))
    fn = getattr(L.lib(), ENTRY[mode])
    L.check(fn(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), q.shape[0], N or q.shape[1], L.stream_ptr(dev)), ENTRY[mode])
    return od


_ATTN = {}


def _attn_case(N, n_seq, kind):
    """The constructions of tests/test_wide_dit.py::test_packed_attention_wide_vs_fp64 (same seeds), with the fp64 softmax
    and the fp64 exp2-softmax of the operands as the one-plane kernel rounds them; computed once."""
    key = (N, n_seq, kind)
    if key in _ATTN:
        return _ATTN[key]
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
        for key_, query in ((base + 3, 100), (base + 17, N - 1), (base + 31, 33)):
            k[:, key_] = q[:, query] * (270.0 / q[:, query].pow(2).sum(-1, keepdim=True))     # q . k = 270
        s2 = (q[:, 100] * k[:, base + 3]).sum(-1) * (32 ** -0.5 * 1.4426950408889634)
        assert float(s2.min()) > 68.0
    exact = torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()
    rb = lambda x: x.float().bfloat16().double()                                               # noqa: E731
    c = torch.tensor(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))         # the kernel's fp32 constant
    s = rb(q * c) @ rb(k).transpose(-1, -2)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    rounded = (p @ rb(v)) / p.sum(dim=-1, keepdim=True)
    _ATTN[key] = (q, k, v, exact, rounded)
    return _ATTN[key]


ATTN_CASES = [(N, n_seq, kind) for N in (800, 1024) for n_seq in (1, 3) for kind in ("plain", "late", "block0")]


@pytest.mark.parametrize("N,n_seq,kind", ATTN_CASES)
def test_attention_x3_wide_vs_fp64(dev, N, n_seq, kind):
    """late: the sticky reference is renewed in the LAST key block (a ring slot read before its DMA landed, or a wait counted
    for the wrong wave, shows here); block0: everything after the first block underflows against it.  Three sequences are 24
    work items over 12 heads."""
    q, k, v, exact, _ = _attn_case(N, n_seq, kind)
    o = _attn(dev, "bf16x3", q, k, v).cpu()
    assert bool(torch.isfinite(o).all())
    err = (o.double() - exact).abs()
    print(f"wide_math_errors | attention bf16x3 vs fp64 | N={N} n_seq={n_seq} {kind} | max {float(err.max()):.3e} rms {float(err.pow(2).mean().sqrt()):.3e}")
    assert float(err.max()) < 2e-5 and float(err.pow(2).mean().sqrt()) < 1e-6


@pytest.mark.parametrize("N,n_seq,kind", ATTN_CASES)
def test_attention_bf16p_wide_vs_fp64_of_the_rounded_operands(dev, N, n_seq, kind):
    q, k, v, exact, rounded = _attn_case(N, n_seq, kind)
    o = _attn(dev, "bf16", q, k, v).cpu()
    assert bool(torch.isfinite(o).all())
    err = (o.double() - rounded).abs()
    vmax = v.abs().amax(dim=(1, 2)).double()
    per_head = err.amax(dim=(1, 2))
    off = float((o.double() - exact).abs().max())
    print(f"wide_math_errors | attention bf16 vs fp64 of the rounded operands | N={N} n_seq={n_seq} {kind} | "
          f"max err / max|v| per head {float((per_head / vmax).max()):.4f} of bound {2.0 ** -8:.4f} | off the unrounded result {off:.3e}")
    assert bool((per_head <= 2.0 ** -8 * vmax).all()), (per_head / vmax).tolist()
    assert off > 1e-3           # the one-plane arithmetic, not the fp32-accurate one


_WALK = {}


def _walk_data(N, n_seq=70):
    """280 heads of N(0,1) operands; every seventh head carries a key in the last block that renews the reference of one
    query (the re-reference branch couples the two tiles of a wave: the pairing must not depend on the launch)."""
    if N not in _WALK:
        g = torch.Generator().manual_seed(N)
        q, k, v = (torch.randn(n_seq * 4, N, 32, generator=g) for _ in range(3))
        k[::7, N - 9] = q[::7, 37] * 9.0
        k[3::7, 40] = q[3::7, N - 3] * 7.0
        _WALK[N] = (q, k, v)
    return _WALK[N]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [1024, 800])
def test_persistent_walk_is_the_single_sequence_launch_bit_for_bit(dev, N, mode):
    """70 sequences = 280 heads = 560 (head, part) work items: more than one per CU, so workgroups walk several items, the
    ring stream runs across item borders and some workgroups straddle heads.  Every head equals the head of an n_seq = 1
    launch of its sequence, and a second launch repeats the bits."""
    q, k, v = (t.to(dev) for t in _walk_data(N))
    o = _attn(dev, mode, q, k, v)
    assert bool(torch.isfinite(o).all())
    assert torch.equal(o, _attn(dev, mode, q, k, v))
    for s in range(q.shape[0] // 4):
        sl = slice(4 * s, 4 * s + 4)
        o1 = _attn(dev, mode, q[sl], k[sl], v[sl])
        assert torch.equal(o1, o[sl]), f"sequence {s}"


@pytest.mark.parametrize("mode,old", [("bf16x3", "t2s_attn_fwd_x3"), ("bf16", "t2s_attn_fwd_bf16p")])
def test_n_entries_at_480_and_their_refusals(dev, mode, old):
    rs = np.random.RandomState(5)
    BH = 12
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)).to(dev) for _ in range(3))
    k[:, 410] = q[:, 200] * 12.0
    a = torch.empty_like(q)
    L.check(getattr(L.lib(), old)(q.data_ptr(), k.data_ptr(), v.data_ptr(), a.data_ptr(), BH, L.stream_ptr(dev)), old)
    assert torch.equal(a, _attn(dev, mode, q, k, v))
    fn = getattr(L.lib(), ENTRY[mode])
    for bad in (0, 32, 512, 832, 2048):
        assert fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), a.data_ptr(), 4, bad, L.stream_ptr(dev)) == -1      # T2S_E_INVALID
        msg = L.lib().t2s_last_error()
        assert f"n_tok={bad}".encode() in msg and b"480, 800 or 1024" in msg, msg


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", gen.FORWARD_CASES, ids=gen.case_key)
def test_forward_bf16x3_against_the_fixture_and_the_f32_path(gold, dev, models, case):
    key, W, B = gen.case_key(case), case["W"], case["B"]
    m = models[W]
    xc, textc, tlc, tfc = gen.forward_inputs(synth, case)
    x, text, t_long, t_float = (a.to(dev) for a in (xc, textc, tlc, tfc))

    def three():
        with torch.no_grad():
            return dict(cond=m(input=x, t=t_long, text_input=text), uncond=m(input=x, t=t_long, text_input=None),
                        cond_float=m(input=x, t=t_float, text_input=text))
    y32 = three()
    m.set_math("bf16x3")
    try:
        y3 = three()
    finally:
        m.set_math("f32")
    y32b = three()
    rec = gold["plan"]["fp32_vs_fp64"][key]
    sd = gen.wide_state_dict(synth, W)
    for name in ("cond", "uncond", "cond_float"):
        assert tuple(y3[name].shape) == (B, 64, W) and bool(torch.isfinite(y3[name]).all())
        assert torch.equal(y32[name], y32b[name]), (key, name)          # back on f32: the f32 bits
        bar = TOL if rec[name] <= 2.5e-5 else 4.0 * rec[name]
        e_gold, e_f32 = _maxdiff(y3[name], gold[f"{name}_{key}"]), _maxdiff(y3[name], y32[name])
        print(f"wide_math_errors | forward bf16x3 | {key} {name} | vs fixture {e_gold:.3e} (bar {bar:.1e}) | vs f32 path {e_f32:.3e} (bar {X3_VS_F32:.0e})")
        assert e_gold < bar, (key, name)
        assert e_f32 < X3_VS_F32, (key, name)
    # fp64-referenced errors of the three fp32-accurate forwards (printed, for profiles/wide_math_errors.md)
    for name, t, tx in (("cond", tlc, textc), ("uncond", tlc, None)):
        ref = WM.forward_fp64(sd, xc, t, tx)
        cpu = WM.forward_fp32(sd, xc, t, tx)
        print(f"wide_math_errors | fp64-referenced max abs | {key} {name} | HIP f32 {WM.err(_np(y32[name]), ref)[1]:.3e} | "
              f"HIP bf16x3 {WM.err(_np(y3[name]), ref)[1]:.3e} | CPU fp32 {WM.err(cpu, ref)[1]:.3e}")


def test_forward_bf16_meets_the_autocast_bar(dev, models):
    pool_hip = pool_bar = 0.0
    for W, B, with_text in WM.BF16_CASES:
        c = WM.bf16_case(W, B, with_text)
        m = models[W].set_math("bf16")
        try:
            with torch.no_grad():
                y = m(input=c["x"].to(dev), t=c["t"].to(dev), text_input=None if c["text"] is None else c["text"].to(dev))
        finally:
            m.set_math("f32")
        with torch.no_grad():
            y32 = m(input=c["x"].to(dev), t=c["t"].to(dev), text_input=None if c["text"] is None else c["text"].to(dev))
        assert bool(torch.isfinite(y).all())
        rms, mx = WM.err(_np(y), c["ref"])
        diff32 = float((y - y32).abs().max()) / float(y32.abs().max())
        print(f"wide_math_errors | forward bf16 | W{W} B{B} text={with_text} | HIP rms {rms:.3e} max {mx:.3e} | autocast bar rms "
              f"{c['bar_rms']:.3e} max {c['bar_max']:.3e} | ratios {rms / c['bar_rms']:.3f} {mx / c['bar_max']:.3f} | "
              f"max|bf16 - f32| / max|f32| {diff32:.3e} | absmax {c['absmax']:.2f}")
        assert rms <= WM.RMS_BAR * c["bar_rms"], (W, B, with_text, rms, c["bar_rms"])
        assert diff32 > 1e-4                     # a dispatch that fell back to f32 / bf16x3 would agree to ~1e-6
        pool_hip, pool_bar = max(pool_hip, mx), max(pool_bar, c["bar_max"])
    print(f"wide_math_errors | forward bf16 | pooled max | HIP {pool_hip:.3e} | autocast bar {pool_bar:.3e} | ratio {pool_hip / pool_bar:.3f}")
    assert pool_hip <= WM.MAX_BAR * pool_bar, (pool_hip, pool_bar)


# ------------------------------------------------------------------------------------------------ bitwise structure
@pytest.mark.parametrize("mode", MODES)
def test_rows_are_batch_invariant_and_a_cfg_pass_is_two_forwards_at_w64(dev, models, mode):
    m, B, W = models[64], 3, 64
    x = synth.make_wide_latents(77, B, W).to(dev)
    text = synth.make_text_embeddings(77, B).to(dev)
    t = torch.tensor([421, 900, 17], device=dev)
    lib, st = L.lib(), L.stream_ptr(dev)
    m.set_math(mode)
    try:
        with torch.no_grad():
            yu, yc = m(input=x, t=t, text_input=None), m(input=x, t=t, text_input=text)
            for b in range(B):
                assert torch.equal(m(input=x[b:b + 1], t=t[b:b + 1], text_input=text[b:b + 1])[0], yc[b]), b
            assert torch.equal(m(input=x[2:3], t=t[2:3], text_input=None)[0], yu[2])
            h = m.t2s_handle(dev, 2 * B)
            temb = m.time_emb(t)
            ou, oc = torch.empty_like(x), torch.empty_like(x)
            L.check(lib.t2s_dit_forward_cfg_rows(h, x.data_ptr(), temb.data_ptr(), B, text.data_ptr(), ou.data_ptr(), oc.data_ptr(), B, st))
            assert torch.equal(ou, yu) and torch.equal(oc, yc)
            t1 = torch.full((B,), 421, dtype=torch.long, device=dev)
            yu1, yc1 = m(input=x, t=t1, text_input=None), m(input=x, t=t1, text_input=text)
            L.check(lib.t2s_dit_forward_cfg(h, x.data_ptr(), m.time_emb(t1[:1]).data_ptr(), text.data_ptr(), ou.data_ptr(), oc.data_ptr(), B, st))
            assert torch.equal(ou, yu1) and torch.equal(oc, yc1)
    finally:
        m.set_math("f32")


def _mc_decoder(dev, width, channels=7):
    from model.pretrained.myvqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256, embedding_dim=64,
                                    flow_dim=width, input_dim=channels))
    v.load_state_dict(synth.make_mvae_state_dict(2025, channels, 128, 3, 256), strict=True)
    return v.to(dev).eval()


@pytest.fixture(scope="module")
def chain(dev):
    """The fixture's chain set-up (tests/test_wide_dit.py): Transformer(50) with the chain weights, x_T, text, noise."""
    c = gen.CHAIN
    m = _wide_model(dev, c["W"], c["weight_seed"], gain=c["gain"])
    xT, text, noise = gen.chain_inputs(synth)
    return m, xT.to(dev), text.to(dev), noise.to(dev), _mc_decoder(dev, c["W"]).decoder


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_chains_and_their_bitwise_forms(gold, dev, chain, backbone, mode):
    """The fixture's two 3-step CFG chains at W 50, B 2.  bf16x3: within TOL * max(1, absmax) of the reference's latent, the
    bar the f32 path is held to.  bf16: finite, its error printed (no autocast bar is computed for the chain, so none is
    asserted).  Both: eager = one-step graph = whole-loop graph = two lanes, and a guidance interval runs."""
    from t2ms_amd.sampler import Sampler
    m, xT, text, noise, dec = chain
    c = gen.CHAIN
    W, B, steps = c["W"], c["B"], c["steps"]
    want = gold["chain_ddpm_latent" if backbone == "ddpm" else "chain_rf_latent"]
    nz = noise if backbone == "ddpm" else None
    try:
        s = Sampler(m, dec, backbone, steps, c["cfg"], B, 37, dev, use_graph=False, math=mode)
        assert s.math == mode and s.width == W
        lat, series, _ = s.run(text, x_T=xT, noise=nz)
        assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(series).all())
        err, absmax = _maxdiff(lat, want), float(np.abs(want).max())
        print(f"wide_math_errors | chain {backbone} {mode} | W{W} B{B} {steps} steps | max abs vs fixture {err:.3e} | latent absmax {absmax:.2f}")
        if mode == "bf16x3":
            assert err < TOL * max(1.0, absmax)
        for kw in (dict(loop_graph=0), dict(loop_graph=1)):
            g = Sampler(m, dec, backbone, steps, c["cfg"], B, 37, dev, use_graph=True, math=mode, **kw)
            lat_g, series_g, _ = g.run(text, x_T=xT, noise=nz)
            assert g.graph_lanes == 1 and torch.equal(lat_g, lat) and torch.equal(series_g, series), kw
        x4, text4 = torch.cat([xT, xT]), torch.cat([text, text])
        nz4 = None if nz is None else torch.cat([nz, nz], dim=1)
        s4 = Sampler(m, None, backbone, steps, c["cfg"], 2 * B, 37, dev, use_graph=True, lanes=2, math=mode)
        lat4, _, _ = s4.run(text4, x_T=x4, noise=nz4, decode=False)
        assert s4.graph_lanes == 2 and torch.equal(lat4[:B], lat) and torch.equal(lat4[B:], lat)
        # guidance on a window of steps: graph = eager, and it is not the fully guided chain
        gi = [Sampler(m, None, backbone, steps, c["cfg"], B, 37, dev, use_graph=ug, math=mode, guide_steps=(0, 2))
              for ug in (False, True)]
        li = [g.run(text, x_T=xT, noise=nz, decode=False)[0] for g in gi]
        assert torch.equal(li[0], li[1]) and bool(torch.isfinite(li[0]).all()) and not torch.equal(li[0], lat)
    finally:
        m.set_math("f32")


@pytest.mark.parametrize("mode", MODES)
def test_the_planes_follow_load_state_dict(dev, mode):
    W, B = 50, 2
    x, text = synth.make_wide_latents(3, B, W).to(dev), synth.make_text_embeddings(3, B).to(dev)
    t = torch.tensor([700, 30], device=dev)
    a = _wide_model(dev, W, 2025).set_math(mode)
    with torch.no_grad():
        ya = a(input=x, t=t, text_input=text)
        hid = a.t2s_handle_id()
        a.load_state_dict(synth.make_dit_state_dict(77, width=W), strict=True)
        yb = a(input=x, t=t, text_input=text)
        assert a.t2s_handle_id() == hid                        # refreshed in place: the planes were rebuilt, not the handle
        fresh = _wide_model(dev, W, 77).set_math(mode)(input=x, t=t, text_input=text)
    assert torch.equal(yb, fresh) and not torch.equal(ya, yb)


# ------------------------------------------------------------------------------------------------ sampler and driver
def test_ragged_sampler_rows_equal_their_uniform_runs(dev, models):
    from t2ms_amd.sampler import Sampler
    m, W, B, CH = models[64], 64, 2, 7
    dec = _mc_decoder(dev, W, CH).decoder
    xT, text = synth.make_wide_latents(4, B, W).to(dev), synth.make_text_embeddings(4, B).to(dev)
    lengths = [36, 140]
    try:
        s = Sampler(m, dec, "flowmatching", 3, 7.0, B, 140, dev, math="bf16x3")
        assert s.math == "bf16x3"
        lat, rows, _ = s.run(text, x_T=xT, lengths=lengths)
        assert [tuple(r.shape) for r in rows] == [(CH, n) for n in lengths]
        for b, n in enumerate(lengths):
            u = Sampler(m, dec, "flowmatching", 3, 7.0, B, n, dev, math="bf16x3")
            lat_u, series_u, _ = u.run(text, x_T=xT)
            assert torch.equal(lat_u, lat) and torch.equal(series_u[b], rows[b]), (b, n)
        # and nobody chose: a wide model's sampler still picks f32
        m.set_math("f32")
        m.__dict__.pop("_t2s_math", None)
        assert Sampler(m, dec, "flowmatching", 3, 7.0, B, 40, dev).math == "f32"
    finally:
        m.set_math("f32")


def test_myinfer_driver_math_bf16x3(dev, tmp_path, monkeypatch):
    import myinfer
    monkeypatch.chdir(tmp_path)
    out = {}
    for math in ("f32", "bf16x3"):
        flags = ["--dataset_name", "deadlift", "--random_init", "--synthetic", "4", "--total_step", "3", "--save_path", str(tmp_path / math)]
        res = myinfer.main(flags + (["--math", math] if math != "f32" else []))
        root = os.path.join(str(tmp_path / math), "generation", "flowmatching_DiT_deadlift_3_3", "run_0")
        summary = json.load(open(os.path.join(root, "summary.json")))
        assert len(res) == 1 and len(summary["clips"]) == 4
        for i, clip in enumerate(summary["clips"]):
            x = np.load(os.path.join(root, f"sample_{i}", "x_t.npy"))
            assert x.shape[1] == clip["length"] and np.isfinite(x).all()
            assert os.path.exists(os.path.join(root, f"sample_{i}", "data.json"))
        out[math] = (summary, np.load(os.path.join(root, "sample_0", "x_t.npy")))
    assert "math" not in out["f32"][0] and out["bf16x3"][0]["math"] == "bf16x3"
    assert {k: v for k, v in out["bf16x3"][0].items() if k not in ("math", "clips", "mean_mse")} == \
           {k: v for k, v in out["f32"][0].items() if k not in ("clips", "mean_mse")}
    # both fp32-accurate: the same series to the decoder's sensitivity, not the same bits
    assert np.abs(out["f32"][1] - out["bf16x3"][1]).max() < 1e-2 * max(1.0, np.abs(out["f32"][1]).max())


# ------------------------------------------------------------------------------------------------ refusals that stay
def test_refusals_on_an_opted_in_handle(dev, models):
    lib = L.lib()
    m = models[64]
    with torch.cuda.device(dev):
        h = m.t2s_handle(dev, 4)
        assert lib.t2s_dit_latent_w(h) == 64
        for code in (L.MATH_BF16X3, L.MATH_BF16, L.MATH_F32):
            assert lib.t2s_dit_set_math(h, code) == 0
        assert lib.t2s_dit_set_math(h, L.MATH_BF16) == 0
        # training: not opted in -> refused as ever; opted in (t2s_dit_set_trainable) -> bf16 training still refused
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) != 0 and b"latent width 30" in lib.t2s_last_error()
        assert lib.t2s_dit_set_trainable(h, 1) == 0
        assert lib.t2s_dit_set_train_dtype(h, L.TRAIN_BF16) != 0 and len(lib.t2s_last_error()) > 0
        assert lib.t2s_dit_set_trainable(h, 0) == 0
        # switching the opt-in off: back on f32 (the f32 bits), and the refusal with its words
        x, t = synth.make_wide_latents(1, 1, 64).to(dev), torch.tensor([5], device=dev)
        assert lib.t2s_dit_set_wide_math(h, 0) == 0
        temb, out = m.time_emb(t), torch.empty(1, 64, 64, device=dev)
        L.check(lib.t2s_dit_forward(h, x.data_ptr(), temb.data_ptr(), 1, None, out.data_ptr(), 1, L.stream_ptr(dev)))
        for code in (L.MATH_BF16X3, L.MATH_BF16):
            assert lib.t2s_dit_set_math(h, code) != 0 and b"latent width 64" in lib.t2s_last_error()
        assert lib.t2s_dit_set_wide_math(h, 1) == 0 and lib.t2s_dit_set_math(h, L.MATH_F32) == 0
        assert lib.t2s_dit_set_wide_math(None, 1) == -1
    m.__dict__.pop("_t2s_math_applied", None)          # the handle was driven by hand: let the mirror re-apply its setting
    with torch.no_grad():
        assert torch.equal(m.set_math("f32")(input=x, t=t, text_input=None), out)
