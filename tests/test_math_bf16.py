"""The single-pass bf16 sampling arithmetic (`--math bf16`, include/t2s.h T2S_MATH_BF16): every matrix operand of the DiT
forward rounded ONCE to bf16, one v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulate; everything else fp32.

The accuracy bars are not measured on the kernels.  They are
  * for the attention kernel alone: derived (see test_attention_bf16p_kernel_vs_fp64_of_the_rounded_operands),
  * for forwards and chains: the reference's arithmetic under PyTorch's own bf16 mixed precision -- the oracle's
    `dit_forward` inside torch.autocast("cpu", dtype=torch.bfloat16), which additionally rounds the OUTPUT of every
    linear / matmul and is therefore the looser of the two -- with the two ratios DESIGN 4.4 uses for "not narrower
    than the reference's arithmetic": rms <= 1.05 x, max <= 1.25 x.
Everything structural (row invariance, graphs, lanes, shards, mixed rows, weight updates, switching) is bitwise."""
import contextlib
import glob
import os

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

RMS_BAR, MAX_BAR = 1.05, 1.25
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- CPU: the switch itself
def test_default_math_accepts_bf16_and_rejects_junk(monkeypatch):
    from t2ms_amd import sampler
    monkeypatch.setenv("T2S_DEFAULT_MATH", "bf16")
    assert sampler.default_math() == "bf16"
    for junk in ("bf16x2", "fp16", "BF16"):
        monkeypatch.setenv("T2S_DEFAULT_MATH", junk)
        with pytest.raises(ValueError):
            sampler.default_math()
    monkeypatch.delenv("T2S_DEFAULT_MATH")
    assert sampler.default_math() == sampler.DEFAULT_MATH == "bf16x3"          # no default moved


def test_infer_parser_accepts_math_bf16():
    import infer
    assert infer.build_parser().parse_args(["--math", "bf16"]).math == "bf16"
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--math", "bf16x2"])


def test_set_math_bf16_on_a_model_without_a_handle():
    from model.denoiser.transformer import Transformer
    m = Transformer()
    assert m.set_math("bf16") is m and m.__dict__["_t2s_math"] == "bf16" and m.t2s_handle_id() is None
    with pytest.raises(ValueError):
        m.set_math("bf16x2")
    assert L.MATH_BF16 == 2 and L.MATH_CODES == {"f32": 0, "bf16x3": 1, "bf16": 2}


# ---------------------------------------------------------------------------------------------- references
@contextlib.contextmanager
def fp64_arithmetic():
    """The oracle in float64 on fp32 data (tools/accuracy_table.py: fp64_arithmetic): default dtype float64; the schedule
    tables and the time embedding stay the fp32 values (computed under a float32 default, then upcast)."""
    te, dt = O.time_embedding, O.ddpm_tables

    def in_f32(fn):
        def wrapped(*a, **k):
            torch.set_default_dtype(torch.float32)
            try:
                a = [x.float() if torch.is_tensor(x) and x.is_floating_point() else x for x in a]
                r = fn(*a, **k)
            finally:
                torch.set_default_dtype(torch.float64)
            return {kk: v.double() for kk, v in r.items()} if isinstance(r, dict) else r.double()
        return wrapped

    O.time_embedding, O.ddpm_tables = in_f32(te), in_f32(dt)
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)
        O.time_embedding, O.ddpm_tables = te, dt


def _dbl(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def forward_fp64(sd, x, t, text):
    with torch.no_grad(), fp64_arithmetic():
        return O.dit_forward(_dbl(sd), x.double(), t, None if text is None else text.double()).numpy()


_ORACLE_DIT_FORWARD = O.dit_forward


def forward_autocast(sd, x, t, text):
    """The bar: the oracle's forward under PyTorch's bf16 autocast on the CPU, cast back to fp32."""
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        y = _ORACLE_DIT_FORWARD(sd, x, t, text)
    return y.float()


@contextlib.contextmanager
def only_dit_forward_under_autocast():
    """O.sample_ddpm / O.sample_rf with ONLY dit_forward under autocast: the CFG combine and the update stay fp32."""
    real = O.dit_forward
    O.dit_forward = lambda sd, x, t, text, taps=None: forward_autocast(sd, x, t, text)
    try:
        yield
    finally:
        O.dit_forward = real


def _err(x, ref):
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(np.sqrt((d ** 2).mean())), float(d.max())


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _rb(x):
    """round to nearest even bf16, as float64"""
    return x.float().bfloat16().double()


# ---------------------------------------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _dit(dev, seed=2025, math="bf16", **kw):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(seed, **kw), strict=True)
    return m.to(dev).eval().set_math(math)


@pytest.fixture(scope="module")
def dit(dev):
    return _dit(dev)


@pytest.fixture(scope="module")
def vae(dev):
    import types
    from model.pretrained.vqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    v.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    return v.to(dev).eval()


# ---------------------------------------------------------------------------------------------- 2. the attention kernel alone
@gpu
def test_attention_bf16p_kernel_vs_fp64_of_the_rounded_operands(dev):
    """t2s_attn_fwd_bf16p against an fp64 exp2-softmax of the operands AS THE KERNEL ROUNDS THEM (include/t2s.h): rb(q * c)
    with c = 32^-0.5 * log2(e) and q * c one fp32 multiplication, rb(k), rb(v).  The construction of
    test_attention_x3_kernel_vs_fp64, spikes included, so the re-reference branch runs at early and late key blocks.
    What is left is P rounded to bf16 in front of PV (the row sum adds the unrounded P, O stays fp32): with P'_j = P_j (1 + d_j)
    the error is sum_j d_j P_j v_j / sum_j P_j, a convex combination of d_j v_j, so |err| <= max|d| max|v| of the head, plus
    fp32 accumulation (~1e-6 here).  The bound asserted is 2^-8 max|v| per head -- derived, not measured.  (2^-8 is the
    unit roundoff of bf16's 8-bit significand, reached just above a power of two; just below one it is 2^-9.  Reaching the
    bound would take every d_j at its maximum with the sign of v_j; on this data the kernel sits at 0.37 ... 0.73 of it.)"""
    rs = np.random.RandomState(21)
    BH = 12
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 333] = q[:, 100] * 5.0
    k[:, 410] = q[:, 200] * 12.0
    k[:, 0:32] = -q[:, 7:8] * 3.0 + 0.01 * k[:, 0:32]
    k[:, 448] = q[:, 7] * 10.0
    c = torch.tensor(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))     # the kernel's fp32 constant
    s = _rb(q * c) @ _rb(k).transpose(-1, -2)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    ref = (p @ _rb(v)) / p.sum(dim=-1, keepdim=True)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    od = torch.empty_like(qd)
    L.check(L.lib().t2s_attn_fwd_bf16p(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), BH, L.stream_ptr(dev)),
            "t2s_attn_fwd_bf16p")
    err = (od.cpu().double() - ref).abs()
    vmax = v.abs().amax(dim=(1, 2)).double()
    per_head = err.amax(dim=(1, 2))
    print("attention bf16p: max err / max|v| per head", (per_head / vmax).tolist(), "bound", 2.0 ** -8,
          "rms", float(err.pow(2).mean().sqrt()))
    assert bool(torch.isfinite(od).all())
    assert bool((per_head <= 2.0 ** -8 * vmax).all()), (per_head / vmax).tolist()
    # and it is the one-plane arithmetic, not the fp32-accurate one: against the UNROUNDED operands it is off by far more
    exact = torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()
    assert float((od.cpu().double() - exact).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 3. one forward: the accuracy bar
ENTRIES = [(1, 500, True), (3, 10, True), (7, 999, False), (7, 250, True), (3, 0, False), (1, 999, True)]   # (B, t, cond)


@gpu
def test_forward_meets_the_autocast_bar_and_is_a_different_arithmetic(dev, dit):
    """Errors against the oracle in fp64 on the same fp32 data; the bar is the oracle under torch.autocast(bfloat16):
    rms <= 1.05 x per entry, max <= 1.25 x with the max pooled over the entries.  Entries: cond / uncond at several t for
    B in {1, 3, 7}, and one B = 256 forward checked on 8 sampled rows."""
    sd = synth.make_dit_state_dict(2025)
    f32 = _dit(dev, math="f32")
    cases = []
    for B, tval, cond in ENTRIES:
        x, text = synth.make_latents(900 + B, B), synth.make_text_embeddings(900 + B, B)
        cases.append((f"B={B} t={tval} {'cond' if cond else 'uncond'}", x, torch.full((B,), tval, dtype=torch.long),
                      text if cond else None, slice(None)))
    rows = [0, 1, 63, 64, 130, 191, 254, 255]
    cases.append(("B=256 t=500 cond, 8 rows", synth.make_latents(4242, 256), torch.full((256,), 500, dtype=torch.long),
                  synth.make_text_embeddings(4242, 256), rows))
    pool_hip, pool_bar = 0.0, 0.0
    for name, x, t, text, sel in cases:
        with torch.no_grad():
            td = None if text is None else text.to(dev)
            y = dit(input=x.to(dev), t=t.to(dev), text_input=td)
            y32 = f32(input=x.to(dev), t=t.to(dev), text_input=td)
        xs, ts, tx = x[sel].contiguous(), t[sel].contiguous(), None if text is None else text[sel].contiguous()
        ref = forward_fp64(sd, xs, ts, tx)
        rms_bar, max_bar = _err(_np(forward_autocast(sd, xs, ts, tx)), ref)
        rms_hip, max_hip = _err(_np(y[sel]), ref)
        diff32 = float((y - y32).abs().max()) / float(y32.abs().max())
        print(f"forward {name}: HIP bf16 rms {rms_hip:.3e} max {max_hip:.3e} | autocast oracle rms {rms_bar:.3e} max {max_bar:.3e} | "
              f"ratios {rms_hip / rms_bar:.3f} {max_hip / max_bar:.3f} | max|bf16 - f32| / max|f32| {diff32:.3e} | max|ref| {np.abs(ref).max():.3g}")
        assert bool(torch.isfinite(y).all())
        assert rms_hip <= RMS_BAR * rms_bar, (name, rms_hip, rms_bar)
        assert diff32 > 1e-4, (name, diff32)       # a dispatch that silently fell back to f32 / bf16x3 agrees to ~4e-6
        pool_hip, pool_bar = max(pool_hip, max_hip), max(pool_bar, max_bar)
    print(f"forward, pooled max: HIP {pool_hip:.3e} autocast oracle {pool_bar:.3e} ratio {pool_hip / pool_bar:.3f}")
    assert pool_hip <= MAX_BAR * pool_bar, (pool_hip, pool_bar)


# ---------------------------------------------------------------------------------------------- 4. row invariance, bitwise
@gpu
def test_rows_are_batch_invariant_and_a_cfg_pass_is_two_forwards_bitwise(dev, dit):
    B = 256
    x = synth.make_latents(4242, B).to(dev)
    text = synth.make_text_embeddings(4242, B).to(dev)
    t = torch.full((B,), 999, dtype=torch.long, device=dev)
    with torch.no_grad():
        h = dit.t2s_handle(dev, 2 * B)
        temb = dit.time_emb(t[:1])
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        L.check(L.lib().t2s_dit_forward_cfg(h, x.data_ptr(), temb.data_ptr(), text.data_ptr(), ou.data_ptr(), oc.data_ptr(), B,
                                            L.stream_ptr(dev)))
        rows = [0, 1, 130, 255]
        small_c = dit(input=x[rows].contiguous(), t=t[:4], text_input=text[rows].contiguous())
        small_u = dit(input=x[rows].contiguous(), t=t[:4], text_input=None)
        assert torch.equal(oc[rows], small_c) and torch.equal(ou[rows], small_u)
        assert bool(torch.isfinite(oc).all()) and bool(torch.isfinite(ou).all())
        # a CFG pass == two plain forwards, at an odd batch
        B = 5
        x, text, t = x[:B].contiguous(), text[:B].contiguous(), torch.full((B,), 421, dtype=torch.long, device=dev)
        yu, yc = dit(input=x, t=t, text_input=None), dit(input=x, t=t, text_input=text)
        h = dit.t2s_handle(dev, 2 * B)
        temb = dit.time_emb(t[:1])
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        L.check(L.lib().t2s_dit_forward_cfg(h, x.data_ptr(), temb.data_ptr(), text.data_ptr(), ou.data_ptr(), oc.data_ptr(), B,
                                            L.stream_ptr(dev)))
    assert torch.equal(ou, yu) and torch.equal(oc, yc)


# ---------------------------------------------------------------------------------------------- 5. the sampler, bitwise
@gpu
@pytest.mark.parametrize("backbone,steps,cfg,B", [("flowmatching", 20, 5.0, 64), ("ddpm", 12, 9.0, 7)])
def test_step_graph_whole_loop_graph_and_eager_agree_bitwise(dev, dit, vae, backbone, steps, cfg, B):
    from t2ms_amd.sampler import Sampler
    text = synth.make_text_embeddings(3, B).to(dev)
    ref = Sampler(dit, vae.decoder, backbone, steps, cfg, B, 96, dev, use_graph=False, seed=9, math="bf16").run(text)
    assert bool(torch.isfinite(ref[1]).all())
    for lanes in (1, 2):
        for loop_graph in (0, 1):
            s = Sampler(dit, vae.decoder, backbone, steps, cfg, B, 96, dev, use_graph=True, seed=9, lanes=lanes, loop_graph=loop_graph,
                        math="bf16")
            assert s.math == "bf16"
            lat, ser, _ = s.run(text)
            assert s.graph_lanes == lanes                                  # the new kernels were captured, per lane
            assert torch.equal(lat, ref[0]) and torch.equal(ser, ref[1]), (backbone, lanes, loop_graph)
            lat2, ser2 = s.run_inplace()                                   # the replay
            assert torch.equal(lat2, ref[0]) and torch.equal(ser2, ref[1]), (backbone, lanes, loop_graph)
    # and the chain really ran in another arithmetic than f32
    f = Sampler(_dit(dev, math="f32"), vae.decoder, backbone, steps, cfg, B, 96, dev, use_graph=True, seed=9, math="f32").run(text)
    assert not torch.equal(f[0], ref[0])
    dit.set_math("bf16")


@gpu
def test_two_lanes_equal_one_lane_bitwise(dev, dit, vae):
    from t2ms_amd.sampler import Sampler
    B = 37                                                                 # odd: 19 + 18 rows
    text = synth.make_text_embeddings(5, B)
    ref = None
    for lanes, use_graph in ((1, True), (2, True), (2, False), (3, True)):
        s = Sampler(dit, vae.decoder, "ddpm", 6, 9.0, B, 96, dev, use_graph=use_graph, seed=11, row0=100, lanes=lanes, math="bf16")
        lat, series, _ = s.run(text)
        if ref is None:
            ref = (lat, series)
            assert bool(torch.isfinite(series).all())
        else:
            assert torch.equal(lat, ref[0]) and torch.equal(series, ref[1]), (lanes, use_graph)
    for B in (128, 32):                                                    # the automatic two lanes, rectified flow
        text = synth.make_text_embeddings(6, B)
        outs = []
        for lanes in (1, 0):
            s = Sampler(dit, vae.decoder, "flowmatching", 4, 5.0, B, 96, dev, seed=3, lanes=lanes, math="bf16")
            outs.append(s.run(text)[:2])
            assert s.graph_lanes == (1 if lanes == 1 else 2)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), B


@gpu
def test_shards_equal_the_full_batch_bitwise(dev, dit, vae):
    """set_row0 (strong-scaling shards, one sampler moved along) and set_rows (per-row keys) against the unsharded batch."""
    from t2ms_amd.sampler import Sampler
    steps, B = 8, 64
    text = synth.make_text_embeddings(2025, B)
    lat, ser, _ = Sampler(dit, vae.decoder, "ddpm", steps, 9.0, B, 96, dev, use_graph=True, seed=2025, row0=0, math="bf16").run(text)
    assert bool(torch.isfinite(ser).all())
    for world in (2, 4):
        n = B // world
        s = Sampler(dit, vae.decoder, "ddpm", steps, 9.0, n, 96, dev, use_graph=True, seed=2025, row0=0, math="bf16")
        for rank in range(world):
            s.set_row0(rank * n)
            la, sa, _ = s.run(text[rank * n:(rank + 1) * n].contiguous())
            assert torch.equal(la, lat[rank * n:(rank + 1) * n]) and torch.equal(sa, ser[rank * n:(rank + 1) * n]), (world, rank)
    n = 16
    s = Sampler(dit, vae.decoder, "ddpm", steps, 9.0, n, 96, dev, use_graph=True, seed=1, row0=0, math="bf16")
    s.set_rows(np.full(n, 2025, dtype=np.uint64), 40 + np.arange(n), np.full(n, 9.0, dtype=np.float32))
    la, sa, _ = s.run(text[40:40 + n].contiguous())
    assert torch.equal(la, lat[40:40 + n]) and torch.equal(sa, ser[40:40 + n])


STEPS, LEN = 4, 48
CELLS = ((5, 11, 0, 5.0), (3, 12, 3, 9.0), (6, 11, 20, 7.5))        # (rows, seed, row0, cfg), as tests/test_grid_sampling.py
MODES = {"eager": dict(use_graph=False), "step_graph": dict(use_graph=True, loop_graph=0), "loop_graph": dict(use_graph=True, loop_graph=1)}


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_mixed_rows_equal_uniform_samplers_per_cell(dev, vae, backbone, mode, lanes):
    """One grid launch with rows of different runs, positions and guidance scales == uniform samplers per cell."""
    from t2ms_amd.sampler import Sampler
    m = _dit(dev, 31337, gain=0.7)
    B = sum(c[0] for c in CELLS)
    text = synth.make_text_embeddings(5, B).to(dev)
    mixed = Sampler(m, vae.decoder, backbone, STEPS, 1.0, B, LEN, dev, seed=999, row0=77, lanes=lanes, math="bf16", **MODES[mode])
    mixed.set_rows(np.concatenate([np.full(n, s, dtype=np.uint64) for n, s, _, _ in CELLS]),
                   np.concatenate([r0 + np.arange(n) for n, _, r0, _ in CELLS]).astype(np.uint32),
                   np.concatenate([np.full(n, c, dtype=np.float32) for n, _, _, c in CELLS]))
    lat, ser, _ = mixed.run(text)
    r = 0
    for n, seed, row0, cfg in CELLS:
        ref = Sampler(m, vae.decoder, backbone, STEPS, cfg, n, LEN, dev, seed=seed, row0=row0, lanes=1, math="bf16", **MODES[mode])
        la, sa, _ = ref.run(text[r:r + n].contiguous())
        assert torch.equal(lat[r:r + n], la) and torch.equal(ser[r:r + n], sa), (backbone, mode, lanes, seed, row0, cfg)
        r += n


# ---------------------------------------------------------------------------------------------- 6. chains against the reference
@gpu
@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_chain_golden_within_the_autocast_bar(golden_dir, dev, vae, backbone):
    """The reference-generated 20-step chains (tests/golden/chains.npz) with math="bf16" and decode, through the captured
    graph.  Bar: O.sample_ddpm / O.sample_rf on the CPU with only dit_forward under bf16 autocast, its rms / max error against
    the golden latents (and, through O.vae_decode, the golden series); the HIP result must stay within 1.05 x / 1.25 x."""
    from t2ms_amd.sampler import Sampler
    g = {k: v for k, v in np.load(os.path.join(golden_dir, "chains.npz")).items()}
    sd = synth.make_dit_state_dict(31337, gain=0.7)
    xT, text = synth.make_latents(31337, 4), synth.make_text_embeddings(31337, 4)
    noises = torch.from_numpy(np.random.RandomState(99).randn(20, 4, 64, 30).astype(np.float32))
    m = _dit(dev, 31337, gain=0.7)
    s = Sampler(m, vae.decoder, backbone, 20, 7.0, 4, 96, dev, use_graph=True, math="bf16")
    key = "ddpm" if backbone == "ddpm" else "rf"
    lat, series, _ = s.run(text, x_T=xT, noise=noises if key == "ddpm" else None)
    assert s.graph_lanes >= 1 and bool(torch.isfinite(lat).all()) and bool(torch.isfinite(series).all())
    with torch.no_grad(), only_dit_forward_under_autocast():
        bar_lat = O.sample_ddpm(sd, xT, text, 20, 7.0, noises) if key == "ddpm" else O.sample_rf(sd, xT, text, 20, 7.0)
    with torch.no_grad():
        bar_series = O.vae_decode(synth.make_vae_state_dict(2025), bar_lat, 96)[0]
    for what, got, bar, gold in (("latent", lat, bar_lat, g[key + "_latent"]), ("series", series, bar_series, g[key + "_series"])):
        rms_hip, max_hip = _err(_np(got), gold)
        rms_bar, max_bar = _err(_np(bar), gold)
        print(f"20-step {key} chain, {what}: HIP bf16 rms {rms_hip:.3e} max {max_hip:.3e} | autocast oracle rms {rms_bar:.3e} max {max_bar:.3e} | "
              f"ratios {rms_hip / rms_bar:.3f} {max_hip / max_bar:.3f} | max|golden| {np.abs(gold).max():.3g}")
        assert rms_hip <= RMS_BAR * rms_bar, (what, rms_hip, rms_bar)
        assert max_hip <= MAX_BAR * max_bar, (what, max_hip, max_bar)


# ---------------------------------------------------------------------------------------------- 7. / 8. weights and switching
@gpu
def test_bf16_follows_weight_updates_bitwise(dev):
    """The one-plane weight pieces are rebuilt by t2s_dit_update_weights: after load_state_dict the forward equals a fresh
    handle's, bit for bit."""
    m = _dit(dev, 2025)
    x = synth.make_latents(5, 3).to(dev)
    t = torch.tensor([1, 500, 999], device=dev)
    text = synth.make_text_embeddings(5, 3).to(dev)
    with torch.no_grad():
        y0 = m(input=x, t=t, text_input=text)
        hid = m.t2s_handle_id()
        m.load_state_dict(synth.make_dit_state_dict(7), strict=True)
        y1 = m(input=x, t=t, text_input=text)
        assert m.t2s_handle_id() == hid                                    # the same handle, refreshed
        fresh = _dit(dev, 7)(input=x, t=t, text_input=text)
    assert torch.equal(y1, fresh) and float((y0 - y1).abs().max()) > 1e-3


@gpu
def test_switching_between_the_three_arithmetics_on_one_handle(dev):
    """f32 -> bf16 -> bf16x3 -> bf16 -> f32 on ONE handle: every result equals a fresh handle's in that mode, bit for bit
    (the three workspaces neither alias nor go stale), also across a weight update made while another mode was selected."""
    B = 3
    x = synth.make_latents(5, B).to(dev)
    t = torch.tensor([3, 500, 999], device=dev)
    text = synth.make_text_embeddings(5, B).to(dev)
    with torch.no_grad():
        want = {k: _dit(dev, 2025, math=k)(input=x, t=t, text_input=text) for k in ("f32", "bf16x3", "bf16")}
        want7 = {k: _dit(dev, 7, math=k)(input=x, t=t, text_input=text) for k in ("bf16x3", "bf16")}
        m = _dit(dev, 2025, math="f32")
        hid = None
        for k in ("f32", "bf16", "bf16x3", "bf16", "f32"):
            y = m.set_math(k)(input=x, t=t, text_input=text)
            hid = hid or m.t2s_handle_id()
            assert m.t2s_handle_id() == hid and torch.equal(y, want[k]), k
        m.load_state_dict(synth.make_dit_state_dict(7), strict=True)        # refreshed while f32 is selected
        m(input=x, t=t, text_input=text)
        for k in ("bf16", "bf16x3"):
            assert torch.equal(m.set_math(k)(input=x, t=t, text_input=text), want7[k]), k
    assert not torch.equal(want["bf16"], want["bf16x3"]) and not torch.equal(want["bf16"], want["f32"])


@gpu
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_first_use_packs_behind_a_weight_update_on_a_side_stream(dev, mode):
    """A bf16 mode's FIRST use right behind a t2s_dit_update_weights that was enqueued on a non-default (non-blocking) stream:
    the planes are packed on the library's set-up stream, which nothing but the handle's event orders after that update.
    The side stream is kept busy first (elementwise passes over 512 MiB, some tens of ms), so that the update is still
    PENDING when set_math packs: a pack that does not wait reads the seed-2025 weights and the comparison fails."""
    B = 3
    x = synth.make_latents(5, B).to(dev)
    t = torch.tensor([3, 500, 999], device=dev)
    text = synth.make_text_embeddings(5, B).to(dev)
    busy = torch.zeros(1 << 27, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.no_grad():
        want = _dit(dev, 7, math=mode)(input=x, t=t, text_input=text)
        m = _dit(dev, 2025, math="f32")
        m(input=x, t=t, text_input=text)                                   # the handle exists, no plane is allocated
        hid = m.t2s_handle_id()
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            m.load_state_dict(synth.make_dit_state_dict(7), strict=True)
            for _ in range(64):
                busy.add_(1.0)
            m(input=x, t=t, text_input=text)                               # t2s_dit_update_weights, on the side stream
            y = m.set_math(mode)(input=x, t=t, text_input=text)            # first use: allocate and pack
        side.synchronize()
    assert m.t2s_handle_id() == hid and torch.equal(y, want), mode


# ---------------------------------------------------------------------------------------------- 9. the driver
@gpu
def test_infer_driver_math_bf16(dev, tmp_path, monkeypatch, capsys):
    """infer.py --math bf16 writes the four files, finite, in the shapes of the --math f32 run; the data and its encoding are
    byte-identical (only the DiT arithmetic changes), the sampled latents are not."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    files = ("x_1.npy", "x_t.npy", "x_t_latent_dec_array.npy", "x_t_latent_enc_array.npy")
    got = {}
    for math in ("f32", "bf16"):
        save = str(tmp_path / math)
        drv.main(["--dataset_name", "ETTh1_24", "--backbone", "ddpm", "--total_step", "10", "--batch_size", "4", "--save_path", save,
                  "--synthetic", "64", "--random_init", "--seed", "11", "--math", math])
        out = glob.glob(os.path.join(save, "generation", "*"))
        assert len(out) == 1, out
        got[math] = {f: np.load(os.path.join(out[0], f)) for f in files}
    assert "matrix arithmetic: bf16 (single-pass bf16" in capsys.readouterr().out
    for f in files:
        a, b = got["f32"][f], got["bf16"][f]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.isfinite(b).all(), f
    assert got["bf16"]["x_t.npy"].shape == (64, 24, 1)
    for f in ("x_1.npy", "x_t_latent_enc_array.npy"):
        assert got["f32"][f].tobytes() == got["bf16"][f].tobytes(), f
    assert not np.array_equal(got["f32"]["x_t_latent_dec_array.npy"], got["bf16"]["x_t_latent_dec_array.npy"])


# ---------------------------------------------------------------------------------------------- 10. the C ABI
@gpu
def test_new_symbol_is_exported_and_unknown_modes_are_refused(dev, dit):
    lib = L.lib()
    assert "t2s_attn_fwd_bf16p" in L.SYMBOLS and hasattr(lib, "t2s_attn_fwd_bf16p")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2s.h")).read()
    assert "#define T2S_MATH_BF16 2" in hdr and "t2s_attn_fwd_bf16p(" in hdr
    h = dit.t2s_handle(dev, 4)
    with torch.cuda.device(dev):
        assert lib.t2s_dit_set_math(h, 3) == -1                           # T2S_E_INVALID
        assert lib.t2s_dit_set_math(h, -1) != 0
        assert b"unknown mode" in lib.t2s_last_error()
        assert lib.t2s_dit_set_math(h, L.MATH_BF16) == 0
        # the stand-alone entry refuses what t2s_attn_fwd_x3 refuses
        assert lib.t2s_attn_fwd_bf16p(None, None, None, None, 4, None) != 0
        assert lib.t2s_attn_fwd_bf16p(1, 1, 1, 1, 6, None) != 0
