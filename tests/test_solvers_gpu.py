"""The few-step solvers on the GPU: t2s_lms_step (the table-driven linear multistep update) against fp64 numpy, its Philox
draw and zero-coefficient rule, the solvers' closed form through the kernel, chains with the real DiT against the oracle in
fp64, the sampler's bitwise properties in T2S_MODE_LMS, the refusals of the two create entries, and infer.py --solver."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth
from test_solvers_host import CLOSED_FORM, SIG, T_CF, X_T, _alpha_bar, _textbook_ddpm, closed_form_ddpm, closed_form_flow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vae(dev):
    import types
    from model.pretrained.vqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    v.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    return v.to(dev).eval()


CHAIN_SEED, CHAIN_GAIN = 31337, 0.7       # the synthetic weights of tests/test_hip_parity.py::_chain_setup


@pytest.fixture(scope="module")
def model(dev):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(CHAIN_SEED, gain=CHAIN_GAIN), strict=True)
    return m.to(dev).eval()


def _lms(x, hist, u, c, noise, coef, index, cfg=0.0, seed=0, sid=0, row0=0):
    from t2ms_amd.sampler import lms_step
    lms_step(x, hist, u, c, coef, index, cfg=cfg, noise=noise, seed=seed, stream_id=sid, row0=row0)


# ---------------------------------------------------------------------------------------------- the kernel against fp64
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("B", [1, 3, 53])      # 53: the first batch past one grid-stride sweep (96 x 256 quads = 51.2 rows)
def test_lms_step_vs_fp64(dev, B, with_c):
    """All six coefficients non-zero, injected noise, CFG 7.  Bar: 4 ulp of the largest term per element, an ulp being the
    fp32 spacing (np.spacing) at that term; the terms are c0*x, c2*h, c3*z and, through c1 (c5), the CFG combine's u and
    cfg*(c-u).  The kernel evaluates in fp64 and rounds once: measured <= 2.0 ulp (a result can be four times its largest
    term); a sum in fp32 reached 6.25 ulp at B = 53 (profiles/EXPERIMENTS.md 0.18)."""
    rs = np.random.RandomState(100 + B)
    x, h, u, c, z = (rs.randn(B, 1920).astype(np.float32) for _ in range(5))
    coef = np.array([[9, 9, 9, 9, 9, 9], [0.83, -1.7, 0.41, 0.6, 1.3, -0.9], [9, 9, 9, 9, 9, 9]], dtype=np.float32)
    cfg = 7.0
    k = coef[1].astype(np.float64)
    X, H, U, Cc, Z = (a.astype(np.float64) for a in (x, h, u, c, z))
    pred = U + cfg * (Cc - U) if with_c else U
    want_x = k[0] * X + k[1] * pred + k[2] * H + k[3] * Z
    want_h = k[4] * X + k[5] * pred
    # the terms that are rounded: the CFG combine's two products enter through c1 (and c5)
    pterms = [np.abs(U), np.abs(cfg * (Cc - U))] if with_c else [np.abs(U)]
    big_x = np.max([np.abs(k[0] * X), np.abs(k[2] * H), np.abs(k[3] * Z)] + [np.abs(k[1]) * p for p in pterms], axis=0)
    big_h = np.max([np.abs(k[4] * X)] + [np.abs(k[5]) * p for p in pterms], axis=0)
    xd, hd, ud, cd, zd = (torch.from_numpy(a).to(dev) for a in (x, h, u, c, z))
    _lms(xd, hd, ud, cd if with_c else None, zd, torch.from_numpy(coef).to(dev), 1, cfg=cfg)
    ex = np.abs(xd.cpu().numpy().astype(np.float64) - want_x) / np.spacing(big_x.astype(np.float32)).astype(np.float64)
    eh = np.abs(hd.cpu().numpy().astype(np.float64) - want_h) / np.spacing(big_h.astype(np.float32)).astype(np.float64)
    print(f"B={B} pred_c={with_c}: max error x' {ex.max():.2f} ulp, h' {eh.max():.2f} ulp of the largest term")
    assert ex.max() <= 4.0 and eh.max() <= 4.0


@pytest.mark.parametrize("B,row0", [(3, 1000), (53, 7)])
def test_philox_through_lms_step_is_the_library_stream(dev, B, row0):
    from t2ms_amd.sampler import philox_normal
    seed, sid = 2025, 17
    rs = np.random.RandomState(1)
    x, h, u = (torch.from_numpy(rs.randn(B, 1920).astype(np.float32)).to(dev) for _ in range(3))
    coef = torch.tensor([[0, 0, 0, 1, 0, 0]], dtype=torch.float32, device=dev)
    _lms(x, h, u, None, None, coef, 0, seed=seed, sid=sid, row0=row0)
    assert torch.equal(x, philox_normal(B, 1920, seed, sid, row0, dev))


def test_zero_coefficient_rule(dev):
    rs = np.random.RandomState(2)
    B = 5
    x0, u, c = (torch.from_numpy(rs.randn(B, 1920).astype(np.float32)).to(dev) for _ in range(3))
    nan = torch.full((B, 1920), float("nan"), device=dev)
    # c2 == 0: a history full of NaN is not read; c4 = c5 = 0: it is not written either (the NaN survive as a sentinel)
    coef = torch.tensor([[0.9, -0.3, 0, 0, 0, 0], [0.9, -0.3, 0, 0, 1.5, -0.5], [0.9, -0.3, 0.2, 0, 0, 0]], dtype=torch.float32, device=dev)
    x, h = x0.clone(), nan.clone()
    _lms(x, h, u, c, None, coef, 0, cfg=3.0)
    assert bool(torch.isfinite(x).all()) and bool(torch.isnan(h).all())
    sentinel = torch.full((B, 1920), 12345.0, device=dev)
    x, h = x0.clone(), sentinel.clone()
    _lms(x, h, u, c, None, coef, 0, cfg=3.0)
    assert torch.equal(h, sentinel)
    # c3 == 0 and noise NULL == c3 == 0 with a noise array of NaN (no draw is made, the array is not read)
    a, b = x0.clone(), x0.clone()
    _lms(a, sentinel.clone(), u, c, None, coef, 0, cfg=3.0)
    _lms(b, sentinel.clone(), u, c, nan, coef, 0, cfg=3.0)
    assert torch.equal(a, b) and torch.equal(a, x)
    # the history IS written from the OLD x when c4 / c5 say so, and read when c2 does
    x, h = x0.clone(), nan.clone()
    _lms(x, h, u, None, None, coef, 1)
    assert torch.allclose(h, 1.5 * x0 - 0.5 * u, rtol=1e-6, atol=1e-6)
    x2, h2 = x0.clone(), h.clone()
    _lms(x2, h2, u, None, None, coef, 2)
    assert torch.allclose(x2, 0.9 * x0 - 0.3 * u + 0.2 * h, rtol=1e-5, atol=1e-6) and torch.equal(h2, h)


# ---------------------------------------------------------------------------------------------- closed form through the kernel
@pytest.mark.parametrize("solver,S", [("dpmpp2m", 40), ("ddim", 40), ("ab2", 20)])
def test_closed_form_through_the_kernel(dev, solver, S):
    """Gaussian data (tests/test_solvers_host.py): the analytic eps / v computed by torch on the device, the update by
    t2s_lms_step.  Agrees with the CPU table run to 1e-5 relative and shows the solver's error of the table to 1 %."""
    from t2ms_amd.sampler import loop_t_values, solver_tables
    x = torch.from_numpy(np.repeat(X_T[:, None], 1920, axis=1).astype(np.float32)).to(dev)      # 3 rows of 1920 values
    h = torch.full_like(x, float("nan"))
    if solver == "ab2":
        tv, coef = solver_tables("flowmatching", solver, S)
        cpu, _ = closed_form_flow(solver, S)
        exact, n = SIG * X_T, S
        tvals = loop_t_values("flowmatching", S).numpy().astype(np.float64)
        scal = [(t * SIG ** 2 - (1 - t)) / (t ** 2 * SIG ** 2 + (1 - t) ** 2) for t in tvals]
    else:
        ab = _alpha_bar(T_CF)
        tv, coef = solver_tables("ddpm", solver, T_CF, S)
        cpu, _ = closed_form_ddpm(solver, S)
        tau = tv.numpy().astype(np.int64)
        n = tau.tolist().index(99)
        exact = X_T * np.sqrt(ab[99] * SIG ** 2 + 1 - ab[99]) / np.sqrt(ab[T_CF - 1] * SIG ** 2 + 1 - ab[T_CF - 1])
        scal = [np.sqrt(1 - ab[t]) / (ab[t] * SIG ** 2 + 1 - ab[t]) for t in tau]
    cd = coef.to(dev)
    for i in range(n):
        pred = x * float(scal[i])                                   # the exact denoiser, fp32 on the device
        _lms(x, h, pred, None, None, cd, i)
    got = x.cpu().numpy().astype(np.float64)
    assert (got == got[:, :1]).all()                                # every element of a row took the same path
    rel_cpu = float(np.abs((got[:, 0] - cpu) / cpu).max())
    err = float(np.abs((got[:, 0] - exact) / exact).max())
    print(f"{solver} S={S}: kernel against the CPU table run {rel_cpu:.2e} relative; solver error {err:.4e} "
          f"(table {CLOSED_FORM[(solver, S)]:.3e})")
    assert rel_cpu <= 1e-5
    assert abs(err - CLOSED_FORM[(solver, S)]) <= 0.01 * CLOSED_FORM[(solver, S)]


# ---------------------------------------------------------------------------------------------- chains with the real DiT
@contextlib.contextmanager
def _fp64_arithmetic():
    """The oracle in float64 on fp32 data, as tools/accuracy_table.py runs it: default dtype float64, the time embedding
    stays the fp32 value (computed under a float32 default, then upcast)."""
    te = O.time_embedding

    def in_f32(*a, **k):
        torch.set_default_dtype(torch.float32)
        try:
            r = te(*[v.float() if torch.is_tensor(v) and v.is_floating_point() else v for v in a], **k)
        finally:
            torch.set_default_dtype(torch.float64)
        return r.double()

    O.time_embedding = in_f32
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)
        O.time_embedding = te


CHAIN_CASES = {"ddim": ("ddpm", "ddim", 100, 8, 0.0), "ddim_eta": ("ddpm", "ddim", 100, 8, 0.5),
               "dpmpp2m": ("ddpm", "dpmpp2m", 100, 8, 0.0), "ab2": ("flowmatching", "ab2", 10, None, 0.0)}
CHAIN_B, CHAIN_CFG = 4, 7.0


def _chain_inputs():
    xT = synth.make_latents(CHAIN_SEED, CHAIN_B)
    text = synth.make_text_embeddings(CHAIN_SEED, CHAIN_B)
    noises = torch.from_numpy(np.random.RandomState(99).randn(20, CHAIN_B, 64, 30).astype(np.float32))
    return xT, text, noises


def _restated_chain(case, dtype):
    """The solver restated in its textbook form (not the collapsed table) around the oracle's dit_forward, every tensor in
    `dtype`; the schedule is the fp32 alpha_bar, its algebra fp64 scalars."""
    from t2ms_amd.sampler import loop_t_values, solver_grid
    backbone, solver, T, S, eta = CHAIN_CASES[case]
    sd = synth.make_dit_state_dict(CHAIN_SEED, gain=CHAIN_GAIN)
    xT, text, noises = _chain_inputs()
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x, text, noises = xT.to(dtype), text.to(dtype), noises.to(dtype)
    prev = None
    with torch.no_grad(), (_fp64_arithmetic() if dtype == torch.float64 else contextlib.nullcontext()):
        if backbone == "flowmatching":
            tv = loop_t_values(backbone, T)
            for j in range(T):
                t = tv[j].repeat(CHAIN_B)
                u, c = O.dit_forward(sd, x, t, None), O.dit_forward(sd, x, t, text)
                v = u + CHAIN_CFG * (c - u)
                x, prev = x + (v if j == 0 else 1.5 * v - 0.5 * prev) / T, v
            return x
        ab, tau = _alpha_bar(T), solver_grid(T, S)
        for i in range(S):
            t = torch.full((CHAIN_B,), int(tau[i]), dtype=torch.long)
            u, c = O.dit_forward(sd, x, t, None), O.dit_forward(sd, x, t, text)
            eps = u + CHAIN_CFG * (c - u)
            x, prev = _textbook_ddpm(solver, ab, tau, i, x, eps, prev, noises[i], eta)
    return x


_CHAIN_REF = {}


def _chain_reference(case):
    """(fp64 restatement, e32 = max-abs error of the fp32 restatement against it), computed once per case."""
    if case not in _CHAIN_REF:
        r64 = _restated_chain(case, torch.float64).numpy()
        r32 = _restated_chain(case, torch.float32).numpy().astype(np.float64)
        _CHAIN_REF[case] = (r64, float(np.abs(r32 - r64).max()))
    return _CHAIN_REF[case]


@pytest.mark.parametrize("case,math", [("ddim", "f32"), ("ddim_eta", "f32"), ("dpmpp2m", "f32"), ("ab2", "f32"),
                                       ("dpmpp2m", "bf16x3")])
def test_chain_with_the_real_dit(dev, vae, case, math):
    """B = 4, L = 96, cfg 7, synthetic weights.  The bar is measured, not fixed: the HIP chain's max-abs error against the
    fp64 restatement must be <= 3 x that of the same restatement with the oracle in fp32 on the CPU (two fp32 summation
    orders differ in their maximum over only 4 x 1920 values by more than the 1.25 x the project allows at 768 rows)."""
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    backbone, solver, T, S, eta = CHAIN_CASES[case]
    r64, e32 = _chain_reference(case)
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(CHAIN_SEED, gain=CHAIN_GAIN), strict=True)
    m = m.to(dev).eval()
    xT, text, noises = _chain_inputs()
    s = Sampler(m, vae.decoder, backbone, T, CHAIN_CFG, CHAIN_B, 96, dev, math=math, solver=solver, sample_steps=S, eta=eta)
    assert s.steps == (S or T)
    lat, series, _ = s.run(text, x_T=xT, noise=noises[:s.steps] if eta else None)
    err = float(np.abs(lat.cpu().numpy().astype(np.float64) - r64).max())
    print(f"chain {case} [{math}]: HIP max-abs error against fp64 {err:.3e}; the oracle in fp32 {e32:.3e} "
          f"(ratio {err / e32:.2f}, bar 3); max |x| {np.abs(r64).max():.2f}")
    assert bool(torch.isfinite(series).all())
    assert err <= 3.0 * e32


# ---------------------------------------------------------------------------------------------- bitwise properties of the sampler
def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("solver,eta", [("ddim", 0.5), ("dpmpp2m", 0.0)])
def test_sampler_bitwise_properties(dev, vae, model, monkeypatch, solver, eta):
    """S = 6 of T = 60, B = 6, Philox noise: graph == eager, one-step == whole-loop graph, lanes 1 == 2 == 3, a second run
    equals the first, 6 rows equal two 3-row shards (row0 0 and 3), set_rows equals the uniform samplers of its values,
    with and without the whole-run adaLN table, and a re-created C sampler keeps its solver."""
    from t2ms_amd.sampler import Sampler
    B, Ls = 6, 48
    text = synth.make_text_embeddings(1, B).to(dev)

    def make(batch=B, **kw):
        a = dict(use_graph=True, seed=7, row0=0, lanes=1, solver=solver, sample_steps=6, eta=eta)
        a.update(kw)
        cfg = a.pop("cfg", 5.0)
        return Sampler(model, vae.decoder, "ddpm", 60, cfg, batch, Ls, dev, **a)

    s0 = make(use_graph=False)
    ref = s0.run(text)[:2]
    assert s0.steps == 6 and s0.graph_lanes == 0 and bool(torch.isfinite(ref[1]).all())
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(lanes=2), dict(lanes=3), dict(lanes=2, use_graph=False),
               dict(lanes=3, loop_graph=0)):
        s = make(**kw)
        got = s.run(text)[:2]
        assert _same(got, ref), kw
        assert s.graph_lanes == (kw.get("lanes", 1) if kw.get("use_graph", True) else 0), kw
        assert _same(s.run_inplace(), ref), kw                      # the second run equals the first
    s._create()                                                      # a re-created C sampler keeps its solver
    assert _same(s.run(text)[:2], ref)
    # shards
    a, b = make(batch=3), make(batch=3, row0=3, use_graph=False)
    la, lb = a.run(text[:3]), b.run(text[3:], trace=True)
    assert torch.equal(torch.cat([la[0], lb[0]]), ref[0]) and torch.equal(torch.cat([la[1], lb[1]]), ref[1])
    assert lb[2].shape == (6, Ls) and torch.equal(lb[2][-1], lb[1][0])         # trace0: row 0 after every step, eager
    b.set_row0(0)                                                    # and set_row0 moves a sampler without a new graph
    assert _same(b.run(text[:3])[:2], la[:2])
    # per-row seed / key row / cfg against the uniform samplers of those values
    rows = make(lanes=2)
    rows.set_rows(seeds=[7, 7, 7, 11, 11, 11], key_rows=[0, 1, 2, 5, 6, 7], cfg=[5.0, 5.0, 5.0, 9.0, 9.0, 9.0])
    got = rows.run(text)[:2]
    other = make(batch=3, seed=11, row0=5, cfg=9.0).run(text[3:])[:2]
    assert torch.equal(got[0][:3], la[0]) and torch.equal(got[1][:3], la[1])
    assert torch.equal(got[0][3:], other[0]) and torch.equal(got[1][3:], other[1])
    # the per-step adaLN kernel in place of the whole-run table
    monkeypatch.setenv("T2S_ADALN_TABLE", "0")
    for kw in (dict(), dict(use_graph=False), dict(lanes=2)):
        assert _same(make(**kw).run(text)[:2], ref), kw


@pytest.mark.parametrize("backbone,solver,total,kw", [("ddpm", "ancestral", 3, {}), ("flowmatching", "euler", 3, {}),
                                                      ("ddpm", "ddim", 60, dict(eta=0.5, sample_steps=3))])
def test_loop_update_past_one_grid_sweep(dev, vae, model, backbone, solver, total, kw):
    """Inside the loop the update kernel's grid is capped at 96 workgroups of 256 quads = 51.2 rows: at B = 53 the last rows
    are updated in a second grid-stride sweep.  Their idx -> (row, quad, Philox key) mapping must be that of the first: the
    53-row latent equals, bit for bit, a 50-row sampler's (24,000 quads, one sweep) followed by a 3-row sampler's at row0 =
    50, and a graph replay repeats it.  Every sampler carries its rows of one per-row guidance table (set_rows)."""
    from t2ms_amd.sampler import Sampler
    B, steps, Ls = 53, 3, 24                  # three loop steps (ddim: 3 of a 60-step schedule)
    text = synth.make_text_embeddings(1, B).to(dev)
    scales = [5.0 if r % 3 else 9.0 for r in range(B)]      # a guidance scale per row: the flow update, which makes no
                                                            # draw, reaches the row of a quad through this table alone

    def make(batch, row0):
        s = Sampler(model, vae.decoder, backbone, total, 5.0, batch, Ls, dev, use_graph=True, seed=7, row0=row0, lanes=1,
                    math="f32", solver=solver, **kw)
        s.set_rows(cfg=scales[row0:row0 + batch])
        return s

    s = make(B, 0)
    assert s.steps == steps
    whole = s.run(text)[0].clone()
    assert s.graph_lanes == 1 and bool(torch.isfinite(whole).all())
    assert torch.equal(s.run_inplace()[0], whole)                    # the replay of the captured graph
    head = make(50, 0).run(text[:50])[0].clone()
    tail = make(3, 50).run(text[50:])[0]
    assert torch.equal(torch.cat([head, tail]), whole)


def test_injected_noise_shape_and_todays_modes_are_untouched(dev, vae, model):
    """self.steps = S is the first dimension of `noise`; solver None / "ancestral" / "euler" build today's sampler (same bits)."""
    from t2ms_amd.sampler import Sampler
    xT, text, noises = _chain_inputs()
    s = Sampler(model, vae.decoder, "ddpm", 100, 7.0, 4, 96, dev, solver="ddim", sample_steps=8, eta=0.5)
    with pytest.raises(L.T2SError, match="noise"):
        s.run(text, x_T=xT, noise=noises[:9])
    a = s.run(text, x_T=xT, noise=noises[:8])[0]
    # the last step is the x0 prediction (c3 == 0): its noise slice is not read
    n2 = noises[:8].clone()
    n2[7] = float("nan")
    assert torch.equal(s.run(text, x_T=xT, noise=n2)[0], a)
    for backbone, name in (("ddpm", "ancestral"), ("flowmatching", "euler")):
        kw = dict(x_T=xT, noise=noises[:5]) if backbone == "ddpm" else dict(x_T=xT)
        ref = Sampler(model, vae.decoder, backbone, 5, 7.0, 4, 96, dev).run(text, **kw)
        got = Sampler(model, vae.decoder, backbone, 5, 7.0, 4, 96, dev, solver=name).run(text, **kw)
        assert _same(got, ref)
    with pytest.raises(ValueError):
        Sampler(model, vae.decoder, "ddpm", 5, 7.0, 4, 96, dev, solver="ab2")
    with pytest.raises(ValueError):
        Sampler(model, vae.decoder, "ddpm", 5, 7.0, 4, 96, dev, sample_steps=3)


# ---------------------------------------------------------------------------------------------- refusals
def test_create_refusals(dev, model):
    lib = L.lib()
    with torch.cuda.device(dev):
        dit = model.t2s_handle(dev, 8)
        tv = torch.tensor([3.0, 1.0])
        good = torch.tensor([[1.0, 0.5, 0, 0, 0, 0], [1.0, 0.5, 0, 0, 0, 0]])
        bad = good.clone()
        bad[1, 2] = float("nan")

        def cfg(mode, steps=2):
            c = L.SampleConfig()
            c.mode, c.steps, c.cfg_scale, c.batch, c.length, c.use_graph, c.seed, c.row0 = mode, steps, 1.0, 4, 96, 1, 1, 0
            c.t_values = tv.data_ptr()
            return c

        def refused(rc, out, word):
            msg = lib.t2s_last_error().decode()
            assert rc != 0 and not out.value and word in msg, (rc, msg)

        out = C.c_void_p()
        c = cfg(L.MODE_LMS)
        refused(lib.t2s_sampler_create(dit, None, C.byref(c), C.byref(out)), out, "mode=2")
        refused(lib.t2s_sampler_create_lms(dit, None, C.byref(c), None, C.byref(out)), out, "NULL")
        refused(lib.t2s_sampler_create_lms(dit, None, C.byref(c), bad.data_ptr(), C.byref(out)), out, "not finite")
        for mode in (L.MODE_DDPM, L.MODE_RF, 3):
            c = cfg(mode)
            refused(lib.t2s_sampler_create_lms(dit, None, C.byref(c), good.data_ptr(), C.byref(out)), out, f"mode={mode}")
        c = cfg(L.MODE_LMS, steps=0)
        refused(lib.t2s_sampler_create_lms(dit, None, C.byref(c), good.data_ptr(), C.byref(out)), out, "steps=0")
        # and the good table is accepted
        c = cfg(L.MODE_LMS)
        L.check(lib.t2s_sampler_create_lms(dit, None, C.byref(c), good.data_ptr(), C.byref(out)), "t2s_sampler_create_lms")
        assert out.value
        lib.t2s_sampler_destroy(out)


# ---------------------------------------------------------------------------------------------- the driver
def test_infer_driver_with_a_solver(dev, tmp_path, monkeypatch):
    """infer.py --solver dpmpp2m --sample_steps 4 (grid form, --trace): its own directories, the four files, a 4-row trace;
    the files are what a Sampler of that solver gives, and the default run next to it keeps its directory."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "results")
    base = ["--dataset_name", "ETTh1_24,ETTh1_48", "--backbone", "ddpm", "--total_step", "20", "--cfg_scale", "9", "--batch_size", "4",
            "--save_path", save, "--synthetic", "10", "--random_init", "--seed", "11", "--no_figs"]
    drv.main(base + ["--solver", "dpmpp2m", "--sample_steps", "4", "--trace"])
    for L_ in (24, 48):
        out = os.path.join(save, "generation", f"ddpm_DiT_ETTh1_{L_}_9.0_20_dpmpp2m4")
        shapes = {"x_1.npy": (8, L_, 1), "x_t.npy": (8, L_, 1), "x_t_latent_dec_array.npy": (8, 64, 30),
                  "x_t_latent_enc_array.npy": (8, 64, 30), "x_infer_trace.npy": (4, L_)}
        for f, shp in shapes.items():
            a = np.load(os.path.join(out, f))
            assert a.shape == shp and np.isfinite(a).all(), (f, a.shape)
    assert not os.path.exists(os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_20"))
    # the same rows through a Sampler of that solver: Philox keyed by (seed, position in the run's order)
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(11), strict=True)
    m = m.to(dev).eval()
    out = os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_20_dpmpp2m4")
    x1 = np.load(os.path.join(out, "x_1.npy"))[:, :, 0]
    from datafactory.dataset import SyntheticT2SDataset
    ds = SyntheticT2SDataset(10, 24)
    rows = [int(np.argmin(np.abs(ds.samples - x1[i][None]).sum(axis=1))) for i in range(8)]
    text = torch.from_numpy(ds.embedding[rows]).float()
    s = Sampler(m, None, "ddpm", 20, 9.0, 8, 24, dev, seed=11, row0=0, solver="dpmpp2m", sample_steps=4)
    lat = s.run(text, decode=False)[0]
    assert np.array_equal(lat.cpu().numpy(), np.load(os.path.join(out, "x_t_latent_dec_array.npy")))
