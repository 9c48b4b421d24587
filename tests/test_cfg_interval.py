"""The guidance interval on the GPU (t2s_sampler_set_guided_steps): classifier-free guidance on a window [j0, j1) of the loop,
ONE conditional pass over the batch rows on every other step.

The reference of the bitwise tests is an eager loop written here against the class API with pairing off: inside the window
`model(x, t, None)` and `model(x, t, text)`, outside it `model(x, t, text)` alone, then the library's stand-alone update entry
(t2s_rf_step / t2s_ddpm_step / t2s_lms_step) with pred_c = NULL outside the window.  A CFG pass equals two forwards bit for bit
in f32 (tests/test_hip_parity.py::test_cfg_pass_equals_two_forwards_bitwise, at W 64 tests/test_wide_dit.py::
test_cfg_pass_equals_two_forwards_bitwise_at_w64) and in bf16 (tests/test_math_bf16.py::
test_rows_are_batch_invariant_and_a_cfg_pass_is_two_forwards_bitwise), so there the fused loop must give the eager loop's bits.
The oracle test restates the loop on the CPU from the oracle's own forward and updates."""
import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu

SEED_W, GAIN = 31337, 0.7     # the synthetic weights of tests/test_hip_parity.py::_chain_setup: the gain makes the branches differ
B, STEPS, WINDOW, CFG, LS = 2, 6, (2, 5), 7.0, 48
PHILOX_SEED = 7
TOL = 1e-4                    # tests/test_hip_parity.py holds its oracle chains to TOL * max(1, max |reference|)

# name -> (backbone, solver, total_step, sample_steps, noise): "philox" draws from the library's stream, "injected" hands the
# draws in, None = the update makes none
CASES = {"rf": ("flowmatching", "euler", STEPS, None, None),
         "ddpm_philox": ("ddpm", "ancestral", STEPS, None, "philox"),
         "ddpm_injected": ("ddpm", "ancestral", STEPS, None, "injected"),
         "dpmpp2m": ("ddpm", "dpmpp2m", 100, STEPS, None),
         "ab2": ("flowmatching", "ab2", STEPS, None, None),
         "rf3": ("flowmatching", "euler", 3, None, None)}      # the 3-step loop of the other arithmetics and of width 64
SIX_STEP_CASES = [c for c in CASES if c != "rf3"]


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


def _model(dev, math="f32"):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(SEED_W, gain=GAIN), strict=True)
    m = m.to(dev).eval().set_math(math)
    return m.set_pairing(False)     # the eager loop updates x in place through raw pointers (Transformer.set_pairing)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


def _inputs(n=B):
    xT = synth.make_latents(SEED_W, n)
    text = synth.make_text_embeddings(SEED_W, n)
    noises = torch.from_numpy(np.random.RandomState(99).randn(STEPS, n, 64, 30).astype(np.float32))
    return xT, text, noises


def _sampler(model, vae, case, window="default", batch=B, **kw):
    from t2ms_amd.sampler import Sampler
    backbone, solver, total, S, _ = CASES[case]
    a = dict(use_graph=True, seed=PHILOX_SEED, row0=0, lanes=1, math="f32", solver=solver, sample_steps=S)
    a.update(kw)
    cfg = a.pop("cfg", CFG)
    if window != "default":
        a["guide_steps"] = window
    return Sampler(model, None if vae is None else vae.decoder, backbone, total, cfg, batch, LS, model_device(model), **a)


def model_device(model):
    return next(model.parameters()).device


def eager_loop(model, case, window, xT, text, noises=None, cfg=CFG, seed=PHILOX_SEED, row0=0, on_step=None):
    """The loop the module docstring describes; returns the final latent (on the GPU).  `noises` None = Philox where the
    update draws (stream_id = the loop index, key rows row0 + r)."""
    from t2ms_amd.model.backbone.DDPM import ddpm_host_tables
    from t2ms_amd.sampler import lms_step, loop_t_values, solver_tables
    backbone, solver, total, S, _ = CASES[case]
    dev = model_device(model)
    lib, st = L.lib(), L.stream_ptr(dev)
    x = xT.to(dev).clone().contiguous()
    text = text.to(dev).contiguous()
    n, row = x.shape[0], x[0].numel()
    table = solver not in ("euler", "ancestral")
    if table:
        tv, coef = solver_tables(backbone, solver, total, S)
        coef_d, hist = coef.to(dev), torch.zeros_like(x)
    else:
        tv = loop_t_values(backbone, total)
        coef_d = ddpm_host_tables(total)["coef"].to(dev) if backbone == "ddpm" else None
    steps = int(tv.numel())
    dt = float(np.float32(1.0) / np.float32(steps))            # the sampler's 1.0f / (float)steps
    if noises is not None:
        noises = noises.to(dev).contiguous()
    j0, j1 = window
    with torch.no_grad(), torch.cuda.device(dev):
        for j in range(steps):
            t = torch.full((n,), int(tv[j]), dtype=torch.long, device=dev) if backbone == "ddpm" else tv[j].repeat(n).to(dev)
            if j0 <= j < j1:
                u, c = model(input=x, t=t, text_input=None), model(input=x, t=t, text_input=text)
            else:
                u, c = model(input=x, t=t, text_input=text), None         # pred = the conditional output, unchanged
            z = None if noises is None else noises[j]
            if table:
                lms_step(x, hist, u, c, coef_d, j, cfg=cfg, noise=z, seed=seed, stream_id=j, row0=row0)
            elif backbone == "ddpm":
                L.check(lib.t2s_ddpm_step(x.data_ptr(), u.data_ptr(), L.dev_ptr(c), L.dev_ptr(z), coef_d.data_ptr(), steps - 1 - j, cfg,
                                          seed, j, row0, n, st), "t2s_ddpm_step")
            else:
                assert n * row % L.LAT == 0          # the stand-alone flow update works in rows of 1920 values
                L.check(lib.t2s_rf_step(x.data_ptr(), u.data_ptr(), L.dev_ptr(c), cfg, dt, n * row // L.LAT, st), "t2s_rf_step")
            if on_step is not None:
                on_step(j, x)
    return x


def _noise_kw(case, noises):
    return dict(noise=noises) if CASES[case][4] == "injected" else {}


_EAGER = {}


def _eager_ref(model, case, window):
    """The eager loop's latent for (case, window) at the module's inputs, computed once and left unchanged."""
    key = (case, tuple(window))
    if key not in _EAGER:
        xT, text, noises = _inputs()
        _EAGER[key] = eager_loop(model, case, window, xT, text, noises if CASES[case][4] == "injected" else None).clone()
    return _EAGER[key]


# ---------------------------------------------------------------------------------------------- 1. the eager loop, bit for bit
@pytest.mark.parametrize("case", SIX_STEP_CASES)
def test_fused_loop_equals_the_eager_class_api_loop_bitwise(dev, vae, model, case):
    xT, text, noises = _inputs()
    ref = _eager_ref(model, case, WINDOW)
    assert bool(torch.isfinite(ref).all())
    # the window matters at these weights: the all-guided and the all-conditional loop give other values
    assert not torch.equal(ref, _eager_ref(model, case, (0, STEPS))) and not torch.equal(ref, _eager_ref(model, case, (0, 0)))
    series = None
    for kw in (dict(use_graph=False), dict(loop_graph=0), dict(loop_graph=1)):
        s = _sampler(model, vae, case, WINDOW, **kw)
        assert s.guided == WINDOW
        lat, ser, _ = s.run(text, x_T=xT, **_noise_kw(case, noises))
        assert torch.equal(lat, ref), (case, kw)
        assert s.graph_lanes == (1 if kw.get("use_graph", True) else 0), kw
        series = ser if series is None else series
        assert torch.equal(ser, series), (case, kw)
        lat2, ser2, _ = s.run(text, x_T=xT, **_noise_kw(case, noises))       # the replay repeats it
        assert torch.equal(lat2, ref) and torch.equal(ser2, series), (case, kw)
    # two lanes: the batch twice, one copy per lane (the Philox key rows of the second copy are those of the first)
    x4, t4, n4 = torch.cat([xT, xT]), torch.cat([text, text]), torch.cat([noises, noises], dim=1)
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(use_graph=False)):
        s = _sampler(model, vae, case, WINDOW, batch=2 * B, lanes=2, **kw)
        s.set_rows(key_rows=[0, 1, 0, 1])
        lat, ser, _ = s.run(t4, x_T=x4, **_noise_kw(case, n4))
        assert s.graph_lanes == (2 if kw.get("use_graph", True) else 0), kw
        assert torch.equal(lat[:B], ref) and torch.equal(lat[B:], ref), (case, kw)
        assert torch.equal(ser[:B], series) and torch.equal(ser[B:], series), (case, kw)


def test_fused_loop_without_the_whole_run_adaln_table(dev, vae, model, monkeypatch):
    """T2S_ADALN_TABLE=0 keeps the per-step adaLN kernel in the loop: an unguided step then computes the modulation of its n
    text rows alone."""
    xT, text, noises = _inputs()
    monkeypatch.setenv("T2S_ADALN_TABLE", "0")
    for case in ("rf", "ddpm_injected"):
        ref = _eager_ref(model, case, WINDOW)
        for kw in (dict(use_graph=False), dict(loop_graph=0), dict(loop_graph=1)):
            lat = _sampler(model, None, case, WINDOW, **kw).run(text, x_T=xT, decode=False, **_noise_kw(case, noises))[0]
            assert torch.equal(lat, ref), (case, kw)


# ---------------------------------------------------------------------------------------------- 2. the oracle
def _oracle_chain(sd, backbone, xT, text, steps, cfg, window, noises, outside_text=True):
    """infer.py:75-88 with the window, from the oracle's forward and updates on the CPU.  outside_text False is the mutant
    that takes the UNCONDITIONAL branch outside the window."""
    tab = O.ddpm_tables(steps)
    x = xT
    with torch.no_grad():
        for j in range(steps):
            if backbone == "ddpm":
                t = torch.full((x.size(0),), steps - 1 - j, dtype=torch.long)
            else:
                t = torch.round(torch.full((x.shape[0],), j * 1.0 / steps) * steps) / steps
            if window[0] <= j < window[1]:
                u, c = O.dit_forward(sd, x, t, None), O.dit_forward(sd, x, t, text)
                pred = u + cfg * (c - u)
            else:
                pred = O.dit_forward(sd, x, t, text if outside_text else None)
            x = O.ddpm_p_sample(tab, x, pred, t, noises[j]) if backbone == "ddpm" else O.rf_euler(x, pred, 1.0 / steps)
    return x


@pytest.mark.parametrize("backbone", ["flowmatching", "ddpm"])
def test_fused_loop_against_the_oracle(dev, vae, model, backbone):
    """B 1, 3 steps, window (1, 2), injected noise: independent of the library's forward.  Bar: TOL * max(1, max |reference|),
    the bar of the oracle chains of tests/test_hip_parity.py.  The loop that takes the unconditional branch outside the
    window lies more than twice that bar away (checked on the oracle itself, so the test can tell the two apart)."""
    from t2ms_amd.sampler import Sampler
    steps, window = 3, (1, 2)
    sd = synth.make_dit_state_dict(SEED_W, gain=GAIN)
    xT, text = synth.make_latents(SEED_W, 1), synth.make_text_embeddings(SEED_W, 1)
    noises = torch.from_numpy(np.random.RandomState(5).randn(steps, 1, 64, 30).astype(np.float32))
    ref = _oracle_chain(sd, backbone, xT, text, steps, CFG, window, noises)
    mutant = _oracle_chain(sd, backbone, xT, text, steps, CFG, window, noises, outside_text=False)
    bar = TOL * max(1.0, float(ref.abs().max()))
    gap = float((mutant - ref).abs().max())
    print(f"{backbone}: max |x| {float(ref.abs().max()):.3f}, bar {bar:.3e}, the unconditional-outside loop is {gap:.3e} away")
    assert gap > 2 * bar      # a loop within the bar of the mutant is then more than the bar away from the reference
    kw = dict(noise=noises) if backbone == "ddpm" else {}
    for use_graph in (False, True):
        s = Sampler(model, vae.decoder, backbone, steps, CFG, 1, LS, dev, use_graph=use_graph, math="f32", guide_steps=window)
        lat = s.run(text, x_T=xT, **kw)[0].cpu()
        err = float((lat - ref).abs().max())
        print(f"{backbone} graph={use_graph}: max |latent - oracle| {err:.3e}")
        assert err < bar, (backbone, use_graph, err, bar)


# ---------------------------------------------------------------------------------------------- 3. - 5. windows
@pytest.mark.parametrize("case", ["rf", "ddpm_philox", "dpmpp2m"])
def test_the_whole_window_is_a_sampler_without_one(dev, vae, model, case):
    xT, text, _ = _inputs()
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(use_graph=False), dict(loop_graph=0, lanes=2)):
        plain = _sampler(model, vae, case, **kw)
        assert plain.guided == (0, STEPS)
        want = plain.run(text, x_T=xT)[:2]
        s = _sampler(model, vae, case, (0, STEPS), **kw)
        got = s.run(text, x_T=xT)[:2]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (case, kw)
        assert s.graph_lanes == plain.graph_lanes == (kw.get("lanes", 1) if kw.get("use_graph", True) else 0)
        s.set_guided_steps(0, STEPS)                   # the same window again keeps the captured graphs
        assert s.graph_lanes == plain.graph_lanes
    assert torch.equal(want[0], _eager_ref(model, case, (0, STEPS)))      # ... and both are the all-guided eager loop


@pytest.mark.parametrize("case", ["rf", "ddpm_philox", "ab2"])
def test_the_empty_window_is_the_all_conditional_loop(dev, model, case):
    xT, text, _ = _inputs()
    ref = _eager_ref(model, case, (0, 0))
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(use_graph=False)):
        s = _sampler(model, None, case, (3, 3), **kw)
        assert torch.equal(s.run(text, x_T=xT, decode=False)[0], ref), (case, kw)
        assert s.graph_lanes == (1 if kw.get("use_graph", True) else 0)           # (a one-step run holds the conditional graph alone)


@pytest.mark.parametrize("window", [(0, 1), (STEPS - 1, STEPS)])
@pytest.mark.parametrize("case", ["rf", "ddpm_philox", "dpmpp2m", "ab2"])
def test_window_edges(dev, model, case, window):
    """The first and the last step alone guided -- for the multistep solvers the step that starts the history and the step
    that writes none."""
    xT, text, _ = _inputs()
    ref = _eager_ref(model, case, window)
    assert not torch.equal(ref, _eager_ref(model, case, (0, 0)))
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(use_graph=False)):
        assert torch.equal(_sampler(model, None, case, window, **kw).run(text, x_T=xT, decode=False)[0], ref), (case, window, kw)


# ---------------------------------------------------------------------------------------------- 6. trace
@pytest.mark.parametrize("case", ["rf", "ddpm_philox"])
def test_trace_rows_decode_the_eager_states(dev, vae, model, case):
    xT, text, _ = _inputs()
    states = []
    eager_loop(model, case, WINDOW, xT, text, on_step=lambda j, x: states.append(x[:1].clone()))
    s = _sampler(model, vae, case, WINDOW)
    lat, ser, tr = s.run(text, x_T=xT, trace=True)
    assert tr.shape == (STEPS, LS) and torch.equal(lat[:1], states[-1])
    h = vae.decoder._handle(dev)
    for j, x in enumerate(states):
        out = torch.empty(1, LS, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().t2s_vae_decode(h, x.data_ptr(), out.data_ptr(), None, 1, LS, L.stream_ptr(dev)), "t2s_vae_decode")
        assert torch.equal(tr[j], out[0]), j
    assert torch.equal(tr[-1], ser[0])


# ---------------------------------------------------------------------------------------------- 7. per-row tables
@pytest.mark.parametrize("case", ["rf", "ddpm_philox"])
def test_set_rows_with_a_window(dev, model, case):
    """Each row of a set_rows sampler equals the row of a uniform sampler of its seed / key row / scale with the same window
    (on unguided steps the row's scale is not read, its seed and key row are)."""
    text = synth.make_text_embeddings(3, 2)
    seeds, keys, scales = [7, 11], [3, 9], [5.0, 9.0]
    for kw in (dict(loop_graph=0), dict(loop_graph=1), dict(lanes=2)):
        s = _sampler(model, None, case, WINDOW, **kw)
        s.set_rows(seeds=seeds, key_rows=keys, cfg=scales)
        lat = s.run(text, decode=False)[0]
        for r in range(2):
            one = _sampler(model, None, case, WINDOW, batch=1, seed=seeds[r], row0=keys[r], cfg=scales[r])
            assert torch.equal(one.run(text[r:r + 1], decode=False)[0], lat[r:r + 1]), (case, kw, r)
    # the scale of a row is used inside the window: another scale, another row
    other = _sampler(model, None, case, WINDOW, batch=1, seed=seeds[1], row0=keys[1], cfg=scales[0])
    assert not torch.equal(other.run(text[1:], decode=False)[0], lat[1:])


# ---------------------------------------------------------------------------------------------- 8. changing the window
@pytest.mark.parametrize("loop_graph", [0, 1])
def test_changing_the_window_between_runs(dev, model, loop_graph):
    xT, text, _ = _inputs()
    case = "ddpm_philox"
    lib = L.lib()
    s = _sampler(model, None, case, loop_graph=loop_graph)
    original = s.run(text, x_T=xT, decode=False)[0]
    assert s.graph_lanes == 1
    for window in (WINDOW, (1, 3), (0, 0)):
        s.set_guided_steps(*window)
        assert s.guided == window and s.graph_lanes == 0           # a changed window drops the graphs
        got = s.run(text, x_T=xT, decode=False)[0]
        fresh = _sampler(model, None, case, window, loop_graph=loop_graph).run(text, x_T=xT, decode=False)[0]
        assert torch.equal(got, fresh) and torch.equal(got, _eager_ref(model, case, window)), window
        assert s.graph_lanes == 1
    s.set_guided_steps(*WINDOW)
    before = s.run(text, x_T=xT, decode=False)[0]
    # refusals: T2S_E_INVALID, the values in the message, nothing touched (window, graphs, the next run)
    for first, end in ((-1, 3), (2, STEPS + 1), (4, 3)):
        rc = lib.t2s_sampler_set_guided_steps(s.ptr, first, end)
        msg = lib.t2s_last_error().decode()
        assert rc == -1 and f"first={first}" in msg and f"end={end}" in msg and f"steps={STEPS}" in msg, (rc, msg)
        with pytest.raises(L.T2SError, match=f"first={first} end={end}"):
            s.set_guided_steps(first, end)
        assert s.guided == WINDOW and s._guided == WINDOW and s.graph_lanes == 1
    assert torch.equal(s.run(text, x_T=xT, decode=False)[0], before)
    s._create()                                                    # a re-created C sampler keeps the window
    assert s.guided == WINDOW and torch.equal(s.run(text, x_T=xT, decode=False)[0], before)
    s.set_guided_steps(0, STEPS)
    assert torch.equal(s.run(text, x_T=xT, decode=False)[0], original)
    with pytest.raises(ValueError):
        _sampler(model, None, case, (2, STEPS + 1))
    with pytest.raises(ValueError):
        _sampler(model, None, case, WINDOW, cfg_interval=(0.2, 0.8))
    assert _sampler(model, None, case, cfg_interval=(0.25, 0.75)).guided == (2, 5)


# ---------------------------------------------------------------------------------------------- the driver
def test_infer_driver_with_a_guidance_interval(dev, tmp_path, monkeypatch):
    """infer.py --cfg_interval 0.25,0.75 (8 DDPM steps: window (2, 6), --trace): its own directory, the files, and the latents
    a Sampler of that window gives for the same rows; the run without the flag next to it keeps today's directory."""
    import os
    import infer as drv
    from datafactory.dataset import SyntheticT2SDataset
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "results")
    base = ["--dataset_name", "ETTh1_24", "--backbone", "ddpm", "--total_step", "8", "--cfg_scale", "9", "--batch_size", "4",
            "--save_path", save, "--synthetic", "10", "--random_init", "--seed", "11", "--no_figs", "--math", "f32"]
    drv.main(base + ["--cfg_interval", "0.25,0.75", "--trace"])
    out = os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_8_gi2-6")
    shapes = {"x_1.npy": (8, 24, 1), "x_t.npy": (8, 24, 1), "x_t_latent_dec_array.npy": (8, 64, 30), "x_infer_trace.npy": (8, 24)}
    for f, shp in shapes.items():
        a = np.load(os.path.join(out, f))
        assert a.shape == shp and np.isfinite(a).all(), (f, a.shape)
    assert not os.path.exists(os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_8"))
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(11), strict=True)
    m = m.to(dev).eval()
    x1 = np.load(os.path.join(out, "x_1.npy"))[:, :, 0]
    ds = SyntheticT2SDataset(10, 24)
    rows = [int(np.argmin(np.abs(ds.samples - x1[i][None]).sum(axis=1))) for i in range(8)]
    text = torch.from_numpy(ds.embedding[rows]).float()
    got = np.load(os.path.join(out, "x_t_latent_dec_array.npy"))
    lat = Sampler(m, None, "ddpm", 8, 9.0, 8, 24, dev, seed=11, row0=0, math="f32", guide_steps=(2, 6)).run(text, decode=False)[0]
    assert np.array_equal(lat.cpu().numpy(), got)
    plain = Sampler(m, None, "ddpm", 8, 9.0, 8, 24, dev, seed=11, row0=0, math="f32").run(text, decode=False)[0]
    assert not np.array_equal(plain.cpu().numpy(), got)
    drv.main(base)                                                  # without the flag: today's directory, today's latents
    old = np.load(os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_8", "x_t_latent_dec_array.npy"))
    assert np.array_equal(plain.cpu().numpy(), old)


# ---------------------------------------------------------------------------------------------- 9. other arithmetics, width 64
def test_bf16_at_480_tokens_bitwise(dev):
    """bf16: a CFG pass is two forwards bit for bit (tests/test_math_bf16.py::
    test_rows_are_batch_invariant_and_a_cfg_pass_is_two_forwards_bitwise), so the fused loop gives the eager loop's bits."""
    m = _model(dev, "bf16")
    steps, window = 3, (1, 2)
    xT, text, _ = _inputs()
    from t2ms_amd.sampler import Sampler
    ref = eager_loop(m, "rf3", window, xT, text)
    for kw in (dict(use_graph=False), dict(loop_graph=0), dict(loop_graph=1)):
        s = Sampler(m, None, "flowmatching", steps, CFG, B, LS, dev, math="bf16", guide_steps=window, **kw)
        assert torch.equal(s.run(text, x_T=xT, decode=False)[0], ref), kw


def test_bf16x3_at_480_tokens(dev):
    """bf16x3: no test of the parent holds a bf16x3 CFG pass to two forwards bit for bit, so the bar is the one
    tests/test_hip_parity.py::test_dit_forward_bf16x3_matches_f32_path applies to ONE bf16x3 forward against another
    fp32-accurate evaluation of it: 2e-5 absolute -- here on the latent after the whole 3-step loop against the eager loop in
    the same arithmetic (the figure is printed: 0 when the pass is the two forwards' bits)."""
    m = _model(dev, "bf16x3")
    steps, window = 3, (1, 2)
    xT, text, _ = _inputs()
    from t2ms_amd.sampler import Sampler
    ref = eager_loop(m, "rf3", window, xT, text)
    for kw in (dict(use_graph=False), dict(loop_graph=0), dict(loop_graph=1)):
        s = Sampler(m, None, "flowmatching", steps, CFG, B, LS, dev, math="bf16x3", guide_steps=window, **kw)
        d = float((s.run(text, x_T=xT, decode=False)[0] - ref).abs().max())
        print(f"bf16x3 {kw}: max |fused - eager| {d:.3e}")
        assert d < 2e-5, kw


def test_w64_bitwise(dev):
    """Width 64 (1024 tokens), f32, rectified flow, 3 steps, window (1, 2).  15 rows: the stand-alone flow update of the eager
    loop works in rows of 1920 values, and 15 x 4096 = 32 x 1920 is the smallest batch of this width it can step."""
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd.sampler import Sampler
    W, n, steps, window = 64, 15, 3, (1, 2)
    m = Transformer(W)
    m.load_state_dict(synth.make_dit_state_dict(SEED_W, width=W, gain=GAIN), strict=True)
    m = m.to(dev).eval().set_pairing(False)
    xT, text = synth.make_wide_latents(SEED_W, n, W), synth.make_text_embeddings(SEED_W, n)
    ref = eager_loop(m, "rf3", window, xT, text)
    assert not torch.equal(ref, eager_loop(m, "rf3", (0, 0), xT, text))
    for kw in (dict(use_graph=False), dict(loop_graph=0), dict(loop_graph=1)):
        s = Sampler(m, None, "flowmatching", steps, CFG, n, 40, dev, math="f32", guide_steps=window, **kw)
        assert torch.equal(s.run(text, x_T=xT, decode=False)[0], ref), kw
