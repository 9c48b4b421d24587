"""Parity of the HIP path (through the C ABI) against the CPU oracle and the committed golden
vectors.  Needs a real MI355X: run with `pytest -m gpu` via gpurun.

Tolerances (fp32): 1e-4 absolute per forward / per step as BASELINE.json's north_star states;
chains are checked relative to max|x|."""
import os

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _load(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name + ".npz")).items()}


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dit(dev):
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def vae(dev):
    import types
    from model.pretrained.vqvae import vqvae
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256,
                                    embedding_dim=64))
    v.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    return v.to(dev).eval()


def _maxdiff(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def test_native_library_is_loaded(dev):
    lib = L.lib()
    maps = open("/proc/self/maps").read()
    assert "libt2s_hip.so" in maps
    assert b"gfx950" in lib.t2s_version()


def test_time_embedding(golden_dir, dev, dit):
    g = _load(golden_dir, "time_emb")
    e_long = dit.time_emb(_t(g["t_long"]).to(dev))
    e_float = dit.time_emb(_t(g["t_float"]).to(dev))
    assert _maxdiff(e_long, g["emb_long"]) < 1e-5
    assert _maxdiff(e_float, g["emb_float"]) < 1e-5
    # all 1000 DDPM steps (arguments up to 99,900 rad)
    t = torch.arange(1000)
    assert _maxdiff(dit.time_emb(t.to(dev)), O.time_embedding(t)) < 1e-5


def test_attention_kernel_vs_oracle(dev):
    rs = np.random.RandomState(11)
    BH = 12
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    q = q * 2.0  # sharper softmax
    ref = torch.softmax((q * 32 ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    od = torch.empty_like(qd)
    L.check(L.lib().t2s_attn_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), BH,
                                 L.stream_ptr(dev)))
    assert _maxdiff(od, ref) < 2e-5


def _pack_frag(x):
    """(BH,480,32) -> fragment-major (include/t2s.h, t2s_attn_fwd_packed)."""
    BH = x.shape[0]
    # [bh][tile][i][g][h][e] -> [bh][tile][g][h][i][e]
    return x.reshape(BH, 15, 32, 4, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous()


def _pack_vT(v):
    """(BH,480,32) -> transposed fragment-major: [bh][tile][g][h][d][e] = V[32 tile + 8g + 4h + e][d]."""
    BH = v.shape[0]
    return v.reshape(BH, 15, 4, 2, 4, 32).permute(0, 1, 2, 3, 5, 4).contiguous()


def test_attention_packed_kernel_vs_oracle(dev):
    """The kernel the DiT forward launches (fragment-major operands, LDS-DMA ring), incl. spikes
    that force the online-softmax rescale at early and late key blocks."""
    rs = np.random.RandomState(21)
    n_seq = 3
    BH = n_seq * 4
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 333] = q[:, 100] * 5.0
    k[:, 5] = q[:, 479] * 4.0
    k[:, 479] = q[:, 0] * 4.0
    # the sticky softmax reference is only renewed when it is stale by > 2^60: force that branch at
    # a late key block (log2-domain jump of ~100 for query 200 at key 410), and make one query's
    # first block hugely negative so its first reference sits far below the later scores
    k[:, 410] = q[:, 200] * 12.0
    k[:, 0:32] = -q[:, 7:8] * 3.0 + 0.01 * k[:, 0:32]
    k[:, 448] = q[:, 7] * 10.0
    ref = (torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()).float()
    qd, kd, vd = _pack_frag(q).to(dev), _pack_frag(k).to(dev), _pack_vT(v).to(dev)
    od = torch.empty(n_seq * 480 * 128, device=dev)
    L.check(L.lib().t2s_attn_fwd_packed(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), n_seq,
                                        L.stream_ptr(dev)))
    # o: [tile = seq*15 + t][G = head*4 + g][h][i][e] = O[seq][head][32 t + i][8g + 4h + e]
    o = od.cpu().reshape(n_seq, 15, 4, 4, 2, 32, 4).permute(0, 2, 1, 5, 3, 4, 6).reshape(BH, 480, 32)
    assert _maxdiff(o, ref) < 2e-5


def test_attention_persistent_kernel_multi_item(dev):
    """n_seq = 200 -> 800 heads on the persistent grid of one workgroup per CU (the launcher goes persistent from three
    heads per CU): 3-4 heads per workgroup, so the cross-head DMA ring, the Q prefetch and the per-head state reset are
    all exercised (plus re-reference spikes in every head)."""
    rs = np.random.RandomState(22)
    n_seq = 200
    BH = n_seq * 4
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 410] = q[:, 200] * 12.0
    k[:, 31] = q[:, 470] * 6.0
    ref = (torch.softmax((q * 32 ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v)
    qd, kd, vd = _pack_frag(q).to(dev), _pack_frag(k).to(dev), _pack_vT(v).to(dev)
    od = torch.full((n_seq * 480 * 128,), float("nan"), device=dev)
    L.check(L.lib().t2s_attn_fwd_packed(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), n_seq,
                                        L.stream_ptr(dev)))
    o = od.cpu().reshape(n_seq, 15, 4, 4, 2, 32, 4).permute(0, 2, 1, 5, 3, 4, 6).reshape(BH, 480, 32)
    assert bool(torch.isfinite(o).all())
    assert _maxdiff(o, ref) < 3e-5


def test_attention_online_softmax_rescale_branch(dev):
    """Force the running max to jump at a late key block (rule: a rare data-dependent branch needs
    its own test): one key row is aligned with the queries and scaled up."""
    rs = np.random.RandomState(12)
    q = torch.from_numpy(rs.randn(4, 480, 32).astype(np.float32))
    k = torch.from_numpy(rs.randn(4, 480, 32).astype(np.float32))
    v = torch.from_numpy(rs.randn(4, 480, 32).astype(np.float32))
    k[:, 333] = q[:, 100] * 6.0      # spike in key block 10 for query 100
    k[:, 5] = q[:, 200] * 4.0        # and an early one
    ref = torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    od = torch.empty_like(qd)
    L.check(L.lib().t2s_attn_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), 4,
                                 L.stream_ptr(dev)))
    assert _maxdiff(od, ref.float()) < 2e-5


def test_dit_forward_golden(golden_dir, dev, dit):
    g = _load(golden_dir, "dit_forward")
    x = synth.make_latents(2025, 4).to(dev)
    text = synth.make_text_embeddings(2025, 4).to(dev)
    with torch.no_grad():
        yc = dit(input=x, t=_t(g["t_long"]).to(dev), text_input=text)
        # the residual stream the forward left behind (post block 3) vs the reference's hook tap
        stream = torch.empty(4, 480, 128, device=dev)
        L.check(L.lib().t2s_dit_read_stream(dit.t2s_handle(dev, 4), stream.data_ptr(), 4, L.stream_ptr(dev)))
        yu = dit(input=x, t=_t(g["t_long"]).to(dev), text_input=None)
        yf = dit(input=x, t=_t(g["t_float"]).to(dev), text_input=text)
    assert _maxdiff(stream[:1, ::7], g["tap_post_mlp_3"]) < TOL
    assert _maxdiff(yc, g["cond"]) < TOL
    assert _maxdiff(yu, g["uncond"]) < TOL
    assert _maxdiff(yf, g["cond_float"]) < TOL


@pytest.mark.parametrize("B", [1, 3, 7])
def test_dit_forward_vs_oracle_ragged_batches(dev, dit, B):
    """Odd batch sizes exercise the partial 64-row tiles (B*480 is not a multiple of 64)."""
    sd = synth.make_dit_state_dict(2025)
    x = synth.make_latents(900 + B, B)
    text = synth.make_text_embeddings(900 + B, B)
    t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(B))
    with torch.no_grad():
        ref_c = O.dit_forward(sd, x, t, text)
        ref_u = O.dit_forward(sd, x, t, None)
        got_c = dit(input=x.to(dev), t=t.to(dev), text_input=text.to(dev))
        got_u = dit(input=x.to(dev), t=t.to(dev), text_input=None)
    assert _maxdiff(got_c, ref_c) < TOL
    assert _maxdiff(got_u, ref_u) < TOL


def test_cfg_pass_equals_two_forwards_bitwise(dev, dit):
    B = 5
    x = synth.make_latents(77, B).to(dev)
    text = synth.make_text_embeddings(77, B).to(dev)
    t = torch.full((B,), 421, dtype=torch.long, device=dev)
    with torch.no_grad():
        yu = dit(input=x, t=t, text_input=None)
        yc = dit(input=x, t=t, text_input=text)
        h = dit.t2s_handle(dev, 2 * B)
        temb = dit.time_emb(t[:1])
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        L.check(L.lib().t2s_dit_forward_cfg(h, x.data_ptr(), temb.data_ptr(), text.data_ptr(), ou.data_ptr(),
                                            oc.data_ptr(), B, L.stream_ptr(dev)))
    assert torch.equal(ou, yu) and torch.equal(oc, yc)


def test_weight_update_is_picked_up(dev):
    from model.denoiser.transformer import Transformer
    m = Transformer().to(dev).eval()
    m.load_state_dict(synth.make_dit_state_dict(5), strict=True)
    x = synth.make_latents(5, 2).to(dev)
    t = torch.tensor([10, 20], device=dev)
    with torch.no_grad():
        y1 = m(input=x, t=t, text_input=None)
        m.load_state_dict(synth.make_dit_state_dict(6), strict=True)   # in-place copy_ -> version bump
        y2 = m(input=x, t=t, text_input=None)
        ref2 = O.dit_forward(synth.make_dit_state_dict(6), x.cpu(), t.cpu(), None)
    assert _maxdiff(y2, ref2) < TOL and _maxdiff(y1, y2) > 1e-3


def test_full_size_batch_invariance(dev, dit):
    """BASELINE size (B=256 -> 512 sequences in one CFG pass): every row must be BITWISE what the
    same row gives in a 4-row batch (rows are independent through the whole network), and rows
    agree with the oracle."""
    B = 256
    x = synth.make_latents(4242, B).to(dev)
    text = synth.make_text_embeddings(4242, B).to(dev)
    t = torch.full((B,), 999, dtype=torch.long, device=dev)
    with torch.no_grad():
        h = dit.t2s_handle(dev, 2 * B)
        temb = dit.time_emb(t[:1])
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        L.check(L.lib().t2s_dit_forward_cfg(h, x.data_ptr(), temb.data_ptr(), text.data_ptr(), ou.data_ptr(),
                                            oc.data_ptr(), B, L.stream_ptr(dev)))
        rows = [0, 1, 130, 255]
        small_c = dit(input=x[rows].contiguous(), t=t[:4], text_input=text[rows].contiguous())
        small_u = dit(input=x[rows].contiguous(), t=t[:4], text_input=None)
        ref_c = O.dit_forward(synth.make_dit_state_dict(2025), x[rows].cpu(), t[:4].cpu(), text[rows].cpu())
    assert torch.equal(oc[rows], small_c) and torch.equal(ou[rows], small_u)
    assert _maxdiff(small_c, ref_c) < TOL
    assert bool(torch.isfinite(oc).all()) and bool(torch.isfinite(ou).all())


def test_ddpm_backbone_golden(golden_dir, dev):
    from model.backbone.DDPM import DDPM
    g = _load(golden_dir, "ddpm")
    for T in (50, 1000):
        d = DDPM(T, dev)
        for k in ("beta", "alpha", "alpha_bar"):
            assert np.array_equal(getattr(d, k).cpu().numpy(), g[f"{k}_{T}"])
    d = DDPM(1000, dev)
    t = _t(g["t"]).to(dev)
    xq, eps = d.q_sample(_t(g["x0"]).to(dev), t, _t(g["eps"]).to(dev))
    assert _maxdiff(xq, g["q_sample"]) < 1e-6
    xp = d.p_sample(_t(g["x0"]).to(dev), _t(g["eps_hat"]).to(dev), t, eps=_t(g["p_noise"]).to(dev))
    assert _maxdiff(xp, g["p_sample"]) < 2e-6
    # default path draws its own noise (like the reference) and stays finite / right shape
    xr = d.p_sample(_t(g["x0"]).to(dev), _t(g["eps_hat"]).to(dev), t)
    assert xr.shape == (4, 64, 30) and bool(torch.isfinite(xr).all())


def test_rectified_flow_golden(golden_dir, dev):
    from model.backbone.rectified_flow import RectifiedFlow
    g = _load(golden_dir, "rf")
    rf = RectifiedFlow()
    assert _maxdiff(rf.euler(_t(g["x1"]).to(dev), _t(g["v"]).to(dev), 1.0 / 100), g["euler"]) < 1e-6
    xt, x0 = rf.create_flow(_t(g["x1"]).to(dev), _t(g["t"]).to(dev), x_0=_t(g["x_0"]).to(dev))
    assert _maxdiff(xt, g["x_t"]) < 1e-6


@pytest.mark.parametrize("B", [6, 53])      # 53: 25,440 quads, past one sweep of a 96-workgroup grid
def test_fused_ddpm_step_vs_oracle(dev, B):
    from t2ms_amd.model.backbone.DDPM import ddpm_host_tables
    rs = np.random.RandomState(3)
    T = 1000
    x, u, c, z = (torch.from_numpy(rs.randn(B, 64, 30).astype(np.float32)) for _ in range(4))
    tab = O.ddpm_tables(T)
    coef = ddpm_host_tables(T)["coef"].to(dev)
    ud, cd, zd = u.to(dev), c.to(dev), z.to(dev)   # keep the device copies alive across the launches
    for t_idx in (0, 1, 517, 999):
        pred = u + 9.0 * (c - u)
        ref = O.ddpm_p_sample(tab, x, pred, torch.full((B,), t_idx), z)
        xd = x.to(dev).clone()
        L.check(L.lib().t2s_ddpm_step(xd.data_ptr(), ud.data_ptr(), cd.data_ptr(), zd.data_ptr(),
                                      coef.data_ptr(), t_idx, 9.0, 0, 0, 0, B, L.stream_ptr(dev)))
        assert _maxdiff(xd, ref) < 2e-5, t_idx
    # RF step
    ref = O.rf_euler(x, u + 5.0 * (c - u), 0.01)
    xd = x.to(dev).clone()
    L.check(L.lib().t2s_rf_step(xd.data_ptr(), ud.data_ptr(), cd.data_ptr(), 5.0, 0.01, B,
                                L.stream_ptr(dev)))
    assert _maxdiff(xd, ref) < 2e-6


@pytest.mark.parametrize("B,row0", [(3, 1000), (53, 7)])
def test_philox_through_ddpm_step_is_the_library_stream(dev, B, row0):
    """x = 0 and the coefficient row {1, 0, 1}: x' = 1 * (0 - 0 * pred) + 1 * z = z exactly, the draw of the given key."""
    from t2ms_amd.sampler import philox_normal
    seed, sid = 2025, 17
    x = torch.zeros(B, 1920, device=dev)
    u = torch.from_numpy(np.random.RandomState(1).randn(B, 1920).astype(np.float32)).to(dev)
    coef = torch.tensor([[1, 0, 1]], dtype=torch.float32, device=dev)
    L.check(L.lib().t2s_ddpm_step(x.data_ptr(), u.data_ptr(), None, None, coef.data_ptr(), 0, 0.0, seed, sid, row0, B,
                                  L.stream_ptr(dev)))
    assert torch.equal(x, philox_normal(B, 1920, seed, sid, row0, dev))


def test_mse(dev):
    from t2ms_amd.train import mse_loss
    rs = np.random.RandomState(8)
    a = torch.from_numpy(rs.randn(9, 64, 30).astype(np.float32))
    b = torch.from_numpy(rs.randn(9, 64, 30).astype(np.float32))
    got = mse_loss(a.to(dev), b.to(dev))
    np.testing.assert_allclose(got.item(), O.mse_loss(a, b).item(), rtol=1e-5)


def test_philox_matches_oracle(dev):
    n_rows, row0, seed, stream = 8, 1000, 2025, 17
    out = torch.empty(n_rows, 1920, device=dev)
    L.check(L.lib().t2s_philox_normal(out.data_ptr(), seed, stream, row0, n_rows, 1920, L.stream_ptr(dev)))
    ref = O.device_normal(seed, stream, row0, n_rows)
    assert _maxdiff(out, ref) < 1e-5
    # sharding invariance: rows 4..7 drawn alone equal rows 4..7 of the big draw, bit for bit
    part = torch.empty(4, 1920, device=dev)
    L.check(L.lib().t2s_philox_normal(part.data_ptr(), seed, stream, row0 + 4, 4, 1920, L.stream_ptr(dev)))
    assert torch.equal(part, out[4:])
    big = torch.empty(4096, 1920, device=dev)
    L.check(L.lib().t2s_philox_normal(big.data_ptr(), seed, 1, 0, 4096, 1920, L.stream_ptr(dev)))
    assert abs(big.mean().item()) < 2e-3 and abs(big.std().item() - 1.0) < 2e-3


def test_philox_uniform_is_exact_sharding_invariant_and_in_range(dev):
    """t2s_philox_uniform (the per-row diffusion time of a training step, train.py:109,113): 24-bit uniforms, so the device
    values must EQUAL the numpy restatement, lie in [0, 1) -- floor(u * T) < T and never an out-of-table row -- and not
    depend on the sharding (rows 5.. drawn alone equal rows 5.. of the whole draw)."""
    from t2ms_amd.sampler import philox_uniform
    for row_elems in (1, 3, 7):
        got = philox_uniform(9, row_elems, 77, 12, 1000, dev)
        assert np.array_equal(got.cpu().numpy(), O.device_uniform(77, 12, 1000, 9, row_elems))
        assert torch.equal(philox_uniform(4, row_elems, 77, 12, 1005, dev), got[5:])
    big = philox_uniform(1 << 20, 1, 2025 ^ 0x74696D65, 3, 0, dev).view(-1)
    assert float(big.min()) >= 0.0 and float(big.max()) < 1.0 and abs(float(big.mean()) - 0.5) < 2e-3
    for T in (100, 1000):
        t = torch.floor(big * T).long()
        assert int(t.min()) == 0 and int(t.max()) == T - 1
        assert float((torch.bincount(t, minlength=T).float() / big.numel() * T - 1).abs().max()) < 0.15
    assert philox_uniform(0, 1, 1, 1, 0, dev).shape == (0, 1)


@pytest.mark.parametrize("L_", [24, 48, 96])
@pytest.mark.parametrize("B", [1, 5])
def test_vae_golden(golden_dir, dev, vae, L_, B):
    g = _load(golden_dir, "vae")
    xs = synth.make_series(100 + L_ + B, B, L_).to(dev)
    with torch.no_grad():
        z, before = vae.encoder(xs)
        rec, after = vae.decoder(z, length=L_)
        rec2, _ = vae.decoder(synth.make_latents(300 + L_, B).to(dev), length=L_)
    assert _maxdiff(z, g[f"z_{L_}_{B}"]) < 1e-5
    assert _maxdiff(before, g[f"before_{L_}_{B}"]) < 1e-5
    assert _maxdiff(after, g[f"after_{L_}_{B}"]) < 1e-5
    assert tuple(rec.shape) == g[f"rec_{L_}_{B}"].shape      # torch.squeeze rule: (L,) when B == 1
    assert _maxdiff(rec, g[f"rec_{L_}_{B}"]) < 1e-5
    assert _maxdiff(rec2, g[f"rec_rand_{L_}_{B}"]) < 2e-5


@pytest.mark.parametrize("L_", [512, 2048])
@pytest.mark.parametrize("B", [1, 3])
def test_vae_long_series_reference_fixture(golden_dir, dev, vae, L_, B):
    """LA-VAE beyond one LDS tile (L > 128: vqvae.py:57-71,97-105 accept any L; the reference's SUSHI set, dataloader.py:88-90,
    is 2048 long): the time-tiled encoder / decoder kernels against the REFERENCE run at L = 512 and 2048
    (tests/golden/vae_long.npz) -- z, recon in full, `before` / `after` at a stride coprime with the tile cores plus their
    fp64 row sums (every position enters) -- and the decode of a random latent for B = 1 (torch.squeeze's (L,) shape)."""
    g = _load(golden_dir, "vae_long")
    xs = synth.make_series(100 + L_ + B, B, L_).to(dev)
    st = 7 if L_ == 512 else 11
    with torch.no_grad():
        z, before = vae.encoder(xs)
        rec, after = vae.decoder(z, length=L_)
    assert tuple(rec.shape) == g[f"rec_{L_}_{B}"].shape
    assert _maxdiff(z, g[f"z_{L_}_{B}"]) < 1e-5 and _maxdiff(rec, g[f"rec_{L_}_{B}"]) < 1e-5
    assert _maxdiff(before[:, :, ::st], g[f"before_s{st}_{L_}_{B}"]) < 1e-5
    assert _maxdiff(after[:, :, ::st], g[f"after_s{st}_{L_}_{B}"]) < 1e-5
    for name, t in (("before", before), ("after", after)):
        rs = t.double().sum(2).cpu().numpy()
        assert np.abs(rs - g[f"{name}_rowsum_{L_}_{B}"]).max() < 1e-5 * (L_ // 4), name
    if B == 1:
        with torch.no_grad():
            rec2, _ = vae.decoder(synth.make_latents(300 + L_, B).to(dev), length=L_)
        assert _maxdiff(rec2, g[f"rec_rand_{L_}_{B}"]) < 2e-5


def test_vae_time_tiles_are_invisible(dev, vae):
    """Tiling at a length with ragged tiles (L = 260: 65 positions = 3 encoder / 3 decoder tiles, the last ones short)
    against the oracle; and the C ABI's refusal of a tiled encode without the `before` buffer."""
    L_, B = 260, 2
    xs = synth.make_series(7, B, L_)
    vsd = synth.make_vae_state_dict(2025)
    with torch.no_grad():
        z, before = vae.encoder(xs.to(dev))
        rec, after = vae.decoder(z, length=L_)
        zo, bo = O.vae_encode(vsd, xs)
        ro, ao = O.vae_decode(vsd, zo, L_)
    assert _maxdiff(z, zo) < 1e-5 and _maxdiff(before, bo) < 1e-5
    assert _maxdiff(rec, ro) < 1e-5 and _maxdiff(after, ao) < 1e-5
    # the C ABI refuses a tiled encode without the `before` buffer instead of skipping the interpolation
    x = xs.to(dev).contiguous()
    zz = torch.empty(B, 64, 30, device=dev)
    with torch.cuda.device(dev):
        rc = L.lib().t2s_vae_encode(vae.encoder._handle(dev), x.data_ptr(), zz.data_ptr(), None, B, L_, L.stream_ptr(dev))
    assert rc != 0 and b"before" in L.lib().t2s_last_error()


def _chain_setup(dev, vae):
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    m = m.to(dev).eval()
    xT = synth.make_latents(31337, 4)
    text = synth.make_text_embeddings(31337, 4)
    noises = torch.from_numpy(np.random.RandomState(99).randn(20, 4, 64, 30).astype(np.float32))
    return m, Sampler, xT, text, noises


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_chain_ddpm_golden(golden_dir, dev, vae, use_graph, lanes):
    g = _load(golden_dir, "chains")
    m, Sampler, xT, text, noises = _chain_setup(dev, vae)
    s = Sampler(m, vae.decoder, "ddpm", 20, 7.0, 4, 96, dev, use_graph=use_graph, lanes=lanes)
    lat, series, _ = s.run(text, x_T=xT, noise=noises)
    scale = max(1.0, float(np.abs(g["ddpm_latent"]).max()))
    assert _maxdiff(lat, g["ddpm_latent"]) < TOL * scale
    assert _maxdiff(series, g["ddpm_series"]) < TOL * scale
    # second run on the same sampler (graph replay) reproduces the first bit for bit
    lat2, series2, _ = s.run(text, x_T=xT, noise=noises)
    assert torch.equal(lat, lat2) and torch.equal(series, series2)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_chain_rf_golden(golden_dir, dev, vae, use_graph, lanes):
    g = _load(golden_dir, "chains")
    m, Sampler, xT, text, _ = _chain_setup(dev, vae)
    s = Sampler(m, vae.decoder, "flowmatching", 20, 7.0, 4, 96, dev, use_graph=use_graph, lanes=lanes)
    lat, series, _ = s.run(text, x_T=xT)
    scale = max(1.0, float(np.abs(g["rf_latent"]).max()))
    assert _maxdiff(lat, g["rf_latent"]) < TOL * scale
    assert _maxdiff(series, g["rf_series"]) < TOL * scale


@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_chain_without_the_whole_run_adaln_table(dev, vae, monkeypatch, backbone):
    """The sampler precomputes the adaLN modulation of every step (csrc/t2s_sampler.hip: mod_table) when the table fits;
    a device too full for it -- or T2S_ADALN_TABLE=0 -- keeps the per-step adaLN kernel in the loop.  Same MFMA order per
    row either way: the two paths agree bit for bit (graph and eager, one and two lanes)."""
    m, Sampler, xT, text, noises = _chain_setup(dev, vae)
    kw = dict(x_T=xT, noise=noises) if backbone == "ddpm" else dict(x_T=xT)
    ref = Sampler(m, vae.decoder, backbone, 20, 7.0, 4, 96, dev, use_graph=True, lanes=1).run(text, **kw)
    monkeypatch.setenv("T2S_ADALN_TABLE", "0")
    for use_graph, lanes in ((True, 1), (False, 1), (True, 2)):
        got = Sampler(m, vae.decoder, backbone, 20, 7.0, 4, 96, dev, use_graph=use_graph, lanes=lanes).run(text, **kw)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (use_graph, lanes)


def test_chain_stepwise_class_api_matches_fused(dev, vae):
    """The reference-style loop (infer.py:76-88) written against the mirrored classes gives the
    fused sampler's result (same kernels, same order)."""
    from model.backbone.DDPM import DDPM
    m, Sampler, xT, text, noises = _chain_setup(dev, vae)
    steps, cfg = 20, 7.0
    ddpm = DDPM(steps, dev)
    x = xT.to(dev)
    textd = text.to(dev)
    with torch.no_grad():
        for j in range(steps):
            t = torch.full((4,), steps - 1 - j, dtype=torch.long, device=dev)
            u = m(input=x, t=t, text_input=None)
            c = m(input=x, t=t, text_input=textd)
            pred = u + cfg * (c - u)      # torch glue, as in infer.py:87
            x = ddpm.p_sample(x, pred, t, eps=noises[j].to(dev))
    s = Sampler(m, vae.decoder, "ddpm", steps, cfg, 4, 96, dev, use_graph=True)
    lat, _, _ = s.run(text, x_T=xT, noise=noises)
    assert _maxdiff(lat, x) < 5e-5 * max(1.0, float(x.abs().max()))


def test_trace_and_perf_mode_sharding(dev, vae):
    """Perf mode (Philox noise): a 6-row batch equals two 3-row shards with row0 offsets, bit for bit
    (multi-GPU sharding is invisible in the results); trace decodes row 0 after every step."""
    m, Sampler, _, _, _ = _chain_setup(dev, vae)
    text = synth.make_text_embeddings(1, 6)
    full = Sampler(m, vae.decoder, "ddpm", 8, 5.0, 6, 48, dev, use_graph=True, seed=7, row0=0)
    lat, ser, _ = full.run(text)
    a = Sampler(m, vae.decoder, "ddpm", 8, 5.0, 3, 48, dev, use_graph=True, seed=7, row0=0)
    b = Sampler(m, vae.decoder, "ddpm", 8, 5.0, 3, 48, dev, use_graph=False, seed=7, row0=3)
    la, sa, _ = a.run(text[:3])
    lb, sb, tr = b.run(text[3:], trace=True)
    assert torch.equal(lat[:3], la) and torch.equal(lat[3:], lb)
    assert torch.equal(ser[:3], sa) and torch.equal(ser[3:], sb)
    assert tr.shape == (8, 48) and torch.equal(tr[-1], sb[0])


def test_class_api_pairs_the_two_cfg_calls_without_changing_a_bit(dev):
    """The mirror runs the reference loop's `model(x_t, t, None)` / `model(x_t, t, emb)` pair (infer.py:79-80, 85-86) as ONE
    2B-sequence CFG pass once it has seen the pattern, handing the conditional half out at the second call.  Every output
    must equal the un-paired forwards bit for bit, and every way the pattern can break must fall back to plain forwards:
    another text tensor, an x_t written in place between the two calls, a per-row t, a lone text-free call, new weights."""
    from model.denoiser.transformer import Transformer

    def fresh():
        m = Transformer()
        m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
        return m.to(dev).eval()

    m, ref = fresh(), fresh()
    B = 5
    emb = synth.make_text_embeddings(3, B).to(dev)
    emb2 = synth.make_text_embeddings(4, B).to(dev)

    def plain(x, t, text):                      # a model that never pairs: every call on its own
        ref.__dict__.pop("_t2s_pair", None)
        return ref(input=x, t=t, text_input=text)

    with torch.no_grad():
        x = synth.make_latents(9, B).to(dev)
        hits = 0
        for j in range(6):
            t = torch.full((B,), 17 - j, dtype=torch.long, device=dev) if j != 3 else torch.arange(B, device=dev) * 7   # per-row t
            u = m(input=x, t=t, text_input=None)
            stashed = m.__dict__["_t2s_pair"]["stash"] is not None
            c = m(input=x, t=t, text_input=emb)
            hits += int(stashed and m.__dict__["_t2s_pair"]["stash"] is None and m.__dict__["_t2s_pair"]["armed"])
            assert torch.equal(u, plain(x, t, None)) and torch.equal(c, plain(x, t, emb)), j
            x = x + 0.1 * (u + 2.0 * (c - u))
        assert hits == 5                          # every step after the first ran as one pass (the per-row t included)
        # another text tensor at the conditional call: the stash must not be handed out
        t = torch.full((B,), 3, dtype=torch.long, device=dev)
        u = m(input=x, t=t, text_input=None)
        c = m(input=x, t=t, text_input=emb2)
        assert torch.equal(c, plain(x, t, emb2))
        assert m.__dict__["_t2s_pair"]["stash"] is None and m.__dict__["_t2s_pair"]["text"] is emb2    # re-armed on the NEW text
        # re-arm, then write x_t in place between the two calls (version bump): recomputed on the new contents
        for _ in range(2):
            u = m(input=x, t=t, text_input=None)
            c = m(input=x, t=t, text_input=emb)
        u = m(input=x, t=t, text_input=None)
        assert m.__dict__["_t2s_pair"]["stash"] is not None
        x.mul_(0.5)
        c = m(input=x, t=t, text_input=emb)
        assert torch.equal(c, plain(x, t, emb))
        # lone text-free calls (e.g. an unconditional sampler) stay correct, and an unclaimed pass disarms the guessing
        # (otherwise every such call would pay for a conditional half nobody asks for)
        for _ in range(2):
            m(input=x, t=t, text_input=None)
            m(input=x, t=t, text_input=emb)
        for i in range(3):
            assert torch.equal(m(input=x, t=t, text_input=None), plain(x, t, None))
            assert m.__dict__["_t2s_pair"]["armed"] == (i == 0) and (m.__dict__["_t2s_pair"]["stash"] is not None) == (i == 0)
        # new weights between the two calls of a pair: the stash is stale and must be dropped
        for _ in range(2):
            m(input=x, t=t, text_input=None)
            m(input=x, t=t, text_input=emb)
        m(input=x, t=t, text_input=None)
        sd2 = synth.make_dit_state_dict(77, gain=0.7)
        m.load_state_dict(sd2, strict=True)
        ref.load_state_dict(sd2, strict=True)
        assert torch.equal(m(input=x, t=t, text_input=emb), plain(x, t, emb))


def test_infer_driver_end_to_end(dev, tmp_path, monkeypatch):
    """The drop-in driver: reference flags and path derivations, the four .npy files evaluation.py reads
    (infer.py:118-123,146), via synthetic data + seeded weights."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "results")
    argv = ["--dataset_name", "ETTh1_24", "--backbone", "ddpm", "--denoiser", "DiT", "--total_step", "3",
            "--cfg_scale", "9", "--batch_size", "4", "--save_path", save, "--synthetic", "10",
            "--random_init", "--seed", "11", "--trace"]
    drv.main(argv)
    out = os.path.join(save, "generation", "ddpm_DiT_ETTh1_24_9.0_3")
    n = (10 // 4) * 4     # drop_last: floor(rows / B) * B
    shapes = {"x_1.npy": (n, 24, 1), "x_t.npy": (n, 24, 1), "x_t_latent_dec_array.npy": (n, 64, 30),
              "x_t_latent_enc_array.npy": (n, 64, 30)}
    for f, shp in shapes.items():
        a = np.load(os.path.join(out, f))
        assert a.shape == shp and a.dtype == np.float32 and np.isfinite(a).all(), (f, a.shape, a.dtype)
    assert np.load(os.path.join(out, "x_infer_trace.npy")).shape == (3, 24)


def test_infer_coalesced_launches_write_the_per_batch_files_bitwise(dev, tmp_path, monkeypatch):
    """The reference launches the loop once per loader batch (infer.py:66-95; default --batch_size 2 = a 4-sequence CFG pass).
    infer.py samples the same rows in the same order `--launch_batch` series at a time: rows are independent, the kernels
    batch-invariant and Philox keyed by the global row, so the four files must not change by a byte -- whatever the launch
    size (incl. a ragged last launch), against the reference's launch shape (`--launch_batch 0`)."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    files = ("x_1.npy", "x_t.npy", "x_t_latent_dec_array.npy", "x_t_latent_enc_array.npy")
    got = {}
    for lb in (0, 64, 256):
        save = str(tmp_path / f"lb{lb}")
        drv.main(["--dataset_name", "ETTh1_48", "--total_step", "3", "--batch_size", "2", "--save_path", save, "--synthetic",
                  "151", "--random_init", "--seed", "9", "--launch_batch", str(lb)])
        out = os.path.join(save, "generation", "flowmatching_DiT_ETTh1_48_7_3")      # the reference's default backbone / cfg
        got[lb] = [np.load(os.path.join(out, f)) for f in files]
        assert got[lb][0].shape == (150, 48, 1) and got[lb][2].shape == (150, 64, 30)      # floor(151 / 2) * 2 rows
    for lb in (64, 256):
        for f, a, b in zip(files, got[0], got[lb]):
            assert np.array_equal(a, b), (lb, f)
    assert np.isfinite(got[0][1]).all() and float(np.abs(got[0][1]).max()) > 0


@pytest.mark.parametrize("backbone,steps,cfg", [("ddpm", 6, 9.0), ("flowmatching", 5, 7.0)])
def test_infer_driver_files_equal_the_oracle_end_to_end(dev, tmp_path, monkeypatch, backbone, steps, cfg):
    """infer.py itself against the CPU oracle: the four files of a DiT run (loader order, encoder, coalesced launches over
    a ragged tail, Philox x_T and per-step draws keyed by the GLOBAL row, CFG loop, decoder) must be what the oracle's
    restatement of infer.py:65-123 gives on the rows the files name -- the loop of the reference, not just its shapes."""
    import infer as drv
    from datafactory.dataset import SyntheticT2SDataset
    monkeypatch.chdir(tmp_path)
    seed, L_, n_ds, bs = 21, 48, 11, 2
    save = str(tmp_path / "res")
    drv.main(["--dataset_name", f"ETTh1_{L_}", "--backbone", backbone, "--denoiser", "DiT", "--total_step", str(steps),
              "--cfg_scale", str(cfg), "--batch_size", str(bs), "--save_path", save, "--synthetic", str(n_ds), "--random_init",
              "--seed", str(seed), "--launch_batch", "4"])                    # launches of 4 + 4 + 2 rows
    out = os.path.join(save, "generation", f"{backbone}_DiT_ETTh1_{L_}_{cfg}_{steps}")
    x1 = np.load(os.path.join(out, "x_1.npy"))[:, :, 0]
    xt = np.load(os.path.join(out, "x_t.npy"))[:, :, 0]
    lat = np.load(os.path.join(out, "x_t_latent_dec_array.npy"))
    enc = np.load(os.path.join(out, "x_t_latent_enc_array.npy"))
    n = (n_ds // bs) * bs
    assert x1.shape == xt.shape == (n, L_) and lat.shape == enc.shape == (n, 64, 30)
    ds = SyntheticT2SDataset(n_ds, L_)
    rows = [int(np.argmin(np.abs(ds.samples - x1[i][None]).sum(axis=1))) for i in range(n)]
    assert len(set(rows)) == n and np.allclose(ds.samples[rows], x1, atol=1e-6)       # a shuffled subset, each row once
    text = torch.from_numpy(ds.embedding[rows]).float()
    sd, vsd = synth.make_dit_state_dict(seed), synth.make_vae_state_dict(seed)
    with torch.no_grad():
        z_ref, _ = O.vae_encode(vsd, torch.from_numpy(x1))
        x_T = torch.from_numpy(O.device_normal(seed, 0xFFFFFFFF, 0, n)).view(n, 64, 30)
        if backbone == "ddpm":
            noises = [torch.from_numpy(O.device_normal(seed, j, 0, n)).view(n, 64, 30) for j in range(steps)]
            ref = O.sample_ddpm(sd, x_T, text, steps, cfg, noises)
        else:
            ref = O.sample_rf(sd, x_T, text, steps, cfg)
        series, _ = O.vae_decode(vsd, ref, L_)
    scale = max(1.0, float(ref.abs().max()))
    assert float(np.abs(enc - z_ref.numpy()).max()) < 1e-5
    assert float(np.abs(lat - ref.numpy()).max()) < 1e-4 * scale, float(np.abs(lat - ref.numpy()).max())
    assert float(np.abs(xt - series.reshape(n, L_).numpy()).max()) < 1e-4 * scale


def test_infer_driver_run_multi_layout(dev, tmp_path, monkeypatch):
    """`--run_multi True` (infer.py:148-164): the base run plus run_0 .. run_9, each with the four files.  The test loader
    shuffles (dataloader.py:111 does too), so every run holds the same ground-truth rows in its own order; the generated
    series differ from run to run (the seed advances)."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "results")
    drv.main(["--dataset_name", "ETTh1_24", "--backbone", "flowmatching", "--denoiser", "DiT", "--total_step", "2",
              "--cfg_scale", "7", "--batch_size", "4", "--save_path", save, "--synthetic", "8", "--random_init",
              "--seed", "3", "--run_multi", "True"])
    base = os.path.join(save, "generation", "flowmatching_DiT_ETTh1_24_7.0_2")
    x1 = np.load(os.path.join(base, "x_1.npy"))
    enc = np.load(os.path.join(base, "x_t_latent_enc_array.npy"))
    gens = [np.load(os.path.join(base, "x_t.npy"))]
    for r in range(10):
        d = os.path.join(base, f"run_{r}")
        x1r = np.load(os.path.join(d, "x_1.npy"))
        encr = np.load(os.path.join(d, "x_t_latent_enc_array.npy"))
        order, order_r = np.lexsort(x1[:, :, 0].T), np.lexsort(x1r[:, :, 0].T)
        assert np.array_equal(x1r[order_r], x1[order]) and np.array_equal(encr[order_r], enc[order])
        g = np.load(os.path.join(d, "x_t.npy"))
        assert g.shape == (8, 24, 1) and np.isfinite(g).all()
        assert np.load(os.path.join(d, "x_t_latent_dec_array.npy")).shape == (8, 64, 30)
        gens.append(g)
    assert not os.path.exists(os.path.join(base, "run_10"))
    for a in range(len(gens)):
        for b in range(a + 1, len(gens)):
            assert not np.array_equal(gens[a], gens[b]), (a, b)


def test_evaluation_driver_reads_the_infer_layout_and_writes_the_reference_json(dev, tmp_path, monkeypatch):
    """evaluation.py (drop-in for the reference's, evaluation.py:269-314) on what `infer.py --run_multi True` wrote: the two
    JSON files under {save_path}/evaluation/{model_name}/ with the reference's keys, the values equal to the metric kernels
    called directly on the files the reference pairs (x_1 of run_0 with the base x_t; x_1 of run_9 with the ten stacked
    runs); `--align_runs` pairs every run's rows with their own ground truth."""
    import glob
    import json
    import evaluation as ev
    import infer as drv
    from t2ms_amd import metrics as M
    monkeypatch.chdir(tmp_path)
    save = str(tmp_path / "results")
    drv.main(["--dataset_name", "ETTh1_24", "--total_step", "2", "--cfg_scale", "7", "--batch_size", "4", "--save_path", save,
              "--synthetic", "13", "--random_init", "--seed", "3", "--run_multi", "True", "--no_figs"])
    argv = ["--dataset_name", "ETTh1_24", "--cfg_scale", "7", "--total_step", "2", "--save_path", save, "--method_list",
            "MSE,WAPE,MRR,CRPS,ED"]
    single, multi = ev.main(argv)
    name = "flowmatching_DiT_ETTh1_24_7.0_2"
    g = os.path.join(save, "generation", name)
    x1 = np.load(os.path.join(g, "run_0", "x_1.npy"))
    xt = np.load(os.path.join(g, "x_t.npy"))
    mse, wape, _ = M.mse_wape(x1, xt)
    assert set(single) == {"MSE", "WAPE", "ED"} and single["MSE"] == mse and single["WAPE"] == wape
    x1_9 = np.load(os.path.join(g, "run_9", "x_1.npy"))
    gens = np.concatenate([np.load(os.path.join(g, f"run_{r}", "x_t.npy"))[..., None] for r in range(10)], axis=-1)
    assert set(multi) == {"MRR", "CRPS"} and multi["MRR"] == M.mrr(x1_9, gens)[0] and multi["CRPS"] == M.crps(x1_9, gens)[0]
    files = sorted(glob.glob(os.path.join(save, "evaluation", name, f"{name}_ETTh1_24_*.json")))
    assert len(files) == 2 and files[1].endswith("_multi.json")
    assert json.load(open(files[0])) == single and json.load(open(files[1])) == multi
    # aligned: rows of every run paired with their own ground truth -> the base run's MSE is that of its OWN (x_1, x_t)
    aligned, _ = ev.main(argv + ["--align_runs"])
    own = M.mse_wape(np.load(os.path.join(g, "x_1.npy")), xt)[0]
    assert abs(aligned["MSE"] - own) <= 1e-6 * max(1.0, own)


def test_config3_rectified_flow_full_batch(dev, vae):
    """BASELINE config 3 shape: B=1024 (2048 sequences per CFG pass), rectified flow, cfg 5, whole
    step in one hipGraph -- at 3 steps; rows must equal the same rows sampled in a 4-row batch
    bitwise, and agree with the oracle."""
    m, Sampler, _, _, _ = _chain_setup(dev, vae)
    B, steps, cfg = 1024, 3, 5.0
    xT = synth.make_latents(606, B)
    text = synth.make_text_embeddings(606, B)
    big = Sampler(m, vae.decoder, "flowmatching", steps, cfg, B, 96, dev, use_graph=True)
    lat, ser, _ = big.run(text, x_T=xT)
    rows = [0, 511, 512, 1023]
    small = Sampler(m, vae.decoder, "flowmatching", steps, cfg, 4, 96, dev, use_graph=True)
    lat4, ser4, _ = small.run(text[rows], x_T=xT[rows])
    assert torch.equal(lat[rows], lat4) and torch.equal(ser[rows], ser4)
    with torch.no_grad():
        ref = O.sample_rf(synth.make_dit_state_dict(31337, gain=0.7), xT[rows], text[rows], steps, cfg)
    assert _maxdiff(lat4, ref) < TOL * max(1.0, float(ref.abs().max()))
    assert bool(torch.isfinite(ser).all())


def test_config5_variable_length_encode_sample_decode(dev, vae):
    """BASELINE config 5: mixed lengths L in {24,48,96}: LA-VAE encode + DiT sampling + decode per
    length group, each group sharded over 2 'ranks' (row offsets) -- sharding must be invisible and
    every stage agrees with the oracle."""
    m, Sampler, _, _, _ = _chain_setup(dev, vae)
    sd = synth.make_dit_state_dict(31337, gain=0.7)
    vsd = synth.make_vae_state_dict(2025)
    steps, cfg, row = 4, 7.0, 0
    for L_ in (24, 48, 96):
        B = 6
        xs = synth.make_series(40 + L_, B, L_)
        text = synth.make_text_embeddings(40 + L_, B)
        with torch.no_grad():
            z, before = vae.encoder(xs.to(dev))
            z_ref, before_ref = O.vae_encode(vsd, xs)
        assert _maxdiff(z, z_ref) < 1e-5 and _maxdiff(before, before_ref) < 1e-5
        noises = torch.from_numpy(np.random.RandomState(L_).randn(steps, B, 64, 30).astype(np.float32))
        xT = synth.make_latents(50 + L_, B)
        full = Sampler(m, vae.decoder, "ddpm", steps, cfg, B, L_, dev, use_graph=True, row0=row)
        lat, ser, _ = full.run(text, x_T=xT, noise=noises)
        halves = []
        for lo, hi in ((0, 3), (3, 6)):
            s = Sampler(m, vae.decoder, "ddpm", steps, cfg, hi - lo, L_, dev, use_graph=True, row0=row + lo)
            halves.append(s.run(text[lo:hi], x_T=xT[lo:hi], noise=noises[:, lo:hi].contiguous()))
        assert torch.equal(torch.cat([h[0] for h in halves]), lat)
        assert torch.equal(torch.cat([h[1] for h in halves]), ser)
        with torch.no_grad():
            ref = O.sample_ddpm(sd, xT, text, steps, cfg, noises)
            ref_ser, _ = O.vae_decode(vsd, ref, L_)
        scale = max(1.0, float(ref.abs().max()))
        assert _maxdiff(lat, ref) < TOL * scale and _maxdiff(ser, ref_ser) < TOL * scale
        assert ser.shape == (B, L_)
        row += B


# ---------------------------------------------------------------------------- bf16x3 arithmetic (opt-in)
def test_attention_x3_kernel_vs_fp64(dev):
    """T2S_MATH_BF16X3 attention (six bf16 MFMAs per fp32 product): same tolerance as the f32 kernel against
    an fp64 softmax, with the spikes that force the stale-reference branch at early and late key blocks."""
    rs = np.random.RandomState(21)
    BH = 12
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 333] = q[:, 100] * 5.0
    k[:, 410] = q[:, 200] * 12.0
    k[:, 0:32] = -q[:, 7:8] * 3.0 + 0.01 * k[:, 0:32]
    k[:, 448] = q[:, 7] * 10.0
    ref = (torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double())
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    od = torch.empty_like(qd)
    L.check(L.lib().t2s_attn_fwd_x3(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), BH,
                                    L.stream_ptr(dev)), "t2s_attn_fwd_x3")
    err = (od.cpu().double() - ref).abs()
    assert float(err.max()) < 2e-5 and float(err.pow(2).mean().sqrt()) < 1e-6


@pytest.mark.parametrize("B", [3, 256])
def test_dit_forward_bf16x3_matches_f32_path(dev, B):
    """The whole forward under T2S_MATH_BF16X3 against the f32-MFMA path (itself within 1e-4 of the oracle):
    both are fp32-accurate, so they agree to a few ulp of the activations -- 2e-5 absolute."""
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    m = m.to(dev).eval()
    x = synth.make_latents(5, B).to(dev)
    t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(1)).to(dev)
    text = synth.make_text_embeddings(5, B).to(dev)
    with torch.no_grad():
        y32 = m(input=x, t=t, text_input=text)
        y3 = m.set_math("bf16x3")(input=x, t=t, text_input=text)
        y32b = m.set_math("f32")(input=x, t=t, text_input=text)
    assert torch.equal(y32, y32b)                      # switching back restores the f32 kernels bit for bit
    assert torch.isfinite(y3).all()
    assert _maxdiff(y3, y32) < 2e-5
    if B == 3:
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ref = O.dit_forward(sd, x.cpu(), t.cpu(), text.cpu())
        assert _maxdiff(y3, ref) < 1e-4


@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_chain_golden_in_bf16x3(golden_dir, dev, vae, backbone):
    """The reference-generated 20-step chains (tests/golden/chains.npz) with attention AND row chain in
    T2S_MATH_BF16X3, through the captured hipGraph: same tolerance as the f32-MFMA path."""
    g = _load(golden_dir, "chains")
    m, Sampler, xT, text, noises = _chain_setup(dev, vae)
    m.set_math("bf16x3")
    s = Sampler(m, vae.decoder, backbone, 20, 7.0, 4, 96, dev, use_graph=True)
    if backbone == "ddpm":
        lat, series, _ = s.run(text, x_T=xT, noise=noises)
        key = "ddpm"
    else:
        lat, series, _ = s.run(text, x_T=xT)
        key = "rf"
    scale = max(1.0, float(np.abs(g[key + "_latent"]).max()))
    assert _maxdiff(lat, g[key + "_latent"]) < TOL * scale
    assert _maxdiff(series, g[key + "_series"]) < TOL * scale


def test_bf16x3_follows_weight_updates(dev):
    """The split-plane weight copies are rebuilt by t2s_dit_update_weights (optimizer step / load_state_dict)."""
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    m = m.to(dev).eval().set_math("bf16x3")
    x = synth.make_latents(5, 3).to(dev)
    t = torch.tensor([1, 500, 999], device=dev)
    text = synth.make_text_embeddings(5, 3).to(dev)
    with torch.no_grad():
        y0 = m(input=x, t=t, text_input=text)
        m.load_state_dict(synth.make_dit_state_dict(7), strict=True)
        y1 = m(input=x, t=t, text_input=text)
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ref = O.dit_forward(sd, x.cpu(), t.cpu(), text.cpu())
    assert _maxdiff(y1, ref) < 1e-4 and _maxdiff(y0, y1) > 1e-3


def test_eval_mse_wape_vs_oracle(dev):
    """t2s_eval_mse_wape on an (N, L, 1) pair as infer.py writes it, incl. an all-zero row (WAPE NaN, skipped)."""
    from t2ms_amd.metrics import mse_wape
    rs = np.random.RandomState(8)
    ori = rs.uniform(0, 1, size=(37, 96, 1)).astype(np.float32)
    gen = (ori + 0.1 * rs.randn(37, 96, 1)).astype(np.float32)
    ori[5] = 0.0
    mse, wape, per = mse_wape(ori, gen, dev)
    np.testing.assert_allclose(mse, O.eval_mse(ori, gen), rtol=1e-5)
    np.testing.assert_allclose(wape, O.eval_wape(ori, gen), rtol=1e-5)
    assert np.isnan(per[5, 1].item()) and per.shape == (37, 2)
    # multi-series layout (N, L, 3): len = L * n_series
    o3, g3 = rs.randn(4, 24, 3).astype(np.float32), rs.randn(4, 24, 3).astype(np.float32)
    m3, w3, _ = mse_wape(o3, g3, dev)
    np.testing.assert_allclose(m3, O.eval_mse(o3, g3), rtol=1e-5)
    np.testing.assert_allclose(w3, O.eval_wape(o3, g3), rtol=1e-5)


def test_eval_mrr_vs_oracle(dev):
    """t2s_eval_mrr (evaluation.py:21-45) on 10 runs of (N, L, 1) series as `infer.py --run_multi` writes them:
    similarities, per-sample scores and the mean against the oracle, incl. a below-threshold row, an exact tie
    (later run wins) and an all-zero original."""
    from t2ms_amd.metrics import mrr
    rs = np.random.RandomState(9)
    n, runs = 41, 10
    ori = rs.uniform(-1, 1, size=(n, 96, 1)).astype(np.float32)
    gens = [(ori * rs.uniform(0.2, 1.0, size=(n, 1, 1)) + rs.uniform(0.1, 1.5) * rs.randn(n, 96, 1)).astype(np.float32)
            for _ in range(runs)]
    for g in gens:
        g[3] = rs.randn(96, 1)           # unrelated: every similarity below the threshold
    gens[2][7] = gens[6][7] = 2.0 * ori[7]   # exact tie at similarity 1: run 6 wins
    ori[11] = 0.0
    m, sims, score = mrr(ori, gens, 0.5, dev)
    stacked = np.stack(gens, axis=-1)
    ref_sims = np.array([[O.eval_cosine(ori[i], stacked[i, :, :, g]) for g in range(runs)] for i in range(n)])
    np.testing.assert_allclose(sims.numpy(), ref_sims, atol=2e-7)
    assert abs(m - O.eval_mrr(ori, stacked, 0.5)) < 1e-6
    assert score[3] == 0 and score[11] == 0 and abs(score[7].item() - 1 / 7) < 1e-7
    m2, _, _ = mrr(ori, stacked, 0.5, dev)   # the stacked (N, L, 1, G) form evaluation.py builds
    assert m2 == m


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
def test_two_lane_sampler_is_bitwise_one_lane(dev, vae, math):
    """t2s_sampler_set_lanes: the loop run as two half-batch chains on two streams (own graph, own step counter,
    own workspace slice, Philox rows by global index) gives bit for bit the one-lane result -- odd batch (19 + 18
    rows), perf-mode noise, graph and eager, and a re-run on the same sampler."""
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(2025), strict=True)
    m = m.to(dev).eval().set_math(math)
    B = 37
    text = synth.make_text_embeddings(5, B)
    ref = None
    for lanes, use_graph in ((1, True), (2, True), (2, False), (3, True), (4, True), (4, False)):
        s = Sampler(m, vae.decoder, "ddpm", 6, 9.0, B, 96, dev, use_graph=use_graph, seed=11, row0=100, lanes=lanes)
        lat, series, _ = s.run(text)
        if ref is None:
            ref = (lat, series)
            assert bool(torch.isfinite(series).all())
        else:
            assert torch.equal(lat, ref[0]) and torch.equal(series, ref[1]), (lanes, use_graph)
        lat2, series2 = s.run_inplace()
        assert torch.equal(lat2, ref[0]) and torch.equal(series2, ref[1])
    # the automatic choice (equal lanes: two for multiples of 64 and for 32 series, three for 96) against one lane, rectified flow
    for B in (128, 32, 96):
        text = synth.make_text_embeddings(6, B)
        outs = []
        for lanes in (1, 0):
            s = Sampler(m, vae.decoder, "flowmatching", 4, 5.0, B, 96, dev, seed=3, lanes=lanes)
            outs.append(s.run(text)[:2])
            assert s.graph_lanes == (1 if lanes == 1 else (3 if B == 96 else 2)), (B, lanes, s.graph_lanes)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), B
    s = Sampler(m, vae.decoder, "flowmatching", 4, 5.0, 48, 96, dev, seed=3, lanes=0)
    s.run(synth.make_text_embeddings(6, 48))
    assert s.graph_lanes == 1                                   # 48 does not split into whole 32-row groups: one lane
    # the smallest batches several lanes can take (1 + 1, 2 + 1 rows; four lanes asked of 3 rows run as three)
    for B in (2, 3):
        text = synth.make_text_embeddings(7, B)
        outs = [Sampler(m, vae.decoder, "ddpm", 3, 9.0, B, 96, dev, seed=5, lanes=lanes).run(text)[:2] for lanes in (1, 2, 4)]
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), B
    # the lanes ran on the library's calibrated stream pool: at least two of its streams really overlap on this device
    # (HIP streams that share a hardware queue execute one after the other -- DESIGN.md 4.5)
    # (timing-based calibration: informational beyond "the pool exists" -- a busy chip may show fewer overlapping streams)
    assert L.lib().t2s_sampler_lane_pool() >= 1, L.lib().t2s_sampler_lane_pool()
    # bad lane counts are refused with the library's error code, not clamped
    assert L.lib().t2s_sampler_set_lanes(s.ptr, 5) != 0 and L.lib().t2s_sampler_set_lanes(s.ptr, -1) != 0
    assert L.lib().t2s_sampler_set_lanes(s.ptr, 4) == 0 and L.lib().t2s_sampler_set_lanes(s.ptr, 2) == 0


def test_every_launch_shape_reproduces_itself_beside_foreign_traffic(dev, dit, vae):
    """A short cut of tools/stress_determinism.py for the hand-counted vmcnt / lgkmcnt rings (tests/test_isa_pins.py pins
    their ISA shape; this checks their behaviour): every launch shape of the DiT forward -- 16- and 32-token row tiles,
    packed and persistent attention, partial tiles, conditional and text-free -- and of the fused sampler (graph replay,
    one / two / three lanes, adaLN table) is run three times while another stream streams 256 MB through HBM, and must
    reproduce its first result bit for bit.  One pass: a property check, not a hunt."""
    from t2ms_amd.sampler import Sampler
    side = torch.cuda.Stream(dev)
    junk = torch.randn(64 << 20, device=dev)
    with torch.no_grad():
        for B in (1, 3, 7, 16, 25, 32, 50, 64, 100, 128, 256):
            x = synth.make_latents(100 + B, B).to(dev)
            t = torch.full((B,), 500, dtype=torch.long, device=dev)
            text = synth.make_text_embeddings(100 + B, B).to(dev)
            first = None
            for rep in range(3):
                with torch.cuda.stream(side):
                    junk.mul_(1.0000001)
                got = (dit(input=x, t=t, text_input=text), dit(input=x, t=t, text_input=None))
                if first is None:
                    first = got
                    assert bool(torch.isfinite(got[0]).all())
                else:
                    assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), (B, rep)
        for B in (8, 32, 96, 256):
            s = Sampler(dit, vae.decoder, "ddpm", 12, 9.0, B, 96, dev, seed=5)
            lat0, ser0, _ = s.run(synth.make_text_embeddings(7, B).to(dev))
            for rep in range(2):
                with torch.cuda.stream(side):
                    junk.mul_(1.0000001)
                lat, ser = s.run_inplace()
                torch.cuda.synchronize(dev)
                assert torch.equal(lat, lat0) and torch.equal(ser, ser0), (B, rep)
    torch.cuda.synchronize(dev)


def test_whole_loop_graph_equals_step_graph_bitwise(dev, dit, vae):
    """SURVEY 8(d) config 3 words the loop as "whole loop in one hipGraph": t2s_sampler_set_loop_graph(1) captures steps x
    (forward + update) nodes per lane and launches them once; the default replays a one-step graph `steps` times.  Every
    node reads its loop index from the lane's device counter, so the two -- and an eager run -- must agree bit for bit,
    for both backbones, one and two lanes, and across a change of form on one sampler (re-capture)."""
    from t2ms_amd.sampler import Sampler
    for backbone, steps, cfg, B in (("flowmatching", 20, 5.0, 64), ("ddpm", 12, 9.0, 7)):
        text = synth.make_text_embeddings(3, B).to(dev)
        ref = Sampler(dit, vae.decoder, backbone, steps, cfg, B, 96, dev, use_graph=False, seed=9).run(text)
        for lanes in (1, 2):
            s = Sampler(dit, vae.decoder, backbone, steps, cfg, B, 96, dev, use_graph=True, seed=9, lanes=lanes, loop_graph=1)
            lat, ser, _ = s.run(text)
            assert torch.equal(lat, ref[0]) and torch.equal(ser, ref[1]), (backbone, lanes)
            lat2, ser2 = s.run_inplace()                                  # the replay of the whole-loop graph
            assert torch.equal(lat2, ref[0]) and torch.equal(ser2, ref[1])
            L.check(L.lib().t2s_sampler_set_loop_graph(s.ptr, 0))         # back to the one-step form: re-captured
            lat3, ser3 = s.run_inplace()
            assert torch.equal(lat3, ref[0]) and torch.equal(ser3, ref[1])
    assert L.lib().t2s_sampler_set_loop_graph(s.ptr, 2) != 0


def test_two_host_threads_drive_two_samplers_on_one_device(dev, vae):
    """Every multi-lane sampler of a process runs on ONE per-device pool of lane streams (lane 0 included).  Two host
    threads driving two samplers at once would capture / record / launch on the same streams -- one thread's work pulled
    into the other's capture, or hipErrorStreamCaptureIsolation -- unless a run holds the pool for the length of its
    enqueue (round-3 ADVICE, medium).  Both threads must finish without an error and reproduce, bit for bit, what each
    sampler gives alone; repeated so that captures (first run) and replays (later runs) of the two meet."""
    import threading
    from t2ms_amd.sampler import Sampler
    from model.denoiser.transformer import Transformer
    models = []
    for seed in (31337, 4242):
        m = Transformer()
        m.load_state_dict(synth.make_dit_state_dict(seed, gain=0.7), strict=True)
        models.append(m.to(dev).eval())
    texts = [synth.make_text_embeddings(21 + i, 64).to(dev) for i in range(2)]
    want = []
    for i in range(2):
        s = Sampler(models[i], vae.decoder, "ddpm", 5, 9.0, 64, 48, dev, seed=100 + i, lanes=2)
        lat, ser, _ = s.run(texts[i])
        assert s.graph_lanes == 2
        want.append((lat.clone(), ser.clone()))
    torch.cuda.synchronize(dev)
    got, errors = [[], []], []

    def work(i):
        try:
            torch.cuda.set_device(dev)
            for rep in range(6):
                s = Sampler(models[i], vae.decoder, "ddpm", 5, 9.0, 64, 48, dev, seed=100 + i, lanes=2)    # fresh: captures
                for _ in range(2):
                    lat, ser, _ = s.run(texts[i])
                    got[i].append((lat.clone(), ser.clone()))
            torch.cuda.synchronize(dev)
        except Exception as e:                       # noqa: BLE001 -- reported by the assertion below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    mismatches = [(i, k) for i in range(2) for k, (lat, ser) in enumerate(got[i])
                  if not (torch.equal(lat, want[i][0]) and torch.equal(ser, want[i][1]))]
    if errors or mismatches or any(len(g) != 12 for g in got):
        # KEEP the evidence (round 4 saw one failure of this test and kept none of its output: which call failed with which
        # error stayed unknown): the T2SError texts carry the failing entry point and HIP's error string
        import json
        import time
        os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out",
                            f"two_thread_failure_{int(time.time())}.json")
        json.dump({"errors": errors, "mismatches": mismatches, "runs_done": [len(g) for g in got],
                   "last_error": L.lib().t2s_last_error().decode("utf-8", "replace"), "lane_pool": int(L.lib().t2s_sampler_lane_pool())},
                  open(path, "w"), indent=1)
        print("two-thread failure recorded in", path)
    assert not errors, errors
    for i in range(2):
        assert len(got[i]) == 12
    assert not mismatches, mismatches


# ---------------------------------------------------------------- 1000-step chain at the headline schedule
@pytest.mark.parametrize("math,lanes", [("f32", 1), ("f32", 2), ("bf16x3", 1)])
def test_chain_1000_steps_reference(dev, vae, math, lanes):
    """north_star: "outputs matching the reference CPU path within fp32 1e-4 on fixed seeds" for the 1000-step run.
    infer.py:76-88 at --total_step 1000, cfg 9.0, B=2 through the REFERENCE (tests/golden/chain1000.npz, injected
    draws regenerated from their seeds) against the fused sampler: hipGraph replayed 1000 times, one and two lanes,
    f32 MFMA and the fp32-accurate bf16x3 arithmetic.  Tolerance 1e-4 relative to max|x| (1.2e3 at the end: an
    untrained model does not cancel the schedule's growth), series 1e-4 relative to max|series|."""
    from model.denoiser.transformer import Transformer
    from t2ms_amd.sampler import Sampler
    from _chain1000 import chain1000_inputs, check_chain1000
    xT, text, noises = chain1000_inputs()
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    m = m.to(dev).eval().set_math(math)
    s = Sampler(m, vae.decoder, "ddpm", 1000, 9.0, 2, 96, dev, use_graph=True, lanes=lanes)
    lat, series, _ = s.run(text, x_T=xT, noise=noises)
    check_chain1000(lat.cpu().numpy(), series.cpu().numpy(), {}, label=f"fused sampler {math} lanes={lanes}")


def test_chain_1000_steps_stepwise_taps(dev, vae):
    """The same chain through the mirrored CLASSES (Transformer.forward x 2, torch CFG glue, DDPM.p_sample), checked
    against the reference after loop indices 0, 1, 9, 99, 499, 998, 999: 1e-4 relative to the state's size there."""
    from model.backbone.DDPM import DDPM
    from model.denoiser.transformer import Transformer
    from _chain1000 import CHAIN_TAPS, chain1000_inputs, check_chain1000
    xT, text, noises = chain1000_inputs()
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    m = m.to(dev).eval()
    ddpm = DDPM(1000, dev)
    x, textd, nz = xT.to(dev), text.to(dev), noises.to(dev)
    taps = {}
    with torch.no_grad():
        for j in range(1000):
            t = torch.full((2,), 999 - j, dtype=torch.long, device=dev)
            u = m(input=x, t=t, text_input=None)
            c = m(input=x, t=t, text_input=textd)
            x = ddpm.p_sample(x, u + 9.0 * (c - u), t, eps=nz[j])
            if j in CHAIN_TAPS:
                taps[j] = x.cpu().numpy()
        series, _ = vae.decoder(x, length=96)
    check_chain1000(x.cpu().numpy(), series.cpu().numpy(), taps, label="class API f32")


# ---------------------------------------------------------------- evaluation metrics against the reference's own functions
def test_eval_ed_crps_mse_wape_mrr_reference_fixture(golden_dir, dev):
    """t2s_eval_* against evaluation.py's calculate_mse / _wape / _ed / _crps / _mrr as the generator ran them
    (tests/golden/metrics.npz: an all-zero row, negated runs, an exact copy at run 7)."""
    from t2ms_amd import metrics as M
    g = _load(golden_dir, "metrics")
    ori, gen, runs = g["ori"], g["gen"], g["runs"]
    mse, wape, _ = M.mse_wape(ori, gen)
    np.testing.assert_allclose(mse, float(g["mse"]), rtol=2e-6)
    np.testing.assert_allclose(wape, float(g["wape"]), rtol=2e-6)
    np.testing.assert_allclose(M.ed(ori, gen)[0], float(g["ed"]), rtol=2e-6)
    np.testing.assert_allclose(M.crps(ori, runs)[0], float(g["crps"]), rtol=1e-5)
    m, sims, _ = M.mrr(ori, runs)
    assert abs(m - float(g["mrr"])) < 1e-6
    np.testing.assert_allclose(sims.numpy(), g["sims"], rtol=1e-5, atol=1e-6)
    assert (sims[4] == 0).all() and bool(torch.isfinite(sims).all())          # the all-zero row: exact zeros, never NaN
    np.testing.assert_allclose(M.fid(g["fid_act1"], g["fid_act2"]), float(g["fid"]), rtol=1e-9)


def test_eval_dtw_vs_oracle(dev):
    """t2s_eval_dtw against the oracle's restatement of dtaidistance's dtw_ndim.distance (UNPINNED: third party, absent)
    on (N, L, n_series) arrays with L in {24, 96} and 1 or 3 series, plus the known answers (shift-invariance of a step)."""
    from t2ms_amd import metrics as M
    rs = np.random.RandomState(5)
    for L_, S in ((24, 1), (96, 1), (40, 3)):
        a = rs.uniform(0, 1, size=(6, L_, S)).astype(np.float32)
        b = (a + 0.3 * rs.randn(6, L_, S)).astype(np.float32)
        got, per = M.dtw(a, b)
        np.testing.assert_allclose(got, O.eval_dtw(a, b), rtol=1e-5)
        assert per.shape == (6,)
    a = np.zeros((1, 8, 1), np.float32)
    a[0, 3:, 0] = 1.0
    b = np.zeros((1, 8, 1), np.float32)
    b[0, 5:, 0] = 1.0
    assert M.dtw(a, b)[0] == 0.0


def test_ts2vec_encoder_reference_fixture(golden_dir, dev):
    """t2s_ts2vec_encode against TSEncoder.forward of the reference (tests/golden/ts2vec.npz, seeded weights, a NaN
    stretch in one series): per-step representations and the full-series max pooling, 1e-4 relative to max|rep|;
    C-FID of two sets through the same encoder equals the oracle's."""
    from t2ms_amd import metrics as M
    g = _load(golden_dir, "ts2vec")
    sd = synth.make_ts2vec_state_dict(2025)
    enc = M.TS2VecEncoder(sd, dev)
    x = torch.from_numpy(g["x"])
    rep = enc.encode(x, encoding_window=None).cpu().numpy()
    full = enc.encode(x).cpu().numpy()
    scale = float(np.abs(g["rep"]).max())
    assert rep.shape == (5, 96, 100) and full.shape == (5, 100)
    assert float(np.abs(rep[:, ::6] - g["rep"]).max()) <= TOL * scale
    assert float(np.abs(full - g["full_series"]).max()) <= TOL * scale
    rs = np.random.RandomState(3)
    a = rs.uniform(0, 1, size=(40, 24, 1)).astype(np.float32)
    b = (a + 0.2 * rs.randn(40, 24, 1)).astype(np.float32)
    with torch.no_grad():
        ra = O.ts2vec_encode(sd, torch.from_numpy(a))[1].numpy()
        rb = O.ts2vec_encode(sd, torch.from_numpy(b))[1].numpy()
    np.testing.assert_allclose(M.cfid(a, b, enc), O.eval_fid(ra, rb), rtol=2e-3)


def test_sampler_set_row0_keeps_graph_and_matches_fresh_sampler(dev, vae):
    """infer.py walks the test loader with ONE sampler: t2s_sampler_set_row0 moves it to another shard position without
    re-capturing the hipGraph (the Philox row key is read from device memory).  The result must equal a sampler created
    at that position, bit for bit, and the corresponding rows of one big batch (sharding invariance)."""
    from t2ms_amd.sampler import Sampler
    from model.denoiser.transformer import Transformer
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    m = m.to(dev).eval()
    text = synth.make_text_embeddings(4, 6).to(dev)
    big = Sampler(m, vae.decoder, "ddpm", 6, 7.0, 6, 48, dev, use_graph=True, seed=77, row0=10)
    lat_big, ser_big, _ = big.run(text)
    s = Sampler(m, vae.decoder, "ddpm", 6, 7.0, 3, 48, dev, use_graph=True, seed=77, row0=10)
    lat_a, ser_a, _ = s.run(text[:3].contiguous())
    ptr_before = s.ptr.value
    s.set_row0(13)
    lat_b, ser_b, _ = s.run(text[3:].contiguous())
    assert s.ptr.value == ptr_before                                   # the C sampler (and its graph) was kept
    fresh = Sampler(m, vae.decoder, "ddpm", 6, 7.0, 3, 48, dev, use_graph=True, seed=77, row0=13)
    lat_c, ser_c, _ = fresh.run(text[3:].contiguous())
    assert torch.equal(lat_b, lat_c) and torch.equal(ser_b, ser_c)
    assert torch.equal(torch.cat([lat_a, lat_b]), lat_big) and torch.equal(torch.cat([ser_a, ser_b]), ser_big)


# ---------------------------------------------------------------- strong-scaling shards (256 series over 1/2/4/8 GPUs)
def test_strong_scaling_shards_equal_the_full_batch_bitwise(dev, dit, vae):
    """BASELINE's metric is B = 256 at 1/2/4/8 GPUs: a strong-scaling rank samples 128 / 64 / 32 of the 256 series.  Those
    shard sizes take other launch shapes than the full batch (one sampler lane below 128 series, the persistent
    attention kernel at exactly one head per CU at 32, a row chain that no longer fills every SIMD) -- the rows a rank
    produces must still be bit for bit the rows of the one-GPU batch (Philox keyed by the global row; batch-invariant
    kernels).  12 steps of the headline schedule shape (DDPM, cfg 9)."""
    from t2ms_amd.sampler import Sampler
    steps, B = 12, 256
    text = synth.make_text_embeddings(2025, B)
    full = Sampler(dit, vae.decoder, "ddpm", steps, 9.0, B, 96, dev, use_graph=True, seed=2025, row0=0)
    lat, ser, _ = full.run(text)
    assert bool(torch.isfinite(ser).all())
    for world in (2, 4, 8):
        n = B // world
        s = Sampler(dit, vae.decoder, "ddpm", steps, 9.0, n, 96, dev, use_graph=True, seed=2025, row0=0)
        for rank in sorted({0, world // 2, world - 1}):
            s.set_row0(rank * n)
            la, sa, _ = s.run(text[rank * n:(rank + 1) * n].contiguous())
            assert torch.equal(la, lat[rank * n:(rank + 1) * n]), (world, rank)
            assert torch.equal(sa, ser[rank * n:(rank + 1) * n]), (world, rank)


def test_sampler_null_stream_with_graph_is_not_an_eager_fallback(dev, vae):
    """Direct C-ABI caller: stream = NULL ("default stream", include/t2s.h) with use_graph = 1.
    The default stream cannot be captured, so the sampler must capture / replay on a stream of its own, ordered after
    and joined back to the default stream -- and report that it holds a graph; the result equals a run on an explicit
    stream bit for bit."""
    m, Sampler, xT, text, noises = _chain_setup(dev, vae)
    lib = L.lib()
    ref_s = Sampler(m, vae.decoder, "ddpm", 20, 7.0, 4, 96, dev, use_graph=True, lanes=1)
    ref_lat, ref_ser, _ = ref_s.run(text, x_T=xT, noise=noises)
    assert lib.t2s_sampler_graph_lanes(ref_s.ptr) == 1
    for lanes in (1, 2):
        s = Sampler(m, vae.decoder, "ddpm", 20, 7.0, 4, 96, dev, use_graph=True, lanes=lanes)
        assert lib.t2s_sampler_graph_lanes(s.ptr) == 0          # nothing captured yet
        x = xT.to(dev).clone()
        td, nd = text.to(dev).contiguous(), noises.to(dev).contiguous()
        series = torch.empty(4, 96, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.device(dev):
            for _ in range(2):                                  # second call replays the kept graph
                x.copy_(xT.to(dev))
                torch.cuda.synchronize(dev)
                L.check(lib.t2s_sampler_run(s.ptr, x.data_ptr(), td.data_ptr(), nd.data_ptr(), series.data_ptr(), None,
                                            None), "t2s_sampler_run(NULL stream)")
                # joined back to the default stream: waiting for THAT stream alone (torch's default stream is the
                # NULL stream) must be enough to see the result
                assert torch.cuda.default_stream(dev).cuda_stream == 0
                torch.cuda.default_stream(dev).synchronize()
                assert lib.t2s_sampler_graph_lanes(s.ptr) == lanes
                assert torch.equal(x, ref_lat) and torch.equal(series, ref_ser)
