"""TSae codec, what needs no GPU: the mirror's state-dict layout, its torch-op path and the plain-tensor restatement
(tests/_tsae_ref.py, explicit key/value cache) against the reference's recorded outputs (tests/golden/tsae.npz), the routing
predicate condition by condition, and the tool's command line; and the inputs of the case table (tests/_tsae_cases.py) that
tests/test_tsae_fp64.py runs on the GPU: each case is well conditioned (the fp32 restatement within a quarter of the bar of the
fp64 one) and, at gain 4, really stresses the softmax."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import _tsae_cases as TC
import _tsae_fixture as FX
import _tsae_ref as R
from t2ms_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref, what):
    err, b = float((got.double() - ref.double()).abs().max()), FX.bar(ref)
    print(f"{what}: max|err| {err:.3e} bar {b:.3e}")
    assert got.shape == ref.shape and err <= b, (what, err, b)


def test_fixture_is_its_own_witness():
    """Every recorded output's fp32-vs-fp64 deviation of the reference is at most a quarter of the bar."""
    z, plan = FX.golden()
    assert len(plan["cases"]) == 17
    for c in plan["cases"]:
        for name in ("memory", "pred", "gen"):
            assert float(z[f"dev_{name}_{FX.case_key(c)}"]) <= FX.bar(FX.expected(c, name)) / 4


def test_state_dict_layout_is_the_references():
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    plan = FX.golden()[1]
    m = AttentionSeq2SeqAutoencoder(FX.args_of("bp"))
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == plan["state_dict_bp"]
    assert got["condition_fusion.text_projection.weight"] == [64, 393216]
    m.load_state_dict(FX.state_dict("bp", fusion=True), strict=True)             # a full reference-layout state dict loads
    n = sum(p.numel() for k, p in m.named_parameters() if not k.startswith("condition_fusion."))
    assert n == 253322
    assert type(m).__module__ == "model.pretrained.TSae"


@pytest.mark.parametrize("c", FX.cases(), ids=FX.case_ids())
def test_mirror_torch_path_matches_reference(c, monkeypatch):
    monkeypatch.setenv("T2S_TSAE", "torch")
    m, x = FX.mirror(c["cfg"]), FX.case_input(c)
    with torch.no_grad():
        memory = m.encoder(x)
        _close(memory, FX.expected(c, "memory"), "memory")
        _close(m.decoder(FX.expected(c, "memory"), x), FX.expected(c, "pred"), "pred")
        _close(m.forward_inference(x, None), FX.expected(c, "gen"), "gen")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("c", FX.cases(), ids=FX.case_ids())
def test_plain_restatement_matches_reference(c, dtype):
    """The explicit key/value cache of _tsae_ref.generate reproduces the reference's recompute-everything generation."""
    sd = {k: v.to(dtype) for k, v in FX.state_dict(c["cfg"]).items()}
    heads, x = FX.cfg_of(c)["heads"], FX.case_input(c)
    memory = R.encode(sd, x, heads)
    _close(memory, FX.expected(c, "memory"), "memory")
    _close(R.decode(sd, FX.expected(c, "memory"), x, heads), FX.expected(c, "pred"), "pred")
    _close(R.generate(sd, memory, heads), FX.expected(c, "gen"), "gen")


def test_sinusoid_table_is_the_references():
    """_tsae_ref forms the table as the reference's buffer is formed: equal to the recorded samples up to the last bit of
    torch's sin / cos (1 ulp of a value <= 1), and to the seeded state dict's `pe`."""
    plan = FX.golden()[1]
    pe = R.sinusoid_table(2000, 64)
    assert float((pe[:8].double() - torch.tensor(plan["pe_head"])).abs().max()) <= 2.0 ** -23
    assert float((pe[1999].double() - torch.tensor(plan["pe_last"])).abs().max()) <= 2.0 ** -23
    assert float((FX.state_dict("bp")["encoder.positional_encoding.pe"][0] - pe).abs().max()) <= 2.0 ** -23


def test_route_conditions():
    from t2ms_amd.model.pretrained import tsae as M
    assert M._route(False, False, False, True, False) == "hip"
    for i in range(5):                                       # each condition alone sends the call to the torch ops
        a = [False, False, False, True, False]
        a[i] = not a[i]
        assert M._route(*a) == "torch", i
    ok = dict(n_features=10, d_model=64, d_ff=128, heads=8, layers=3, T=144)
    assert M._covered(**ok)
    for k, v in (("n_features", 0), ("n_features", 17), ("d_model", 128), ("d_ff", 96), ("d_ff", 576), ("heads", 2), ("heads", 16),
                 ("layers", 0), ("layers", 7), ("T", 0), ("T", 2001)):
        assert not M._covered(**{**ok, k: v}), (k, v)
    for k, v in (("n_features", 1), ("n_features", 16), ("d_ff", 64), ("d_ff", 512), ("heads", 4), ("layers", 1), ("layers", 6),
                 ("T", 1), ("T", 2000)):
        assert M._covered(**{**ok, k: v}), (k, v)


def test_route_of_a_module(monkeypatch):
    monkeypatch.delenv("T2S_TSAE", raising=False)
    m = FX.mirror("bp")
    x = FX.case_input(FX.cases()[4])
    enc, dec = m.encoder, m.decoder
    with torch.no_grad():
        assert enc._route_of(x, x.shape[1], False, x.shape[0]) == "hip"
        assert enc._route_of(x, x.shape[1], True, x.shape[0]) == "torch"                     # a mask
        assert enc._route_of(x, 2001, False, x.shape[0]) == "torch"                          # an uncovered shape
        monkeypatch.setenv("T2S_TSAE", "torch")
        assert enc._route_of(x, x.shape[1], False, x.shape[0]) == "torch"                    # the switch, read at call time
        monkeypatch.setenv("T2S_TSAE", "fast")
        with pytest.raises(L.T2SError, match="T2S_TSAE"):
            enc._route_of(x, x.shape[1], False, x.shape[0])
        monkeypatch.delenv("T2S_TSAE")
        try:
            enc.train()
            assert enc._route_of(x, x.shape[1], False, x.shape[0]) == "torch"                # training mode: dropout
        finally:
            enc.eval()
    assert dec._route_of(x, x.shape[1], False, x.shape[0]) == "torch"                        # grad enabled, parameters want one
    # an uncovered configuration takes the torch ops end to end, on the CPU
    from model.pretrained.TSae import TimeSeriesEncoder
    wide = TimeSeriesEncoder(n_features=3, flow_dim=32, num_layers=1, d_ff=64, num_heads=4).eval()
    with torch.no_grad():
        assert wide(torch.zeros(1, 5, 3)).shape == (1, 5, 32)


def test_hip_route_refuses_cpu_tensors(monkeypatch):
    monkeypatch.delenv("T2S_TSAE", raising=False)
    m = FX.mirror("bp")
    x = FX.case_input(FX.cases()[4])
    with torch.no_grad():
        with pytest.raises(L.T2SError, match="GPU"):
            m.encoder(x)
        with pytest.raises(L.T2SError, match="GPU"):
            m.decoder(FX.expected(FX.cases()[4], "memory"), x)
        with pytest.raises(L.T2SError, match="GPU"):
            m.decoder.generate(FX.expected(FX.cases()[4], "memory"))
    with pytest.raises(L.T2SError, match="GPU"):
        m.shared_eval(x, None, None, "test")


def test_train_mode_shared_eval_steps_on_torch_ops():
    """shared_eval(..., 'train') wants gradients: torch ops under autograd, on any device; one step lowers nothing by itself
    but must change the parameters and return a finite loss."""
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    m = AttentionSeq2SeqAutoencoder(FX.args_of("h4"))
    m.load_state_dict(FX.state_dict("h4"), strict=False)
    m.condition_fusion = None
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    before = m.decoder.output_projection.weight.detach().clone()
    loss, recon = m.shared_eval(FX.case_input(FX.cases()[-2]), None, opt, "train")
    assert torch.isfinite(loss) and recon.shape == (2, 8, 10)
    assert not torch.equal(before, m.decoder.output_projection.weight)


def test_symbols_declared():
    for name in ("t2s_tsae_create", "t2s_tsae_destroy", "t2s_tsae_workspace_bytes", "t2s_tsae_encode", "t2s_tsae_decode",
                 "t2s_tsae_generate", "t2s_tsae_positional"):
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)


def test_switch_is_documented():
    assert "T2S_TSAE" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_reconstruct_tool_help_parses():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tsae_reconstruct.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--random_init" in r.stdout and "--state_dict" in r.stdout


# ---- the case table of tests/_tsae_cases.py ---------------------------------------------------------------------------------
GATED = TC.TABLE + (TC.MIRROR,)
GATED_IDS = TC.IDS + ["mirror_" + TC.case_id(TC.MIRROR)]


@functools.lru_cache(maxsize=None)
def _restated(c, dtype):
    """(memory, teacher-forced prediction, generation) of the restatement in `dtype`, computed once per case."""
    sd, x = TC.state_dict_as(c, dtype), TC.series(c)
    memory = R.encode(sd, x, c.heads)
    return memory, R.decode(sd, memory, x, c.heads), R.generate(sd, memory, c.heads)


def test_table_reaches_the_kernels_branch_points():
    """What the table is for, as data: the d_ff chunkings, layer counts, feature widths and lengths the recorded fixture lacks."""
    t = [c for c in TC.TABLE if c.gain == 4.0]
    assert 20 <= len(TC.TABLE) <= 25 and len(set(TC.TABLE)) == len(TC.TABLE) and max(c.gain for c in GATED) == 4.0
    assert {64, 192, 512} <= {c.d_ff for c in t} and {320, 448} & {c.d_ff for c in t}
    assert {(6, 6), (2, 1), (1, 2)} <= {(c.n_enc, c.n_dec) for c in t}
    assert any((c.n_enc, c.n_dec, c.heads) == (3, 3, 4) for c in t)
    assert any((c.n_enc, c.n_dec, c.d_ff, c.n_features) == (6, 6, 512, 16) for c in t)
    assert {1, 5} <= {c.n_features for c in t}
    for T in (31, 32, 33, 63, 64, 127, 128, 129, 257):
        assert any(c.T == T and c.B in (1, 3) for c in t), T
    assert any(c.B == 5 and c.n_dec >= 3 for c in t)
    assert any((c.T, c.B, c.heads, c.d_ff, c.n_enc, c.n_dec) == (2000, 1, 4, 192, 2, 1) for c in t)
    assert any((c.T, c.heads, c.n_enc, c.n_dec) == (600, 8, 1, 2) for c in t)
    assert TC.TABLE[0] == TC.BP_GAIN1 and TC.TABLE[1] == TC.BP_GAIN1._replace(gain=4.0)
    k = FX.golden()[1]["cfgs"]["bp"]
    assert (k["n_features"], k["d_ff"], k["n_enc"], k["n_dec"], k["heads"], k["seed"]) == TC.BP_GAIN1[:5] + (TC.BP_GAIN1.seed,)
    assert TC.BAR == FX.golden()[1]["bar"]


def test_gain_one_is_the_recorded_weights():
    """At gain 1 the builder returns the recorded configuration's state dict unchanged; a gain touches q and k rows only."""
    a, b, g = FX.state_dict("bp"), TC.state_dict(TC.BP_GAIN1), TC.state_dict(TC.TABLE[1])
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    for k in a:
        if k.endswith(".in_proj_weight"):
            assert torch.equal(g[k][:128], a[k][:128] * 4.0) and torch.equal(g[k][128:], a[k][128:])
        else:
            assert torch.equal(g[k], a[k]), k


@pytest.mark.parametrize("c", GATED, ids=GATED_IDS)
def test_case_is_well_conditioned(c):
    """Conditioning gate, a condition on the INPUTS (the rule of test_fixture_is_its_own_witness): the fp32 restatement is within
    a quarter of the bar of the fp64 one for memory, teacher-forced prediction and generation.  A case that fails is replaced
    (seed, gain, T); the bar is not moved."""
    for name, a, b in zip(("memory", "pred", "gen"), _restated(c, torch.float32), _restated(c, torch.float64)):
        dev, bar = float((a.double() - b).abs().max()), TC.bar(b)
        print(f"{TC.case_id(c)} {name}: fp32 vs fp64 {dev / bar:.3f} of the bar, max|out| {float(b.abs().max()):.3f}")
        assert bool(torch.isfinite(b).all()) and dev <= bar / 4, (name, dev, bar)


@pytest.mark.parametrize("c", GATED, ids=GATED_IDS)
def test_case_stresses_the_softmax(c):
    """Stress gate, from encoder layer 0's logits: at gain 4 the per-row logit spread has median >= 8 and, for T > 64, at least
    a quarter of the rows see the running maximum over 64-key chunks rise by more than 1 after the first chunk (the mirror's
    T = 65 case is exempt from the second: its last chunk holds one key).  The recorded `bp` weights at gain 1 fail both --
    the reason the table exists."""
    spread, rising = TC.stress(c)
    print(f"{TC.case_id(c)}: logit spread median {spread:.2f}, rows with a rising maximum {rising:.3f}")
    if c.gain == 1.0:
        assert c == TC.BP_GAIN1 and spread < TC.MIN_SPREAD and rising < TC.MIN_RISING, (spread, rising)
        return
    assert spread >= TC.MIN_SPREAD, spread
    if c.T > 64 and c != TC.MIRROR:
        assert rising >= TC.MIN_RISING, rising


@pytest.mark.parametrize("c", GATED, ids=GATED_IDS)
def test_cached_generation_is_the_causal_pass(c):
    """generate (explicit cache, one row a step) equals decode fed generate's output (all rows at once).  In fp64 the two differ
    by summation order alone: 1e-9 is five orders above 2^-53 times the amplification the conditioning gate allows fp32
    (2^-24 -> a quarter of the bar) and four below the bar.  In fp32, the bar."""
    for dtype, bound in ((torch.float64, 1e-9), (torch.float32, None)):
        memory, _, gen = _restated(c, dtype)
        again = R.decode(TC.state_dict_as(c, dtype), memory, gen, c.heads)
        err = float((again - gen).abs().max())
        assert err <= (TC.bar(gen) if bound is None else bound), (dtype, err)
