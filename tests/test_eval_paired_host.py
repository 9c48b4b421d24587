"""CPU pins of tests/_eval_paired_ref.py, the per-sample fp64 restatements that tests/test_eval_paired.py judges the paired
evaluation kernels (t2s_eval_mse_wape / _ed / _crps / _dtw / _mrr) by: their means against the oracle's eval_* functions on
small multichannel cases, against tests/golden/metrics.npz (the reference's own functions on (9, 24, 1) arrays) with the
tolerances tests/test_reference_fixtures_r2.py applies to the oracle, and against the multichannel fixture
tests/golden/metrics_mc.npz (tests/golden/gen_golden_metrics_mc.py).  DTW is UNPINNED (dtaidistance is third party and
absent): the anti-diagonal walk is held to the oracle's double loop and to known answers.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _eval_paired_ref as R
from oracle import t2s_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_metrics_mc", os.path.join(REPO, "tests", "golden", "gen_golden_metrics_mc.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


# CRPS in the kernel's documented arithmetic (statistics rounded once from fp64, z and Phi in fp64) against the reference's,
# which takes mean / std with numpy's pairwise fp32 sums and hands fp32 arrays to scipy's norm.cdf, so its z is fp32 too.
#   statistics: fp32 pairwise sums of L <= 130 values err by about (log2(L) + 2) u <= 9 u, u = 2^-24, relative to mean |g|
#     resp. to the std; |d crps / d mean| <= 2 * 0.399 / std and |d crps / d std| <= 2 max |z| phi(z) / std = 0.484 / std, so
#     with mean |g| <= 4 std in the series drawn here |delta crps| <= (0.8 * 4 + 0.484) * 9 u = 2e-6;
#   z in fp32: |delta z| <= 2 u |z|, |delta Phi| <= 2 u max |z| phi(z) = 2.9e-8, |delta crps| <= 5.8e-8.
# Against values of 0.05 and more that is 4e-5 relative at the very worst.  Asserted is the tighter 1e-5 that the suite's
# kernel-against-reference test (tests/test_hip_parity.py) already holds CRPS to; metrics.npz keeps the oracle's 1e-9.
CRPS_REFERENCE_RTOL = 1e-5


def _case(seed, n, L, S, runs):
    rs = np.random.RandomState(seed)
    scale = 1.0 + np.arange(n)[:, None, None] + 0.3 * np.arange(S)[None, None, :]
    ori = (scale * rs.uniform(-1, 1, (n, L, S))).astype(np.float32)
    gen = (ori + 0.3 * scale * rs.randn(n, L, S)).astype(np.float32)
    stack = np.stack([(ori * rs.uniform(0.3, 1.0) + 0.4 * (g + 1) * scale * rs.randn(n, L, S)).astype(np.float32)
                      for g in range(runs)], axis=-1)
    return ori, gen, stack


@pytest.fixture(scope="module")
def mc(golden_dir):
    z = np.load(os.path.join(golden_dir, "metrics_mc.npz"))
    return [{k: z[f"{k}_{i}"] for k in ("ori", "gen", "runs", "sims", "mse", "wape", "ed", "crps", "mrr")} for i in range(len(G.CASES))]


@pytest.mark.parametrize("shape", [(5, 24, 1, 4), (4, 33, 3, 3), (3, 48, 7, 2), (2, 70, 10, 5)])
def test_means_equal_the_oracle(shape):
    n, L, S, runs = shape
    ori, gen, stack = _case(11 + L, n, L, S, runs)
    ori[1] = 0.0                                        # WAPE NaN (skipped), every similarity 0
    stack[0, :, :, 1] = stack[0, :, :, runs - 1] = 2.0 * ori[0]     # an exact tie at similarity 1: the later run wins
    mse_i, wape_i = R.mse_wape(ori, gen)
    np.testing.assert_allclose(mse_i.mean(), O.eval_mse(ori, gen), rtol=1e-12)
    np.testing.assert_allclose(R.nanmean(wape_i), O.eval_wape(ori, gen), rtol=1e-12)
    assert np.isnan(wape_i[1]) and not np.isnan(np.delete(wape_i, 1)).any()
    np.testing.assert_allclose(R.ed(ori, gen).mean(), O.eval_ed(ori, gen), rtol=1e-6)      # the oracle's norm runs in fp32
    np.testing.assert_allclose(R.crps(ori, stack).mean(), O.eval_crps(ori, stack), rtol=CRPS_REFERENCE_RTOL)
    sims, score = R.mrr(ori, stack, 0.5)
    want = np.array([[O.eval_cosine(ori[i], stack[i, :, :, g]) for g in range(runs)] for i in range(n)])
    np.testing.assert_allclose(sims, want, rtol=1e-12, atol=1e-15)
    for thr in (0.5, 0.0, -1.0):
        assert abs(R.mrr(ori, stack, thr)[1].mean() - O.eval_mrr(ori, stack, thr)) < 1e-7      # 1 / (g + 1) is rounded to fp32
    assert score[0] == np.float32(1) / np.float32(runs) and score[1] == 0
    if L <= 48:
        np.testing.assert_allclose(R.dtw(ori, gen).mean(), O.eval_dtw(ori, gen), rtol=1e-12)


def test_dtw_walk_equals_the_double_loop_per_sample():
    rs = np.random.RandomState(3)
    for L, S in ((1, 1), (2, 3), (7, 1), (40, 3), (48, 2)):
        a = rs.uniform(0, 1, (4, L, S)).astype(np.float32)
        b = (a + 0.3 * rs.randn(4, L, S)).astype(np.float32)
        got = R.dtw(a, b)
        want = np.array([O.eval_dtw(a[i:i + 1], b[i:i + 1]) for i in range(4)])
        np.testing.assert_allclose(got, want, rtol=1e-13)


def test_dtw_known_answers_beyond_one_pass_of_the_diagonal():
    L, S, k, c = 300, 3, 37, 0.375
    rs = np.random.RandomState(4)
    a = rs.uniform(0, 1, (2, L, S)).astype(np.float32)
    assert (R.dtw(a, a) == 0).all()
    s1, s2 = np.zeros((1, L, 1), np.float32), np.zeros((1, L, 1), np.float32)
    s1[0, 140:] = 1.0
    s2[0, 140 + k:] = 1.0
    assert R.dtw(s1, s2)[0] == 0.0
    flat = np.full((1, L, S), 0.25, np.float32)
    np.testing.assert_allclose(R.dtw(flat, flat + np.float32(c))[0], c * np.sqrt(S * L), rtol=1e-14)


def test_reference_fixture_single_channel(golden_dir):
    """metrics.npz, with the tolerances test_metric_restatements_equal_reference applies to the oracle."""
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    ori, gen, runs = g["ori"], g["gen"], g["runs"]
    mse_i, wape_i = R.mse_wape(ori, gen)
    sims, score = R.mrr(ori, runs, 0.5)
    crps = R.crps(ori, runs).mean()
    print("mse", mse_i.mean() / float(g["mse"]) - 1, "wape", R.nanmean(wape_i) / float(g["wape"]) - 1,
          "ed", R.ed(ori, gen).mean() / float(g["ed"]) - 1, "crps", crps / float(g["crps"]) - 1)
    np.testing.assert_allclose(mse_i.mean(), float(g["mse"]), rtol=1e-6)
    np.testing.assert_allclose(R.nanmean(wape_i), float(g["wape"]), rtol=1e-6)
    assert abs(score.mean() - float(g["mrr"])) < 1e-12
    np.testing.assert_allclose(crps, float(g["crps"]), rtol=1e-9)
    np.testing.assert_allclose(R.ed(ori, gen).mean(), float(g["ed"]), rtol=1e-6)
    np.testing.assert_allclose(sims, g["sims"], rtol=1e-6, atol=1e-7)
    assert np.all(sims[4] == 0) and np.all(sims[2, :6] < 0) and abs(sims[6, 7] - 1) < 1e-6


def test_reference_fixture_multichannel(mc):
    """metrics_mc.npz: 7 and 10 channels, L = 70 and 130, 10 and 3 runs, by the same tolerances (CRPS: see CRPS_REFERENCE_RTOL)."""
    for k, c in enumerate(mc):
        n, L, S, runs = G.CASES[k]
        assert c["ori"].shape == (n, L, S) and c["runs"].shape == (n, L, S, runs) and c["ori"].dtype == np.float32
        mse_i, wape_i = R.mse_wape(c["ori"], c["gen"])
        sims, score = R.mrr(c["ori"], c["runs"], G.THRESHOLD)
        crps = R.crps(c["ori"], c["runs"])
        print(k, "mse", mse_i.mean() / float(c["mse"]) - 1, "wape", R.nanmean(wape_i) / float(c["wape"]) - 1,
              "ed", R.ed(c["ori"], c["gen"]).mean() / float(c["ed"]) - 1, "crps", crps.mean() / float(c["crps"]) - 1)
        np.testing.assert_allclose(mse_i.mean(), float(c["mse"]), rtol=1e-6)
        np.testing.assert_allclose(R.nanmean(wape_i), float(c["wape"]), rtol=1e-6)
        np.testing.assert_allclose(R.ed(c["ori"], c["gen"]).mean(), float(c["ed"]), rtol=1e-6)
        np.testing.assert_allclose(crps.mean(), float(c["crps"]), rtol=CRPS_REFERENCE_RTOL)
        assert abs(score.mean() - float(c["mrr"])) < 1e-7
        np.testing.assert_allclose(sims, c["sims"], rtol=1e-6, atol=1e-7)
        # the rows with a purpose
        assert np.isnan(wape_i[G.ROWS["zero"]]) and np.all(sims[G.ROWS["zero"]] == 0) and score[G.ROWS["zero"]] == 0
        assert np.all(sims[G.ROWS["negated"]] < 0) and score[G.ROWS["negated"]] == 0
        assert score[G.ROWS["copy"]] == np.float32(1) / np.float32(G.COPY_RUN[runs] + 1)
        const = c["runs"][G.ROWS["constant"], :, G.CONST_SERIES, G.CONST_RUN]
        obs = c["ori"][G.ROWS["constant"], :, G.CONST_SERIES]
        assert (const == 0.5).all() and (obs > 0.5).any() and (obs < 0.5).any() and (obs == 0.5).any()
        # with std = 1e-8 Phi is 0, 1/2 or 1: that series and run contribute exactly 1/4 per observation ON the constant
        one = R.crps(c["ori"][:1, :, G.CONST_SERIES:G.CONST_SERIES + 1], c["runs"][:1, :, G.CONST_SERIES:G.CONST_SERIES + 1, G.CONST_RUN:G.CONST_RUN + 1])
        assert one[0] == 0.25 * (obs == 0.5).sum() / L


def test_fixture_arrays_are_the_generators(mc):
    for k, (n, L, S, runs) in enumerate(G.CASES):
        ori, gen, stack = G.make_case(n, L, S, runs, 5200 + k)
        assert np.array_equal(ori, mc[k]["ori"]) and np.array_equal(gen, mc[k]["gen"]) and np.array_equal(stack, mc[k]["runs"])
    assert max(g for _, _, _, g in G.CASES) <= 16
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "metrics_mc.npz")) < 100 * 1024


# ---------------------------------------------------------------------- what a NaN or an Inf does (include/t2s.h states it)
def test_non_finite_inputs_in_the_restatements():
    ori, gen, stack = _case(5, 4, 20, 2, 3)
    for bad in (np.nan, np.inf):
        g = gen.copy()
        g[2, 7, 1] = bad
        mse_i, wape_i = R.mse_wape(ori, g)
        want = np.isnan if np.isnan(bad) else np.isposinf
        assert want(mse_i[2]) and want(wape_i[2]) and np.isfinite(np.delete(mse_i, 2)).all()
        assert want(R.ed(ori, g)[2]) and np.isfinite(np.delete(R.ed(ori, g), 2)).all()
        assert want(R.dtw(ori, g)[2]) and np.isfinite(np.delete(R.dtw(ori, g), 2)).all()
        st = stack.copy()
        st[2, 7, 1, 0] = bad
        assert np.isnan(R.crps(ori, st)[2]) and np.isfinite(np.delete(R.crps(ori, st), 2)).all()
        sims, _ = R.mrr(ori, st)
        assert sims[2, 0] == 0 and (sims[2, 1:] != 0).all()
    o = ori.copy()
    o[2, 7, 1] = np.inf                                 # Inf in the original: |d| and |ori| are both Inf, their ratio is NaN
    mse_i, wape_i = R.mse_wape(o, gen)
    assert np.isposinf(mse_i[2]) and np.isnan(wape_i[2]) and np.isposinf(R.ed(o, gen)[2]) and np.isposinf(R.dtw(o, gen)[2])
    assert np.isfinite(R.crps(o, stack)).all()          # Phi(+Inf) = 1 = the step: that observation contributes 0
    assert (R.mrr(o, stack)[0][2] == 0).all() and R.mrr(o, stack, -1.0)[1][2] == np.float32(1) / np.float32(3)
    o[2, 7, 1] = np.nan
    assert np.isnan(R.crps(o, stack)[2]) and np.isnan(R.dtw(o, gen)[2]) and np.isnan(R.mse_wape(o, gen)[1][2])


def test_header_states_the_non_finite_rule_next_to_each_entry():
    txt = open(os.path.join(REPO, "include", "t2s.h")).read()
    for name in ("t2s_eval_mse_wape", "t2s_eval_mrr", "t2s_eval_ed", "t2s_eval_crps", "t2s_eval_dtw"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", txt, flags=re.S)
        assert m and "NaN" in m.group(1) and "Inf" in m.group(1), name
