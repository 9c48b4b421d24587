"""The paired evaluation kernels t2s_eval_mse_wape / _ed / _crps / _dtw / _mrr (csrc/t2s_eval.hip, mirrored in
t2ms_amd.metrics) against the per-sample fp64 restatements of tests/_eval_paired_ref.py, which tests/test_eval_paired_host.py
pins on the CPU: every per_sample / sims / score element and the mean, at the layout, stride, sample-count and LDS edges of
the kernels.  Needs a real MI355X (`pytest -m gpu`).

Tolerances (u = 2^-24, the unit roundoff of fp32; errors are relative, an expected exact 0 must come out as exact 0).
  ED, CRPS, DTW, the MRR similarities: fp64 accumulation, one rounding to fp32 -> 2 u = 2^-23 (one rounding plus one u of slack
    for the device's sqrt / erfc and another fp64 summation order).
  MSE: eval_per_sample_kernel runs in fp32.  With m = ceil(len / 64) terms per lane: d = a - b carries 1 u, so d * d carries
    3 u with the product's rounding; a lane adds m non-negative terms in m - 1 rounded additions (errors of non-negative
    sums do not amplify: each addition adds at most 1 u to the relative error); six shuffle additions; the division by len
    (exact in fp32): 3 + (m - 1) + 6 + 1 = (m + 9) u.
  WAPE: the numerator sum |d| carries 1 + (m - 1) + 6 = (m + 6) u, the denominator sum |a| (m - 1) + 6 = (m + 5) u, their
    quotient one more: (2 m + 12) u.
  Both with the usual k u / (1 - k u) for the higher orders.  The means are fp64 sums of the fp32 per-sample values rounded
  once: the per-sample bound plus 1 u (all terms are non-negative).  Scores are exact: 1 / (g + 1) in fp32, or 0.
The measured worst errors are in profiles/eval_paired_errors.md; every check prints its own as an `EVALERR` line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _eval_paired_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 64
ENTRIES = ("t2s_eval_mse_wape", "t2s_eval_mrr", "t2s_eval_ed", "t2s_eval_crps", "t2s_eval_dtw")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------------- helpers
def gamma(k):
    """k roundings, in units of u, higher orders included."""
    return k / (1.0 - k * R.U)


def mse_bound(length):
    return gamma(-(-length // 64) + 9)


def wape_bound(length):
    return gamma(2 * -(-length // 64) + 12)


def worst(got, want):
    """Largest relative error of got (fp32) against want (fp64) in units of u; NaN / Inf / exact 0 must agree exactly."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[special], want[special], equal_nan=True), (got[special], want[special])
    if special.all():
        return 0.0
    g, w = got[~special], want[~special]
    return float(np.max(np.abs(g - w) / np.abs(w)) / R.U)


def check(entry, what, shape, got, want, bound):
    err = worst(got, want)
    print(f"EVALERR {entry} {what} shape={shape} worst={err:.3f}u bound={bound:.3f}u")
    assert err <= bound, (entry, what, shape, err, bound)


def draw(seed, n, length, S, runs=0):
    """ori, gen (n, L, S) and `runs` stacked generations (n, L, S, runs).  Series j of sample i is scaled by (1 + 0.7 i)
    (1 + 0.45 j), run k's noise by 0.4 (k + 1): a value read at a wrong offset is off by far more than any tolerance."""
    rs = np.random.RandomState(seed)
    f = (1.0 + 0.7 * np.arange(n))[:, None, None] * (1.0 + 0.45 * np.arange(S))[None, None, :]
    ori = (f * rs.uniform(0.1, 1.0, (n, length, S))).astype(np.float32)
    gen = (ori + 0.25 * f * rs.randn(n, length, S)).astype(np.float32)
    stack = np.stack([(ori + 0.4 * (k + 1) * f * rs.randn(n, length, S)).astype(np.float32) for k in range(runs)], axis=-1) if runs else None
    return ori, gen, stack


def check_mse_wape(ori, gen, dev, what="layout"):
    mse, wape, per = M.mse_wape(ori, gen, dev)
    want_m, want_w = R.mse_wape(ori, gen)
    shape, length = ori.shape, int(np.prod(ori.shape[1:]))
    assert per.shape == (ori.shape[0], 2)
    check("mse", what, shape, per[:, 0].numpy(), want_m, mse_bound(length))
    check("wape", what, shape, per[:, 1].numpy(), want_w, wape_bound(length))
    check("mse", what + " mean", shape, [mse], [want_m.mean()], mse_bound(length) + 1)
    check("wape", what + " mean", shape, [wape], [R.nanmean(want_w)], wape_bound(length) + 1)
    return per


def check_simple(name, fn, ref, ori, other, dev, what="layout"):
    """ED / DTW (other = gen) and CRPS (other = the stacked runs): per sample and the mean at 2 u resp. 3 u."""
    value, per = fn(ori, other, dev)
    want = ref(ori, other)
    assert per.shape == (ori.shape[0],)
    check(name, what, np.shape(other), per.numpy(), want, 2)
    check(name, what + " mean", np.shape(other), [value], [want.mean()], 3)
    return per


def raw(dev, entry, ori, gen, dims, extra=(), out_floats=1, per_floats=None):
    """One call of a C entry on guarded outputs: `per` and `out` sit in one buffer filled with SENTINEL, with GUARD floats
    after each; -> (rc, message, per, out, guards untouched)."""
    n = dims[0]
    per_floats = n if per_floats is None else per_floats
    buf = torch.full((per_floats + GUARD + out_floats + GUARD,), SENTINEL, device=dev)
    per, out = buf[:per_floats], buf[per_floats + GUARD:per_floats + GUARD + out_floats]
    a = None if ori is None else torch.from_numpy(np.ascontiguousarray(ori)).to(dev)
    g = None if gen is None else torch.from_numpy(np.ascontiguousarray(gen)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = getattr(L.lib(), entry)(ptr(a), ptr(g), *extra, per.data_ptr(), out.data_ptr(), *dims, L.stream_ptr(dev))
    torch.cuda.synchronize()
    msg = L.lib().t2s_last_error().decode() if rc != 0 else ""
    host = buf.cpu()
    guards = bool((host[per_floats:per_floats + GUARD] == SENTINEL).all() and (host[per_floats + GUARD + out_floats:] == SENTINEL).all())
    return rc, msg, host[:per_floats].clone(), host[per_floats + GUARD:per_floats + GUARD + out_floats].clone(), guards


# ------------------------------------------------------------------------------------------- layout and stride edges
LAYOUTS = [(5, 63, 1), (5, 64, 7), (4, 65, 10), (3, 130, 3)]


@pytest.mark.parametrize("shape", LAYOUTS)
def test_ed_mse_wape_layout_and_stride_edges(dev, shape):
    """One wave per sample strides time by 64: L = 63 / 64 / 65 / 130 end the stride loop inside, on and just after a pass;
    n_series 7 and 10 exercise t * S + j (ED) and len = L * S not a multiple of 64 (MSE / WAPE)."""
    ori, gen, _ = draw(100 + shape[1], *shape)
    check_simple("ed", M.ed, R.ed, ori, gen, dev)
    check_mse_wape(ori, gen, dev)


@pytest.mark.parametrize("runs", [1, 3])
@pytest.mark.parametrize("shape", LAYOUTS)
def test_crps_layout_and_stride_edges(dev, shape, runs):
    """The run-major offset (k * n + i) * L * S with n_series > 1 and runs > 1; the generations given as a list of runs and
    as the stacked trailing-axis array must give the same bits."""
    ori, _, stack = draw(200 + shape[1], *shape, runs=runs)
    per = check_simple("crps", M.crps, R.crps, ori, stack, dev)
    value_l, per_l = M.crps(ori, [stack[..., k] for k in range(runs)], dev)
    assert torch.equal(per, per_l) and value_l == M.crps(ori, stack, dev)[0]


def test_crps_constant_and_tiny_std(dev):
    """A generated series that is exactly constant (std 0 -> 1e-8f: Phi is 0, 1/2 or 1) with the observations above, below
    and exactly on it, at a value whose sums are exact (0.5) and at one where only the fp64 sums are (0.3f); a generated
    series whose std is tiny but not 0; a run axis of length 1."""
    n, length, S = 3, 70, 2
    ori, _, stack = draw(31, n, length, S, runs=1)
    pattern = np.arange(length) % 3                       # 0: on it, 1: above, 2: below
    for i, c in enumerate((np.float32(0.5), np.float32(0.3))):
        stack[i, :, 1, 0] = c
        ori[i, :, 1] = np.where(pattern == 0, c, np.where(pattern == 1, c * np.float32(1.5), c * np.float32(0.5)))
    rs = np.random.RandomState(32)
    stack[2, :, 0, 0] = (1e-3 + 1e-6 * rs.randn(length)).astype(np.float32)        # std ~ 1e-6: z = O(1) in fp64 only
    ori[2, :, 0] = (1e-3 + 1e-6 * rs.randn(length)).astype(np.float32)
    assert 0 < stack[2, :, 0, 0].astype(np.float64).std() < 2e-6
    check_simple("crps", M.crps, R.crps, ori, stack, dev, what="constant / tiny std")
    # the constant series alone: exactly 1/4 per observation that lies on the constant
    for i in range(2):
        value, per = M.crps(ori[i:i + 1, :, 1:2], stack[i:i + 1, :, 1:2], dev)
        want = np.float32(0.25 * (pattern == 0).sum() / length)
        assert per[0].item() == want and np.float32(value) == want


def test_mse_wape_zero_rows(dev):
    """An all-zero original row: its WAPE is NaN and the mean skips it; every row all-zero: WAPE itself is NaN.  len = 3 * 23
    = 69 is not a multiple of 64."""
    ori, gen, _ = draw(41, 6, 23, 3)
    ori[2] = 0.0
    per = check_mse_wape(ori, gen, dev, what="zero row")
    assert np.isnan(per[2, 1].item()) and not torch.isnan(per[:, 0]).any() and int(torch.isnan(per[:, 1]).sum()) == 1
    mse, wape, per = M.mse_wape(np.zeros_like(ori), gen, dev)
    assert np.isnan(wape) and bool(torch.isnan(per[:, 1]).all())
    check("mse", "all rows zero", ori.shape, per[:, 0].numpy(), R.mse_wape(np.zeros_like(ori), gen)[0], mse_bound(69))
    check("mse", "all rows zero mean", ori.shape, [mse], [R.mse_wape(np.zeros_like(ori), gen)[0].mean()], mse_bound(69) + 1)


# ------------------------------------------------------------------------------------------------------- sample count
@pytest.fixture(scope="module")
def many():
    """300 samples of 8 steps x 2 series with 2 runs, and their restatements: the n of the cases below are its first rows."""
    ori, gen, stack = draw(51, 300, 8, 2, runs=2)
    ori[7] = 0.0
    ref = {"mse_wape": R.mse_wape(ori, gen), "ed": R.ed(ori, gen), "crps": R.crps(ori, stack), "dtw": R.dtw(ori, gen),
           "mrr": R.mrr(ori, stack, 0.5)}
    return ori, gen, stack, ref


@pytest.mark.parametrize("n", [1, 256, 257, 300])
def test_sample_count_takes_the_reductions_through_a_second_pass(dev, many, n):
    """eval_mean_kernel / eval_reduce_kernel: 256 threads stride the samples; n = 256 is the last single pass, 257 and 300
    the first with a second one (a thread adding two samples; the NaN-skipping count of WAPE included)."""
    ori, gen, stack, ref = many
    o, g, s = ori[:n], gen[:n], stack[:n]
    shape = o.shape
    mse, wape, per = M.mse_wape(o, g, dev)
    check("mse", "n", shape, per[:, 0].numpy(), ref["mse_wape"][0][:n], mse_bound(16))
    check("wape", "n", shape, per[:, 1].numpy(), ref["mse_wape"][1][:n], wape_bound(16))
    check("mse", "n mean", shape, [mse], [ref["mse_wape"][0][:n].mean()], mse_bound(16) + 1)
    check("wape", "n mean", shape, [wape], [R.nanmean(ref["mse_wape"][1][:n])], wape_bound(16) + 1)
    for name, fn, other in (("ed", M.ed, g), ("crps", M.crps, s), ("dtw", M.dtw, g)):
        value, per = fn(o, other, dev)
        assert per.shape == (n,)
        check(name, "n", shape, per.numpy(), ref[name][:n], 2)
        check(name, "n mean", shape, [value], [ref[name][:n].mean()], 3)
    m, sims, score = M.mrr(o, s, 0.5, dev)
    check("mrr", "n sims", s.shape, sims.numpy(), ref["mrr"][0][:n], 2)
    assert np.array_equal(score.numpy(), ref["mrr"][1][:n].astype(np.float32))
    check("mrr", "n mean", s.shape, [m], [ref["mrr"][1][:n].mean()], 1)


# ------------------------------------------------------------------------------------------------------------------ DTW
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("length", [1, 2, 255, 256, 257, 600])
def test_dtw_diagonal_passes_and_corners(dev, length, S):
    """256 threads stride a diagonal: L = 255 / 256 / 257 / 600 end the loop `i += 256` inside, on, just after a pass and in
    the third; beyond 256 the diagonals are clamped (`lo`, `hi`) at both corners of the table; L = 1 and 2 are the table's
    degenerate ends."""
    ori, gen, _ = draw(300 + length, 2, length, S)
    check_simple("dtw", M.dtw, R.dtw, ori, gen, dev)


def test_dtw_known_answers_beyond_one_pass(dev):
    length, S, k, c = 300, 3, 37, 0.375
    a = draw(61, 2, length, S)[0]
    value, per = M.dtw(a, a, dev)
    assert value == 0.0 and (per == 0).all()                                   # identical sequences
    s1, s2 = np.zeros((1, length, 1), np.float32), np.zeros((1, length, 1), np.float32)
    s1[0, 140:] = 1.0
    s2[0, 140 + k:] = 1.0
    assert M.dtw(s1, s2, dev)[0] == 0.0                                        # a step moved by k positions warps away
    flat = np.full((2, length, S), 0.25, np.float32)
    value, per = M.dtw(flat, flat + np.float32(c), dev)                        # a constant offset on S series
    check("dtw", "constant offset", flat.shape, per.numpy(), np.full(2, c * np.sqrt(S * length)), 2)


def test_dtw_lds_cap_boundary_and_longest_series(dev):
    """3 * L * 8 bytes of dynamic LDS: L = 2048 is exactly 48 KiB (the cap is not raised), L = 2049 the first that raises
    it, L = 4096 the contract's bound (96 KiB); a small launch afterwards is not disturbed by the raised cap.  In this
    order: the cap stays raised for the rest of the process."""
    for n, length, S in ((1, 2048, 1), (1, 2049, 1), (1, 4096, 2), (2, 24, 2)):
        ori, gen, _ = draw(400 + length, n, length, S)
        check_simple("dtw", M.dtw, R.dtw, ori, gen, dev, what="lds cap")


def test_dtw_refuses_4097_before_any_launch(dev):
    z = np.zeros((1, 4097, 1), np.float32)
    rc, msg, per, out, guards = raw(dev, "t2s_eval_dtw", z, z, (1, 4097, 1))
    assert rc == -1 and "t2s_eval_dtw" in msg and "4096" in msg and "4097" in msg, (rc, msg)
    assert guards and (per == SENTINEL).all() and (out == SENTINEL).all()
    with pytest.raises(L.T2SError, match="4096"):
        M.dtw(z, z, dev)


# ------------------------------------------------------------------------------------------------------------------ MRR
def mrr_case():
    n, length, S, runs = 12, 33, 3, 10
    rs = np.random.RandomState(9)
    ori = rs.uniform(-1, 1, (n, length, S)).astype(np.float32) * (1.0 + 0.45 * np.arange(S, dtype=np.float32))
    gens = [(ori * rs.uniform(0.2, 1.0, (n, 1, 1)) + rs.uniform(0.1, 1.5) * rs.randn(n, length, S)).astype(np.float32) for _ in range(runs)]
    for g in gens:
        g[3] = rs.randn(length, S)               # unrelated: every similarity below 0.5
    gens[2][7] = gens[6][7] = 2.0 * ori[7]       # an exact tie at similarity 1: run 6 wins
    ori[11] = 0.0                                # every similarity 0
    return ori, np.stack(gens, axis=-1)


@pytest.mark.parametrize("threshold", [0.5, 0.0, -1.0])
def test_mrr_multichannel_sims_scores_and_thresholds(dev, threshold):
    ori, stack = mrr_case()
    m, sims, score = M.mrr(ori, stack, threshold, dev)
    want_sims, want_score = R.mrr(ori, stack, threshold)
    check("mrr", f"sims thr={threshold}", stack.shape, sims.numpy(), want_sims, 2)
    assert np.array_equal(score.numpy(), want_score.astype(np.float32))          # exact: 1 / (g + 1) in fp32, or 0
    check("mrr", f"mean thr={threshold}", stack.shape, [m], [want_score.mean()], 1)
    assert (sims[11] == 0).all() and sims[7, 2] == sims[7, 6] and score[7] == np.float32(1) / np.float32(7)
    assert score[11] == (np.float32(0.1) if threshold < 0 else 0)               # all similarities 0: the last run, if 0 passes
    assert (score[3] == 0) == (threshold == 0.5)
    m_list, sims_list, score_list = M.mrr(ori, [stack[..., g] for g in range(stack.shape[-1])], threshold, dev)
    assert m_list == m and torch.equal(sims_list, sims) and torch.equal(score_list, score)


def test_mrr_non_finite_generations_and_originals(dev):
    """include/t2s.h: a similarity that is not finite is stored as 0 and competes as 0 (the reference's nan_to_num).  An Inf
    in run 0 used to store NaN (inf / inf), which no later run could beat: the sample scored 0."""
    n, length, S, runs = 5, 20, 2, 4
    ori, _, stack = draw(71, n, length, S, runs=runs)
    near = (ori * np.float32(1.01)).astype(np.float32)
    stack[0, 3, 1, 0] = np.inf                   # +Inf in run 0, a near copy at run 2
    stack[0, :, :, 2] = near[0]
    stack[1, 3, 1, runs - 1] = np.inf            # the Inf run last, a near copy at run 1
    stack[1, :, :, 1] = near[1]
    stack[2, 5, 0, 0] = np.nan                   # a NaN in run 0, a near copy at run 3
    stack[2, :, :, 3] = near[2]
    stack[3, 4, 1, 1] = -np.inf                  # -Inf in run 1 (a near copy at run 0)
    stack[3, :, :, 0] = near[3]
    ori[4, 2, 0] = np.inf                        # an Inf in the original: every similarity 0
    for threshold in (0.5, -1.0):
        m, sims, score = M.mrr(ori, stack, threshold, dev)
        want_sims, want_score = R.mrr(ori, stack, threshold)
        assert bool(torch.isfinite(sims).all()) and bool(torch.isfinite(score).all()) and np.isfinite(m)
        check("mrr", f"non-finite sims thr={threshold}", stack.shape, sims.numpy(), want_sims, 2)
        assert np.array_equal(score.numpy(), want_score.astype(np.float32)), (score, want_score)
        assert sims[0, 0] == 0 and sims[1, runs - 1] == 0 and sims[2, 0] == 0 and sims[3, 1] == 0 and (sims[4] == 0).all()
        one = np.float32(1)
        assert score[0] == one / np.float32(3) and score[1] == one / np.float32(2) and score[2] == one / np.float32(4) and score[3] == 1
        assert score[4] == (one / np.float32(runs) if threshold < 0 else 0)
        check("mrr", f"non-finite mean thr={threshold}", stack.shape, [m], [want_score.mean()], 1)


# ------------------------------------------------------------------------------- non-finite inputs of the other entries
def test_non_finite_inputs_follow_the_header(dev):
    """include/t2s.h next to each entry: NaN / Inf are not filtered; the sample that holds one and the mean take what IEEE
    arithmetic gives (the restatement's value), the other samples are not touched."""
    ori, gen, stack = draw(81, 4, 70, 3, runs=2)
    clean = {"ed": M.ed(ori, gen, dev)[1], "dtw": M.dtw(ori, gen, dev)[1], "crps": M.crps(ori, stack, dev)[1],
             "mse_wape": M.mse_wape(ori, gen, dev)[2]}
    for where, bad in (("gen", np.nan), ("gen", np.inf), ("ori", np.inf), ("ori", np.nan)):
        o, g, s = ori.copy(), gen.copy(), stack.copy()
        if where == "gen":
            g[2, 66, 1] = bad
            s[2, 66, 1, 1] = bad
        else:
            o[2, 66, 1] = bad
        what = f"{bad} in {where}"
        keep = np.array([0, 1, 3])
        for name, fn, ref, other in (("ed", M.ed, R.ed, g), ("dtw", M.dtw, R.dtw, g), ("crps", M.crps, R.crps, s)):
            value, per = fn(o, other, dev)
            want = ref(o, other)
            check(name, what, o.shape, per.numpy(), want, 2)
            check(name, what + " mean", o.shape, [value], [want.mean()], 3)
            assert torch.equal(per[keep], clean[name][keep])
            if not (name == "crps" and where == "ori" and np.isinf(bad)):
                assert not np.isfinite(per[2].item()) and not np.isfinite(value), (name, what)
        mse, wape, per = M.mse_wape(o, g, dev)
        want_m, want_w = R.mse_wape(o, g)
        check("mse", what, o.shape, per[:, 0].numpy(), want_m, mse_bound(210))
        check("wape", what, o.shape, per[:, 1].numpy(), want_w, wape_bound(210))
        check("mse", what + " mean", o.shape, [mse], [want_m.mean()], mse_bound(210) + 1)
        check("wape", what + " mean", o.shape, [wape], [R.nanmean(want_w)], wape_bound(210) + 1)
        assert torch.equal(per[keep], clean["mse_wape"][keep]) and not np.isfinite(per[2, 0].item())


# ------------------------------------------------------------------------------------------------------------ properties
def test_rows_are_independent_repeatable_and_outputs_end_at_n(dev):
    """Row i of a batch equals row i evaluated alone, bit for bit; a second call gives the same bits; per_sample holds
    exactly n entries (2 n for MSE / WAPE, n * runs similarities): the floats after it and after `out` keep their sentinel."""
    n, length, S, runs = 5, 70, 3, 3
    ori, gen, stack = draw(91, n, length, S, runs=runs)
    run_major = np.ascontiguousarray(np.moveaxis(stack, -1, 0))
    flat = lambda x: x.reshape(x.shape[0], -1)

    def calls(o, g, rm, rows):
        sims = torch.full((rows * runs + GUARD,), SENTINEL, device=dev)
        res = {"t2s_eval_mse_wape": raw(dev, "t2s_eval_mse_wape", flat(o), flat(g), (rows, length * S), out_floats=2, per_floats=2 * rows),
               "t2s_eval_ed": raw(dev, "t2s_eval_ed", o, g, (rows, length, S)),
               "t2s_eval_dtw": raw(dev, "t2s_eval_dtw", o, g, (rows, length, S)),
               "t2s_eval_crps": raw(dev, "t2s_eval_crps", o, rm, (rows, length, S, runs)),
               "t2s_eval_mrr": raw(dev, "t2s_eval_mrr", flat(o), rm.reshape(runs, rows, -1), (rows, length * S, runs, C.c_float(0.5)),
                                   extra=(sims.data_ptr(),))}
        torch.cuda.synchronize()
        return res, sims.cpu()

    first, sims1 = calls(ori, gen, run_major, n)
    again, sims2 = calls(ori, gen, run_major, n)
    for entry in ENTRIES:
        rc, msg, per, out, guards = first[entry]
        assert rc == 0 and guards, (entry, msg)
        assert not (per == SENTINEL).any() and not (out == SENTINEL).any(), entry          # every slot was written
        assert torch.equal(per, again[entry][2]) and torch.equal(out, again[entry][3]), entry
    assert torch.equal(sims1, sims2) and (sims1[n * runs:] == SENTINEL).all() and not (sims1[:n * runs] == SENTINEL).any()
    for i in range(n):
        alone, sims_i = calls(ori[i:i + 1], gen[i:i + 1], run_major[:, i:i + 1], 1)
        for entry in ENTRIES:
            width = 2 if entry == "t2s_eval_mse_wape" else 1
            assert alone[entry][0] == 0 and alone[entry][4], entry
            assert torch.equal(alone[entry][2], first[entry][2][width * i:width * (i + 1)]), (entry, i)
        assert torch.equal(sims_i[:runs], sims1[i * runs:(i + 1) * runs]), i


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_back_as_error_codes_before_any_launch(dev):
    """n = 0, L = 0, n_series = 0, runs = 0 and a NULL array: T2S_E_INVALID with a message naming the entry; the checks run
    before any launch (csrc/t2s_eval.hip: T2S_REQUIRE heads every entry), so the outputs keep their sentinel."""
    x = draw(95, 2, 8, 2)[0]
    rm = np.stack([x, x])
    flat = x.reshape(2, -1)
    sims = torch.full((8,), SENTINEL, device=dev)
    cases = []
    for dims in ((0, 16), (2, 0)):
        cases.append(("t2s_eval_mse_wape", flat, flat, dims, ()))
    for dims in ((0, 8, 2), (2, 0, 2), (2, 8, 0)):
        cases.append(("t2s_eval_ed", x, x, dims, ()))
        cases.append(("t2s_eval_dtw", x, x, dims, ()))
    for dims in ((0, 8, 2, 2), (2, 0, 2, 2), (2, 8, 0, 2), (2, 8, 2, 0)):
        cases.append(("t2s_eval_crps", x, rm, dims, ()))
    for dims in ((0, 16, 2), (2, 0, 2), (2, 16, 0)):
        cases.append(("t2s_eval_mrr", flat, rm.reshape(2, 2, -1), dims + (C.c_float(0.5),), (sims.data_ptr(),)))
    good = {"t2s_eval_mse_wape": (flat, flat, (2, 16), ()), "t2s_eval_ed": (x, x, (2, 8, 2), ()), "t2s_eval_dtw": (x, x, (2, 8, 2), ()),
            "t2s_eval_crps": (x, rm, (2, 8, 2, 2), ()), "t2s_eval_mrr": (flat, rm.reshape(2, 2, -1), (2, 16, 2, C.c_float(0.5)), (sims.data_ptr(),))}
    for entry, (a, g, dims, extra) in good.items():
        cases.append((entry, None, g, dims, extra))
        cases.append((entry, a, None, dims, extra))
    cases.append(("t2s_eval_mrr", flat, rm.reshape(2, 2, -1), (2, 16, 2, C.c_float(0.5)), (None,)))
    for entry, a, g, dims, extra in cases:
        rc, msg, per, out, guards = raw(dev, entry, a, g, dims, extra=extra, out_floats=2, per_floats=4)
        assert rc == -1 and msg.startswith(entry + ":"), (entry, dims, rc, msg)
        assert guards and (per == SENTINEL).all() and (out == SENTINEL).all(), (entry, dims)
    assert (sims.cpu() == SENTINEL).all()
    # NULL outputs
    a = torch.from_numpy(x).to(dev)
    out = torch.full((2,), SENTINEL, device=dev)
    lib, st = L.lib(), L.stream_ptr(dev)
    assert lib.t2s_eval_ed(a.data_ptr(), a.data_ptr(), None, out.data_ptr(), 2, 8, 2, st) == -1
    assert lib.t2s_eval_dtw(a.data_ptr(), a.data_ptr(), out.data_ptr(), None, 2, 8, 2, st) == -1
    assert lib.t2s_eval_mse_wape(a.data_ptr(), a.data_ptr(), None, out.data_ptr(), 2, 16, st) == -1
    assert lib.t2s_eval_crps(a.data_ptr(), a.data_ptr(), None, out.data_ptr(), 2, 8, 2, 1, st) == -1
    assert lib.t2s_eval_mrr(a.data_ptr(), a.data_ptr(), out.data_ptr(), None, out.data_ptr(), 2, 16, 1, 0.5, st) == -1
    assert "t2s_eval_mrr" in lib.t2s_last_error().decode()
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all()
    # the entries still work
    assert M.ed(x, x, dev)[0] == 0.0


# ----------------------------------------------------------------------------------------------------- reference fixture
def test_multichannel_reference_fixture(dev, golden_dir):
    """tests/golden/metrics_mc.npz (the reference's calculate_mse / _wape / _ed / _crps / _mrr and cosine_similarity on 7- and
    10-channel series) with the tolerances of test_eval_ed_crps_mse_wape_mrr_reference_fixture."""
    z = np.load(os.path.join(golden_dir, "metrics_mc.npz"))
    for k in range(2):
        ori, gen, runs = z[f"ori_{k}"], z[f"gen_{k}"], z[f"runs_{k}"]
        mse, wape, _ = M.mse_wape(ori, gen, dev)
        np.testing.assert_allclose(mse, float(z[f"mse_{k}"]), rtol=2e-6)
        np.testing.assert_allclose(wape, float(z[f"wape_{k}"]), rtol=2e-6)
        np.testing.assert_allclose(M.ed(ori, gen, dev)[0], float(z[f"ed_{k}"]), rtol=2e-6)
        np.testing.assert_allclose(M.crps(ori, runs, dev)[0], float(z[f"crps_{k}"]), rtol=1e-5)
        m, sims, _ = M.mrr(ori, runs, 0.5, dev)
        assert abs(m - float(z[f"mrr_{k}"])) < 1e-6
        np.testing.assert_allclose(sims.numpy(), z[f"sims_{k}"], rtol=1e-5, atol=1e-6)
