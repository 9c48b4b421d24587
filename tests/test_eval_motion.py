"""The motion entries t2s_eval_corr / t2s_eval_shift / t2s_eval_dtw_ragged (csrc/t2s_eval_motion.hip, mirrored in
t2ms_amd.metrics) against the fp64 restatements of tests/_eval_motion_ref.py, which tests/test_eval_motion_host.py pins on
the CPU to the reference-made fixture: every table / min_dist / per_sample / matrix element and every mean, at the lane
stride, block, length and chunk edges of the kernels, and the two drivers.  Needs a real MI355X (`pytest -m gpu`).

Tolerances (u = 2^-24, the unit roundoff of fp32; relative unless stated; an expected exact 0, NaN or Inf must come out
as exactly that).
  Shift table, min_dist, DTW per sample: fp64 accumulation and one rounding to fp32 -> 2 u (one rounding plus one u of slack
    for the device's fp64 sqrt and another fp64 summation order, as tests/test_eval_paired.py allows ED / DTW).
  out of shift / DTW: the fp64 mean of non-negative fp32 values carrying 2 u each, rounded once -> 3 u.
  Correlation elements: |got - want| <= 2 u |want| + 2^-29.  The first term is the rounding of the stored element; the
    second the fp64 sums: a sum of rows <= 2^24 products errs by at most rows 2^-53 <= 2^-29 relative to sum |x_i x_j|, which
    after the normalisation by sqrt(c_ii c_jj) is at most 1 (Cauchy-Schwarz).
  Score: see test_correlation_layouts.
best_shift is compared with the restatement's only on pairs that tests/test_eval_motion_host.py
(test_every_compared_search_is_far_from_a_tie) holds >= 1e-3 = 2^14 u away from a tie, or whose tie is exact by construction.
Every check prints its own worst error as an `EVALERR` line."""
import glob
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _eval_motion_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, GUARD = -7.0, 64
CORR_ABS = 2.0 ** -29
_spec = importlib.util.spec_from_file_location("gen_golden_motion", os.path.join(REPO, "tests", "golden", "gen_golden_motion.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "motion_metrics.npz"))


# --------------------------------------------------------------------------------------------------------------- helpers
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


def bits(t):
    return np.asarray(t, dtype=np.float32).view(np.uint32)


def check_shift(a, b, la, lb, dev, what):
    """One call of the mirror against the restatement: table, min_dist, best_shift, out; min_dist is table[best] bitwise."""
    value, best, dist, table = M.sequence_correlation(a, b, None if la is None and lb is None else (la, lb), dev)
    want_t, want_b, want_d = R.shift(a, b, la, lb)
    shape = (a.shape, b.shape)
    zero = min(a.shape[1], b.shape[1]) - 1
    assert table.shape == want_t.shape and best.dtype == torch.int32
    check("shift", what + " table", shape, table.numpy(), want_t, 2)          # NaN exactly in the absent columns, nowhere else
    check("shift", what + " min_dist", shape, dist.numpy(), want_d, 2)
    assert np.array_equal(best.numpy(), want_b), (what, best, want_b)
    picked = table.numpy()[np.arange(a.shape[0]), zero + best.numpy()]
    assert np.array_equal(bits(picked), bits(dist.numpy())), what
    if np.isfinite(want_d).all():
        check("shift", what + " out", shape, [value], [want_d.mean()], 3)
    return best, dist, table


def raw_shift(dev, a, b, la, lb, dims, table_floats, null=()):
    """t2s_eval_shift on guarded outputs (table, min_dist, out in one SENTINEL buffer, GUARD floats after each; best_shift
    in an int buffer of its own) -> (rc, message, table, best, dist, out, guards untouched)."""
    n = dims[0]
    sizes = (table_floats, n, 1)
    buf = torch.full((sum(sizes) + 3 * GUARD,), SENTINEL, device=dev)
    offs = [0, table_floats + GUARD, table_floats + n + 2 * GUARD]
    parts = [buf[o:o + s] for o, s in zip(offs, sizes)]
    best = torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev)
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    tla = None if la is None else torch.from_numpy(np.asarray(la, np.int32)).to(dev)
    tlb = None if lb is None else torch.from_numpy(np.asarray(lb, np.int32)).to(dev)
    ptr = lambda t, name: None if t is None or name in null else t.data_ptr()
    with torch.cuda.device(dev):
        rc = L.lib().t2s_eval_shift(ptr(ta, "a"), ptr(tb, "b"), ptr(tla, "la"), ptr(tlb, "lb"), ptr(parts[0], "table"),
                                    ptr(best, "best"), ptr(parts[1], "dist"), ptr(parts[2], "out"), *dims, L.stream_ptr(dev))
    torch.cuda.synchronize()
    msg = L.lib().t2s_last_error().decode() if rc != 0 else ""
    host, hb = buf.cpu(), best.cpu()
    guards = all(bool((host[o + s:o + s + GUARD] == SENTINEL).all()) for o, s in zip(offs, sizes)) and bool((hb[n:] == -7).all())
    return rc, msg, host[:table_floats].clone(), hb[:n].clone(), parts[1].cpu(), parts[2].cpu(), guards


def raw_dtw(dev, entry_args, n, null_out=False):
    """(rc, message, per, out, guards untouched) of t2s_eval_dtw_ragged(a, b, la, lb, per, out, *dims) on guarded outputs."""
    a, b, la, lb, dims = entry_args
    buf = torch.full((n + GUARD + 1 + GUARD,), SENTINEL, device=dev)
    per, out = buf[:n], buf[n + GUARD:n + GUARD + 1]
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    tla = None if la is None else torch.from_numpy(np.asarray(la, np.int32)).to(dev)
    tlb = None if lb is None else torch.from_numpy(np.asarray(lb, np.int32)).to(dev)
    with torch.cuda.device(dev):
        rc = L.lib().t2s_eval_dtw_ragged(ta.data_ptr(), tb.data_ptr(), None if tla is None else tla.data_ptr(),
                                         None if tlb is None else tlb.data_ptr(), per.data_ptr(),
                                         None if null_out else out.data_ptr(), *dims, L.stream_ptr(dev))
    torch.cuda.synchronize()
    msg = L.lib().t2s_last_error().decode() if rc != 0 else ""
    host = buf.cpu()
    guards = bool((host[n:n + GUARD] == SENTINEL).all() and (host[n + GUARD + 1:] == SENTINEL).all())
    return rc, msg, host[:n].clone(), host[n + GUARD:n + GUARD + 1].clone(), guards


# ----------------------------------------------------------------------------------------------------- sequence correlation
@pytest.mark.parametrize("name", list(R.GPU_SHIFT_CASES))
def test_shift_lane_stride_block_and_length_edges(dev, name):
    """ragged_10ch: m > n' and m < n', min(m, n') = 97 / 63 / 33 / 2 in one batch of 5, overlaps of 1 .. 97 points (63, 64,
    65 end the lane stride inside, on and after a pass), NaN padding; one_point: min = 1, W = 1; full_130_1ch: S = 1,
    overlaps up to 130 (a third pass of the stride), 259 shifts = four blocks and three, no length arrays;
    one_block_plus_one: min = 33, 65 shifts, n = 1; two_points: W = 3; longer_b: S = 7, lengths 1 and 2 inside a batch."""
    a, b, la, lb = R.gpu_shift_case(name)
    _, _, table = check_shift(a, b, la, lb, dev, name)
    lo = np.minimum(R.lengths_of(a, la), R.lengths_of(b, lb))
    zero = min(a.shape[1], b.shape[1]) - 1
    for i in range(a.shape[0]):                       # the padding is NaN: none of it reached a column the pair has
        valid = table[i, zero - (lo[i] - 1):zero + lo[i]]
        assert valid.numel() == 2 * lo[i] - 1 and bool(torch.isfinite(valid).all())
        assert int(torch.isnan(table[i]).sum()) == table.shape[1] - valid.numel()


@pytest.mark.parametrize("name", ["ragged_10ch", "longer_b"])
def test_shift_row_of_a_batch_is_that_pair_alone(dev, name):
    """The summation order depends on (m, n', s) alone: pair i cut out of the batch and out of its padding, and the batch
    in reverse order, give the same bits."""
    a, b, la, lb = R.gpu_shift_case(name)
    _, best, dist, table = M.sequence_correlation(a, b, (la, lb), dev)
    zero = min(a.shape[1], b.shape[1]) - 1
    for i in range(a.shape[0]):
        _, b1, d1, t1 = M.sequence_correlation(a[i:i + 1, :la[i]], b[i:i + 1, :lb[i]], None, dev)
        m = min(la[i], lb[i]) - 1
        assert t1.shape == (1, 2 * m + 1)
        assert np.array_equal(bits(t1[0]), bits(table[i, zero - m:zero + m + 1])) and b1[0] == best[i]
        assert np.array_equal(bits(d1), bits(dist[i:i + 1]))
    _, rb, rd, rt = M.sequence_correlation(a[::-1].copy(), b[::-1].copy(), (la[::-1].copy(), lb[::-1].copy()), dev)
    assert np.array_equal(bits(rt.numpy()[::-1]), bits(table)) and np.array_equal(rb.numpy()[::-1], best.numpy())
    again = M.sequence_correlation(a, b, (la, lb), dev)
    assert np.array_equal(bits(again[3]), bits(table)) and np.array_equal(bits(again[2]), bits(dist))


def test_shift_known_answers_and_the_search_rule(dev):
    a, _ = R.planted(5, 3, 20, 20, 4, (0, 0, 0))
    value, best, dist, table = M.sequence_correlation(a, a, None, dev)
    assert value == 0.0 and (best == 0).all() and (dist == 0).all() and (table[:, 19] == 0).all()
    # every shift 0.75 exactly: the first one, -M, wins
    ta, tb, la, lb = R.tie_case()
    value, best, dist, table = M.sequence_correlation(ta, tb, (la, lb), dev)
    assert best.tolist() == [-6, -4] and (dist == 0.75).all() and value == 0.75
    assert bool((table[~torch.isnan(table)] == 0.75).all()) and int(torch.isnan(table[1]).sum()) == 13 - 9
    # the NaN rule: at the first shift it stays, elsewhere it is never chosen
    na, nb, _, _ = R.nan_cases()
    best, dist, _ = check_shift(na, nb, None, None, dev, "nan rule")
    assert best.tolist() == [-11, -6] and np.isnan(dist[0].item()) and np.isfinite(dist[1].item())
    # the one-point overlap that beats the planted shift at one channel
    m = 8
    oa = np.arange(m, dtype=np.float32).reshape(1, m, 1)
    ob = (np.arange(m, dtype=np.float32) - 1 + 0.125).reshape(1, m, 1)
    ob[0, 0, 0] = oa[0, m - 1, 0]
    _, best, dist, table = M.sequence_correlation(oa, ob, None, dev)
    assert best[0] == -(m - 1) and dist[0] == 0.0 and table[0, m] == 0.125
    # two lists of recordings are the padded arrays with their lengths
    a, b, la, lb = R.gpu_shift_case("longer_b")
    got = M.sequence_correlation([a[i, :la[i]] for i in range(5)], [b[i, :lb[i]] for i in range(5)], None, dev)
    want = M.sequence_correlation(a, b, (la, lb), dev)
    w = got[3].shape[1]                                # the lists pad to the longest recording: 63 / 65 here too
    assert w == want[3].shape[1] and np.array_equal(bits(got[3]), bits(want[3])) and torch.equal(got[1], want[1])


def test_shift_equals_the_reference_on_the_fixture(dev, gold):
    for k in range(len(G.SHIFT_CASES)):
        a, b, la, lb = (gold[f"{p}_{k}"] for p in ("sa", "sb", "sla", "slb"))
        _, best, dist, _ = M.sequence_correlation(a, b, (la, lb), dev)
        assert np.array_equal(best.numpy(), gold[f"sbest_{k}"])
        check("shift", f"fixture {k} min_dist", a.shape, dist.numpy(), gold[f"sdist_{k}"], 2)


def test_shift_refusals_and_clamped_lengths(dev):
    a, b, la, lb = R.gpu_shift_case("longer_b")
    n, La, Lb, S = 5, 63, 65, 7
    W = 2 * min(La, Lb) - 1
    # the kernels clamp a length into [1, L]: lengths beyond either end behave as 1 resp. L (the mirror refuses them)
    a0, b0 = np.nan_to_num(a, nan=0.25), np.nan_to_num(b, nan=0.5)
    rc, _, t_wild, best_wild, d_wild, _, guards = raw_shift(dev, a0, b0, [0, -5, 63, 64, 10 ** 9], [66, 1, 2, -1, 65], (n, La, Lb, S), n * W)
    assert rc == 0 and guards
    rc, _, t_ok, best_ok, d_ok, _, _ = raw_shift(dev, a0, b0, [1, 1, 63, 63, 63], [65, 1, 2, 1, 65], (n, La, Lb, S), n * W)
    assert rc == 0 and np.array_equal(bits(t_wild), bits(t_ok)) and torch.equal(best_wild, best_ok) and np.array_equal(bits(d_wild), bits(d_ok))
    for dims, null, word in (((n, 4097, Lb, S), (), "La=4097"), ((n, La, 4097, S), (), "Lb=4097"), ((n, 0, Lb, S), (), "La=0"),
                             ((0, La, Lb, S), (), "n=0"), ((n, La, Lb, 0), (), "n_series=0"), ((n, La, Lb, S), ("table",), "NULL"),
                             ((n, La, Lb, S), ("a",), "NULL")):
        rc, msg, t, bs, d, o, guards = raw_shift(dev, a0, b0, la, lb, dims, n * W, null)
        assert rc != 0 and "t2s_eval_shift" in msg and word in msg, (dims, null, msg)
        assert guards and bool((t == SENTINEL).all()) and bool((d == SENTINEL).all()) and bool((o == SENTINEL).all()) and bool((bs == -7).all())


# ---------------------------------------------------------------------------------------------------------------- ragged DTW
DTW_LENGTHS = [(1, 1), (1, 9), (9, 1), (40, 33), (33, 40), (257, 130)]


@pytest.fixture(scope="module")
def dtw_batch():
    """The six pairs as one padded batch (6, 257, 3) / (6, 130, 3) with NaN padding, and the restatement, computed once."""
    rs = np.random.RandomState(81)
    n = len(DTW_LENGTHS)
    scale = 1.0 + 0.5 * np.arange(n)[:, None, None] + 0.25 * np.arange(3)[None, None, :]
    a = (scale * rs.uniform(0.1, 1.0, (n, 257, 3))).astype(np.float32)
    b = (scale * rs.uniform(0.1, 1.0, (n, 130, 3))).astype(np.float32)
    la, lb = np.asarray([m for m, _ in DTW_LENGTHS], np.int32), np.asarray([k for _, k in DTW_LENGTHS], np.int32)
    for i in range(n):
        a[i, la[i]:] = np.nan
        b[i, lb[i]:] = np.nan
    return a, b, la, lb, R.dtw_ragged(a, b, la, lb)


def test_dtw_ragged_lengths(dev, dtw_batch):
    """(1, 1), a single row and a single column, m > n' and m < n', and (257, 130): more than 256 cells on a diagonal, a
    second pass of the 256 threads.  As one batch, and every pair alone without padding: the same bits."""
    a, b, la, lb, want = dtw_batch
    value, per = M.dtw_ragged(a, b, (la, lb), dev)
    check("dtw_ragged", "batch", (a.shape, b.shape), per.numpy(), want, 2)
    check("dtw_ragged", "batch out", (a.shape, b.shape), [value], [want.mean()], 3)
    for i in range(a.shape[0]):
        v1, p1 = M.dtw_ragged(a[i:i + 1, :la[i]], b[i:i + 1, :lb[i]], None, dev)
        assert np.array_equal(bits(p1), bits(per[i:i + 1])) and np.float32(v1) == p1[0].item()
    got = M.dtw_ragged([a[i, :la[i]] for i in range(6)], [b[i, :lb[i]] for i in range(6)], None, dev)
    assert np.array_equal(bits(got[1]), bits(per))


def test_dtw_ragged_equals_the_reference_on_the_fixture(dev, gold):
    first = [gold[f"da_{k}"] for k in range(len(G.DTW_CASES))]
    second = [gold[f"db_{k}"] for k in range(len(G.DTW_CASES))]
    _, per = M.dtw_ragged(first, second, None, dev)
    check("dtw_ragged", "fixture", G.DTW_CASES, per.numpy(), [float(gold[f"dtw_{k}"]) for k in range(len(G.DTW_CASES))], 2)
    _, swapped = M.dtw_ragged(second[:1], first[:1], None, dev)
    check("dtw_ragged", "fixture swapped", G.DTW_CASES[0], swapped.numpy(), [float(gold["dtw_0"])], 2)


def test_dtw_ragged_equal_lengths_is_t2s_eval_dtw_bit_for_bit(dev, dtw_batch):
    """(2, 300, 300, S 3): 37.5 KiB of diagonals, under the default cap; (1, 4096, 4096, S 1): 96 KiB, the raised cap, the
    largest table either entry takes; then a small launch after the raised cap gives the bits it gave before."""
    a, b, la, lb, _ = dtw_batch
    _, small_before = M.dtw_ragged(a[2:3, :9], b[2:3, :1], None, dev)
    rs = np.random.RandomState(82)
    x = rs.uniform(0, 1, (2, 300, 3)).astype(np.float32)
    y = (x + 0.3 * rs.randn(2, 300, 3)).astype(np.float32)
    v0, p0 = M.dtw(x, y, dev)
    v1, p1 = M.dtw_ragged(x, y, None, dev)
    assert np.array_equal(bits(p0), bits(p1)) and v0 == v1 and bool((p1 > 0).all())
    check("dtw_ragged", "300 x 300", x.shape, p1.numpy(), R.dtw_ragged(x, y), 2)
    x = rs.uniform(0, 1, (1, 4096, 1)).astype(np.float32)
    y = np.roll(x, 5, axis=1) + np.float32(0.125)
    v0, p0 = M.dtw(x, y, dev)
    v1, p1 = M.dtw_ragged(x, y, None, dev)
    assert np.array_equal(bits(p0), bits(p1)) and v0 == v1 and p1[0] > 0
    _, small_after = M.dtw_ragged(a[2:3, :9], b[2:3, :1], None, dev)
    assert np.array_equal(bits(small_before), bits(small_after))
    # a length array that cuts the 4096 x 4096 storage down to 40 x 33 is the small case
    _, cut = M.dtw_ragged(x, y, ([40], [33]), dev)
    _, alone = M.dtw_ragged(x[:, :40], y[:, :33], None, dev)
    assert np.array_equal(bits(cut), bits(alone))


def test_dtw_ragged_non_finite_and_refusals(dev, dtw_batch):
    a, b, la, lb, want = dtw_batch
    for bad, ok in ((np.nan, np.isnan), (np.inf, np.isposinf)):
        g = b.copy()
        g[3, 7, 1] = bad
        value, per = M.dtw_ragged(a, g, (la, lb), dev)
        assert ok(per[3].item()) and ok(value) and np.array_equal(bits(np.delete(per.numpy(), 3)), bits(np.delete(M.dtw_ragged(a, b, (la, lb), dev)[1].numpy(), 3)))
    a0, b0 = np.nan_to_num(a, nan=0.25), np.nan_to_num(b, nan=0.5)
    for dims, word in (((6, 4097, 130, 3), "La=4097"), ((6, 257, 4097, 3), "Lb=4097"), ((6, 257, 0, 3), "Lb=0"), ((0, 257, 130, 3), "n=0")):
        rc, msg, per, out, guards = raw_dtw(dev, (a0, b0, la, lb, dims), 6)
        assert rc != 0 and "t2s_eval_dtw_ragged" in msg and word in msg, (dims, msg)
        assert guards and bool((per == SENTINEL).all()) and bool((out == SENTINEL).all())
    rc, msg, per, out, guards = raw_dtw(dev, (a0, b0, la, lb, (6, 257, 130, 3)), 6, null_out=True)
    assert rc != 0 and "NULL" in msg and guards and bool((per == SENTINEL).all())
    # clamped lengths: beyond either end they behave as 1 resp. L
    rc, _, wild, _, guards = raw_dtw(dev, (a0, b0, [0, 300, 9, 40, -3, 257], [131, 9, 0, 33, 40, 130], (6, 257, 130, 3)), 6)
    rc2, _, tame, _, _ = raw_dtw(dev, (a0, b0, [1, 257, 9, 40, 1, 257], [130, 9, 1, 33, 40, 130], (6, 257, 130, 3)), 6)
    assert rc == 0 and rc2 == 0 and guards and np.array_equal(bits(wild), bits(tame))


# ------------------------------------------------------------------------------------------------------ correlational score
def corr_sets(seed, shape_o, shape_g):
    """Two sets of correlated channels on a 1/64 grid (so that a constant written into one is an exact mean)."""
    rs = np.random.RandomState(seed)
    S = shape_o[-1]
    mix = rs.uniform(-1, 1, (S, S)) + np.eye(S)
    ori = rs.randn(*shape_o[:-1], S) @ mix + 0.3 * np.arange(S)
    gen = rs.randn(*shape_g[:-1], S) @ (mix + 0.4 * rs.uniform(-1, 1, (S, S))) + 0.3 * np.arange(S)
    return (np.round(ori * 64) / 64).astype(np.float32), (np.round(gen * 64) / 64).astype(np.float32)


def score_bound(want_c, want_s):
    """The absolute bound of the score that test_correlation_layouts derives."""
    S = want_c.shape[-1]
    ratio = np.abs(want_c[0] - want_c[1]).sum() / np.abs(want_c[0]).sum()
    return S * (2 + ratio) * CORR_ABS / (1 - S * CORR_ABS) + 2 * R.U * abs(want_s)


def check_corr(ori, gen, dev, what):
    score, corr = M.correlational_score(ori, gen, dev)
    want_s, want_c = R.corr_score(ori, gen)
    S = ori.shape[-1]
    assert corr.shape == (2, S, S)
    got = corr.numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want_c))
    fin = ~np.isnan(want_c)
    excess = np.abs(got[fin] - want_c[fin]) - (2 * R.U * np.abs(want_c[fin]) + CORR_ABS)
    print(f"EVALERR corr {what} shape={ori.shape, gen.shape} worst excess over 2u|want| + 2^-29 = {excess.max():.3e} (<= 0)")
    assert excess.max() <= 0, (what, excess.max())
    assert (np.abs(got[fin]) <= 1).all()
    if np.isnan(want_s):
        assert np.isnan(score)
    else:
        bound = score_bound(want_c, want_s)
        print(f"EVALERR corr {what} score |got - want| = {abs(score - want_s):.3e} bound = {bound:.3e}")
        assert abs(score - want_s) <= bound, (what, score, want_s, bound)
    return score, corr


@pytest.mark.parametrize("shape_o,shape_g", [((2, 1), (63, 1)), ((63, 2), (2, 2)), ((1024, 7), (1025, 7)), ((1025, 64), (300, 64)),
                                             ((6, 40, 7), (6, 40, 7)), ((3, 10, 5), (7, 4, 5))])
def test_correlation_layouts(dev, shape_o, shape_g):
    """rows = 2 (the fewest), 63, 1024 (the last shape with one row per chunk) and 1025 (the first chunk of two rows);
    S = 1, 2, 7 and 64 (the most); rows_ori != rows_gen; (N, L, S) input flattened as the reference does.
    Score bound (absolute).  The kernel takes the score from its fp64 matrices, whose elements carry the 2^-29 part of the
    element bound (the 2 u |want| part is the rounding of the STORED element, which the score never sees); write d = 2^-29,
    N = sum |C_ori - C_gen|, D = sum |C_ori|.  |dN| <= 2 S^2 d (two matrices), |dD| <= S^2 d, and D >= S (the diagonal is
    1), so |d(N / D)| <= (|dN| + (N / D) |dD|) / (D - |dD|) <= S d (2 + N / D) / (1 - S d); the score is then rounded once to
    fp32 and the fp64 sums of S^2 <= 4096 terms add less than another u of |score|: + 2 u |score|."""
    ori, gen = corr_sets(90 + shape_o[0], shape_o, shape_g)
    score, corr = check_corr(ori, gen, dev, "layout")
    again = M.correlational_score(ori, gen, dev)
    assert again[0] == score and np.array_equal(bits(again[1]), bits(corr))
    if shape_o[-1] == 1:
        assert score == 1.0 and bool((corr == 1).all())


def test_correlation_identical_sets_and_constant_channels(dev, gold):
    ori, gen = corr_sets(95, (5, 30, 6), (4, 20, 6))
    score, corr = M.correlational_score(ori, ori, dev)
    assert score == 1.0 and np.array_equal(bits(corr[0]), bits(corr[1]))
    gen[..., 2] = 0.375                                  # a constant channel of the generated set: its row and column, and the score
    score, corr = check_corr(ori, gen, dev, "constant channel (gen)")
    nan = torch.isnan(corr[1])
    assert np.isnan(score) and bool(nan[2].all()) and bool(nan[:, 2].all()) and int(nan.sum()) == 11 and not bool(torch.isnan(corr[0]).any())
    score, corr = check_corr(gen, ori, dev, "constant channel (ori)")
    assert np.isnan(score) and int(torch.isnan(corr[0]).sum()) == 11
    for k in range(3):                                   # the reference's own matrices and scores
        s, c = M.correlational_score(gold[f"co_{k}"], gold[f"cg_{k}"], dev)
        for got, want in ((c[0].numpy(), gold[f"cmo_{k}"]), (c[1].numpy(), gold[f"cmg_{k}"])):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            fin = ~np.isnan(want)
            assert (np.abs(got[fin] - want[fin]) <= 2 * R.U * np.abs(want[fin]) + CORR_ABS).all()
        want = float(gold[f"cs_{k}"])
        assert (np.isnan(s) and np.isnan(want)) or abs(s - want) <= score_bound(np.stack([gold[f"cmo_{k}"], gold[f"cmg_{k}"]]), want)


def test_correlation_refusals(dev):
    ori, gen = corr_sets(96, (40, 5), (30, 5))
    a, g = torch.from_numpy(ori).to(dev), torch.from_numpy(gen).to(dev)
    need = L.lib().t2s_eval_corr_workspace_bytes(40, 30, 5)
    assert need > 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    buf = torch.full((50 + GUARD + 1 + GUARD,), SENTINEL, device=dev)
    corr, out = buf[:50], buf[50 + GUARD:50 + GUARD + 1]

    def call(rows_o, rows_g, S, ws_bytes, ptr_ori=a.data_ptr()):
        with torch.cuda.device(dev):
            rc = L.lib().t2s_eval_corr(ptr_ori, g.data_ptr(), corr.data_ptr(), out.data_ptr(), rows_o, rows_g, S, ws.data_ptr(), ws_bytes,
                                       L.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, (L.lib().t2s_last_error().decode() if rc else "")

    for args, word in (((40, 30, 65, need), "n_series=65"), ((1, 30, 5, need), "rows_ori=1"), ((40, 1, 5, need), "rows_gen=1"),
                       ((40, 30, 0, need), "n_series=0"), ((40, 30, 5, need - 1), f"workspace of {need - 1} bytes"),
                       ((40, 30, 5, need, None), "NULL")):
        rc, msg = call(*args)
        assert rc != 0 and "t2s_eval_corr" in msg and word in msg, (args, msg)
        assert bool((buf == SENTINEL).all()), args
    rc, _ = call(40, 30, 5, need)
    host = buf.cpu()
    assert rc == 0 and bool((host[50:50 + GUARD] == SENTINEL).all()) and bool((host[51 + GUARD:] == SENTINEL).all())
    want_s, want_c = R.corr_score(ori, gen)
    assert np.abs(host[:50].numpy().reshape(2, 5, 5) - want_c).max() <= 2 * R.U + CORR_ABS
    assert abs(host[50 + GUARD].item() - want_s) <= score_bound(want_c, want_s)
    # corr may be NULL: the score is the same bits
    with torch.cuda.device(dev):
        rc = L.lib().t2s_eval_corr(a.data_ptr(), g.data_ptr(), None, buf[50:51].data_ptr(), 40, 30, 5, ws.data_ptr(), need, L.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(bits(buf[50:51].cpu()), bits(host[50 + GUARD:51 + GUARD]))


# ------------------------------------------------------------------------------------------------------------------- drivers
def test_evaluation_driver_writes_cs_and_sc(dev, tmp_path, monkeypatch):
    import evaluation as ev
    monkeypatch.chdir(tmp_path)
    ori, gen = R.planted(97, 5, 24, 24, 3, (0, 1, -2, 3, 0))
    save = str(tmp_path / "results")
    name = "flowmatching_DiT_ETTh1_24_9.0_10"
    g = os.path.join(save, "generation", name)
    for r in range(10):
        os.makedirs(os.path.join(g, f"run_{r}"))
        np.save(os.path.join(g, f"run_{r}", "x_1.npy"), ori)
        np.save(os.path.join(g, f"run_{r}", "x_t.npy"), gen)
    np.save(os.path.join(g, "x_t.npy"), gen)
    single, _ = ev.main(["--dataset_name", "ETTh1_24", "--save_path", save, "--method_list", "MSE,CS,SC"])
    assert set(single) == {"MSE", "CS", "SC"}
    assert single["CS"] == M.correlational_score(ori, gen, dev)[0] and single["SC"] == M.sequence_correlation(ori, gen, None, dev)[0]
    assert single["MSE"] == M.mse_wape(ori, gen)[0] and np.isfinite(single["CS"]) and single["SC"] > 0
    files = sorted(glob.glob(os.path.join(save, "evaluation", name, f"{name}_ETTh1_24_*.json")))
    assert json.load(open(files[0])) == single


def test_compare_recordings_equals_direct_calls(dev, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("compare_recordings", os.path.join(REPO, "tools", "compare_recordings.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a, b = R.planted(98, 2, 30, 22, 4, (3, -2))
    recs = [a[0].astype(np.float64) * 3 + 1, b[0].astype(np.float64) * 3 + 1, a[1].astype(np.float64)[:22]]
    paths = [str(tmp_path / "r0.npy"), str(tmp_path / "r1.txt"), str(tmp_path / "r2.npy")]
    np.save(paths[0], recs[0])
    np.savetxt(paths[1], recs[1], delimiter=",", fmt="%.17g")
    np.save(paths[2], recs[2])
    result = tool.main(paths)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(result))
    norm = [tool.min_max_normalize_columns(r).astype(np.float32) for r in recs]
    assert all(x.min() == 0 and x.max() == 1 for x in norm) and result["lengths"] == [30, 22, 22]
    for i in range(3):
        for j in range(3):
            if i == j:
                assert all(result[k][i][j] is None for k in ("CS", "SC_dist", "SC_shift", "DTW", "MSE", "WAPE"))
                continue
            _, shift, dist, _ = M.sequence_correlation([norm[i]], [norm[j]], None, dev)
            assert result["SC_shift"][i][j] == int(shift[0]) and result["SC_dist"][i][j] == float(dist[0])
            assert result["DTW"][i][j] == float(M.dtw_ragged([norm[i]], [norm[j]], None, dev)[1][0])
            assert result["CS"][i][j] == M.correlational_score(norm[i], norm[j], dev)[0]
            if len(norm[i]) == len(norm[j]):
                mse, wape, _ = M.mse_wape(norm[i][None], norm[j][None], dev)
                assert result["MSE"][i][j] == mse and result["WAPE"][i][j] == wape
            else:
                assert result["MSE"][i][j] is None and result["WAPE"][i][j] is None
