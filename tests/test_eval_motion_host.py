"""CPU pins of tests/_eval_motion_ref.py, the fp64 restatements that tests/test_eval_motion.py judges the motion entries
(t2s_eval_corr / t2s_eval_shift / t2s_eval_dtw_ragged, csrc/t2s_eval_motion.hip) by: against tests/golden/motion_metrics.npz,
which the reference's evaluate/metrics.py made (tests/golden/gen_golden_motion.py), and against known answers.  Both sides
of the fixture comparison are fp64 on inputs that are exact in fp32 and fp64 and differ only in the order of their sums:
rtol 1e-12 for values, best_shift must be equal.  Also held here: the condition that makes best_shift comparable at all
(test_every_compared_search_is_far_from_a_tie), the header's NaN / Inf rules, the symbol table and the mirror's host
refusals.  No GPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import _eval_motion_ref as R
import _eval_paired_ref as P
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_motion", os.path.join(REPO, "tests", "golden", "gen_golden_motion.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ENTRIES = ("t2s_eval_corr", "t2s_eval_shift", "t2s_eval_dtw_ragged")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "motion_metrics.npz"))


# ------------------------------------------------------------------------------------------- the reference-made fixture
def test_shift_restatement_equals_the_reference(gold):
    for k, (n, La, Lb, S, shifts) in enumerate(G.SHIFT_CASES):
        a, b, la, lb = (gold[f"{p}_{k}"] for p in ("sa", "sb", "sla", "slb"))
        assert a.shape == (n, La, S) and b.shape == (n, Lb, S) and a.dtype == np.float32
        table, best, dist = R.shift(a, b, la, lb)
        assert np.array_equal(best, gold[f"sbest_{k}"]), (k, best, gold[f"sbest_{k}"])
        np.testing.assert_allclose(dist, gold[f"sdist_{k}"], rtol=1e-12)
        assert np.array_equal(best, shifts)                       # the planted shift is the one the reference finds
        zero = min(La, Lb) - 1
        for i in range(n):                                        # columns outside the pair's own -M .. M are NaN
            m = min(la[i], lb[i]) - 1
            assert np.isfinite(table[i, zero - m:zero + m + 1]).all()
            assert np.isnan(table[i, :zero - m]).all() and np.isnan(table[i, zero + m + 1:]).all()


def test_correlation_restatement_equals_the_reference(gold):
    for k, (_, _, const) in enumerate(G.CORR_CASES):
        score, c = R.corr_score(gold[f"co_{k}"], gold[f"cg_{k}"])
        for got, want in ((c[0], gold[f"cmo_{k}"]), (c[1], gold[f"cmg_{k}"])):
            assert np.array_equal(np.isnan(got), np.isnan(want))              # NaN exactly where numpy puts it
            np.testing.assert_allclose(got, want, rtol=1e-12)
        if const is None:
            np.testing.assert_allclose(score, float(gold[f"cs_{k}"]), rtol=1e-12)
        else:
            assert np.isnan(score) and np.isnan(float(gold[f"cs_{k}"]))
            nan = np.isnan(c[1])
            assert nan[const].all() and nan[:, const].all() and nan.sum() == 2 * c.shape[1] - 1 and not np.isnan(c[0]).any()


def test_dtw_restatement_equals_the_reference(gold):
    for k, (m, n) in enumerate(G.DTW_CASES):
        a, b = gold[f"da_{k}"], gold[f"db_{k}"]
        assert a.shape == (m, G.DTW_SERIES) and b.shape == (n, G.DTW_SERIES)
        np.testing.assert_allclose(R.dtw_ragged(a[None], b[None])[0], float(gold[f"dtw_{k}"]), rtol=1e-12)
    # symmetric in its arguments, in the reference and here
    a, b = gold["da_0"], gold["db_0"]
    np.testing.assert_allclose(R.dtw_ragged(b[None], a[None])[0], float(gold["dtw_0"]), rtol=1e-12)


def test_fixture_arrays_are_the_generators(gold):
    for k in range(len(G.SHIFT_CASES)):
        for got, want in zip((gold[f"{p}_{k}"] for p in ("sa", "sb", "sla", "slb")), G.make_shift_case(k)):
            assert np.array_equal(got, want) and got.dtype == want.dtype
    for k in range(len(G.CORR_CASES)):
        ori, gen = G.make_corr_case(k)
        assert np.array_equal(gold[f"co_{k}"], ori) and np.array_equal(gold[f"cg_{k}"], gen)
    for k in range(len(G.DTW_CASES)):
        a, b = G.make_dtw_case(k)
        assert np.array_equal(gold[f"da_{k}"], a) and np.array_equal(gold[f"db_{k}"], b)
    for key in gold.files:                                        # every input sits on the 1/1024 grid: exact in fp32 and fp64
        if gold[key].dtype == np.float32:
            assert np.array_equal(gold[key] * 1024, np.round(gold[key] * 1024)), key
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "motion_metrics.npz")) < 100 * 1024


# -------------------------------------------------------------------------------------------------------- known answers
def test_identical_sequences_give_shift_0_and_distance_0():
    a, _ = R.planted(5, 3, 20, 20, 4, (0, 0, 0))
    table, best, dist = R.shift(a, a)
    assert (best == 0).all() and (dist == 0).all() and (table[:, 19] == 0).all()
    assert (R.dtw_ragged(a, a) == 0).all()


def test_all_tie_case_goes_to_the_first_shift():
    a, b, la, lb = R.tie_case()
    table, best, dist = R.shift(a, b, la, lb)
    assert np.array_equal(best, [-6, -4]) and (dist == 0.75).all()
    assert (table[~np.isnan(table)] == 0.75).all()


def test_one_point_overlap_can_win_at_one_channel():
    """The reference's rule, not a bug of the restatement: with one channel a one-point overlap whose two values happen to
    agree beats the planted alignment.  a = 0, 1, 2, ..., b = a shifted by 1 plus 1/8, but b's first value equals a's last:
    shift -M compares exactly that pair."""
    m = 8
    a = np.arange(m, dtype=np.float32).reshape(1, m, 1)
    b = (np.arange(m, dtype=np.float32) - 1 + 0.125).reshape(1, m, 1)
    b[0, 0, 0] = a[0, m - 1, 0]
    table, best, dist = R.shift(a, b)
    assert best[0] == -(m - 1) and dist[0] == 0.0
    assert table[0, m - 1 + 1] == 0.125                          # the planted shift 1: every point 1/8 apart


def test_nan_rule_of_the_search():
    a, b, _, _ = R.nan_cases()
    table, best, dist = R.shift(a, b)
    assert best[0] == -11 and np.isnan(dist[0])                   # the first shift's only point pair holds the NaN: it stays
    assert best[1] == -6 and np.isfinite(dist[1])                 # a NaN elsewhere is never chosen
    assert np.isnan(table[1, 11 - 6 + 1:]).sum() > 0 and np.isfinite(table[1, 11 - 6])
    assert R.search(np.asarray([np.nan, 1.0, 0.5], np.float32)) == 0
    assert R.search(np.asarray([2.0, np.nan, 0.5, 0.5], np.float32)) == 2


def test_correlation_edges():
    rs = np.random.RandomState(8)
    x = (np.round(rs.randn(5, 9, 6) * 64) / 64).astype(np.float32)
    score, c = R.corr_score(x, x)
    assert score == 1.0 and np.array_equal(c[0], c[1]) and (np.abs(c) <= 1).all()
    np.testing.assert_allclose(c[0], np.corrcoef(x.reshape(-1, 6).astype(np.float64), rowvar=False), rtol=1e-12)
    y = x.copy()
    y[..., 3] = 0.375
    score, c = R.corr_score(y, x)                                 # a constant channel in the ORIGINAL set
    assert np.isnan(score) and np.isnan(c[0][3]).all() and np.isnan(c[0][:, 3]).all() and np.isnan(c[0]).sum() == 11
    one, c1 = R.corr_score(x[..., :1], y[..., 1:2])               # one channel: trivially 1 whenever it is defined
    assert abs(one - 1.0) <= 2.0 ** -50 and c1.shape == (2, 1, 1)


def test_dtw_ragged_at_equal_lengths_is_the_paired_restatement():
    rs = np.random.RandomState(9)
    for L_, S in ((1, 1), (7, 2), (40, 3)):
        a = rs.uniform(0, 1, (3, L_, S)).astype(np.float32)
        b = (a + 0.3 * rs.randn(3, L_, S)).astype(np.float32)
        assert np.array_equal(R.dtw_ragged(a, b), P.dtw(a, b))
    # unequal lengths against the plain double loop
    a, b = rs.uniform(0, 1, (1, 11, 2)), rs.uniform(0, 1, (1, 6, 2))
    t = np.full((12, 7), np.inf)
    t[0, 0] = 0
    for i in range(1, 12):
        for j in range(1, 7):
            t[i, j] = ((a[0, i - 1].astype(np.float32).astype(np.float64) - b[0, j - 1].astype(np.float32).astype(np.float64)) ** 2).sum() \
                + min(t[i - 1, j], t[i, j - 1], t[i - 1, j - 1])
    np.testing.assert_allclose(R.dtw_ragged(a, b)[0], np.sqrt(t[11, 6]), rtol=1e-14)
    padded = np.concatenate([a, np.full((1, 4, 2), np.nan)], axis=1)
    assert R.dtw_ragged(padded, b, [11], [6])[0] == R.dtw_ragged(a, b)[0]


# ------------------------------------------------------------------------------------------- the condition on the inputs
def _compared_pairs(gold):
    """(label, a_i, b_i, exact tie by construction) of EVERY pair whose best_shift a test compares, here or on the GPU."""
    sets = [(f"fixture {k}", gold[f"sa_{k}"], gold[f"sb_{k}"], gold[f"sla_{k}"], gold[f"slb_{k}"], False) for k in range(len(G.SHIFT_CASES))]
    sets += [(name, *R.gpu_shift_case(name), False) for name in R.GPU_SHIFT_CASES]
    sets += [("tie", *R.tie_case(), True), ("nan", *R.nan_cases(), False)]
    for label, a, b, la, lb, exact in sets:
        la, lb = R.lengths_of(a, la), R.lengths_of(b, lb)
        for i in range(a.shape[0]):
            yield f"{label}[{i}]", a[i, :la[i]], b[i, :lb[i]], exact


def test_every_compared_search_is_far_from_a_tie(gold):
    """best_shift of the kernel (fp32 values from one summation order) is compared with the restatement's (fp32 values from
    another): that is sound only where the smallest stored distance is not within a rounding of the second smallest.  For
    every such pair: the second smallest fp32-rounded distance exceeds the smallest by >= 1e-3 relative (2^14 u), or the
    tie is exact by construction (every distance the same exactly representable number).  No pair is left out."""
    count = 0
    for label, a, b, exact in _compared_pairs(gold):
        d = R.shift_distances(a, b)
        v32 = np.asarray(list(d.values())).astype(np.float32)
        if exact:
            assert len(set(v32.tolist())) == 1 and float(v32[0]) == list(d.values())[0], label
        else:
            assert R.gap(v32) >= 1e-3, (label, R.gap(v32))
        count += 1
    assert count == sum(c[0] for c in G.SHIFT_CASES) + sum(c[1] for c in R.GPU_SHIFT_CASES.values()) + 2 + 2


def test_planted_shifts_are_found(gold):
    for name, (_, n, _, _, S, shifts, la, lb) in R.GPU_SHIFT_CASES.items():
        a, b, la, lb = R.gpu_shift_case(name)
        _, best, _ = R.shift(a, b, la, lb)
        lo = np.minimum(R.lengths_of(a, la), R.lengths_of(b, lb))
        for i in range(n):
            if S > 1 and lo[i] >= 33:                             # long multichannel overlaps: the planted shift wins
                assert best[i] == shifts[i], (name, i, best[i])


# -------------------------------------------------------------------------------------------------- header and symbols
def test_header_states_the_non_finite_rule_next_to_each_entry():
    txt = open(os.path.join(REPO, "include", "t2s.h")).read()
    for name in ENTRIES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", txt, flags=re.S)
        assert m and "NaN" in m.group(1) and "Inf" in m.group(1), name
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int t2s_eval_shift\(", txt, flags=re.S).group(1)
    assert "left-to-right" in m and "strictly smaller" in m and "calculate_sequence_correlation" in m and "LAST pair" in m


def test_symbols_have_the_declared_signatures():
    I, VP, U64 = C.c_int, C.c_void_p, C.c_uint64
    assert L.SYMBOLS["t2s_eval_corr_workspace_bytes"] == (U64, [I, I, I])
    assert L.SYMBOLS["t2s_eval_corr"] == (I, [VP, VP, VP, VP, I, I, I, VP, U64, VP])
    assert L.SYMBOLS["t2s_eval_shift"] == (I, [VP] * 8 + [I, I, I, I, VP])
    assert L.SYMBOLS["t2s_eval_dtw_ragged"] == (I, [VP] * 6 + [I, I, I, I, VP])
    lib = L.lib()
    for name in ENTRIES + ("t2s_eval_corr_workspace_bytes",):
        assert hasattr(lib, name)
    txt = open(os.path.join(REPO, "include", "t2s.h")).read()
    assert re.search(r"#define\s+T2S_EVAL_CORR_MAX_SERIES\s+64\b", txt) and L.EVAL_CORR_MAX_SERIES == 64
    assert re.search(r"#define\s+T2S_EVAL_MOTION_MAX_LEN\s+4096\b", txt) and L.EVAL_MOTION_MAX_LEN == 4096
    # the workspace query refuses what the entry refuses, and names the value
    assert lib.t2s_eval_corr_workspace_bytes(1, 5, 3) == 0 and b"rows_ori=1" in lib.t2s_last_error()
    assert lib.t2s_eval_corr_workspace_bytes(5, 5, 65) == 0 and b"n_series=65" in lib.t2s_last_error()
    assert lib.t2s_eval_corr_workspace_bytes(2, 1025, 64) >= 8 * (2 * 1024 * 64 * 65 + 2 * 64 * 64)


# ------------------------------------------------------------------------------------------------ the mirror's refusals
def test_mirror_refuses_on_the_host(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a refusal must come before any GPU call")
    monkeypatch.setattr(L, "lib", no_gpu)
    monkeypatch.setattr(L, "stream_ptr", no_gpu)
    z = lambda *s: np.zeros(s, np.float32)
    for fn in (M.sequence_correlation, M.dtw_ragged):
        with pytest.raises(L.T2SError, match="no CPU fallback"):
            fn(z(2, 8, 3), z(2, 6, 3), device="cpu")
        with pytest.raises(L.T2SError, match="channel counts differ"):
            fn(z(2, 8, 3), z(2, 6, 4))
        with pytest.raises(L.T2SError, match=r"outside \[1, 8\]"):
            fn(z(2, 8, 3), z(2, 6, 3), lengths=([8, 9], None))
        with pytest.raises(L.T2SError, match=r"outside \[1, 6\]"):
            fn(z(2, 8, 3), z(2, 6, 3), lengths=(None, [0, 6]))
        with pytest.raises(L.T2SError, match="L=4097"):
            fn(z(1, 4097, 1), z(1, 6, 1))
        with pytest.raises(L.T2SError, match="L=4097"):
            fn(z(1, 6, 1), z(1, 4097, 1))
        with pytest.raises(L.T2SError, match="lists"):
            fn([z(4, 2)], z(1, 4, 2))
        with pytest.raises(L.T2SError, match="pad_ragged"):
            fn([z(4, 2), z(3, 3)], [z(4, 2), z(3, 2)])
    with pytest.raises(L.T2SError, match="no CPU fallback"):
        M.correlational_score(z(4, 8, 3), z(4, 8, 3), device="cpu")
    with pytest.raises(L.T2SError, match="channel counts differ"):
        M.correlational_score(z(4, 8, 3), z(4, 8, 2))
    with pytest.raises(L.T2SError, match="S=65"):
        M.correlational_score(z(4, 65), z(4, 65))
    with pytest.raises(L.T2SError, match="at least 2"):
        M.correlational_score(z(1, 1, 3), z(4, 8, 3))


def test_pad_ragged():
    seqs = [np.arange(6, dtype=np.float64).reshape(3, 2), np.ones((5, 2)), np.full((1, 2), 7.0)]
    x, n = M.pad_ragged(seqs)
    assert x.shape == (3, 5, 2) and x.dtype == np.float32 and n.dtype == np.int32 and n.tolist() == [3, 5, 1]
    assert np.array_equal(x[0, :3], seqs[0]) and (x[0, 3:] == 0).all() and (x[2, 1:] == 0).all() and x[2, 0, 1] == 7
    x1, n1 = M.pad_ragged([np.arange(4.0)])                       # a 1-D recording is one channel
    assert x1.shape == (1, 4, 1) and n1.tolist() == [4]


def test_driver_parser_accepts_cs_and_sc():
    import evaluation as ev
    args = ev.build_parser().parse_args(["--method_list", "MSE,CS,SC"])
    assert ev._methods(args.method_list) == ["MSE", "CS", "SC"]
    assert ev.build_parser().parse_args([]).method_list == "MSE,WAPE,MRR"
    assert "CS" in ev.__doc__ and "SC" in ev.__doc__ and "trivially 1" in ev.__doc__
