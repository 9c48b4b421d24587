"""The feature-based measures MDD / ACD / SD / KD (t2ms_amd.metrics, csrc/t2s_eval.hip) against the reference-made
fixture tests/golden/features.npz (evaluate/feature_based_measures.py run by tests/golden/gen_golden_features.py) and
against an fp64 numpy restatement of the definitions kept here.

Tolerances.  The four scalars, the per-set statistics and MDD's per-column losses are held to rtol 1e-5 (atol 1e-6 on the
statistics, whose ACF values pass through zero): the reference computes in fp32, whose sums over <= 7e3 values carry a
few 1e-7 of relative error, the kernels sum in fp64 and round once.  MDD's counts are integers and the fixture keeps every
judged value >= 1e-3 bin widths off a bin edge (the generator's `edge_margin`), so rtol 1e-5 on a column loss of
|count differences| / (50 n delta) means that every count is exact."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L
from t2ms_amd import metrics as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_features", os.path.join(REPO, "tests", "golden", "gen_golden_features.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
gpu = pytest.mark.gpu
NAMES = ("MDD", "ACD", "SD", "KD")


# ------------------------------------------------------------------------------------- fp64 restatement of the definitions
def np_stats(x):
    """mean, population variance, skewness, excess kurtosis (n_series,) and acf (n_series, K) of one (n, L, n_series) set."""
    x = np.asarray(x, dtype=np.float64)
    n, length, _ = x.shape
    d = x - x.mean(axis=(0, 1))
    var = (d ** 2).mean(axis=(0, 1))
    acf = np.stack([(d[:, k:] * d[:, :length - k]).mean(axis=(0, 1)) / var for k in range(min(64, length))], axis=1)
    skew = (d ** 3).mean(axis=(0, 1)) / (np.sqrt((d ** 2).sum(axis=(0, 1)) / (n * length - 1))) ** 3
    kurt = (d ** 4).mean(axis=(0, 1)) / var ** 2 - 3.0
    return {"mean": x.mean(axis=(0, 1)), "var": var, "skew": skew, "kurt": kurt, "acf": acf}


def np_counts(ori, x):
    """(50, L, n_series) counts of x's values in the 50 bins of each real column's [min, max]; outside counts nowhere."""
    o, x = np.asarray(ori, dtype=np.float64), np.asarray(x, dtype=np.float64)
    a, b = o.min(axis=0), o.max(axis=0)
    b = np.where(b == a, a + 1e-5, b)
    k = np.minimum(np.floor((x - a) / (b - a) * 50), 49).astype(np.int64)
    inside = (x >= a) & (x <= b)
    return np.stack([((k == j) & inside).sum(axis=0) for j in range(50)]), (b - a) / 50


def np_mdd_columns(ori, gen):
    co, delta = np_counts(ori, ori)
    cg, _ = np_counts(ori, gen)
    return (np.abs(cg - co) / (ori.shape[0] * delta)).mean(axis=0)           # (L, n_series)


def np_measures(ori, gen):
    so, sg = np_stats(ori), np_stats(gen)
    return {"MDD": float(np_mdd_columns(ori, gen).mean()),
            "ACD": float(np.sqrt(((sg["acf"] - so["acf"]) ** 2).sum(axis=1)).mean()),
            "SD": float(np.abs(sg["skew"] - so["skew"]).mean()),
            "KD": float(np.abs(sg["kurt"] - so["kurt"]).mean())}


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "features.npz"))
    cases = []
    for k, shape in enumerate(G.CASES):
        c = {name: z[f"{name}_{k}"] for name in ("ori", "gen", "mdd_cols", "acf_ori", "acf_gen", "skew_ori", "skew_gen",
                                                 "kurt_ori", "kurt_gen")}
        c.update({m: float(z[f"{m.lower()}_{k}"]) for m in NAMES})
        assert c["ori"].shape == shape and c["gen"].shape == shape
        cases.append(c)
    return cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def big():
    """n = 5000 samples of 24 steps: enough for every split of n over workgroups to engage; off the bin edges."""
    ori, gen, _ = G.snapped_sets(5000, 24, 1, 77)
    return ori, gen, np_measures(ori, gen), np_mdd_columns(ori, gen)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_is_off_the_bin_edges_and_well_away_from_zero(gold):
    for c in gold:
        assert G.edge_margin(c["ori"], c["ori"], True) >= G.MARGIN and G.edge_margin(c["ori"], c["gen"], False) >= G.MARGIN
        assert (c["ori"].max(axis=0) > c["ori"].min(axis=0)).all()
        assert min(c[m] for m in NAMES) > 0.3


def test_fp64_restatement_reproduces_the_reference(gold):
    for c in gold:
        got = np_measures(c["ori"], c["gen"])
        for m in NAMES:
            print(m, got[m], c[m], abs(got[m] - c[m]) / c[m])
            assert got[m] == pytest.approx(c[m], rel=1e-5), m
        n, length, s = c["ori"].shape
        # the reference lists the column losses channel-major
        np.testing.assert_allclose(np_mdd_columns(c["ori"], c["gen"]).T.reshape(-1), c["mdd_cols"], rtol=1e-5)
        for name in ("ori", "gen"):
            st = np_stats(c[name])
            np.testing.assert_allclose(st["acf"].T, c[f"acf_{name}"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(st["skew"], c[f"skew_{name}"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(st["kurt"], c[f"kurt_{name}"], rtol=1e-5, atol=1e-6)


def test_header_declares_the_three_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s.h")).read(), flags=re.S)
    for name in ("t2s_eval_features_workspace_bytes", "t2s_eval_moments", "t2s_eval_mdd"):
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in L.SYMBOLS
    assert "#define T2S_EVAL_MAX_LAG 64" in txt and "#define T2S_EVAL_MDD_BINS 50" in txt


def test_driver_parser_accepts_the_four_names():
    import evaluation as ev
    args = ev.build_parser().parse_args(["--method_list", "MSE,MDD,ACD,SD,KD"])
    assert ev._methods(args.method_list) == ["MSE", "MDD", "ACD", "SD", "KD"]
    assert ev.build_parser().parse_args([]).method_list == "MSE,WAPE,MRR"
    for fn in (M.mdd, M.acd, M.sd, M.kd, M.feature_measures):
        with pytest.raises(L.T2SError, match="no CPU fallback"):
            fn(np.zeros((4, 8, 1), np.float32), np.zeros((4, 8, 1), np.float32), device="cpu")


# ------------------------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("case", range(len(G.CASES)))
def test_parity_with_the_reference_fixture(gold, dev, case):
    c = gold[case]
    values, detail = M.feature_measures(c["ori"], c["gen"], device=dev)
    singles = {"MDD": M.mdd(c["ori"], c["gen"], device=dev)[0], "ACD": M.acd(c["ori"], c["gen"], device=dev)[0],
               "SD": M.sd(c["ori"], c["gen"], device=dev)[0], "KD": M.kd(c["ori"], c["gen"], device=dev)[0]}
    for m in NAMES:
        print(m, values[m], c[m], abs(values[m] - c[m]) / c[m])
    for m in NAMES:
        assert values[m] == pytest.approx(c[m], rel=1e-5), m
        assert singles[m] == values[m], m
    st = detail["stats"]
    for s_idx, name in enumerate(("ori", "gen")):
        np.testing.assert_allclose(st["acf"][s_idx].numpy().T, c[f"acf_{name}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(st["skew"][s_idx].numpy(), c[f"skew_{name}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(st["kurt"][s_idx].numpy(), c[f"kurt_{name}"], rtol=1e-5, atol=1e-6)
    per = detail["per_column"].numpy()                                          # (L, n_series)
    assert per.shape == c["ori"].shape[1:] and per.size == c["mdd_cols"].size
    print("per-column max rel", float(np.max(np.abs(per.T.reshape(-1) - c["mdd_cols"]) / c["mdd_cols"])))
    np.testing.assert_allclose(per.T.reshape(-1), c["mdd_cols"], rtol=1e-5)


@gpu
def test_identical_sets_give_exact_zeros(gold, dev):
    for c in gold:
        values, detail = M.feature_measures(c["ori"], c["ori"], device=dev)
        assert values == {"MDD": 0.0, "ACD": 0.0, "SD": 0.0, "KD": 0.0}
        assert float(detail["per_column"].abs().max()) == 0.0


@gpu
def test_common_row_permutation_changes_nothing(gold, dev):
    c = gold[1]
    perm = np.random.RandomState(5).permutation(c["ori"].shape[0])
    v0, d0 = M.feature_measures(c["ori"], c["gen"], device=dev)
    v1, d1 = M.feature_measures(c["ori"][perm], c["gen"][perm], device=dev)
    for m in ("ACD", "SD", "KD"):
        assert v1[m] == pytest.approx(v0[m], rel=1e-6), m
    assert v1["MDD"] == v0["MDD"] and torch.equal(d0["per_column"], d1["per_column"])    # integer counts: bit-identical


@gpu
def test_constant_real_column_is_finite(gold, dev):
    """histogram_torch's `b = a + 1e-5` rule.  Finiteness only: every fake value at the same constant sits exactly on
    the strict `> 0` boundary of the reference's counter, so parity on such a column is ill-posed."""
    ori, gen = gold[1]["ori"].copy(), gold[1]["gen"].copy()
    ori[:, 3, 1] = 0.5
    gen[:, 3, 1] = 0.5
    gen[0, 3, 1] = 0.7
    value, per = M.mdd(ori, gen, device=dev)
    assert np.isfinite(value) and bool(torch.isfinite(per).all())


@gpu
def test_sample_split_is_exact_and_repeatable(big, dev):
    ori, gen, want, want_cols = big
    v0, d0 = M.feature_measures(ori, gen, device=dev)
    v1, d1 = M.feature_measures(ori, gen, device=dev)
    for m in NAMES:
        print(m, v0[m], want[m], abs(v0[m] - want[m]) / want[m])
    for m in NAMES:
        assert v0[m] == pytest.approx(want[m], rel=1e-5), m
    np.testing.assert_allclose(d0["per_column"].numpy(), want_cols, rtol=1e-5)
    st = np_stats(ori)
    np.testing.assert_allclose(d0["stats"]["acf"][0].numpy(), st["acf"], rtol=1e-5, atol=1e-6)
    assert v0 == v1 and torch.equal(d0["per_column"], d1["per_column"])
    for key in d0["stats"]:
        assert torch.equal(d0["stats"][key], d1["stats"][key]), key


@gpu
def test_longest_series_and_fewest_samples(dev):
    """L = 4096 (the bound: a whole centred series in LDS, 64 column tiles) with n = 3 and two channels."""
    ori, gen, _ = G.snapped_sets(3, 4096, 2, 78)
    want = np_measures(ori, gen)
    values, detail = M.feature_measures(ori, gen, device=dev)
    for m in NAMES:
        print(m, values[m], want[m], abs(values[m] - want[m]) / want[m])
    for m in NAMES:
        assert values[m] == pytest.approx(want[m], rel=1e-5), m
    np.testing.assert_allclose(detail["per_column"].numpy(), np_mdd_columns(ori, gen), rtol=1e-5)


@gpu
def test_refusals(dev):
    x = np.random.RandomState(1).rand(4, 8, 1).astype(np.float32)
    for fn in (M.mdd, M.acd, M.feature_measures):
        with pytest.raises(L.T2SError, match="n=1"):
            fn(x[:1], x[:1], device=dev)
        with pytest.raises(L.T2SError, match="L=4097"):
            fn(np.zeros((2, 4097, 1), np.float32), np.zeros((2, 4097, 1), np.float32), device=dev)
        with pytest.raises(L.T2SError, match="expected two"):
            fn(x, x[:, :7], device=dev)
        with pytest.raises(L.T2SError, match="no CPU fallback"):
            fn(x, x, device="cpu")
    a = torch.from_numpy(x).to(dev)
    need = L.lib().t2s_eval_features_workspace_bytes(4, 8, 1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((3,), -7.0, device=dev)
    for entry in ("t2s_eval_moments", "t2s_eval_mdd"):
        with pytest.raises(L.T2SError, match="workspace"):
            L.check(getattr(L.lib(), entry)(a.data_ptr(), a.data_ptr(), None, out.data_ptr(), 4, 8, 1, ws.data_ptr(), need - 1,
                                            L.stream_ptr(dev)), entry)
        with pytest.raises(L.T2SError, match="workspace"):
            L.check(getattr(L.lib(), entry)(a.data_ptr(), a.data_ptr(), None, out.data_ptr(), 4, 8, 1, None, need,
                                            L.stream_ptr(dev)), entry)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7.0, -7.0, -7.0]                               # nothing was launched


@gpu
def test_evaluation_driver_writes_the_four_keys(gold, dev, tmp_path, monkeypatch):
    import glob
    import evaluation as ev
    monkeypatch.chdir(tmp_path)
    c = gold[1]
    save = str(tmp_path / "results")
    name = "flowmatching_DiT_ETTh1_70_9.0_10"
    g = os.path.join(save, "generation", name)
    for r in range(10):
        os.makedirs(os.path.join(g, f"run_{r}"))
        np.save(os.path.join(g, f"run_{r}", "x_1.npy"), c["ori"])
        np.save(os.path.join(g, f"run_{r}", "x_t.npy"), c["gen"])
    np.save(os.path.join(g, "x_t.npy"), c["gen"])
    single, _ = ev.main(["--dataset_name", "ETTh1_70", "--save_path", save, "--method_list", "MSE,MDD,ACD,SD,KD"])
    values, _ = M.feature_measures(c["ori"], c["gen"], device=dev)
    assert set(single) == {"MSE", "MDD", "ACD", "SD", "KD"}
    assert {m: single[m] for m in NAMES} == values
    assert single["MSE"] == M.mse_wape(c["ori"], c["gen"])[0]
    files = sorted(glob.glob(os.path.join(save, "evaluation", name, f"{name}_ETTh1_70_*.json")))
    assert json.load(open(files[0])) == single
    only_mse, _ = ev.main(["--dataset_name", "ETTh1_70", "--save_path", save, "--method_list", "MSE"])
    assert only_mse == {"MSE": single["MSE"]}
