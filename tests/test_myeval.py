"""t2s_eval_runs (csrc/t2s_eval_runs.hip), its mirror t2ms_amd.metrics.motion_runs and the driver myevaluation.py against the
restatement tests/_myeval_ref.py, which tests/test_myeval_host.py pins to reference-made values on the CPU.  Needs a real
MI355X (`pytest -m gpu`).

Tolerances (u = 2^-24, the unit roundoff of fp32; errors are relative; an expected NaN, Inf or exact 0 must come out exactly).
  The normalised planes are fp32 and bit for bit numpy's.
  per_run: every sum is fp64 over those fp32 values and is rounded once to fp32 -> 2 u: the one rounding (at most 1 u relative)
    plus one u for the device's sqrt and another fp64 summation order (the derivation at the top of tests/test_eval_paired.py
    for ED / DTW).
  per_clip: the fp64 mean of the runs' fp32 values (all of one sign, so their relative errors do not amplify), rounded once
    more -> 3 u.  out: the fp64 mean of those clip means before their rounding, rounded once -> 3 u as well.
Against the reference-made fixture the bars are those the same reference functions are held to elsewhere: rtol 2e-6 for MSE /
WAPE / ED (test_eval_paired_host.py), rtol 1e-5 / atol 1e-6 for ACD / SD / KD (test_feature_metrics.py).
The measured worst errors are in profiles/myeval_errors.md; every check prints its own as a `MYEVALERR` line."""
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

import _myeval_ref as R
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 64
LENGTHS = (1, 8, 63, 64, 65, 127, 130, 200, 64)
U = R.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------------- helpers
def draw(seed, C, runs, lengths=LENGTHS):
    """x1 [K] (C, T_i) and runs [R][K]; channel c is scaled by 1 + 0.45 c and shifted by c, run r's noise grows with r: a value
    read at a wrong offset is off by far more than any tolerance."""
    rs = np.random.RandomState(seed)
    scale = (1.0 + 0.45 * np.arange(C))[:, None]
    x1 = [(scale * rs.uniform(0.1, 1.0, (C, T)) + np.arange(C)[:, None]).astype(np.float32) for T in lengths]
    xt = [[(x + 0.15 * (r + 1) * scale * rs.randn(*x.shape)).astype(np.float32) for x in x1] for r in range(runs)]
    return x1, xt


@functools.lru_cache(maxsize=None)
def batch(C, runs):
    """One drawn batch and its restatement, computed once and shared (never modified)."""
    x1, xt = draw(900 + 17 * C + runs, C, runs)
    return x1, xt, R.evaluate(x1, xt)


def raw(dev, x1, xt, lens=None, off=None, max_T=None, C=None, runs=None, null=None):
    """One call of the C entry on sentinel-filled outputs with GUARD floats after each -> dict(rc, msg, per_run (K, R, 4),
    per_clip (K, 4), out (4,), norm1 (N,), normt (R, N), guards = every guard float untouched, all arrays numpy)."""
    p1, pt, plens, poff, chans = M.pack_motion_runs(x1, xt)
    lens = plens if lens is None else np.asarray(lens, dtype=np.int32)
    off = poff if off is None else np.asarray(off, dtype=np.uint64)
    K, n_runs, N = len(lens), pt.shape[0], p1.shape[0]
    C = chans if C is None else C
    runs = n_runs if runs is None else runs
    sizes = (K * n_runs * 4, K * 4, 4, N, n_runs * N)
    starts = np.cumsum([0] + [s + GUARD for s in sizes])
    with torch.cuda.device(dev):
        buf = torch.full((int(starts[-1]),), SENTINEL, device=dev)
        d1, dt = torch.from_numpy(p1).to(dev), torch.from_numpy(pt).to(dev)
        dl, do = torch.from_numpy(lens).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
        ptrs = [d1.data_ptr(), dt.data_ptr(), dl.data_ptr(), do.data_ptr()] + [buf.data_ptr() + 4 * int(s) for s in starts[:-1]]
        if null is not None:
            ptrs[null] = None
        rc = L.lib().t2s_eval_runs(*ptrs, K, runs, C, int(lens.max()) if max_T is None else max_T, L.stream_ptr(dev))
        msg = L.lib().t2s_last_error().decode() if rc else ""
        host = buf.cpu().numpy()
    parts = [host[int(s):int(s) + n] for s, n in zip(starts[:-1], sizes)]
    guards = all((host[int(s) + n:int(s) + n + GUARD] == SENTINEL).all() for s, n in zip(starts[:-1], sizes))
    return dict(rc=rc, msg=msg, per_run=parts[0].reshape(K, n_runs, 4), per_clip=parts[1].reshape(K, 4), out=parts[2],
                norm1=parts[3], normt=parts[4].reshape(n_runs, N), guards=guards, off=off, C=chans)


def planes(res, i):
    """Clip i's normalised planes out of a raw() result: (C, T_i) and (R, C, T_i)."""
    C, lo, hi = res["C"], res["C"] * int(res["off"][i]), res["C"] * int(res["off"][i + 1])
    return res["norm1"][lo:hi].reshape(C, -1), res["normt"][:, lo:hi].reshape(res["normt"].shape[0], C, -1)


def check(what, shape, got, want, bound):
    err = R.worst(got, want) / U
    print(f"MYEVALERR {what} shape={shape} worst={err:.3f}u bound={bound}u")
    assert err <= bound, (what, shape, err, bound)


def check_against(res, ref, shape, clips=None):
    """A raw() result against a restatement (R.evaluate's tuple) on the clips listed (all by default)."""
    summary, per_clip, per_run, norm1, normt = ref
    assert res["rc"] == 0 and res["guards"], res["msg"]
    for k, i in enumerate(range(len(norm1)) if clips is None else clips):
        n1, nt = planes(res, i)
        assert R.same_bits(n1, norm1[k]) and R.same_bits(nt, normt[k]), (shape, i)
    rows = slice(None) if clips is None else list(clips)
    for m, name in enumerate(R.NAMES):
        check(f"per_run {name}", shape, res["per_run"][rows][..., m], per_run[..., m], 2)
        check(f"per_clip {name}", shape, res["per_clip"][rows][:, m], per_clip[:, m], 3)
        check(f"out {name}", shape, res["out"][m], summary[m], 3)


# ------------------------------------------------------------------------------------------- the entry against the restatement
@pytest.mark.parametrize("runs", [1, 3, 10])
@pytest.mark.parametrize("C", [1, 7, 16])
def test_entry_against_restatement(dev, C, runs):
    x1, xt, ref = batch(C, runs)
    res = raw(dev, x1, xt)
    check_against(res, ref, (len(LENGTHS), runs, C))
    assert np.isnan(res["per_clip"][0, 1]) and np.isnan(res["out"][1])        # the one-step clip: every normalised value is 0
    # without that clip WAPE's summary is a number
    res = raw(dev, x1[1:], [run[1:] for run in xt])
    check_against(res, (ref[1][1:].mean(axis=0), ref[1][1:], ref[2][1:], ref[3][1:], ref[4][1:]), (len(LENGTHS) - 1, runs, C))
    assert np.isfinite(res["out"]).all()


# ----------------------------------------------------------------------------------------------------- bitwise properties
same = R.same_bits            # bit for bit; NaNs by position


def test_a_repeat_call_is_bit_equal(dev):
    x1, xt, _ = batch(7, 3)
    a, b = raw(dev, x1, xt), raw(dev, x1, xt)
    for key in ("per_run", "per_clip", "out", "norm1", "normt"):
        assert same(a[key], b[key]), key


def test_each_clip_alone_equals_its_row_of_the_batch(dev):
    x1, xt, _ = batch(7, 3)
    whole = raw(dev, x1, xt)
    for i in range(len(x1)):
        one = raw(dev, [x1[i]], [[run[i]] for run in xt])
        assert one["rc"] == 0 and one["guards"]
        assert same(one["per_run"][0], whole["per_run"][i]) and same(one["per_clip"][0], whole["per_clip"][i]), i
        assert same(one["per_clip"][0], one["out"])                          # the mean over one clip
        n1, nt = planes(whole, i)
        assert same(one["norm1"], n1.reshape(-1)) and same(one["normt"], nt.reshape(3, -1)), i


def test_permuting_the_clips_permutes_the_rows(dev):
    x1, xt, _ = batch(7, 3)
    whole = raw(dev, x1, xt)
    order = [4, 0, 8, 2, 7, 1, 6, 3, 5]
    moved = raw(dev, [x1[i] for i in order], [[run[i] for i in order] for run in xt])
    for k, i in enumerate(order):
        assert same(moved["per_run"][k], whole["per_run"][i]) and same(moved["per_clip"][k], whole["per_clip"][i]), (k, i)
        assert all(same(p, q) for p, q in zip(planes(moved, k), planes(whole, i)))


def test_adding_runs_leaves_the_earlier_runs_unchanged(dev):
    x1, xt, _ = batch(7, 10)
    many, few = raw(dev, x1, xt), raw(dev, x1, xt[:3])
    assert few["rc"] == 0 and same(many["per_run"][:, :3], few["per_run"])
    assert same(many["normt"][:3], few["normt"]) and same(many["norm1"], few["norm1"])


# ----------------------------------------------------------------------------------------------------------------- edges
def test_constant_rows_and_constant_runs(dev):
    x1, xt = draw(41, 7, 3)
    x1, xt = [x.copy() for x in x1], [[x.copy() for x in run] for run in xt]
    x1[2][4] = 1.5                                        # a constant recording channel
    xt[1][3][0] = -2.0                                    # a constant channel in one sample
    xt[0][5][:] = np.arange(7, dtype=np.float32)[:, None]  # every channel of one run constant: its WAPE is NaN
    for run in xt:                                        # ... and of all runs: the clip's WAPE is NaN
        run[6][:] = 3.0
    ref = R.evaluate(x1, xt)
    assert np.isnan(ref[2][5, 0, 1]) and np.isfinite(ref[1][5, 1]) and np.isnan(ref[1][6, 1])
    res = raw(dev, x1, xt)
    check_against(res, ref, (9, 3, 7))
    assert (planes(res, 2)[0][4] == 0).all() and (planes(res, 3)[1][1, 0] == 0).all()
    assert np.isnan(res["per_run"][5, 0, 1]) and np.isfinite(res["per_clip"][5, 1]) and np.isnan(res["per_clip"][6, 1])
    # a sample that is its recording: exact zeros
    xt[2][4] = x1[4].copy()
    res = raw(dev, x1, xt)
    assert (res["per_run"][4, 2] == 0).all()


def test_zeros_of_both_signs_normalise_to_plus_zero_in_any_order(dev):
    """The one stated exception to 'numpy's bits' (t2s_eval_runs.h): a row whose minimum is zero and holds -0 and +0.  The
    entry orders the zeros, so lo = -0 and every zero of the row comes out +0 wherever the two signs sit; all other values are
    numpy's bits, whichever zero numpy took for lo."""
    rs = np.random.RandomState(9)
    base = rs.uniform(0.5, 2.0, (3, 70)).astype(np.float32)
    outs = []
    for neg, pos in (((0, 5), (1, 3)), ((1, 3), (0, 5)), ((69,), (0,)), ((0,), (69,))):
        x = base.copy()
        x[1, list(neg)], x[1, list(pos)] = -0.0, 0.0
        res = raw(dev, [x], [[x.copy()]])
        assert res["rc"] == 0 and res["guards"]
        n1, nt = planes(res, 0)
        zeros = sorted(neg + pos)
        assert (n1[1, zeros] == 0).all() and not np.signbit(n1[1, zeros]).any() and same(n1, nt[0])
        want = R.normalize(x)
        keep = np.ones(70, bool)
        keep[zeros] = False
        assert same(n1[[0, 2]], want[[0, 2]]) and same(n1[1, keep], want[1, keep])
        assert (res["per_run"][0, 0, [0, 2, 3]] == 0).all()              # the sample is the recording
        outs.append(np.delete(n1[1], [0, 1, 3, 5, 69]))                  # the columns no placement puts a zero in
    assert all(same(o, outs[0]) for o in outs[1:])


def test_nan_and_inf_stay_in_their_clip(dev):
    x1, xt, _ = batch(7, 3)
    clean = raw(dev, x1, xt)
    y1, yt = [x.copy() for x in x1], [[x.copy() for x in run] for run in xt]
    yt[1][2][3, 40] = np.nan                              # clip 2 (63 steps), run 1, channel 3
    y1[5][0, 100] = np.inf                                # clip 5 (127 steps), the recording's channel 0
    yt[2][7][6, 5] = -np.inf                              # clip 7 (200 steps), run 2, channel 6
    ref = R.evaluate(y1, yt)
    res = raw(dev, y1, yt)
    check_against(res, ref, (9, 3, 7))
    n1, nt = planes(res, 2)
    assert np.isnan(nt[1, 3]).all() and np.isfinite(np.delete(nt[1], 3, axis=0)).all() and np.isfinite(nt[[0, 2]]).all()
    assert np.isnan(res["per_run"][2, 1]).all() and np.isfinite(res["per_run"][2, [0, 2]]).all()
    assert np.isfinite(res["per_clip"][2, 1])              # the nanmean skips the NaN run
    n1, _ = planes(res, 5)
    assert np.isnan(n1[0, 100]) and (np.delete(n1[0], 100) == 0).all()         # finite / inf = 0, inf / inf = NaN
    assert np.isnan(res["per_run"][5]).all()
    assert np.isnan(planes(res, 7)[1][2, 6]).all()          # x - (-inf) = inf everywhere, inf / inf
    for i in (0, 1, 3, 4, 6, 8):
        assert same(res["per_run"][i], clean["per_run"][i]) and same(res["per_clip"][i], clean["per_clip"][i]), i
        assert all(same(p, q) for p, q in zip(planes(res, i), planes(clean, i)))


def test_skipped_rows_are_untouched(dev):
    """Storage of lengths (8, 63, 200, 65, 130); the call says (8, 0, 200, 64, 130) with max_T = 130: clip 1 is empty, clip 2 is
    longer than max_T, clip 3's offsets span 65 steps, not 64.  Clips 0 and 4 come out as alone, everything else stays."""
    stored = (8, 63, 200, 65, 130)
    x1, xt = draw(77, 7, 3, stored)
    res = raw(dev, x1, xt, lens=[8, 0, 200, 64, 130], max_T=130)
    assert res["rc"] == 0 and res["guards"], res["msg"]
    keep = [0, 4]
    ref = R.evaluate([x1[i] for i in keep], [[run[i] for i in keep] for run in xt])
    check_against(res, ref, (5, 3, 7), clips=keep)
    for i in (1, 2, 3):
        assert (res["per_run"][i] == SENTINEL).all() and (res["per_clip"][i] == SENTINEL).all(), i
        assert all((p == SENTINEL).all() for p in planes(res, i)), i
    for i in keep:
        one = raw(dev, [x1[i]], [[run[i]] for run in xt])
        assert same(one["per_run"][0], res["per_run"][i]) and same(one["per_clip"][0], res["per_clip"][i])
    # nothing evaluated at all: out is NaN, nothing else is written
    res = raw(dev, x1, xt, lens=[0, 0, 0, 0, 0], max_T=130)
    assert res["rc"] == 0 and res["guards"] and np.isnan(res["out"]).all()
    assert all((res[k] == SENTINEL).all() for k in ("per_run", "per_clip", "norm1", "normt"))


def test_refusals(dev):
    x1, xt = draw(5, 7, 3, (8, 63))
    for kwargs, needle in ((dict(C=17), "channels=17"), (dict(max_T=4097), "max_T=4097"), (dict(runs=0), "runs=0"),
                           (dict(null=0), "NULL"), (dict(null=3), "NULL"), (dict(null=4), "NULL"), (dict(null=8), "NULL")):
        res = raw(dev, x1, xt, **kwargs)
        assert res["rc"] == -1 and res["msg"].startswith("t2s_eval_runs:") and needle in res["msg"], (kwargs, res["msg"])
        assert res["guards"] and all((res[k] == SENTINEL).all() for k in ("per_run", "per_clip", "out", "norm1", "normt"))
    with pytest.raises(L.T2SError, match="C=17"):
        M.motion_runs([np.zeros((17, 8), np.float32)], [[np.zeros((17, 8), np.float32)]], device=dev)


# ------------------------------------------------------------------------------------------ the mirror against the fixture
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "myeval.npz"))


def golden_case(golden, k, K, runs):
    x1 = [golden[f"x1_{k}_{i}"] for i in range(K)]
    return x1, [[golden[f"xt_{k}_{i}"][r] for i in range(K)] for r in range(runs)]


@pytest.mark.parametrize("k,K,runs", [(0, 5, 3), (1, 2, 10)])
def test_mirror_against_the_reference_fixture(dev, golden, k, K, runs):
    x1, xt = golden_case(golden, k, K, runs)
    summary, per_clip, per_run, norm1, normt = M.motion_runs(x1, xt, device=dev, detail=True)
    assert per_clip.shape == (K, 4) and per_run.shape == (K, runs, 4) and list(summary) == list(R.NAMES)
    want = golden[f"ref_{k}"]
    for i in range(K):
        assert norm1[i].is_cuda and normt[i].shape == (runs,) + x1[i].shape
        assert R.same_bits(norm1[i].cpu().numpy(), golden[f"n1_{k}_{i}"]) and R.same_bits(normt[i].cpu().numpy(), golden[f"nt_{k}_{i}"])
        assert R.worst(per_run[i, :, :3].numpy(), golden[f"runs_{k}_{i}"]) <= 2e-6
    err = R.worst(per_clip[:, :3].numpy(), want[:, :3])
    print(f"MYEVALERR mirror vs reference case={k} worst={err:.3e} bound=2e-6")
    assert err <= 2e-6
    assert R.worst([summary[m] for m in R.NAMES[:3]], want[:, :3].mean(axis=0)) <= 2e-6
    again = M.motion_runs(x1, xt, device=dev)
    assert len(again) == 3 and same(again[1].numpy(), per_clip.numpy()) and again[0] == summary


@pytest.mark.parametrize("k,K,runs", [(0, 5, 3), (1, 2, 10)])
def test_feature_measures_through_the_drivers_path(dev, golden, k, K, runs):
    import myevaluation as E
    x1, xt = golden_case(golden, k, K, runs)
    args = E.get_args(["--method_list", "MSE,ACD,SD,KD,DTW"])
    result = E.evaluate(args, list(range(K)), x1, xt, dev)
    assert list(result) == list(range(K)) + ["summary"] and list(result[0]) == ["MSE", "ACD", "SD", "KD", "DTW"]
    got = np.array([[result[s][m] for m in ("ACD", "SD", "KD")] for s in range(K)])
    np.testing.assert_allclose(got, golden[f"ref_{k}"][:, 3:6], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose([result["summary"][m] for m in ("ACD", "SD", "KD")], golden[f"ref_{k}"][:, 3:6].mean(axis=0), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------ end to end
def latest_json(save, name):
    d = os.path.join(save, "evaluation", name)
    files = sorted(os.listdir(d))
    assert len(files) == 1, files
    return json.load(open(os.path.join(d, files[0])))


@pytest.fixture(scope="module")
def sampled(dev, tmp_path_factory):
    """myinfer.py --save_eval_files once: five synthetic clips, three runs, two steps."""
    import myinfer
    save = str(tmp_path_factory.mktemp("myeval"))
    myinfer.main(["--dataset_name", "deadlift", "--random_init", "--synthetic", "5", "--run_time", "3", "--total_step", "2",
                  "--save_eval_files", "--save_path", save])
    return save


def test_end_to_end_both_layouts(dev, sampled, tmp_path):
    import myevaluation as E
    name = "flowmatching_DiT_deadlift_3_2"
    g = os.path.join(sampled, "generation", name)
    flags = ["--dataset_name", "deadlift", "--total_step", "2", "--run_time", "3", "--clips", "0", "--method_list", "MSE,WAPE,ED,DTW,ACD,SD,KD"]
    E.main(flags + ["--save_path", sampled])
    got = latest_json(sampled, name)
    assert list(got) == ["0", "1", "2", "3", "4", "summary"] and list(got["0"]) == ["MSE", "WAPE", "ED", "ACD", "SD", "KD", "DTW"]
    # the restatement on the files the reference's myevaluation.py would read
    x1 = [np.load(os.path.join(g, f"x_1_sample_{s}.npy")) for s in range(5)]
    xt = [[np.load(os.path.join(g, f"run_{j}", f"x_t_sample_{s}.npy")) for s in range(5)] for j in range(3)]
    assert all(np.array_equal(xt[j][s], np.load(os.path.join(g, f"run_{j}", f"sample_{s}", "x_t.npy"))) for j in range(3) for s in range(5))
    summary, per_clip, _, norm1, normt = R.evaluate(x1, xt)
    for m, metric in enumerate(R.NAMES):
        check(f"driver {metric}", (5, 3, 7), [got[str(s)][metric] for s in range(5)], per_clip[:, m], 3)
        check(f"driver summary {metric}", (5, 3, 7), [got["summary"][metric]], [summary[m]], 3)
    feats = np.array([R.feature_measures(normt[s], np.broadcast_to(norm1[s], normt[s].shape)) for s in range(5)])
    np.testing.assert_allclose([[got[str(s)][m] for m in ("ACD", "SD", "KD")] for s in range(5)], feats, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose([got["summary"][m] for m in ("ACD", "SD", "KD")], feats.mean(axis=0), rtol=1e-5, atol=1e-6)
    # the same samples through the sample_<s>/x_t.npy layout, the recordings from the synthetic set: the same table
    other = str(tmp_path)
    for j in range(3):
        for s in range(5):
            os.makedirs(os.path.join(other, "generation", name, f"run_{j}", f"sample_{s}"))
            shutil.copy(os.path.join(g, f"run_{j}", f"sample_{s}", "x_t.npy"), os.path.join(other, "generation", name, f"run_{j}", f"sample_{s}", "x_t.npy"))
    E.main(flags + ["--save_path", other, "--synthetic", "5"])
    assert latest_json(other, name) == got


def test_cfid_on_one_clip(dev, sampled, tmp_path):
    import myevaluation as E
    name = "flowmatching_DiT_deadlift_3_2"
    shutil.copytree(os.path.join(sampled, "generation", name), os.path.join(str(tmp_path), "generation", name))
    result, path = E.main(["--dataset_name", "deadlift", "--total_step", "2", "--run_time", "3", "--clips", "1", "--method_list", "C-FID",
                           "--cfid_engine", "hip", "--save_path", str(tmp_path)])
    assert list(result) == [0, "summary"] and list(result[0]) == ["C-FID"] and os.path.exists(path)
    assert np.isfinite(result[0]["C-FID"]) and result["summary"]["C-FID"] == result[0]["C-FID"]
