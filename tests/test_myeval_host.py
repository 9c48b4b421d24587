"""Host side of the motion-run evaluation (no GPU): the restatement tests/_myeval_ref.py against the reference-made values of
tests/golden/myeval.npz (gen_golden_myeval.py), the extension header and its symbol table, the bars of tests/test_myeval.py
against deliberately damaged results, the mirror's host validation, and myevaluation.py's file handling."""
import ctypes as C
import glob
import json
import os
import re
import sys

import numpy as np
import pytest

import _eval_paired_ref as P
import _myeval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-6                                # the bar tests/test_eval_paired_host.py holds the same reference functions to
CASES = ((7, 3, (8, 63, 64, 65, 130)), (10, 10, (8, 65)))          # gen_golden_myeval.CASES


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "myeval.npz"))


def case(golden, k):
    C_, runs, lengths = CASES[k]
    x1 = [golden[f"x1_{k}_{i}"] for i in range(len(lengths))]
    xt = [golden[f"xt_{k}_{i}"] for i in range(len(lengths))]
    assert all(x.shape == (C_, T) for x, T in zip(x1, lengths)) and all(x.shape == (runs, C_, T) for x, T in zip(xt, lengths))
    return x1, xt, [[xt[i][r] for i in range(len(lengths))] for r in range(runs)]


# ---------------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("k", range(len(CASES)))
def test_restatement_reproduces_the_reference(golden, k):
    x1, xt, runs = case(golden, k)
    summary, clips, per_run, norm1, normt = R.evaluate(x1, runs)
    for i in range(len(x1)):
        assert R.same_bits(norm1[i], golden[f"n1_{k}_{i}"]) and R.same_bits(normt[i], golden[f"nt_{k}_{i}"])
        assert R.worst(per_run[i][:, :3], golden[f"runs_{k}_{i}"]) <= RTOL
    assert R.worst(clips[:, :3], golden[f"ref_{k}"][:, :3]) <= RTOL
    assert np.allclose(summary, clips.mean(axis=0), rtol=0, atol=0, equal_nan=True)
    assert np.isfinite(per_run[..., 3]).all() and (per_run[..., 3] >= 0).all()       # DTW: unpinned, but defined everywhere


def test_the_rows_with_a_purpose_are_in_the_fixture(golden):
    for k, (C_, runs, lengths) in enumerate(CASES):
        K = len(lengths)
        x1, xt, _ = case(golden, k)
        assert np.ptp(x1[0][2]) == 0 and (golden[f"n1_{k}_0"][2] == 0).all()                     # a constant recording channel
        assert np.ptp(xt[1 % K][1, 3]) == 0 and (golden[f"nt_{k}_{1 % K}"][1, 3] == 0).all()     # a constant sample channel
        copy = golden[f"runs_{k}_{2 % K}"][runs - 1]
        assert np.array_equal(xt[2 % K][runs - 1], x1[2 % K]) and (copy == 0).all()              # an exact copy: exact zeros
        flat = golden[f"runs_{k}_{3 % K}"]
        assert np.isnan(flat[0, 1]) and np.isfinite(flat[1:, 1]).all()                           # an all-constant run: WAPE NaN
        assert np.isfinite(golden[f"ref_{k}"]).all()                                             # ... which the nanmean skips


# ------------------------------------------------------------------------------------------ the header and its symbol table
def test_extension_header_and_its_symbol_table_agree():
    from t2ms_amd import _lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s_eval_runs.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(L.SYMBOLS_EVAL_RUNS) == {"t2s_eval_runs"}
    for other in (L.SYMBOLS, L.SYMBOLS_WIDE_TRAIN, L.SYMBOLS_WIDE_MATH, L.SYMBOLS_WIDE_TRAIN_BF16, L.SYMBOLS_TRAIN_ROWS):
        assert not declared & set(other)
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS_EVAL_RUNS["t2s_eval_runs"] == (I, [VP] * 9 + [I] * 4 + [VP])
    assert int(re.search(r"#define\s+T2S_EVAL_RUNS_MAX_CHANNELS\s+(\d+)", txt).group(1)) == L.EVAL_RUNS_MAX_CHANNELS == 16
    main = open(os.path.join(REPO, "include", "t2s.h")).read()
    assert "t2s_eval_runs" not in main
    fn = L.lib().t2s_eval_runs
    assert fn.restype is I and fn.argtypes == L.SYMBOLS_EVAL_RUNS["t2s_eval_runs"][1]


def test_the_entry_refuses_on_the_host_before_any_launch():
    """The refusals need no device: they come before the first launch."""
    from t2ms_amd import _lib as L
    lib = L.lib()
    p = 4096                                                         # any non-NULL address: never dereferenced on a refusal
    for args, needle in (((p,) * 9 + (1, 1, 17, 8), "channels=17"), ((p,) * 9 + (1, 1, 0, 8), "channels=0"),
                         ((p,) * 9 + (1, 1, 7, 4097), "max_T=4097"), ((p,) * 9 + (1, 0, 7, 8), "runs=0"),
                         ((p,) * 9 + (0, 1, 7, 8), "clips=0"), ((None,) + (p,) * 8 + (1, 1, 7, 8), "NULL"),
                         ((p,) * 8 + (None,) + (1, 1, 7, 8), "NULL")):
        assert lib.t2s_eval_runs(*args, None) == -1
        msg = lib.t2s_last_error().decode()
        assert msg.startswith("t2s_eval_runs:") and needle in msg, msg


# ------------------------------------------------------------------------------------- the bars reject damaged results
def test_the_bars_reject_damaged_results(golden):
    k = 0
    x1, xt, runs = case(golden, k)
    _, clips, per_run, norm1, normt = R.evaluate(x1, runs)
    i = 4                                                            # an ordinary clip (130 steps)
    a, b = normt[i], norm1[i]
    # a plane off by one ulp in one place
    bent = norm1[i].copy()
    bent[3, 17] = np.nextafter(bent[3, 17], np.float32(2))
    assert R.same_bits(norm1[i], norm1[i].copy()) and not R.same_bits(bent, norm1[i])
    # WAPE with the recording's denominator
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    wape_x1 = np.abs(a64 - b64).sum(axis=(1, 2)) / np.abs(b64).sum()
    assert R.worst(wape_x1, golden[f"runs_{k}_{i}"][:, 1]) > 1e3 * RTOL
    # ED taken over time instead of channels
    ed_time = np.sqrt(((a64 - b64) ** 2).sum(axis=2)).mean(axis=1)
    assert R.worst(ed_time, golden[f"runs_{k}_{i}"][:, 2]) > 1e3 * RTOL
    # DTW on the transposed sequences (T points of C dimensions): unpinned by the fixture, held to the restatement at 2 U
    g = np.broadcast_to(b, a.shape)
    dtw_t = P.dtw(np.transpose(a, (0, 2, 1)), np.transpose(g, (0, 2, 1)))
    assert R.worst(dtw_t, per_run[i][:, 3]) > 1e3 * 2 * R.U
    # a mean that counts the NaN run: as NaN, and as 0
    j = 3                                                            # the clip with the all-constant run
    w = per_run[j][:, 1]
    assert np.isnan(w[0]) and np.isnan(w.mean()) and np.isfinite(clips[j, 1])
    assert R.worst([np.nansum(w) / len(w)], [golden[f"ref_{k}"][j, 1]]) > 1e3 * RTOL
    assert R.worst([clips[j, 1]], [golden[f"ref_{k}"][j, 1]]) <= RTOL
    # and worst() itself: an expected exact 0 or NaN is not a tolerance matter
    with pytest.raises(AssertionError):
        R.worst([1e-30], [0.0])
    with pytest.raises(AssertionError):
        R.worst([0.5], [np.nan])
    assert R.worst([1.0 + 4 * R.U], [1.0]) > 3 * R.U > R.worst([1.0 + 2 * R.U], [1.0])


# ----------------------------------------------------------------------------------------------- the mirror's host side
def test_pack_motion_runs_layout_and_refusals():
    from t2ms_amd import metrics as M
    from t2ms_amd._lib import T2SError
    rs = np.random.RandomState(3)
    x1 = [rs.rand(3, T).astype(np.float32) for T in (5, 1, 9)]
    runs = [[rs.rand(*x.shape).astype(np.float32) for x in x1] for _ in range(2)]
    p1, pt, lens, off, chans = M.pack_motion_runs(x1, runs)
    assert chans == 3 and lens.dtype == np.int32 and off.dtype == np.uint64
    assert lens.tolist() == [5, 1, 9] and off.tolist() == [0, 5, 6, 15] and p1.shape == (45,) and pt.shape == (2, 45)
    for i in range(3):
        lo, hi = 3 * int(off[i]), 3 * int(off[i + 1])
        assert np.array_equal(p1[lo:hi].reshape(3, -1), x1[i]) and np.array_equal(pt[1, lo:hi].reshape(3, -1), runs[1][i])
    for bad_x1, bad_runs, needle in (
            ([], [], "no clip"), (x1, [], "no run"), (x1, [runs[0][:2]], "holds 2 clips"),
            (x1, [[runs[0][0], runs[0][1], runs[0][2][:, :8]]], "run 0 clip 2"),
            ([x1[0], rs.rand(4, 3).astype(np.float32)], [runs[0][:2]], "4 channels"),
            ([np.zeros((17, 4), np.float32)], [[np.zeros((17, 4), np.float32)]], "C=17"),
            ([np.zeros((2, 4097), np.float32)], [[np.zeros((2, 4097), np.float32)]], "T=4097"),
            ([np.zeros((2, 0), np.float32)], [[np.zeros((2, 0), np.float32)]], "T=0"),
            ([np.zeros(4, np.float32)], [[np.zeros(4, np.float32)]], "(C, T_i)")):
        with pytest.raises(T2SError, match=re.escape(needle)):
            M.pack_motion_runs(bad_x1, bad_runs)
    with pytest.raises(T2SError, match="GPU"):
        M.motion_runs(x1, runs, device="cpu")


# --------------------------------------------------------------------------------------------------------- the driver
def write_runs(root, name, x1, runs, layout, with_x1=True):
    g = os.path.join(root, "generation", name)
    for j, run in enumerate(runs):
        for s, x in enumerate(run):
            f = os.path.join(g, f"run_{j}", f"x_t_sample_{s}.npy") if layout == "reference" else os.path.join(g, f"run_{j}", f"sample_{s}", "x_t.npy")
            os.makedirs(os.path.dirname(f), exist_ok=True)
            np.save(f, x)
    if with_x1:
        for s, x in enumerate(x1):
            np.save(os.path.join(g, f"x_1_sample_{s}.npy"), x)
    return g


def driver_case(golden):
    x1, _, runs = case(golden, 0)
    return x1, runs


def test_driver_paths_and_names(tmp_path):
    import myevaluation as E
    a = E.get_args(["--dataset_name", "deadlift", "--cfg_scale", "3", "--total_step", "7", "--save_path", str(tmp_path)])
    assert a.model_name == "flowmatching_DiT_deadlift_3_7" and a.method_list == "MSE,WAPE,DTW" and a.run_time == 10 and a.clips == 10
    assert a.generation_save_path == os.path.join(str(tmp_path), "generation", a.model_name)
    assert a.evaluation_save_path == os.path.join(str(tmp_path), "evaluation", a.model_name)
    assert E.get_args(["--cfg_scale", "2.5"]).model_name == "flowmatching_DiT_benchpress_2.5_100"
    assert E.get_args([]).model_name == "flowmatching_DiT_benchpress_3_100"
    import myinfer
    b = myinfer.get_args(["--dataset_name", "deadlift", "--cfg_scale", "3", "--total_step", "7", "--save_path", str(tmp_path)])
    assert b.generation_save_path == a.generation_save_path and b.save_eval_files is False
    assert myinfer.get_args(["--dataset_name", "deadlift", "--save_eval_files"]).save_eval_files is True


@pytest.mark.parametrize("layout", ["reference", "myinfer"])
def test_driver_reads_both_layouts(golden, tmp_path, layout):
    import myevaluation as E
    x1, runs = driver_case(golden)
    a = E.get_args(["--dataset_name", "deadlift", "--run_time", "3", "--clips", "0", "--save_path", str(tmp_path)])
    g = write_runs(str(tmp_path), a.model_name, x1, runs, layout)
    assert g == a.generation_save_path
    indices, got1, got = E.load_inputs(a)
    assert indices == [0, 1, 2, 3, 4]
    assert all(np.array_equal(p, q) for p, q in zip(got1, x1))
    assert all(np.array_equal(got[j][s], runs[j][s]) for j in range(3) for s in range(5))
    # --clips N scores the first N; one past what is there names the missing file
    a.clips = 2
    assert E.load_inputs(a)[0] == [0, 1]
    a.clips = 6
    with pytest.raises(SystemExit, match=r"run 0 has no sample of clip 5.*x_t_sample_5\.npy.*sample_5"):
        E.load_inputs(a)
    a.clips, a.run_time = 0, 4
    with pytest.raises(SystemExit, match="run 3 has no sample of clip 0"):
        E.load_inputs(a)


def test_driver_mismatches_and_missing_recordings(golden, tmp_path):
    import myevaluation as E
    x1, runs = driver_case(golden)
    a = E.get_args(["--dataset_name", "deadlift", "--run_time", "3", "--clips", "0", "--save_path", str(tmp_path)])
    g = write_runs(str(tmp_path), a.model_name, x1, runs, "myinfer")
    np.save(os.path.join(g, "run_1", "sample_2", "x_t.npy"), runs[1][2][:, :-1])
    with pytest.raises(SystemExit, match=r"clip 2: run 1's sample is \(7, 63\), the recording is \(7, 64\)"):
        E.load_inputs(a)
    np.save(os.path.join(g, "run_1", "sample_2", "x_t.npy"), runs[1][2])
    os.remove(os.path.join(g, "x_1_sample_3.npy"))
    with pytest.raises(SystemExit, match=r"x_1_sample_3\.npy is missing"):
        E.load_inputs(a)
    for f in glob.glob(os.path.join(g, "x_1_sample_*.npy")):
        os.remove(f)
    # no recording on disk: the clips myinfer.py sampled, by the same flags
    b = E.get_args(["--dataset_name", "deadlift", "--run_time", "3", "--clips", "0", "--save_path", str(tmp_path), "--synthetic", "5"])
    import myinfer
    clips = myinfer.load_clips(b)
    with pytest.raises(SystemExit, match=r"clip 0: run 0's sample is \(7, 8\), the recording is \(7, \d+\)"):
        E.load_inputs(b)
    b.synthetic = 3
    with pytest.raises(SystemExit, match="clip 4 asked for, the synthetic set holds 3"):
        E.load_inputs(b)
    assert len(clips) == 5


def test_driver_refuses_mrr_and_crps():
    import myevaluation as E
    for m in ("MRR", "CRPS"):
        with pytest.raises(SystemExit, match=f"{m} is not available.*IndexError"):
            E.main(["--method_list", f"MSE,{m}"])
    with pytest.raises(SystemExit, match="unknown metric 'MDD'"):
        E.methods_of("MSE,MDD")
    assert E.methods_of("[MSE, WAPE,DTW]") == ["MSE", "WAPE", "DTW"]


def test_driver_json_shape(golden, tmp_path, monkeypatch, capsys):
    """evaluate() and save() with the one GPU call replaced by the restatement: the reference's keys, key order, summary, path."""
    import torch

    import myevaluation as E
    from t2ms_amd import metrics as M
    x1, runs = driver_case(golden)

    def fake(x1_list, xt_runs, device="cuda", detail=False):
        summary, clips, per_run, norm1, normt = R.evaluate(x1_list, xt_runs)
        return (dict(zip(R.NAMES, (float(np.float32(v)) for v in summary))), torch.from_numpy(clips.astype(np.float32)),
                torch.from_numpy(per_run.astype(np.float32)), [torch.from_numpy(v) for v in norm1], [torch.from_numpy(v) for v in normt])

    monkeypatch.setattr(M, "motion_runs", fake)
    a = E.get_args(["--dataset_name", "deadlift", "--run_time", "3", "--clips", "0", "--save_path", str(tmp_path), "--method_list", "DTW,MSE,WAPE"])
    write_runs(str(tmp_path), a.model_name, x1, runs, "reference")
    indices, got1, got = E.load_inputs(a)
    result = E.evaluate(a, indices, got1, got, "cpu")
    path = E.save(result, a)
    assert os.path.dirname(path) == a.evaluation_save_path
    assert re.fullmatch(re.escape(f"{a.model_name}_deadlift_") + r"\d{8}-\d{6}\.json", os.path.basename(path))
    assert f"saved to {path}." in capsys.readouterr().out
    back = json.load(open(path))
    assert list(back) == ["0", "1", "2", "3", "4", "summary"]
    for key in back:
        assert list(back[key]) == ["MSE", "WAPE", "DTW"]                  # the order evaluate_data fills them in
    want = golden["ref_0"]
    assert R.worst([back[str(s)]["MSE"] for s in range(5)], want[:, 0]) <= RTOL
    assert R.worst([back[str(s)]["WAPE"] for s in range(5)], want[:, 1]) <= RTOL
    for m in ("MSE", "WAPE", "DTW"):
        assert R.worst([back["summary"][m]], [np.mean([back[str(s)][m] for s in range(5)])]) <= RTOL
    # the feature measures need two samples per clip
    a.method_list, one = "MSE,ACD", [got[0]]
    with pytest.raises(SystemExit, match="--run_time >= 2"):
        E.evaluate(a, indices, got1, one, "cpu")


def test_driver_needs_a_gpu(monkeypatch, tmp_path):
    import torch

    import myevaluation as E
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible"):
        E.main(["--save_path", str(tmp_path)])


@pytest.mark.parametrize("k", range(len(CASES)))
def test_feature_restatement_reproduces_the_reference(golden, k):
    """R.feature_measures (what the end-to-end GPU test judges the driver's ACD / SD / KD by) at the bars of test_feature_metrics.py."""
    for i in range(len(CASES[k][2])):
        nt = golden[f"nt_{k}_{i}"]
        got = R.feature_measures(nt, np.broadcast_to(golden[f"n1_{k}_{i}"], nt.shape))
        np.testing.assert_allclose(got, golden[f"ref_{k}"][i, 3:6], rtol=1e-5, atol=1e-6)


def test_driver_takes_recordings_from_the_dataset(tmp_path):
    """No x_1_sample files, no --synthetic: the recordings are the clips of the dataset's split, as myinfer.py's default
    output needs them -- on the fixture dataset tests/golden/motion_ds, in the sample_<s>/x_t.npy layout, --split test."""
    import myevaluation as E
    import myinfer
    flags = ["--dataset_name", "benchpress", "--dataset_root", os.path.join(REPO, "tests", "golden", "motion_ds"), "--split", "test",
             "--run_time", "2", "--clips", "0", "--save_path", str(tmp_path)]
    want = myinfer.load_clips(myinfer.get_args(flags[:6] + ["--save_path", str(tmp_path)]))
    assert len(want) >= 2 and all(c[0].shape[0] == 10 for c in want)
    x1 = [c[0].numpy() for c in want]
    rs = np.random.RandomState(11)
    runs = [[(x + 0.1 * rs.randn(*x.shape)).astype(np.float32) for x in x1] for _ in range(2)]
    a = E.get_args(flags)
    assert not hasattr(a, "batch_size")
    write_runs(str(tmp_path), a.model_name, x1, runs, "myinfer", with_x1=False)
    indices, got1, got = E.load_inputs(a)
    assert indices == list(range(len(want)))
    assert all(np.array_equal(p, q) for p, q in zip(got1, x1))
    assert all(np.array_equal(got[j][s], runs[j][s]) for j in range(2) for s in indices)
    for split in ("train", "all"):                                                  # the other splits load too
        a.split, a.clips = split, 1
        b = myinfer.get_args(flags[:4] + ["--split", split, "--save_path", str(tmp_path)])
        assert np.array_equal(E.load_recordings(a, [0])[0], myinfer.load_clips(b)[0][0].numpy())
    a.split, a.clips = "test", len(want) + 1
    for j in range(2):
        f = os.path.join(a.generation_save_path, f"run_{j}", f"sample_{len(want)}", "x_t.npy")
        os.makedirs(os.path.dirname(f))
        np.save(f, runs[j][0])
    with pytest.raises(SystemExit, match=f"clip {len(want)} asked for, the test split holds {len(want)}"):
        E.load_inputs(a)
