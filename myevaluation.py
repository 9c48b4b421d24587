#!/usr/bin/env python3
"""Drop-in for the reference's myevaluation.py: score the `run_<j>` directories myinfer.py wrote for a T2MS motion dataset
(bench press / deadlift) and write the reference's JSON table -- with every clip of every run scored in ONE launch sequence.

    python myevaluation.py --dataset_name benchpress --cfg_scale 3 --total_step 100 --run_time 10
    python myevaluation.py --dataset_name deadlift --synthetic 64 --run_time 3 --clips 0 --method_list MSE,WAPE,ED,DTW,ACD,SD,KD

Per clip s the reference stacks the clip's `run_time` samples, min-max normalises every channel of the samples and of the
recording, and calls evaluate_data(ori = the normalised SAMPLES, gen = the normalised recording repeated), both
(run_time, C, T_s).  Its metric functions read axis 1 as time and axis 2 as series, so on these arrays the channel axis plays
time and the T_s steps play the series; the swap is the reference's and is kept, because its numbers are what a table made here
is compared with (t2s_eval_runs.h spells the resulting formulas out).  Clips have their own lengths, so there is no rectangular
array for the paired entries of evaluation.py: MSE / WAPE / ED / DTW of all clips and runs come from one
t2ms_amd.metrics.motion_runs call (t2s_eval_runs: three launches over the packed ragged layout, one download).  ACD / SD / KD
run per clip on the existing feature kernels over the normalised planes that call leaves on the device (they compare two SETS,
so they need --run_time >= 2), C-FID per clip through the existing TS2Vec fit / encode (`--cfid_engine` as in evaluation.py).

Kept from the reference: the flags, `{save_path}/generation/{backbone}_{denoiser}_{dataset}_{cfg_scale}_{total_step}/` and
`{save_path}/evaluation/{model_name}/{model_name}_{dataset}_{time}.json`, the result keys (one dict per clip index, then
`summary` = the plain mean over the evaluated clips), the print lines.
What differs, on purpose:
  * input names: the reference reads `run_<j>/x_t_sample_<s>.npy` and `<generation>/x_1_sample_<s>.npy`, names its own
    myinfer.py never writes.  Both layouts are read here: those names when present (`myinfer.py --save_eval_files` writes
    them), else `run_<j>/sample_<s>/x_t.npy`, with the recordings taken from the dataset by the flags myinfer.py sampled with
    (`--synthetic`, `--split`, `--dataset_root`, ...).  A missing file or a recording whose shape is not its sample's ends the
    run with a message naming it.
  * `--clips N`: the reference scores `range(10)`; N = 0 scores every clip found.
  * `--cfg_scale` is a float as in the reference, and names the directory as myinfer.py does: an integral value prints
    without a fraction (`..._3_100`).  myinfer.py parses an int, so a fractional value names a directory only another
    sampler could have written; it is accepted for that case and otherwise ends in the missing-file message.
  * MRR and CRPS index `gen_data.shape[3]` on the 3-D arrays in the reference and raise IndexError there; they are refused here.
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from t2ms_amd import motion_cli                      # noqa: E402

PROG = "myevaluation.py"
METHODS = ("C-FID", "MSE", "WAPE", "ED", "ACD", "SD", "KD", "DTW")        # the order evaluate_data fills a clip's dict in
RUNS_METHODS = ("MSE", "WAPE", "ED", "DTW")                                # motion_runs' columns
REFUSED = ("MRR", "CRPS")


def methods_of(method_list):
    """The reference's parsing of --method_list, then what this driver cannot or will not compute."""
    names = method_list if isinstance(method_list, list) else [m.strip() for m in method_list.strip("[]").split(",")]
    names = [m for m in names if m]
    for m in names:
        if m in REFUSED:
            sys.exit(f"{PROG}: {m} is not available for motion runs: the reference indexes gen_data.shape[3] on its 3-D "
                     f"(run_time, C, T) arrays there and raises IndexError")
        if m not in METHODS:
            sys.exit(f"{PROG}: unknown metric {m!r} in --method_list (known: {', '.join(METHODS)})")
    if not names:
        sys.exit(f"{PROG}: --method_list names no metric")
    return names


def scale_text(v):
    """--cfg_scale as the generation directory spells it: myinfer.py parses an int."""
    return str(int(v)) if float(v) == int(v) else str(float(v))


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate the runs of a motion model (reference myevaluation.py)")
    # the reference's command line
    p.add_argument("--method_list", type=str, default="MSE,WAPE,DTW", help="metric list [MSE,WAPE,C-FID,ED,ACD,SD,KD,DTW]")
    p.add_argument("--save_path", type=str, default="./results/denoiser_results", help="root of generation/ and evaluation/")
    p.add_argument("--dataset_name", type=str, choices=["deadlift", "benchpress"], default="benchpress", help="dataset name")
    p.add_argument("--cfg_scale", type=float, default=3, help="CFG scale")
    p.add_argument("--total_step", type=int, default=100, help="sampling steps")
    p.add_argument("--run_time", type=int, default=10, help="number of runs (run_0 .. run_<N-1>)")
    motion_cli.add_config_flags(p)       # --config and config.yaml's values as flags (they name the paths)
    # this driver's own
    p.add_argument("--clips", type=int, default=10, help="score clips 0 .. N-1 (the reference: 10); 0 = every clip found")
    p.add_argument("--cfid_engine", choices=("torch", "hip"), default=None,
                   help="what trains the C-FID encoder: torch autograd or the fused HIP step (unset: T2S_TS2VEC_FIT, else torch)")
    p.add_argument("--synthetic", type=int, default=0, help="the --synthetic N myinfer.py sampled (recordings not on disk)")
    p.add_argument("--split", choices=["test", "train", "all"], default="test", help="the --split myinfer.py sampled")
    args = p.parse_args(argv)
    if args.run_time < 1:
        p.error("--run_time must be >= 1")
    if args.clips < 0:
        p.error("--clips must be >= 0")
    motion_cli.resolve(args, PROG)
    args.model_name = "{}_{}_{}_{}_{}".format(args.backbone, args.denoiser, args.dataset_name, scale_text(args.cfg_scale), args.total_step)
    args.generation_save_path = os.path.join(args.save_path, "generation", args.model_name)
    args.evaluation_save_path = os.path.join(args.save_path, "evaluation", args.model_name)
    return args


def sample_file(generation, run, s, must=True):
    """The file holding run `run`'s sample of clip s: the reference's name, else myinfer.py's."""
    names = (os.path.join(generation, f"run_{run}", f"x_t_sample_{s}.npy"), os.path.join(generation, f"run_{run}", f"sample_{s}", "x_t.npy"))
    for n in names:
        if os.path.exists(n):
            return n
    if must:
        sys.exit(f"{PROG}: run {run} has no sample of clip {s}: neither {names[0]} nor {names[1]} exists")
    return None


def clip_indices(generation, clips):
    """Clips 0 .. N-1, or with N = 0 every clip run_0 holds a sample of."""
    if clips > 0:
        return list(range(clips))
    s = 0
    while sample_file(generation, 0, s, must=False) is not None:
        s += 1
    if s == 0:
        sys.exit(f"{PROG}: no sample of clip 0 under {os.path.join(generation, 'run_0')}")
    return list(range(s))


def load_recordings(args, indices):
    """x_1 of every clip: `<generation>/x_1_sample_<s>.npy` where it exists, else the dataset's clips by myinfer.py's flags."""
    g = args.generation_save_path
    names = [os.path.join(g, f"x_1_sample_{s}.npy") for s in indices]
    have = [os.path.exists(n) for n in names]
    if all(have):
        return [np.load(n) for n in names]
    if any(have):
        sys.exit(f"{PROG}: {names[have.index(False)]} is missing while other x_1_sample files exist")
    import myinfer
    args.batch_size = 1                  # what the dataset's test loader is built with (myinfer.py's default); the clips do not depend on it
    clips = myinfer.load_clips(args)
    if indices[-1] >= len(clips):
        sys.exit(f"{PROG}: clip {indices[-1]} asked for, the {'synthetic set' if args.synthetic > 0 else args.split + ' split'} "
                 f"holds {len(clips)} (no {names[-1]} either)")
    return [clips[s][0].numpy() for s in indices]


def load_inputs(args):
    """(indices, x_1 [K] (C, T_s), x_t [R][K]) with every shape checked against its recording's."""
    g = args.generation_save_path
    indices = clip_indices(g, args.clips)
    runs = []
    for j in range(args.run_time):
        files = [sample_file(g, j, s) for s in indices]
        for f in files:
            print(f)
        runs.append([np.load(f) for f in files])
    x1 = load_recordings(args, indices)
    for k, s in enumerate(indices):
        if x1[k].ndim != 2:
            sys.exit(f"{PROG}: the recording of clip {s} is {x1[k].shape}, expected (C, T)")
        for j in range(args.run_time):
            if runs[j][k].shape != x1[k].shape:
                sys.exit(f"{PROG}: clip {s}: run {j}'s sample is {runs[j][k].shape}, the recording is {x1[k].shape}")
    return indices, x1, runs


def evaluate(args, indices, x1, runs, device):
    """result[s] = {metric: value} per clip, in the reference's key order, plus result['summary']."""
    from t2ms_amd import metrics as M
    methods = methods_of(args.method_list)
    R = len(runs)
    if R < 2 and any(m in methods for m in ("ACD", "SD", "KD", "C-FID")):
        sys.exit(f"{PROG}: ACD / SD / KD / C-FID compare two sets of samples and need --run_time >= 2 (got {R})")
    try:
        summary, per_clip, _, norm1, normt = M.motion_runs(x1, runs, device=device, detail=True)
    except M.L.T2SError as e:
        sys.exit(f"{PROG}: {e}")
    result = {}
    for k, s in enumerate(indices):
        print(f"ori_data shape:{tuple(normt[k].shape)}, gen_data shape:{tuple(normt[k].shape)}")
        row = {}
        ori, gen = normt[k], norm1[k].unsqueeze(0).expand_as(normt[k])      # (R, C, T_s): the reference's `ori` is the samples
        if "C-FID" in methods:
            from t2ms_amd.ts2vec import initialize_ts2vec
            o = ori.permute(0, 2, 1).contiguous().cpu().numpy()
            h = gen.permute(0, 2, 1).contiguous().cpu().numpy()
            model = initialize_ts2vec(o, device=device, engine=args.cfid_engine)
            row["C-FID"] = M.fid(model.encode(o, encoding_window="full_series"), model.encode(h, encoding_window="full_series"))
        for m in ("MSE", "WAPE", "ED"):
            if m in methods:
                row[m] = float(per_clip[k, RUNS_METHODS.index(m)])
        if any(m in methods for m in ("ACD", "SD", "KD")):
            (acd, sd, kd), _ = M._Features(ori, gen, device, "myevaluation").moments()
            row.update({m: v for m, v in (("ACD", acd), ("SD", sd), ("KD", kd)) if m in methods})
        if "DTW" in methods:
            row["DTW"] = float(per_clip[k, 3])
        result[s] = row
    result["summary"] = {m: summary[m] if m in RUNS_METHODS else float(np.mean([result[s][m] for s in indices]))
                         for m in result[indices[0]]}
    return result


def save(result, args):
    stamp = datetime.datetime.now().strftime("%Y%m%d-%H%M%S")
    path = os.path.join(args.evaluation_save_path, f"{args.model_name}_{args.dataset_name}_{stamp}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=4)
    print(f"Evaluation denoiser_results saved to {path}.")
    return path


def main(argv=None):
    args = get_args(argv)
    methods_of(args.method_list)                                             # refuse before anything is read
    if not torch.cuda.is_available():
        sys.exit(f"{PROG}: no GPU visible -- the metrics kernels run on the GPU (no CPU fallback)")
    device = torch.device(f"cuda:{torch.cuda.current_device()}")
    indices, x1, runs = load_inputs(args)
    result = evaluate(args, indices, x1, runs, device)
    path = save(result, args)
    print(f"Evaluation done. Results:{result}.")
    return result, path


if __name__ == "__main__":
    main()
