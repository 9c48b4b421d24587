"""The grid job against separate invocations: wall time and byte identity.

    python tools/grid_probe.py --parent DIR [--workloads W1,W2,W3,bench] [--repeats 3] [--out profiles/grid_sampling.json]

DIR is a tree of the parent commit (the one before the grid existed), built with its own build().  Per workload and
size, each repeat runs the parent's separate invocations -- one fresh process per (dataset, cfg) cell, as the authors'
scripts/script.sh does -- and this tree's ONE grid process, alternating which side goes first; every process is timed
(wall, including interpreter start; `python -c "import torch, t2ms_amd"` is timed too, to tell start-up from sampling).
All output files of the grid are compared with the parent's byte for byte.  Every child runs under `timeout`; the first
failing child stops the probe (no further GPU process is started) and what was measured so far is written.

  W1  the authors' ETTh1 line under the evaluation protocol: ETTh1_24,ETTh1_48,ETTh1_96, flowmatching, cfg 9, 10 steps,
      --run_multi True, N in {64, 256, 2048} synthetic test rows per dataset
  W2  a guidance sweep (script.sh:4): exchangerate_24, cfg 5,7,9,12, 100 steps, --run_multi True, N in {64, 256}
  W3  the 1x1 path at the shape of bench.py's infer_driver: exchangerate_24, cfg 7, 100 steps, N = 2048
  bench  `bench.py --gpus 1 --steps 3 --warmup 1` on both trees, alternating (the headline must not move)

A gain is claimed only where the grid's median wall time is below the parent's summed median by more than the larger of
the two run-to-run spreads (max - min over the repeats); otherwise "no measurable difference".
"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = {
    "W1": dict(datasets=["ETTh1_24", "ETTh1_48", "ETTh1_96"], cfgs=["9"], backbone="flowmatching", steps=10, run_multi=True,
               sizes=[64, 256, 2048]),
    "W2": dict(datasets=["exchangerate_24"], cfgs=["5", "7", "9", "12"], backbone="flowmatching", steps=100, run_multi=True,
               sizes=[64, 256]),
    "W3": dict(datasets=["exchangerate_24"], cfgs=["7"], backbone="flowmatching", steps=100, run_multi=False, sizes=[2048]),
}
SEED = 2025


class ChildFailed(RuntimeError):
    pass


def run(cmd, cwd, timeout):
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, cwd=cwd, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise ChildFailed(f"rc={r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return wall, r.stdout


def infer_argv(tree, datasets, cfgs, w, n, save):
    argv = [sys.executable, os.path.join(tree, "infer.py"), "--dataset_name", ",".join(datasets), "--cfg_scale", ",".join(cfgs),
            "--backbone", w["backbone"], "--total_step", str(w["steps"]), "--synthetic", str(n), "--random_init",
            "--seed", str(SEED), "--no_figs", "--save_path", save]
    return argv + (["--run_multi", "True"] if w["run_multi"] else [])


def files_of(root):
    return sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, "**", "*.npy"), recursive=True))


def same_bytes(a, b):
    fa, fb = files_of(a), files_of(b)
    if fa != fb:
        return False, len(fa), f"file sets differ: {sorted(set(fa) ^ set(fb))[:5]}"
    for f in fa:
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            if x.read() != y.read():
                return False, len(fa), f"{f} differs"
    return True, len(fa), ""


def summary(xs):
    return {"raw_s": [round(x, 3) for x in xs], "median_s": round(statistics.median(xs), 3), "spread_s": round(max(xs) - min(xs), 3)}


def probe_workload(name, w, parent, repeats, timeout):
    out = {"config": {k: v for k, v in w.items() if k != "sizes"}, "sizes": {}}
    for n in w["sizes"]:
        par, grid, ident = [], [], None
        for rep in range(repeats):
            tmp = tempfile.mkdtemp(prefix=f"grid_probe_{name}_{n}_")
            try:
                def parent_side():
                    walls = []
                    for d in w["datasets"]:
                        for c in w["cfgs"]:
                            walls.append(run(infer_argv(parent, [d], [c], w, n, os.path.join(tmp, "parent")), parent, timeout)[0])
                    return sum(walls)

                def grid_side():
                    return run(infer_argv(REPO, w["datasets"], w["cfgs"], w, n, os.path.join(tmp, "grid")), REPO, timeout)[0]
                if rep % 2 == 0:
                    par.append(parent_side())
                    grid.append(grid_side())
                else:
                    grid.append(grid_side())
                    par.append(parent_side())
                ok, n_files, why = same_bytes(os.path.join(tmp, "parent"), os.path.join(tmp, "grid"))
                if ident is None:
                    ident = {"identical": ok, "files_compared": n_files, "repeats_compared": 0}
                ident["identical"] = ident["identical"] and ok
                ident["repeats_compared"] += 1
                if not ok:
                    ident["why"] = why
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            print(f"{name} N={n} repeat {rep}: parent {par[-1]:.2f} s, grid {grid[-1]:.2f} s, identical {ident['identical']}",
                  flush=True)
        p, g = summary(par), summary(grid)
        margin = max(p["spread_s"], g["spread_s"])
        diff = p["median_s"] - g["median_s"]
        verdict = ("gain" if diff > margin else "loss" if -diff > margin else "no measurable difference")
        out["sizes"][str(n)] = {"parent_separate_processes": p, "grid_one_process": g, "byte_identity": ident,
                                "median_difference_s": round(diff, 3), "spread_margin_s": margin, "verdict": verdict,
                                # wall time: this tree's median must not exceed the parent's slowest repeat
                                "this_median_within_parent_spread_or_faster": g["median_s"] <= max(par)}
    return out


def probe_bench(parent, repeats, timeout):
    vals = {"parent": [], "this": []}
    for rep in range(repeats):
        for side in (("parent", "this") if rep % 2 == 0 else ("this", "parent")):
            tree = parent if side == "parent" else REPO
            _, stdout = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                            tree, timeout)
            line = [ln for ln in stdout.splitlines() if ln.startswith("{")][-1]
            vals[side].append(float(json.loads(line)["value"]))
            print(f"bench {side} repeat {rep}: {vals[side][-1]:.2f}", flush=True)
    res = {}
    for side, xs in vals.items():
        res[side] = {"raw": xs, "median": statistics.median(xs), "spread": max(xs) - min(xs)}
    # series/s: this tree's median must not fall below the parent's slowest repeat (within its spread, or faster)
    res["this_median_within_parent_spread_or_faster"] = res["this"]["median"] >= min(vals["parent"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", required=True, help="a built tree of the parent commit")
    ap.add_argument("--workloads", default="W1,W2,W3,bench")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grid_sampling.json"))
    ap.add_argument("--parent-commit", default=None, help="commit id of --parent (an exported tree carries none)")
    ap.add_argument("--this-commit", default=None, help="commit id of this tree, if it has none of its own")
    a = ap.parse_args(argv)
    parent = os.path.abspath(a.parent)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("workloads", {})
    res["protocol"] = ("per repeat: the parent's separate invocations (one fresh process per cell, wall times summed) and "
                       "this tree's one grid process, alternating which goes first; synthetic rows, --random_init, seed "
                       f"{SEED}; gain only where the grid median is below the parent median by more than the larger spread")

    def commit(tree):
        r = subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 else None
    res["this_commit"] = a.this_commit or commit(REPO) or res.get("this_commit")
    res["parent_commit"] = a.parent_commit or commit(parent) or res.get("parent_commit")
    try:
        for tree, key in ((parent, "parent"), (REPO, "this")):
            res.setdefault("import_s", {})[key] = summary(
                [run([sys.executable, "-c", "import torch, t2ms_amd"], tree, 120)[0] for _ in range(a.repeats)])
        for name in a.workloads.split(","):
            if name == "bench":
                res["bench_headline"] = probe_bench(parent, a.repeats, a.timeout)
            else:
                res["workloads"][name] = probe_workload(name, WORKLOADS[name], parent, a.repeats, a.timeout)
            json.dump(res, open(a.out, "w"), indent=1)
    except ChildFailed as e:
        res["stopped"] = str(e)[:4000]
        json.dump(res, open(a.out, "w"), indent=1)
        print(e, file=sys.stderr)
        return 1
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res)[:2000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
