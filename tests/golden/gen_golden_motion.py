#!/usr/bin/env python3
"""Fixture of the motion measures (correlational score, sequence correlation, DTW of unequal lengths), made by RUNNING THE
REFERENCE's evaluate/metrics.py on seeded arrays (see gen_golden.py for the rules: the reference never travels, only the
arrays written here are committed).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_motion.py --reference <checkout of the reference>

Writes motion_metrics.npz.  Every input is a seeded fp32 array rounded to a 1/1024 grid and handed to the reference as an
fp64 copy (its own __main__, :290-370, feeds these functions fp64 arrays read from text): every input is exact in both
precisions and the reference's arithmetic is fp64 throughout.
  shift case k of SHIFT_CASES = (n, La, Lb, S, planted shifts): `sa_k` (n, La, S), `sb_k` (n, Lb, S), `sla_k` / `slb_k` (n)
    int32 lengths (RAGGED gives those of the one ragged case, the others use the full lengths), and what
    sequence_correlation(a_i[:la], b_i[:lb]) returns per pair: `sbest_k` (n) and `sdist_k` (n).  a is a sum of sines,
    series j of pair i scaled by 1 + 0.5 i + 0.25 j, and b[t + k] = a[t] + 0.02 noise for the planted shift k.
  correlation case k of CORR_CASES = (shape of ori, shape of gen, constant channel of gen or None): `co_k`, `cg_k`, and
    calculate_correlation_matrix of each (`cmo_k`, `cmg_k`) and calculate_correlational_score (`cs_k`).
  DTW case k of DTW_CASES = (m, n): `da_k` (m, 3), `db_k` (n, 3) and calculate_dtw(da, db) (`dtw_k`)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = 1024.0
SHIFT_CASES = ((4, 70, 70, 7, (0, 5, -9, 20)), (4, 130, 97, 10, (3, -17, 40, -2)), (3, 64, 65, 1, (1, -1, 7)),
               (3, 9, 8, 3, (0, 2, -3)))
RAGGED = {1: ((130, 101, 130, 77), (97, 97, 64, 90))}         # per-pair lengths (len_a, len_b) of shift case 1
CORR_CASES = (((6, 40, 7), (6, 40, 7), None), ((3, 10, 5), (7, 4, 5), None), ((4, 12, 4), (4, 12, 4), 2))
DTW_CASES = ((40, 33), (33, 40), (1, 9), (9, 1), (13, 13))
DTW_SERIES = 3


def _grid(x):
    return (np.round(np.asarray(x) * GRID) / GRID).astype(np.float32)


def make_shift_case(k):
    """a (n, La, S), b (n, Lb, S) fp32 on the 1/1024 grid, lengths (n) int32 each."""
    n, La, Lb, S, shifts = SHIFT_CASES[k]
    rs = np.random.RandomState(6100 + k)
    w = rs.uniform(0.15, 0.9, (3, n, 1, S))
    ph = rs.uniform(0, 2 * np.pi, (3, n, 1, S))
    amp = np.array([0.5, 0.3, 0.2])[:, None, None, None]
    scale = 1.0 + 0.5 * np.arange(n)[:, None, None] + 0.25 * np.arange(S)[None, None, :]

    def f(t):                                        # t (n, T, 1): the pair's own time axis
        return scale * (amp * np.sin(w * t[None] + ph)).sum(axis=0)

    ta = np.broadcast_to(np.arange(La, dtype=np.float64)[None, :, None], (n, La, 1))
    tb = np.arange(Lb, dtype=np.float64)[None, :, None] - np.asarray(shifts, dtype=np.float64)[:, None, None]
    a = f(ta)
    b = f(tb) + 0.02 * rs.randn(n, Lb, S)
    la, lb = RAGGED.get(k, ((La,) * n, (Lb,) * n))
    return _grid(a), _grid(b), np.asarray(la, dtype=np.int32), np.asarray(lb, dtype=np.int32)


def make_corr_case(k):
    so, sg, const = CORR_CASES[k]
    rs = np.random.RandomState(6200 + k)
    S = so[-1]
    mix = rs.uniform(-1, 1, (S, S)) + np.eye(S)
    ori = rs.randn(*so[:-1], S) @ mix + 0.3 * np.arange(S)
    gen = rs.randn(*sg[:-1], S) @ (mix + 0.4 * rs.uniform(-1, 1, (S, S))) + 0.3 * np.arange(S)
    ori, gen = _grid(ori), _grid(gen)
    if const is not None:
        gen[..., const] = 0.625
    return ori, gen


def make_dtw_case(k):
    m, n = DTW_CASES[k]
    rs = np.random.RandomState(6300 + k)
    scale = 1.0 + 0.25 * np.arange(DTW_SERIES)
    a = scale * (0.5 + 0.4 * np.sin(0.3 * np.arange(m)[:, None] + rs.uniform(0, 6, DTW_SERIES)))
    b = scale * (0.5 + 0.4 * np.sin(0.3 * np.arange(n)[:, None] * m / max(n, 1) + rs.uniform(0, 6, DTW_SERIES))) + 0.1 * rs.randn(n, DTW_SERIES)
    return _grid(a), _grid(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ref = os.path.abspath(ap.parse_args().reference)
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    os.chdir(HERE)                                   # '' on sys.path must not resolve to a checkout of this project
    sys.path.insert(0, ref)
    import evaluate.metrics as E
    assert E.__file__.startswith(ref + os.sep), E.__file__
    out = {}
    for k, (n, La, Lb, S, shifts) in enumerate(SHIFT_CASES):
        a, b, la, lb = make_shift_case(k)
        res = [E.sequence_correlation(a[i, :la[i]].astype(np.float64), b[i, :lb[i]].astype(np.float64)) for i in range(n)]
        out.update({f"sa_{k}": a, f"sb_{k}": b, f"sla_{k}": la, f"slb_{k}": lb,
                    f"sbest_{k}": np.asarray([r[0] for r in res], dtype=np.int32), f"sdist_{k}": np.asarray([r[1] for r in res])})
        print(f"shift case {k} {(n, La, Lb, S)}: planted {shifts} found {[int(r[0]) for r in res]} dist {[round(float(r[1]), 5) for r in res]}")
    for k in range(len(CORR_CASES)):
        ori, gen = make_corr_case(k)
        o64, g64 = ori.astype(np.float64), gen.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update({f"co_{k}": ori, f"cg_{k}": gen, f"cmo_{k}": E.calculate_correlation_matrix(o64),
                        f"cmg_{k}": E.calculate_correlation_matrix(g64), f"cs_{k}": E.calculate_correlational_score(o64, g64)})
        print(f"correlation case {k} {CORR_CASES[k]}: score {out[f'cs_{k}']}")
    for k in range(len(DTW_CASES)):
        a, b = make_dtw_case(k)
        out.update({f"da_{k}": a, f"db_{k}": b, f"dtw_{k}": E.calculate_dtw(a.astype(np.float64), b.astype(np.float64))})
        print(f"DTW case {k} {DTW_CASES[k]}: {out[f'dtw_{k}']:.6f}")
    path = os.path.join(HERE, "motion_metrics.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"motion_metrics.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
