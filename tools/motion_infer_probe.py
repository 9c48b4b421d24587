#!/usr/bin/env python3
"""Measure the motion-inference job of myinfer.py against the reference-style loop it replaces, on one GPU, in one process.

Workload: 64 synthetic bench-press clips (10 channels, latent width 64 = 1024 tokens, lengths drawn once from 30..160 with a
fixed seed), 100-step flow matching, cfg 3, synthetic weights.
  side A  one ragged job: ONE Sampler run over the 64 rows, the final decode at a length per row (Sampler.run(lengths=...));
  side B  the reference-style loop on the same build: one Sampler run per clip at batch 1 and the clip's own length (one
          Sampler per distinct length, built and warmed before any timed round) -- the only form without per-row lengths.
Both sides key row i's noise by the clip's index, so their outputs must agree bit for bit per clip; the probe checks that and
fails otherwise.  Sides alternate A, B, A, B, ... for `--rounds` rounds after one warm-up round of each; a round is timed with a
host clock around work that ends in a device synchronise.  Reported: the median of the rounds and the max - min spread.

Also: the ragged decode alone (t2s_vae_decode_mc_ragged, one launch over the lengths of tests/test_ragged_codec.py) against the
same rows as one uniform t2s_vae_decode_mc call each, `--decode_reps` repetitions per timed window, alternating likewise.

    python tools/motion_infer_probe.py --out profiles/motion_infer.json
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from t2ms_amd import synth                      # noqa: E402
from t2ms_amd.sampler import Sampler            # noqa: E402

DECODE_LENGTHS = [8, 11, 36, 41, 128, 131, 132, 203]


def stats(xs):
    return dict(median_s=float(np.median(xs)), spread_s=float(max(xs) - min(xs)), rounds_s=[float(x) for x in xs])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cfg", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode_reps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "motion_infer.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("motion_infer_probe.py: no GPU visible -- nothing is measured without one")
    from model.denoiser.mytransformer import Transformer
    from model.pretrained.myvqvae import vqvae
    dev = torch.device("cuda:0")
    C, W, N = 10, 64, a.clips
    model = Transformer(W)
    model.load_state_dict(synth.make_dit_state_dict(a.seed, width=W), strict=True)
    vae = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256, embedding_dim=64,
                                      flow_dim=W, input_dim=C))
    vae.load_state_dict(synth.make_mvae_state_dict(a.seed, C, 128, 3, 256), strict=True)
    model, dec = model.to(dev).eval(), vae.to(dev).eval().decoder
    lengths = [int(n) for n in np.random.RandomState(a.seed).randint(30, 161, size=N)]
    text = synth.make_text_embeddings(a.seed, N).to(dev)

    ragged = Sampler(model, dec, "flowmatching", a.steps, a.cfg, N, max(lengths), dev, seed=a.seed)
    ragged.set_rows(seeds=[a.seed] * N, key_rows=list(range(N)))
    singles = {n: Sampler(model, dec, "flowmatching", a.steps, a.cfg, 1, n, dev, seed=a.seed) for n in sorted(set(lengths))}

    def side_a():
        return ragged.run(text, lengths=lengths)[1]

    def side_b():
        rows = []
        for i, n in enumerate(lengths):
            s = singles[n]
            s.set_rows(seeds=[a.seed], key_rows=[i])
            rows.append(s.run(text[i:i + 1])[1][0])
        return rows

    with torch.no_grad():
        (_, rows_a), (_, rows_b) = timed(side_a), timed(side_b)          # warm-up: graphs captured, every shape run once
        equal = all(torch.equal(x, y) for x, y in zip(rows_a, rows_b))
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(side_a)[0])
            tb.append(timed(side_b)[0])

        # the decode alone, at the lengths of the codec test
        z = synth.make_wide_latents(a.seed, len(DECODE_LENGTHS), W).to(dev)

        def dec_a():
            for _ in range(a.decode_reps):
                rows = dec.decode_ragged(z, DECODE_LENGTHS)
            return rows

        def dec_b():
            for _ in range(a.decode_reps):
                rows = [dec(z[b:b + 1], n)[0][0] for b, n in enumerate(DECODE_LENGTHS)]
            return rows

        (_, d_a), (_, d_b) = timed(dec_a), timed(dec_b)
        dec_equal = all(torch.equal(x, y) for x, y in zip(d_a, d_b))
        da, db = [], []
        for _ in range(a.rounds):
            da.append(timed(dec_a)[0] / a.decode_reps)
            db.append(timed(dec_b)[0] / a.decode_reps)

    A, B, DA, DB = stats(ta), stats(tb), stats(da), stats(db)
    gain = B["median_s"] - A["median_s"]
    result = dict(
        device=torch.cuda.get_device_name(0),
        workload=dict(clips=N, channels=C, latent_w=W, steps=a.steps, cfg=a.cfg, backbone="flowmatching", math=ragged.math,
                      lengths=lengths, seed=a.seed, rounds=a.rounds, distinct_lengths=len(singles)),
        ragged_job=A, per_clip_loop=B, outputs_bit_equal=bool(equal),
        speedup_median=B["median_s"] / A["median_s"],
        faster_by_more_than_the_spread=bool(gain > max(A["spread_s"], B["spread_s"])),
        clips_per_s=dict(ragged_job=N / A["median_s"], per_clip_loop=N / B["median_s"]),
        decode_alone=dict(lengths=DECODE_LENGTHS, reps_per_window=a.decode_reps, ragged_one_launch=DA, uniform_calls=DB,
                          outputs_bit_equal=bool(dec_equal), speedup_median=DB["median_s"] / DA["median_s"],
                          note="seconds per pass over the 8 rows, host clock around a synchronised window; includes the "
                               "mirrors' host work (the ragged call stages its length tables each time)"),
        timing="host clock around work that ends in torch.cuda.synchronize(); sides alternate in one process after one warm-up each")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "workload"}, indent=1))
    if not (equal and dec_equal):
        sys.exit("motion_infer_probe.py: the two sides disagree")


if __name__ == "__main__":
    main()
