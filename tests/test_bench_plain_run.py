"""A plain `bench.py` run (no --full) on a small workload: it times exactly --steps batches, prints one result line
without the --full legs, and --dump-outputs writes what the timed path returned -- the same bits a Sampler built from
the bench's seeded models and inputs returns in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "roofline_rows", "kernel_breakdown_us", "strong", "strong_shards", "train", "config3", "config5",
             "alt_math", "cpu_baseline", "infer_driver", "train_driver", "class_api")


def test_plain_bench_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    B, steps, L = 64, 10, 96
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--diffusion-steps", str(steps), "--batch", str(B), "--dump-outputs", str(dump)]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "series/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] == pytest.approx(B / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in out], sorted(out)

    lat, series = np.load(dump / "latent.npy"), np.load(dump / "series.npy")
    assert lat.dtype == np.float32 and lat.shape == (B, 64, 30)
    assert series.dtype == np.float32 and series.shape == (B, L)

    import bench
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    dev = torch.device("cuda", 0)
    model, vae = bench.build_models(dev)
    s = Sampler(model, vae.decoder, "ddpm", steps, 9.0, B, L, dev, use_graph=True, seed=2025, row0=0)
    ref_lat, ref_series, _ = s.run(synth.make_text_embeddings(2025, B).to(dev), decode=True)
    np.testing.assert_array_equal(lat, ref_lat.cpu().numpy())
    np.testing.assert_array_equal(series, ref_series.cpu().numpy())
