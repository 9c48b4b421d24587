"""Per-row series lengths in the fused sampler (t2s_sampler_set_lengths, Sampler.run(lengths=...)) and the motion driver
myinfer.py on top of it.

Transformer(64) with a 3-channel decoder, 3 steps, cfg 7, batch 3, lengths [36, 41, 140] under a maximum of 140 (one-tile
rows, a resampled row and a tiled row in one decode).  Every criterion is a bit-equality: the latent against the same run
without lengths (the loop does not know them), every row against the decoder mirror's uniform decode of its latent row
(t2s_vae_decode_mc, held to the reference by tests/test_mvae.py).
"""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, MAX_L, B, W, CH, STEPS, CFG = [36, 41, 140], 140, 3, 64, 3, 3, 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def parts(dev):
    from model.denoiser.mytransformer import Transformer
    from model.pretrained.myvqvae import vqvae
    m = Transformer(W)
    m.load_state_dict(synth.make_dit_state_dict(2025, width=W), strict=True)
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64,
                                    flow_dim=W, input_dim=CH))
    v.load_state_dict(synth.make_mvae_state_dict(2025, CH, 128, 2, 256), strict=True)
    return (m.to(dev).eval(), v.to(dev).eval().decoder, synth.make_wide_latents(4, B, W).to(dev),
            synth.make_text_embeddings(4, B).to(dev))


def _check_rows(dec, lat, rows, lengths):
    assert isinstance(rows, list) and [tuple(r.shape) for r in rows] == [(CH, n) for n in lengths]
    with torch.no_grad():
        for b, n in enumerate(lengths):
            if n:
                assert torch.equal(rows[b], dec(lat[b:b + 1], n)[0][0]), (b, n)


@pytest.mark.parametrize("kw", [dict(backbone="flowmatching", use_graph=True, loop_graph=1),
                                dict(backbone="flowmatching", use_graph=True, loop_graph=0),
                                dict(backbone="flowmatching", use_graph=False),
                                dict(backbone="ddpm", use_graph=True, solver="ddim", steps=100, sample_steps=3)],
                         ids=["whole-loop-graph", "one-step-graph", "eager", "ddim"])
def test_ragged_run_is_the_uniform_latent_decoded_per_row(dev, parts, kw):
    from t2ms_amd.sampler import Sampler
    m, dec, xT, text = parts
    kw = dict(kw)
    s = Sampler(m, dec, kw.pop("backbone"), kw.pop("steps", STEPS), CFG, B, MAX_L, dev, **kw)
    lat_u, series_u, _ = s.run(text, x_T=xT)
    assert tuple(series_u.shape) == (B, CH, MAX_L)
    lat, rows, _ = s.run(text, x_T=xT, lengths=LENGTHS)
    assert torch.equal(lat, lat_u)                                # the loop does not know the lengths
    _check_rows(dec, lat, rows, LENGTHS)
    # views of ONE packed buffer, in row order
    assert all(rows[b + 1].data_ptr() == rows[b].data_ptr() + 4 * CH * LENGTHS[b] for b in range(B - 1))
    # an empty row and the maximum first; the trace decodes row 0 at its own length
    other = [140, 0, 8]
    lat_o, rows_o, tr = s.run(text, x_T=xT, lengths=other, trace=True)
    assert torch.equal(lat_o, lat_u) and tuple(tr.shape) == (s.steps, CH, 140)
    _check_rows(dec, lat_o, rows_o, other)
    assert torch.equal(tr[-1], rows_o[0])
    # run_inplace keeps the lengths of the last run; a run without lengths clears them (NULL): (B,C,L) again
    s.set_rows(seeds=[s.seed] * B, key_rows=list(range(B)))       # (x_T from Philox: only shapes and the decode are compared)
    lat_i, rows_i = s.run_inplace()
    _check_rows(dec, lat_i.clone(), [r.clone() for r in rows_i], other)
    lat_c, series_c, _ = s.run(text, x_T=xT)
    assert torch.equal(lat_c, lat_u) and torch.equal(series_c, series_u)


def test_refusals(dev, parts):
    from model.denoiser.transformer import Transformer as Transformer30
    from model.pretrained.vqvae import vqvae as vqvae1
    from t2ms_amd.sampler import Sampler
    m, dec, xT, text = parts
    s = Sampler(m, dec, "flowmatching", STEPS, CFG, B, MAX_L, dev, use_graph=False)
    lib = L.lib()

    def refused(lengths, n, *words):
        a = None if lengths is None else (C.c_int32 * len(lengths))(*lengths)
        rc = lib.t2s_sampler_set_lengths(s.ptr, a, n)
        msg = lib.t2s_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    refused([36, 41], 2, b"n=2", b"batch is 3")
    refused([36, 41, 141], 3, b"lengths[2]=141")
    refused([36, 5, 140], 3, b"lengths[1]=5")
    refused([36, -8, 140], 3, b"lengths[1]=-8")
    assert lib.t2s_sampler_set_lengths(None, None, 0) == -1
    # nothing was taken over: the sampler is still the uniform one
    lat, series, _ = s.run(text, x_T=xT)
    assert tuple(series.shape) == (B, CH, MAX_L)
    # the Python side refuses the same, before any library call
    for bad, word in (([36, 41], "2 lengths for 3 rows"), ([36, 41, 141], "lengths\\[2\\] = 141"), ([36, 5, 140], "lengths\\[1\\] = 5"),
                      ([36.0, 41, 140], "integers")):
        with pytest.raises(L.T2SError, match=word):
            s.run(text, x_T=xT, lengths=bad)
    # a single-channel decoder has no ragged decode: the library and the mirror both say so
    m30 = Transformer30()
    m30.load_state_dict(synth.make_dit_state_dict(31337), strict=True)
    v1 = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    v1.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    s1 = Sampler(m30.to(dev).eval(), v1.to(dev).eval().decoder, "flowmatching", STEPS, CFG, B, 96, dev, use_graph=False)
    a = (C.c_int32 * 3)(36, 40, 96)
    assert lib.t2s_sampler_set_lengths(s1.ptr, a, 3) == -1 and b"multichannel decoder" in lib.t2s_last_error()
    with pytest.raises(L.T2SError, match="multichannel decoder"):
        s1.run(synth.make_text_embeddings(1, B).to(dev), lengths=[36, 40, 96])
    # ... nor has a sampler without a decoder
    s0 = Sampler(m, None, "flowmatching", STEPS, CFG, B, MAX_L, dev, use_graph=False)
    assert lib.t2s_sampler_set_lengths(s0.ptr, (C.c_int32 * 3)(*LENGTHS), 3) == -1


def _myinfer(tmp_path, name, launch_batch):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(REPO, "myinfer.py"), "--dataset_name", "benchpress", "--random_init", "--total_step", "3",
           "--cfg_scale", "3", "--run_time", "1", "--launch_batch", str(launch_batch), "--save_path", str(out), "--split", "all",
           "--max_clips", "9", "--dataset_root", os.path.join(REPO, "tests", "golden", "motion_ds"), "--reconstruct"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out / "generation" / "flowmatching_DiT_benchpress_3_3" / "run_0"


def test_myinfer_synthetic_weights_on_the_fixture_dataset(tmp_path):
    """The driver on tests/golden/motion_ds/benchpress with synthetic weights (--random_init), the first 9 clips (20 .. 144
    samples: resampled, one-tile and tiled decodes): one x_t.npy (C, T_i), one data.json and one x_rec.npy per clip, a
    summary, and the same bits whether the clips ride in launches of 2 or of 8."""
    a = _myinfer(tmp_path, "lb2", 2)
    b = _myinfer(tmp_path, "lb8", 8)
    summary = json.load(open(a / "summary.json"))
    clips = summary["clips"]
    assert [c["length"] for c in clips] == [20, 36, 57, 58, 60, 77, 78, 90, 144] and summary["channels"] == 10
    assert summary["features"][0] == "left_shoulder_y" and len(summary["features"]) == 10
    assert sorted(os.listdir(a)) == sorted([f"sample_{i}" for i in range(9)] + ["summary.json"])
    for i, clip in enumerate(clips):
        d = a / f"sample_{i}"
        assert sorted(os.listdir(d)) == ["data.json", "x_rec.npy", "x_t.npy"]
        x = np.load(d / "x_t.npy")
        assert x.dtype == np.float32 and x.shape == (10, clip["length"]) and np.isfinite(x).all()
        data = json.load(open(d / "data.json"))
        assert list(data) == summary["features"] and all(len(v) == clip["length"] for v in data.values())
        assert np.array_equal(np.asarray(data[summary["features"][3]], dtype=np.float32), x[3])
        assert np.load(d / "x_rec.npy").shape == x.shape
        assert np.isfinite(clip["mse"]) and np.isfinite(clip["recon_mse"]) and clip["subject"] == "S01_correct"
        for f in ("x_t.npy", "x_rec.npy"):
            assert np.array_equal(np.load(d / f).view(np.int32), np.load(b / f"sample_{i}" / f).view(np.int32)), (i, f)
    assert clips == json.load(open(b / "summary.json"))["clips"]
