"""Rows of different runs, positions and guidance scales in ONE sampler launch (t2s_sampler_set_rows,
t2s_philox_normal_rows), and the grid job of infer.py built on it: every row must come out bit for bit as in a uniform
sampler / a separate invocation of its own."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, LEN = 4, 48
# three "cells" of unequal size: 5 + 3 + 6 = 14 rows, split 7 + 7 by two lanes (no cell boundary on the lane split)
CELLS = ((5, 11, 0, 5.0), (3, 12, 3, 9.0), (6, 11, 20, 7.5))        # (rows, seed, row0, cfg)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    import types
    from model.denoiser.transformer import Transformer
    from model.pretrained.vqvae import vqvae
    m = Transformer()
    m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True)
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    v.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    return m.to(dev).eval(), v.to(dev).eval()


def _cell_tables():
    seeds = np.concatenate([np.full(n, s, dtype=np.uint64) for n, s, _, _ in CELLS])
    keys = np.concatenate([r0 + np.arange(n) for n, _, r0, _ in CELLS]).astype(np.uint32)
    cfgs = np.concatenate([np.full(n, c, dtype=np.float32) for n, _, _, c in CELLS])
    return seeds, keys, cfgs


MODES = {"eager": dict(use_graph=False), "step_graph": dict(use_graph=True, loop_graph=0),
         "loop_graph": dict(use_graph=True, loop_graph=1)}


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_mixed_rows_equal_uniform_samplers_per_cell(dev, models, backbone, math, mode, lanes):
    from t2ms_amd.sampler import Sampler
    m, v = models
    B = sum(c[0] for c in CELLS)
    text = synth.make_text_embeddings(5, B).to(dev)
    mixed = Sampler(m, v.decoder, backbone, STEPS, 1.0, B, LEN, dev, seed=999, row0=77, lanes=lanes, math=math, **MODES[mode])
    mixed.set_rows(*_cell_tables())
    lat, ser, _ = mixed.run(text)
    if mode != "eager":
        assert mixed.graph_lanes == lanes
    r = 0
    for n, seed, row0, cfg in CELLS:
        ref = Sampler(m, v.decoder, backbone, STEPS, cfg, n, LEN, dev, seed=seed, row0=row0, lanes=1, math=math, **MODES[mode])
        la, sa, _ = ref.run(text[r:r + n].contiguous())
        assert torch.equal(lat[r:r + n], la), (backbone, math, mode, lanes, seed, row0, cfg)
        assert torch.equal(ser[r:r + n], sa), (backbone, math, mode, lanes, seed, row0, cfg)
        r += n


@pytest.mark.parametrize("backbone", ["ddpm", "flowmatching"])
def test_tables_holding_the_uniform_values_give_the_uniform_bits(dev, models, backbone):
    from t2ms_amd.sampler import Sampler
    m, v = models
    B, seed, row0, cfg = 12, 41, 9, 7.0
    text = synth.make_text_embeddings(6, B).to(dev)
    for lanes in (1, 2):
        uni = Sampler(m, v.decoder, backbone, STEPS, cfg, B, LEN, dev, seed=seed, row0=row0, lanes=lanes, math="f32")
        want = uni.run(text)
        tab = Sampler(m, v.decoder, backbone, STEPS, cfg, B, LEN, dev, seed=seed, row0=row0, lanes=lanes, math="f32")
        tab.set_rows(np.full(B, seed, dtype=np.uint64), row0 + np.arange(B), np.full(B, cfg))
        got = tab.run(text)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), lanes
        # each table on its own (the others uniform)
        for which in range(3):
            tables = [None, None, None]
            tables[which] = (np.full(B, seed, dtype=np.uint64), row0 + np.arange(B), np.full(B, cfg))[which]
            tab.set_rows(*tables)
            got = tab.run(text)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (lanes, which)


def test_updating_tables_keeps_the_graph_and_equals_a_fresh_sampler(dev, models):
    from t2ms_amd.sampler import Sampler
    m, v = models
    B = sum(c[0] for c in CELLS)
    text = synth.make_text_embeddings(7, B).to(dev)
    kw = dict(use_graph=True, lanes=2, loop_graph=1, math="f32")
    s = Sampler(m, v.decoder, "ddpm", STEPS, 6.0, B, LEN, dev, seed=5, row0=0, **kw)
    first = s.run(text)
    assert s.graph_lanes == 2
    ptr = s.ptr.value
    seeds, keys, cfgs = _cell_tables()
    for tables in ((seeds, keys, cfgs), (seeds[::-1].copy(), keys + 1000, cfgs * 2), (None, keys, None), (seeds, None, cfgs)):
        s.set_rows(*tables)
        got = s.run(text)
        assert s.graph_lanes == 2 and s.ptr.value == ptr
        fresh = Sampler(m, v.decoder, "ddpm", STEPS, 6.0, B, LEN, dev, seed=5, row0=0, **kw)
        fresh.set_rows(*tables)
        want = fresh.run(text)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(got[0], first[0])
    s.set_rows()                                                  # NULL everywhere: the uniform sampler again
    again = s.run(text)
    assert s.graph_lanes == 2
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # refused: wrong length, non-finite cfg, out-of-range keys -- and at the C ABI n != batch
    with pytest.raises(L.T2SError):
        s.set_rows(seeds=np.zeros(B + 1, dtype=np.uint64))
    with pytest.raises(L.T2SError):
        s.set_rows(cfg=np.full(B, np.nan))
    with pytest.raises(L.T2SError):
        s.set_rows(cfg=np.full(B, 1e39))
    with pytest.raises(L.T2SError):
        s.set_rows(key_rows=np.full(B, -1))
    bad = np.full(B, np.inf, dtype=np.float32)
    assert L.lib().t2s_sampler_set_rows(s.ptr, None, None, bad.ctypes.data, B) != 0
    assert L.lib().t2s_sampler_set_rows(s.ptr, None, None, None, B + 1) != 0
    assert torch.equal(s.run(text)[0], first[0])                  # a refused call changes nothing


def test_philox_normal_rows_equals_the_per_row_draw_and_the_oracle(dev):
    from t2ms_amd.sampler import XT_STREAM, philox_normal, philox_normal_rows
    seeds = np.array([2025, 7, 2025, (1 << 63) + 5, 0, 12345678901], dtype=np.uint64)
    keys = np.array([1000, 0, 3, 77, 2 ** 32 - 1, 5], dtype=np.uint32)
    for stream in (XT_STREAM, 0, 17):
        out = philox_normal_rows(seeds, keys, 1920, stream, dev)
        for r in range(len(seeds)):
            one = philox_normal(1, 1920, int(seeds[r]), stream, int(keys[r]), dev)
            assert torch.equal(out[r:r + 1], one), (stream, r)
            ref = O.device_normal(int(seeds[r]), stream, int(keys[r]), 1)
            assert float(np.abs(out[r:r + 1].cpu().numpy().astype(np.float64) - ref).max()) < 1e-5   # as test_philox_matches_oracle
    # row_elems other than the latent's
    out = philox_normal_rows(seeds[:2], keys[:2], 24, 3, dev)
    assert torch.equal(out[1:], philox_normal(1, 24, int(seeds[1]), 3, int(keys[1]), dev))


FILES = ("x_1.npy", "x_t.npy", "x_t_latent_dec_array.npy", "x_t_latent_enc_array.npy", "x_infer_trace.npy")


def _tree(root):
    return sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, "**", "*.npy"), recursive=True))


def test_driver_grid_writes_the_separate_invocations_files(dev, tmp_path, monkeypatch):
    """infer.main with 2 datasets x 2 cfg scales x (1 + 10) runs in ONE job, its launches mixing cells and runs, against the
    parent's main() loop replayed: per cell, infer(args) one run at a time, seed 3 + k, weights from seed 3."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    common = ["--backbone", "ddpm", "--total_step", "3", "--batch_size", "2", "--synthetic", "13", "--random_init",
              "--seed", "3", "--no_figs", "--trace"]
    grid = str(tmp_path / "grid")
    a = drv.main(["--dataset_name", "exchangerate_24,exchangerate_48", "--cfg_scale", "5,9", "--run_multi", "True",
                  "--launch_batch", "5", "--save_path", grid] + common)
    st = a.stats
    assert st["cells"] == 4 and st["runs"] == 11 and st["series"] == 4 * 11 * 12 and st["mixed_launches"] > 0
    for k in ("series", "loop_s", "launches", "series_per_launch_and_gpu", "loader_batch"):
        assert k in st
    assert a.math in ("f32", "bf16x3")
    one = str(tmp_path / "one")
    for name in ("exchangerate_24", "exchangerate_48"):
        for cfg in ("5", "9"):
            args = drv.build_parser().parse_args(["--dataset_name", name, "--cfg_scale", cfg, "--save_path", one] + common)
            args.mix_train = False
            args.device = "cuda:0"
            args.weight_seed = 3
            args.checkpoint_path = ""
            base = os.path.join(one, "generation", f"ddpm_DiT_{name}_{float(cfg)}_3")
            for k in range(11):
                args.seed = 3 + k
                args.cfg_scale = float(cfg)
                args.generation_save_path_result = base if k == 0 else os.path.join(base, f"run_{k - 1}")
                drv.infer(args)
    files = _tree(one)
    assert len(files) == 4 * 11 * len(FILES) and _tree(grid) == files
    for f in files:
        with open(os.path.join(one, f), "rb") as x, open(os.path.join(grid, f), "rb") as y:
            assert x.read() == y.read(), f


def _env(port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), T2S_DIST_BACKEND="gloo", T2S_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    return env


def test_two_rank_grid_writes_the_single_process_grids_files(tmp_path):
    """Two ranks on the one GPU (fresh children under torch.distributed.run, gloo, T2S_SHARE_GPU=1, as
    tests/test_two_ranks_one_gpu.py): launches mixing cells and runs, sharded over the ranks, one final gather."""
    argv = [os.path.join(REPO, "infer.py"), "--dataset_name", "exchangerate_24,exchangerate_48", "--cfg_scale", "5,9",
            "--run_multi", "True", "--backbone", "ddpm", "--total_step", "2", "--batch_size", "2", "--synthetic", "7",
            "--launch_batch", "3", "--random_init", "--seed", "4", "--no_figs"]
    runs = ((29591, [sys.executable], "one"),
            (29592, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                     "127.0.0.1", "--master-port", "29592"], "two"))
    for port, head, name in runs:
        r = subprocess.run(head + argv + ["--save_path", str(tmp_path / name)], env=_env(port), cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{name}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    files = _tree(tmp_path / "one")
    assert len(files) == 4 * 11 * 4 and _tree(tmp_path / "two") == files
    for f in files:
        with open(tmp_path / "one" / f, "rb") as x, open(tmp_path / "two" / f, "rb") as y:
            assert x.read() == y.read(), f


def _same_trees(a, b, n_files):
    files = _tree(a)
    assert len(files) == n_files and _tree(b) == files
    for f in files:
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            assert x.read() == y.read(), f


def test_a_flush_after_every_launch_writes_the_one_final_flushs_files(tmp_path, monkeypatch):
    """T2S_INFER_FLUSH_ROWS=1: the sink gathers and files after every launch instead of once at the end.  The grid of
    test_two_rank_grid_writes_the_single_process_grids_files (6 rows per unit, 3 per GPU and launch): 88 launches and
    flushes on one process; on two ranks every launch holds 6 rows, 3 per rank, so in every flush rank 0 files two ranks'
    rows by global row.  Both trees equal the default's (one flush at the end of the job)."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset_name", "exchangerate_24,exchangerate_48", "--cfg_scale", "5,9", "--run_multi", "True", "--backbone", "ddpm",
            "--total_step", "2", "--batch_size", "2", "--synthetic", "7", "--launch_batch", "3", "--random_init", "--seed", "4",
            "--no_figs"]
    monkeypatch.delenv("T2S_INFER_FLUSH_ROWS", raising=False)
    drv.main(argv + ["--save_path", str(tmp_path / "end")])
    monkeypatch.setenv("T2S_INFER_FLUSH_ROWS", "1")
    a = drv.main(argv + ["--save_path", str(tmp_path / "each")])
    assert a.stats["series"] == 4 * 11 * 6 and a.stats["launches"] == 88
    _same_trees(tmp_path / "end", tmp_path / "each", 4 * 11 * 4)
    monkeypatch.delenv("T2S_INFER_FLUSH_ROWS")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", "29594", os.path.join(REPO, "infer.py")] + argv +
                       ["--save_path", str(tmp_path / "two")], env=dict(_env(29594), T2S_INFER_FLUSH_ROWS="1"),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    _same_trees(tmp_path / "end", tmp_path / "two", 4 * 11 * 4)


def test_mlp_run_multi_in_one_job_writes_the_run_by_run_files(tmp_path, monkeypatch):
    """`--denoiser MLP --run_multi True` as the 11 units of ONE job (models built once) against infer(args) one run at a
    time, seed 3 + k, weights from seed 3, as the parent's main() looped."""
    import infer as drv
    monkeypatch.chdir(tmp_path)
    common = ["--denoiser", "MLP", "--backbone", "ddpm", "--dataset_name", "ETTh1_24", "--total_step", "3", "--batch_size", "4",
              "--synthetic", "9", "--random_init", "--seed", "3", "--no_figs"]
    job = str(tmp_path / "job")
    a = drv.main(common + ["--run_multi", "True", "--save_path", job])
    st = a.stats
    assert st["series"] == 11 * 8 and st["launches"] == 22 and st["loader_batch"] == 4 and st["series_per_launch_and_gpu"] == 4
    assert (st["cells"], st["runs"], st["mixed_launches"]) == (1, 11, 0)
    one = str(tmp_path / "one")
    args = drv.build_parser().parse_args(common + ["--save_path", one])
    args.mix_train = False
    args.device = "cuda:0"
    args.weight_seed = 3
    args.checkpoint_path = ""
    base = os.path.join(one, "generation", "ddpm_MLP_ETTh1_24_7_3")
    for k in range(11):
        args.seed = 3 + k
        args.generation_save_path_result = base if k == 0 else os.path.join(base, f"run_{k - 1}")
        drv.infer(args)
    _same_trees(one, job, 11 * 4)
