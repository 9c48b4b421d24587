"""Host logic of the grid job (infer.py --dataset_name A,B --cfg_scale x,y --run_multi True): the cells and their paths,
the loader order of every (dataset, seed), and the launch plan with its per-row (seed, key row, cfg).  CPU only."""
import os
import types

import numpy as np
import pytest
import torch

import infer as drv
from datafactory.dataloader import epoch_index_batches, loader_provider
from model.denoiser.mlp import MLP
from model.denoiser.transformer import Transformer
from model.pretrained.vqvae import vqvae
from t2ms_amd import dist as tdist


def _args(argv):
    a = drv.build_parser().parse_args(argv)
    a.mix_train = False
    return a


def _parent_dir(save, backbone, denoiser, name, cfg, steps):
    """The parent's directory formula (infer.py main): '{}_{}_{}_{}_{}'.format(..., args.cfg_scale, ...) with --cfg_scale
    parsed by argparse as type=float (the default 7 stays an int)."""
    return os.path.join(save, "generation", "{}_{}_{}_{}_{}".format(backbone, denoiser, name, cfg, steps))


def test_single_values_keep_todays_args_and_paths(tmp_path):
    save = str(tmp_path)
    cells = drv.parse_cells(_args(["--save_path", save]))
    assert len(cells) == 1 and cells[0].dataset_name == "exchangerate_24" and cells[0].cfg == 7.0
    assert cells[0].path == _parent_dir(save, "flowmatching", "DiT", "exchangerate_24", 7, 100)
    assert cells[0].path.endswith("_7_100")          # argparse's unconverted default
    for given, want in (("7", 7.0), ("7.0", 7.0), ("9", 9.0), ("12.5", 12.5), ("1e1", 10.0)):
        a = _args(["--save_path", save, "--dataset_name", "ETTh1_96", "--cfg_scale", given, "--backbone", "ddpm",
                   "--total_step", "1000"])
        (c,) = drv.parse_cells(a)
        assert c.cfg == want and c.dataset_name == "ETTh1_96"
        assert c.path == _parent_dir(save, "ddpm", "DiT", "ETTh1_96", float(given), 1000)
    assert drv.parse_cells(_args(["--save_path", save, "--cfg_scale", "7"]))[0].path.endswith("_7.0_100")


def test_lists_give_the_cells_in_order_with_the_separate_invocations_paths(tmp_path):
    save = str(tmp_path)
    a = _args(["--save_path", save, "--dataset_name", "ETTh1_24,ETTh1_48,ETTh1_96", "--cfg_scale", "9,5", "--total_step", "10"])
    cells = drv.parse_cells(a)
    want = [(n, c) for n in ("ETTh1_24", "ETTh1_48", "ETTh1_96") for c in (9.0, 5.0)]
    assert [(c.dataset_name, c.cfg) for c in cells] == want
    for c, (n, cfg) in zip(cells, want):
        assert c.path == _parent_dir(save, "flowmatching", "DiT", n, cfg, 10)
    units = drv.grid_units(cells, 11, 40)
    assert len(units) == 66
    for k, u in enumerate(units):
        c, r = cells[k // 11], k % 11
        assert (u.cell, u.run, u.seed, u.cfg, u.dataset_name) == (k // 11, r, 40 + r, c.cfg, c.dataset_name)
        assert u.path == (c.path if r == 0 else os.path.join(c.path, f"run_{r - 1}"))


@pytest.mark.parametrize("argv", [
    ["--dataset_name", "ETTh1_24,exchangerate_24"],                       # two roots
    ["--dataset_name", "ETTh1_24,ETTh1_48", "--denoiser", "MLP"],         # MLP with lists
    ["--cfg_scale", "5,7", "--denoiser", "MLP"],
    ["--cfg_scale", "5,x"], ["--cfg_scale", "5,,7"], ["--cfg_scale", ""], ["--cfg_scale", "nan"], ["--cfg_scale", "7,inf"],
    ["--cfg_scale=-inf"], ["--cfg_scale", "1e39"],                        # not finite in fp32
    ["--dataset_name", "ETTh1_24,"], ["--cfg_scale", "7,7.0"],            # empty entry, a cell twice
])
def test_refused_grids(argv, tmp_path):
    with pytest.raises(ValueError):
        drv.parse_cells(_args(["--save_path", str(tmp_path)] + argv))


def _literal_parent_order(args, name, seed, denoiser=Transformer):
    """The parent's infer() up to the order, replayed literally: manual_seed, loader_provider, the model constructors
    of _load_models (the LA-VAE's, then the denoiser's), epoch_index_batches."""
    torch.manual_seed(seed)
    a = types.SimpleNamespace(**vars(args))
    a.dataset_name, a.seed = name, seed
    _, loader = loader_provider(a, period="test")
    if args.random_init:
        vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    denoiser()
    return epoch_index_batches(loader), torch.get_rng_state()


@pytest.mark.parametrize("random_init", [True, False])
def test_loader_order_replays_the_parents_generator_sequence(random_init):
    argv = ["--synthetic", "13", "--batch_size", "2"] + (["--random_init"] if random_init else [])
    args = _args(argv)
    S = 3
    drv._DRAWS_AFTER.clear()
    for name in ("exchangerate_24", "ETTh1_48", "ETTh1_96"):
        for seed in range(S, S + 11):
            want, state = _literal_parent_order(args, name, seed)
            ds, got = drv.loader_order(args, name, seed)
            assert len(ds) == 13
            assert torch.equal(got, want), (name, seed)
            assert torch.equal(torch.get_rng_state(), state), (name, seed)
    # the MLP job takes the same path, its own constructor in the Transformer's place: the same order as a run that builds
    # the MLP where the parent's did
    mlp = _args(argv + ["--denoiser", "MLP"])
    want, state = _literal_parent_order(mlp, "ETTh1_24", 7, denoiser=MLP)
    for _ in range(2):                                  # the constructors' draws themselves, then their replay from the cache
        _, got = drv.loader_order(mlp, "ETTh1_24", 7)
        assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)


def _tables_1x1(n_rows, seed, cfg, B, launch_batch, world):
    """What the 1x1 path keys row i of a unit by: its own launches, its own rows only."""
    per_row = {}
    for s0, s1 in drv.grid_plan([n_rows], B, launch_batch, world):
        for rank in range(world):
            lo, hi = tdist.shard_rows(s1 - s0, rank, world)
            if hi > lo:
                segs = drv.launch_segments([n_rows], s0 + lo, s0 + hi)
                s, k, c = drv.row_tables(segs, [seed], [cfg])
                for j, i in enumerate(range(s0 + lo, s0 + hi)):
                    per_row[i] = (int(s[j]), int(k[j]), float(c[j]))
    return per_row


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("launch_batch", [0, 1, 4, 5, 256])
def test_launch_plan_covers_every_row_once_with_its_own_keys(world, launch_batch):
    B = 2
    cells = [types.SimpleNamespace(dataset_name=n, cfg=c, path=f"/x/{n}_{c}") for n, c in
             (("ETTh1_24", 5.0), ("ETTh1_24", 9.0), ("ETTh1_48", 12.5))]
    units = drv.grid_units(cells, 3, 100)
    unit_rows = [12 if u.cell < 2 else 6 for u in units]            # unequal cells; every unit a multiple of B
    seeds, cfgs = [u.seed for u in units], [u.cfg for u in units]
    plan = drv.grid_plan(unit_rows, B, launch_batch, world)
    assert plan[0][0] == 0 and plan[-1][1] == sum(unit_rows)
    assert all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    seen = {}
    mixed = 0
    for s0, s1 in plan:
        assert 0 < s1 - s0 <= (launch_batch * world if launch_batch > 0 else B)
        if launch_batch <= 0:
            assert len(drv.launch_segments(unit_rows, s0, s1)) == 1          # one loader batch of one unit
        mixed += len(drv.launch_segments(unit_rows, s0, s1)) > 1
        for rank in range(world):
            lo, hi = tdist.shard_rows(s1 - s0, rank, world)
            if hi <= lo:
                continue
            segs = drv.launch_segments(unit_rows, s0 + lo, s0 + hi)
            assert sum(i1 - i0 for _, i0, i1 in segs) == hi - lo
            s, k, c = drv.row_tables(segs, seeds, cfgs)
            assert s.dtype == np.uint64 and k.dtype == np.uint32 and c.dtype == np.float32 and len(s) == hi - lo
            j = 0
            for u, i0, i1 in segs:
                for i in range(i0, i1):
                    assert (u, i) not in seen
                    seen[(u, i)] = (int(s[j]), int(k[j]), float(c[j]))
                    j += 1
    assert len(seen) == sum(unit_rows)
    if launch_batch <= 0 or launch_batch == 1 and world == 1:
        assert mixed == 0
    elif launch_batch * world in (5, 8, 10, 15, 40, 256, 512, 768, 2048):      # sizes that do not divide 6 and 12
        assert mixed > 0
    for u, unit in enumerate(units):
        one = _tables_1x1(unit_rows[u], unit.seed, unit.cfg, B, launch_batch, world)
        assert {i: seen[(u, i)] for i in range(unit_rows[u])} == one
        assert all(v == (unit.seed, i, unit.cfg) for i, v in one.items())
    # launch_batch 0: exactly the parent's per-unit launch shape
    if launch_batch <= 0:
        off = 0
        want = []
        for n in unit_rows:
            want += [(off + a, off + b) for a, b in drv.launch_plan(n, B, 0, world)]
            off += n
        assert plan == want
