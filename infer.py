#!/usr/bin/env python3
"""Drop-in sampling driver (reference infer.py): same flags, same checkpoint / output paths, same
four .npy files -- with the loop of infer.py:76-95 run by the fused HIP sampler.

    python infer.py --dataset_name ETTh1_96 --backbone ddpm --denoiser DiT --total_step 1000 --cfg_scale 9
    python -m torch.distributed.run --nproc-per-node 8 infer.py ...      # batch sharded over GPUs

Differences from the reference, all additive:
  * `--seed` (the reference never seeds, infer.py:15-25 is dead code) keys the on-device Philox
    noise stream; results do not depend on the number of GPUs;
  * `--synthetic N` / `--random_init` let the driver run without the (offline-unavailable) CSVs and
    trained checkpoints;
  * loader batches are coalesced: the reference samples one loader batch per launch (default
    `--batch_size 2`, a 4-sequence CFG pass); here the same rows in the same order go `--launch_batch`
    (256) per GPU at a time -- rows are independent and the kernels batch-invariant bit for bit, so
    the files do not change by a byte (`--launch_batch 0` = the reference's launch shape).  The test
    split, its embeddings and every output stay in HBM; the host touches no row inside the loop;
  * under torchrun every rank samples rows [lo,hi) of each launch and keeps them in HBM; the ranks
    meet in ONE gather at the end (a rank without rows joins empty-handed), rank 0 writes;
  * the per-step decode of the first batch (infer.py:90-93, GIF only) is `--trace`, off by default;
  * `--dataset_name` and `--cfg_scale` take comma-separated lists: ONE job samples the grid datasets x cfg scales (each
    with `--run_multi`'s 1 + 10 runs) and writes exactly the directories the separate invocations write.  The rows of
    every (cell, run) share the launches (per-row Philox key and guidance scale, t2s_sampler_set_rows).

  * `--solver {ancestral,ddim,dpmpp2m,euler,ab2}`, `--sample_steps S`, `--eta`: few-step solvers (no counterpart in
    the reference, sample quality on trained checkpoints not assessed).  The default follows the backbone and is the reference's
    run, byte for byte; `ddim` / `dpmpp2m` sample a `--total_step` DDPM checkpoint in S evaluations, `ab2` is a second-order
    step for the flow model; a non-default solver writes to `..._{total_step}_{solver}{S}/`.

  * `--cfg_interval LO,HI`: guidance interval (not in the reference, quality on trained checkpoints not
    assessed).  Classifier-free guidance on the loop steps `LO*steps <= j < HI*steps` only, the conditional pass alone (half the
    sequences) on the others; a window short of the whole loop writes to `..._gi{j0}-{j1}/`, after the solver suffix.

    python infer.py --dataset_name ETTh1_24,ETTh1_48,ETTh1_96 --cfg_scale 9 --total_step 10 --run_multi True
    python infer.py --dataset_name ETTh1_96 --backbone ddpm --total_step 1000 --solver dpmpp2m --sample_steps 50
"""
import argparse
import copy
import math
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from datafactory.dataloader import epoch_index_batches, loader_provider, resident_tables, walk_index_batches   # noqa: E402
from model.backbone.DDPM import DDPM                          # noqa: E402,F401  (API parity)
from model.backbone.rectified_flow import RectifiedFlow      # noqa: E402,F401
from model.denoiser.transformer import Transformer            # noqa: E402
from t2ms_amd import dist as tdist                            # noqa: E402
from t2ms_amd import synth                                    # noqa: E402
from t2ms_amd._lib import LAT, LAT_C, LAT_W                   # noqa: E402  (a row's latent: LAT = LAT_C x LAT_W floats)
from t2ms_amd.sampler import Sampler, default_math, np_save_outputs, resolve_cfg_interval, resolve_solver   # noqa: E402


def _weight_seed(args):
    """--random_init: the synthetic weights keep the seed the driver started with (--run_multi advances the NOISE seed)."""
    return getattr(args, "weight_seed", args.seed)


def _load_models(args, device):
    root = args.dataset_name.split("_")[0]
    if args.random_init:
        from model.pretrained.vqvae import vqvae
        vae = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256,
                                          embedding_dim=64))
        vae.load_state_dict(synth.make_vae_state_dict(_weight_seed(args)), strict=True)
    else:
        vae = torch.load(f"results/saved_pretrained_models/dataset{root}_epoch2000/final_model.pth",
                         map_location=torch.device("cpu"), weights_only=False)     # infer.py:39
    vae = vae.float().to(device).eval()
    if args.denoiser == "MLP":
        # BASELINE configs[0] (plumbing): the MLP denoiser on the (B,64,L/4) latent, L = 24 (t2s_mlp_forward under no_grad)
        from model.denoiser.mlp import MLP
        model = MLP()
        if args.random_init:
            model.load_state_dict(synth.make_mlp_state_dict(_weight_seed(args)), strict=True)
        else:
            model.load_state_dict(torch.load(args.checkpoint_path, map_location="cpu")["model"], strict=False)
        model.encoder = vae.encoder
        return model.to(device).eval(), vae
    if args.denoiser != "DiT":
        raise ValueError("No denoiser found")
    model = Transformer().to(device)
    model.encoder = vae.encoder                                                     # infer.py:47
    if args.random_init:
        sd = synth.make_dit_state_dict(_weight_seed(args))
        sd.update({"encoder." + k: v for k, v in vae.encoder.state_dict().items()})
        model.load_state_dict(sd, strict=True)
    else:
        model.load_state_dict(torch.load(args.checkpoint_path, map_location="cpu")["model"])   # infer.py:48
    return model.to(device).eval(), vae


def sample_mlp_config1(model, vae, backbone, x_1, embedding, args, device, row0):
    """The loop of infer.py:76-95 for `--denoiser MLP`, in the runnable form SURVEY.md 8(d) config 1 prescribes: the
    reference's MLP needs a 6-wide latent (mlp.py:55,67) while its encoder emits 30 (vqvae.py:70), so the diffusion
    state is the PRE-interpolation latent `before` (B,64,L/4), L = 24, and the decoder's 6 -> 6 interpolation is the
    identity.  Every step is HIP kernels: the two `model(...)` calls are one launch of t2s_mlp_forward each (row a20), then
    the DDPM update; encoder and decoder likewise; x_T and the per-step draws come from the library's Philox stream keyed
    by the global row."""
    from t2ms_amd.sampler import XT_STREAM, philox_normal
    if backbone != "ddpm":
        raise ValueError("config 1 (MLP denoiser) is wired for --backbone ddpm")
    z_enc, before = model.encoder(x_1.contiguous())
    B, C, W = before.shape
    if W != 6:
        raise ValueError(f"the MLP denoiser needs the 6-wide latent of L = 24 series (mlp.py:67), got L/4 = {W}")
    from model.backbone.DDPM import DDPM as _DDPM
    ddpm = _DDPM(args.total_step, device)
    x_t = philox_normal(B, C * W, args.seed, XT_STREAM, row0, device).view(B, C, W)
    for j in range(args.total_step):
        t = torch.full((B,), args.total_step - 1 - j, dtype=torch.long, device=device)
        u = model(x_t, t, None)
        c = model(x_t, t, embedding)
        pred = u + args.cfg_scale * (c - u)                                               # infer.py:87
        x_t = ddpm.p_sample(x_t, pred, t, eps=philox_normal(B, C * W, args.seed, j, row0, device).view(B, C, W))
    series, _ = vae.decoder(x_t, length=x_1.shape[-1])
    return x_t, series.reshape(B, -1), z_enc


def launch_plan(n_rows, loader_batch, launch_batch, world):
    """Global row ranges [(s0, s1)] of the sampler launches.  The reference launches once per loader batch
    (infer.py:66-95; default --batch_size 2 = a 4-sequence CFG pass); rows are independent through the whole loop and the
    kernels are batch-invariant bit for bit, so the SAME rows in the SAME order may be sampled `launch_batch` per GPU at a
    time (default 256: the chip-filling shape) without changing a byte of the output.  launch_batch = 0 keeps the
    reference's launch shape (one launch per loader batch)."""
    per = loader_batch if launch_batch <= 0 else launch_batch * world
    return [(s0, min(s0 + per, n_rows)) for s0 in range(0, n_rows, per)]


# ------------------------------------------------------------------ the grid: datasets x cfg scales x runs in one job
class Cell(types.SimpleNamespace):
    """One (dataset, cfg scale) of the grid: `cfg` the guidance scale, `path` the directory its base run writes."""


_CFG_MAX = 3.4028234663852886e38        # the largest finite fp32: the kernels combine in fp32


def _cfg_values(value):
    """--cfg_scale -> [(value as the directory name formats it, float)].  A number passes as it is (argparse leaves a
    non-string default unconverted: the default 7 names `..._7_...`), a string is a comma-separated list of floats."""
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        vals = [value]
    else:
        vals = []
        for part in str(value).split(","):
            try:
                vals.append(float(part.strip()))
            except ValueError:
                raise ValueError(f"--cfg_scale: {part.strip()!r} is not a number") from None
    for v in vals:
        if not (math.isfinite(float(v)) and abs(float(v)) <= _CFG_MAX):
            raise ValueError(f"--cfg_scale: {v!r} is not a finite fp32 value")
    return [(v, float(v)) for v in vals]


def parse_cells(args):
    """The cells of the job, datasets x cfg scales in the order given, each with the generation directory the separate
    invocation `infer.py --dataset_name D --cfg_scale C` computes (infer.py:297-299 of the parent layout).  Refused: datasets
    of different roots (checkpoint and LA-VAE paths are per root), a list with `--denoiser MLP` (its loop is the per-batch
    config-1 loop, not the sampler), malformed or non-finite cfg values, a cell named twice."""
    names = [n.strip() for n in str(args.dataset_name).split(",")]
    if not all(names):
        raise ValueError(f"--dataset_name: empty entry in {args.dataset_name!r}")
    cfgs = _cfg_values(args.cfg_scale)
    roots = sorted({n.split("_")[0] for n in names})
    if len(roots) > 1:
        raise ValueError(f"--dataset_name: all datasets of one job must share one root (checkpoint and LA-VAE), got {roots}")
    if args.denoiser == "MLP" and len(names) * len(cfgs) > 1:
        raise ValueError("--denoiser MLP samples one dataset at one cfg scale per job (lists are for the DiT sampler)")
    # --solver / --sample_steps / --eta: the default follows the backbone and leaves every path as it was; a few-step solver
    # names its own directory ("..._{steps}_{solver}{S}")
    args.solver, suffix = resolve_solver(args.backbone, getattr(args, "solver", None), getattr(args, "sample_steps", None),
                                         getattr(args, "eta", None), args.total_step)
    if suffix and args.denoiser == "MLP":
        raise ValueError(f"--solver {args.solver} runs in the DiT sampler (--denoiser MLP keeps the reference's loop)")
    # --cfg_interval LO,HI: guidance on a window of the loop (every cell of the job); the loop is --sample_steps long with a
    # few-step ddpm solver.  Absent, or the whole loop: every path as it was; else the directory gets "_gi{j0}-{j1}"
    interval = getattr(args, "cfg_interval", None)
    if interval is not None and args.denoiser == "MLP":
        raise ValueError("--cfg_interval runs in the DiT sampler (--denoiser MLP keeps the reference's loop)")
    loop_steps = args.sample_steps if (suffix and getattr(args, "sample_steps", None) is not None) else args.total_step
    args.guide_steps, gi_suffix = resolve_cfg_interval(interval, loop_steps)
    suffix += gi_suffix
    cells = []
    for name in names:
        for shown, cfg in cfgs:
            path = os.path.join(args.save_path, "generation",
                                "{}_{}_{}_{}_{}".format(args.backbone, args.denoiser, name, shown, args.total_step) + suffix)
            cells.append(Cell(dataset_name=name, cfg=cfg, cfg_shown=shown, path=path))
    if len({c.path for c in cells}) != len(cells):
        raise ValueError("the grid names the same (dataset, cfg scale) twice")
    return cells


def grid_units(cells, n_runs, seed):
    """The (cell, run) pairs of a job, cell-major: run 0 is the base run (seed S, the cell's directory), run r >= 1 is the
    `--run_multi` run `run_{r-1}` with seed S + r (infer.py:303-307 of the parent: the seed advances by one per run)."""
    units = []
    for ci, c in enumerate(cells):
        for r in range(n_runs):
            units.append(types.SimpleNamespace(cell=ci, run=r, seed=seed + r, dataset_name=c.dataset_name, cfg=c.cfg,
                                               path=c.path if r == 0 else os.path.join(c.path, f"run_{r - 1}")))
    return units


def _constructor_draws(args):
    """Build and drop the modules _load_models constructs, for their initialisation draws from the global CPU generator:
    the `vqvae(...)` constructor under --random_init (else the LA-VAE is unpickled: no draws), then the denoiser's."""
    if args.random_init:
        from model.pretrained.vqvae import vqvae
        vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    if args.denoiser == "MLP":
        from model.denoiser.mlp import MLP
        MLP()
    else:
        Transformer()


_DRAWS_AFTER = {}     # (random_init, denoiser, generator state before the constructors) -> state after them


def loader_order(args, dataset_name, seed):
    """-> (dataset, index batches (n_batches, B)) of the test loader of `dataset_name` in a run seeded with `seed`.  THE
    order of every run, single or grid, either denoiser: the parent's infer() drew it as
        torch.manual_seed(seed); loader_provider(...); _load_models(...) (the constructors' initialisation draws from the
        global CPU generator); epoch_index_batches(loader)
    and this helper replays exactly that sequence; the generator state the constructors leave is replayed from a cache
    keyed by the state before them (their draws are a function of that state alone)."""
    torch.manual_seed(seed)
    a = copy.copy(args)
    a.dataset_name, a.seed = dataset_name, seed
    dataset, loader = loader_provider(a, period="test")
    key = (bool(args.random_init), args.denoiser, torch.get_rng_state().numpy().tobytes())
    after = _DRAWS_AFTER.get(key)
    if after is None:
        _constructor_draws(args)
        _DRAWS_AFTER[key] = torch.get_rng_state()
    else:
        torch.set_rng_state(after)
    batches = walk_index_batches(loader) if getattr(args, "loader_batches", False) else epoch_index_batches(loader)
    return dataset, batches


def grid_plan(unit_rows, loader_batch, launch_batch, world):
    """Global row ranges [(s0, s1)] of the launches of a grid over the concatenated rows of its units (cell-major, then
    run, then the run's loader order).  launch_batch > 0: `launch_batch * world` rows per launch ACROSS unit boundaries (a
    launch may mix cells, runs and lengths); 0: one launch per loader batch of each unit (the reference's launch shape)."""
    if launch_batch > 0:
        return launch_plan(int(sum(unit_rows)), loader_batch, launch_batch, world)
    plan, off = [], 0
    for n in unit_rows:
        plan += [(off + a, off + b) for a, b in launch_plan(int(n), loader_batch, 0, world)]
        off += int(n)
    return plan


def launch_segments(unit_rows, g0, g1):
    """Rows [g0, g1) of the concatenation as [(unit, i0, i1)]: rows [i0, i1) of that unit's loader order."""
    out, off = [], 0
    for u, n in enumerate(unit_rows):
        a, b = max(g0, off), min(g1, off + int(n))
        if a < b:
            out.append((u, a - off, b - off))
        off += int(n)
    return out


def row_tables(segments, unit_seeds, unit_cfgs):
    """Per-row (seed, key row, cfg) of the rows `segments` name: a row of a unit is keyed as that unit's own one-run
    invocation keys it -- its seed, its position in the run's order (the global row of a 1x1 job), the cell's cfg."""
    seeds = np.concatenate([np.full(i1 - i0, int(unit_seeds[u]) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
                            for u, i0, i1 in segments])
    keys = np.concatenate([np.arange(i0, i1, dtype=np.int64) for u, i0, i1 in segments]).astype(np.uint32)
    cfgs = np.concatenate([np.full(i1 - i0, unit_cfgs[u], dtype=np.float32) for u, i0, i1 in segments])
    return seeds, keys, cfgs


# ------------------------------------------------------------------ the job: prologue, resident tables, row sink, launch loop
def _job_prologue(args):
    """-> (device, rank, world, dist, backbone name) of a sampling job, the process group up and the seed agreed."""
    device = torch.device(args.device)
    rank, _, world = tdist.env_world()
    dist = tdist.init("nccl", device)
    # ONE seed for the whole job: it seeds the loader shuffle (every rank must walk the same batches to take ITS rows
    # of each) and keys the Philox noise.  A per-rank time-based default would silently mis-pair series across ranks.
    args.seed = tdist.broadcast_int(dist, args.seed)
    if args.backbone not in ("flowmatching", "ddpm"):
        raise ValueError("No backbone found")
    return device, rank, world, dist, args.backbone


def _unit_tables(args, units, device):
    """Per unit its rows in its loader order (loader_order: the parent's generator sequence per (dataset, seed)), resident:
    x1_host (N, L) fp32, x1_dev, emb_dev, the length L and the loader batch B.  Output row i of a unit is dataset row
    order[i] -- the concatenation of the reference's batches (shuffle=True, drop_last=True, infer.py:66; N = floor(test / B)
    * B rows).  The test splits live in HBM."""
    tabs = []
    for u in units:
        dataset, batches = loader_order(args, u.dataset_name, u.seed)
        if batches.shape[0] == 0:
            raise RuntimeError(f"{u.dataset_name}: the test loader produced no full batch (drop_last=True): lower --batch_size")
        order = batches.reshape(-1)
        (series_tab, emb_tab, _), = resident_tables(dataset)
        xh = torch.as_tensor(series_tab)[order].float()              # (N, L) fp32: what `x_1.float()` gives per batch
        tabs.append(types.SimpleNamespace(x1_host=xh, x1_dev=xh.to(device), L=int(xh.shape[1]), B=int(batches.shape[1]),
                                          emb_dev=torch.as_tensor(emb_tab)[order].float().to(device)))
    return tabs


def rank_rows(held_chunks, r, world):
    """The global rows rank `r` of `world` holds of the launches `held_chunks` [(s0, s1)], in the order it sampled them:
    its shard_rows slice of every launch.  A function of its arguments alone, so every rank knows every rank's rows."""
    return np.concatenate([np.arange(0)] + [s0 + np.arange(*tdist.shard_rows(s1 - s0, r, world)) for s0, s1 in held_chunks])


class RowSink:
    """Where the sampled rows of a job go: they stay in HBM as packed fp32 rows
        (series zero-padded to Lmax | latent, LAT | encoding, LAT)
    until a flush gathers them and rank 0 files them by global row into `out` = (series (N, Lmax), latent (N, LAT_C,
    LAT_W), encoding likewise).  A flush runs at the end of the job and whenever the launches held since the last one
    reach T2S_INFER_FLUSH_ROWS rows (default 2^17; a row is 16 KB)."""

    def __init__(self, n_rows, Lmax, dist, rank, world, device):
        self.Lmax, self.dist, self.rank, self.world, self.device = Lmax, dist, rank, world, device
        self.flush_rows = int(os.environ.get("T2S_INFER_FLUSH_ROWS", str(1 << 17)))
        self.out = None
        if rank == 0:
            self.out = (np.empty((n_rows, Lmax), np.float32), np.empty((n_rows, LAT_C, LAT_W), np.float32),
                        np.empty((n_rows, LAT_C, LAT_W), np.float32))
        self.held, self.held_chunks = [], []

    @staticmethod
    def pack(series, lat, z_enc):
        n = series.shape[0]
        return torch.cat([series, lat.reshape(n, LAT), z_enc.reshape(n, LAT)], dim=1)

    def add(self, s0, s1, packed):
        """Launch [s0, s1) is done: `packed` holds this rank's rows of it, None for a rank without rows in the launch (it
        records the launch all the same, and joins the flush)."""
        if packed is not None:
            self.held.append(packed)
        self.held_chunks.append((s0, s1))
        if sum(b - a for a, b in self.held_chunks) >= self.flush_rows:
            self.flush()

    def flush(self):
        """Collective: every rank hands over the rows it sampled since the last flush (ONE all_gather of the packed rows; a
        rank without rows joins with an empty tensor) and rank 0 files them by global row."""
        if not self.held_chunks:
            return
        Lmax = self.Lmax
        dest = [rank_rows(self.held_chunks, r, self.world) for r in range(self.world)]
        mine = torch.cat(self.held, dim=0) if self.held else torch.empty(0, Lmax + 2 * LAT, device=self.device)
        parts = tdist.gather_ragged(self.dist, mine, [len(d) for d in dest], self.rank)
        if self.rank == 0:
            for d, part in zip(dest, parts):
                if len(d) == 0:
                    continue
                p = part.cpu().numpy()
                self.out[0][d] = p[:, :Lmax]
                self.out[1][d] = p[:, Lmax:Lmax + LAT].reshape(-1, LAT_C, LAT_W)
                self.out[2][d] = p[:, Lmax + LAT:].reshape(-1, LAT_C, LAT_W)
        self.held.clear()
        self.held_chunks.clear()


def _dit_launch(args, device, backbone, model, vae, tabs, unit_seeds, unit_cfgs):
    """-> (sample_launch, trace_rows) of the DiT: the fused Sampler on the rows of a launch, each keyed by (unit seed,
    position in the unit's order, cell cfg) through Sampler.set_rows; encode and decode run per length group (a launch that
    mixes lengths decodes outside the sampler's graph: the same decode kernel)."""
    lens = [t.L for t in tabs]
    Lmax = max(lens)
    samplers = {}
    # the few-step solver of the job (parse_cells resolved it; absent = the backbone's own update, as before)
    solver_kw = dict(solver=getattr(args, "solver", None), sample_steps=getattr(args, "sample_steps", None),
                     eta=getattr(args, "eta", None) or 0.0, guide_steps=getattr(args, "guide_steps", None))

    def sampler_of(key, cfg, n, L):
        if key not in samplers:
            samplers[key] = Sampler(model, vae.decoder, backbone, args.total_step, cfg, n, L, device, use_graph=True,
                                    seed=args.seed, row0=0, **solver_kw)
        return samplers[key]

    def length_groups(segs):
        """{L: (row positions in the launch, the segments of that length)} in launch order."""
        groups, pos = {}, 0
        for u, i0, i1 in segs:
            g = groups.setdefault(lens[u], ([], []))
            g[0].append(torch.arange(pos, pos + i1 - i0, device=device))        # made on the device: no host wait
            g[1].append((u, i0, i1))
            pos += i1 - i0
        return {Lg: (torch.cat(p), s) for Lg, (p, s) in groups.items()}

    def sample_launch(segs, n):
        seeds, keys, cfgs = row_tables(segs, unit_seeds, unit_cfgs)
        embedding = torch.cat([tabs[u].emb_dev[i0:i1] for u, i0, i1 in segs]) if len(segs) > 1 else \
            tabs[segs[0][0]].emb_dev[segs[0][1]:segs[0][2]]
        groups = length_groups(segs)
        if len(groups) == 1:
            x_1 = torch.cat([tabs[u].x1_dev[i0:i1] for u, i0, i1 in segs])
            z_enc, _ = model.encoder(x_1.contiguous())                      # infer.py:73-74
        else:
            z_enc = torch.empty(n, LAT_C, LAT_W, device=device)
            for Lg, (pos, gsegs) in groups.items():
                z_enc[pos] = model.encoder(torch.cat([tabs[u].x1_dev[i0:i1] for u, i0, i1 in gsegs]).contiguous())[0]
        L0 = lens[segs[0][0]]
        sampler = sampler_of((n, L0), unit_cfgs[segs[0][0]], n, L0)
        sampler.set_rows(seeds, keys, cfgs)       # this launch's (seed, key row, cfg) per row; the graph is kept
        lat, series, _ = sampler.run(embedding.contiguous(), decode=len(groups) == 1)
        ser = torch.zeros(n, Lmax, device=device)
        if len(groups) == 1:
            ser[:, :L0] = series.reshape(n, L0)
        else:
            for Lg, (pos, _) in groups.items():
                ser[pos, :Lg] = vae.decoder(lat[pos].contiguous(), length=Lg)[0].reshape(-1, Lg)
        return ser, lat, z_enc

    def trace_rows(ui, m):
        """The per-step decode of row 0 (infer.py:90-93) of unit `ui`, from an eager run of its first `m` rows."""
        ts = sampler_of(("trace", m, lens[ui]), unit_cfgs[ui], m, lens[ui])
        ts.set_rows(*row_tables([(ui, 0, m)], unit_seeds, unit_cfgs))
        return ts.run(tabs[ui].emb_dev[:m].contiguous(), decode=True, trace=True)[2].cpu().numpy()

    return sample_launch, trace_rows


def _mlp_launch(args, device, backbone, model, vae, tabs, unit_seeds, unit_cfgs):
    """-> (sample_launch, no trace) of the MLP denoiser (BASELINE configs[0] plumbing): sample_mlp_config1 on one loader
    batch of one unit, keyed by the unit's seed and the rows' position in the unit, at the cell's cfg."""
    runs = []
    for seed, cfg in zip(unit_seeds, unit_cfgs):
        a = copy.copy(args)
        a.seed, a.cfg_scale = seed, cfg
        runs.append(a)

    def sample_launch(segs, n):
        assert len(segs) == 1, "an MLP launch is one loader batch of one unit"
        u, i0, i1 = segs[0]
        lat, series, z_enc = sample_mlp_config1(model, vae, backbone, tabs[u].x1_dev[i0:i1], tabs[u].emb_dev[i0:i1], runs[u],
                                                device, i0)
        lat = torch.nn.functional.pad(lat, (0, LAT_W - lat.shape[2]))      # the .npy layout is (N,64,30): zero-padded
        return series, lat, z_enc

    return sample_launch, None


def infer(args):
    """ONE run of one (dataset, cfg scale): args.dataset_name, args.cfg_scale, seeded by args.seed, into
    args.generation_save_path_result -- the 1x1 job of sample_grid, either denoiser."""
    cell = Cell(dataset_name=args.dataset_name, cfg=float(args.cfg_scale), cfg_shown=args.cfg_scale,
                path=args.generation_save_path_result)
    res = sample_grid(args, [cell], 1)
    return res[0] if res is not None else None


def sample_grid(args, cells, n_runs):
    """THE sampling job: every (cell, run) of `cells` x `n_runs` in one go; every unit writes exactly the four files (and
    `--trace`'s x_infer_trace.npy) its own one-run invocation writes.  Models are built once; the rows of all units are
    concatenated (cell-major, then run, then the run's loader order), cut into launches (grid_plan) and each launch is
    sharded over the ranks; what differs between the denoisers is how the rows of a launch are sampled.  DiT:
    `--launch_batch` rows per GPU across unit boundaries, the fused Sampler with per-row tables (_dit_launch) -- rows never
    interact and the kernels are batch-invariant bit for bit, so a row comes out as in its own invocation.  MLP: one
    launch per loader batch of one unit, as the reference (_mlp_launch).
    -> on rank 0 [(x_1, x_t, lat_dec, lat_enc)] per unit, grid order; None elsewhere."""
    device, rank, world, dist, backbone = _job_prologue(args)
    dit = args.denoiser == "DiT"
    units = grid_units(cells, n_runs, args.seed)
    if rank == 0:
        grid = f"\t cells: {len(cells)} x runs: {n_runs}" if dit or len(units) > 1 else ""       # one MLP run: the reference's line
        print(f"Inference config::Step: {args.total_step}\t CFG Scale: {', '.join(str(c.cfg_shown) for c in cells)}\t "
              f"Use Pretrained VAE: {args.usepretrainedvae}\t GPUs: {world}{grid}")
        for u in units:
            os.makedirs(u.path, exist_ok=True)
    first = copy.copy(args)
    first.dataset_name = cells[0].dataset_name          # every cell shares the root (parse_cells): one checkpoint, one LA-VAE
    model, vae = _load_models(first, device)
    if dit:
        args.math = getattr(args, "math", None) or default_math()
        model.set_math(args.math)
        if rank == 0:
            print(f"matrix arithmetic: {args.math}" + {"bf16x3": " (fp32-accurate split-bf16 products; --math f32 = exact f32 MFMA)",
                                                       "bf16": " (single-pass bf16 operands, fp32 accumulate and residual stream: NOT fp32-accurate; "
                                                               "--math bf16x3 = fp32-accurate)"}.get(args.math, ""))
    tabs = _unit_tables(args, units, device)
    unit_rows = [int(t.x1_host.shape[0]) for t in tabs]
    offs = np.cumsum([0] + unit_rows)
    n_rows, Lmax, B = int(offs[-1]), max(t.L for t in tabs), tabs[0].B
    if rank == 0:
        print("dataset length:", ", ".join(str(n // B) for n in unit_rows[::n_runs]))
    launch_batch = int(getattr(args, "launch_batch", 256)) if dit else 0     # MLP: one sampling loop per loader batch
    plan = grid_plan(unit_rows, B, launch_batch, world)
    sample_launch, trace_rows = (_dit_launch if dit else _mlp_launch)(args, device, backbone, model, vae, tabs,
                                                                      [u.seed for u in units], [u.cfg for u in units])
    sink = RowSink(n_rows, Lmax, dist, rank, world, device)
    mixed, traces = 0, {}
    t_start = time.time()
    with torch.no_grad():
        for k, (s0, s1) in enumerate(plan):
            if len(launch_segments(unit_rows, s0, s1)) > 1:
                mixed += 1
            lo, hi = tdist.shard_rows(s1 - s0, rank, world)
            n = hi - lo                   # a rank without rows in this launch (fewer rows than GPUs) only joins the flush
            sink.add(s0, s1, sink.pack(*sample_launch(launch_segments(unit_rows, s0 + lo, s0 + hi), n)) if n > 0 else None)
            if rank == 0:
                print(f"Generating {k}th Batch TS...  (rows {s0}..{s1 - 1} of {n_rows}, {s1 - s0} series per launch)")
        sink.flush()
        if getattr(args, "trace", False) and rank == 0 and trace_rows is not None:
            # from exactly the rows the unit's own invocation holds in its first launch on rank 0
            for ui in range(len(units)):
                first_launch = min(B if launch_batch <= 0 else launch_batch * world, unit_rows[ui])
                traces[ui] = trace_rows(ui, tdist.shard_rows(first_launch, 0, world)[1])
    tdist.barrier(dist, device)
    loop_s = time.time() - t_start
    args.stats = {"series": n_rows, "loop_s": loop_s, "launches": len(plan), "loader_batch": B, "gpus": world,
                  "series_per_launch_and_gpu": (plan[0][1] - plan[0][0]) // world, "cells": len(cells), "runs": n_runs,
                  "mixed_launches": mixed}
    results = None
    if rank == 0:
        print(f"{n_rows} series in {loop_s:.2f} s ({n_rows / loop_s:.1f} series/s)")
        results = []
        for ui, u in enumerate(units):
            a, b = int(offs[ui]), int(offs[ui + 1])
            x_1 = tabs[ui].x1_host.numpy()
            x_t = np.ascontiguousarray(sink.out[0][a:b, :tabs[ui].L])
            lat_dec, lat_enc = sink.out[1][a:b], sink.out[2][a:b]
            np_save_outputs(u.path, x_1, x_t, lat_dec, lat_enc)                    # infer.py:118-123
            if ui in traces:
                np.save(os.path.join(u.path, "x_infer_trace.npy"), traces[ui])
            print(f"saved {x_1.shape[0]} series to {u.path}")
            results.append((x_1[:, :, None], x_t[:, :, None], lat_dec, lat_enc))
    tdist.barrier(dist, device)
    return results


def _save_figs(path, x_1, x_t):
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except Exception:                                          # plotting is optional
        return
    for i in range(min(10, x_1.shape[0])):
        plt.clf()
        plt.plot(x_1[i], label="ground truth")
        plt.plot(x_t[i], label="generated")
        plt.legend()
        plt.savefig(os.path.join(path, f"fig_{i}.jpg"))


def build_parser():
    p = argparse.ArgumentParser(description="Inference flow matching model")
    p.add_argument("--batch_size", type=int, default=2, help="batch size")
    p.add_argument("--save_path", type=str, default="./results/denoiser_results", help="Denoiser Model save path")
    p.add_argument("--usepretrainedvae", default=True, help="pretrained vae")
    p.add_argument("--backbone", type=str, default="flowmatching", help="flowmatching or DDPM or EDM")
    p.add_argument("--denoiser", type=str, default="DiT", help="DiT or MLP")
    p.add_argument("--cfg_scale", type=str, default=7,
                   help="CFG Scale; a comma-separated list samples every dataset at each scale in one job")
    p.add_argument("--total_step", type=int, default=100, help="total step sampled from [0,1]")
    p.add_argument("--checkpoint_id", type=int, default=19999, help="model id")
    p.add_argument("--dataset_name", type=str, default="exchangerate_24",
                   help="dataset name; a comma-separated list (one root) samples the grid datasets x cfg scales in one job")
    p.add_argument("--run_multi", type=bool, default=False, help="run multi times for CRPS,MAP,MRR,NDCG")
    # additions (see module docstring)
    p.add_argument("--seed", type=int, default=None, help="Philox noise seed (default: time based)")
    p.add_argument("--synthetic", type=int, default=0, help="serve N synthetic rows instead of the CSV")
    p.add_argument("--random_init", action="store_true", help="seeded synthetic weights instead of checkpoints")
    p.add_argument("--trace", action="store_true", help="decode row 0 after every step of the first batch")
    p.add_argument("--no_figs", action="store_true", help="skip the ten fig_i.jpg plots (infer.py:157-163)")
    p.add_argument("--launch_batch", type=int, default=256,
                   help="series per GPU and sampler launch: loader batches are coalesced into launches of this size (same "
                        "rows, same order, same bytes in the files); 0 = one launch per loader batch as the reference")
    p.add_argument("--loader_batches", action="store_true",
                   help="take the row order from a real DataLoader walk (public torch API) instead of the emulated draws of "
                        "datafactory.epoch_index_batches -- same order, same files; the cross-check after a torch upgrade")
    p.add_argument("--math", default=None, choices=["f32", "bf16x3", "bf16"],
                   help="matrix arithmetic of the DiT: bf16x3 (default; fp32-ACCURATE split-bf16 products on the bf16 matrix cores, "
                        "+35 %%; its error against fp64 is not larger than the reference's PyTorch-CPU fp32 arithmetic, "
                        "profiles/r05_accuracy.md), f32 (exact f32 MFMA) or bf16 (opt-in mixed precision: operands rounded "
                        "once to bf16, fp32 accumulate; 2.5x bf16x3, rms error ~1e-3 on outputs of ~4.5 per forward, DESIGN.md 4.4)")
    p.add_argument("--solver", default=None, choices=["ancestral", "ddim", "dpmpp2m", "euler", "ab2"],
                   help="sampling update (default: the backbone's own -- ancestral for ddpm, euler for flowmatching: the reference's "
                        "run).  ddpm: ddim / dpmpp2m sample a --total_step checkpoint in --sample_steps denoiser evaluations; "
                        "flowmatching: ab2 is a second-order step at the same --total_step evaluations.  No counterpart in the "
                        "reference; the output directory gets the suffix _{solver}{S}")
    p.add_argument("--sample_steps", type=int, default=None,
                   help="denoiser evaluations S <= --total_step of --solver ddim / dpmpp2m (default: --total_step)")
    p.add_argument("--eta", type=float, default=None, help="--solver ddim: noise scale (0 = deterministic, the default)")
    p.add_argument("--cfg_interval", default=None, metavar="LO,HI",
                   help="guidance interval (DiT only): classifier-free guidance on the loop steps j with LO*steps <= j < HI*steps "
                        "(fractions of the loop, 0 <= LO <= HI <= 1, j = 0 the noisiest step), the conditional pass alone -- half the "
                        "sequences -- on the others; applies to every cell of the job.  No counterpart in the reference; a window "
                        "short of the whole loop adds the suffix _gi{j0}-{j1} to the output directory")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.mix_train = False
    try:
        resolve_solver(args.backbone, args.solver, args.sample_steps, args.eta, args.total_step)
        if args.cfg_interval is not None and args.denoiser == "MLP":
            raise ValueError("--cfg_interval runs in the DiT sampler (--denoiser MLP keeps the reference's loop)")
        resolve_cfg_interval(args.cfg_interval, args.sample_steps or args.total_step)
    except ValueError as e:
        sys.exit(f"infer.py: {e}")
    if not torch.cuda.is_available():
        sys.exit("infer.py: no GPU visible -- this build runs the HIP path only (no CPU fallback)")
    local_rank = tdist.local_device_index()
    torch.cuda.set_device(local_rank)
    args.device = f"cuda:{local_rank}"
    if args.seed is None:
        args.seed = int(time.time()) & 0x7FFFFFFF
    args.weight_seed = args.seed
    cells = parse_cells(args)
    root = cells[0].dataset_name.split("_")[0]
    args.checkpoint_path = os.path.join(args.save_path, "checkpoints", f"{args.backbone}_{args.denoiser}_{root}",
                                        f"model_{args.checkpoint_id}.pth")
    print("start generate", args.run_multi)
    n_runs = 11 if args.run_multi else 1                         # infer.py:148-164: 1 + 10 runs
    if len(cells) == 1:                                          # a single cell: the args of the parent's one-cell job
        args.dataset_name, args.cfg_scale = cells[0].dataset_name, cells[0].cfg_shown
    results = sample_grid(args, cells, n_runs)
    if results is not None and not args.no_figs:
        for ci, c in enumerate(cells):                           # each cell's figures from its last run, as before
            last = results[(ci + 1) * n_runs - 1]
            _save_figs(c.path, last[0], last[1])
    return args


if __name__ == "__main__":
    main()
