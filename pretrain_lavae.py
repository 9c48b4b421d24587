#!/usr/bin/env python3
"""LA-VAE pre-training driver (reference pretrained_lavae_unified.py): same flags and defaults, the epoch loop of
lines 142-174, the same output paths -- with every optimisation step (vqvae.shared_eval(..., 'train')) on the HIP
kernels: encoder and decoder forward + backward, both MSE terms, fused AdamW.

    python pretrain_lavae.py --dataset_name ETTh1 --mix_train True
    python pretrain_lavae.py --dataset_name ETTh1_24 --split_train --synthetic 600
    python pretrain_lavae.py --dataset_name benchpress --input_dim 10 --flow_dim 64 --series_npy g36.npy,g72.npy,g144.npy

writes results/saved_pretrained_models/dataset{name}_epoch{updates}/final_model.pth, the file train.py:22 and infer.py:39
start from (they look it up under the dataset's family name, i.e. what a mix-train run on `--dataset_name ETTh1` writes).

Kept from the reference: AdamW(lr, weight_decay 1e-2) as BaseModel.configure_optimizers builds it, and NO scheduler step
(the reference builds one and never steps it); `epochs = int(updates / len(loader) + 0.5)`; a whole-module checkpoint
`model_epoch_{e}.pth` whenever `e % (updates / 10) == 0`; afterwards the test split goes through
shared_eval(..., 'test') and metrics.txt gets MAE and RMSE.
Different on purpose: `final_model.pth` is ALWAYS the whole module (torch.save(model, ...)) -- the reference's non-mix
branch writes a bare state dict there, which its own train.py:22 / infer.py:39 cannot use; data comes from this project's
loader_provider (`--dataset_name`, `--synthetic N`, `--split_train` as in train.py) instead of the fork's bench-press
loader; MAE / RMSE run over every test series (the reference keeps one length group); the plots are omitted.

`--input_dim C` > 1 pre-trains the C-channel motion codec (model.pretrained.myvqvae.vqvae, latent width `--flow_dim`) instead,
with the reference's mix-train loop (pretrained_mylavae.py:198-211): per batch index one step per length group, on the HIP
forwards and backwards where the shape is covered (t2s_vae_*_backward_mc: L <= 192).  Its data are arrays, one (N, C, L) float
array per length group (`--series_npy a.npy,b.npy,...`) or synthetic groups of `--split_base_num` x 1, 2, 4 samples
(`--synthetic N`); the fork's JSON motion loaders and its embedding fetch are not part of this driver, and MAE / RMSE run over
the training groups (there is no test split).  The saved file loads into Sampler(Transformer(flow_dim), model.decoder, ...).
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def seed_everything(seed_value=42):
    random.seed(seed_value)
    np.random.seed(seed_value)
    torch.manual_seed(seed_value)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed_value)
    print(f"seed: {seed_value}")


def save_dir_of(args):
    """pretrained_lavae_unified.py:130-131."""
    return os.path.join(args.save_path, "dataset{}_epoch{}".format(args.dataset_name, args.num_training_updates))


def pretrain_step(model, opt, batch):
    """One optimisation step on a (B, L) device batch (pretrained_lavae_unified.py:151-152 / 166-167) -> its loss (device)."""
    loss, _, _, _ = model.shared_eval(batch, opt, "train")
    return loss


def _series_batches(data, mix):
    """The series tensors of one loader batch: the non-empty length groups of a mix-train batch, or the one batch."""
    groups = data if mix else [data]
    return [g[1] for g in groups if g is not None and g[1] is not None]


NO_MOTION_DATA = ("pretrain_lavae.py: --input_dim > 1 needs a data source: --series_npy a.npy,b.npy,... (one (N,C,L) array per "
                  "length group) or --synthetic N")


def motion_groups(args):
    """The length groups of a motion run -> [float tensor (N, C, L)], one per group: the `--series_npy` arrays in the order
    given, `--synthetic N` rows at `--split_base_num` x 1, 2, 4, or the train split of the bench-press / deadlift dataset
    under `--dataset_root` (datafactory.motion.motion_groups: the reference's length groups and alignment)."""
    C = args.input_dim
    if args.series_npy:
        groups = [torch.from_numpy(np.asarray(np.load(path), dtype=np.float32)) for path in args.series_npy.split(",") if path]
    elif args.synthetic > 0:
        from t2ms_amd import synth
        groups = [synth.make_mseries(args.general_seed + k, args.synthetic, C, args.split_base_num * m) for k, m in enumerate((1, 2, 4))]
    elif getattr(args, "dataset_root", ""):
        from datafactory.motion import motion_groups as dataset_groups
        groups = [g for g in dataset_groups(args) if g.shape[0]]
    else:
        sys.exit(NO_MOTION_DATA)
    for g in groups:
        if g.dim() != 3 or g.shape[1] != C or g.shape[0] < 1:
            sys.exit(f"pretrain_lavae.py: a length group must be a non-empty (N, {C}, L) array, got {tuple(g.shape)}")
    return groups


class MotionLoader:
    """The mix-train loader over length groups: batch index i holds, per group, its rows [i * batch_size, (i + 1) * batch_size)
    in this epoch's order (None once a shorter group has run out), in the (label, series) pairs _series_batches reads.
    `seed` None keeps the stored order; otherwise every epoch draws a new order per group from one seeded generator."""

    def __init__(self, groups, batch_size, seed=None):
        self.groups, self.batch_size = groups, int(batch_size)
        self.gen = None if seed is None else torch.Generator().manual_seed(int(seed))

    def __len__(self):
        return max((g.shape[0] + self.batch_size - 1) // self.batch_size for g in self.groups)

    def __iter__(self):
        order = [torch.arange(g.shape[0]) if self.gen is None else torch.randperm(g.shape[0], generator=self.gen) for g in self.groups]
        for i in range(len(self)):
            rows = [o[i * self.batch_size:(i + 1) * self.batch_size] for o in order]
            yield [(None, g[r]) if len(r) else None for g, r in zip(self.groups, rows)]


def epochs_of(num_training_updates, batches):
    """pretrained_lavae_unified.py:143 / pretrained_mylavae.py:198."""
    return int((num_training_updates / max(1, batches)) + 0.5)


def inference(model, test_loader, device, save_dir, mix):
    """pretrained_lavae_unified.py:55-94 without the plots: MAE / RMSE of the reconstruction over the test split."""
    model.eval()
    abs_sum = sq_sum = torch.zeros((), device=device, dtype=torch.float64)
    n = 0
    for data in test_loader:
        for batch_x in _series_batches(data, mix):
            real = batch_x.float().to(device)
            _, _, recon, _ = model.shared_eval(real, None, "test")
            diff = (real - recon.reshape(real.shape)).double()
            abs_sum = abs_sum + diff.abs().sum()
            sq_sum = sq_sum + (diff * diff).sum()
            n += diff.numel()
    mae = float(abs_sum) / max(n, 1)
    rmse = (float(sq_sum) / max(n, 1)) ** 0.5
    with open(os.path.join(save_dir, "metrics.txt"), "w") as f:
        f.write(f"MAE: {mae}\n")
        f.write(f"RMSE: {rmse}\n")
    return mae, rmse


def pretrain(args):
    """-> the loss of every optimisation step, in order."""
    if not torch.cuda.is_available():
        sys.exit("pretrain_lavae.py: no GPU visible -- this build runs the HIP path only (no CPU fallback)")
    from datafactory.dataloader import loader_provider
    from t2ms_amd.train import T2SAdamW
    motion = args.input_dim > 1
    if motion:
        from model.pretrained.myvqvae import vqvae
        groups = motion_groups(args)
    else:
        from model.pretrained.vqvae import vqvae
    device = torch.device(getattr(args, "device", None) or f"cuda:{torch.cuda.current_device()}")
    save_dir = save_dir_of(args)
    os.makedirs(save_dir, exist_ok=True)
    seed_everything(args.general_seed)
    model = vqvae(args).to(device)
    # BaseModel.configure_optimizers' hyper-parameters on the fused kernel; its scheduler is never stepped by the reference
    opt = T2SAdamW(model.parameters(), lr=args.learning_rate, weight_decay=1e-2)
    mix = args.mix_train or motion
    if motion:
        train_loader = MotionLoader(groups, args.batch_size, seed=args.general_seed)
    else:
        if args.mix_train:
            args.data_length = 0
        _, train_loader = loader_provider(args, period="train")
    losses, pending = [], []
    model.train()
    for epoch in range(epochs_of(args.num_training_updates, len(train_loader))):
        i = -1
        for i, data in enumerate(train_loader):
            for batch_x in _series_batches(data, mix):
                batch = batch_x.clone().detach().float().to(device)
                pending.append(pretrain_step(model, opt, batch))        # (.item() here would drain the GPU at every step)
        if pending:
            ep = torch.stack(pending).tolist()
            pending.clear()
            losses.extend(ep)
            print(f"Epoch: {epoch}, Batch: {i}, Loss: {float(np.mean(ep))}")
        if epoch % (args.num_training_updates / 10) == 0:
            torch.save(model, os.path.join(save_dir, f"model_epoch_{epoch}.pth"))
            print(f"Saved Model from epoch: {epoch}")
    torch.save(model, os.path.join(save_dir, "final_model.pth"))
    print("Training complete.")
    print("Starting inference...")
    if motion:
        test_loader = MotionLoader(groups, args.batch_size)
    else:
        _, test_loader = loader_provider(args, period="test")
    mae, rmse = inference(model, test_loader, device, save_dir, mix)
    print(f"MAE: {mae}  RMSE: {rmse}")
    return losses


def add_dataset_root(p):
    """The third data source of a motion run (shared with pretrain_tsae.py)."""
    p.add_argument("--dataset_root", type=str, default="", help="motion codec: train on <dataset_root>/<dataset_name> (benchpress / "
                   "deadlift: data.json + captions), the reference's three length groups; --series_npy / --synthetic come first")
    p.add_argument("--caption", type=str, default="", help="--dataset_root: the caption directory (default: the reference's per dataset)")


def resolve_dataset_root(p, args):
    """With --dataset_root in use: a motion dataset name, and the dataset's own group lengths and caption directory unless the
    command line gave them."""
    if not args.dataset_root or args.series_npy or args.synthetic > 0:
        return
    from datafactory.motion import DEFAULTS
    if args.dataset_name not in DEFAULTS:
        p.error(f"--dataset_root serves the motion datasets: --dataset_name {' / '.join(DEFAULTS)}, got {args.dataset_name!r}")
    if args.split_base_num == p.get_default("split_base_num"):
        args.split_base_num = DEFAULTS[args.dataset_name]["split_base_num"]
    args.caption = args.caption or DEFAULTS[args.dataset_name]["caption"]


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Pre-train the LA-VAE")
    p.add_argument("--dataset_name", type=str, default="ETTh1", help="dataset served by loader_provider")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--num_training_updates", type=int, default=2000, help="optimisation steps the epoch count is derived from")
    p.add_argument("--save_path", type=str, default="results/saved_pretrained_models/", help="root of the checkpoint directories")
    p.add_argument("--general_seed", type=int, default=42, help="seed of the python / numpy / torch generators")
    p.add_argument("--learning_rate", type=float, default=1e-3, help="AdamW learning rate")
    p.add_argument("--block_hidden_size", type=int, default=128, help="channels of the codec (128 for the HIP backward)")
    p.add_argument("--num_residual_layers", type=int, default=2, help="residual layers per stack (<= 4)")
    p.add_argument("--res_hidden_size", type=int, default=256, help="channels inside a residual layer (128 / 256 for the HIP backward)")
    p.add_argument("--embedding_dim", type=int, default=64, help="latent channels (64)")
    p.add_argument("--num_embeddings", type=int, default=128, help="accepted as in the reference, unused (no quantiser)")
    p.add_argument("--compression_factor", type=int, default=4, help="accepted as in the reference, unused")
    p.add_argument("--commitment_cost", type=float, default=0.25, help="accepted as in the reference, unused")
    p.add_argument("--mix_train", type=bool, default=False, help="train on the 24 / 48 / 96 length groups of one dataset family")
    p.add_argument("--synthetic", type=int, default=0, help="serve N synthetic rows per length instead of the CSVs")
    p.add_argument("--split_train", action="store_true", help="mix_train=False (argparse type=bool cannot be switched off)")
    p.add_argument("--input_dim", type=int, default=1, help="series channels; > 1 pre-trains the motion codec (myvqvae) on --series_npy / --synthetic")
    p.add_argument("--flow_dim", type=int, default=30, help="latent width of the motion codec (50 deadlift, 64 bench press)")
    p.add_argument("--series_npy", type=str, default="", help="motion codec: comma-separated .npy files, one (N,C,L) array per length group")
    p.add_argument("--split_base_num", type=int, default=36, help="motion codec: --synthetic groups are this long x 1, 2, 4")
    add_dataset_root(p)
    args = p.parse_args(argv)
    if args.split_train:
        args.mix_train = False
    if args.input_dim < 1:
        p.error("--input_dim must be >= 1")
    if args.input_dim > 1 and not args.series_npy and args.synthetic <= 0 and not args.dataset_root:
        sys.exit(NO_MOTION_DATA)
    if args.input_dim > 1:
        resolve_dataset_root(p, args)
    return args


if __name__ == "__main__":
    pretrain(get_args())
