#!/usr/bin/env python3
"""Pre-train the attention seq2seq codec (model/pretrained/TSae.py, AttentionSeq2SeqAutoencoder): the training loop of the
reference's pretrained_mylavae.py (lines 195-234) with its flags, the model's shape on the command line where that script reads
config.yaml, and arrays where it reads the bench-press loader.

    python pretrain_tsae.py --dataset_name benchpress --series_npy g36.npy,g72.npy,g144.npy --train_engine hip
    python pretrain_tsae.py --dataset_name synth --synthetic 64 --split_base_num 36 --pretrained_epc 200 --train_engine hip

Data: one (N,C,L) float array per length group (`--series_npy a.npy,b.npy,...`) or `--synthetic N` seeded rows per group at
`--split_base_num` x 1, 2, 4 (as pretrain_lavae.py's motion run).  Batch index i holds rows [i * batch_size, (i + 1) * batch_size)
of every group in this epoch's order; each group of a batch is one `shared_eval(xs, None, optimizer, 'train')` call.

Kept from the reference: AdamW + the warm-up / cosine scheduler of BaseModel.configure_optimizers, one `scheduler.step()` per epoch;
`total_epochs = int((pretrained_epc + epoch) / max(1, batches_per_epoch) + 0.5)`; `--epoch` != 0 resumes from final_model.pth
(strict=False); every max(1, total_epochs // 10) epochs a 'val' pass (encode + generate, here over the same groups in stored order)
and `model_epoch_<n>.pth`; `final_model.pth` is a plain state dict under <save_path>/<split_base_num>_<dataset_name>_epoch<pretrained_epc>/
(tools/tsae_reconstruct.py --state_dict loads it).  No plots.  `--train_engine hip` runs every covered step (T <= 192) on
csrc/t2s_tsae_train.hip; the default follows T2S_TSAE_TRAIN (torch).
"""
import argparse
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from pretrain_lavae import (MotionLoader, add_dataset_root, motion_groups, resolve_dataset_root,  # noqa: E402
                            seed_everything)                            # (the length-group plumbing is shared)


def save_dir_of(args):
    return os.path.join(args.save_path, "{}_{}_epoch{}".format(args.split_base_num, args.dataset_name, args.pretrained_epc))


def total_epochs_of(pretrained_epc, epoch, batches_per_epoch):
    """pretrained_mylavae.py:198, `batches_per_epoch` standing in for len(train_loader)."""
    return int(((pretrained_epc + epoch) / max(1, batches_per_epoch)) + 0.5)


def _groups_of(batch, device):
    """The (B,T,F) device tensors of one loader batch: its non-empty length groups, (N,C,L) -> (N,L,C)."""
    return [g[1].transpose(1, 2).clone().detach().float().contiguous().to(device) for g in batch if g is not None]


def validate(model, loader, device):
    """The 'val' pass over every group in stored order -> mean loss."""
    model.eval()
    losses = [model.shared_eval(xs, None, None, "val")[0] for batch in loader for xs in _groups_of(batch, device)]
    return float(torch.stack(losses).mean())


def pretrain(args):
    """-> the mean training loss of every epoch."""
    if not torch.cuda.is_available():
        sys.exit("pretrain_tsae.py: no GPU visible -- the 'val' pass and the HIP engine have no CPU fallback")
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    device = torch.device(f"cuda:{torch.cuda.current_device()}")
    save_dir = save_dir_of(args)
    os.makedirs(save_dir, exist_ok=True)
    seed_everything(args.general_seed)
    model = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(
        input_dim=args.input_dim, flow_dim=args.flow_dim, d_ff=args.d_ff, num_encoder_layers=args.num_encoder_layers,
        num_decoder_layers=args.num_decoder_layers, num_heads=args.num_heads)).to(device)
    model.set_train_engine(args.train_engine)
    print(f"train engine: {model._train_engine()}")
    optimizer, scheduler = model.configure_optimizers(lr=args.learning_rate)
    groups = motion_groups(args)
    train_loader, val_loader = MotionLoader(groups, args.batch_size, seed=args.general_seed), MotionLoader(groups, args.batch_size)
    final = os.path.join(save_dir, "final_model.pth")
    loss_list = []
    if not args.only_inference:
        if args.epoch != 0:
            model.load_state_dict(torch.load(final, map_location=device), strict=False)
        total_epochs = total_epochs_of(args.pretrained_epc, args.epoch, len(train_loader))
        print(f"total epoch : {total_epochs}")
        for epoch in range(total_epochs):
            model.train()
            group_losses = []                                   # device scalars: one read-back per epoch, not per step
            for batch in train_loader:
                for xs in _groups_of(batch, device):
                    loss, _ = model.shared_eval(xs, None, optimizer, "train")
                    group_losses.append(loss.detach())
            loss_list.append(float(torch.stack(group_losses).mean()))
            print(f"epoch {epoch + 1}/{total_epochs}: {len(group_losses)} steps, training loss {loss_list[-1]:.6f}")
            scheduler.step()
            if epoch % max(1, total_epochs // 10) == 0:
                print(f"validation loss {validate(model, val_loader, device):.6f}")
                torch.save(model.state_dict(), os.path.join(save_dir, f"model_epoch_{epoch}.pth"))
                print(f"Saved Model from epoch: {epoch}")
        torch.save(model.state_dict(), final)
        print("Training complete.")
    print("Starting inference...")
    model.load_state_dict(torch.load(final, map_location=device), strict=False)
    print(f"reconstruction loss {validate(model, val_loader, device):.6f}")
    return loss_list


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Pre-train the attention seq2seq codec (TSae)")
    p.add_argument("--dataset_name", type=str, default="benchpress", help="names the checkpoint directory")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--save_path", type=str, default="results/saved_pretrained_models/", help="root of the checkpoint directories")
    p.add_argument("--only_inference", type=bool, default=False)
    p.add_argument("--epoch", type=int, default=0, help="!= 0: resume from final_model.pth and add this many updates")
    p.add_argument("--learning_rate", type=float, default=1e-3, help="learning rate for the optimizer")
    p.add_argument("--input_dim", type=int, default=10)
    p.add_argument("--flow_dim", type=int, default=64)
    p.add_argument("--d_ff", type=int, default=128)
    p.add_argument("--num_encoder_layers", type=int, default=3)
    p.add_argument("--num_decoder_layers", type=int, default=3)
    p.add_argument("--num_heads", type=int, default=8)
    p.add_argument("--pretrained_epc", type=int, default=2000, help="optimisation updates the epoch count is derived from")
    p.add_argument("--split_base_num", type=int, default=36, help="--synthetic groups are this long x 1, 2, 4; names the directory")
    p.add_argument("--general_seed", type=int, default=42)
    p.add_argument("--series_npy", type=str, default="", help="comma-separated .npy files, one (N,C,L) array per length group")
    p.add_argument("--synthetic", type=int, default=0, help="N seeded rows per length group instead of files")
    p.add_argument("--train_engine", choices=["hip", "torch"], default=None, help="engine of the 'train' steps (default: T2S_TSAE_TRAIN)")
    add_dataset_root(p)
    args = p.parse_args(argv)
    if not args.series_npy and args.synthetic <= 0 and not args.dataset_root:
        p.error("a data source is needed: --series_npy a.npy,b.npy,... or --synthetic N")
    resolve_dataset_root(p, args)
    return args


if __name__ == "__main__":
    pretrain(get_args())
