#!/usr/bin/env python3
"""Drop-in for the reference's mytrain.py: train the wide-latent DiT (Transformer(flow_dim): deadlift W = 50, 800 tokens;
bench press W = 64, 1024 tokens) on the multichannel LA-VAE's latents, every optimisation step on the HIP kernels.

    python mytrain.py --dataset_name benchpress
    python mytrain.py --dataset_name deadlift --random_init --synthetic 64 --batch_size 32 --epochs 10 --save_path /tmp/out

The reference's loop (mytrain.py:58-97), kept:
  * loaders: datafactory.<name>.dataloader.loader_provider(args); a loader batch is a list of up to three length groups
    (texts, x (b,C,L_g), embedding(s), subjects), and every group is one optimisation step.  The reference unpacks FOUR
    fields per group although the bench-press loader yields five (text, x, prefix embedding, summary embedding, subject):
    here `--embedding summary|prefix` picks the stored embedding that conditions, as myinfer.py does;
  * models: vqvae(args) from results/saved_pretrained_models/<split_base_num>_<name>_epoch<pretrained_epc>/final_model.pth (or
    `--random_init`), Transformer(flow_dim).set_trainable(True), model.encoder = vae.encoder -- frozen unless
    `--usepretrainedvae ""`, in which case the encoder trains through its HIP backward (t2s_vae_encode_backward_mc) and the
    denoiser's input gradient (t2s_dit_train_input_grad);
  * the step (mytrain.py:66-86): flow matching t = round(u * total_step) / total_step, x_t = t x_1 + (1 - t) x_0, target
    x_1 - x_0; DDPM t = floor(u * total_step), x_t = q_sample(x_1, t, eps), target eps; one CFG coin `rand(1) < 0.3` per
    group drops the text; MSE loss; AdamW(lr 1e-4, weight_decay 0) as the fused T2SAdamW; OneCycleLR(max_lr 1e-4,
    total_steps = len(train_loader) * epochs) stepped once per loader batch;
  * checkpoints: dict(model, optimizer, epoch, loss_list) at <save_path>/checkpoints/<backbone>_DiT_<dataset>_<caption>_
    <pretrained_epc>/model_<epoch>.pth -- the file `myinfer.py --checkpoint_id <epoch>` loads -- every 100 epochs and at the
    last one; `--checkpoint_path FILE` resumes at its epoch + 1 with the optimiser state (the scheduler starts afresh, as
    in the reference).
Different on purpose: `loss_list` holds the per-epoch mean losses (the reference saves a list it never appends to); the
reference's hard stop after epoch 4000 and its loss-curve plot are not built; `--max_steps N` ends the run after N
optimisation steps (the epoch it stops in is checkpointed by the usual rule); `--synthetic N` serves N seeded clips per
length group, one loader batch per `--batch_size` clips of each group, without a dataset.  The arithmetic is fp32;
`--bf16` (train.py's flag) runs the bf16 mixed-precision step instead: bf16 MFMA operands and saved activations, fp32
accumulation, master weights, statistics and gradients.  The checkpoints are the same files either way (fp32 weights).
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

from datafactory.motion import dataset_module        # noqa: E402
from t2ms_amd import motion_cli                      # noqa: E402
from t2ms_amd.motion_cli import checkpoint_file      # noqa: E402,F401
from t2ms_amd.train import T2SAdamW, mse_loss        # noqa: E402


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Train a motion denoiser (reference mytrain.py)")
    # the reference's command line
    p.add_argument("--checkpoint_path", type=str, default="", help="resume from this checkpoint")
    p.add_argument("--dataset_name", type=str, choices=["deadlift", "benchpress"], required=True, help="dataset name")
    p.add_argument("--batch_size", type=int, default=512, help="clips per loader batch")
    p.add_argument("--epochs", type=int, default=20000, help="training epochs")
    p.add_argument("--save_path", type=str, default="./results/denoiser_results", help="root of checkpoints/")
    p.add_argument("--usepretrainedvae", default=True, help='freeze the codec\'s encoder ("" trains it)')
    p.add_argument("--total_step", type=int, default=100, help="time grid of the backbone")
    motion_cli.add_config_flags(p)       # --config and config.yaml's values as flags, --embedding, --random_init
    # this driver's own
    p.add_argument("--synthetic", type=int, default=0, help="N seeded synthetic clips per length group instead of the dataset")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many optimisation steps (0: run all epochs)")
    p.add_argument("--bf16", action="store_true", help="bf16 mixed-precision training step (fp32 master weights and gradients)")
    args = p.parse_args(argv)
    if args.batch_size < 1 or args.epochs < 1:
        p.error("--batch_size and --epochs must be >= 1")
    return motion_cli.resolve(args, "mytrain.py")


class _Groups(list):
    """--synthetic: loader batches held in memory (a list of lists of groups, as the DataLoader yields them)."""


def synthetic_loader(args):
    """N seeded clips per length group (split_base_num x 1, 2, 4 samples), `batch_size` clips of each group per loader batch."""
    from t2ms_amd import synth
    n, groups = args.synthetic, []
    for g, mult in enumerate((1, 2, 4)):
        x = synth.make_mseries(args.general_seed + g, n, args.input_dim, args.split_base_num * mult)
        groups.append((x, synth.make_text_embeddings(args.general_seed + g, n)))
    batches = _Groups()
    for lo in range(0, n, args.batch_size):
        batches.append([([f"synthetic/{g}/{i}" for i in range(lo, min(n, lo + args.batch_size))], x[lo:lo + args.batch_size],
                         emb[lo:lo + args.batch_size], ["synthetic"] * len(x[lo:lo + args.batch_size])) for g, (x, emb) in enumerate(groups)])
    return batches


def load_models(args, device):
    """(denoiser with the codec's encoder grafted on, codec), mytrain.py:23-42."""
    from model.denoiser.mytransformer import Transformer
    from model.pretrained.myvqvae import vqvae
    from t2ms_amd import synth
    vae = vqvae(args).float()
    model = Transformer(args.flow_dim).set_trainable(True)
    if getattr(args, "bf16", False):
        model.set_wide_train_bf16(True).set_train_dtype("bf16")
    if args.random_init:
        vae.load_state_dict(synth.make_mvae_state_dict(args.general_seed, args.input_dim, args.block_hidden_size,
                                                       args.num_residual_layers, args.res_hidden_size), strict=True)
        model.load_state_dict(synth.make_dit_state_dict(args.general_seed, width=args.flow_dim), strict=True)
    else:
        vae.load_state_dict(torch.load(args.pretrainedvae_path, map_location="cpu"))
    model.encoder = vae.encoder
    model, vae = model.to(device), vae.to(device)
    for name, param in model.named_parameters():
        if "encoder" in name:
            param.requires_grad = not args.usepretrainedvae
    return model, vae


def noisy_latent(args, backbone, x_1):
    """(x_t, t, target) of one group, mytrain.py:66-75.  Elementwise host-level torch ops where a gradient has to reach the
    encoder; the DDPM mix of a frozen encoder's latent runs in the backbone's kernel."""
    B, dev = x_1.size(0), x_1.device
    if args.backbone == "flowmatching":
        t = torch.round(torch.rand(B, device=dev) * args.total_step) / args.total_step
        x_0 = torch.randn_like(x_1)
        tt = t[:, None, None]
        return tt * x_1 + (1 - tt) * x_0, t, x_1 - x_0
    t = torch.floor(torch.rand(B).to(dev) * args.total_step).long()
    eps = torch.randn_like(x_1).float()
    if x_1.requires_grad:
        x_t = backbone._sqrt_ab[t][:, None, None] * x_1 + backbone._sqrt_1mab[t][:, None, None] * eps
    else:
        x_t, _ = backbone.q_sample(x_1, t, eps)
    return x_t, t, eps


def train_step(args, model, backbone, optimizer, x, emb):
    """One optimisation step on one length group (mytrain.py:62-85) -> its loss (device scalar)."""
    if args.usepretrainedvae:
        with torch.no_grad():
            x_1, _ = model.encoder(x)          # series -> clean latent (B,64,flow_dim)
    else:
        x_1, _ = model.encoder(x)
    x_t, t, target = noisy_latent(args, backbone, x_1)
    optimizer.zero_grad()
    if bool(torch.rand(1) < 0.3):              # the CFG coin: this group trains the text-free branch
        emb = None
    pred = model(input=x_t, t=t, text_input=emb)
    loss = mse_loss(pred, target)
    loss.backward()
    optimizer.step()
    return loss.detach()


def train(args):
    """-> the per-epoch mean losses of this run (after those of a resumed checkpoint)."""
    if not torch.cuda.is_available():
        sys.exit("mytrain.py: no GPU visible -- this build runs the HIP path only (no CPU fallback)")
    device = torch.device(f"cuda:{torch.cuda.current_device()}")
    from model.backbone.DDPM import DDPM
    from model.backbone.rectified_flow import RectifiedFlow
    print(f"Training config::\tepoch: {args.epochs}\tsave_path: {args.checkpoint_dir}\tdevice: {device}")
    os.makedirs(args.checkpoint_dir, exist_ok=True)
    if args.synthetic > 0:
        train_loader = synthetic_loader(args)
    else:
        train_loader, _ = dataset_module(args.dataset_name).loader_provider(args)
    if len(train_loader) == 0:
        sys.exit("mytrain.py: the train split holds no full batch (lower --batch_size)")
    model, _vae = load_models(args, device)
    backbone = RectifiedFlow() if args.backbone == "flowmatching" else DDPM(args.total_step, device)
    print(f"Training arithmetic: {'bf16 mixed precision (fp32 master weights, statistics and gradients)' if args.bf16 else 'fp32'}")
    print(f"Total learnable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
    print(f"VAE learnable parameters: {sum(p.numel() for p in model.encoder.parameters() if p.requires_grad)}")
    optimizer = T2SAdamW(model.parameters(), lr=1e-4, weight_decay=0.0)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=1e-4, total_steps=len(train_loader) * args.epochs)
    loss_list, start_epoch = [], 0
    if args.checkpoint_path:
        checkpoint = torch.load(args.checkpoint_path, map_location=device)
        model.load_state_dict(checkpoint["model"])
        optimizer.load_state_dict(checkpoint["optimizer"])
        start_epoch = checkpoint["epoch"] + 1
        loss_list = list(checkpoint["loss_list"])
    model.train()
    steps_done, stop = 0, False
    for epoch in range(start_epoch, args.epochs):
        group_losses = []
        for batch in train_loader:
            for group in batch:
                which = motion_cli.embedding_index(len(group), args.embedding)
                x = group[1].float().to(device)
                emb = group[which].float().to(device)
                group_losses.append(train_step(args, model, backbone, optimizer, x, emb))
                steps_done += 1
                stop = bool(args.max_steps) and steps_done >= args.max_steps
                if stop:
                    break
            if stop:
                break
            scheduler.step()
        loss_list.append(float(torch.stack(group_losses).mean()))     # one device read per epoch
        print(f"[Epoch {epoch}] loss: {loss_list[-1]:.5f}")
        if epoch % 100 == 0 or epoch == args.epochs - 1:
            path = checkpoint_file(args, epoch)
            print(f"Saving model {epoch} to {path}...")
            torch.save(dict(model=model.state_dict(), optimizer=optimizer.state_dict(), epoch=epoch, loss_list=loss_list), path)
        if stop:
            break
    args.model = model          # (for callers that go on with the trained module)
    return loss_list


def main(argv=None):
    args = get_args(argv)
    seed_everything(args.general_seed)
    losses = train(args)
    print("Training complete.")
    return losses


if __name__ == "__main__":
    main()
