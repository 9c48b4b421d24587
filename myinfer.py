#!/usr/bin/env python3
"""Drop-in for the reference's myinfer.py: sample the test split of a T2MS motion dataset (bench press / deadlift) with the
wide-latent DiT and the multichannel LA-VAE, every clip at ITS OWN length, in one sampling job.

    python myinfer.py --dataset_name benchpress --cfg_scale 3 --total_step 100 --checkpoint_id 2500
    python myinfer.py --dataset_name deadlift --random_init --synthetic 64 --reconstruct --save_path /tmp/out

The reference walks the test loader at batch_size 1 -- clip lengths differ, so it cannot stack them -- and runs one
1024-token (800 for deadlift) sampling loop per clip.  The latent of a run is (B,64,W) whatever the clip length; only the
decode depends on it.  Here all clips ride in launches of up to `--launch_batch` rows through ONE fused Sampler whose final
decode takes a length per row (Sampler.run(lengths=...), t2s_vae_decode_mc_ragged).  Row seeds are per clip index
(Sampler.set_rows: key row = the clip's index in the split), so a clip's sample does not depend on the launch it rides in.

What differs from the reference, on purpose:
  * conditioning: each clip is conditioned on the embedding STORED in its caption.json (`--embedding summary|prefix` for bench
    press; deadlift stores one).  The reference re-embeds the summary through a network service at inference time; that fetch
    is not reproduced.
  * outputs: per clip `sample_<i>/x_t.npy` (C, T_i) and `sample_<i>/data.json` (feature name -> list), as the reference's
    save_result writes them, without GIFs and plots; plus `summary.json` with the reference's per-clip normalised MSE
    (myevaluation.normalize + calculate_mse).  `--reconstruct` adds the codec's reconstruction of every clip (ragged encode ->
    ragged decode), `sample_<i>/x_rec.npy`, and its MSE.
  * every clip of the split is sampled (the reference stops after 11); `--max_clips N` caps it.
  * `--math bf16x3|bf16` runs the denoiser's matrix products on the bf16 matrix cores (fp32-accurate split / single pass);
    the default stays f32, and summary.json names the arithmetic only when it is not f32.
  * `--save_eval_files` additionally writes `run_<j>/x_t_sample_<i>.npy` and, once, `x_1_sample_<i>.npy` next to the run
    directories: the names the reference's myevaluation.py reads (its own myinfer.py never writes them), so that it runs
    unchanged on this output; myevaluation.py here reads either layout.
  * `--random_init` (seeded synthetic weights) and `--synthetic N` (N seeded clips of 30..160 samples instead of a dataset)
    let the driver run without checkpoints or data, as infer.py's flags do.
The model shape comes from flags whose defaults are the reference's config.yaml values per dataset; `--config FILE` overrides
them from a YAML file when PyYAML is installed (it is not a dependency).  mytrain.py trains the checkpoints this driver
loads; both resolve their flags and paths through t2ms_amd/motion_cli.py.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from datafactory.motion import dataset_module        # noqa: E402
from t2ms_amd import motion_cli                      # noqa: E402
from t2ms_amd.motion_cli import FEATURES, PRETRAINED_EPC        # noqa: E402,F401


def normalize(x):
    """myevaluation.normalize: min-max per row (channel) along time."""
    lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    return (x - lo) / (hi - lo + 1e-8)


def clip_mse(x_1, x_t):
    """The reference's per-clip figure, calculate_mse(normalize(x_1)[None], normalize(x_t)[None]) on (C,T) arrays: the squared
    difference of the normalised channels, averaged over channels per time step and then over time."""
    d = normalize(x_1) - normalize(x_t)
    return float((d * d).mean(axis=0).mean())


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Sample a motion test split (reference myinfer.py)")
    # the reference's command line
    p.add_argument("--batch_size", type=int, default=1, help="accepted as in the reference; launches are sized by --launch_batch")
    p.add_argument("--save_path", type=str, default="./results/denoiser_results", help="root of checkpoints/ and generation/")
    p.add_argument("--cfg_scale", type=int, default=3, help="CFG scale")
    p.add_argument("--total_step", type=int, default=100, help="sampling steps")
    p.add_argument("--checkpoint_id", type=int, default=2500, help="model id")
    p.add_argument("--dataset_name", type=str, choices=["deadlift", "benchpress"], required=True, help="dataset name")
    p.add_argument("--run_time", type=int, default=1, help="number of runs (run_<i>; run i draws with general_seed + i)")
    motion_cli.add_config_flags(p)       # --config and config.yaml's values as flags, --embedding, --random_init
    # this driver's own
    p.add_argument("--launch_batch", type=int, default=64, help="clips per sampling launch")
    p.add_argument("--split", choices=["test", "train", "all"], default="test", help="which part of the 0.9 / 0.1 split to sample")
    p.add_argument("--max_clips", type=int, default=0, help="sample at most N clips (0: all)")
    p.add_argument("--reconstruct", action="store_true", help="also the codec reconstruction of every clip and its MSE")
    p.add_argument("--synthetic", type=int, default=0, help="N seeded synthetic clips (30..160 samples) instead of the dataset")
    p.add_argument("--no_graph", action="store_true", help="run the loop eagerly (same bits)")
    p.add_argument("--save_eval_files", action="store_true",
                   help="also write run_<j>/x_t_sample_<i>.npy and, once, x_1_sample_<i>.npy: the names the reference's myevaluation.py reads")
    p.add_argument("--math", choices=["f32", "bf16x3", "bf16"], default="f32",
                   help="matrix arithmetic of the denoiser: f32 (default), bf16x3 (fp32-accurate, bf16 matrix cores) or bf16 "
                        "(single pass, not fp32-accurate); the latter two opt the wide model in (Transformer.set_wide_math)")
    args = p.parse_args(argv)
    if args.launch_batch < 1:
        p.error("--launch_batch must be >= 1")
    name = args.dataset_name
    motion_cli.resolve(args, "myinfer.py")
    args.checkpoint_path = motion_cli.checkpoint_file(args, args.checkpoint_id)
    args.generation_save_path = os.path.join(args.save_path, "generation", "{}_{}_{}_{}_{}".format(
        args.backbone, args.denoiser, name, args.cfg_scale, args.total_step))
    return args


def load_models(args, device):
    """(denoiser with the codec's encoder grafted on, codec), as myinfer.py:126-137."""
    from model.denoiser.mytransformer import Transformer
    from model.pretrained.myvqvae import vqvae
    from t2ms_amd import synth
    vae = vqvae(args)
    model = Transformer(args.flow_dim)
    if args.random_init:
        vae.load_state_dict(synth.make_mvae_state_dict(args.general_seed, args.input_dim, args.block_hidden_size,
                                                       args.num_residual_layers, args.res_hidden_size), strict=True)
        model.load_state_dict(synth.make_dit_state_dict(args.general_seed, width=args.flow_dim), strict=True)
        model.encoder = vae.encoder
    else:
        vae.load_state_dict(torch.load(args.pretrainedvae_path, map_location="cpu"))
        model.encoder = vae.encoder
        model.load_state_dict(torch.load(args.checkpoint_path, map_location="cpu")["model"])
    if args.math != "f32":               # (mytrain.py has no such flag: wide training is fp32)
        model.set_wide_math(True).set_math(args.math)
    return model.to(device).float().eval(), vae.to(device).float().eval()


def load_clips(args):
    """[(x (C,T) float32 CPU tensor, embedding (128,), subject, text)] of the split, in split order."""
    if args.synthetic > 0:
        rng = np.random.RandomState(args.general_seed)
        lengths = rng.randint(30, 161, size=args.synthetic)
        from t2ms_amd import synth
        text = synth.make_text_embeddings(args.general_seed, args.synthetic)
        return [(synth.make_mseries(args.general_seed + i, 1, args.input_dim, int(n))[0], text[i], "synthetic", f"synthetic/{i}")
                for i, n in enumerate(lengths)]
    train_loader, test_loader = dataset_module(args.dataset_name).loader_provider(args, period="test")
    if args.split == "all":
        records = list(test_loader.dataset.dataset.records)
    else:
        part = (test_loader if args.split == "test" else train_loader).dataset
        records = [part[i] for i in range(len(part))]
    which = motion_cli.embedding_index(len(records[0]), args.embedding)
    clips = [(r[1], r[which], r[-1], r[0]) for r in records]
    for x, _, subject, _ in clips:
        if x.shape[0] != args.input_dim:
            sys.exit(f"myinfer.py: a clip of {subject} has {x.shape[0]} channels, --input_dim is {args.input_dim}")
    return clips


def sample_clips(sampler, clips, device):
    """Every clip's sample (C, T_i), CPU numpy, in launches of sampler.batch rows.  A short last launch is padded with
    empty rows (length 0: nothing is decoded for them)."""
    B, out = sampler.batch, []
    for start in range(0, len(clips), B):
        part = clips[start:start + B]
        pad = B - len(part)
        lengths = [int(c[0].shape[1]) for c in part] + [0] * pad
        text = torch.stack([c[1].float() for c in part] + [torch.zeros(128)] * pad).to(device)
        sampler.set_rows(seeds=[sampler.seed] * B, key_rows=[start + r for r in range(B)])      # a clip's noise: its own index
        _, rows, _ = sampler.run(text, lengths=lengths)
        out += [r.cpu().numpy() for r in rows[:len(part)]]
    return out


def reconstruct_clips(vae, clips, device, launch_batch):
    """Every clip through the codec at its own length: ragged encode -> ragged decode."""
    out = []
    for start in range(0, len(clips), launch_batch):
        xs = [c[0].to(device) for c in clips[start:start + launch_batch]]
        z = vae.encoder.encode_ragged(xs)
        out += [r.cpu().numpy() for r in vae.decoder.decode_ragged(z, [x.shape[1] for x in xs])]
    return out


def infer(args, run, device, model, vae, clips):
    from t2ms_amd.sampler import Sampler
    root = os.path.join(args.generation_save_path, f"run_{run}")
    os.makedirs(root, exist_ok=True)
    names = args.features[-args.input_dim:]
    print(f"Inference config::Step: {args.total_step}\t CFG Scale: {args.cfg_scale}\t clips: {len(clips)}")
    B = min(args.launch_batch, len(clips))
    max_len = max(int(c[0].shape[1]) for c in clips)
    sampler = Sampler(model, vae.decoder, args.backbone, args.total_step, float(args.cfg_scale), B, max_len, device,
                      use_graph=not args.no_graph, seed=args.general_seed + run)
    samples = sample_clips(sampler, clips, device)
    recons = reconstruct_clips(vae, clips, device, args.launch_batch) if args.reconstruct else None
    rows = []
    for i, (clip, x_t) in enumerate(zip(clips, samples)):
        x_1 = clip[0].numpy()
        d = os.path.join(root, f"sample_{i}")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "x_t.npy"), x_t)
        if args.save_eval_files:
            np.save(os.path.join(root, f"x_t_sample_{i}.npy"), x_t)
            if run == 0:
                np.save(os.path.join(args.generation_save_path, f"x_1_sample_{i}.npy"), x_1)
        with open(os.path.join(d, "data.json"), "w") as f:
            json.dump({name: x_t[c].astype(float).tolist() for c, name in enumerate(names)}, f, indent=4)
        row = dict(index=i, subject=clip[2], text=clip[3], length=int(x_1.shape[1]), mse=clip_mse(x_1, x_t))
        if recons is not None:
            np.save(os.path.join(d, "x_rec.npy"), recons[i])
            row["recon_mse"] = clip_mse(x_1, recons[i])
        rows.append(row)
    summary = dict(dataset=args.dataset_name, channels=args.input_dim, features=names, backbone=args.backbone,
                   total_step=args.total_step, cfg_scale=args.cfg_scale, seed=args.general_seed + run, launch_batch=B,
                   embedding=args.embedding, mean_mse=float(np.mean([r["mse"] for r in rows])), clips=rows)
    if sampler.math != "f32":            # (f32 runs keep the summary they have always written)
        summary["math"] = sampler.math
    with open(os.path.join(root, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(f"run {run}: {len(rows)} clips, mean normalised MSE {summary['mean_mse']:.6f} -> {root}")
    return summary


def main(argv=None):
    args = get_args(argv)
    if not torch.cuda.is_available():
        sys.exit("myinfer.py: no GPU visible -- this build runs the HIP path only (no CPU fallback)")
    device = torch.device(f"cuda:{torch.cuda.current_device()}")
    clips = load_clips(args)
    if args.max_clips > 0:
        clips = clips[:args.max_clips]
    if not clips:
        sys.exit("myinfer.py: the split holds no clip")
    model, vae = load_models(args, device)
    with torch.no_grad():
        return [infer(args, run, device, model, vae, clips) for run in range(args.run_time)]


if __name__ == "__main__":
    main()
