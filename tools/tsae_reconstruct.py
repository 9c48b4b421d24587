"""Reconstruct motion series with the attention seq2seq codec (model/pretrained/TSae.py): what the reference's
pretrained_mylavae.py --only_inference does, minus the plots.

    python tools/tsae_reconstruct.py (--state_dict FILE | --random_init SEED) (GROUP.npy ... | --synthetic N) [--out DIR]

Every GROUP.npy is one length group, (N,C,L) -- the layout of the datasets; the codec reads it as (N,L,C).  Per group the model's
``shared_eval(batch, None, None, 'test')`` runs (encode, then autoregressive generation in one launch on the HIP kernels) and the
reconstruction is written to DIR/<group>_recon.npy in the input's layout.  One JSON object goes to stdout and DIR/tsae_reconstruct.json:
the per-group MSE.  --synthetic N makes two groups of N seeded U[0,1] series (lengths 36 and 144) instead of files.
"""
import argparse
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--state_dict", metavar="FILE", help="a state dict torch.save'd by the reference (or a whole pickled module)")
    src.add_argument("--random_init", metavar="SEED", type=int, help="seeded weights at the reference's initialisation scale")
    ap.add_argument("groups", nargs="*", metavar="GROUP.npy", help="one (N,C,L) array per length group")
    ap.add_argument("--synthetic", metavar="N", type=int, help="N seeded series per group instead of files")
    ap.add_argument("--input_dim", type=int, default=10)
    ap.add_argument("--flow_dim", type=int, default=64)
    ap.add_argument("--d_ff", type=int, default=128)
    ap.add_argument("--num_encoder_layers", type=int, default=3)
    ap.add_argument("--num_decoder_layers", type=int, default=3)
    ap.add_argument("--num_heads", type=int, default=8)
    ap.add_argument("--batch", type=int, default=128, help="series per shared_eval call")
    ap.add_argument("--out", default="tsae_recon")
    a = ap.parse_args()
    if bool(a.groups) == (a.synthetic is not None):
        ap.error("give GROUP.npy files or --synthetic N (one of the two)")

    import numpy as np
    import torch

    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    from t2ms_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("tsae_reconstruct: needs a GPU (the HIP codec has no CPU fallback)")
    dev = torch.device("cuda:0")
    m = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=a.input_dim, flow_dim=a.flow_dim, d_ff=a.d_ff,
                                                          num_encoder_layers=a.num_encoder_layers,
                                                          num_decoder_layers=a.num_decoder_layers, num_heads=a.num_heads))
    if a.state_dict is not None:
        sd = torch.load(a.state_dict, map_location="cpu", weights_only=False)
        sd = sd.state_dict() if hasattr(sd, "state_dict") else sd
        m.load_state_dict(sd, strict=True)
    else:
        sd = synth.make_tsae_state_dict(a.random_init, a.input_dim, a.d_ff, a.num_encoder_layers, a.num_decoder_layers, a.num_heads,
                                        d_model=a.flow_dim)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("condition_fusion.") for k in missing), (missing, unexpected)
    m.condition_fusion = None                  # never read by shared_eval: no device copy of its 25 M parameters
    m = m.to(dev).eval()

    if a.synthetic is not None:
        groups = [(f"synthetic_L{Ln}", synth.make_mseries(a.random_init or 0, a.synthetic, a.input_dim, Ln).numpy()) for Ln in (36, 144)]
    else:
        groups = [(os.path.splitext(os.path.basename(p))[0], np.load(p)) for p in a.groups]
    os.makedirs(a.out, exist_ok=True)
    report = {"groups": {}}
    for name, arr in groups:
        if arr.ndim != 3 or arr.shape[1] != a.input_dim:
            raise SystemExit(f"tsae_reconstruct: {name} must be (N,{a.input_dim},L), got {arr.shape}")
        x = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).permute(0, 2, 1).contiguous()
        recon, sq = [], 0.0
        for i in range(0, x.shape[0], a.batch):
            batch = x[i:i + a.batch].to(dev)
            loss, r = m.shared_eval(batch, None, None, "test")
            recon.append(r.cpu())
            sq += float(loss) * batch.numel()
        rec = torch.cat(recon).permute(0, 2, 1).contiguous().numpy()
        np.save(os.path.join(a.out, f"{name}_recon.npy"), rec)
        report["groups"][name] = {"n": int(x.shape[0]), "length": int(x.shape[1]), "mse": sq / x.numel(),
                                  "finite": bool(np.isfinite(rec).all())}
    with open(os.path.join(a.out, "tsae_reconstruct.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
