"""What tests/test_tsae_host.py and tests/test_tsae.py share: tests/golden/tsae.npz read back (gen_golden_tsae.py wrote it from
the reference), the seeded weights and inputs of its cases, and mirror modules built from them -- each made once."""
import functools
import json
import os
import types

import numpy as np
import torch

from t2ms_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsae.npz")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["plan"]))


def cases():
    return golden()[1]["cases"]


def case_key(c):
    return f"{c['cfg']}_T{c['T']}_B{c['B']}"


def case_ids():
    return [case_key(c) for c in cases()]


def cfg_of(c):
    return golden()[1]["cfgs"][c["cfg"]]


@functools.lru_cache(maxsize=None)
def state_dict(cfg, fusion=False):
    k = golden()[1]["cfgs"][cfg]
    return synth.make_tsae_state_dict(k["seed"], k["n_features"], k["d_ff"], k["n_enc"], k["n_dec"], k["heads"], fusion=fusion)


def case_input(c):
    k = cfg_of(c)
    return synth.make_tsae_series(100 * c["T"] + 7 * c["B"] + k["seed"], c["B"], c["T"], k["n_features"])


def expected(c, name):
    return torch.from_numpy(golden()[0][f"{name}_{case_key(c)}"])


def bar(ref):
    """The bar of every comparison: 1e-5 * max(1, max|reference output|)."""
    return golden()[1]["bar"] * max(1.0, float(ref.abs().max()))


def args_of(cfg):
    k = golden()[1]["cfgs"][cfg]
    return types.SimpleNamespace(input_dim=k["n_features"], flow_dim=64, num_encoder_layers=k["n_enc"],
                                 num_decoder_layers=k["n_dec"], d_ff=k["d_ff"], num_heads=k["heads"])


@functools.lru_cache(maxsize=None)
def mirror(cfg, device="cpu"):
    """The mirror with the configuration's weights, in eval mode.  The fusion block keeps its own initialisation: the recorded
    paths never read it (strict loading of a full reference state dict is a test of its own)."""
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    m = AttentionSeq2SeqAutoencoder(args_of(cfg))
    missing, unexpected = m.load_state_dict(state_dict(cfg), strict=False)
    assert not unexpected and all(k.startswith("condition_fusion.") for k in missing), (missing, unexpected)
    m.condition_fusion = None            # 25 M unused parameters: not worth a device copy
    return m.to(device).eval()
