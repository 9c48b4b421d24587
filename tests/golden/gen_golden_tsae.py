#!/usr/bin/env python3
"""Generate tests/golden/tsae.npz by RUNNING THE REFERENCE's attention seq2seq codec (model/pretrained/TSae.py, imported
unmodified) on the CPU.  Run with the reference checkout at hand:

    MKL_CBWR=COMPATIBLE,STRICT PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tsae.py --reference DIR

(MKL_CBWR: see gen_golden.py.)  The reference never travels: only the arrays written below are committed.  Weights and inputs are
regenerated from seeds by ``t2ms_amd.synth``, so the file holds OUTPUTS only, plus -- as one JSON string under "plan" -- the
weight configurations, the recorded cases, the reference module's state-dict key names and shapes and two samples of its
positional buffer (pe[:, :8] and pe[:, 1999]).

Per case (cfg, T, B): memory (B,T,64) = encoder(x), pred (B,T,F) = decoder(memory, x) (teacher forcing), gen (B,T,F) =
forward_inference(x, None), loss = shared_eval(x, None, None, 'test')[0]; and dev_memory / dev_pred / dev_gen, the largest
absolute deviation of each output between the reference in fp32 and the same module in fp64.  The tests hold every
implementation to BAR = 1e-5 * max(1, max|output|); a case whose fp32-vs-fp64 deviation exceeds a quarter of that is refused
here, not written: the reference itself would not be a witness for it.
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

# "bp": the bench-press `vae:` block of the reference's config.yaml
CFGS = {
    "bp": dict(n_features=10, d_ff=128, n_enc=3, n_dec=3, heads=8, seed=3101),
    "f7": dict(n_features=7, d_ff=128, n_enc=3, n_dec=3, heads=8, seed=3102),
    "f16": dict(n_features=16, d_ff=128, n_enc=3, n_dec=3, heads=8, seed=3103),
    "h4": dict(n_features=10, d_ff=256, n_enc=1, n_dec=1, heads=4, seed=3104),
}
BAR = 1e-5


def plan_cases():
    cases = [dict(cfg="bp", T=T, B=B) for T in (1, 2, 8, 37, 65, 144) for B in (1, 3)]   # 1: BOS only; 65: past a 64-row tile
    cases.append(dict(cfg="bp", T=300, B=1))                                             # past 256
    cases += [dict(cfg="f7", T=37, B=2), dict(cfg="f16", T=37, B=2)]
    cases += [dict(cfg="h4", T=8, B=2), dict(cfg="h4", T=37, B=2)]
    return cases


def case_key(c):
    return f"{c['cfg']}_T{c['T']}_B{c['B']}"


def case_input(synth, c):
    """x (B,T,F) of a case: a function of the case alone."""
    return synth.make_tsae_series(100 * c["T"] + 7 * c["B"] + CFGS[c["cfg"]]["seed"], c["B"], c["T"], CFGS[c["cfg"]]["n_features"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (Bill9125/T2MS)")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    torch.set_num_threads(8)
    from t2ms_amd import synth
    # the repo's own `model/` package would shadow the reference's: take the repo off the path once synth is imported
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for k in [k for k in sys.modules if k.split(".")[0] == "model"]:
        del sys.modules[k]
    os.chdir(HERE)
    sys.path.insert(0, ref)
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    assert sys.modules["model.pretrained.TSae"].__file__.startswith(ref + os.sep), sys.modules["model.pretrained.TSae"].__file__

    models = {}

    def model(cfg):
        if cfg not in models:
            k = CFGS[cfg]
            ns = types.SimpleNamespace(input_dim=k["n_features"], flow_dim=64, num_encoder_layers=k["n_enc"],
                                       num_decoder_layers=k["n_dec"], d_ff=k["d_ff"], num_heads=k["heads"])
            m = AttentionSeq2SeqAutoencoder(ns).eval()
            m.load_state_dict(synth.make_tsae_state_dict(k["seed"], k["n_features"], k["d_ff"], k["n_enc"], k["n_dec"], k["heads"],
                                                         fusion=True), strict=True)
            m.condition_fusion = None                      # never called by the recorded paths; not worth a double copy
            models[cfg] = (m, copy.deepcopy(m).double().eval())
        return models[cfg]

    out, cases, worst = {}, plan_cases(), 0.0
    ref_model = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=10, flow_dim=64, num_encoder_layers=3,
                                                                  num_decoder_layers=3, d_ff=128, num_heads=8))
    ref_sd = ref_model.state_dict()
    pe = ref_sd["encoder.positional_encoding.pe"]
    assert torch.equal(pe, ref_sd["decoder.positional_encoding.pe"]) and tuple(pe.shape) == (1, 2000, 64)
    with torch.no_grad():
        for c in cases:
            m32, m64 = model(c["cfg"])
            key, x = case_key(c), case_input(synth, c)
            res = {}
            for tag, m, xx in (("32", m32, x), ("64", m64, x.double())):
                memory = m.encoder(xx)
                pred = m.decoder(memory, xx)
                gen = m.forward_inference(xx, None)
                res[tag] = dict(memory=memory, pred=pred, gen=gen)
            loss, recon = m32.shared_eval(x, None, None, "test")
            assert torch.equal(recon, res["32"]["gen"])
            for name in ("memory", "pred", "gen"):
                a, b = res["32"][name], res["64"][name]
                dev = float((a.double() - b).abs().max())
                bar = BAR * max(1.0, float(a.abs().max()))
                if not dev <= bar / 4:
                    raise SystemExit(f"{key} {name}: the reference's own fp32-vs-fp64 deviation {dev:.3e} exceeds a quarter of the "
                                     f"bar {bar:.3e}; this case cannot be recorded")
                worst = max(worst, dev / bar)
                out[f"{name}_{key}"] = a.numpy()
                out[f"dev_{name}_{key}"] = np.float64(dev)
            out[f"loss_{key}"] = np.float64(float(loss))
            print(f"{key}: max|memory| {float(res['32']['memory'].abs().max()):.2f} max|gen| {float(res['32']['gen'].abs().max()):.2f} "
                  f"dev {[out[f'dev_{n}_{key}'].item() for n in ('memory', 'pred', 'gen')]}")
    plan = dict(cfgs=CFGS, cases=cases, bar=BAR, state_dict_bp={k: list(v.shape) for k, v in ref_sd.items()},
                pe_head=pe[0, :8].double().tolist(), pe_last=pe[0, 1999].double().tolist())
    arrs = dict(out)
    arrs["plan"] = np.asarray(json.dumps(plan))
    path = os.path.join(args.out, "tsae.npz")
    np.savez_compressed(path, **arrs)
    print(f"tsae.npz  {os.path.getsize(path) / 1024:.1f} KiB, {len(cases)} cases, worst fp32-vs-fp64 deviation {worst:.3f} of the bar")


if __name__ == "__main__":
    main()
