#!/usr/bin/env python3
"""Generate the motion-loader fixtures: the synthetic datasets under tests/golden/motion_ds/ (always, from seeds) and, with the
reference checkout at hand, tests/golden/motion_loader.npz by RUNNING THE REFERENCE's dataset classes and loader_provider
(datafactory/benchpress, datafactory/deadlift, imported unmodified) on them:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_motion_loader.py --reference DIR

The reference never travels: only the JSON datasets and the arrays written below are committed.

Datasets (the reference's format: <name>/data.json = {subject: {clip: {feature: [T floats]}}} and
<name>/<caption>/<subject>/<clip>/caption.json = {"Summary", embeddings}), two subjects of ten clips each:
  bench press  13 features (feature_0..2 are dropped by the loader), lengths around the group thresholds 57 | 58 and 77 | 78,
               both resampling directions and the identity in every group (36 / 72 / 144), plus one clip whose features
               disagree in length; Prefix_embedding / Summary_embedding, 128 floats each;
  deadlift     7 features, lengths around 80 | 81 and 98 | 99 (groups 48 / 96 / 192), plus one clip of 9 samples and one with
               inconsistent lengths; embedding, 128 floats.
Every Summary starts with "<subject>/<clip>", so a record names its clip.

motion_loader.npz, per dataset <d>, under general_seed 2025:
  <d>_train<g>_x (N,C,L), <d>_train<g>_emb<k> (N,128), g = 0..2: the records of the reference class built for group g;
  <d>_test_x (sum of C*T_i), <d>_test_len (N), <d>_test_emb<k>: the records of period 'test', series end to end;
  <d>_split_train_train / _split_train_test / _split_test_train / _split_test_test: the indices of random_split
  (period, part) as loader_provider draws them;
  "plan": JSON with the clip names of every record list above, in order.
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "motion_ds")
SEED = 2025
SPECS = {
    "benchpress": dict(caption="Caption_explain_no_barbell_length", base=36, features=[f"feature_{i}" for i in range(13)],
                       embeddings=("Prefix_embedding", "Summary_embedding"), cls="BenchpressT2SDataset",
                       subjects={"S01_correct": [20, 36, 57, 58, 60, 77, 78, 90, 144, 150],
                                 "S02_elbows_flaring_tilting_to_the_left": [57, 30, 72, 58, 77, 40, 78, 100, 160, 36]},
                       odd={"S02_elbows_flaring_tilting_to_the_left": ("clip_10", "ragged", 40)}),
    "deadlift": dict(caption="Caption_explain_no_barbell", base=48, features=[f"feature_{i}" for i in range(7)],
                     embeddings=("embedding",), cls="DeadliftT2SDataset",
                     subjects={"D01_correct": [10, 48, 80, 81, 90, 98, 99, 120, 192, 200],
                               "D02_Lower_back_rounding": [80, 30, 96, 81, 98, 60, 99, 110, 48, 130]},
                     odd={"D01_correct": ("clip_10", "short", 9), "D02_Lower_back_rounding": ("clip_10", "ragged", 50)}),
}


def write_datasets():
    for d, (name, spec) in enumerate(SPECS.items()):
        rng = np.random.RandomState(SEED + d)
        data = {}
        for subject, lengths in spec["subjects"].items():
            clips = {f"clip_{i}": ("plain", T) for i, T in enumerate(lengths)}
            if subject in spec["odd"]:
                clip, kind, T = spec["odd"][subject]
                clips[clip] = (kind, T)
            data[subject] = {}
            for clip, (kind, T) in clips.items():
                feats = {}
                for k, f in enumerate(spec["features"]):
                    n = T - 3 if kind == "ragged" and k == len(spec["features"]) - 1 else T
                    # a slow wave per feature plus noise, one decimal: small files, no two clips alike
                    wave = 5.0 + 3.0 * np.sin(np.arange(n) * (0.05 + 0.01 * k) + rng.uniform(0, 6.28)) + rng.normal(0, 0.4, n)
                    feats[f] = [float(v) for v in np.round(wave, 1)]
                data[subject][clip] = feats
                cap = {"Summary": f"{subject}/{clip}: a synthetic {name} repetition of {T} samples ({kind})."}
                for key in spec["embeddings"]:
                    cap[key] = [float(v) for v in np.round(rng.normal(0, 0.09, 128), 3)]
                cdir = os.path.join(ROOT, name, spec["caption"], subject, clip)
                os.makedirs(cdir, exist_ok=True)
                with open(os.path.join(cdir, "caption.json"), "w", encoding="utf-8") as fh:
                    json.dump(cap, fh, separators=(",", ":"))
        with open(os.path.join(ROOT, name, "data.json"), "w", encoding="utf-8") as fh:
            json.dump(data, fh, separators=(",", ":"))


def loader_args(name, batch_size=1):
    spec = SPECS[name]
    return types.SimpleNamespace(dataset_root=ROOT, dataset_name=name, caption=spec["caption"], embedding_dim=64,
                                 split_base_num=spec["base"], general_seed=SEED, batch_size=batch_size)


def clip_of(record):
    return record[0].split(":")[0]


def record_arrays(prefix, records, out, flat=False):
    """The series and embeddings of a record list under `prefix`; -> the clip names."""
    xs = [r[1].numpy() for r in records]
    if flat:
        out[f"{prefix}_x"] = np.concatenate([x.reshape(-1) for x in xs]) if xs else np.zeros(0, np.float32)
        out[f"{prefix}_len"] = np.asarray([x.shape[1] for x in xs], dtype=np.int64)
    else:
        out[f"{prefix}_x"] = np.stack(xs)
    for k in range(len(records[0]) - 3):
        out[f"{prefix}_emb{k}"] = np.stack([r[2 + k].numpy() for r in records])
    return [clip_of(r) for r in records]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference checkout; without it only the datasets are written")
    a = ap.parse_args()
    write_datasets()
    if not a.reference:
        return
    sys.dont_write_bytecode = True
    # the reference's datafactory under a name of its own (this repository has a datafactory package too)
    pkg = types.ModuleType("t2ms_reference_datafactory")
    pkg.__path__ = [os.path.join(os.path.abspath(a.reference), "datafactory")]
    sys.modules[pkg.__name__] = pkg
    out, plan = {}, {}
    for name, spec in SPECS.items():
        ds_mod = importlib.import_module(f"{pkg.__name__}.{name}.dataset")
        dl_mod = importlib.import_module(f"{pkg.__name__}.{name}.dataloader")
        cls = getattr(ds_mod, spec["cls"])
        args = loader_args(name)
        kw = dict(json_path=os.path.join(ROOT, name, "data.json"), caption_root=os.path.join(ROOT, name, spec["caption"]),
                  emb_dim=64)
        for g, m in enumerate((1, 2, 4)):
            ds = cls(data_dim=spec["base"] * m, period="train", **kw)
            plan[f"{name}_train{g}"] = record_arrays(f"{name}_train{g}", ds.records, out)
        ds = cls(data_dim=0 if name == "deadlift" else spec["base"] * 2, period="test", **kw)
        plan[f"{name}_test"] = record_arrays(f"{name}_test", ds.records, out, flat=True)
        for period in ("train", "test"):
            train_loader, test_loader = dl_mod.loader_provider(args, period=period)
            out[f"{name}_split_{period}_train"] = np.asarray(train_loader.dataset.indices, dtype=np.int64)
            out[f"{name}_split_{period}_test"] = np.asarray(test_loader.dataset.indices, dtype=np.int64)
    out["plan"] = np.asarray(json.dumps(plan))
    np.savez_compressed(os.path.join(HERE, "motion_loader.npz"), **out)
    print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items() if k != "plan"})


if __name__ == "__main__":
    main()
