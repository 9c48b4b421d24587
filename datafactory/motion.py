"""The T2MS motion datasets (reference datafactory/benchpress, datafactory/deadlift), once: what the two loader packages
share.  One-off host work on the CPU -- JSON parsing and two torch CPU resampling ops per clip -- so no HIP kernel.

A dataset is ``<dataset_root>/<dataset_name>/data.json`` ({subject: {clip: {feature: [T floats]}}}) plus one
``<caption>/<subject>/<clip>/caption.json`` per clip (the text under "Summary" and the stored 128-float text embeddings).
What a dataset class does per clip, in the reference's order:

  * features named in ``SKIP`` are left out (bench press: feature_0..2, the barbell channels);
  * a clip whose remaining features differ in length (or that has none left) is dropped;
  * a clip shorter than ``MIN_T`` is dropped (deadlift: 10), in every period;
  * period 'train': the clip belongs to ONE length group -- ``BASE`` x 1 below ``BOUNDS[0]``, x 2 from there to below
    ``BOUNDS[1]``, x 4 from there on -- and a dataset built for ``data_dim`` keeps only its group's clips, aligned to
    data_dim samples with the same torch CPU ops: adaptive_avg_pool1d down, linear interpolation (align_corners) up;
  * period 'test': clips keep their own lengths.

A record is (text, x (C,T) float32, *embeddings (128,) float32, subject), the tuple the reference's loops unpack.
"""
import json
import os

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset, random_split

# config.yaml of the reference, per dataset: what a driver needs to find and read one
DEFAULTS = {
    "benchpress": dict(input_dim=10, flow_dim=64, split_base_num=36, caption="Caption_explain_no_barbell_length"),
    "deadlift": dict(input_dim=7, flow_dim=50, split_base_num=48, caption="Caption_explain_no_barbell"),
}


class MotionT2SDataset(Dataset):
    SKIP = ()                 # feature names that are not channels
    MIN_T = 0                 # shorter clips are dropped
    BASE = 0                  # the shortest length group
    BOUNDS = (0, 0)           # first clip length of the second / third group
    EMBEDDINGS = ()           # caption.json keys that travel with the record

    def __init__(self, json_path, caption_root, period, emb_dim=128, data_dim=0):
        super().__init__()
        self.period, self.data_dim, self.emb_dim = period, int(data_dim), int(emb_dim)
        self.records, self.dropped = [], []           # dropped: (subject, clip, why) of every clip that left no record
        with open(json_path, "r", encoding="utf-8") as f:
            subjects = json.load(f)
        for subject, clips in subjects.items():
            for clip, features in clips.items():
                with open(os.path.join(caption_root, subject, clip, "caption.json"), "r", encoding="utf-8") as f:
                    caption = json.load(f)
                x, why = self._series(features)
                if x is None:
                    self.dropped.append((subject, clip, why))
                    continue
                embeddings = tuple(torch.as_tensor(caption[k], dtype=torch.float32) for k in self.EMBEDDINGS)
                self.records.append((caption["Summary"], x, *embeddings, subject))

    def _series(self, features):
        """(x (C,T) or None, why it was dropped)."""
        rows = []
        for name, values in features.items():
            if name in self.SKIP:
                continue
            row = torch.as_tensor(values, dtype=torch.float32)
            if row.dim() != 1:
                raise ValueError(f"Feature '{name}' must be [T], got {tuple(row.size())}")
            rows.append(row)
        if len({r.numel() for r in rows}) != 1:
            return None, "inconsistent feature lengths"
        x = torch.stack(rows, dim=0)
        T = x.shape[1]
        if T < self.MIN_T:
            return None, f"shorter than {self.MIN_T}"
        if self.period != "train":
            return x, ""
        target = self._map_target_len(T, self.data_dim)
        if not target:
            return None, "another length group"
        if target < T:
            x = F.adaptive_avg_pool1d(x.unsqueeze(0), output_size=target).squeeze(0)
        elif target > T:
            x = F.interpolate(x.unsqueeze(0), size=target, mode="linear", align_corners=True).squeeze(0)
        return x, ""

    def _map_target_len(self, T, target_T):
        """target_T when a clip of T samples belongs to the group of target_T, else 0."""
        lo, hi = self.BOUNDS
        groups = {self.BASE: T < lo, 2 * self.BASE: lo <= T < hi, 4 * self.BASE: T >= hi}
        if target_T not in groups:
            raise ValueError(f"Undefined length {target_T}.")
        return target_T if groups[target_T] else 0

    def __len__(self):
        return len(self.records)

    def __getitem__(self, idx):
        return self.records[idx]


class AlternatingDataset(Dataset):
    """The three length groups end to end: item i is (record, group index)."""

    def __init__(self, dataset1, dataset2, dataset3):
        self.datasets = [dataset1, dataset2, dataset3]
        self.lengths = [len(d) for d in self.datasets]
        self.total_length = sum(self.lengths)
        self.index_map = {}
        for g, n in enumerate(self.lengths):
            start = sum(self.lengths[:g])
            self.index_map.update({start + j: (g, j) for j in range(n)})

    def __len__(self):
        return self.total_length

    def __getitem__(self, index):
        g, j = self.index_map[index]
        return self.datasets[g][j], g


def custom_collate_fn(batch):
    """One entry per length group present in the batch, groups in order: (texts, xs (n,C,L), *embeddings (n,128), subjects)."""
    out = []
    for g in range(3):
        members = [record for record, group in batch if group == g]
        if not members:
            continue
        columns = list(zip(*members))
        texts, xs, subjects = list(columns[0]), torch.stack(columns[1]), list(columns[-1])
        out.append((texts, xs, *(torch.stack(c) for c in columns[2:-1]), subjects))
    return out


def _paths(args):
    root = os.path.join(args.dataset_root, args.dataset_name)
    return os.path.join(root, "data.json"), os.path.join(root, args.caption)


def _group_datasets(cls, args):
    json_path, caption_root = _paths(args)
    return [cls(json_path=json_path, caption_root=caption_root, emb_dim=getattr(args, "embedding_dim", 128),
                data_dim=args.split_base_num * m, period="train") for m in (1, 2, 4)]


def _split(dataset, seed):
    """The reference's reproducible 0.9 / 0.1 split."""
    return random_split(dataset, [0.9, 0.1], generator=torch.Generator().manual_seed(int(seed)))


def loader_provider(cls, args, period="train"):
    """(train_loader, test_loader) over the 0.9 / 0.1 split under args.general_seed.  'train': the three aligned length
    groups, batches grouped by custom_collate_fn; 'test': clips at their own lengths (batch_size 1 unless they agree)."""
    if period == "train":
        dataset = AlternatingDataset(*_group_datasets(cls, args))
        common = dict(batch_size=args.batch_size, collate_fn=custom_collate_fn)
    elif period == "test":
        json_path, caption_root = _paths(args)
        dataset = cls(json_path=json_path, caption_root=caption_root, emb_dim=getattr(args, "embedding_dim", 128),
                      data_dim=0, period="test")
        common = dict(batch_size=args.batch_size)
    else:
        raise ValueError("Not expected period")
    train_ds, test_ds = _split(dataset, args.general_seed)
    return (DataLoader(train_ds, shuffle=True, drop_last=True, **common),
            DataLoader(test_ds, shuffle=False, drop_last=False, **common))


def group_arrays(cls, args, split="train"):
    """The three (N, C, L) float32 training arrays, L = split_base_num x 1, 2, 4: the aligned clips of each length group, in
    dataset order.  split 'train' (default) keeps the 0.9 part of the split -- what the reference trains on, and what leaves
    the held-out clips unseen --, 'test' the 0.1 part, None every clip."""
    datasets = _group_datasets(cls, args)
    joined = AlternatingDataset(*datasets)
    if split is None:
        keep = range(len(joined))
    else:
        keep = sorted(_split(joined, args.general_seed)[0 if split == "train" else 1].indices)
    rows = [[], [], []]
    for i in keep:
        g, j = joined.index_map[i]
        rows[g].append(datasets[g][j][1])
    C = next((d[0][1].shape[0] for d in datasets if len(d)), 0)
    return [torch.stack(r) if r else torch.empty(0, C, args.split_base_num * m) for r, m in zip(rows, (1, 2, 4))]


def dataset_module(name):
    """The loader package of a dataset name."""
    if name == "benchpress":
        from .benchpress import dataloader
    elif name == "deadlift":
        from .deadlift import dataloader
    else:
        raise ValueError(f"motion dataset {name!r}: expected 'benchpress' or 'deadlift'")
    return dataloader


def with_defaults(args):
    """Fill what config.yaml would have set for args.dataset_name (caption, split_base_num, general_seed) where args lacks it."""
    d = DEFAULTS[args.dataset_name]
    for k in ("caption", "split_base_num"):
        if getattr(args, k, None) in (None, "", 0):
            setattr(args, k, d[k])
    if getattr(args, "general_seed", None) is None:
        args.general_seed = 2025
    return args


def motion_groups(args, split="train"):
    """group_arrays for args.dataset_name ('benchpress' / 'deadlift')."""
    return dataset_module(args.dataset_name).motion_groups(args, split)
