"""The motion dataset loaders (datafactory/benchpress, datafactory/deadlift) against the reference's own classes, and the
host-side halves of the ragged interfaces.  No GPU.

Fixture: tests/golden/motion_ds/ (synthetic datasets in the reference's format) and tests/golden/motion_loader.npz, the records
of the reference's dataset classes and the split indices of its loader_provider on them under seed 2025, both written by
tests/golden/gen_golden_motion_loader.py.  The loaders use the same torch CPU ops on the same floats: every array is compared
bit for bit, every kept / dropped clip by name.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.join(REPO, "tests", "golden", "motion_ds")
DATASETS = {"benchpress": dict(caption="Caption_explain_no_barbell_length", base=36, channels=10, n_emb=2,
                               dropped={"S02_elbows_flaring_tilting_to_the_left/clip_10": "inconsistent"}),
            "deadlift": dict(caption="Caption_explain_no_barbell", base=48, channels=7, n_emb=1,
                             dropped={"D01_correct/clip_10": "shorter than 10", "D02_Lower_back_rounding/clip_10": "inconsistent"})}


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "motion_loader.npz")) as f:
        g = {k: f[k] for k in f.files}
    g["plan"] = json.loads(str(g["plan"]))
    return g


def _args(name, **kw):
    d = DATASETS[name]
    return types.SimpleNamespace(dataset_root=ROOT, dataset_name=name, caption=d["caption"], embedding_dim=64,
                                 split_base_num=d["base"], general_seed=2025, batch_size=kw.pop("batch_size", 1), **kw)


def _cls(name):
    if name == "benchpress":
        from datafactory.benchpress.dataset import BenchpressT2SDataset as cls
    else:
        from datafactory.deadlift.dataset import DeadliftT2SDataset as cls
    return cls


def _dataset(name, period, data_dim):
    d = DATASETS[name]
    return _cls(name)(json_path=os.path.join(ROOT, name, "data.json"), caption_root=os.path.join(ROOT, name, d["caption"]),
                      period=period, emb_dim=64, data_dim=data_dim)


def _clip(record):
    return record[0].split(":")[0]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", list(DATASETS))
def test_train_groups_are_the_references_records(gold, name):
    d = DATASETS[name]
    seen = []
    for g, m in enumerate((1, 2, 4)):
        ds = _dataset(name, "train", d["base"] * m)
        want = gold["plan"][f"{name}_train{g}"]
        assert [_clip(r) for r in ds.records] == want                      # every kept / dropped decision, in order
        assert len(ds) == len(want) and all(len(r) == 3 + d["n_emb"] for r in ds.records)
        assert _same(torch.stack([r[1] for r in ds.records]).numpy(), gold[f"{name}_train{g}_x"])
        for k in range(d["n_emb"]):
            assert _same(torch.stack([r[2 + k] for r in ds.records]).numpy(), gold[f"{name}_train{g}_emb{k}"])
        assert all(r[-1] == _clip(r).split("/")[0] for r in ds.records)     # the subject rides last
        seen += want
    # every clip lands in exactly one group, but for the dropped ones
    assert len(seen) == len(set(seen)) == 20 and not set(seen) & set(d["dropped"])
    with pytest.raises(ValueError, match="Undefined length"):
        _dataset(name, "train", d["base"] * 3)


@pytest.mark.parametrize("name", list(DATASETS))
def test_test_period_keeps_the_clips_own_lengths(gold, name):
    d = DATASETS[name]
    ds = _dataset(name, "test", 0)
    assert [_clip(r) for r in ds.records] == gold["plan"][f"{name}_test"]
    assert [r[1].shape[1] for r in ds.records] == gold[f"{name}_test_len"].tolist()
    assert all(r[1].shape[0] == d["channels"] and r[1].dtype == torch.float32 for r in ds.records)
    assert _same(torch.cat([r[1].reshape(-1) for r in ds.records]).numpy(), gold[f"{name}_test_x"])
    for k in range(d["n_emb"]):
        assert _same(torch.stack([r[2 + k] for r in ds.records]).numpy(), gold[f"{name}_test_emb{k}"])
    # the dropped clips, by name and by reason
    assert {f"{s}/{c}": why for s, c, why in ds.dropped}.keys() == d["dropped"].keys()
    for s, c, why in ds.dropped:
        assert d["dropped"][f"{s}/{c}"] in why
    if name == "benchpress":        # feature_0..2 are not channels: channel 0 is feature_3
        raw = json.load(open(os.path.join(ROOT, name, "data.json")))
        s, c = _clip(ds.records[0]).split("/")
        assert ds.records[0][1][0].tolist() == np.asarray(raw[s][c]["feature_3"], dtype=np.float32).tolist()


@pytest.mark.parametrize("name", list(DATASETS))
def test_loader_provider_splits_as_the_reference(gold, name):
    from datafactory.motion import dataset_module
    mod = dataset_module(name)
    for period in ("train", "test"):
        train_loader, test_loader = mod.loader_provider(_args(name, batch_size=4 if period == "train" else 1), period=period)
        assert train_loader.dataset.indices == gold[f"{name}_split_{period}_train"].tolist()
        assert test_loader.dataset.indices == gold[f"{name}_split_{period}_test"].tolist()
    # a train batch: one entry per length group present, series stacked per group
    batch = next(iter(mod.loader_provider(_args(name, batch_size=4))[0]))
    n_emb = DATASETS[name]["n_emb"]
    for texts, xs, *embs, subjects in batch:
        assert xs.dim() == 3 and xs.shape[1] == DATASETS[name]["channels"] and xs.shape[2] in [DATASETS[name]["base"] * m for m in (1, 2, 4)]
        assert len(texts) == len(subjects) == xs.shape[0] and len(embs) == n_emb and all(e.shape == (xs.shape[0], 128) for e in embs)
    # a test batch is one clip at its own length
    rec = next(iter(mod.loader_provider(_args(name), period="test")[1]))
    assert rec[1].shape[0] == 1 and rec[1].shape[1] == DATASETS[name]["channels"]
    with pytest.raises(ValueError):
        mod.loader_provider(_args(name), period="val")


@pytest.mark.parametrize("name", list(DATASETS))
def test_motion_groups_stacks_the_train_split(gold, name):
    from datafactory.motion import motion_groups
    sizes = [len(gold["plan"][f"{name}_train{g}"]) for g in range(3)]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    everything = motion_groups(_args(name), split=None)
    for g in range(3):
        assert _same(everything[g].numpy(), gold[f"{name}_train{g}_x"])
    for split, key in (("train", "train_train"), ("test", "train_test")):
        idx = np.sort(gold[f"{name}_split_{key}"])
        groups = motion_groups(_args(name), split=split) if split != "train" else motion_groups(_args(name))
        for g in range(3):
            rows = idx[(idx >= starts[g]) & (idx < starts[g + 1])] - starts[g]
            assert tuple(groups[g].shape[1:]) == (DATASETS[name]["channels"], DATASETS[name]["base"] * (1, 2, 4)[g])
            assert _same(groups[g].numpy(), gold[f"{name}_train{g}_x"][rows])


def test_pretrain_drivers_take_dataset_root():
    import pretrain_lavae
    import pretrain_tsae
    d = DATASETS["deadlift"]
    argv = ["--dataset_name", "deadlift", "--dataset_root", ROOT, "--input_dim", "7", "--general_seed", "2025"]
    a = pretrain_lavae.get_args(argv)
    groups = pretrain_lavae.motion_groups(a)
    assert [tuple(g.shape[1:]) for g in groups] == [(7, 48), (7, 96), (7, 192)] and sum(g.shape[0] for g in groups) == 18
    assert a.caption == d["caption"] and a.split_base_num == 48
    b = pretrain_tsae.get_args(argv)
    assert all(torch.equal(x, y) for x, y in zip(pretrain_lavae.motion_groups(b), groups))
    # the other sources and the refusal are as they were
    assert pretrain_lavae.get_args(["--input_dim", "7", "--synthetic", "4"]).dataset_root == ""
    with pytest.raises(SystemExit) as e:
        pretrain_lavae.get_args(["--input_dim", "7"])
    assert e.value.code == pretrain_lavae.NO_MOTION_DATA
    with pytest.raises(SystemExit):
        pretrain_tsae.get_args([])
    with pytest.raises(SystemExit):
        pretrain_lavae.get_args(["--input_dim", "7", "--dataset_root", ROOT])         # --dataset_name ETTh1 is no motion dataset


# ------------------------------------------------------------------------------------------------ ragged interfaces, host side
def test_ragged_layout_validates_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "lib", no_library)
    lens, off, off4 = L.ragged_layout([36, 0, 41, 140], 140, "t")
    assert lens.dtype == np.int32 and off.dtype == np.uint64 and off4.dtype == np.uint64
    assert lens.tolist() == [36, 0, 41, 140] and off.tolist() == [0, 36, 36, 77, 217] and off4.tolist() == [0, 9, 9, 19, 54]
    for bad, word in (([36, 141], r"lengths\[1\] = 141"), ([5], r"lengths\[0\] = 5"), ([-8, 36], r"lengths\[0\] = -8"), ([], "empty"),
                      ([36.5], "integers"), ([True, 36], "integers"), (None, "integers"), (["36"], "integers")):
        with pytest.raises(L.T2SError, match=word):
            L.ragged_layout(bad, 140, "t")
    with pytest.raises(L.T2SError, match="2 lengths for 3 rows"):
        L.ragged_layout([36, 41], 140, "t", batch=3)
    assert L.ragged_layout(np.asarray([8, 1 << 20]), None, "t")[1].tolist() == [0, 8, 8 + (1 << 20)]
    with pytest.raises(L.T2SError, match="1048577"):
        L.ragged_layout([(1 << 20) + 1], None, "t")

    # the Sampler's check (no C sampler is built: the check reads three attributes)
    from t2ms_amd.sampler import Sampler
    s = Sampler.__new__(Sampler)
    s.channels, s.length, s.batch = 3, 140, 3
    assert s.check_lengths([36, 41, 140])[1].tolist() == [0, 36, 77, 217]
    for bad, word in (([36, 41], "2 lengths for 3 rows"), ([36, 41, 141], r"lengths\[2\] = 141"), ([36, 5, 140], r"lengths\[1\] = 5")):
        with pytest.raises(L.T2SError, match=word):
            s.check_lengths(bad)
        with pytest.raises(L.T2SError, match=word):
            s.run(torch.zeros(3, 128), lengths=bad)
    s.channels = None
    with pytest.raises(L.T2SError, match="multichannel decoder"):
        s.run(torch.zeros(3, 128), lengths=[36, 41, 140])

    # the codec mirrors: bad arguments raise before the handle is asked for, CPU tensors are refused, not computed
    from model.pretrained.myvqvae import vqvae
    from model.pretrained.vqvae import vqvae as vqvae1
    m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64,
                                    flow_dim=64, input_dim=3))
    z = torch.zeros(2, 64, 64)
    for bad, word in (([36], "1 lengths for 2 rows"), ([36, 5], r"lengths\[1\] = 5"), ([36, 40.0], "integers")):
        with pytest.raises(L.T2SError, match=word):
            m.decoder.decode_ragged(z, bad)
    with pytest.raises(L.T2SError, match=r"latent must be \(B,64,W\)"):
        m.decoder.decode_ragged(torch.zeros(2, 32, 64), [36, 40])
    with pytest.raises(L.T2SError, match="GPU"):
        m.decoder.decode_ragged(z, [36, 40])
    for bad, word in (([torch.zeros(3, 36), torch.zeros(4, 36)], r"series\[1\] must be a \(3,L\)"), ([torch.zeros(3, 5)], r"lengths\[0\] = 5"),
                      ([torch.zeros(1, 3, 36)], r"series\[0\] must be"), ([], "empty")):
        with pytest.raises(L.T2SError, match=word):
            m.encoder.encode_ragged(bad)
    with pytest.raises(L.T2SError, match="GPU"):
        m.encoder.encode_ragged([torch.zeros(3, 36)])
    m1 = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    with pytest.raises(L.T2SError, match="single-channel"):
        m1.decoder.decode_ragged(torch.zeros(2, 64, 30), [36, 40])
    with pytest.raises(L.T2SError, match="single-channel"):
        m1.encoder.encode_ragged([torch.zeros(1, 36)])


N_SYMBOLS_BEFORE = 107      # the entries of include/t2s.h before the ragged ones


def test_symbols_gain_exactly_the_three_names():
    """The table holds what it held (by count, and test_cabi_symbols.py ties it to the header and the library by name) plus
    the ragged codec entries and the sampler's lengths; version string and config size are 0.7's."""
    import ctypes as C
    new = {"t2s_vae_decode_mc_ragged", "t2s_vae_encode_mc_ragged", "t2s_sampler_set_lengths"}
    assert new <= set(L.SYMBOLS)
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS["t2s_vae_decode_mc_ragged"] == (I, [VP] * 5 + [I, I, I, VP])
    assert L.SYMBOLS["t2s_vae_encode_mc_ragged"] == (I, [VP] * 7 + [I, I, I, VP])
    assert L.SYMBOLS["t2s_sampler_set_lengths"] == (I, [VP, VP, I])
    assert len(L.SYMBOLS) == N_SYMBOLS_BEFORE + 3
    lib = L.lib()
    assert lib.t2s_version() == b"t2s 0.7 gfx950 fp32-mfma" and C.sizeof(L.SampleConfig) == 56
    header = open(os.path.join(REPO, "include", "t2s.h")).read()
    assert all(f"int {n}(" in header for n in new)


def test_myinfer_parser_accepts_the_references_command_line():
    import myinfer
    a = myinfer.get_args(["--dataset_name", "benchpress", "--cfg_scale", "3", "--total_step", "100", "--checkpoint_id", "2500",
                          "--run_time", "1", "--save_path", "./results/denoiser_results", "--batch_size", "1"])
    assert (a.dataset_name, a.cfg_scale, a.total_step, a.checkpoint_id, a.run_time, a.batch_size) == ("benchpress", 3, 100, 2500, 1, 1)
    assert (a.input_dim, a.flow_dim, a.split_base_num, a.caption) == (10, 64, 36, "Caption_explain_no_barbell_length")
    assert a.backbone == "flowmatching" and a.denoiser == "DiT" and a.general_seed == 2025 and a.dataset_root == "./Data"
    assert len(a.features) == 13 and a.features[-10:][0] == "left_shoulder_y"
    assert a.checkpoint_path.endswith(os.path.join("checkpoints", "flowmatching_DiT_benchpress_Caption_explain_no_barbell_length_16000",
                                                   "model_2500.pth"))
    assert a.pretrainedvae_path.endswith(os.path.join("36_benchpress_epoch16000", "final_model.pth"))
    assert a.generation_save_path.endswith(os.path.join("generation", "flowmatching_DiT_benchpress_3_100"))
    d = myinfer.get_args(["--dataset_name", "deadlift"])
    assert (d.input_dim, d.flow_dim, d.split_base_num, d.caption, d.pretrained_epc) == (7, 50, 48, "Caption_explain_no_barbell", 20000)
    assert len(d.features) == 9 and d.cfg_scale == 3 and d.total_step == 100 and d.launch_batch >= 1 and d.embedding == "summary"
    with pytest.raises(SystemExit):
        myinfer.get_args(["--dataset_name", "squat"])
