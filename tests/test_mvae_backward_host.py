"""Host-side logic of the multichannel LA-VAE backward (no GPU): the mirror's coverage predicate and switch, the new symbols, and
the motion path of pretrain_lavae.py -- flags, the refusal without a data source, `--series_npy` grouping and the epoch count."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L


def test_coverage_predicate():
    from t2ms_amd.model.pretrained.myvqvae import _mc_backward_covers as covers
    ok = dict(hidden=128, emb=64, res_hidden=256, n_res=3, Ln=144, W=64, channels=10)
    assert covers(**ok)
    for change, want in (({"res_hidden": 128}, True), ({"n_res": 1}, True), ({"n_res": 4}, True), ({"Ln": 8}, True), ({"Ln": 192}, True),
                         ({"Ln": 37}, True), ({"W": 1}, True), ({"channels": 1}, True), ({"channels": 16}, True),
                         ({"hidden": 64}, False), ({"emb": 32}, False), ({"res_hidden": 64}, False), ({"res_hidden": 192}, False),
                         ({"res_hidden": None}, False), ({"n_res": 0}, False), ({"n_res": 5}, False), ({"Ln": 7}, False),
                         ({"Ln": 193}, False), ({"Ln": 196}, False), ({"W": 65}, False), ({"W": 0}, False), ({"channels": 17}, False)):
        assert covers(**{**ok, **change}) is want, change


def test_mirror_reads_its_shape_into_the_predicate():
    import types
    from model.pretrained.myvqvae import vqvae
    mk = lambda **kw: vqvae(types.SimpleNamespace(**{**dict(block_hidden_size=128, num_residual_layers=3, res_hidden_size=256,  # noqa: E731
                                                            embedding_dim=64, flow_dim=50, input_dim=7), **kw}))
    m = mk()
    assert m.encoder._hip_backward_ok(36) and m.encoder._hip_backward_ok(192) and not m.encoder._hip_backward_ok(196)
    assert m.decoder._hip_backward_ok(36, 50) and m.decoder._hip_backward_ok(39, 64) and not m.decoder._hip_backward_ok(36, 65)
    assert len(m.encoder._grad_params()) == 14 and len(m.decoder._grad_params()) == 12
    assert tuple(m.encoder._grad_params()[0].shape) == (64, 7, 4) and tuple(m.decoder._grad_params()[-2].shape) == (64, 7, 4)
    r0 = mk(num_residual_layers=0)
    assert not r0.encoder._hip_backward_ok(36) and not r0.decoder._hip_backward_ok(36, 50)
    assert not mk(block_hidden_size=64).encoder._hip_backward_ok(36)
    assert not mk(flow_dim=65).encoder._hip_backward_ok(36)
    assert not mk(input_dim=17).decoder._hip_backward_ok(36, 50)


def test_switch_is_read_at_call_time(monkeypatch):
    from t2ms_amd.model.pretrained.myvqvae import _backward_mode
    monkeypatch.delenv("T2S_MVAE_BACKWARD", raising=False)
    default = _backward_mode()
    assert default in ("hip", "torch")
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "torch")
    assert _backward_mode() == "torch"
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "hip")
    assert _backward_mode() == "hip"
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "")
    assert _backward_mode() == default
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "fast")
    with pytest.raises(L.T2SError, match="T2S_MVAE_BACKWARD"):
        _backward_mode()


def test_lib_declares_the_new_symbols():
    I, VP = C.c_int, C.c_void_p
    assert L.SYMBOLS["t2s_vae_encode_backward_mc"] == (I, [VP, VP, VP, VP, C.POINTER(L.VaeEncGrads), I, I, I, VP])
    assert L.SYMBOLS["t2s_vae_decode_backward_mc"] == (I, [VP, VP, VP, VP, C.POINTER(L.VaeDecGrads), VP, I, I, I, VP])
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2s.h")).read()
    for n in ("t2s_vae_encode_backward_mc", "t2s_vae_decode_backward_mc"):
        assert f"int {n}(" in header
        assert hasattr(L.lib(), n)


def test_driver_flags_and_the_refusal_without_data(capsys):
    import pretrain_lavae as drv
    a = drv.get_args([])
    assert (a.input_dim, a.flow_dim, a.series_npy, a.split_base_num) == (1, 30, "", 36)      # today's path
    a = drv.get_args(["--input_dim", "10", "--flow_dim", "64", "--synthetic", "5"])
    assert (a.input_dim, a.flow_dim, a.synthetic, a.split_base_num) == (10, 64, 5, 36)
    a = drv.get_args(["--input_dim", "7", "--flow_dim", "50", "--series_npy", "a.npy,b.npy", "--split_base_num", "48"])
    assert (a.series_npy, a.split_base_num) == ("a.npy,b.npy", 48)
    with pytest.raises(SystemExit) as e:
        drv.get_args(["--input_dim", "7", "--flow_dim", "50"])
    assert "--series_npy" in str(e.value) and "--synthetic" in str(e.value)
    with pytest.raises(SystemExit):
        drv.get_args(["--input_dim", "0"])


def test_series_npy_grouping_and_epoch_count(tmp_path):
    import pretrain_lavae as drv
    rs = np.random.RandomState(0)
    shapes = [(5, 3, 8), (2, 3, 16), (7, 3, 12)]
    paths = []
    for i, sh in enumerate(shapes):
        paths.append(str(tmp_path / f"g{i}.npy"))
        np.save(paths[-1], rs.rand(*sh))                      # float64 on disk: the loader casts
    a = drv.get_args(["--input_dim", "3", "--series_npy", ",".join(paths), "--batch_size", "3", "--num_training_updates", "8"])
    groups = drv.motion_groups(a)
    assert [tuple(g.shape) for g in groups] == shapes and all(g.dtype == torch.float32 for g in groups)
    loader = drv.MotionLoader(groups, a.batch_size)
    assert len(loader) == 3                                   # ceil(7 / 3): the longest group sets the batch count
    batches = list(loader)
    got = [[None if g is None else tuple(g[1].shape) for g in b] for b in batches]
    assert got == [[(3, 3, 8), (2, 3, 16), (3, 3, 12)], [(2, 3, 8), None, (3, 3, 12)], [None, None, (1, 3, 12)]]
    assert [tuple(t.shape) for t in drv._series_batches(batches[1], True)] == [(2, 3, 8), (3, 3, 12)]
    for k, g in enumerate(groups):                            # stored order without a seed: every row once
        assert torch.equal(torch.cat([b[k][1] for b in batches if b[k] is not None]), g)
    assert drv.epochs_of(a.num_training_updates, len(loader)) == 3          # int(8 / 3 + 0.5)
    assert drv.epochs_of(4, 2) == 2 and drv.epochs_of(2000, 7) == 286 and drv.epochs_of(1, 4) == 0
    # a seeded loader draws a new order per epoch, the same for the same seed, and still serves every row once
    s1, s2 = drv.MotionLoader(groups, 3, seed=42), drv.MotionLoader(groups, 3, seed=42)
    e1, e2, f1 = list(s1), list(s1), list(s2)
    rows = lambda ep: torch.cat([b[2][1] for b in ep if b[2] is not None])  # noqa: E731
    assert torch.equal(rows(e1), rows(f1)) and not torch.equal(rows(e1), rows(e2))
    assert torch.equal(rows(e1).sum(0), groups[2].sum(0)) or torch.allclose(rows(e1).sum(0), groups[2].sum(0))
    # a wrong channel count is refused
    a.input_dim = 4
    with pytest.raises(SystemExit) as e:
        drv.motion_groups(a)
    assert "(N, 4, L)" in str(e.value)
