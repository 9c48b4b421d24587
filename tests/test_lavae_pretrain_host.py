"""LA-VAE pre-training, the parts that need no GPU: the C ABI declaration and its ctypes mirror, the driver's arguments and
paths, and the loud failure on CPU tensors."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from t2ms_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_backward_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "t2s.h")).read()
    assert re.search(r"\bint\s+t2s_vae_decode_backward\s*\(", header)
    assert re.search(r"\}\s*t2s_vae_dec_grads\s*;", header)
    res, argtypes = L.SYMBOLS["t2s_vae_decode_backward"]
    assert res is C.c_int and len(argtypes) == 10
    assert argtypes[4] is C.POINTER(L.VaeDecGrads)


def test_dec_grads_layout():
    assert C.sizeof(L.VaeDecGrads) == 14 * 8
    assert [f[0] for f in L.VaeDecGrads._fields_] == ["conv1_w", "conv1_b", "stack_conv3_w", "stack_conv1_w", "ct1_w", "ct1_b",
                                                      "ct2_w", "ct2_b"]
    assert L.VaeDecGrads.stack_conv3_w.offset == 16 and L.VaeDecGrads.ct1_w.offset == 16 + 64


def test_driver_defaults_are_the_reference_ones():
    import pretrain_lavae as drv
    a = drv.get_args([])
    assert (a.batch_size, a.num_training_updates, a.save_path, a.general_seed) == (8, 2000, "results/saved_pretrained_models/", 42)
    assert a.learning_rate == 1e-3
    assert (a.block_hidden_size, a.num_residual_layers, a.res_hidden_size, a.embedding_dim) == (128, 2, 256, 64)
    assert (a.num_embeddings, a.compression_factor, a.commitment_cost) == (128, 4, 0.25)
    assert a.mix_train is False and a.synthetic == 0
    assert drv.get_args(["--mix_train", "True"]).mix_train is True
    assert drv.get_args(["--mix_train", "True", "--split_train"]).mix_train is False


def test_driver_save_directory():
    import pretrain_lavae as drv
    assert drv.save_dir_of(drv.get_args(["--dataset_name", "ETTh1"])) == "results/saved_pretrained_models/datasetETTh1_epoch2000"
    a = drv.get_args(["--dataset_name", "ETTh1_24", "--num_training_updates", "6", "--save_path", "/x/y"])
    assert drv.save_dir_of(a) == "/x/y/datasetETTh1_24_epoch6"
    assert callable(drv.pretrain_step) and callable(drv.pretrain)


def test_cpu_tensors_fail_loudly():
    """No CPU fallback: a training step on a CPU batch is a T2SError that names the GPU, and so is a CPU latent."""
    from model.pretrained.vqvae import vqvae
    from t2ms_amd.model.pretrained.vqvae import _DecodeFn    # noqa: F401  (the HIP pair exists)
    v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    opt = torch.optim.SGD(v.parameters(), lr=0.1)
    with pytest.raises(L.T2SError, match="GPU"):
        v.shared_eval(torch.zeros(2, 24), opt, "train")
    with pytest.raises(L.T2SError, match="GPU"):
        v.decoder(torch.zeros(2, 64, 30, requires_grad=True), length=24)
