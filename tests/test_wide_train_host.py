"""Host side of the wide-latent training path (no GPU): the plain-torch restatement the GPU tests differentiate is the
reference project's network (tests/golden/wide_dit.npz holds the reference's own outputs), fp32 autograd through it is
far inside the GPU tests' gradient bar, mytrain.py resolves its paths as myinfer.py does, and the mirror's switches
default off."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

import _wide_train_ref as R
from t2ms_amd import synth

_spec = importlib.util.spec_from_file_location("gen_golden_wide", os.path.join(os.path.dirname(__file__), "golden", "gen_golden_wide.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GPU_GRAD_BAR = 2e-4          # tests/test_wide_train.py (= tests/test_hip_train.py): per gradient tensor, of its absmax


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = {k: v for k, v in np.load(os.path.join(golden_dir, "wide_dit.npz")).items()}
    g["plan"] = json.loads(str(g["plan"]))
    return g


@pytest.mark.parametrize("case", gen.FORWARD_CASES, ids=gen.case_key)
def test_restatement_reproduces_the_reference_outputs(gold, case):
    """fp32 restatement against the reference's own mytransformer.py outputs: cond (integer t), uncond, cond with float t."""
    key = gen.case_key(case)
    sd = gen.wide_state_dict(synth, case["W"])
    x, text, t_long, t_float = gen.forward_inputs(synth, case)
    with torch.no_grad():
        got = {"cond": R.forward(sd, x, t_long, text), "uncond": R.forward(sd, x, t_long, None),
               "cond_float": R.forward(sd, x, t_float, text)}
    for name, y in got.items():
        err = float(np.abs(y.numpy().astype(np.float64) - gold[f"{name}_{key}"].astype(np.float64)).max())
        print(f"wide_train_errors | restatement fp32 vs reference | {key} {name} | max abs {err:.3e}")
        assert err <= 1e-5, (key, name, err)


@pytest.mark.parametrize("W,B", [(50, 3), (64, 2)])
def test_fp32_autograd_is_a_quarter_of_the_gpu_bar(W, B):
    """The restatement in fp32 against itself in fp64 (same fp32 time embedding): per gradient tensor, max deviation over the
    tensor's absmax.  At most GPU_GRAD_BAR / 4, so 2e-4 of absmax holds the HIP step to 4 x fp32's own error or better."""
    _, _, _, _, pred64, loss64, g64, dx64 = R.batch_case(W, B, True, torch.float64, input_grad=True)
    _, _, _, _, pred32, loss32, g32, dx32 = R.batch_case(W, B, True, torch.float32, input_grad=True)
    assert len(g64) == 48 and set(g64) == set(g32)
    worst = 0.0
    for k in sorted(g64):
        d = float((g32[k] - g64[k]).abs().max() / g64[k].abs().max())
        worst = max(worst, d)
        print(f"wide_train_errors | fp32 vs fp64 autograd | W{W} B{B} | {k} | {d:.3e}")
        assert d <= GPU_GRAD_BAR / 4, (k, d)
    d = float((dx32 - dx64).abs().max() / dx64.abs().max())
    print(f"wide_train_errors | fp32 vs fp64 autograd | W{W} B{B} | dx | {d:.3e} | worst parameter {worst:.3e} | "
          f"pred {float((pred32 - pred64).abs().max()):.3e} | loss rel {abs(float(loss32 - loss64)) / float(loss64):.3e}")
    assert d <= GPU_GRAD_BAR / 4


def test_mytrain_and_myinfer_build_the_same_checkpoint_path(tmp_path):
    import myinfer
    import mytrain
    flags = ["--dataset_name", "benchpress", "--save_path", str(tmp_path / "res"), "--caption", "cap", "--pretrained_epc", "7",
             "--backbone", "ddpm"]
    a = mytrain.get_args(flags)
    b = myinfer.get_args(flags + ["--checkpoint_id", "300"])
    assert mytrain.checkpoint_file(a, 300) == b.checkpoint_path
    assert os.path.basename(os.path.dirname(b.checkpoint_path)) == "ddpm_DiT_benchpress_cap_7"
    assert a.flow_dim == b.flow_dim == 64 and mytrain.get_args(["--dataset_name", "deadlift"]).flow_dim == 50


def test_wide_bf16_training_is_refused():
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd._lib import T2SError
    with pytest.raises(T2SError, match="train in 'f32' only"):
        Transformer(50).set_train_dtype("bf16")
    assert Transformer(50).set_train_dtype("f32") is not None
    Transformer(30).set_train_dtype("bf16")


def test_the_switch_defaults_off():
    """A fresh Transformer(64) refuses a grad-mode forward (the check runs before any device work: a stand-in with the
    attributes forward() looks at is enough), set_trainable(True) returns the model and lifts exactly that refusal, and the
    setting travels with a pickle."""
    import pickle
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd._lib import T2SError
    m = Transformer(64)
    x = types.SimpleNamespace(is_cuda=True, dim=lambda: 3, shape=(2, 64, 64), requires_grad=True)
    with torch.enable_grad(), pytest.raises(T2SError, match="training runs at dim 30"):
        m(input=x, t=None, text_input=None)
    assert m.set_trainable(True) is m
    with torch.enable_grad(), pytest.raises(Exception) as ei:       # past the refusal: fails later, on the stand-in
        m(input=x, t=None, text_input=None)
    assert "training runs at dim 30" not in str(ei.value)
    assert pickle.loads(pickle.dumps(m)).__dict__.get("_t2s_trainable") is True
    assert "_t2s_trainable" not in pickle.loads(pickle.dumps(Transformer(64))).__dict__


def test_extension_header_and_its_symbol_table_agree():
    """include/t2s_wide_train.h declares exactly the entries of _lib.SYMBOLS_WIDE_TRAIN (with these argtypes), none of them
    is also in t2s.h / SYMBOLS, and the built library exports them -- what tests/test_cabi_symbols.py checks for t2s.h."""
    import ctypes as C
    import re
    from t2ms_amd import _lib as L
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo, "include", "t2s_wide_train.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(L.SYMBOLS_WIDE_TRAIN) == {"t2s_dit_set_trainable", "t2s_attn_train_n"}
    assert not declared & set(L.SYMBOLS)
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS_WIDE_TRAIN["t2s_dit_set_trainable"] == (I, [VP, I])
    assert L.SYMBOLS_WIDE_TRAIN["t2s_attn_train_n"] == (I, [VP] * 7 + [I, I, I, VP])
    lib = L.lib()
    for name, (res, args) in L.SYMBOLS_WIDE_TRAIN.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
