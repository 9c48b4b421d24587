"""Host side of bf16 mixed-precision training at the wide latent widths (no GPU): the extension header and its symbol table,
the mirror's opt-in switch, the driver's flag, and what the GPU test of the bf16 attention rests on -- its inputs, and the
fp64-with-roundings restatement its bars come from (tests/_wide_train_bf16_ref.py)."""
import os
import pickle
import re

import pytest
import torch

import _wide_train_bf16_ref as WB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_header_and_its_symbol_table_agree():
    """include/t2s_wide_train_bf16.h declares exactly the entries of _lib.SYMBOLS_WIDE_TRAIN_BF16 (with these argtypes), none of
    them is in one of the other three tables, and the built library exports them."""
    import ctypes as C
    from t2ms_amd import _lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s_wide_train_bf16.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(L.SYMBOLS_WIDE_TRAIN_BF16) == {"t2s_dit_set_wide_train_bf16", "t2s_attn_train_bf16_n"}
    for other in (L.SYMBOLS, L.SYMBOLS_WIDE_TRAIN, L.SYMBOLS_WIDE_MATH):
        assert not declared & set(other)
    for header in ("t2s.h", "t2s_wide_train.h", "t2s_wide_math.h"):
        body = open(os.path.join(REPO, "include", header)).read()
        assert not any(re.search(r"\b%s\s*\(" % name, body) for name in declared), header
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS_WIDE_TRAIN_BF16["t2s_dit_set_wide_train_bf16"] == (I, [VP, I])
    assert L.SYMBOLS_WIDE_TRAIN_BF16["t2s_attn_train_bf16_n"] == (I, [VP, VP, VP, VP, VP, VP, VP, I, I, VP])
    lib = L.lib()
    for name, (res, args) in L.SYMBOLS_WIDE_TRAIN_BF16.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args


def test_the_switch_defaults_off_and_travels_with_a_pickle():
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd._lib import T2SError
    for W in (50, 64):
        m = Transformer(W).set_trainable(True)
        with pytest.raises(T2SError, match="train in 'f32' only"):
            m.set_train_dtype("bf16")
        assert "_t2s_train_dtype" not in m.__dict__
        assert m.set_wide_train_bf16(True) is m
        assert m.__dict__.get("_t2s_train_dtype", "f32") == "f32"              # opting in moves nothing
        assert m.set_train_dtype("bf16") is m and m.__dict__["_t2s_train_dtype"] == "bf16"
        back = pickle.loads(pickle.dumps(m))
        assert back.__dict__.get("_t2s_wide_train_bf16") is True and back.__dict__.get("_t2s_train_dtype") == "bf16"
        assert back.__dict__.get("_t2s_trainable") is True
        assert back.set_train_dtype("f32").set_train_dtype("bf16") is back
        # switching off: the model is on f32 again and the refusal is back
        assert m.set_wide_train_bf16(False) is m and m.__dict__["_t2s_train_dtype"] == "f32"
        with pytest.raises(T2SError, match="train in 'f32' only"):
            m.set_train_dtype("bf16")
        with pytest.raises(ValueError):
            m.set_wide_train_bf16(True).set_train_dtype("fp16")
    assert "_t2s_wide_train_bf16" not in pickle.loads(pickle.dumps(Transformer(64))).__dict__
    # either order of the two switches
    assert Transformer(50).set_wide_train_bf16(True).set_trainable(True).set_train_dtype("bf16").__dict__["_t2s_train_dtype"] == "bf16"
    # the sampling switch is another one
    with pytest.raises(T2SError, match="set_wide_train_bf16"):
        Transformer(50).set_wide_math(True).set_train_dtype("bf16")


def test_width_30_is_unaffected():
    from model.denoiser.mytransformer import Transformer
    m = Transformer(30)
    assert m.set_train_dtype("bf16").__dict__["_t2s_train_dtype"] == "bf16"     # always had both arithmetics
    assert m.set_wide_train_bf16(False) is m and m.__dict__["_t2s_train_dtype"] == "bf16"
    assert m.set_wide_train_bf16(True).set_train_dtype("f32") is m


def test_mytrain_parser_takes_bf16_and_defaults_to_fp32():
    import mytrain
    base = ["--dataset_name", "deadlift"]
    assert mytrain.get_args(base).bf16 is False
    assert mytrain.get_args(base + ["--bf16"]).bf16 is True
    with pytest.raises(SystemExit):
        mytrain.get_args(base + ["--bf16", "1"])


@pytest.mark.parametrize("N", [800, 1024])
def test_the_attention_inputs_take_the_re_reference_branch_and_the_restatement_rounds(N):
    """_sequence(seed, N) on the bf16-rounded operands: the properties tests/test_wide_attn_train.py builds it for hold
    (case() runs _check_reference); the sticky forward re-references query 7's tile (tile 0) in one of the last two key
    blocks, in every head, and not at block 0; the restatement deviates from the fp64 reference in every tensor."""
    c = WB.case(1, N)
    reref = c["res"]["reref"]                                 # (heads, query tiles, key blocks)
    nkb = N // 32
    assert tuple(reref.shape) == (WB.NH, nkb, nkb)
    assert bool(reref[:, 7 // 32, nkb - 2:].any(-1).all()), "query 7's tile never re-references: the 2^40 branch is dead"
    assert not bool(reref[:, :, 0].any()), "the reference IS the first block's maximum: block 0 cannot be stale"
    assert bool(reref[:, 200 // 32].any(-1).all())            # the twins of query 200, too
    dev_, bars = WB.bars(c, N)
    for name in ("o", "lse", "dq", "dk", "dv"):
        d = dev_[(name, None)]
        print(f"wide_train_bf16_errors | attention restatement N={N} | {name} | deviation {d:.3e} | bar {bars[(name, None)]:.3e}")
        assert torch.isfinite(torch.tensor(d)) and d > 0.0, name
    for key, d in dev_.items():
        assert d == d and 0.0 < d < 1.0, key
