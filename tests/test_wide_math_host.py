"""Host side of bf16x3 / bf16 inference at the wide latent widths (no GPU): the extension header and its symbol table, the
mirror's opt-in switch, the driver's flag, and the CPU bar the GPU test of the single-pass arithmetic is held to."""
import os
import pickle
import re

import pytest

import _wide_math_ref as WM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_header_and_its_symbol_table_agree():
    """include/t2s_wide_math.h declares exactly the entries of _lib.SYMBOLS_WIDE_MATH (with these argtypes), none of them is
    also in t2s.h / SYMBOLS or t2s_wide_train.h / SYMBOLS_WIDE_TRAIN, and the built library exports them."""
    import ctypes as C
    from t2ms_amd import _lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s_wide_math.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(L.SYMBOLS_WIDE_MATH) == {"t2s_dit_set_wide_math", "t2s_attn_fwd_x3_n", "t2s_attn_fwd_bf16p_n"}
    assert not declared & set(L.SYMBOLS) and not declared & set(L.SYMBOLS_WIDE_TRAIN)
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS_WIDE_MATH["t2s_dit_set_wide_math"] == (I, [VP, I])
    assert L.SYMBOLS_WIDE_MATH["t2s_attn_fwd_x3_n"] == (I, [VP, VP, VP, VP, I, I, VP])
    assert L.SYMBOLS_WIDE_MATH["t2s_attn_fwd_bf16p_n"] == (I, [VP, VP, VP, VP, I, I, VP])
    lib = L.lib()
    for name, (res, args) in L.SYMBOLS_WIDE_MATH.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args


def test_the_switch_defaults_off_and_travels_with_a_pickle():
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd._lib import T2SError
    m = Transformer(64)
    for math in ("bf16x3", "bf16"):
        with pytest.raises(T2SError, match="f32"):
            m.set_math(math)
    assert m.set_wide_math(True) is m
    for math in ("bf16x3", "bf16", "f32", "bf16x3"):
        assert m.set_math(math) is m and m.__dict__["_t2s_math"] == math
    back = pickle.loads(pickle.dumps(m))
    assert back.__dict__.get("_t2s_wide_math") is True and back.__dict__.get("_t2s_math") == "bf16x3"
    assert back.set_math("bf16") is back
    assert "_t2s_wide_math" not in pickle.loads(pickle.dumps(Transformer(64))).__dict__
    # switching off: the refusal is back and the model is on f32 again
    assert m.set_wide_math(False) is m and m.__dict__["_t2s_math"] == "f32"
    with pytest.raises(T2SError, match="f32"):
        m.set_math("bf16x3")
    with pytest.raises(ValueError):
        m.set_wide_math(True).set_math("bf16x2")
    # training stays fp32 at the wide widths, opted in or not
    with pytest.raises(T2SError, match="train in 'f32' only"):
        Transformer(50).set_wide_math(True).set_train_dtype("bf16")


def test_width_30_is_unaffected():
    from model.denoiser.mytransformer import Transformer
    m = Transformer(30)
    assert m.set_math("bf16").__dict__["_t2s_math"] == "bf16"           # always had the three arithmetics
    assert m.set_wide_math(False) is m and m.__dict__["_t2s_math"] == "bf16"
    assert m.set_wide_math(True).set_math("bf16x3") is m


def test_myinfer_parser_takes_math_and_defaults_to_f32():
    import myinfer
    import mytrain
    base = ["--dataset_name", "benchpress"]
    assert myinfer.get_args(base).math == "f32"
    assert myinfer.get_args(base + ["--math", "bf16"]).math == "bf16"
    assert myinfer.get_args(base + ["--math", "bf16x3"]).math == "bf16x3"
    with pytest.raises(SystemExit):
        myinfer.get_args(base + ["--math", "bf16x2"])
    with pytest.raises(SystemExit):                                     # wide training is fp32: mytrain.py has no such flag
        mytrain.get_args(["--dataset_name", "deadlift", "--math", "bf16"])


@pytest.mark.parametrize("W,B,with_text,rms,mx,absmax", [(50, 3, True, 4.1e-3, 2.0e-2, 4.5), (64, 2, True, 4.3e-3, 1.9e-2, 5.3)])
def test_the_bf16_bar_is_computable_on_the_cpu(W, B, with_text, rms, mx, absmax):
    """The bar of tests/test_wide_math.py's bf16 forward: the restatement under torch.autocast(bfloat16) against itself in
    fp64.  It is a property of the reference arithmetic and the case, not of any kernel: here it is only checked to be what
    was recorded when the test was written (to the two digits quoted), so that a change of torch's autocast that moved the
    bar would be seen."""
    c = WM.bf16_case(W, B, with_text)
    print(f"wide_math_errors | autocast bar | W{W} B{B} | rms {c['bar_rms']:.3e} max {c['bar_max']:.3e} | absmax {c['absmax']:.2f}")
    assert abs(c["absmax"] - absmax) < 0.06
    assert 0.8 * rms <= c["bar_rms"] <= 1.25 * rms and 0.8 * mx <= c["bar_max"] <= 1.25 * mx
    # fp32 on the CPU sits three orders of magnitude inside it (for orientation: 2.4e-6 / 3.5e-6 max)
    assert WM.err(WM.forward_fp32(c["sd"], c["x"], c["t"], c["text"]), c["ref"])[1] < 1e-5
