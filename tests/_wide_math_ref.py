"""References shared by tests/test_wide_math_host.py and tests/test_wide_math.py: the fp64 restatement of the wide forward
(tests/_wide_train_ref.forward on the fp32 values, fp32 time embedding) and the bar of the single-pass bf16 arithmetic -- the
same restatement under torch.autocast("cpu", dtype=torch.bfloat16), the project's bar for `--math bf16` (tests/test_math_bf16.py).
Each is computed once per case and left unchanged."""
import numpy as np
import torch

import _wide_train_ref as R

BF16_CASES = [(50, 3, True), (64, 2, True), (64, 2, False)]     # (W, B, with_text) of _wide_train_ref.batch_inputs
RMS_BAR, MAX_BAR = 1.05, 1.25                                   # tests/test_math_bf16.py: per case / pooled
_CACHE = {}


def forward_fp64(sd, x, t, text):
    """(B,64,W) float64 numpy: the restatement in fp64 on the fp32 data, with the fp32 time embedding upcast (as the wide
    fixture's generator and _wide_train_ref.grads do)."""
    with torch.no_grad():
        temb = R.time_embedding(t, torch.float32).double()
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        return R.forward(sd64, x.double(), t, None if text is None else text.double(), temb=temb).numpy()


def forward_fp32(sd, x, t, text):
    with torch.no_grad():
        return R.forward(sd, x, t, text).numpy()


def forward_autocast(sd, x, t, text):
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        y = R.forward(sd, x, t, text)
    return y.float().numpy()


def err(x, ref):
    """(rms, max) of x - ref in float64"""
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(np.sqrt((d ** 2).mean())), float(d.max())


def bf16_case(W, B, with_text):
    """dict(sd, x, t, text, ref (fp64), bar_rms, bar_max, absmax) of one case of BF16_CASES"""
    key = (W, B, with_text)
    if key not in _CACHE:
        sd = R.state_dict(W)
        x, t, text, _ = R.batch_inputs(W, B, with_text)
        ref = forward_fp64(sd, x, t, text)
        bar_rms, bar_max = err(forward_autocast(sd, x, t, text), ref)
        _CACHE[key] = dict(sd=sd, x=x, t=t, text=text, ref=ref, bar_rms=bar_rms, bar_max=bar_max, absmax=float(np.abs(ref).max()))
    return _CACHE[key]
