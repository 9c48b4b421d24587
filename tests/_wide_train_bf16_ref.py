"""The bf16 training attention (t2s_attn_bf16.hip: attn16_fwd_kernel, attn16_bwd_dq_kernel, attn16_bwd_dkv_kernel) restated in
fp64 with a bf16 rounding exactly where the kernels have one, at ANY token count -- _sticky_forward_bf16 / _restate_bf16 of
tests/test_train_kernels.py without the 480 -- and the cases the wide bf16 attention tests share.  No tests in here.

Roundings: P before P V and before P^T dO; dS before both of its products; O on store (and so inside D_i); dq, dk, dv on
store.  The forward exponentiates against a STICKY reference: the row max of the first key block, moved up (for the 32
queries of a tile at once) only when a lane's sum over its 16 keys of a block reaches 2^40.

Inputs: _sequence(seed, N) of tests/test_wide_attn_train.py (spikes and twins in every head; query 7's first key block is
hugely negative and its maximum sits in the last blocks).  Reference: that file's fp64 autograd on the ROUNDED operands.
Bars: the rule of _bars_bf16 in tests/test_train_kernels.py."""
import torch

import test_wide_attn_train as WA
from test_train_kernels import _rb

NH, DH, SCALE, QS, LN2 = WA.NH, WA.DH, WA.SCALE, WA.QS, WA.LN2
LSE_ABS = 2e-3                                     # the suite's absolute bar for the lse (tests/test_hip_train.py)


def sticky_forward_bf16(s, v):
    """attn16_fwd_kernel on log2-domain scores s (BH, N, N): (o rounded on store, lse, reref) with reref (BH, N / 32, N / 32)
    bool: query tile i re-referenced at key block j."""
    BH, N, _ = s.shape
    nkb = N // 32
    half1 = ((torch.arange(32) >> 2) & 1).bool()       # accumulator layout: key (r & 3) + 8 (r >> 2) + 4 half of a block
    m = s[:, :, 0:32].amax(-1)
    l = torch.zeros_like(m)
    acc = torch.zeros(BH, N, DH, dtype=s.dtype)
    reref = torch.zeros(BH, nkb, nkb, dtype=torch.bool)
    for jb in range(nkb):
        st = s[:, :, jb * 32:jb * 32 + 32] - m.unsqueeze(-1)
        pt = torch.exp2(st)
        lane = torch.stack([pt[..., ~half1].sum(-1), pt[..., half1].sum(-1)], -1)            # (BH, N, 2)
        tile_stale = (~(lane < 2.0 ** 40)).reshape(BH, nkb, 64).any(-1)
        reref[:, :, jb] = tile_stale
        stale = tile_stale.repeat_interleave(32, dim=1)
        up = torch.where(stale, st.amax(-1).clamp(min=0.0), torch.zeros_like(m))
        pt = torch.where(stale.unsqueeze(-1), torch.exp2(st - up.unsqueeze(-1)), pt)
        alpha = torch.exp2(-up)
        m = m + up
        l = l * alpha + pt.sum(-1)
        acc = acc * alpha.unsqueeze(-1) + _rb(pt) @ v[:, jb * 32:jb * 32 + 32]
    return _rb(acc / l.unsqueeze(-1)), m + torch.log2(l), reref


def restate_bf16(qs, k, v, do):
    """qs, k, v, do: the operands as the kernels read them (fp64 values of bf16 numbers, qs = rb(q ATT_QS))."""
    s = qs @ k.transpose(-1, -2)
    o, lse, reref = sticky_forward_bf16(s, v)
    p = torch.exp2(s - lse.unsqueeze(-1))
    d = (do * o).sum(-1, keepdim=True)
    ds = _rb(p * (do @ v.transpose(-1, -2) - d))
    return {"o": o, "lse": lse, "dq": _rb((ds @ k) * SCALE), "dk": _rb((ds.transpose(-1, -2) @ qs) * LN2),
            "dv": _rb(_rb(p).transpose(-1, -2) @ do), "reref": reref}


def restate_lse_f32(qs, k):
    """The lse has no bf16 rounding behind it: fp32 sums of exact products (the fp32 rule of _bars_bf16)."""
    s = qs.float() @ k.float().transpose(-1, -2)
    m = s.amax(-1, keepdim=True)
    return (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))).squeeze(-1).double()


_CASES = {}


def case(n_seq, N):
    """Inputs, fp64 reference of the rounded operands and bf16 restatement of one (n_seq, N): computed once, left unchanged."""
    if (n_seq, N) not in _CASES:
        q, k, v, do = WA._inputs(n_seq, N)
        qs = _rb(q * QS)                           # one fp32 multiplication, then the rounding (the qkv GEMM's epilogue)
        kb, vb, dob = _rb(k), _rb(v), _rb(do)
        ref = WA._reference(qs / QS, kb, vb, dob)  # dq comes out with respect to the UNSCALED q
        WA._check_reference(ref, N)
        _CASES[(n_seq, N)] = {"in": (q, k, v, do), "ref": ref, "res": restate_bf16(qs, kb, vb, dob), "lse32": restate_lse_f32(qs, kb)}
    return _CASES[(n_seq, N)]


def measure(got, ref, N):
    """{(tensor, row or None): relative L2 error}, per tensor and per named row (worst head); a gradient row smaller than
    the tensor's median row is taken relative to the median row (tests/test_train_kernels.py _measure says why).  The lse:
    max abs error over absmax."""
    out = {}
    size = lambda t: t.norm(dim=-1)
    for name in ("o", "dq", "dk", "dv"):
        g, r = got[name], ref[name]
        out[(name, None)] = float((g - r).norm() / r.norm())
        for row in (WA._qrows(N) if name in ("o", "dq") else WA._krows(N)):
            den = size(r[:, row])
            if name != "o":
                den = torch.clamp(den, min=float(size(r).median()))
            out[(name, row)] = float((size(g[:, row] - r[:, row]) / den).max())
    out[("lse", None)] = float((got["lse"] - ref["lse"]).abs().max() / ref["lse"].abs().max())
    return out


def bars(c, N):
    """(restatement's deviation, bar) per key: 2 x the restatement's relative L2 deviation; the lse min(4 x the fp32
    restatement's deviation, 2e-3 absolute)."""
    ref = c["ref"]
    dev_ = measure(c["res"], ref, N)
    dev_[("lse", None)] = float((c["lse32"] - ref["lse"]).abs().max() / ref["lse"].abs().max())
    out = {key: 2.0 * d for key, d in dev_.items()}
    out[("lse", None)] = min(4.0 * dev_[("lse", None)], LSE_ABS / float(ref["lse"].abs().max()))
    return dev_, out
