"""The training path's attention and weight-gradient kernels, each called ALONE (t2s_attn_train, t2s_wgrad: the launchers
of t2s_dit_train_forward / _backward on plain buffers) and compared with a plain high-precision reference.  Needs an MI355X.

Attention (attn_train_fwd_kernel, attn_dsum_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel; attn16_fwd_kernel,
attn16_bwd_dq_kernel, attn16_bwd_dkv_kernel).  The whole-model gradient tests run near-uniform attention; here the softmax
is PEAKED: N(0,1) q, k, v, dO plus the spikes of tests/test_attn_quad.py in every head, two of them turned into TWINS -- a
second key with the same score for that query but another direction -- so that P = 0.5 / 0.5 at a log-sum-exp near 90 in the
log2 domain and the spiked rows carry gradients well above zero (with one spike, or two identical keys, dq of that row is 0
and the row tests nothing).  Reference: fp64 torch autograd of softmax(q k^T / sqrt(32)) v.  The bars are MEASURED, never
against the kernel: a CPU restatement of the kernel's algorithm in the kernel's precision is compared with the same fp64
reference and the kernel may deviate by a fixed multiple of what the restatement does (see _bars_f32 / _bars_bf16).

Weight gradients (wgrad_kernel, wgrad16_kernel<XGELU>, wgrad16_reduce_kernel): integer operands, so every partial sum is
exact in any order and dW, db must equal the reference BIT FOR BIT, at row counts chosen from a restatement of wgrad16_plan
so that every path of the kernels is taken (multi-pass slabs, a ragged last slab, slab counts that are no multiple of 4 / 8,
both walk directions, one real row and 63 masked ones, db == NULL).

profiles/train_kernel_errors.md holds the figures these tests print (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1                                   # T2S_TRAIN_F32 / T2S_TRAIN_BF16
NTOK, NH, DH = 480, 4, 32
SCALE = 32 ** -0.5
QS = float(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))   # t2s_bf16.h ATT_QS, t2s_attn_bwd.hip QS
LN2 = float(np.log(2.0))
QROWS = (200, 7, 100, 0, 479)                      # named query rows of o / dq
KROWS = (410, 37, 448, 447, 333, 5)                # named key rows of dk / dv
TINY_DQ_ROWS = (100, 0)                            # one spike and no twin: P ~ 1 and dq ~ 0 in some heads (1e-8 .. 1e-6)
SEED = 2102


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ attention: inputs
def _sequence(seed):
    """One sequence: q, k, v (4, 480, 32) and dO (4, 480, 32), fp32, spikes and twins in every head."""
    rs = np.random.RandomState(seed)
    q, k, v, do = (torch.from_numpy(rs.randn(NH, NTOK, DH).astype(np.float32)) for _ in range(4))
    k[:, 333] = q[:, 100] * 5.0
    k[:, 5] = q[:, 479] * 4.0
    k[:, 479] = q[:, 0] * 4.0
    k[:, 410] = q[:, 200] * 12.0                       # block 12
    k[:, 0:32] = -q[:, 7:8] * 3.0 + 0.01 * k[:, 0:32]  # first block hugely negative for query 7 ...
    k[:, 448] = q[:, 7] * 10.0                         # ... and its real maximum in block 14
    k[:, 440] = q[:, 390] * 12.0
    k[:, 400] = q[:, 470] * 12.0
    k[:, 425] = q[:, 270] * 12.0
    k[:, 300] = q[:, 345] * 12.0
    for key, qrow, gain in ((37, 200, 12.0), (447, 7, 10.0)):       # twins of keys 410 (block 1 vs 12) and 448 (13 vs 14)
        qq = q[:, qrow].double()
        r = torch.from_numpy(rs.randn(NH, DH))
        r = r - (r * qq).sum(-1, keepdim=True) / (qq * qq).sum(-1, keepdim=True) * qq
        k[:, key] = (gain * qq + 2.0 * r).float()
    return q, k, v, do


def _inputs(n_seq):
    """n_seq = 1 is the sequence of seed SEED; n_seq = 3 carries that same sequence in the middle."""
    seeds = [SEED] if n_seq == 1 else [SEED + 1, SEED, SEED + 2]
    assert len(seeds) == n_seq
    parts = [_sequence(s) for s in seeds]
    return tuple(torch.cat([p[i] for p in parts]).contiguous() for i in range(4))       # (BH, 480, 32) each


def _rows(t):      # heads (BH, 480, 32) -> token rows (n_seq * 480, 128)
    n_seq = t.shape[0] // NH
    return t.reshape(n_seq, NH, NTOK, DH).permute(0, 2, 1, 3).reshape(n_seq * NTOK, NH * DH).contiguous()


def _heads(t):     # token rows (n_seq * 480, 128) -> heads (BH, 480, 32)
    n_seq = t.shape[0] // NTOK
    return t.reshape(n_seq, NTOK, NH, DH).permute(0, 2, 1, 3).reshape(n_seq * NH, NTOK, DH).contiguous()


def _rb(t):        # round to nearest even bf16, back in fp64
    return t.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ attention: references
def _reference(q, k, v, do):
    """fp64 autograd of softmax(q k^T / sqrt(32)) v; q, k, v, do fp64 heads (BH, 480, 32)."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = torch.softmax(s, dim=-1) @ v
    o.backward(do)
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), dim=-1) / LN2, "dq": q.grad, "dk": k.grad, "dv": v.grad,
            "s2": s.detach() / LN2}


def _restate_f32(q, k, v, do, qs=None):
    """The fp32 kernels' algorithm in fp32 torch (t2s_attn_bwd.hip): scores in the log2 domain, lse = m + log2(l),
    P = exp2(S - lse), D = sum(dO * O), dS = P * (dP - D).  `qs`: the already scaled q (bf16 arm: its rounded one)."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    qs = q * QS if qs is None else qs.float()
    s = qs @ k.transpose(-1, -2)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    lse = m + torch.log2(l)
    o = (e @ v) / l
    p = torch.exp2(s - lse)
    d = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - d)
    return {"o": o.double(), "lse": lse.squeeze(-1).double(), "dq": ((ds @ k) * SCALE).double(),
            "dk": ((ds.transpose(-1, -2) @ q) * SCALE).double(), "dv": (p.transpose(-1, -2) @ do).double()}


def _sticky_forward_bf16(s, v):
    """attn16_fwd_kernel's forward on log2-domain scores s (BH, 480, 480), in fp64 with its bf16 roundings.  The kernel
    exponentiates against a STICKY reference -- the row max of the first key block, moved up (classic online-softmax step,
    for all 32 queries of a tile at once) only when a lane's sum over its 16 keys of a block reaches 2^40 -- and rounds
    THAT P to bf16 for P V while the row sum l takes the unrounded one.  Against the row max a lone spike would be P = 1
    exactly; against the sticky reference it is some 2^30.4, whose rounding (up to 2^-9) is common to the whole row of O
    and comes back through D_i = dO . O in dq and dk of the peaked rows: the term that makes them bf16-hard."""
    BH = s.shape[0]
    half1 = ((torch.arange(32) >> 2) & 1).bool()       # accumulator layout: key (r & 3) + 8 (r >> 2) + 4 half of a block
    m = s[:, :, 0:32].amax(-1)
    l = torch.zeros_like(m)
    acc = torch.zeros(BH, NTOK, DH, dtype=s.dtype)
    for jb in range(NTOK // 32):
        st = s[:, :, jb * 32:jb * 32 + 32] - m.unsqueeze(-1)
        pt = torch.exp2(st)
        lane = torch.stack([pt[..., ~half1].sum(-1), pt[..., half1].sum(-1)], -1)            # (BH, 480, 2)
        stale = (~(lane < 2.0 ** 40)).reshape(BH, NTOK // 32, 64).any(-1).repeat_interleave(32, dim=1)
        up = torch.where(stale, st.amax(-1).clamp(min=0.0), torch.zeros_like(m))
        pt = torch.where(stale.unsqueeze(-1), torch.exp2(st - up.unsqueeze(-1)), pt)
        alpha = torch.exp2(-up)
        m = m + up
        l = l * alpha + pt.sum(-1)
        acc = acc * alpha.unsqueeze(-1) + _rb(pt) @ v[:, jb * 32:jb * 32 + 32]
    return _rb(acc / l.unsqueeze(-1)), m + torch.log2(l)       # normalised after the sum, rounded on store


def _restate_bf16(qs, k, v, do):
    """The bf16 kernels' arithmetic in fp64 with a bf16 rounding exactly where t2s_attn_bf16.hip has one: P before P V
    (_sticky_forward_bf16) and before P^T dO; dS before both of its products; O on store (and so inside D_i); dq, dk, dv
    on store.  qs, k, v, do: the operands as the kernels read them (fp64 values of bf16 numbers, qs = rb(q ATT_QS))."""
    s = qs @ k.transpose(-1, -2)
    o, lse = _sticky_forward_bf16(s, v)
    p = torch.exp2(s - lse.unsqueeze(-1))
    d = (do * o).sum(-1, keepdim=True)
    ds = _rb(p * (do @ v.transpose(-1, -2) - d))
    return {"o": o, "lse": lse, "dq": _rb((ds @ k) * SCALE), "dk": _rb((ds.transpose(-1, -2) @ qs) * LN2),
            "dv": _rb(_rb(p).transpose(-1, -2) @ do)}


_CASES = {}


def _case(n_seq, dtype):
    """Inputs, fp64 reference and CPU restatement of one (n_seq, dtype), computed once and left unchanged."""
    key = (n_seq, dtype)
    if key not in _CASES:
        q, k, v, do = _inputs(n_seq)
        if dtype == F32:
            ops = tuple(t.double() for t in (q, k, v, do))
            ref = _reference(*ops)
            res = _restate_f32(q, k, v, do)
            lse32 = res["lse"]
        else:
            qs = _rb(q * QS)                           # one fp32 multiplication, then the rounding (the qkv GEMM's epilogue)
            kb, vb, dob = _rb(k), _rb(v), _rb(do)
            ref = _reference(qs / QS, kb, vb, dob)     # dq comes out with respect to the UNSCALED q
            res = _restate_bf16(qs, kb, vb, dob)
            lse32 = _restate_f32(q, kb, vb, dob, qs=qs)["lse"]   # the lse is fp32 arithmetic on exact products in both arms
        _check_reference(ref)
        _CASES[key] = {"in": (q, k, v, do), "ref": ref, "res": res, "lse32": lse32}
    return _CASES[key]


def _check_reference(ref):
    """What the inputs are built for, asserted on the fp64 reference before any kernel is looked at."""
    s2, lse, dq, dk = ref["s2"], ref["lse"], ref["dq"], ref["dk"]
    p = torch.exp2(s2 - lse.unsqueeze(-1))
    for qrow, a, b in ((200, 410, 37), (7, 448, 447)):
        assert float(p[:, qrow, a].min()) > 0.25 and float(p[:, qrow, b].min()) > 0.25, "twins do not share the row"
        assert float(lse[:, qrow].min()) > 50.0
        # a reference taken in the first key block is stale by far more than 2^40 when the twins arrive
        assert float((lse[:, qrow] - s2[:, qrow, 0:32].amax(-1)).min()) > 45.0
    assert float(s2[:, 7, 0:32].amax(-1).max()) < -10.0          # query 7: even the first block's maximum is far below 0
    med = float(dq.abs().amax(-1).median())
    for qrow in (200, 7):                                        # with one spike, or identical twins, these rows would be 0
        top = dq[:, qrow].abs().amax(-1)
        assert float(top.median()) > 0.5 * med and float(top.max()) > 2.0 * med, "a twin row carries no gradient"
    for krow in (410, 37, 448, 447):
        assert float(dk[:, krow].abs().amax(-1).min()) > 2.0
    for qrow in TINY_DQ_ROWS:                                    # why these rows are not normalised by themselves
        assert float(dq[:, qrow].abs().amax(-1).min()) < 1e-3 * med


# ------------------------------------------------------------------------------------------------ attention: the kernel
_RUNS = {}


def _call_attn(dev, q, k, v, do_rows, n_seq, dtype):
    from t2ms_amd import _lib as L
    qd, kd, vd, dod = (t.contiguous().to(dev) for t in (q, k, v, do_rows))
    nan = float("nan")
    od = torch.full((n_seq * NTOK, NH * DH), nan, device=dev)
    lsed = torch.full((n_seq * NH, NTOK), nan, device=dev)
    dd = torch.full((n_seq * NTOK, 3 * NH * DH), nan, device=dev)
    L.check(L.lib().t2s_attn_train(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), dod.data_ptr(), od.data_ptr(), lsed.data_ptr(),
                                   dd.data_ptr(), n_seq, dtype, L.stream_ptr(dev)), "t2s_attn_train")
    return od.cpu(), lsed.cpu(), dd.cpu()


def _run(dev, n_seq, dtype):
    key = (n_seq, dtype)
    if key not in _RUNS:
        q, k, v, do = _case(n_seq, dtype)["in"]
        _RUNS[key] = _call_attn(dev, q, k, v, _rows(do), n_seq, dtype)
    return _RUNS[key]


def _unpack(raw):
    o_rows, lse, dqkv = raw
    for t in raw:
        assert torch.isfinite(t).all(), "an output element was not written, or is not finite"
    n_seq = o_rows.shape[0] // NTOK
    g = dqkv.reshape(n_seq * NTOK, 3, NH * DH)
    return {"o": _heads(o_rows).double(), "lse": lse.double(), "dq": _heads(g[:, 0]).double(), "dk": _heads(g[:, 1]).double(),
            "dv": _heads(g[:, 2]).double()}


# ------------------------------------------------------------------------------------------------ attention: measures
def _named_rows(name):
    return QROWS if name in ("o", "dq") else KROWS if name in ("dk", "dv") else ()


def _measure(got, ref, norm):
    """{(tensor, row or None): error}.  norm "max": max abs error over the tensor / the reference's absmax, and per named
    row (worst head) max abs error / that row's own absmax.  norm "l2": relative L2, per tensor and per named row (worst
    head).  A gradient row that is SMALLER than the tensor's median row is taken relative to the median row instead: dq of
    the single-spike rows 100 and 0 is ~ 0 (1e-10 .. 1e-6: the lone key takes the whole row and dS = 0), and dq of a twin
    row is 0.25 SCALE (dO . (v_a - v_b)) (k_a - k_b), which in one head of twelve is 100 times smaller than in the others
    by the chance of dO . (v_a - v_b).  The rounding error of such a row is that of its CANCELLED terms (the restatement's
    is 9 times the row itself in bf16, 4e-3 in fp32), so against the row itself it says nothing about a kernel.  The
    median row is still 8 to 15 times below the tensor's absmax: a wrong row cannot hide there."""
    out = {}
    for name in ("o", "lse", "dq", "dk", "dv"):
        g, r = got[name], ref[name]
        if norm == "max":
            out[(name, None)] = float((g - r).abs().max() / r.abs().max())
            size = lambda t: t.abs().amax(-1)
        else:
            out[(name, None)] = float((g - r).norm() / r.norm())
            size = lambda t: t.norm(dim=-1)
        for row in _named_rows(name):
            den = size(r[:, row])
            if name != "o":
                den = torch.clamp(den, min=float(size(r).median()))
            out[(name, row)] = float((size(g[:, row] - r[:, row]) / den).max())
    return out


# the bars the suite already holds these tensors to (fp32): 2e-4 * absmax per gradient tensor (tests/test_hip_train.py),
# 3e-5 absolute for o (tests/test_attn_quad.py's kernels), 2e-3 absolute for the lse (tests/test_hip_train.py)
_EXISTING_ABS = {"o": 3e-5, "lse": 2e-3}
_EXISTING_REL = 2e-4


def _bars_f32(case):
    """4 x the deviation of the fp32 restatement from the fp64 reference, per tensor and per named row.  Margin 4: the MFMA
    accumulates in another order than the CPU's matrix product, v_exp_f32 / v_log_f32 are ~1 ulp and not libm, and the
    forward rescales its running sums block by block.  Per tensor never above the bar the suite already has."""
    ref = case["ref"]
    dev_ = _measure(case["res"], ref, "max")
    bars = {}
    for key, d in dev_.items():
        bar = 4.0 * d
        if key[1] is None:
            name = key[0]
            cap = _EXISTING_ABS[name] / float(ref[name].abs().max()) if name in _EXISTING_ABS else _EXISTING_REL
            bar = min(bar, cap)
        bars[key] = bar
    return dev_, bars


def _bars_bf16(case):
    """2 x the relative L2 deviation of the bf16 restatement from the fp64 reference of the ROUNDED operands: the kernel
    rounds where the restatement does and accumulates in fp32 where the restatement is exact.  The lse has no bf16
    rounding behind it (fp32 sums of exact products): it is held to the fp32 rule -- 4 x the fp32 restatement on the
    rounded operands, max abs error over absmax, never above the 2e-3 absolute the suite already has."""
    ref = case["ref"]
    dev_ = _measure(case["res"], ref, "l2")
    bars = {key: 2.0 * d for key, d in dev_.items()}
    d_lse = float((case["lse32"] - ref["lse"]).abs().max() / ref["lse"].abs().max())
    dev_[("lse", None)] = d_lse
    bars[("lse", None)] = min(4.0 * d_lse, _EXISTING_ABS["lse"] / float(ref["lse"].abs().max()))
    return dev_, bars


def _kernel_errors(got, ref, dtype):
    if dtype == F32:
        return _measure(got, ref, "max")
    err = _measure(got, ref, "l2")
    err[("lse", None)] = float((got["lse"] - ref["lse"]).abs().max() / ref["lse"].abs().max())
    return err


def _judge(got, case, dtype, tag):
    """Print every figure, then name every (tensor, row) whose kernel error is above its bar."""
    dev_, bars = _bars_f32(case) if dtype == F32 else _bars_bf16(case)
    err = _kernel_errors(got, case["ref"], dtype)
    bad = []
    for key in sorted(bars, key=lambda kr: (kr[0], -1 if kr[1] is None else kr[1])):
        name, row = key
        print(f"train_kernel_errors | {tag} | {name} | {'tensor' if row is None else 'row %d' % row} | "
              f"kernel {err[key]:.3e} | restatement {dev_[key]:.3e} | bar {bars[key]:.3e}")
        if not err[key] <= bars[key]:
            bad.append((name, row, err[key], bars[key]))
    return bad


@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_attention_forward_and_backward_on_a_peaked_softmax(dev, dtype, n_seq):
    """o, lse, dq, dk, dv of t2s_attn_train against fp64 autograd: per tensor and per named spike row, each row normalised
    by itself (_measure) so that a wrong row cannot hide in the tensor's maximum; outputs pre-filled with NaN must come back finite.
    fp32: max abs error over absmax, bar 4 x the fp32 restatement's (and <= the suite's existing bars).  bf16: relative L2
    against the reference of the rounded operands, bar 2 x the bf16-rounding restatement's.
    Measured on an MI355X (profiles/train_kernel_errors.md): fp32 kernel errors are 0.4 .. 3.0 x the restatement's, at most
    0.74 of a bar; the bf16 kernel's equal the restatement's to three digits, i.e. half a bar."""
    case = _case(n_seq, dtype)
    got = _unpack(_run(dev, n_seq, dtype))
    bad = _judge(got, case, dtype, f"{'f32' if dtype == F32 else 'bf16'} n_seq={n_seq}")
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_attention_zero_upstream_gradient_of_one_head(dev, dtype):
    """dO of head 2 set to zero: that head's dq, dk, dv columns are bitwise 0 (D_i = 0, dP = 0), and every other head's are
    the bits of the run without the zeroing -- a head-column offset in do_rows / dqkv cannot survive both."""
    n_seq, head = 1, 2
    q, k, v, do = _case(n_seq, dtype)["in"]
    base = _run(dev, n_seq, dtype)
    do0 = do.clone()
    do0[head::NH] = 0.0
    o_rows, lse, dqkv = _call_attn(dev, q, k, v, _rows(do0), n_seq, dtype)
    assert torch.equal(o_rows, base[0]) and torch.equal(lse, base[1])
    g, g0 = dqkv.reshape(-1, 3, NH, DH), base[2].reshape(-1, 3, NH, DH)
    assert torch.isfinite(g).all()
    assert torch.equal(g[:, :, head], torch.zeros_like(g[:, :, head])), "the zeroed head's gradient is not exactly 0"
    assert float(g0[:, :, head].abs().max()) > 0
    others = [h for h in range(NH) if h != head]
    assert torch.equal(g[:, :, others], g0[:, :, others]), "another head's gradient depends on the zeroed head's dO"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_attention_rows_do_not_depend_on_the_batch(dev, dtype):
    """n_seq = 3 whose middle sequence is the n_seq = 1 input reproduces that run's rows bit for bit."""
    one, three = _run(dev, 1, dtype), _run(dev, 3, dtype)
    for t in one + three:
        assert torch.isfinite(t).all()
    assert torch.equal(three[0][NTOK:2 * NTOK], one[0]), "o"
    assert torch.equal(three[1][NH:2 * NH], one[1]), "lse"
    assert torch.equal(three[2][NTOK:2 * NTOK], one[2]), "dqkv"


# ------------------------------------------------------------------------------------------------ weight gradients
WGRAD_SHAPES = [(128, 128), (256, 128), (384, 128), (128, 256), (768, 128),       # proj, fc1, qkv, fc2, adaLN
                (128, 384), (256, 384)]                                           # the LA-VAE's conv3 layers


def _plan(M, N, K, n_cu):
    """wgrad16_plan (t2s_bf16.h): rows per workgroup and row slabs."""
    tiles = (N // 128) * (K // 128)
    per = max(1, 3 * n_cu // tiles)
    rows = max(64, ((M + per - 1) // per + 63) // 64 * 64)
    return rows, (M + rows - 1) // rows, per


def _row_counts(N, K, n_cu):
    per = _plan(1, N, K, n_cu)[2]
    Ms = [1, 63, 64, 65, 129, 321, 1440, 64 * per + 1, 64 * per + 64 * 3 + 17]
    plans = [_plan(M, N, K, n_cu) for M in Ms]
    assert per < 6 or [gx for _, gx, _ in plans[:6]] == [1, 1, 1, 2, 3, 6]
    assert any(rows >= 128 for rows, _, _ in plans), "no multi-pass workgroup"
    assert any((M - (gx - 1) * rows) % 64 != 0 for M, (rows, gx, _) in zip(Ms, plans)), "no ragged last slab"
    assert any(rows >= 128 and (M - (gx - 1) * rows) % 64 != 0 and M - (gx - 1) * rows > 64
               for M, (rows, gx, _) in zip(Ms, plans)), "no ragged second pass"
    assert any(gx % 4 != 0 for _, gx, _ in plans) and any(gx % 8 != 0 for _, gx, _ in plans)
    assert any(gx > 8 and gx % 8 != 0 for _, gx, _ in plans) or per <= 8, "the padded grid is never partly filled"
    assert max(Ms) <= 50000
    return Ms


def _call_wgrad(dev, dY, X, M, N, K, dtype, flags, with_db=True):
    from t2ms_amd import _lib as L
    nan = float("nan")
    dW = torch.full((N, K), nan, device=dev)
    db = torch.full((N,), nan, device=dev) if with_db else None
    L.check(L.lib().t2s_wgrad(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), None if db is None else db.data_ptr(), M, N, K,
                              dtype, flags, L.stream_ptr(dev)), "t2s_wgrad")
    return dW, db


def _draw(dev, seed, shape, values):
    g = torch.Generator(device="cpu").manual_seed(seed)
    vals = torch.tensor(values, dtype=torch.float32)
    return vals[torch.randint(0, len(values), shape, generator=g)].to(dev)


def _exact_product(dY, X):
    """dY^T X and the column sums of dY for integer-valued (or coarse dyadic) operands: fp64 is exact here."""
    y, x = dY.double(), X.double()
    return (y.transpose(0, 1) @ x), y.sum(0)


@pytest.mark.parametrize("N,K", WGRAD_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_weight_gradient_is_exact_on_integers(dev, dtype, N, K):
    """dY, X integers in {-2..2} (exact in fp32 and bf16): every partial sum is an integer below 2^24, so the result does
    not depend on the summation order and dW, db must be the reference's bits -- at every row count of _row_counts, for
    bf16 in both walk directions (flags bit 1), and with db == NULL."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    for M in _row_counts(N, K, n_cu):
        dY = _draw(dev, 1000 + M, (M, N), [-2.0, -1.0, 0.0, 1.0, 2.0])
        X = _draw(dev, 2000 + M, (M, K), [-2.0, -1.0, 0.0, 1.0, 2.0])
        assert 4 * M < 2 ** 24
        want_w, want_b = _exact_product(dY, X)
        for flags in ((0,) if dtype == F32 else (0, 2)):
            dW, db = _call_wgrad(dev, dY, X, M, N, K, dtype, flags)
            plan = _plan(M, N, K, n_cu)
            assert torch.equal(dW.double(), want_w), (M, flags, plan, "dW", float((dW.double() - want_w).abs().max()))
            assert torch.equal(db.double(), want_b), (M, flags, plan, "db", float((db.double() - want_b).abs().max()))
        dW2, _ = _call_wgrad(dev, dY, X, M, N, K, dtype, 0, with_db=False)
        assert torch.equal(dW2, dW), (M, "dW changes when db is NULL")


# x values of the gelu arm (bf16-exact, so the door's rounding keeps them) and the gate on them
GELU_X = [0.0, 1.0, 1.5, 2.0, 3.0, 4.0]


def _gelu_table():
    """bf16(gelu_tanh(x)) per GELU_X value -- accepted only if the fp32 tanh-gelu perturbed by +-16 ulp (the issue asks 4;
    the kernel's is x * rcp(1 + exp(-2u)) with ~1 ulp v_exp / v_rcp) still rounds to the same bf16 value."""
    x = torch.tensor(GELU_X, dtype=torch.float32)
    assert torch.equal(x.to(torch.bfloat16).float(), x)
    g = torch.nn.functional.gelu(x.double(), approximate="tanh").float()
    want = g.to(torch.bfloat16)
    bits = g.view(torch.int32)
    for d in (-16, -4, 4, 16):
        moved = torch.where(g != 0, (bits + d).view(torch.float32), g)          # gelu(0) is an exact 0 in any arithmetic
        assert torch.equal(moved.to(torch.bfloat16), want), (d, GELU_X)
    alt = (x * torch.sigmoid(2.0 * 0.7978845608028654 * (x + 0.044715 * x * x * x))).to(torch.bfloat16)
    assert torch.equal(alt, want)
    return want.float()


@pytest.mark.parametrize("N,K", WGRAD_SHAPES)
def test_weight_gradient_with_gelu_on_the_operand_is_exact(dev, N, K):
    """flags bit 0 (wgrad16_kernel<true>, the fc2 weight gradient): X from GELU_X, dY in {-1, 0, 1} (half of it 0).  Every
    term dY * bf16(gelu(x)) is a multiple of the finest quantum among the table's values; where the sum of |terms| of an
    output stays below 2^24 such quanta, every partial sum is exact in fp32 in any order, and dW must equal
    sum(dY * bf16(gelu(x))) bit for bit -- at every row count, the largest included, in both walk directions."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    table = _gelu_table()
    nz = table[table != 0]
    quantum = float(torch.exp2(torch.floor(torch.log2(nz.abs())) - 7).min())     # a bf16 value has 8 significant bits
    assert torch.equal(torch.round(table.double() / quantum) * quantum, table.double())
    for M in _row_counts(N, K, n_cu):
        dY = _draw(dev, 3000 + M, (M, N), [-1.0, 0.0, 0.0, 1.0])
        idx = torch.randint(0, len(GELU_X), (M, K), generator=torch.Generator(device="cpu").manual_seed(4000 + M)).to(dev)
        X = torch.tensor(GELU_X, device=dev)[idx]
        G = table.to(dev)[idx]
        bound = (dY.abs().double().transpose(0, 1) @ G.abs().double()).max()
        assert float(bound) < 2 ** 24 * quantum, (M, float(bound), quantum)
        want_w, want_b = _exact_product(dY, G)
        for flags in (1, 3):
            dW, db = _call_wgrad(dev, dY, X, M, N, K, BF16, flags)
            assert torch.equal(dW.double(), want_w), (M, flags, _plan(M, N, K, n_cu), float((dW.double() - want_w).abs().max()))
            assert torch.equal(db.double(), want_b), (M, flags, "db")


def test_weight_gradient_door_refuses_what_it_does_not_cover(dev):
    from t2ms_amd import _lib as L
    lib = L.lib()
    a = torch.zeros(64, 256, device=dev)
    w = torch.zeros(256, 256, device=dev)
    st = L.stream_ptr(dev)
    p = a.data_ptr()
    assert lib.t2s_wgrad(p, p, w.data_ptr(), None, 64, 96, 128, F32, 0, st) != 0          # N % 128
    assert b"unsupported shape" in lib.t2s_last_error()
    assert lib.t2s_wgrad(p, p, w.data_ptr(), None, 64, 128, 64, BF16, 0, st) != 0         # K % 128
    assert lib.t2s_wgrad(p, p, w.data_ptr(), None, 0, 128, 128, F32, 0, st) != 0          # M
    assert lib.t2s_wgrad(p, p, w.data_ptr(), None, 64, 128, 128, F32, 1, st) != 0         # gelu is a bf16 kernel
    assert b"bf16" in lib.t2s_last_error()
    assert lib.t2s_wgrad(p, p, w.data_ptr(), None, 64, 128, 128, 7, 0, st) != 0
    assert lib.t2s_attn_train(p, p, p, p, p, p, p, 0, F32, st) != 0
    assert lib.t2s_attn_train(p, p, p, p, p, p, p, 1, 7, st) != 0
    assert lib.t2s_attn_train(None, p, p, p, p, p, p, 1, F32, st) != 0
