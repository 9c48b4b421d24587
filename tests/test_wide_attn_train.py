"""The training attention at the wide token counts, ALONE (t2s_attn_train_n: the launchers of a wide handle's training step
on plain buffers; attn_train_fwd_kernel<0>, attn_dsum_kernel<0>, attn_bwd_dq_kernel<0>, attn_bwd_dkv_kernel<0>, which stage
their LDS operand pair in chunks of 512 rows).  Needs an MI355X.

Method of tests/test_train_kernels.py: a PEAKED softmax (N(0,1) q, k, v, dO plus spikes in every head), fp64 torch autograd
as the reference, and a bar of 4 x the deviation of an fp32 CPU restatement of the kernels' algorithm from that reference,
never above the bars the suite already has (2e-4 of absmax per gradient tensor, 3e-5 absolute for o, 2e-3 absolute for the
lse).  The spikes are placed for the chunking: the twin keys of query 200 sit at keys 37 and n_tok - 70 (any split into two
or more chunks separates them: the row's P = 0.5 / 0.5 is only right if the lse joins the chunks), the twins of query 7
at n_tok - 33 and n_tok - 1 (the last two blocks; at 800 tokens the ragged last chunk), and query 7's first key block is
hugely negative while its maximum sits in the last block (the running maximum is carried across the chunk border).

profiles/wide_train_errors.md holds the figures these tests print (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1                                   # T2S_TRAIN_F32 / T2S_TRAIN_BF16
E_INVALID = -1                                     # T2S_E_INVALID
NH, DH = 4, 32
SCALE = 32 ** -0.5
QS = float(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))   # t2s_attn_bwd.hip QS
LN2 = float(np.log(2.0))
SEED = 4102
_EXISTING_ABS = {"o": 3e-5, "lse": 2e-3}
_EXISTING_REL = 2e-4


def _qrows(N):
    return (200, 7, 100, 0, N - 1)


def _krows(N):
    return (N - 70, 37, N - 1, N - 33, N - 147, 45)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ inputs
def _sequence(seed, N):
    """One sequence: q, k, v, dO (4, N, 32) fp32, spikes and twins in every head."""
    rs = np.random.RandomState(seed)
    q, k, v, do = (torch.from_numpy(rs.randn(NH, N, DH).astype(np.float32)) for _ in range(4))
    unit = lambda row: q[:, row] * (DH / q[:, row].pow(2).sum(-1, keepdim=True))   # u with q . u = 32 in every head
    k[:, N - 147] = unit(100) * 5.0
    k[:, 45] = unit(N - 1) * 4.0
    k[:, N - 2] = unit(0) * 4.0
    k[:, N - 70] = unit(200) * 12.0                    # a late block ...
    k[:, 0:32] = -unit(7).unsqueeze(1) * 3.0 + 0.01 * k[:, 0:32]   # first block hugely negative for query 7 ...
    k[:, N - 1] = unit(7) * 10.0                       # ... and its real maximum in the last block
    k[:, N - 100] = unit(390) * 12.0
    k[:, 400] = unit(N - 10) * 12.0
    k[:, 530] = unit(270) * 12.0                       # query in chunk 0, key in chunk 1
    k[:, 300] = unit(545) * 12.0                       # query in chunk 1, key in chunk 0
    for key, qrow, gain in ((37, 200, 12.0), (N - 33, 7, 10.0)):       # twins of keys N - 70 and N - 1: same score, another direction
        qq = q[:, qrow].double()
        r = torch.from_numpy(rs.randn(NH, DH))
        r = r - (r * qq).sum(-1, keepdim=True) / (qq * qq).sum(-1, keepdim=True) * qq
        k[:, key] = (gain * unit(qrow).double() + 2.0 * r).float()
    return q, k, v, do


def _inputs(n_seq, N):
    """n_seq = 1 is the sequence of seed SEED; n_seq = 3 carries that same sequence in the middle."""
    seeds = [SEED] if n_seq == 1 else [SEED + 1, SEED, SEED + 2]
    parts = [_sequence(s, N) for s in seeds]
    return tuple(torch.cat([p[i] for p in parts]).contiguous() for i in range(4))       # (BH, N, 32) each


def _rows(t):      # heads (BH, N, 32) -> token rows (n_seq * N, 128)
    BH, N, _ = t.shape
    return t.reshape(BH // NH, NH, N, DH).permute(0, 2, 1, 3).reshape(BH // NH * N, NH * DH).contiguous()


def _heads(t, N):  # token rows (n_seq * N, 128) -> heads (BH, N, 32)
    n_seq = t.shape[0] // N
    return t.reshape(n_seq, N, NH, DH).permute(0, 2, 1, 3).reshape(n_seq * NH, N, DH).contiguous()


# ------------------------------------------------------------------------------------------------ references
def _reference(q, k, v, do):
    """fp64 autograd of softmax(q k^T / sqrt(32)) v; q, k, v, do fp64 heads (BH, N, 32)."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = torch.softmax(s, dim=-1) @ v
    o.backward(do)
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), dim=-1) / LN2, "dq": q.grad, "dk": k.grad, "dv": v.grad,
            "s2": s.detach() / LN2}


def _restate_f32(q, k, v, do):
    """The fp32 kernels' algorithm in fp32 torch (t2s_attn_bwd.hip): scores in the log2 domain, lse = m + log2(l),
    P = exp2(S - lse), D = sum(dO * O), dS = P * (dP - D)."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    s = (q * QS) @ k.transpose(-1, -2)
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


def _check_reference(ref, N):
    """What the inputs are built for, asserted on the fp64 reference before any kernel is looked at."""
    s2, lse, dq, dk = ref["s2"], ref["lse"], ref["dq"], ref["dk"]
    p = torch.exp2(s2 - lse.unsqueeze(-1))
    assert 37 // 512 != (N - 70) // 512, "the first twins share a chunk"
    assert (N - 33) // 32 == N // 32 - 2 and (N - 1) // 32 == N // 32 - 1, "the second twins are not in the last two blocks"
    for qrow, a, b in ((200, N - 70, 37), (7, N - 1, N - 33)):
        assert float(p[:, qrow, a].min()) > 0.25 and float(p[:, qrow, b].min()) > 0.25, "twins do not share the row"
        assert float(lse[:, qrow].min()) > 50.0
        assert float((lse[:, qrow] - s2[:, qrow, 0:32].amax(-1)).min()) > 45.0
    assert float(s2[:, 7, 0:32].amax(-1).max()) < -10.0          # query 7: even the first block's maximum is far below 0
    assert bool((s2[:, 7].argmax(-1) >= N - 64).all())           # ... and its maximum sits in the last two blocks
    med = float(dq.abs().amax(-1).median())
    for qrow in (200, 7):                                        # with one spike, or identical twins, these rows would be 0
        top = dq[:, qrow].abs().amax(-1)
        # (0.25 SCALE (dO . (v_a - v_b)) (k_a - k_b): small in a head by the chance of dO . (v_a - v_b), never in most)
        assert float((top > 0.25 * med).float().mean()) >= 0.5 and float(top.max()) > 2.0 * med, "a twin row carries no gradient"
    for krow in (N - 70, 37, N - 1, N - 33):
        assert float(dk[:, krow].abs().amax(-1).min()) > 2.0


_CASES = {}


def _case(n_seq, N):
    """Inputs, fp64 reference and fp32 CPU restatement of one (n_seq, N), computed once and left unchanged."""
    if (n_seq, N) not in _CASES:
        q, k, v, do = _inputs(n_seq, N)
        ref = _reference(*(t.double() for t in (q, k, v, do)))
        _check_reference(ref, N)
        _CASES[(n_seq, N)] = {"in": (q, k, v, do), "ref": ref, "res": _restate_f32(q, k, v, do)}
    return _CASES[(n_seq, N)]


# ------------------------------------------------------------------------------------------------ the kernels
_RUNS = {}


def _call(dev, q, k, v, do_rows, n_seq, N, dtype=F32, entry="t2s_attn_train_n"):
    from t2ms_amd import _lib as L
    qd, kd, vd, dod = (t.contiguous().to(dev) for t in (q, k, v, do_rows))
    nan = float("nan")
    od = torch.full((n_seq * N, NH * DH), nan, device=dev)
    lsed = torch.full((n_seq * NH, N), nan, device=dev)
    dd = torch.full((n_seq * N, 3 * NH * DH), nan, device=dev)
    ptrs = (qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), dod.data_ptr(), od.data_ptr(), lsed.data_ptr(), dd.data_ptr())
    if entry == "t2s_attn_train_n":
        L.check(L.lib().t2s_attn_train_n(*ptrs, n_seq, N, dtype, L.stream_ptr(dev)), entry)
    else:
        assert N == 480
        L.check(L.lib().t2s_attn_train(*ptrs, n_seq, dtype, L.stream_ptr(dev)), entry)
    return od.cpu(), lsed.cpu(), dd.cpu()


def _run(dev, n_seq, N):
    if (n_seq, N) not in _RUNS:
        q, k, v, do = _case(n_seq, N)["in"]
        _RUNS[(n_seq, N)] = _call(dev, q, k, v, _rows(do), n_seq, N)
    return _RUNS[(n_seq, N)]


def _unpack(raw, N):
    o_rows, lse, dqkv = raw
    for t in raw:
        assert torch.isfinite(t).all(), "an output element was not written, or is not finite"
    g = dqkv.reshape(-1, 3, NH * DH)
    return {"o": _heads(o_rows, N).double(), "lse": lse.double(), "dq": _heads(g[:, 0], N).double(),
            "dk": _heads(g[:, 1], N).double(), "dv": _heads(g[:, 2], N).double()}


def _measure(got, ref, N):
    """{(tensor, row or None): max abs error over absmax}: per tensor, and per named row (worst head) over that row's own
    absmax -- a gradient row smaller than the tensor's median row is taken relative to the median row, as in
    tests/test_train_kernels.py (_measure there says why)."""
    out = {}
    size = lambda t: t.abs().amax(-1)
    for name in ("o", "lse", "dq", "dk", "dv"):
        g, r = got[name], ref[name]
        out[(name, None)] = float((g - r).abs().max() / r.abs().max())
        for row in (_qrows(N) if name in ("o", "dq") else _krows(N) if name in ("dk", "dv") else ()):
            den = size(r[:, row])
            if name != "o":
                den = torch.clamp(den, min=float(size(r).median()))
            out[(name, row)] = float((size(g[:, row] - r[:, row]) / den).max())
    return out


def _bars(case, N):
    """4 x the deviation of the fp32 restatement from the fp64 reference, per tensor and per named row; per tensor never
    above the bar the suite already has."""
    ref = case["ref"]
    dev_ = _measure(case["res"], ref, N)
    bars = {}
    for key, d in dev_.items():
        bar = 4.0 * d
        if key[1] is None:
            name = key[0]
            cap = _EXISTING_ABS[name] / float(ref[name].abs().max()) if name in _EXISTING_ABS else _EXISTING_REL
            bar = min(bar, cap)
        bars[key] = bar
    return dev_, bars


@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("N", [800, 1024])
def test_wide_attention_forward_and_backward_on_a_peaked_softmax(dev, N, n_seq):
    """o, lse, dq, dk, dv of t2s_attn_train_n against fp64 autograd, per tensor and per named spike row; outputs pre-filled
    with NaN must come back finite.  Measured on an MI355X (profiles/wide_train_errors.md)."""
    case = _case(n_seq, N)
    got = _unpack(_run(dev, n_seq, N), N)
    dev_, bars = _bars(case, N)
    err = _measure(got, case["ref"], N)
    bad = []
    for key in sorted(bars, key=lambda kr: (kr[0], -1 if kr[1] is None else kr[1])):
        name, row = key
        print(f"wide_train_errors | attention f32 N={N} n_seq={n_seq} | {name} | {'tensor' if row is None else 'row %d' % row} | "
              f"kernel {err[key]:.3e} | restatement {dev_[key]:.3e} | bar {bars[key]:.3e}")
        if not err[key] <= bars[key]:
            bad.append((name, row, err[key], bars[key]))
    assert not bad, bad


def test_wide_attention_rows_do_not_depend_on_the_batch(dev):
    """n_seq = 3 whose middle sequence is the n_seq = 1 input reproduces that run's rows bit for bit (800 tokens: the
    ragged last chunk, and workgroups of 7, 6, 6, 6 tiles)."""
    N = 800
    one, three = _run(dev, 1, N), _run(dev, 3, N)
    assert torch.equal(three[0][N:2 * N], one[0]), "o"
    assert torch.equal(three[1][NH:2 * NH], one[1]), "lse"
    assert torch.equal(three[2][N:2 * N], one[2]), "dqkv"


def test_two_runs_at_1024_tokens_are_bit_equal(dev):
    q, k, v, do = _case(3, 1024)["in"]
    again = _call(dev, q, k, v, _rows(do), 3, 1024)
    for a, b in zip(_run(dev, 3, 1024), again):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_n_tok_480_gives_the_bits_of_t2s_attn_train(dev):
    """t2s_attn_train_n(n_tok = 480) against t2s_attn_train on the inputs of tests/test_train_kernels.py, n_seq 3."""
    from test_train_kernels import _inputs as inputs480, _rows as rows480
    q, k, v, do = inputs480(3)
    a = _call(dev, q, k, v, rows480(do), 3, 480, entry="t2s_attn_train")
    b = _call(dev, q, k, v, rows480(do), 3, 480, entry="t2s_attn_train_n")
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_unsupported_token_counts_and_dtypes_are_refused(dev):
    from t2ms_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    buf = torch.zeros(4 * 1024 * 32 * 3, device=dev)
    p = buf.data_ptr()
    for n_tok, dtype, word in ((512, F32, b"n_tok=512"), (800, BF16, b"T2S_TRAIN_BF16"), (0, F32, b"n_tok=0"), (1024, 7, b"dtype")):
        assert lib.t2s_attn_train_n(p, p, p, p, p, p, p, 1, n_tok, dtype, st) == E_INVALID, (n_tok, dtype)
        msg = lib.t2s_last_error()
        assert b"t2s_attn_train_n" in msg and word in msg, msg
    assert lib.t2s_attn_train_n(None, p, p, p, p, p, p, 1, 800, F32, st) == E_INVALID
