"""The bf16 training attention at the wide token counts, ALONE (t2s_attn_train_bf16_n: the launchers of a wide handle's bf16
training step on plain buffers; attn16_fwd_kernel<0>, attn16_bwd_dq_kernel<0>, attn16_bwd_dkv_kernel<0>, whose whole operand
pair lives in LDS as bf16 images).  Needs an MI355X.

Inputs: the peaked softmax of tests/test_wide_attn_train.py.  Reference: fp64 autograd on the bf16-ROUNDED operands.  Bars:
the rule of _bars_bf16 in tests/test_train_kernels.py -- per tensor and per named spike row the relative L2 error is at most
2 x that of the fp64-with-roundings restatement (tests/_wide_train_bf16_ref.py); the lse at most min(4 x the fp32
restatement's deviation, 2e-3 absolute).  tests/test_wide_train_bf16_host.py asserts on the CPU that the restatement takes
the 2^40 re-reference branch for query 7 on these inputs.

profiles/wide_train_bf16_errors.md holds the figures these tests print (pytest -s)."""
import pytest
import torch

import _wide_train_bf16_ref as WB
import test_wide_attn_train as WA

pytestmark = pytest.mark.gpu

E_INVALID = -1
NH, DH = WA.NH, WA.DH


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_RUNS = {}


def _call(dev, q, k, v, do_rows, n_seq, N):
    from t2ms_amd import _lib as L
    qd, kd, vd, dod = (t.contiguous().to(dev) for t in (q, k, v, do_rows))
    nan = float("nan")
    od = torch.full((n_seq * N, NH * DH), nan, device=dev)
    lsed = torch.full((n_seq * NH, N), nan, device=dev)
    dd = torch.full((n_seq * N, 3 * NH * DH), nan, device=dev)
    L.check(L.lib().t2s_attn_train_bf16_n(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), dod.data_ptr(), od.data_ptr(), lsed.data_ptr(),
                                          dd.data_ptr(), n_seq, N, L.stream_ptr(dev)), "t2s_attn_train_bf16_n")
    return od.cpu(), lsed.cpu(), dd.cpu()


def _run(dev, n_seq, N):
    if (n_seq, N) not in _RUNS:
        q, k, v, do = WB.case(n_seq, N)["in"]
        _RUNS[(n_seq, N)] = _call(dev, q, k, v, WA._rows(do), n_seq, N)
    return _RUNS[(n_seq, N)]


@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("N", [800, 1024])
def test_wide_bf16_attention_forward_and_backward_on_a_peaked_softmax(dev, N, n_seq):
    """o, lse, dq, dk, dv of t2s_attn_train_bf16_n against fp64 autograd of the rounded operands, per tensor and per named
    spike row; outputs pre-filled with NaN must come back finite.  Measured on an MI355X (profiles/wide_train_bf16_errors.md)."""
    c = WB.case(n_seq, N)
    got = WA._unpack(_run(dev, n_seq, N), N)
    dev_, bars = WB.bars(c, N)
    err = WB.measure(got, c["ref"], N)
    bad = []
    for key in sorted(bars, key=lambda kr: (kr[0], -1 if kr[1] is None else kr[1])):
        name, row = key
        print(f"wide_train_bf16_errors | attention bf16 N={N} n_seq={n_seq} | {name} | {'tensor' if row is None else 'row %d' % row} | "
              f"kernel {err[key]:.3e} | restatement {dev_[key]:.3e} | bar {bars[key]:.3e}")
        if not err[key] <= bars[key]:
            bad.append((name, row, err[key], bars[key]))
    assert not bad, bad


@pytest.mark.parametrize("N", [800, 1024])
def test_wide_bf16_attention_rows_do_not_depend_on_the_batch(dev, N):
    """n_seq = 3 whose middle sequence is the n_seq = 1 input reproduces that run's rows bit for bit."""
    one, three = _run(dev, 1, N), _run(dev, 3, N)
    assert torch.equal(three[0][N:2 * N], one[0]), "o"
    assert torch.equal(three[1][NH:2 * NH], one[1]), "lse"
    assert torch.equal(three[2][N:2 * N], one[2]), "dqkv"


@pytest.mark.parametrize("N", [800, 1024])
def test_two_wide_bf16_attention_runs_are_bit_equal(dev, N):
    q, k, v, do = WB.case(3, N)["in"]
    again = _call(dev, q, k, v, WA._rows(do), 3, N)
    for a, b in zip(_run(dev, 3, N), again):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_n_tok_480_gives_the_bits_of_t2s_attn_train_in_bf16(dev):
    """t2s_attn_train_bf16_n(n_tok = 480) against t2s_attn_train(..., T2S_TRAIN_BF16) on the inputs of
    tests/test_train_kernels.py, n_seq 3."""
    from test_train_kernels import _inputs as inputs480, _rows as rows480
    q, k, v, do = inputs480(3)
    a = WA._call(dev, q, k, v, rows480(do), 3, 480, dtype=WA.BF16, entry="t2s_attn_train")
    b = _call(dev, q, k, v, rows480(do), 3, 480)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_unsupported_token_counts_are_refused_and_the_old_entry_still_refuses_bf16(dev):
    from t2ms_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    buf = torch.zeros(4 * 1024 * 32 * 3, device=dev)
    p = buf.data_ptr()
    for n_tok, word in ((512, b"n_tok=512"), (0, b"n_tok=0")):
        assert lib.t2s_attn_train_bf16_n(p, p, p, p, p, p, p, 1, n_tok, st) == E_INVALID, n_tok
        msg = lib.t2s_last_error()
        assert b"t2s_attn_train_bf16_n" in msg and word in msg, msg
    assert lib.t2s_attn_train_bf16_n(None, p, p, p, p, p, p, 1, 800, st) == E_INVALID
    assert lib.t2s_attn_train_bf16_n(p, p, p, p, p, p, p, 0, 800, st) == E_INVALID
    assert lib.t2s_attn_train_n(p, p, p, p, p, p, p, 1, 800, WA.BF16, st) == E_INVALID
    assert b"T2S_TRAIN_BF16 runs at 480 tokens only" in lib.t2s_last_error()
