"""t2s_ts2vec_encode_long (csrc/t2s_ts2vec_encode.hip) on the GPU: parity with oracle.ts2vec_encode and the reference's
fixtures at the bar of test_ts2vec_encoder_reference_fixture (every element within 1e-4 of max|rep|), the bitwise
properties the header promises, the mirror's routing and chunking, C-FID end to end at L = 160, and the refusals."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M
from t2ms_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
E_INVALID = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _load(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name + ".npz")).items()}


@functools.lru_cache(maxsize=None)
def _sd(input_dims=1, output_dims=100, hidden=64, depth=10):
    return synth.make_ts2vec_state_dict(2025, input_dims=input_dims, output_dims=output_dims, hidden=hidden, depth=depth)


@functools.lru_cache(maxsize=None)
def _encoder(dev, **kw):
    return M.TS2VecEncoder(_sd(**kw), dev)


@functools.lru_cache(maxsize=None)
def _case(input_dims, T, B, **kw):
    """(x, oracle rep, oracle full) of a seeded (B, T, input_dims) batch with a NaN stretch in its last series; read-only."""
    x = np.random.RandomState(1000 * input_dims + T).uniform(0, 1, size=(B, T, input_dims)).astype(np.float32)
    if T >= 8:
        x[B - 1, T // 2:T // 2 + 3, input_dims - 1] = np.nan
    with torch.no_grad():
        rep, full = O.ts2vec_encode(_sd(input_dims=input_dims, **kw), torch.from_numpy(x))
    out = (x, rep.numpy(), full.numpy())
    for a in out:
        a.setflags(write=False)
    return out


def _long(enc, x, rep=True, fill=None):
    """A direct t2s_ts2vec_encode_long call with a workspace of exactly workspace_bytes: (rep or None, full) on the host."""
    xs = torch.from_numpy(np.array(x, dtype=np.float32)).contiguous().to(enc.device)
    B, T = xs.shape[0], xs.shape[1]
    need =L.lib().t2s_ts2vec_encode_workspace_bytes(C.byref(enc._w), B, T)
    assert need > 0, L.lib().t2s_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=enc.device)
    if fill is not None:
        ws.fill_(fill)
    full = torch.empty(B, enc._w.output_dims, device=enc.device)
    r = torch.empty(B, T, enc._w.output_dims, device=enc.device) if rep else None
    with torch.cuda.device(enc.device):
        L.check(L.lib().t2s_ts2vec_encode_long(C.byref(enc._w), xs.data_ptr(), None if r is None else r.data_ptr(), full.data_ptr(),
                                               B, T, ws.data_ptr(), need, L.stream_ptr(enc.device)), "t2s_ts2vec_encode_long")
    return (None if r is None else r.cpu().numpy()), full.cpu().numpy()


def _check(got_rep, got_full, want_rep, want_full, stride=1):
    scale = float(np.abs(want_rep).max())
    assert scale > 0.1
    assert np.isfinite(got_rep).all() and np.isfinite(got_full).all()
    err_rep = float(np.abs(got_rep[:, ::stride] - want_rep).max())
    err_full = float(np.abs(got_full - want_full).max())
    print(f"max|rep| {scale:.4f}  rep error {err_rep / scale:.3e}  full error {err_full / scale:.3e}  (bar {TOL:.0e})")
    assert err_rep <= TOL * scale
    assert err_full <= TOL * scale


@pytest.mark.parametrize("input_dims,T,B", [(1, 137, 3), (10, 300, 3), (1, 1025, 2), (1, 4096, 1),
                                            (1, 1, 2), (1, 2, 2), (1, 31, 2), (1, 33, 2), (1, 129, 2)])
def test_parity_with_the_oracle_at_default_sizes(dev, input_dims, T, B):
    """(1, 137): the first length the LDS kernel refuses; (1, 1025): dilation 1024 is live for one pair of steps; 4096: the
    upper bound; T in {1, 2, 31, 33, 129}: tile tails and blocks that run their centre tap only."""
    x, rep, full = _case(input_dims, T, B)
    got_rep, got_full = _long(_encoder(dev, input_dims=input_dims), x)
    assert got_rep.shape == (B, T, 100) and got_full.shape == (B, 100)
    _check(got_rep, got_full, rep, full)


def test_parity_at_sizes_that_are_no_multiple_of_the_tile(dev):
    kw = dict(input_dims=3, hidden=48, output_dims=36, depth=3)
    x, rep, full = _case(3, 70, 5, hidden=48, output_dims=36, depth=3)
    got_rep, got_full = _long(_encoder(dev, **kw), x, fill=0xFF)      # a workspace full of NaNs: padding rows must not leak
    assert got_rep.shape == (5, 70, 36)
    _check(got_rep, got_full, rep, full)


def test_reference_fixtures(dev, golden_dir):
    """The x of ts2vec.npz (T = 96, a NaN stretch) and the three cases of ts2vec_long.npz through the new entry, against
    what the reference's TSEncoder recorded."""
    g = _load(golden_dir, "ts2vec")
    got_rep, got_full = _long(_encoder(dev), g["x"])
    _check(got_rep, got_full, g["rep"], g["full_series"], stride=6)
    g = _load(golden_dir, "ts2vec_long")
    for k, (cin, T, B, stride) in enumerate(g["cases"]):
        got_rep, got_full = _long(_encoder(dev, input_dims=int(cin)), g[f"x_{k}"])
        assert got_rep.shape == (B, T, 100)
        _check(got_rep, got_full, g[f"rep_{k}"], g[f"full_{k}"], stride=int(stride))


def test_nan_steps_give_finite_output(dev):
    x = np.random.RandomState(4).uniform(0, 1, size=(2, 200, 10)).astype(np.float32)
    x[0, :7, 3] = np.nan
    x[0, 150:, :] = np.nan
    x[1, 199, 9] = np.nan
    rep, full = _long(_encoder(dev, input_dims=10), x)
    assert np.isfinite(rep).all() and np.isfinite(full).all()
    with torch.no_grad():
        want_rep, want_full = O.ts2vec_encode(_sd(input_dims=10), torch.from_numpy(x))
    _check(rep, full, want_rep.numpy(), want_full.numpy())


def test_bitwise_properties(dev):
    """Same bits on a second call (whatever the workspace held); row i of a batch equals that row alone; full equals the
    maximum over time of the returned rep; rep = NULL gives the same full."""
    enc = _encoder(dev)
    x, _, _ = _case(1, 300, 3)
    rep, full = _long(enc, x, fill=0)
    rep2, full2 = _long(enc, x, fill=0xFF)
    assert np.array_equal(rep, rep2) and np.array_equal(full, full2)
    for i in range(3):
        r1, f1 = _long(enc, x[i:i + 1])
        assert np.array_equal(r1[0], rep[i]) and np.array_equal(f1[0], full[i])
    assert np.array_equal(full, rep.max(axis=1))
    none, full3 = _long(enc, x, rep=False)
    assert none is None and np.array_equal(full3, full)


def test_mirror_chunks_change_no_bit(dev, monkeypatch):
    enc = M.TS2VecEncoder(_sd(), dev)
    x, rep, full = _case(1, 137, 3)
    x = np.array(x)
    one_rep = enc.encode(x, encoding_window=None).cpu().numpy()
    one_full = enc.encode(x).cpu().numpy()
    cap = M._encode_workspace_bytes(1, 137, 64, 100, 10)
    monkeypatch.setattr(M, "ENCODE_WORKSPACE_CAP", cap)
    assert M._encode_chunks(3, 137, 64, 100, 10) == [(0, 1), (1, 1), (2, 1)]
    assert np.array_equal(enc.encode(x, encoding_window=None).cpu().numpy(), one_rep)
    assert np.array_equal(enc.encode(x).cpu().numpy(), one_full)
    _check(one_rep, one_full, rep, full)


def test_mirror_routing(dev):
    enc = M.TS2VecEncoder(_sd(), dev)
    x = np.random.RandomState(6).uniform(0, 1, size=(3, 137, 1)).astype(np.float32)
    # T = 136 with path=None: the bits of a direct t2s_ts2vec_encode call
    xs = torch.from_numpy(x[:, :136]).contiguous().to(dev)
    rep = torch.empty(3, 136, 100, device=dev)
    full = torch.empty(3, 100, device=dev)
    L.check(L.lib().t2s_ts2vec_encode(C.byref(enc._w), xs.data_ptr(), rep.data_ptr(), full.data_ptr(), 3, 136, L.stream_ptr(dev)))
    assert torch.equal(enc.encode(x[:, :136], encoding_window=None), rep) and torch.equal(enc.encode(x[:, :136]), full)
    # T = 137: the LDS kernel refuses, path=None takes the new entry
    with torch.no_grad():
        want_rep, want_full = O.ts2vec_encode(_sd(), torch.from_numpy(x))
    _check(enc.encode(x, encoding_window=None).cpu().numpy(), enc.encode(x).cpu().numpy(), want_rep.numpy(), want_full.numpy())
    with pytest.raises(L.T2SError, match="exceed the 160 KB LDS"):
        enc.encode(x, path="lds")
    with pytest.raises(L.T2SError, match="path"):
        enc.encode(x, path="torch")
    # a forced 'gemm' at a length the LDS kernel takes
    with torch.no_grad():
        want_rep, want_full = O.ts2vec_encode(_sd(), torch.from_numpy(x[:, :96]))
    _check(enc.encode(x[:, :96], encoding_window=None, path="gemm").cpu().numpy(), enc.encode(x[:, :96], path="gemm").cpu().numpy(),
           want_rep.numpy(), want_full.numpy())


def test_cfid_end_to_end_at_160_steps(dev):
    """TS2Vec trained 3 iterations (torch engine) on 16 series of L = 160, then C-FID of two sets through TS2Vec.encode
    (the long entry: 160 > 136) against the oracle's FID of the oracle's encodings under the trained weights.  The three
    iterations run on the CPU (the torch engine runs wherever the module lives; a first GPU backward costs seconds of
    library start-up) and the trained weights move to a GPU model, whose encode is what is under test."""
    from t2ms_amd.ts2vec import TS2Vec
    torch.manual_seed(11)
    np.random.seed(11)
    rs = np.random.RandomState(12)
    train = rs.uniform(0, 1, size=(16, 160, 1)).astype(np.float32)
    kw = dict(input_dims=1, output_dims=100, batch_size=8, max_train_length=3000, engine="torch")
    fitted = TS2Vec(device="cpu", **kw)
    fitted.fit(train, n_iters=3)
    model = TS2Vec(device=dev, **kw)
    model.net.load_state_dict(fitted.net.state_dict())
    model._hip = None
    a = rs.uniform(0, 1, size=(40, 160, 1)).astype(np.float32)
    b = (a + 0.2 * rs.randn(40, 160, 1)).astype(np.float32)
    sd = {k: v.detach().cpu().float() for k, v in model.net.module.state_dict().items()}
    with torch.no_grad():
        ra = O.ts2vec_encode(sd, torch.from_numpy(a))[1].numpy()
        rb = O.ts2vec_encode(sd, torch.from_numpy(b))[1].numpy()
    ea, eb = model.encode(a, encoding_window="full_series"), model.encode(b, encoding_window="full_series")
    assert ea.shape == (40, 100)
    np.testing.assert_allclose(M.fid(ea, eb), O.eval_fid(ra, rb), rtol=2e-3)


def test_refusals_leave_the_outputs_untouched(dev):
    enc = _encoder(dev)
    lib = L.lib()
    st = L.stream_ptr(dev)

    def attempt(w, B, T, x=True, full=True, ws=True, short=0, words=()):
        Tn = min(T, 4096)
        xs = torch.zeros(B, Tn, w.input_dims, device=dev)
        rep = torch.full((B, Tn, w.output_dims), -7.0, device=dev)
        fl = torch.full((B, w.output_dims), -7.0, device=dev)
        need = lib.t2s_ts2vec_encode_workspace_bytes(C.byref(w), B, Tn) or 1 << 20
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
        rc = lib.t2s_ts2vec_encode_long(C.byref(w), xs.data_ptr() if x else None, rep.data_ptr(), fl.data_ptr() if full else None,
                                        B, T, buf.data_ptr() if ws else None, need - short, st)
        msg = lib.t2s_last_error().decode()
        assert rc == E_INVALID, (rc, msg)
        assert "t2s_ts2vec_encode_long" in msg and all(wd in msg for wd in words), msg
        torch.cuda.synchronize(dev)
        assert bool((rep == -7.0).all()) and bool((fl == -7.0).all())

    attempt(enc._w, 2, 4097, words=("T=4097", "4096"))
    attempt(enc._w, 2, 137, x=False, words=("x", "NULL"))
    attempt(enc._w, 2, 137, full=False, words=("full", "NULL"))
    attempt(enc._w, 2, 137, ws=False, words=("workspace", "NULL"))
    attempt(enc._w, 2, 137, short=1, words=("workspace", "bytes"))
    wide = M.TS2VecEncoder(synth.make_ts2vec_state_dict(2025, hidden=129, depth=1), dev)
    attempt(wide._w, 2, 137, words=("hidden=129",))
