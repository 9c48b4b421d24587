"""The HIP engine of TS2Vec.fit (csrc/t2s_ts2vec_train.hip; t2ms_amd.ts2vec.TS2Vec(engine="hip")): one training step's loss
and gradients against fp64 autograd, bit reproducibility, the reference's loss curves of tests/golden/ts2vec_fit.npz, the
C ABI's refusals, and one optimiser + averaging step against torch.

The gradient bar (loss 1e-5 relative; per tensor max|g - g64| <= 2e-5 max|g64|): torch's own fp32 CPU autograd sits at
1.4e-7 .. 1.1e-6 max|g64| per tensor on these configurations, with loss gaps up to 7e-8 (profiles/EXPERIMENTS.md 0.17); the
bar leaves about 20x for another fp32 summation order over up to 2,048 (series, time) terms and is ten times tighter than
the DiT's 2e-4.  Measured for the HIP step on an MI355X: 0.9e-6 .. 2.9e-6 per case (worst tensor), loss gaps <= 1.5e-7."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ts2vec_fit.npz")
DEV = "cuda:0"

# (B, T, hidden, out, depth, input_dims, seed of the draws).  The seeds were picked for their crops: (8,128) draws an odd
# crop_l = 89 with views of 102 and 100 steps; (3,37) draws a view of 34 steps, so the dilation-32 block has live outer taps.
CASES = [(8, 24, 64, 100, 10, 1, 3), (3, 37, 64, 100, 10, 1, 9), (1, 37, 64, 100, 10, 1, 0), (8, 128, 64, 100, 10, 1, 3),
         (16, 96, 64, 100, 10, 1, 1), (5, 13, 16, 24, 3, 2, 0),
         (8, 128, 64, 100, 10, 1, -1)]      # seed -1: no crop at all, both views are the full 128 steps (the LDS limit)


def _draw(B, T, out, cin, seed):
    from t2ms_amd.ts2vec import FitDraw
    rs = np.random.RandomState(abs(seed))
    tg = torch.Generator().manual_seed(abs(seed))
    x = torch.from_numpy(rs.randn(B, T, cin).astype(np.float32))
    if seed < 0:
        crop_l, left, eleft, eright = T, 0, 0, T
    else:
        crop_l = rs.randint(2, T + 1)
        left = rs.randint(T - crop_l + 1)
        eleft = rs.randint(left + 1)
        eright = rs.randint(left + crop_l, T + 1)
    right = left + crop_l
    offs = rs.randint(-eleft, T - eright + 1, size=B)
    views = []
    for start, length in ((offs + eleft, right - eleft), (offs + left, eright - left)):
        mask = torch.from_numpy(rs.binomial(1, 0.5, size=(B, length))).to(torch.bool)
        keep = torch.empty(B, out, length).bernoulli_(0.9, generator=tg).div_(0.9)
        views.append((start, int(length), mask, keep))
    return FitDraw(x, int(crop_l), views)


def _model(B, hidden, out, depth, cin, seed=5, **kw):
    from t2ms_amd.ts2vec import TS2Vec
    torch.manual_seed(seed)
    return TS2Vec(input_dims=cin, output_dims=out, hidden_dims=hidden, depth=depth, device=DEV, batch_size=B, engine="hip", **kw)


class _Step:
    """One t2s_ts2vec_train_step on a model's own tensors, through the ctypes binding."""

    def __init__(self, m, draw):
        self.m = m
        self.w, self.g, self.tables, self.n_tensors, self.chunks, (self.grads, self.moments) = m._hip_tables()
        self.keep, (self.step,) = m._hip_plan([draw])
        B, T, _ = draw.x.shape
        self.ws_bytes = int(L.lib().t2s_ts2vec_train_workspace_bytes(C.byref(self.w), B, T))
        assert self.ws_bytes > 0, L.lib().t2s_last_error()
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        self.loss = torch.zeros(1, device=DEV)

    def call(self, ws_bytes=None):
        return L.lib().t2s_ts2vec_train_step(C.byref(self.w), C.byref(self.g), C.byref(self.step), self.loss.data_ptr(),
                                             self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes,
                                             L.stream_ptr(DEV))

    def run(self):
        L.check(self.call(), "t2s_ts2vec_train_step")
        torch.cuda.synchronize()
        return float(self.loss.item()), {n: self.grads[id(p)].cpu() for n, p in self.m._net.named_parameters()}


def _fp64(m, draw):
    from t2ms_amd import ts2vec as T
    net = copy.deepcopy(m._net).cpu().double()
    x = draw.x.double()
    outs = [net(T._take_rows(x, start, length), mask, keep.double()) for start, length, mask, keep in draw.views]
    loss = T.hierarchical_contrastive_loss(outs[0][:, -draw.crop_l:], outs[1][:, :draw.crop_l])
    assert loss.dtype == torch.float64
    loss.backward()
    return float(loss), {n: p.grad for n, p in net.named_parameters()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-T%d-h%d-o%d-d%d-c%d-s%d" % c)
def test_step_gradients_against_fp64_autograd(case):
    B, T, hidden, out, depth, cin, seed = case
    m = _model(B, hidden, out, depth, cin)
    draw = _draw(B, T, out, cin, seed)
    if case == CASES[3]:
        assert draw.crop_l % 2 == 1 and draw.views[0][1] != draw.views[1][1]
    if case == CASES[1]:
        assert max(draw.views[0][1], draw.views[1][1]) > 32
    st = _Step(m, draw)
    for grad in st.grads.values():
        grad.fill_(float("nan"))                                   # every entry must be overwritten
    loss, grads = st.run()
    loss64, g64 = _fp64(m, draw)
    print(f"case {case}: crop_l {draw.crop_l} views {draw.views[0][1]}/{draw.views[1][1]} loss {loss:.7f} fp64 {loss64:.7f} "
          f"rel {abs(loss - loss64) / abs(loss64):.2e}")
    worst = 0.0
    for n, ref in g64.items():
        got = grads[n].double()
        assert torch.isfinite(got).all(), n
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        worst = max(worst, err / scale)
        print(f"   {n:52s} max|g64| {scale:.3e} err/max {err / scale:.2e}")
        assert err <= 2e-5 * scale, (n, err, scale)
        zero = ref == 0
        assert (got[zero] == 0).all(), (n, "an exactly-zero fp64 gradient is not exactly zero")
    print(f"   worst err/max|g64| {worst:.2e}")
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    # the outer taps of every block whose dilation reaches both view lengths really are among those zeros
    longest = max(draw.views[0][1], draw.views[1][1])
    for i in range(depth + 1):
        if 2 ** i >= longest:
            for conv in ("conv1", "conv2"):
                gw = grads[f"feature_extractor.net.{i}.{conv}.conv.weight"]
                assert (gw[:, :, 0] == 0).all() and (gw[:, :, 2] == 0).all() and (gw[:, :, 1] != 0).any()


def test_step_is_bit_reproducible():
    B, T, hidden, out, depth, cin, seed = CASES[0]
    m = _model(B, hidden, out, depth, cin)
    st = _Step(m, _draw(B, T, out, cin, seed))
    loss_a, a = st.run()
    a = {k: v.clone() for k, v in a.items()}
    st.ws.fill_(0xff)
    loss_b, b = st.run()
    assert loss_a == loss_b
    for k in a:
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


def _fit(seed, n_iters, engine="hip", callback=False, epoch_callback=False):
    from t2ms_amd.ts2vec import TS2Vec
    g = np.load(GOLD)
    torch.manual_seed(seed)
    np.random.seed(seed)
    seen, epochs = [], []
    m = TS2Vec(input_dims=1, device=DEV, batch_size=8, lr=0.001, output_dims=100, max_train_length=3000, engine=engine,
               after_iter_callback=(lambda model, loss: seen.append((loss, model.n_iters))) if callback else None,
               after_epoch_callback=(lambda model, loss: epochs.append(loss)) if epoch_callback else None)
    log = m.fit(g["ori"].copy(), n_iters=n_iters, verbose=False)
    losses = [v for v, _ in seen] if callback else list(m.losses_)
    if callback:
        assert [k for _, k in seen] == list(range(1, len(seen) + 1))     # the callback sees the model of its iteration
    if epoch_callback:
        assert epochs == log
    return g, m, losses, log


@pytest.fixture(scope="module")
def fit12():
    return _fit(7, 12)


def _same_state(a, b):
    sa, sb = a.net.state_dict(), b.net.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    for p, q in zip(a._net.parameters(), b._net.parameters()):
        assert torch.equal(p, q)


def test_fit_is_bit_reproducible_with_and_without_callbacks(fit12):
    _, m, losses, log = fit12
    _, m2, losses2, log2 = _fit(7, 12)
    assert losses == losses2 and log == log2 and len(losses) == 12
    _same_state(m, m2)
    _, m3, losses3, log3 = _fit(7, 12, callback=True, epoch_callback=True)
    assert losses == losses3 and log == log3
    _same_state(m, m3)


def test_fit_12_iterations_follows_the_reference_curve(fit12):
    from t2ms_amd import metrics
    g, m, losses, log = fit12
    assert m.n_iters == 12 and len(losses) == 12
    np.testing.assert_allclose(np.asarray(losses), g["losses"], rtol=2e-3)
    np.testing.assert_allclose(np.asarray(log), g["epoch_log"], rtol=2e-3)
    r_ori = m.encode(g["ori"], encoding_window="full_series")
    r_gen = m.encode(g["gen"], encoding_window="full_series")
    assert r_ori.shape == (24, 100)
    scale = float(np.abs(g["repr_ori"]).max())
    assert float(np.abs(r_ori - g["repr_ori"]).max()) < 2e-2 * scale and float(np.abs(r_gen - g["repr_gen"]).max()) < 2e-2 * scale
    fid_ref = metrics.fid(g["repr_ori"], g["repr_gen"])
    fid_ours = metrics.fid(r_ori, r_gen)
    assert abs(fid_ours - fid_ref) <= 0.05 * abs(fid_ref) + 1e-3, (fid_ours, fid_ref)
    _, mt, losses_t, _ = _fit(7, 12, engine="torch", callback=True)
    assert int(m.net.n_averaged) == int(mt.net.n_averaged) == 13
    assert [m.n_iters, m.n_epochs] == [mt.n_iters, mt.n_epochs]
    np.testing.assert_allclose(np.asarray(losses), np.asarray(losses_t), rtol=2e-3)


def test_default_200_iteration_fit_save_and_load(tmp_path):
    from t2ms_amd.ts2vec import TS2Vec, initialize_ts2vec
    g = np.load(GOLD)
    torch.manual_seed(8)
    np.random.seed(8)
    m = TS2Vec(input_dims=1, device=DEV, batch_size=8, lr=0.001, output_dims=100, max_train_length=3000, engine="hip")
    m.fit(g["ori"].copy(), verbose=False)
    assert [m.n_iters, m.n_epochs] == g["n_iters200"].tolist()
    log = np.asarray(m.losses_)
    np.testing.assert_allclose(log[:10], g["losses200"][:10], rtol=5e-3)
    assert abs(log[-30:].mean() - g["losses200"][-30:].mean()) < 0.15 * g["losses200"][-30:].mean()
    assert log[-30:].mean() < 0.5 * log[:5].mean()
    model = initialize_ts2vec(g["ori"].copy(), device=DEV, engine="hip")
    assert model.engine == "hip" and model.n_iters == 200
    rep = model.encode(g["gen"], encoding_window="full_series")
    assert np.isfinite(rep).all()
    model.save(str(tmp_path / "ts2vec.pt"))
    fresh = TS2Vec(input_dims=1, device=DEV, batch_size=8, lr=0.001, output_dims=100, max_train_length=3000)
    fresh.load(str(tmp_path / "ts2vec.pt"))
    assert fresh.encode(g["gen"], encoding_window="full_series").tobytes() == rep.tobytes()


def test_unsupported_shapes_raise_with_the_librarys_message():
    from t2ms_amd.ts2vec import TS2Vec
    torch.manual_seed(1)
    np.random.seed(1)
    m = TS2Vec(input_dims=1, device=DEV, batch_size=8, output_dims=100, engine="hip")
    with pytest.raises(L.T2SError, match="T=129"):
        m.fit(np.random.randn(16, 129, 1).astype(np.float32), n_iters=1)
    m = TS2Vec(input_dims=1, device=DEV, batch_size=17, output_dims=100, engine="hip")
    with pytest.raises(L.T2SError, match="B=17"):
        m.fit(np.random.randn(34, 24, 1).astype(np.float32), n_iters=1)
    assert m.n_iters == 0


def test_c_abi_refuses_before_any_launch():
    B, T, hidden, out, depth, cin, seed = CASES[5]
    m = _model(B, hidden, out, depth, cin)
    st = _Step(m, _draw(B, T, out, cin, seed))
    lib = L.lib()

    def refused(match):
        with pytest.raises(L.T2SError, match=match):
            L.check(st.call(), "t2s_ts2vec_train_step")

    st.step.T = 129
    refused("T=129")
    st.step.T = T
    st.step.B = 17
    refused("B=17")
    st.step.B = B
    with pytest.raises(L.T2SError, match="workspace"):
        L.check(st.call(ws_bytes=st.ws_bytes - 1), "t2s_ts2vec_train_step")
    keep = st.g.conv2_b[1]
    st.g.conv2_b[1] = None
    refused("grads of block 1")
    st.g.conv2_b[1] = keep
    st.step.x_nan_count = 3
    refused("3 NaN")
    st.step.x_nan_count = 0
    assert lib.t2s_ts2vec_train_workspace_bytes(C.byref(st.w), 17, 24) == 0 and b"B=17" in lib.t2s_last_error()
    assert lib.t2s_ts2vec_train_workspace_bytes(C.byref(st.w), 8, 129) == 0 and b"T=129" in lib.t2s_last_error()
    torch.cuda.synchronize()
    loss, grads = st.run()                                        # and the untouched step still runs
    assert np.isfinite(loss) and all(torch.isfinite(v).all() for v in grads.values())


def test_one_optimiser_and_averaging_step_against_torch():
    """train_step + t2s_adamw_step_multi + t2s_swa_update_multi against torch.optim.AdamW + AveragedModel from identical
    weights, gradients and (zero) moments.  1e-6 absolute: lr is 1e-3 and a normalised first update is at most 1 in
    magnitude, so 1e-6 is a 1e-3 relative band on the update, the +-lr band argument of the resumed-step test."""
    B, T, hidden, out, depth, cin, seed = CASES[0]
    m = _model(B, hidden, out, depth, cin, lr=0.001)
    ref_net = copy.deepcopy(m._net)
    ref_avg = copy.deepcopy(m.net)
    init = [p.detach().clone() for p in m._net.parameters()]
    st = _Step(m, _draw(B, T, out, cin, seed))
    _, grads = st.run()
    lib, stream = L.lib(), L.stream_ptr(DEV)
    adam, swa = st.tables.data_ptr(), st.tables.data_ptr() + 40 * st.n_tensors
    L.check(lib.t2s_adamw_step_multi(adam, st.n_tensors, st.chunks, 0.001, 0.9, 0.999, 1e-8, 0.01, 1, stream))
    L.check(lib.t2s_swa_update_multi(swa, st.n_tensors, st.chunks, int(m.net.n_averaged), stream))
    torch.cuda.synchronize()
    opt = torch.optim.AdamW(ref_net.parameters(), lr=0.001)
    for n, p in ref_net.named_parameters():
        p.grad = grads[n].to(DEV)
    opt.step()
    ref_avg.update_parameters(ref_net)
    for (n, p), q in zip(m._net.named_parameters(), ref_net.parameters()):
        assert float((p - q).abs().max()) <= 1e-6, n
    for (n, p), q in zip(m.net.module.named_parameters(), ref_avg.module.parameters()):
        assert float((p - q).abs().max()) <= 1e-6, n
    # the step did move the weights and the average (not a comparison of untouched copies)
    assert max(float((p - q).abs().max()) for p, q in zip(m._net.parameters(), init)) > 5e-4
    assert max(float((p - q).abs().max()) for p, q in zip(m.net.module.parameters(), init)) > 2e-4
