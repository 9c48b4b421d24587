"""Host side of the HIP engine of TS2Vec.fit (csrc/t2s_ts2vec_train.hip): the C ABI's new symbols and struct layouts, the
helper that draws a whole fit's random numbers up front, and the refusal to run without a GPU.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "ts2vec_fit.npz")
NEW = ("t2s_ts2vec_train_workspace_bytes", "t2s_ts2vec_train_step", "t2s_swa_update_multi")


def test_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s.h")).read(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.SYMBOLS["t2s_ts2vec_train_workspace_bytes"][0] is C.c_uint64
    assert re.search(r"#define\s+T2S_TS2VEC_TRAIN_MAX_T\s+%d\b" % L.TS2VEC_TRAIN_MAX_T, header)
    assert re.search(r"#define\s+T2S_TS2VEC_TRAIN_MAX_B\s+%d\b" % L.TS2VEC_TRAIN_MAX_B, header)


def test_struct_layouts_match_the_header():
    nb = L.TS2VEC_MAX_BLOCKS
    assert C.sizeof(L.Ts2vecWeights) == 16 + 8 * (4 + 4 * nb)
    assert C.sizeof(L.Ts2vecGrads) == 8 * (4 + 4 * nb)                # the same pointers without the four sizes
    assert [f[0] for f in L.Ts2vecGrads._fields_] == [f[0] for f in L.Ts2vecWeights._fields_[4:]]
    assert C.sizeof(L.Ts2vecView) == 3 * 8 + 2 * 4
    assert C.sizeof(L.Ts2vecStep) == 8 + 8 * 4 + 2 * C.sizeof(L.Ts2vecView)
    assert L.Ts2vecStep.view.offset == 40 and L.Ts2vecStep.alpha.offset == 24 and L.Ts2vecView.length.offset == 24
    assert C.sizeof(L.AdamwTensor) == 40


def _model(seed, **kw):
    from t2ms_amd.ts2vec import TS2Vec
    torch.manual_seed(seed)
    np.random.seed(seed)
    return TS2Vec(input_dims=1, device="cpu", batch_size=8, lr=0.001, output_dims=100, max_train_length=3000, **kw)


def test_plan_fed_to_the_torch_arithmetic_reproduces_the_reference_curve():
    """The draws of 12 iterations under seeds 7, taken up front by draw_plan, then the torch arithmetic on the CPU: the
    reference's own loss curve (rtol 1e-6, the bar of test_fit_reproduces_the_reference_loss_curve_on_cpu)."""
    from t2ms_amd import ts2vec as T
    g = np.load(GOLD)
    m = _model(7)
    plan = m.draw_plan(g["ori"].copy(), n_iters=12)
    assert sum(ev[0] == "iter" for ev in plan) == 12 and sum(ev[0] == "epoch" for ev in plan) == len(g["epoch_log"])
    opt = torch.optim.AdamW(m._net.parameters(), lr=m.lr)
    losses, log, cum = [], [], []
    for ev in plan:
        if ev[0] == "epoch":
            log.append(sum(cum, 0.0) / len(cum))
            cum = []
            continue
        d = ev[1]
        assert d.x.shape == (8, 24, 1) and 2 <= d.crop_l <= 24
        opt.zero_grad()
        outs = []
        for start, length, mask, keep in d.views:
            assert mask.shape == (8, length) and keep.shape == (8, 100, length) and d.crop_l <= length <= 24
            assert (start >= 0).all() and (start + length <= 24).all()
            outs.append(m._net(T._take_rows(d.x, start, length), mask, keep))
        loss = T.hierarchical_contrastive_loss(outs[0][:, -d.crop_l:], outs[1][:, :d.crop_l])
        loss.backward()
        opt.step()
        m.net.update_parameters(m._net)
        losses.append(loss.item())
        cum.append(loss.item())
    np.testing.assert_allclose(np.asarray(losses), g["losses"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(np.asarray(log), g["epoch_log"], rtol=1e-6)


@pytest.mark.parametrize("n_iters", [12, 7])
def test_plan_leaves_both_generators_where_the_torch_fit_leaves_them(n_iters):
    g = np.load(GOLD)
    m = _model(7)
    m.fit(g["ori"].copy(), n_iters=n_iters)
    t_fit, n_fit = torch.get_rng_state(), np.random.get_state()
    m = _model(7)
    plan = m.draw_plan(g["ori"].copy(), n_iters=n_iters)
    assert sum(ev[0] == "iter" for ev in plan) == n_iters
    assert m.n_iters == 0 and m.n_epochs == 0                      # the helper does not touch the model
    assert torch.equal(torch.get_rng_state(), t_fit)
    n_plan = np.random.get_state()
    assert n_plan[0] == n_fit[0] and np.array_equal(n_plan[1], n_fit[1]) and n_plan[2:] == n_fit[2:]


def test_engine_selection_and_no_cpu_path(monkeypatch):
    from t2ms_amd import ts2vec as T
    monkeypatch.delenv("T2S_TS2VEC_FIT", raising=False)
    assert _model(1).engine == "torch" and _model(1, engine="torch").engine == "torch"
    with pytest.raises(L.T2SError, match="GPU"):
        _model(1, engine="hip")
    monkeypatch.setenv("T2S_TS2VEC_FIT", "hip")
    with pytest.raises(L.T2SError, match="GPU"):
        _model(1)
    assert _model(1, engine="torch").engine == "torch"            # a named engine wins over the environment
    with pytest.raises(L.T2SError, match="GPU"):
        T.initialize_ts2vec(np.zeros((8, 24, 1), np.float32), device="cpu")
    with pytest.raises(L.T2SError, match="engine"):
        _model(1, engine="triton")


def test_evaluation_driver_names_the_engine_and_leaves_it_unset_by_default():
    import evaluation
    p = evaluation.build_parser()
    assert p.parse_args([]).cfid_engine is None                    # unset: T2S_TS2VEC_FIT, else torch -- today's behaviour
    assert p.parse_args(["--cfid_engine", "hip"]).cfid_engine == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(["--cfid_engine", "triton"])
