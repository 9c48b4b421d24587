"""Host side of the few-step solvers (t2ms_amd.sampler.solver_tables, the drivers' --solver / --sample_steps / --eta): the
grids and refusals, the collapsed coefficient tables against the textbook x0-prediction form restated here in fp64, and the
solvers' order of convergence on a closed form (Gaussian data: the exact denoiser and the exact ODE solution are known).
No GPU: the table-driven update x' = c0*x + c1*pred + c2*h + c3*z, h' = c4*x + c5*pred is applied in numpy."""
import os

import numpy as np
import pytest

from t2ms_amd.model.backbone.DDPM import ddpm_host_tables
from t2ms_amd.sampler import loop_t_values, resolve_solver, solver_grid, solver_tables


def _alpha_bar(T):
    return ddpm_host_tables(T)["alpha_bar"].numpy().astype(np.float64)


def _apply(c, x, pred, h, z):
    """The kernel's update in the dtype of x, with its zero-coefficient rule (an operand with a 0 coefficient is not read)."""
    xn = c[0] * x + c[1] * pred
    if c[2] != 0:
        xn = xn + c[2] * h
    if c[3] != 0:
        xn = xn + c[3] * z
    hn = c[4] * x + c[5] * pred if (c[4] != 0 or c[5] != 0) else h
    return xn, hn


# ---------------------------------------------------------------------------------------------- grids and refusals
def test_trailing_grid():
    assert solver_grid(1000, 10).tolist() == [999, 899, 799, 699, 599, 499, 399, 299, 199, 99]
    assert solver_grid(1000, 1000).tolist() == list(range(999, -1, -1))
    assert solver_grid(50, 50).tolist() == list(range(49, -1, -1))
    assert solver_grid(7, 1).tolist() == [6]
    for T, S in ((1000, 37), (50, 4), (100, 8), (60, 6), (1000, 999)):
        tau = solver_grid(T, S)
        assert tau.shape == (S,) and tau[0] == T - 1 and tau[-1] >= 0 and (np.diff(tau) < 0).all(), (T, S)
    tv, coef = solver_tables("ddpm", "ddim", 1000, 10)
    assert tv.dtype.is_floating_point and tv.tolist() == [999., 899., 799., 699., 599., 499., 399., 299., 199., 99.]
    assert tuple(coef.shape) == (10, 6) and str(coef.dtype) == "torch.float32"
    assert solver_tables("ddpm", "dpmpp2m", 100)[0].tolist() == loop_t_values("ddpm", 100).tolist()      # S defaults to T
    tv, coef = solver_tables("flowmatching", "ab2", 10)
    assert tv.tolist() == loop_t_values("flowmatching", 10).tolist() and tuple(coef.shape) == (10, 6)
    assert solver_tables("flowmatching", "ab2", 10, 10)[1].tolist() == coef.tolist()


@pytest.mark.parametrize("args", [
    ("ddpm", "ddim", 100, 101), ("ddpm", "ddim", 100, 0), ("ddpm", "dpmpp2m", 100, -3), ("ddpm", "dpmpp2m", 100, 1),
    ("flowmatching", "ab2", 10, 5), ("flowmatching", "ab2", 10, 20), ("ddpm", "ab2", 100, None), ("flowmatching", "ddim", 10, None),
    ("ddpm", "ancestral", 100, None), ("flowmatching", "euler", 10, None), ("edm", "ddim", 10, None)])
def test_refusals(args):
    with pytest.raises(ValueError):
        solver_tables(*args)


def test_eta_belongs_to_ddim():
    with pytest.raises(ValueError):
        solver_tables("ddpm", "dpmpp2m", 100, 10, eta=0.5)
    with pytest.raises(ValueError):
        solver_tables("flowmatching", "ab2", 10, eta=0.5)
    with pytest.raises(ValueError):
        solver_tables("ddpm", "ddim", 100, 10, eta=-1.0)


# ---------------------------------------------------------------------------------------------- tables against the textbook form
def _textbook_ddpm(solver, ab, tau, i, x, eps, x0_prev, z, eta):
    """One step tau_i -> tau_{i+1} (clean after the last) in the x0-prediction form, fp64.  -> (x', x0)."""
    S = len(tau)
    ab_t = ab[tau[i]]
    ab_n = ab[tau[i + 1]] if i + 1 < S else 1.0
    a, s, a_n, s_n = np.sqrt(ab_t), np.sqrt(1 - ab_t), np.sqrt(ab_n), np.sqrt(1 - ab_n)
    x0 = (x - s * eps) / a
    if solver == "ddim":
        g = eta * np.sqrt((1 - ab_n) / (1 - ab_t)) * np.sqrt(1 - ab_t / ab_n)
        return a_n * x0 + np.sqrt(1 - ab_n - g * g) * eps + g * z, x0
    lam = np.log(a / s)
    if i + 1 == S:                       # onto the clean level: h = inf, expm1(-h) = -1, first order
        return (s_n / s) * x + a_n * x0, x0
    h = np.log(a_n / s_n) - lam
    if i == 0:
        D = x0
    else:
        ab_p = ab[tau[i - 1]]
        r = (lam - np.log(np.sqrt(ab_p) / np.sqrt(1 - ab_p))) / h
        D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * x0_prev
    return (s_n / s) * x - a_n * np.expm1(-h) * D, x0


@pytest.mark.parametrize("T,S", [(1000, 20), (50, 50)])
@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp2m", 0.0)])
def test_tables_equal_the_textbook_form(solver, eta, T, S):
    tv, coef = solver_tables("ddpm", solver, T, S, eta=eta)
    coef = coef.numpy().astype(np.float64)
    tau = tv.numpy().astype(np.int64)
    assert tau.tolist() == solver_grid(T, S).tolist()
    ab = _alpha_bar(T)
    rs = np.random.RandomState(T + S)
    for i in range(S):
        x, eps, hp, z = rs.randn(4, 64)
        want_x, want_x0 = _textbook_ddpm(solver, ab, tau, i, x, eps, hp, z, eta)
        # the first step reads no history: hand it NaN
        got_x, got_h = _apply(coef[i], x, eps, np.full_like(hp, np.nan) if i == 0 else hp, z)
        tol = 1e-6 * np.abs([x, eps, hp, z]).max() * np.abs(coef[i]).max()
        assert np.abs(got_x - want_x).max() <= tol, (solver, i)
        if solver == "dpmpp2m" and i + 1 < S:
            assert np.abs(got_h - want_x0).max() <= tol, (solver, i)      # the history is the x0 prediction
        if solver == "ddim":
            assert coef[i, 2] == 0 and coef[i, 4] == 0 and coef[i, 5] == 0
            assert (coef[i, 3] == 0.0) if (eta == 0 or i + 1 == S) else (coef[i, 3] > 0)
        else:
            assert coef[i, 3] == 0.0
            assert (coef[i, 2] == 0.0) == (i == 0 or i + 1 == S)            # first and last step: first order
    assert coef[S - 1, 4] == 0 and coef[S - 1, 5] == 0                       # nothing reads a history after the last step


@pytest.mark.parametrize("T,S", [(1000, 20), (50, 50), (1000, 2)])
def test_first_and_last_dpmpp2m_rows_are_ddim(T, S):
    """The first-order steps of dpmpp2m are ddim with eta 0: the same x-update coefficients c0 .. c3 (the history
    coefficients c4, c5 differ by design -- dpmpp2m's first step stores its x0 prediction, ddim keeps no history)."""
    d = solver_tables("ddpm", "ddim", T, S)[1].numpy().astype(np.float64)
    m = solver_tables("ddpm", "dpmpp2m", T, S)[1].numpy().astype(np.float64)
    for i in (0, S - 1):
        assert np.abs(m[i, :4] - d[i, :4]).max() <= 1e-6 * np.abs(d[i, :4]).max(), i


def test_ab2_table():
    S = 8
    coef = solver_tables("flowmatching", "ab2", S)[1].numpy()
    dt = np.float32(1.0 / S)
    assert coef[0].tolist() == [1.0, dt, 0.0, 0.0, 0.0, 1.0]
    for j in range(1, S):
        assert coef[j].tolist() == [1.0, np.float32(1.5 / S), np.float32(-0.5 / S), 0.0, 0.0, 1.0 if j + 1 < S else 0.0]
    rs = np.random.RandomState(0)
    x, v, vp, z = rs.randn(4, 16)
    got, h = _apply(coef[3].astype(np.float64), x, v, vp, z)
    assert np.abs(got - (x + (1.5 * v - 0.5 * vp) / S)).max() <= 1e-6 * 1.5 and (h == v).all()


# ---------------------------------------------------------------------------------------------- order of convergence, closed form
SIG, T_CF, X_T = 0.5, 1000, np.array([1.0, -0.7, 0.3])
# max relative error at tau = 99 (ddpm) / t = 1 (flow), fp64 numpy: DDIM and Euler halve with the step (order 1), DPM-Solver++(2M)
# and AB2 quarter and better (order 2)
CLOSED_FORM = {("ddim", 10): 1.062e-1, ("ddim", 20): 5.475e-2, ("ddim", 40): 2.778e-2,
               ("dpmpp2m", 10): 2.212e-2, ("dpmpp2m", 20): 3.060e-3, ("dpmpp2m", 40): 2.552e-4,
               ("euler", 10): 1.384e-1, ("euler", 20): 7.150e-2, ("euler", 40): 3.638e-2,
               ("ab2", 10): 1.684e-2, ("ab2", 20): 3.778e-3, ("ab2", 40): 8.793e-4}


def closed_form_ddpm(solver, S, dtype=np.float64, stop=99):
    """Data ~ N(0, SIG^2): eps = s*x/(a^2 SIG^2 + s^2) exactly, and the probability-flow solution is
    x_tau = x_T * sqrt(a_tau^2 SIG^2 + s_tau^2) / sqrt(a_T^2 SIG^2 + s_T^2).  Runs the table from tau_0 = T-1 down to the
    grid point `stop`.  -> (x at `stop`, max relative error)."""
    ab = _alpha_bar(T_CF)
    tv, coef = solver_tables("ddpm", solver, T_CF, S)
    tau, coef = tv.numpy().astype(np.int64), coef.numpy().astype(dtype)
    n = tau.tolist().index(stop)
    x, h = X_T.astype(dtype), np.full(3, np.nan, dtype)
    for i in range(n):
        a2 = ab[tau[i]]
        eps = (np.sqrt(1 - a2) * x / (a2 * SIG ** 2 + 1 - a2)).astype(dtype)
        x, h = _apply(coef[i], x, eps, h, None)
    exact = X_T * np.sqrt(ab[stop] * SIG ** 2 + 1 - ab[stop]) / np.sqrt(ab[T_CF - 1] * SIG ** 2 + 1 - ab[T_CF - 1])
    return x, float(np.abs((x - exact) / exact).max())


def closed_form_flow(solver, S):
    """x_t = (1-t) x_0 + t x_1, x_1 ~ N(0, SIG^2): v = x (t SIG^2 - (1-t)) / (t^2 SIG^2 + (1-t)^2), exact end x_1 = SIG x_0."""
    coef = np.tile(np.array([1.0, 1.0 / S, 0, 0, 0, 0]), (S, 1)) if solver == "euler" else \
        solver_tables("flowmatching", "ab2", S)[1].numpy().astype(np.float64)
    tv = loop_t_values("flowmatching", S).numpy().astype(np.float64)
    x, h = X_T.copy(), np.full(3, np.nan)
    for j in range(S):
        t = tv[j]
        v = x * (t * SIG ** 2 - (1 - t)) / (t ** 2 * SIG ** 2 + (1 - t) ** 2)
        x, h = _apply(coef[j], x, v, h, None)
    return x, float(np.abs((x - SIG * X_T) / (SIG * X_T)).max())


@pytest.mark.parametrize("solver,S", sorted(CLOSED_FORM))
def test_order_of_convergence_on_the_closed_form(solver, S):
    err = (closed_form_ddpm if solver in ("ddim", "dpmpp2m") else closed_form_flow)(solver, S)[1]
    print(f"{solver} S={S}: max relative error {err:.4e} (expected {CLOSED_FORM[(solver, S)]:.3e})")
    assert abs(err - CLOSED_FORM[(solver, S)]) <= 0.01 * CLOSED_FORM[(solver, S)]


def test_fp32_arithmetic_keeps_the_closed_form_figures():
    """The same runs with every operation rounded to fp32 (what the kernel computes in) stay inside the 1 % of the table:
    fp32 rounding is far below the solvers' own error, even at dpmpp2m's 2.55e-4."""
    for solver in ("ddim", "dpmpp2m"):
        e32 = closed_form_ddpm(solver, 40, np.float32)[1]
        print(f"{solver} S=40 in fp32: {e32:.5e}")
        assert abs(e32 - CLOSED_FORM[(solver, 40)]) <= 0.01 * CLOSED_FORM[(solver, 40)]


# ---------------------------------------------------------------------------------------------- the drivers' flags
def _infer_args(*argv):
    import infer
    return infer.build_parser().parse_args(list(argv))


def test_infer_parser_defaults_give_todays_run():
    import infer
    a = _infer_args()
    assert a.solver is None and a.sample_steps is None and a.eta is None
    cells = infer.parse_cells(a)
    assert a.solver == "euler"
    assert [c.path for c in cells] == [os.path.join("./results/denoiser_results", "generation", "flowmatching_DiT_exchangerate_24_7_100")]
    a = _infer_args("--backbone", "ddpm", "--total_step", "1000", "--cfg_scale", "9", "--dataset_name", "ETTh1_96")
    cells = infer.parse_cells(a)
    assert a.solver == "ancestral"
    assert cells[0].path == os.path.join("./results/denoiser_results", "generation", "ddpm_DiT_ETTh1_96_9.0_1000")
    # naming today's mode changes nothing either
    assert infer.parse_cells(_infer_args("--solver", "euler"))[0].path.endswith("flowmatching_DiT_exchangerate_24_7_100")
    assert infer.parse_cells(_infer_args("--backbone", "ddpm", "--solver", "ancestral"))[0].path.endswith("ddpm_DiT_exchangerate_24_7_100")


def test_infer_parser_solver_flags_and_path_suffix():
    import infer
    a = _infer_args("--backbone", "ddpm", "--total_step", "1000", "--solver", "dpmpp2m", "--sample_steps", "50",
                    "--dataset_name", "ETTh1_24,ETTh1_96", "--cfg_scale", "5,9")
    assert (a.solver, a.sample_steps, a.eta) == ("dpmpp2m", 50, None)
    paths = [os.path.basename(c.path) for c in infer.parse_cells(a)]
    assert paths == ["ddpm_DiT_ETTh1_24_5.0_1000_dpmpp2m50", "ddpm_DiT_ETTh1_24_9.0_1000_dpmpp2m50",
                     "ddpm_DiT_ETTh1_96_5.0_1000_dpmpp2m50", "ddpm_DiT_ETTh1_96_9.0_1000_dpmpp2m50"]
    units = infer.grid_units(infer.parse_cells(a), 11, 3)
    assert units[1].path.endswith(os.path.join("ddpm_DiT_ETTh1_24_5.0_1000_dpmpp2m50", "run_0"))      # --run_multi keeps the layout
    a = _infer_args("--backbone", "ddpm", "--total_step", "100", "--solver", "ddim", "--eta", "0.5")
    assert a.eta == 0.5 and os.path.basename(infer.parse_cells(a)[0].path) == "ddpm_DiT_exchangerate_24_7_100_ddim100"
    a = _infer_args("--solver", "ab2", "--total_step", "10")
    assert os.path.basename(infer.parse_cells(a)[0].path) == "flowmatching_DiT_exchangerate_24_7_10_ab210"
    import evaluation
    e = evaluation.build_parser().parse_args(["--backbone", "ddpm", "--total_step", "1000", "--solver", "dpmpp2m",
                                              "--sample_steps", "50", "--cfg_scale", "9"])
    assert evaluation.model_name(e) == "ddpm_DiT_ETTh1_96_9.0_1000_dpmpp2m50"
    assert evaluation.model_name(evaluation.build_parser().parse_args([])) == "flowmatching_DiT_ETTh1_96_9.0_10"


@pytest.mark.parametrize("argv,word", [
    (("--backbone", "ddpm", "--solver", "ab2"), "ab2"),
    (("--backbone", "flowmatching", "--solver", "ddim"), "ddim"),
    (("--backbone", "flowmatching", "--solver", "ab2", "--sample_steps", "10"), "sample_steps"),
    (("--backbone", "flowmatching", "--sample_steps", "10"), "sample_steps"),
    (("--backbone", "ddpm", "--sample_steps", "10"), "sample_steps"),
    (("--backbone", "ddpm", "--eta", "0.5"), "eta"),
    (("--backbone", "ddpm", "--solver", "dpmpp2m", "--eta", "0.5"), "eta"),
    (("--backbone", "ddpm", "--solver", "ddim", "--total_step", "100", "--sample_steps", "101"), "sample_steps"),
    (("--backbone", "ddpm", "--solver", "dpmpp2m", "--sample_steps", "1"), "dpmpp2m"),
    (("--backbone", "ddpm", "--solver", "ddim", "--denoiser", "MLP"), "MLP")])
def test_infer_refuses_a_mismatched_pair_with_a_message(argv, word):
    import infer
    with pytest.raises(ValueError, match=word):
        infer.parse_cells(_infer_args(*argv))
    if "MLP" not in argv:
        with pytest.raises(SystemExit) as e:               # main() exits with that message before it looks for a GPU
            infer.main(list(argv))
        assert isinstance(e.value.code, str) and word in e.value.code
    assert resolve_solver("ddpm", "ddim", 5, 0.0, 10) == ("ddim", "_ddim5")
