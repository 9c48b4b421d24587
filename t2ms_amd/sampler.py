"""Fused CFG sampling loop (reference infer.py:73-95) on top of t2s_sampler_*.

x_T -> steps x [2B-sequence DiT forward + CFG combine + DDPM/RF update] -> LA-VAE decode,
with one sampling step captured in a hipGraph and replayed `steps` times on a private
HIP stream.  Parity mode injects x_T and the per-step Gaussian draws; perf mode draws both
from the library's Philox stream keyed by (seed, step, GLOBAL row) so the result does not
depend on how a batch is sharded over GPUs.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction
from math import ceil as _ceil
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._handle import Handle
from .model.backbone.DDPM import ddpm_host_tables

XT_STREAM = 0xFFFFFFFF  # Philox stream id reserved for x_T

# Matrix arithmetic a Sampler selects when neither its caller nor the model's owner chose one: the fp32-ACCURATE split-bf16
# products ("bf16x3", include/t2s.h T2S_MATH_BF16X3; +35 % series/s).  Round 5 settled it with a statistics-sized table against
# an fp64 run of the oracle (profiles/r05_accuracy.md: its error is not larger than that of the reference's own PyTorch-CPU
# fp32 arithmetic at any of the 17 entries); "f32" = the exact v_mfma_f32 path, which stays the bench headline and the
# class-API default.  T2S_DEFAULT_MATH overrides (the test-suite pins f32 so the headline kernels stay covered).
# "bf16" (T2S_MATH_BF16: operands rounded once to bf16, fp32 accumulate; 2.5x bf16x3, NOT fp32-accurate) is never a default:
# a caller asks for it by name.
DEFAULT_MATH = "bf16x3"


def default_math() -> str:
    m = os.environ.get("T2S_DEFAULT_MATH", "") or DEFAULT_MATH
    if m not in ("f32", "bf16x3", "bf16"):
        raise ValueError(f"T2S_DEFAULT_MATH must be 'f32', 'bf16x3' or 'bf16', got {m!r}")
    return m


def loop_t_values(backbone: str, steps: int) -> torch.Tensor:
    """The t handed to the denoiser at loop index j (host, fp32).
    ddpm: floor(steps-1-j) as int64 -> fp32 (infer.py:84); flowmatching:
    round(full(j/steps)*steps)/steps in fp32 (infer.py:78)."""
    if backbone == "ddpm":
        return torch.arange(steps - 1, -1, -1, dtype=torch.int64).to(torch.float32)
    if backbone == "flowmatching":
        vals = [torch.round(torch.full((1,), j * 1.0 / steps) * steps) / steps for j in range(steps)]
        return torch.cat(vals).to(torch.float32)
    raise ValueError("No backbone found")


SOLVERS = {"ddpm": ("ancestral", "ddim", "dpmpp2m"), "flowmatching": ("euler", "ab2")}   # [0] = today's update kernel


def default_solver(backbone: str) -> str:
    if backbone not in SOLVERS:
        raise ValueError("No backbone found")
    return SOLVERS[backbone][0]


def resolve_solver(backbone: str, solver: Optional[str] = None, sample_steps: Optional[int] = None, eta: Optional[float] = None,
                   total_step: Optional[int] = None):
    """The drivers' --solver / --sample_steps / --eta against --backbone -> (solver, directory suffix).  The default
    follows the backbone (ancestral / euler: today's run, suffix ""); a few-step solver appends "_{solver}{S}" to the
    generation directory so that runs with different solvers do not overwrite one another.  ValueError with a plain
    message for a mismatched pair: a solver of the other backbone, --sample_steps with flowmatching or without a few-step
    solver, --eta without ddim."""
    if backbone not in SOLVERS:
        raise ValueError("No backbone found")
    solver = solver or default_solver(backbone)
    if solver not in SOLVERS[backbone]:
        raise ValueError(f"--solver {solver} does not go with --backbone {backbone} (its solvers: {', '.join(SOLVERS[backbone])})")
    if eta is not None and solver != "ddim":
        raise ValueError(f"--eta is ddim's noise scale; --solver is {solver}")
    if sample_steps is not None and backbone == "flowmatching":
        raise ValueError("--sample_steps is for the ddpm solvers; the flow model's step count is --total_step")
    if sample_steps is not None and solver == default_solver(backbone):
        raise ValueError(f"--sample_steps needs --solver ddim or dpmpp2m; {solver} runs all --total_step steps")
    if solver == default_solver(backbone):
        return solver, ""
    if total_step is not None:
        solver_tables(backbone, solver, total_step, sample_steps, eta or 0.0)      # its refusals (S > T, dpmpp2m with S = 1, ...)
    S = sample_steps if sample_steps is not None else total_step
    return solver, f"_{solver}{S}"


def solver_grid(total_step: int, sample_steps: int) -> np.ndarray:
    """The "trailing" grid of S = sample_steps trained DDPM times out of T = total_step: tau_i = round(T - i*T/S) - 1
    (int64, strictly decreasing, tau_0 = T-1; S = T gives T-1 .. 0).  Integers: the denoiser only sees times it was
    trained on.  After tau_{S-1} the target level is clean (alpha_bar = 1)."""
    T, S = int(total_step), int(sample_steps)
    if not 1 <= S <= T:
        raise ValueError(f"sample_steps must lie in [1, total_step = {T}], got {S}")
    tau = np.round(T - np.arange(S, dtype=np.float64) * T / S).astype(np.int64) - 1
    assert tau[0] == T - 1 and tau[-1] >= 0 and (np.diff(tau) < 0).all()
    return tau


def solver_tables(backbone: str, solver: str, total_step: int, sample_steps: Optional[int] = None, eta: float = 0.0):
    """-> (t_values (S,) fp32, coef (S,6) fp32) of a few-step solver for the table-driven update of t2s_lms_step,
        x' = c0*x + c1*pred + c2*h + c3*z        h' = c4*x + c5*pred        (row j = loop index j)
    All algebra in fp64 from the fp32 alpha_bar of ddpm_host_tables(total_step) (the trained schedule as the reference
    computes it), rounded to fp32 once at the end.  These solvers have no counterpart in the reference.

    ddpm, on solver_grid(total_step, sample_steps); a = sqrt(ab), s = sqrt(1 - ab) at tau_i, primes at tau_{i+1} (clean
    after the last: a' = 1, s' = 0, so the last update returns the x0 prediction), x0 = (x - s*eps)/a:
      "ddim"     x' = a'*x0 + sqrt(1 - ab' - g^2)*eps + g*z,  g = eta*sqrt((1-ab')/(1-ab))*sqrt(1 - ab/ab')
                 (Song et al. 2021, eq. 12 / 16); eta = 0: c3 == 0 exactly; no history (c2 = c4 = c5 = 0)
      "dpmpp2m"  DPM-Solver++ multistep, order 2, on eps-prediction (Lu et al. 2022, alg. 2): lam = log(a/s),
                 h = lam' - lam, r = (lam - lam_prev)/h, D = (1 + 1/(2r))*x0 - 1/(2r)*x0_prev,
                 x' = (s'/s)*x - a'*expm1(-h)*D; history = x0 (c4 = 1/a, c5 = -s/a); first and last step of order 1
                 (= ddim with eta 0); S >= 2
    flowmatching, t_values of loop_t_values, dt = 1/S, S = total_step (sample_steps None or equal):
      "ab2"      step 0 Euler (c0 = 1, c1 = dt), then x' = x + dt*(1.5*v - 0.5*v_prev); history = v (c5 = 1)
    The last row writes no history (nothing reads it).  "ancestral" / "euler" are today's update kernels, not tables:
    ValueError here."""
    T = int(total_step)
    if backbone not in SOLVERS:
        raise ValueError("No backbone found")
    if solver not in SOLVERS[backbone] or solver == SOLVERS[backbone][0]:
        raise ValueError(f"solver_tables: no table for solver {solver!r} with backbone {backbone!r} "
                         f"(tables: {', '.join(SOLVERS[backbone][1:])}; {SOLVERS[backbone][0]!r} is the existing update kernel)")
    eta = float(eta)
    if backbone == "flowmatching":
        if sample_steps is not None and int(sample_steps) != T:
            raise ValueError(f"{solver}: the flow model's step count is total_step ({T}); sample_steps must be None or equal, "
                             f"got {sample_steps}")
        if eta != 0.0:
            raise ValueError("eta belongs to ddim")
        if T < 1:
            raise ValueError(f"total_step must be >= 1, got {T}")
        S, dt = T, 1.0 / T
        coef = np.zeros((S, 6), dtype=np.float64)
        coef[:, 0] = 1.0
        coef[0, 1] = dt
        coef[1:, 1], coef[1:, 2] = 1.5 * dt, -0.5 * dt
        coef[:-1, 5] = 1.0
        return loop_t_values(backbone, S).contiguous(), torch.from_numpy(coef.astype(np.float32))
    S = T if sample_steps is None else int(sample_steps)
    tau = solver_grid(T, S)
    if solver == "dpmpp2m" and S < 2:
        raise ValueError("dpmpp2m is a two-step method: sample_steps must be >= 2")
    if solver != "ddim" and eta != 0.0:
        raise ValueError("eta belongs to ddim")
    if not (np.isfinite(eta) and eta >= 0.0):
        raise ValueError(f"eta must be finite and >= 0, got {eta}")
    ab_all = ddpm_host_tables(T)["alpha_bar"].numpy().astype(np.float64)
    ab = ab_all[tau]
    ab_n = np.append(ab[1:], 1.0)                       # the next level; clean after the last grid point
    a, s, a_n, s_n = np.sqrt(ab), np.sqrt(1.0 - ab), np.sqrt(ab_n), np.sqrt(1.0 - ab_n)
    coef = np.zeros((S, 6), dtype=np.float64)
    if solver == "ddim":
        g = eta * np.sqrt((1.0 - ab_n) / (1.0 - ab)) * np.sqrt(1.0 - ab / ab_n)
        if (1.0 - ab_n - g * g < 0.0).any():
            raise ValueError(f"ddim: eta = {eta} gives a variance above 1 - alpha_bar' on this grid")
        coef[:, 0] = a_n / a
        coef[:, 1] = np.sqrt(1.0 - ab_n - g * g) - a_n * s / a
        coef[:, 3] = g
    else:
        lam = np.log(a / s)
        with np.errstate(divide="ignore"):
            lam_n = np.append(lam[1:], np.inf)          # clean: h = inf, expm1(-h) = -1
        h = lam_n - lam
        E = -a_n * np.expm1(-h)                         # x' = (s'/s)*x + E*D
        w = np.zeros(S)                                 # 1/(2r); 0 = first order (first and last step)
        w[1:-1] = 0.5 * h[1:-1] / (lam[1:-1] - lam[:-2])
        coef[:, 0] = s_n / s + E * (1.0 + w) / a
        coef[:, 1] = -E * (1.0 + w) * s / a
        coef[:, 2] = -E * w
        coef[:-1, 4] = 1.0 / a[:-1]
        coef[:-1, 5] = -s[:-1] / a[:-1]
    c32 = (coef + 0.0).astype(np.float32)               # (+ 0.0: a -0.0 coefficient becomes the 0.0 it stands for)
    if not np.isfinite(c32).all():
        raise ValueError(f"{solver}: a coefficient is not finite in fp32 on this grid")
    return torch.from_numpy(tau.astype(np.float32)), torch.from_numpy(c32)


def _fraction(v, what: str) -> Fraction:
    """The exact value a float, an int, a Fraction or a decimal string WRITES: Fraction(str(v)) for floats and strings, so
    0.7 is 7/10 and not the binary 0.6999999999999999556."""
    try:
        if isinstance(v, bool):
            raise ValueError
        f = v if isinstance(v, Fraction) else Fraction(v) if isinstance(v, int) else Fraction(str(v).strip())
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"cfg interval: {what} = {v!r} is not a number") from None
    return f


def guided_steps(interval, steps: int):
    """The guided window (j0, j1) in loop indices of interval = (lo, hi), fractions of a loop of `steps` iterations with
    0 <= lo <= hi <= 1: step j (j = 0 the noisiest) runs classifier-free guidance iff lo*steps <= j < hi*steps, i.e.
    j0 = ceil(lo*steps), j1 = ceil(hi*steps); every other step runs the conditional pass alone (t2s_sampler_set_guided_steps).
    Evaluated exactly in rationals from the decimal text of lo / hi (floats and command-line strings alike), never by float
    multiplication: (0.07, 0.5) of 100 steps is (7, 50), where ceil(0.07 * 100 = 7.000000000000001) would give 8.
    ValueError outside that range, for lo > hi or steps < 1."""
    try:
        lo, hi = interval
    except (TypeError, ValueError):
        raise ValueError(f"cfg interval must be a pair (lo, hi), got {interval!r}") from None
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"cfg interval: steps must be >= 1, got {steps}")
    lo, hi = _fraction(lo, "lo"), _fraction(hi, "hi")
    if not 0 <= lo <= hi <= 1:
        raise ValueError(f"cfg interval must satisfy 0 <= lo <= hi <= 1, got lo = {interval[0]}, hi = {interval[1]}")
    return _ceil(lo * steps), _ceil(hi * steps)


def parse_cfg_interval(text: str):
    """--cfg_interval LO,HI -> (lo, hi) as exact Fractions; ValueError for anything else."""
    parts = str(text).split(",")
    if len(parts) != 2:
        raise ValueError(f"--cfg_interval takes LO,HI (two fractions of the loop, e.g. 0.2,0.8), got {text!r}")
    return _fraction(parts[0], "lo"), _fraction(parts[1], "hi")


def resolve_cfg_interval(text, steps: int):
    """The drivers' --cfg_interval LO,HI against a loop of `steps` iterations -> (guided window or None, directory suffix).
    Without the flag: (None, ""), every path as before.  With it: the window of guided_steps, and the suffix "_gi{j0}-{j1}"
    unless the window is the whole loop (the run is then today's run and keeps today's directory)."""
    if text is None:
        return None, ""
    j0, j1 = guided_steps(parse_cfg_interval(text), steps)
    return (j0, j1), ("" if (j0, j1) == (0, int(steps)) else f"_gi{j0}-{j1}")


_STREAMS = {}


def _sampler_stream(device) -> "torch.cuda.Stream":
    """ONE capture stream per device for every Sampler of the process.  HIP maps streams onto a few hardware queues in
    creation order and two streams on one queue run one after the other: with a stream per Sampler, lane 0 (this stream)
    landed on the queue of lane 1 (the library's pooled stream, csrc/t2s_sampler.hip lane_streams) for every fourth Sampler
    a process built -- 52 instead of 61 series/s at 64 series, reproducibly by construction order (tools/strong_probe.py)."""
    key = str(torch.device(device))
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(torch.device(device))
    return _STREAMS[key]


def philox_normal(n_rows: int, row_elems: int, seed: int, stream_id: int, row0: int, device) -> torch.Tensor:
    """(n_rows, row_elems) N(0,1) draws of the library's Philox stream: element e of GLOBAL row row0 + r uses counter
    (e/4, row0 + r, stream_id), key = seed -- the same values however the rows are sharded over GPUs."""
    device = torch.device(device)
    out = torch.empty(n_rows, row_elems, device=device, dtype=torch.float32)
    if n_rows:
        with torch.cuda.device(device):
            L.check(L.lib().t2s_philox_normal(L.dev_ptr(out), int(seed), int(stream_id) & 0xFFFFFFFF, int(row0), n_rows,
                                              row_elems, L.stream_ptr(device)), "t2s_philox_normal")
    return out


def _u64_table(seeds, n: int, what: str) -> np.ndarray:
    a = np.asarray(seeds)
    if a.shape != (n,) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == object):
        raise L.T2SError(f"{what}: seeds must be {n} integers, got shape {a.shape} dtype {a.dtype}")
    vals = [int(v) for v in a.tolist()]
    if any(v < 0 or v >= 1 << 64 for v in vals):
        raise L.T2SError(f"{what}: seeds must lie in [0, 2**64)")
    return np.asarray(vals, dtype=np.uint64)


def _u32_table(key_rows, n: int, what: str) -> np.ndarray:
    a = np.asarray(key_rows)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise L.T2SError(f"{what}: key_rows must be {n} integers, got shape {a.shape} dtype {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 32):
        raise L.T2SError(f"{what}: key_rows must lie in [0, 2**32)")
    return a.astype(np.uint32)


def _cfg_table(cfg, n: int, what: str) -> np.ndarray:
    a = np.asarray(cfg, dtype=np.float64)
    if a.shape != (n,):
        raise L.T2SError(f"{what}: cfg must hold {n} values, got shape {a.shape}")
    with np.errstate(over="ignore"):
        f = a.astype(np.float32)
    if not np.isfinite(f).all():
        raise L.T2SError(f"{what}: cfg values must be finite (in fp32)")
    return f


def _device_tables(seeds: np.ndarray, key_rows: np.ndarray, device):
    """(u64 seeds, u32 key rows) as device tensors of the same bits (int64 / int32 storage).  Staged through pinned memory
    and copied asynchronously on the current stream: a pageable copy would make the host wait for the work queued before
    it (the previous launch), which the uniform x_T draw never did."""
    s = torch.from_numpy(np.ascontiguousarray(seeds.astype(np.uint64)).view(np.int64)).pin_memory()
    k = torch.from_numpy(np.ascontiguousarray(key_rows.astype(np.uint32)).view(np.int32)).pin_memory()
    return s.to(device, non_blocking=True), k.to(device, non_blocking=True)


def philox_normal_rows(seeds, key_rows, row_elems: int, stream_id: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_rows, row_elems) N(0,1) draws with a key and a key row per row (t2s_philox_normal_rows): row r equals
    philox_normal(1, row_elems, seeds[r], stream_id, key_rows[r], device) bit for bit."""
    device = torch.device(device)
    n = len(seeds)
    s = _u64_table(seeds, n, "philox_normal_rows")
    k = _u32_table(key_rows, n, "philox_normal_rows")
    if out is None:
        out = torch.empty(n, row_elems, device=device, dtype=torch.float32)
    if out.numel() != n * row_elems:
        raise L.T2SError(f"philox_normal_rows: out holds {out.numel()} values, expected {n} x {row_elems}")
    if n:
        ds, dk = _device_tables(s, k, device)
        with torch.cuda.device(device):
            L.check(L.lib().t2s_philox_normal_rows(L.dev_ptr(out), ds.data_ptr(), dk.data_ptr(), int(stream_id) & 0xFFFFFFFF,
                                                   n, row_elems, L.stream_ptr(device)), "t2s_philox_normal_rows")
    return out


def philox_uniform(n_rows: int, row_elems: int, seed: int, stream_id: int, row0: int, device) -> torch.Tensor:
    """(n_rows, row_elems) U[0,1) draws of the library's Philox stream (t2s_philox_uniform): 24-bit uniforms keyed like
    philox_normal by (seed, stream_id, GLOBAL row) -- the per-row diffusion time of a training step (train.py:109,113)."""
    device = torch.device(device)
    out = torch.empty(n_rows, row_elems, device=device, dtype=torch.float32)
    if n_rows:
        with torch.cuda.device(device):
            L.check(L.lib().t2s_philox_uniform(L.dev_ptr(out), int(seed), int(stream_id) & 0xFFFFFFFF, int(row0), n_rows,
                                               row_elems, L.stream_ptr(device)), "t2s_philox_uniform")
    return out


def lms_step(x: torch.Tensor, hist: torch.Tensor, pred_u: torch.Tensor, pred_c: Optional[torch.Tensor], coef: torch.Tensor,
             index: int, cfg: float = 0.0, noise: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0,
             row0: int = 0) -> None:
    """One update of t2s_lms_step, IN PLACE on x and hist ((B,64,W) or (B,64 W) fp32 on the GPU; W = 30, or the width of a
    wide model -- t2s_lms_step_n):
    x' = c0*x + c1*pred + c2*h + c3*z, h' = c4*x + c5*pred with {c0..c5} = coef[index] (DEVICE (S,6)), pred = u + cfg*(c-u)
    (pred = u when pred_c is None), z = `noise` or, when None, the Philox draw (seed, stream_id, row0 + row).  For stepwise
    loops; the Sampler runs the same kernel from its loop."""
    B = x.shape[0]
    row = x.numel() // max(B, 1)
    if row % L.LAT_C or row // L.LAT_C not in (30, 50, 64):
        raise L.T2SError(f"lms_step: x must hold ({B},64,W) values with W 30, 50 or 64, got {tuple(x.shape)}")
    for name, v in (("x", x), ("hist", hist), ("pred_u", pred_u), ("pred_c", pred_c), ("noise", noise)):
        if v is not None and (v.shape[0] != B or v.numel() != B * row):
            raise L.T2SError(f"lms_step: {name} must hold ({B},{row}) values, got {tuple(v.shape)}")
    if coef.dim() != 2 or coef.shape[1] != 6 or not 0 <= int(index) < coef.shape[0]:
        raise L.T2SError(f"lms_step: coef must be (S,6) with 0 <= index < S, got {tuple(coef.shape)}, index {index}")
    with torch.cuda.device(x.device):
        L.check(L.lib().t2s_lms_step_n(L.dev_ptr(x, "x"), L.dev_ptr(hist, "hist"), L.dev_ptr(pred_u, "pred_u"),
                                       L.dev_ptr(pred_c, "pred_c"), L.dev_ptr(noise, "noise"), L.dev_ptr(coef, "coef"), int(index),
                                       float(cfg), int(seed), int(stream_id) & 0xFFFFFFFF, int(row0), B, row,
                                       L.stream_ptr(x.device)), "t2s_lms_step_n")


class Sampler:
    def __init__(self, model, decoder, backbone: str, steps: int, cfg_scale: float, batch: int, length: int,
                 device, use_graph: bool = True, seed: int = 2025, row0: int = 0, lanes: int = 0, loop_graph: int = -1,
                 math: Optional[str] = None, solver: Optional[str] = None, sample_steps: Optional[int] = None, eta: float = 0.0,
                 guide_steps=None, cfg_interval=None):
        """lanes: 0 = automatic (equal part-batch chains on own streams: two when the batch is a multiple of 64 or 32 series, three for 96), 1 .. 4 -- see
        t2s_sampler_set_lanes; a scheduling choice only, the results are bitwise the same.
        math: "f32" | "bf16x3" | "bf16" (single-pass bf16 mixed precision: opt-in, not fp32-accurate) selects the model's matrix arithmetic (Transformer.set_math) for this sampler and everything else
        that runs the model afterwards; None = what the model's owner chose with set_math, else default_math() (bf16x3).
        solver: None / "ancestral" (ddpm) / "euler" (flowmatching) = the reference's update, exactly what was created before
        the solvers existed; "ddim" / "dpmpp2m" (ddpm) and "ab2" (flowmatching) = the few-step solvers of solver_tables
        (t2s_sampler_create_lms).  `steps` stays the TRAINED schedule length (--total_step); with a ddpm solver the loop runs
        sample_steps (default: steps) denoiser evaluations and self.steps becomes that S -- the first dimension of `noise`.
        eta: ddim's stochasticity (0 = deterministic).
        guide_steps = (j0, j1) / cfg_interval = (lo, hi): the guided window (at most one of the two; None = every step) in
        loop indices of self.steps / as fractions of the loop (guided_steps) -- classifier-free guidance on steps j0 <= j < j1,
        the conditional pass alone on the others, which run half the sequences (set_guided_steps).  Not in the reference."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.T2SError("Sampler needs a GPU device; the HIP path has no CPU fallback")
        self.model, self.decoder = model, decoder
        # a multichannel decoder (model/pretrained/myvqvae.py Decoder: C-channel motion series) decodes to (B,C,L), any L >= 8
        self.channels = getattr(decoder, "channels", None)      # (None too without a decoder: the single-channel (B,L) layout)
        # the model's latent width (mytransformer.Transformer(dim): 50 / 64 for the motion models); the wide widths run f32
        # unless somebody chose otherwise on a model opted in with set_wide_math(True) -- set_math below refuses it without
        self.width = int(getattr(model, "H", L.LAT_W))
        flow_dim = getattr(decoder, "flow_dim", None)      # (stamped by myvqvae.vqvae; a bare Decoder does not know it)
        if flow_dim is not None and int(flow_dim) != self.width:
            raise L.T2SError(f"Sampler: the decoder's flow_dim {int(flow_dim)} differs from the model's latent width {self.width}")
        if decoder is not None and self.width != L.LAT_W and self.channels is None:
            raise L.T2SError(f"Sampler: a model of latent width {self.width} needs the multichannel decoder (myvqvae)")
        self.math = math or model.__dict__.get("_t2s_math") or ("f32" if self.width != L.LAT_W else default_math())
        if hasattr(model, "set_math"):
            model.set_math(self.math)
        self.backbone, self.steps, self.cfg_scale = backbone, int(steps), float(cfg_scale)
        self.total_step, self.solver, self.eta = int(steps), solver, float(eta)
        self._lms = None
        if solver is not None and solver != default_solver(backbone):
            self._lms = solver_tables(backbone, solver, self.total_step, sample_steps, self.eta)    # raises on a mismatched pair
            self.steps = int(self._lms[0].numel())
        elif sample_steps is not None or self.eta != 0.0:
            raise ValueError(f"sample_steps / eta need a few-step solver ({', '.join(SOLVERS.get(backbone, ('?',))[1:])}); "
                             f"{default_solver(backbone)!r} runs the trained schedule")
        if guide_steps is not None and cfg_interval is not None:
            raise ValueError("give guide_steps (loop indices) or cfg_interval (fractions of the loop), not both")
        if cfg_interval is not None:
            guide_steps = guided_steps(cfg_interval, self.steps)
        self._guided = (0, self.steps) if guide_steps is None else self._check_window(*guide_steps)
        self.batch, self.length, self.seed, self.row0 = int(batch), int(length), int(seed), int(row0)
        self.use_graph = bool(use_graph)
        self.lanes = int(lanes)
        self.loop_graph = int(loop_graph)     # 1: the whole loop as one hipGraph per lane, 0: one step replayed, -1: library default
        self.stream = _sampler_stream(self.device)
        self.ptr = None
        self._create()

    def _create(self):
        """(Re)build the C sampler against the model's CURRENT t2s_dit handle.  The package's per-device lock
        (_lib.device_lock) is held for EVERYTHING a Sampler does on the GPU -- building its handle and C sampler (allocations,
        copies, a device synchronize), staging inputs, the run itself.  Foreign GPU work of other threads is not covered."""
        with L.device_lock(self.device):
            self._create_locked()

    def _create_locked(self):
        if self.ptr is not None:
            self._h.close()
            self.ptr = None          # (a create that raises below leaves no freed pointer behind)
        model, decoder, backbone, use_graph = self.model, self.decoder, self.backbone, self.use_graph
        lms = self.__dict__.get("_lms")
        tvals = loop_t_values(backbone, self.steps).contiguous() if lms is None else lms[0].contiguous()
        cfg = L.SampleConfig()
        cfg.mode = L.MODE_LMS if lms is not None else (L.MODE_DDPM if backbone == "ddpm" else L.MODE_RF)
        cfg.steps, cfg.cfg_scale, cfg.batch, cfg.length = self.steps, self.cfg_scale, self.batch, self.length
        cfg.use_graph, cfg.seed, cfg.row0 = int(bool(use_graph)), self.seed, self.row0
        coef = None
        if lms is not None:
            coef = lms[1].contiguous()                   # host (S,6), copied by the library
        elif backbone == "ddpm":
            coef = ddpm_host_tables(self.steps)["coef"].contiguous()
            cfg.ddpm_coef = coef.data_ptr()          # host pointers, copied by the library
        cfg.t_values = tvals.data_ptr()
        with torch.cuda.device(self.device):
            dit = model.t2s_handle(self.device, 2 * self.batch)
            self._dit_uid = model.t2s_handle_id()
            vae = decoder._handle(self.device) if decoder is not None else None
            create = ("t2s_sampler_create",) if lms is None else ("t2s_sampler_create_lms", coef.data_ptr())
            self._h = Handle(self.device, create[0], "t2s_sampler_destroy", dit, vae, C.byref(cfg), *create[1:])
            self.ptr = self._h.ptr
            L.check(L.lib().t2s_sampler_set_lanes(self.ptr, self.lanes), "t2s_sampler_set_lanes")
            L.check(L.lib().t2s_sampler_set_loop_graph(self.ptr, self.loop_graph), "t2s_sampler_set_loop_graph")
        if self.__dict__.get("_rows") is not None:      # a re-created C sampler keeps the per-row tables
            self.set_rows(*self._rows)
        if self.__dict__.get("_lengths") is not None:   # ... and the per-row lengths
            self._set_lengths_locked(self._lengths, force=True)
        if self._guided != (0, self.steps):             # ... and the guided window (a new C sampler guides every step)
            L.check(L.lib().t2s_sampler_set_guided_steps(self.ptr, *self._guided), "t2s_sampler_set_guided_steps")
        self._keep = (tvals, coef)

    def _check_window(self, j0, j1):
        j0, j1 = int(j0), int(j1)
        if not 0 <= j0 <= j1 <= self.steps:
            raise ValueError(f"guided steps must satisfy 0 <= j0 <= j1 <= steps = {self.steps}, got ({j0}, {j1})")
        return j0, j1

    def set_guided_steps(self, j0: int, j1: int):
        """Classifier-free guidance on loop indices j0 <= j < j1 for the NEXT runs, the conditional pass alone on the others
        (t2s_sampler_set_guided_steps; (0, steps) = every step).  A window that differs from the current one drops the
        captured hipGraphs; the library refuses, and changes nothing, unless 0 <= j0 <= j1 <= steps."""
        with L.device_lock(self.device):
            if (int(j0), int(j1)) != self._guided:
                self.stream.synchronize()       # a graph the last run launched is not destroyed under it
            L.check(L.lib().t2s_sampler_set_guided_steps(self.ptr, int(j0), int(j1)), "t2s_sampler_set_guided_steps")
            self._guided = (int(j0), int(j1))

    @property
    def guided(self):
        """The guided window (j0, j1) in loop indices, as the C sampler holds it."""
        j0, j1 = C.c_int(), C.c_int()
        L.check(L.lib().t2s_sampler_guided_steps(self.ptr, C.byref(j0), C.byref(j1)), "t2s_sampler_guided_steps")
        return j0.value, j1.value

    def set_row0(self, row0: int):
        """Global index of this shard's first series for the NEXT run (the Philox key of row r is row0 + r);
        the captured hipGraph is kept (t2s_sampler_set_row0)."""
        self.row0 = int(row0)
        L.check(L.lib().t2s_sampler_set_row0(self.ptr, self.row0), "t2s_sampler_set_row0")

    def set_rows(self, seeds=None, key_rows=None, cfg=None):
        """Per-row noise key, key row and guidance scale for the NEXT runs (t2s_sampler_set_rows): row r draws x_T and its
        per-step noise as row key_rows[r] of the Philox stream keyed by seeds[r] and combines u + cfg[r] * (c - u) -- what
        a uniform sampler of that seed / row0 / cfg_scale does for it, so rows of several runs and guidance scales share one
        launch.  Each argument: `batch` values, or None = uniform (the sampler's seed, row0 + r, cfg_scale).  All None
        restores the uniform sampler.  The captured hipGraph is kept."""
        n = self.batch
        s = None if seeds is None else _u64_table(seeds, n, "Sampler.set_rows")
        k = None if key_rows is None else _u32_table(key_rows, n, "Sampler.set_rows")
        c = None if cfg is None else _cfg_table(cfg, n, "Sampler.set_rows")
        L.check(L.lib().t2s_sampler_set_rows(self.ptr, None if s is None else s.ctypes.data,
                                             None if k is None else k.ctypes.data,
                                             None if c is None else c.ctypes.data, n), "t2s_sampler_set_rows")
        self._rows = (s, k, c)

    def check_lengths(self, lengths):
        """Host-side validation of a run's per-row lengths, before anything reaches the library: `batch` integers, each 0 or
        in [8, length], for a sampler with a multichannel decoder -> (int32 lengths, uint64 offsets).  T2SError otherwise."""
        if self.channels is None:
            raise L.T2SError("Sampler: per-row lengths need the multichannel decoder (model/pretrained/myvqvae.py); "
                             "the single-channel codec has no ragged decode")
        lens, off, _ = L.ragged_layout(lengths, self.length, "Sampler: lengths", batch=self.batch)
        return lens, off

    def _set_lengths_locked(self, lengths, force=False):
        """lengths: what check_lengths returned, or None = the uniform (B,C,L) sampler again (t2s_sampler_set_lengths)."""
        cur = self.__dict__.get("_lengths")
        same = (cur is None) == (lengths is None) and (cur is None or np.array_equal(cur[0], lengths[0]))
        if same and not force:
            return
        L.check(L.lib().t2s_sampler_set_lengths(self.ptr, None if lengths is None else lengths[0].ctypes.data,
                                                0 if lengths is None else len(lengths[0])), "t2s_sampler_set_lengths")
        self._lengths = lengths

    def _ragged_rows(self, packed):
        """The rows of a packed series buffer as (C, L_b) views."""
        lens, off = self._lengths
        ch = self.channels
        return [packed[ch * int(off[b]):ch * int(off[b + 1])].view(ch, int(lens[b])) for b in range(self.batch)]

    def draw_xT(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_T ~ N(0,1) from the Philox stream (perf mode), (batch,64,W); per row as set_rows keyed it."""
        row = L.LAT_C * self.width
        if out is None:
            out = torch.empty(self.batch, L.LAT_C, self.width, device=self.device, dtype=torch.float32)
        s, k, _ = self.__dict__.get("_rows") or (None, None, None)
        if s is not None or k is not None:
            if s is None:
                s = np.full(self.batch, self.seed, dtype=np.uint64)
            if k is None:
                k = (self.row0 + np.arange(self.batch, dtype=np.int64)).astype(np.uint32)
            return philox_normal_rows(s, k, row, XT_STREAM, self.device, out=out)
        with torch.cuda.device(self.device):
            L.check(L.lib().t2s_philox_normal(L.dev_ptr(out), self.seed, XT_STREAM, self.row0, self.batch, row,
                                              L.stream_ptr(self.device)), "t2s_philox_normal")
        return out

    def run(self, text: torch.Tensor, x_T: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
            decode: bool = True, trace: bool = False, lengths=None):
        """Returns (latent (B,64,W), series (B,L) or None, trace (steps,L) or None); with a multichannel decoder the series
        is (B,C,L) and the trace (steps,C,L).  W is the model's latent width (30; 50 / 64 for mytransformer.Transformer).
        ``noise`` (steps,B,64,W) injects the per-step draws (parity mode).
        ``lengths`` (multichannel decoder only): B integers, each 0 or in [8, length] -- row b is decoded at lengths[b], the
        series is a LIST of (C, L_b) tensors (views of one packed buffer) and the trace (steps,C,lengths[0]).  The latent
        does not depend on them.  They hold for this run and for run_inplace until a run() without them."""
        ragged = None if lengths is None else self.check_lengths(lengths)       # host-side, before anything is uploaded
        if ragged is not None and trace and int(ragged[0][0]) == 0:
            raise L.T2SError("Sampler.run: trace requested but lengths[0] is 0")
        with L.device_lock(self.device):
            dev = self.device
            text = L.as_f32(text.to(dev))
            if tuple(text.shape) != (self.batch, L.D_MODEL):
                raise L.T2SError(f"Sampler.run: text must be ({self.batch},128), got {tuple(text.shape)}")
            # persistent device buffers: the captured hipGraph is bound to their addresses
            if self.__dict__.get("_x") is None:
                self._x = torch.empty(self.batch, L.LAT_C, self.width, device=dev, dtype=torch.float32)
                self._text = torch.empty(self.batch, L.D_MODEL, device=dev, dtype=torch.float32)
                self._series = torch.empty(self.batch, *self._row_shape(), device=dev, dtype=torch.float32)
            self._text.copy_(text)
            if x_T is None:
                self.draw_xT(self._x)
            else:
                if tuple(x_T.shape) != (self.batch, L.LAT_C, self.width):
                    raise L.T2SError(f"Sampler.run: x_T must be ({self.batch},64,{self.width}), got {tuple(x_T.shape)}")
                self._x.copy_(x_T)
            if noise is not None:
                noise = L.as_f32(noise.to(dev))
                if tuple(noise.shape) != (self.steps, self.batch, L.LAT_C, self.width):
                    raise L.T2SError(f"Sampler.run: noise must be ({self.steps},{self.batch},64,{self.width})")
            if (decode or trace) and self.decoder is None:
                raise L.T2SError("Sampler.run: decode requested but no decoder was given")
            tr_shape = self._row_shape() if ragged is None else (self.channels, int(ragged[0][0]))
            tr = torch.empty(self.steps, *tr_shape, device=dev, dtype=torch.float32) if trace else None
            with torch.cuda.device(dev):
                # weights may have changed since the last run: refresh the packed copy on the caller's stream
                self.model.t2s_handle(dev, 2 * self.batch)
                if self.model.t2s_handle_id() != self._dit_uid:
                    self._create()  # the model re-created its handle (capacity grew / device moved): drop the graph
                self._set_lengths_locked(ragged)
                cur = torch.cuda.current_stream(dev)
                self.stream.wait_stream(cur)
                L.check(L.lib().t2s_sampler_run(self.ptr, L.dev_ptr(self._x), L.dev_ptr(self._text), L.dev_ptr(noise),
                                                L.dev_ptr(self._series) if decode else None, L.dev_ptr(tr),
                                                self.stream.cuda_stream), "t2s_sampler_run")
                cur.wait_stream(self.stream)
            self._last = (noise, tr)  # keep caller-provided buffers alive until the stream has consumed them
            if ragged is not None and decode:      # the packed rows fill the front of the (B,C,length) buffer
                packed = self._series.view(-1)[:self.channels * int(ragged[1][-1])].clone()
                return self._x.clone(), self._ragged_rows(packed), tr
            return self._x.clone(), (self._series.clone() if decode else None), tr

    def _row_shape(self):
        """One decoded series: (L,), or (C,L) with a multichannel decoder."""
        return (self.length,) if self.channels is None else (self.channels, self.length)

    @property
    def graph_lanes(self) -> int:
        """Lanes of the hipGraphs the sampler currently holds (0: nothing captured / the last run was eager)."""
        return int(L.lib().t2s_sampler_graph_lanes(self.ptr))

    def run_inplace(self, decode: bool = True):
        """Benchmark entry: x_T from Philox into the persistent buffers, no output copies.
        Requires one prior run() (buffers + text in place).  Returns (latent, series) views; after a run() with lengths
        the series is the list of (C, L_b) views of the packed buffer."""
        dev = self.device
        with L.device_lock(dev), torch.cuda.device(dev):
            if self.model.t2s_handle_id() != self._dit_uid:
                self._create()
            self.draw_xT(self._x)
            cur = torch.cuda.current_stream(dev)
            self.stream.wait_stream(cur)
            L.check(L.lib().t2s_sampler_run(self.ptr, L.dev_ptr(self._x), L.dev_ptr(self._text), None,
                                            L.dev_ptr(self._series) if decode else None, None,
                                            self.stream.cuda_stream), "t2s_sampler_run")
            cur.wait_stream(self.stream)
        if self.__dict__.get("_lengths") is not None:
            return self._x, self._ragged_rows(self._series.view(-1))
        return self._x, self._series


def host_shard(total: int, rank: int, world: int):
    """Rows [lo,hi) of a batch of `total` series owned by `rank` (contiguous, remainder to low ranks)."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def np_save_outputs(path: str, x_1: np.ndarray, x_t: np.ndarray, lat_dec: np.ndarray, lat_enc: np.ndarray):
    """The four arrays evaluation.py reads (infer.py:118-123)."""
    import os
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "x_1.npy"), x_1[:, :, np.newaxis])
    np.save(os.path.join(path, "x_t.npy"), x_t[:, :, np.newaxis])
    np.save(os.path.join(path, "x_t_latent_dec_array.npy"), lat_dec)
    np.save(os.path.join(path, "x_t_latent_enc_array.npy"), lat_enc)
