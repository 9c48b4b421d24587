"""References of the training step's row kernels called alone (include/t2s_train_rows.h), shared by tests/test_train_rows.py
(GPU) and tests/test_train_rows_host.py (CPU).  Per launch form and case:

  * the fp64 reference, written from the DEFINITIONS: LayerNorm (eps 1e-6, no affine) + adaLN modulate, the final LayerNorm
    (eps 1e-5, affine), tanh-GELU, x + gate * branch; every backward form is torch autograd of its forward in fp64, so the
    reference shares no formula with the kernels;
  * a CPU RESTATEMENT in the kernel's precision (the _restate_f32 / _bars_bf16 pattern of tests/test_train_kernels.py): fp32
    arithmetic, the backward formulas of the comment above ln_mod_bwd_kernel (t2s_train.hip), and in T2S_TRAIN_BF16 a bf16
    round-to-nearest-even exactly where the kernel has one -- the prologue's output in front of the MFMA (which is also the
    saved activation), every bf16 store, q after the multiplication by ATT_QS;
  * the per-tile measure and the bars: 2 x (bf16-rounded outputs) or 4 x (fp32 outputs) the restatement's own deviation from
    the same fp64 reference -- never anything the kernel gave.

bf16 operands are rounded to bf16 BEFORE both, so the reference is "fp64 of the rounded operands"."""
import numpy as np
import torch

F32, BF16 = 0, 1                                    # T2S_TRAIN_F32 / T2S_TRAIN_BF16
D, MODROW, NH, DH = 128, 3072, 4, 32
QS = float(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))   # t2s_bf16.h ATT_QS, as tests/test_train_kernels.py
TOKENS = (480, 800, 1024)
SHIFT_OFF, SCALE_OFF, GATE_OFF = 2 * 768 + 3 * D, 2 * 768 + 4 * D, 1 * 768 + 5 * D   # three distinct slices of a MODROW row
SENTINEL = 7.0e3                                    # the unused columns of mod / dmod: +-7e3, alternating
CAP = {"b": 1e-2, "f": 2e-4, "s": 2e-4, "t": 2e-4}  # the whole-step bars the suite already has (bf16 1e-2, fp32 2e-4)
MULT = {"b": 2.0, "f": 4.0, "s": 4.0, "t": 4.0}     # tests/test_train_kernels.py: _bars_bf16 / _bars_f32

# case name -> (T2S_ROWS_* name, dtype, with the next branch's gate backward)
FORMS = {
    "QKV0": ("QKV0", BF16, False), "QKV1": ("QKV1", BF16, False), "FC1": ("FC1", BF16, False), "FC2": ("FC2", BF16, False),
    "LIN128": ("LIN128", BF16, False), "GELUBWD": ("GELUBWD", BF16, False),
    "LNBWD256": ("LNBWD256", BF16, True), "LNBWD256_NOGATE": ("LNBWD256", BF16, False),
    "LNBWD384": ("LNBWD384", BF16, True), "LNBWD384_NOGATE": ("LNBWD384", BF16, False),
    "FINAL_FUSED": ("FINAL_FUSED", BF16, False),
    "F_QKV": ("F_QKV", F32, False), "F_FC1": ("F_FC1", F32, False), "F_FC2": ("F_FC2", F32, False),
    "F_LIN128": ("F_LIN128", F32, False), "F_LIN256": ("F_LIN256", F32, False), "F_LIN384": ("F_LIN384", F32, False),
    "F_GELUBWD": ("F_GELUBWD", F32, False), "F_GATE_RES": ("F_GATE_RES", F32, False), "F_GATE_BWD": ("F_GATE_BWD", F32, False),
    "F_LN_MOD_BWD": ("F_LN_MOD_BWD", F32, False), "F_GELU": ("F_GELU", F32, False), "F_FINAL": ("F_FINAL", F32, False),
}
BF16_FORMS = tuple(n for n, f in FORMS.items() if f[1] == BF16)
LINEAR_KN = {"QKV0": (128, 384), "QKV1": (128, 384), "F_QKV": (128, 384), "FC1": (128, 256), "F_FC1": (128, 256),
             "FC2": (256, 128), "F_FC2": (256, 128), "LIN128": (128, 128), "F_LIN128": (128, 128), "F_LIN256": (256, 128),
             "F_LIN384": (384, 128), "GELUBWD": (128, 256), "F_GELUBWD": (128, 256), "LNBWD256": (256, 128), "LNBWD384": (384, 128)}


def rb(t):
    """Round to nearest even bf16, back in the tensor's own type."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def heads(y, n_seq, n_tok):       # rows (M, 128) -> heads (n_seq * 4, n_tok, 32)
    return y.reshape(n_seq, n_tok, NH, DH).permute(0, 2, 1, 3).reshape(n_seq * NH, n_tok, DH).contiguous()


def seq_rows(mod, off, n_tok):    # (n_seq, MODROW) slice -> one row per token (M, 128)
    return mod[:, off:off + D].repeat_interleave(n_tok, dim=0)


def seq_sum(t, n_seq):            # (M, 128) -> (n_seq, 128)
    return t.reshape(n_seq, -1, D).sum(1)


def patch_index(n_tok):
    """(n_tok, 4) index into a (64 * latw) latent: token n = hh * 32 + ww owns lat[2 ww + (p & 1)][2 hh + (p >> 1)]."""
    latw = n_tok // 16
    tok = torch.arange(n_tok).unsqueeze(1)
    p = torch.arange(4).unsqueeze(0)
    return (2 * (tok & 31) + (p & 1)) * latw + 2 * (tok >> 5) + (p >> 1)


# ------------------------------------------------------------------------------------------------ inputs
def mod_table(g, n_seq):
    """Every sequence its OWN shift / scale / gate row, drawn separately, at three distinct offsets of a full-width table whose
    other columns hold the sentinel pattern."""
    cols = torch.arange(MODROW)
    mod = (SENTINEL * (1.0 - 2.0 * (cols & 1).float())).repeat(n_seq, 1)
    for s in range(n_seq):
        mod[s, SHIFT_OFF:SHIFT_OFF + D] = torch.randn(D, generator=g)
        mod[s, SCALE_OFF:SCALE_OFF + D] = 0.5 * torch.randn(D, generator=g)
        mod[s, GATE_OFF:GATE_OFF + D] = torch.randn(D, generator=g)
    return mod.contiguous()


_BASE = {}


def base(n_tok, n_seq):
    """The fp32 operands every form of one (n_tok, n_seq) draws from; drawn once, left unchanged."""
    key = (n_tok, n_seq)
    if key not in _BASE:
        g = torch.Generator().manual_seed(7100 + n_tok * 10 + n_seq)
        M = n_seq * n_tok
        mean = 16.0 * torch.rand(M, 1, generator=g) - 8.0                                  # per-row means in +-8
        std = torch.exp2(4.0 * torch.rand(M, 1, generator=g) - 2.0)                        # per-row deviations over 0.25 .. 4
        b = {"x": mean + std * torch.randn(M, D, generator=g), "mod": mod_table(g, n_seq)}
        for name, width in (("res", D), ("a128", D), ("a256", 2 * D), ("a384", 3 * D), ("da", D), ("dx", D)):
            b[name] = torch.randn(M, width, generator=g)
        b["u"] = 1.5 * torch.randn(M, 2 * D, generator=g)
        b["dout"] = torch.randn(n_seq, 4 * n_tok, generator=g)
        for (K, N) in sorted(set(LINEAR_KN.values())):
            b["w%dx%d" % (N, K)] = torch.randn(N, K, generator=g) / K ** 0.5
            b["b%dx%d" % (N, K)] = 0.1 * torch.randn(N, generator=g)
        b["ln_w"] = 1.0 + 0.1 * torch.randn(D, generator=g)
        b["ln_b"] = 0.1 * torch.randn(D, generator=g)
        b["ow"] = torch.randn(4, D, generator=g) / D ** 0.5
        b["dx"] = torch.where(b["dx"] == 0, torch.ones(()), b["dx"])                       # the dx passed in is non-zero everywhere
        _BASE[key] = b
    return _BASE[key]


def form_args(name, n_tok, n_seq):
    """The argument fields (t2s_train_rows_args names -> fp32 tensors) of one case; bf16 operands pre-rounded."""
    op, dtype, gate = FORMS[name]
    b = base(n_tok, n_seq)
    r = rb if dtype == BF16 else (lambda t: t)
    A = {"shift_off": SHIFT_OFF, "scale_off": SCALE_OFF, "gate_off": GATE_OFF}
    if op in LINEAR_KN:
        K, N = LINEAR_KN[op]
        A["w"] = r(b["w%dx%d" % (N, K)])
        if op not in ("GELUBWD", "F_GELUBWD", "LNBWD256", "LNBWD384"):   # the data-gradient forms run without a bias
            A["bias"] = b["b%dx%d" % (N, K)]
    if op in ("QKV0", "QKV1", "FC1", "F_QKV", "F_FC1"):
        A.update(a=b["x"], mod=b["mod"])
        if op in ("QKV1", "FC1"):
            A["res"] = r(b["res"])
    elif op in ("FC2", "F_FC2", "F_GELU"):
        A["a"] = r(b["u"])
    elif op in ("LIN128", "F_LIN128", "GELUBWD", "F_GELUBWD"):
        A["a"] = r(b["a128"])
        if "GELUBWD" in op:
            A["aux"] = r(b["u"])
    elif op == "F_LIN256":
        A["a"] = b["a256"]
    elif op == "F_LIN384":
        A["a"] = b["a384"]
    elif op in ("LNBWD256", "LNBWD384"):
        A.update(a=r(b["a256" if op == "LNBWD256" else "a384"]), ln_x=b["x"], mod=b["mod"], dx=b["dx"])
        if gate:
            A["res"] = r(b["res"])
    elif op in ("FINAL_FUSED", "F_FINAL"):
        A.update(a=b["x"], dout=b["dout"], ln_w=b["ln_w"], ln_b=b["ln_b"], w=b["ow"])
        if op == "FINAL_FUSED":
            A.update(res=r(b["res"]), mod=b["mod"])
    elif op == "F_GATE_RES":
        A.update(a=b["x"], res=b["res"], mod=b["mod"])
    elif op == "F_GATE_BWD":
        A.update(dx=b["dx"], res=b["res"], mod=b["mod"])
    elif op == "F_LN_MOD_BWD":
        A.update(a=b["da"], ln_x=b["x"], mod=b["mod"], dx=b["dx"])
    else:
        raise KeyError(op)
    return A


# ------------------------------------------------------------------------------------------------ the two computations
def _ln(x, eps):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd


def _gelu_grad_formula(u):        # gelu_tanh_grad of t2s_gemm.h
    c = 0.7978845608028654
    sg = torch.sigmoid(2.0 * c * (u + 0.044715 * u * u * u))
    return sg + u * sg * (1.0 - sg) * 2.0 * c * (1.0 + 3.0 * 0.044715 * u * u)


def _mm_k_order(a, w):
    """a (M, K) @ w (N, K)^T in fp32 the way gemm_rows_kernel accumulates it: ONE chain per output, the matrix core taking k in
    the order of the packed weights (k-group g of 8, MFMA e contracts the pair {8g + e, 8g + 4 + e}).  A blocked CPU product
    sums in a tree and deviates from fp64 about three times less at K = 384: it would understate what the kernel's algorithm
    costs."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    wt = w.T.contiguous()
    for g in range(a.shape[1] // 8):
        for e in range(4):
            for h in range(2):
                k = 8 * g + 4 * h + e
                acc.addcmul_(a[:, k:k + 1], wt[k:k + 1])
    return acc


def compute(name, A, n_tok, n_seq, hi):
    """Outputs of one form.  hi: the fp64 reference (definitions, autograd, no rounding).  Otherwise the restatement in the
    kernel's precision (fp32, the kernels' backward formulas, bf16 roundings where the bf16 kernels round)."""
    op, dtype, _ = FORMS[name]
    dt = torch.float64 if hi else torch.float32
    rnd = rb if (dtype == BF16 and not hi) else (lambda t: t)
    c = lambda key: A[key].to(dt)
    so, co, go = A["shift_off"], A["scale_off"], A["gate_off"]
    gelu = lambda t: torch.nn.functional.gelu(t, approximate="tanh")
    mm = _mm_k_order if (dtype == F32 and not hi) else (lambda a, w: a @ w.T)      # (bf16: exact products, the roundings dominate)
    O = {}
    if op in ("QKV0", "QKV1", "FC1", "F_QKV", "F_FC1"):
        x, mod = c("a"), c("mod")
        if op in ("QKV1", "FC1"):
            x = x + seq_rows(mod, go, n_tok) * c("res")
            O["x_out"] = x
        a = rnd(_ln(x, 1e-6)[0] * (1.0 + seq_rows(mod, co, n_tok)) + seq_rows(mod, so, n_tok))
        O["save_a"] = a
        y = mm(a, c("w")) + c("bias")
        if op in ("FC1", "F_FC1"):
            O["out"] = rnd(y)
        else:
            q = y[:, :D] * QS if dtype == BF16 else y[:, :D]
            O["q"], O["k"], O["v"] = (heads(rnd(t), n_seq, n_tok) for t in (q, y[:, D:2 * D], y[:, 2 * D:]))
    elif op in ("FC2", "F_FC2"):
        O["out"] = rnd(mm(rnd(gelu(c("a"))), c("w")) + c("bias"))
    elif op in ("LIN128", "F_LIN128", "F_LIN256", "F_LIN384"):
        O["out"] = rnd(mm(c("a"), c("w")) + c("bias"))
    elif op in ("GELUBWD", "F_GELUBWD"):
        u = c("aux")
        if hi:
            u = u.clone().requires_grad_(True)
            gelu(u).sum().backward()
            gp = u.grad
        else:
            gp = _gelu_grad_formula(u)
        O["out"] = rnd(mm(c("a"), c("w")) * gp)
    elif op == "F_GELU":
        O["out"] = gelu(c("a"))
    elif op == "F_GATE_RES":
        O["x_out"] = c("a") + seq_rows(c("mod"), go, n_tok) * c("res")
    elif op == "F_GATE_BWD":
        O["out"] = seq_rows(c("mod"), go, n_tok) * c("dx")
        O["dmod_gate"] = seq_sum(c("dx") * c("res"), n_seq)
    elif op in ("LNBWD256", "LNBWD384", "F_LN_MOD_BWD"):
        mod = c("mod")
        da = c("a") if op == "F_LN_MOD_BWD" else c("a") @ c("w").T         # (the bf16 step never rounds da: it stays in the accumulators)
        if hi:
            x = c("ln_x").clone().requires_grad_(True)
            sh = mod[:, so:so + D].clone().requires_grad_(True)
            sc = mod[:, co:co + D].clone().requires_grad_(True)
            y = _ln(x, 1e-6)[0] * (1.0 + sc.repeat_interleave(n_tok, dim=0)) + sh.repeat_interleave(n_tok, dim=0)
            y.backward(da)
            dxo, O["dmod_shift"], O["dmod_scale"] = c("dx") + x.grad, sh.grad, sc.grad
        else:
            n, rstd = _ln(c("ln_x"), 1e-6)
            O["dmod_shift"], O["dmod_scale"] = seq_sum(da, n_seq), seq_sum(da * n, n_seq)
            dn = da * (1.0 + seq_rows(mod, co, n_tok))
            dxo = c("dx") + (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True)) * rstd
            O["_da"] = da
        O["dx"] = dxo
        if "res" in A:
            O["out"] = rnd(seq_rows(mod, go, n_tok) * dxo)
            O["dmod_gate"] = seq_sum(dxo * c("res"), n_seq)
    elif op in ("FINAL_FUSED", "F_FINAL"):
        x = c("a")
        if op == "FINAL_FUSED":
            x = x + seq_rows(c("mod"), go, n_tok) * c("res")
        dl = c("dout")[:, patch_index(n_tok)].reshape(n_seq * n_tok, 4)
        gam, bet, ow = c("ln_w"), c("ln_b"), c("w")
        if hi:
            x, gam, bet, ow = (t.detach().clone().requires_grad_(True) for t in (x, gam, bet, ow))
            lin = (_ln(x, 1e-5)[0] * gam + bet) @ ow.T                       # (+ bias: its gradient is the column sum of dl)
            (lin * dl).sum().backward()
            dxo, O["g_ln_w"], O["g_ln_b"], O["g_out_w"] = x.grad, gam.grad, bet.grad, ow.grad
        else:
            n, rstd = _ln(x, 1e-5)
            dy = dl @ ow
            O["g_ln_w"], O["g_ln_b"], O["g_out_w"] = (dy * n).sum(0), dy.sum(0), dl.T @ (n * gam + bet)
            dn = dy * gam
            dxo = (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True)) * rstd
        O["g_out_b"] = dl.sum(0)
        O["dx"] = dxo
        if op == "FINAL_FUSED":
            O["out"] = rnd(seq_rows(c("mod"), go, n_tok) * dxo)
            O["dmod_gate"] = seq_sum(dxo * c("res"), n_seq)
    else:
        raise KeyError(op)
    return {k: v.detach().double() for k, v in O.items()}


def kind(name, out):
    """"b": bf16-rounded rows / heads; "f": fp32 rows (also of the bf16 step); "s": per-sequence fp32; "t": tail gradient."""
    if out.startswith("dmod_"):
        return "s"
    if out.startswith("g_"):
        return "t"
    return "b" if FORMS[name][1] == BF16 and out in ("out", "save_a", "q", "k", "v") else "f"


_CASES = {}


def case(name, n_tok, n_seq):
    key = (name, n_tok, n_seq)
    if key not in _CASES:
        A = form_args(name, n_tok, n_seq)
        ref = compute(name, A, n_tok, n_seq, hi=True)
        res = compute(name, A, n_tok, n_seq, hi=False)
        _CASES[key] = {"name": name, "n_tok": n_tok, "n_seq": n_seq, "args": A, "ref": ref, "res": res}
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ measure, bars, verdict
def groups(t, knd, n_seq):
    """The slices an output is judged in: 32-token tiles (rows (M, width) -> 32 rows; heads (BH, tokens, 32) -> the same 32
    tokens of a sequence's four heads), whole per-sequence rows, or the whole tensor."""
    if knd in ("b", "f"):
        if t.dim() == 3:
            t = t.reshape(-1, NH, t.shape[1], DH).permute(0, 2, 1, 3).reshape(-1, NH * DH)     # heads -> token rows
        return t.reshape(-1, 32 * t.shape[-1])
    return t.reshape(n_seq, -1) if knd == "s" else t.reshape(1, -1)


def measure(got, ref, knd, n_seq):
    """Worst slice: max abs error over the slice / the slice's abs-max of the reference."""
    g, r = groups(got.double(), knd, n_seq), groups(ref, knd, n_seq)
    den = r.abs().amax(-1)
    assert float(den.min()) > 0.0, "a reference slice is all zero"
    err = (g - r).abs().amax(-1) / den
    return float("inf") if not bool(torch.isfinite(g).all()) else float(err.max())


def outputs(cs):
    return sorted(k for k in cs["ref"] if not k.startswith("_"))


def bars(cs):
    """{output: (restatement's deviation, bar)}; a bar above the suite's whole-step bar means the case is mis-built."""
    out = {}
    for o in outputs(cs):
        knd = kind(cs["name"], o)
        d = measure(cs["res"][o], cs["ref"][o], knd, cs["n_seq"])
        out[o] = (d, MULT[knd] * d)
        assert 0.0 < out[o][1] <= CAP[knd], (cs["name"], cs["n_tok"], cs["n_seq"], o, out[o], "mis-built case")
    return out


def judge(cs, got, tag="", quiet=False):
    """Print kernel | restatement | bar per output, return the outputs above their bar."""
    bad = []
    for o, (d, bar) in bars(cs).items():
        e = measure(got[o], cs["ref"][o], kind(cs["name"], o), cs["n_seq"])
        if not quiet:
            print(f"train_rows_errors | {cs['name']} | n_tok={cs['n_tok']} n_seq={cs['n_seq']} {tag}| {o} | kernel {e:.3e} | "
                  f"restatement {d:.3e} | bar {bar:.3e}")
        if not e <= bar:
            bad.append((o, e, bar))
    return bad


# ------------------------------------------------------------------------------------------------ Arm A: integer operands
def integer_weight(N, K):
    """W in {-1, 0, 1}, 8 non-zeros per output row: one in each eighth of the input range, its place moving with the row so
    that all rows together hit every input column (every k-step of 16 / k-group of 8 and both of its halves)."""
    W = torch.zeros(N, K)
    n = torch.arange(N)
    for j in range(8):
        k = j * (K // 8) + (13 * n + 3 * j) % (K // 8)
        W[n, k] = 1.0 - 2.0 * ((n + j) & 1).float()
    assert int((W != 0).sum(1).max()) == 8 and bool((W != 0).any(0).all())
    halves = ((torch.arange(K) >> 3) & 1).bool()
    assert bool((W[:, halves] != 0).any()) and bool((W[:, ~halves] != 0).any())
    return W


def integer_case(name, n_tok, n_seq):
    """Arm A operands of a linear form (drawn here: nothing of base(), so that a large n_seq stays cheap) and the exact product:
    A integer in [-8, 8] (the LayerNorm forms get it through scale = -1, which makes modulate(LN(x)) the sequence's own shift
    row exactly, whatever x is), W of integer_weight, integer bias in [-8, 8]."""
    op = FORMS[name][0]
    K, N = LINEAR_KN[op]
    g = torch.Generator().manual_seed(900 + n_tok + 7 * n_seq)
    M = n_seq * n_tok
    A = {"shift_off": SHIFT_OFF, "scale_off": SCALE_OFF, "gate_off": GATE_OFF, "w": integer_weight(N, K),
         "bias": torch.randint(-8, 9, (N,), generator=g).float()}
    if op in ("QKV0", "QKV1"):
        mod = mod_table(g, n_seq)
        mod[:, SCALE_OFF:SCALE_OFF + D] = -1.0
        mod[:, SHIFT_OFF:SHIFT_OFF + D] = torch.randint(-8, 9, (n_seq, D), generator=g).float()
        A.update(mod=mod, a=3.0 + 2.0 * torch.randn(M, D, generator=g))
        if op == "QKV1":
            A["res"] = rb(torch.randn(M, D, generator=g))
        a = seq_rows(mod, SHIFT_OFF, n_tok)
    else:
        a = A["a"] = torch.randint(-8, 9, (M, K), generator=g).float()
    y = a @ A["w"].T + A["bias"]                          # integers of magnitude <= 72: exact in fp32 and in bf16, in any order
    assert float(y.abs().max()) <= 256 and torch.equal(y, torch.round(y))
    if M <= 4096:
        assert torch.equal(y.double(), a.double() @ A["w"].double().T + A["bias"].double())
    return A, a, y


# ------------------------------------------------------------------------------------------------ what a launch writes
ROW_FIELDS = ("a", "res", "aux", "ln_x", "dx")        # argument fields with one row per token; "mod" and "dout" have one per sequence


def out_shapes(name, A, n_tok, n_seq):
    """{output: shape} of one form, as compute() names them (dmod_* are the (n_seq, 128) slices of dmod)."""
    op = FORMS[name][0]
    M = n_seq * n_tok
    row, hd, sq = (M, D), (n_seq * NH, n_tok, DH), (n_seq, D)
    S = {}
    if op in ("QKV0", "QKV1", "F_QKV"):
        S.update(save_a=row, q=hd, k=hd, v=hd)
    if op in ("FC1", "F_FC1"):
        S.update(out=(M, 2 * D), save_a=row)
    if op in ("QKV1", "FC1", "F_GATE_RES"):
        S["x_out"] = row
    if op in ("FC2", "F_FC2", "LIN128", "F_LIN128", "F_LIN256", "F_LIN384"):
        S["out"] = row
    if op in ("GELUBWD", "F_GELUBWD", "F_GELU"):
        S["out"] = (M, 2 * D)
    if op == "F_GATE_BWD":
        S.update(out=row, dmod_gate=sq)
    if op in ("LNBWD256", "LNBWD384", "F_LN_MOD_BWD"):
        S.update(dx=row, dmod_shift=sq, dmod_scale=sq)
        if "res" in A:
            S.update(out=row, dmod_gate=sq)
    if op in ("FINAL_FUSED", "F_FINAL"):
        S.update(dx=row, g_ln_w=(D,), g_ln_b=(D,), g_out_w=(4, D), g_out_b=(4,))
        if op == "FINAL_FUSED":
            S.update(out=row, dmod_gate=sq)
    return S
