"""The training step's fused row GEMMs and row kernels, each launch form called ALONE (t2s_train_rows, include/t2s_train_rows.h:
the host helpers of t2s_dit_train_forward / _backward on plain buffers) and held to fp64.  Needs an MI355X.

The forms: the bf16 step's bgemm_kernel prologues and epilogues (LayerNorm+modulate, gated residual+LayerNorm, GELU; q/k/v
scatter, gelu', LayerNorm backward + lnbwd_colsum_reduce_kernel), the fp32 step's gemm_rows_kernel forms with gate_res_kernel,
gate_bwd_kernel, ln_mod_bwd_kernel (f_next == NULL, the only arm a recipe reaches) and gelu_kernel, and final_bwd_kernel of
both steps -- at 480, 800 and 1024 tokens (the compile-time and the run-time forms).

  Arm A  integer operands: the layout of the plain linear forms and of the q/k/v scatter, bit for bit.
  Arm B  every form against its fp64 reference PER 32-TOKEN TILE (per sequence for the adaLN sums), at 1 and 3 sequences.  The
         bars are 2 x (bf16-rounded outputs) / 4 x (fp32 outputs) what a CPU restatement in the kernel's precision deviates from
         the same reference -- the rule and the reasons of tests/test_train_kernels.py (_bars_bf16, _bars_f32) -- and never come
         from the kernel (tests/_train_rows_ref.py; tests/test_train_rows_host.py shows that they reject subtle faults).
  Arm C  the persistent loop's later trips: enough sequences that a wave takes a second tile, both walk directions; every
         sequence must give the bits the same sequence gave in a one-trip launch.

profiles/train_rows_errors.md holds the figures these tests print (pytest -s)."""
import pytest
import torch

import _train_rows_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _to_dev(A, dev):
    return {k: (v.contiguous().to(dev) if torch.is_tensor(v) else v) for k, v in A.items()}


def _dmod_sentinel(n_seq, dev):
    cols = torch.arange(R.MODROW, device=dev)
    return (-R.SENTINEL * (1.0 - 2.0 * (cols & 1).float())).repeat(n_seq, 1).contiguous()


def _launch(dev, name, A, n_tok, n_seq, flags, op=None, dtype=None, drop=()):
    """One t2s_train_rows call on device tensors A.  Outputs are pre-filled with NaN (dmod with a sentinel pattern, dx with the
    caller's dx).  -> (rc, {output: device tensor}, the raw buffers)."""
    from t2ms_amd import _lib as L
    shapes = R.out_shapes(name, A, n_tok, n_seq)
    args = L.TrainRowsArgs()
    keep = []
    for f in ("a", "w", "bias", "mod", "res", "aux", "ln_x", "dout", "ln_w", "ln_b"):
        if f in A and f not in drop:
            assert A[f].dtype == torch.float32 and A[f].is_contiguous() and A[f].is_cuda
            setattr(args, f, A[f].data_ptr())
    args.shift_off, args.scale_off, args.gate_off = A["shift_off"], A["scale_off"], A["gate_off"]
    buf = {}
    for o, shp in shapes.items():
        if not o.startswith("dmod_") and not (o == "dx" and "dx" in A):      # (the final-layer forms only WRITE dx)
            buf[o] = torch.full(shp, float("nan"), device=dev)
    if "dx" in A:
        buf["dx"] = A["dx"].clone()
    if any(o.startswith("dmod_") for o in shapes):
        buf["dmod"] = _dmod_sentinel(n_seq, dev)
    for f, t in buf.items():
        if f not in drop:
            setattr(args, f, t.data_ptr())
    keep.append(args)
    form = R.FORMS[name]
    rc = L.lib().t2s_train_rows(L.TRAIN_ROWS_OPS[form[0]] if op is None else op, form[1] if dtype is None else dtype, n_tok, n_seq,
                                flags, args, L.stream_ptr(dev))
    out = {}
    offs = {"dmod_shift": A["shift_off"], "dmod_scale": A["scale_off"], "dmod_gate": A["gate_off"]}
    for o in shapes:
        out[o] = buf["dmod"][:, offs[o]:offs[o] + R.D] if o.startswith("dmod_") else buf[o]
    return rc, out, buf


def _run(dev, name, A, n_tok, n_seq, flags):
    from t2ms_amd import _lib as L
    try:
        rc, out, buf = _launch(dev, name, A, n_tok, n_seq, flags)
        L.check(rc, "t2s_train_rows")
        torch.cuda.synchronize(dev)
    except (RuntimeError, L.T2SError) as e:      # a HIP error: nothing more of this module is started on the device
        pytest.exit(f"t2s_train_rows {name} n_tok={n_tok} n_seq={n_seq} flags={flags}: {e}", returncode=3)
    for o, t in out.items():
        assert bool(torch.isfinite(t).all()), (name, o, "an output element was not written, or is not finite")
    if "dmod" in buf:            # nothing but the asked slices of dmod was written
        written = torch.zeros(R.MODROW, dtype=torch.bool, device=dev)
        for o, off in (("dmod_shift", A["shift_off"]), ("dmod_scale", A["scale_off"]), ("dmod_gate", A["gate_off"])):
            if o in out:
                written[off:off + R.D] = True
        assert torch.equal(buf["dmod"][:, ~written], _dmod_sentinel(n_seq, dev)[:, ~written]), (name, "dmod written outside its slices")
    return out


# ------------------------------------------------------------------------------------------------ Arm A
ARM_A = ("LIN128", "QKV0", "QKV1", "F_LIN128", "F_LIN256", "F_LIN384")


def _check_integer(dev, name, n_tok, n_seq, flags):
    A, _, y = R.integer_case(name, n_tok, n_seq)
    got = _run(dev, name, _to_dev(A, dev), n_tok, n_seq, flags)
    if name in ("QKV0", "QKV1"):
        q = (y[:, :R.D].float() * R.QS).to(torch.bfloat16).float()
        want = {"q": R.heads(q, n_seq, n_tok), "k": R.heads(y[:, R.D:2 * R.D], n_seq, n_tok), "v": R.heads(y[:, 2 * R.D:], n_seq, n_tok),
                "save_a": R.seq_rows(A["mod"], R.SHIFT_OFF, n_tok)}
        if name == "QKV1":       # x + gate * res: fp32, to an ulp of the fused multiply-add the compiler may or may not form
            x = A["a"].double() + R.seq_rows(A["mod"], R.GATE_OFF, n_tok).double() * A["res"].double()
            assert float(((got["x_out"].cpu().double() - x).abs() / x.abs().clamp(min=1.0)).max()) < 2.0 ** -22
    else:
        want = {"out": y}
    for o, w in want.items():
        g = got[o].cpu()
        assert torch.equal(g, w), (name, n_tok, n_seq, flags, o, int((g != w).sum()), float((g - w).abs().max()))


@pytest.mark.parametrize("n_tok", R.TOKENS)
@pytest.mark.parametrize("name", ARM_A)
def test_linear_forms_and_the_qkv_scatter_are_exact_on_integers(dev, name, n_tok):
    """A integer in [-8, 8], W in {-1, 0, 1} with 8 non-zeros per output row over every k-step and both halves, integer bias:
    every output is an integer of magnitude <= 72, exact in fp32 and bf16 in any summation order, and must be the fp32 CPU
    product's bits -- k and v (and the saved activation) of the q/k/v scatter included, q as (y * QS) rounded to bf16.  Three
    sequences with a shift row each; both tile walk directions of the persistent bf16 GEMMs."""
    for flags in ((0, 2) if R.FORMS[name][1] == R.BF16 else (0,)):
        _check_integer(dev, name, n_tok, 3, flags)


# ------------------------------------------------------------------------------------------------ Arm B
@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("n_tok", R.TOKENS)
@pytest.mark.parametrize("name", sorted(R.FORMS))
def test_every_form_against_fp64_per_tile(dev, name, n_tok, n_seq):
    """Every output of every launch form against the fp64 reference of the (rounded) operands: per 32-token tile the max abs
    error over the tile's abs-max of the reference (per sequence for the adaLN sums, per tensor for the tail gradients), bar
    2 x / 4 x the CPU restatement's worst slice (bf16-rounded / fp32 outputs; _train_rows_ref.bars, which also refuses a bar
    above the suite's whole-step bars 1e-2 / 2e-4 as a mis-built case).  15, 25 and 32 tiles per sequence with the sequence
    boundary inside the launch (n_seq = 3, walked descending) and without; every sequence has adaLN rows of its own in a
    full-width table whose other columns would poison the result; dx comes in non-zero.
    Measured on an MI355X: profiles/train_rows_errors.md."""
    cs = R.case(name, n_tok, n_seq)
    flags = 2 if n_seq == 3 else 0
    got = {o: t.cpu() for o, t in _run(dev, name, _to_dev(cs["args"], dev), n_tok, n_seq, flags).items()}
    bad = R.judge(cs, got, tag=f"flags={flags} ")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ Arm C
def _later_trip_sequences(dev, name, n_tok):
    """Sequences for a launch in which some wave of the persistent grid takes a second tile: launch_bgemm (t2s_bf16.h) caps
    the grid at n_cu workgroups of 12 waves (8 with the LayerNorm-backward epilogue)."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    waves = (8 if name.startswith("LNBWD") else 12) * n_cu
    tps = n_tok // 32
    n_big = waves // tps + 2                   # the smallest count with more tiles than waves, plus one whole sequence
    assert (n_big - 1) * tps > waves and n_big * tps < 3 * waves, (n_cu, n_big)      # some wave takes two tiles, none a fourth
    return n_cu, n_big


def _source(n_big, dev):
    """Which of the three base sequences each sequence of the large launch is (neighbours differ, no period of 3)."""
    i = torch.arange(n_big, device=dev)
    return (i * i + i // 3) % 3


def _tile_args(A3, src, n_tok):
    big = {}
    for f, t in A3.items():
        if f in R.ROW_FIELDS:
            big[f] = t.reshape(3, -1)[src].reshape(-1, t.shape[-1]).contiguous()
        elif f in ("mod", "dout"):
            big[f] = t[src].contiguous()
        else:
            big[f] = t
    return big


def _same_bits_per_sequence(name, got, base, src, n_big, skip=()):
    for o, t in got.items():
        if o in skip:
            continue
        want = base[o].reshape(3, -1)[src]
        same = (t.reshape(n_big, -1) == want).all(1)
        assert bool(same.all()), (name, o, "sequences that differ from the one-trip launch", torch.nonzero(~same).flatten()[:8].tolist())


@pytest.mark.parametrize("n_tok", R.TOKENS)
@pytest.mark.parametrize("name", [n for n in R.BF16_FORMS if n != "FINAL_FUSED"])
def test_later_trips_of_the_persistent_loop_give_the_one_trip_bits(dev, name, n_tok):
    """The Arm B three-sequence case tiled to the smallest launch in which a wave takes a second tile (asserted from the CU
    count), each sequence one of the three with ITS adaLN row: rows are independent and the column-sum partials keep their
    tile order, so every output row and every per-sequence dmod slice must be bit for bit what that sequence gave in the
    one-trip launch -- in both walk directions.  (Staging-tile reuse, the reverse tile order, the colpart row index.)"""
    n_cu, n_big = _later_trip_sequences(dev, name, n_tok)
    A3 = _to_dev(R.case(name, n_tok, 3)["args"], dev)
    base = _run(dev, name, A3, n_tok, 3, 0)
    src = _source(n_big, dev)
    big = _tile_args(A3, src, n_tok)
    print(f"train_rows_errors | later trips | {name} | n_tok={n_tok} | n_cu={n_cu} | n_seq={n_big} | tiles={n_big * n_tok // 32}")
    for flags in (0, 2):
        _same_bits_per_sequence(name, _run(dev, name, big, n_tok, n_big, flags), base, src, n_big)


@pytest.mark.parametrize("n_tok", R.TOKENS)
@pytest.mark.parametrize("name", ["LIN128", "QKV0", "QKV1"])
def test_later_trips_are_exact_on_integers(dev, name, n_tok):
    """Arm A at the size of Arm C, against the fp32 CPU product."""
    _, n_big = _later_trip_sequences(dev, name, n_tok)
    for flags in (0, 2):
        _check_integer(dev, name, n_tok, n_big, flags)


@pytest.mark.parametrize("n_tok", R.TOKENS)
def test_fused_final_backward_does_not_depend_on_the_batch(dev, n_tok):
    """final_bwd_kernel<true, ...> + final_gate_reduce_kernel at 11 sequences (no multiple of the 3 / 5 / 8 workgroups a sequence
    takes): dx, t and the dgate row of every sequence are the bits of the three-sequence launch; the tail gradients are sums
    over all rows and are only required to be finite here (Arm B holds them to fp64)."""
    name, n_big = "FINAL_FUSED", 11
    A3 = _to_dev(R.case(name, n_tok, 3)["args"], dev)
    base = _run(dev, name, A3, n_tok, 3, 0)
    src = _source(n_big, dev)
    got = _run(dev, name, _tile_args(A3, src, n_tok), n_tok, n_big, 0)
    _same_bits_per_sequence(name, got, base, src, n_big, skip=("g_ln_w", "g_ln_b", "g_out_w", "g_out_b"))


# ------------------------------------------------------------------------------------------------ refusals
def test_the_entry_refuses_bad_arguments_before_any_launch(dev):
    from t2ms_amd import _lib as L
    lib = L.lib()
    n_tok, n_seq = 480, 1
    A = _to_dev(R.case("LIN128", n_tok, n_seq)["args"], dev)

    def refused(needle, **kw):
        n_t, n_s = kw.pop("n_tok", n_tok), kw.pop("n_seq", n_seq)
        rc, out, _ = _launch(dev, kw.pop("name", "LIN128"), A, n_t, n_s, kw.pop("flags", 0), **kw)
        msg = lib.t2s_last_error()
        assert rc != 0 and needle in msg, (rc, msg)
        for t in out.values():
            assert bool(torch.isnan(t).all()), "an output was written by a refused call"

    refused(b"unknown op", op=9)
    refused(b"unknown op", op=28)
    refused(b"unknown dtype", dtype=7)
    refused(b"n_tok=512", n_tok=512)
    refused(b"n_seq=0", n_seq=0)
    refused(b"needs a", drop=("a",))
    refused(b"needs w", drop=("w",))
    refused(b"needs out", drop=("out",))
    refused(b"T2S_TRAIN_BF16 launch form", dtype=R.F32)                              # a bf16 form asked in fp32 ...
    refused(b"T2S_TRAIN_F32 launch form", op=L.TRAIN_ROWS_OPS["F_LIN128"], dtype=R.BF16)   # ... and the other way round
    refused(b"unknown flags", flags=1)
    assert lib.t2s_train_rows(L.TRAIN_ROWS_OPS["LIN128"], R.BF16, n_tok, n_seq, 0, None, L.stream_ptr(dev)) != 0
    assert b"args is NULL" in lib.t2s_last_error()
