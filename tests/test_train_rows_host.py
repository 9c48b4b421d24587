"""Host side of the row-kernel tests (no GPU): the extension header include/t2s_train_rows.h and its symbol table, and what
tests/test_train_rows.py rests on -- the CPU restatements agree with the fp64 references (tests/_train_rows_ref.py), and the
per-tile comparison built on them REJECTS subtly damaged results: the evidence that its bars are sharp, without a GPU."""
import glob
import os
import re

import pytest
import torch

import _train_rows_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_header_and_its_symbol_table_agree():
    """include/t2s_train_rows.h declares exactly the entries of _lib.SYMBOLS_TRAIN_ROWS (with these argtypes), none of them is in
    another table or header, the T2S_ROWS_* codes are _lib.TRAIN_ROWS_OPS, and the struct mirrors field for field."""
    import ctypes as C
    from t2ms_amd import _lib as L
    raw = open(os.path.join(REPO, "include", "t2s_train_rows.h")).read()
    assert "for tests / benchmarking of those" in raw
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(L.SYMBOLS_TRAIN_ROWS) == {"t2s_train_rows"}
    for other in (L.SYMBOLS, L.SYMBOLS_WIDE_TRAIN, L.SYMBOLS_WIDE_MATH, L.SYMBOLS_WIDE_TRAIN_BF16):
        assert not declared & set(other)
    for header in ("t2s.h", "t2s_wide_train.h", "t2s_wide_math.h", "t2s_wide_train_bf16.h"):
        body = open(os.path.join(REPO, "include", header)).read()
        assert not any(re.search(r"\b%s\s*\(" % name, body) for name in declared), header
    VP, I = C.c_void_p, C.c_int
    assert L.SYMBOLS_TRAIN_ROWS["t2s_train_rows"] == (I, [I, I, I, I, I, C.POINTER(L.TrainRowsArgs), VP])
    codes = {k: int(v) for k, v in re.findall(r"\bT2S_ROWS_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert codes == L.TRAIN_ROWS_OPS and {f[0] for f in R.FORMS.values()} == set(codes)
    struct = re.search(r"typedef struct t2s_train_rows_args \{(.*?)\}", txt, flags=re.S).group(1)
    fields = re.findall(r"(const float\*|float\*|int)\s+([a-z_]+);", struct)
    assert [n for _, n in fields] == [n for n, _ in L.TrainRowsArgs._fields_]
    assert all((t == "int") == (ct is C.c_int) for (t, _), (_, ct) in zip(fields, L.TrainRowsArgs._fields_))
    lib = L.lib()
    for name, (res, args) in L.SYMBOLS_TRAIN_ROWS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args


def test_nothing_of_the_product_path_calls_the_entry():
    files = [f for pat in ("*.py", "t2ms_amd/*.py", "model/**/*.py", "datafactory/**/*.py") for f in glob.glob(os.path.join(REPO, pat), recursive=True)]
    assert len(files) > 20
    users = [os.path.relpath(f, REPO) for f in files if "t2s_train_rows" in open(f).read()]
    assert users == [os.path.join("t2ms_amd", "_lib.py")], users


@pytest.mark.parametrize("n_tok", R.TOKENS)
@pytest.mark.parametrize("name", sorted(R.FORMS))
def test_restatements_agree_with_the_fp64_references(name, n_tok):
    """Every output of every case, per tile / sequence / tensor: the restatement deviates (it is another arithmetic) and its
    bar -- 2 x / 4 x the deviation -- stays within the suite's whole-step bars (R.bars asserts it); the restatement itself
    passes the comparison; per tensor the relative L2 deviation is within those bars too."""
    for n_seq in (1, 3):
        cs = R.case(name, n_tok, n_seq)
        for o, (d, bar) in R.bars(cs).items():
            knd = R.kind(name, o)
            l2 = float((cs["res"][o] - cs["ref"][o]).norm() / cs["ref"][o].norm())
            print(f"train_rows_errors | restatement | {name} | n_tok={n_tok} n_seq={n_seq} | {o} | worst slice {d:.3e} | bar {bar:.3e} | L2 {l2:.3e}")
            assert 0.0 < d and bar <= R.CAP[knd] and l2 < R.CAP[knd], (o, d, bar, l2)
        assert R.judge(cs, cs["res"], quiet=True) == []


def test_the_inputs_are_what_the_comparison_is_built_for():
    for n_tok in R.TOKENS:
        b = R.base(n_tok, 3)
        x, mod = b["x"].double(), b["mod"]
        assert float(x.mean(1).min()) < -7.0 and float(x.mean(1).max()) > 7.0
        assert float(x.std(1).min()) < 0.35 and float(x.std(1).max()) > 3.0
        used = torch.zeros(R.MODROW, dtype=torch.bool)
        for off in (R.SHIFT_OFF, R.SCALE_OFF, R.GATE_OFF):
            assert not bool(used[off:off + R.D].any())
            used[off:off + R.D] = True
            rows = mod[:, off:off + R.D]
            assert float((rows[0] - rows[1]).abs().min()) >= 0.0 and not torch.equal(rows[0], rows[1]) and not torch.equal(rows[1], rows[2])
            assert float(rows.abs().max()) < 10.0
        assert float(mod[:, ~used].abs().min()) == R.SENTINEL
        assert float(b["dx"].abs().min()) > 0.0
    for (K, N) in sorted(set(R.LINEAR_KN.values())):
        R.integer_weight(N, K)


# ------------------------------------------------------------------------------------------------ the checker is sharp
N_TOK, N_SEQ = 480, 3


def _damaged(name):
    cs = R.case(name, N_TOK, N_SEQ)
    assert R.judge(cs, cs["res"], quiet=True) == []
    return cs, {o: t.clone() for o, t in cs["res"].items()}


def _rejected(cs, got, output):
    bad = R.judge(cs, got, quiet=True)
    assert [b[0] for b in bad] == [output], (cs["name"], bad)
    l2 = float((got[output] - cs["ref"][output]).norm() / cs["ref"][output].norm())
    print(f"train_rows_errors | damaged | {cs['name']} | {output} | worst slice {bad[0][1]:.3e} | bar {bad[0][2]:.3e} | whole-tensor L2 {l2:.3e}")


@pytest.mark.parametrize("name,output", [("FC1", "x_out"), ("LIN128", "out"), ("F_FC2", "out")])
def test_rejects_two_rows_swapped_inside_one_tile(name, output):
    cs, got = _damaged(name)
    got[output][[40, 41]] = got[output][[41, 40]]
    _rejected(cs, got, output)


@pytest.mark.parametrize("name,output", [("QKV0", "k"), ("QKV1", "save_a"), ("F_QKV", "v")])
def test_rejects_a_tile_computed_with_the_neighbouring_sequences_scale_row(name, output):
    """The LAST tile of sequence 0 modulated with sequence 1's scale row (what a tile -> sequence map that is off by one tile
    at the boundary gives)."""
    cs, got = _damaged(name)
    A = dict(cs["args"])
    mod = A["mod"].clone()
    mod[0, R.SCALE_OFF:R.SCALE_OFF + R.D] = A["mod"][1, R.SCALE_OFF:R.SCALE_OFF + R.D]
    A["mod"] = mod
    wrong = R.compute(name, A, N_TOK, N_SEQ, hi=False)[output]
    if wrong.dim() == 3:
        got[output][0:R.NH, N_TOK - 32:] = wrong[0:R.NH, N_TOK - 32:]
    else:
        got[output][N_TOK - 32:N_TOK] = wrong[N_TOK - 32:N_TOK]
    _rejected(cs, got, output)


@pytest.mark.parametrize("name", ["LNBWD256", "LNBWD384_NOGATE"])
@pytest.mark.parametrize("output", ["dmod_shift", "dmod_scale"])
def test_rejects_a_tile_left_out_of_a_dmod_column_sum(name, output):
    cs, got = _damaged(name)
    da = cs["res"]["_da"]
    n = R._ln(cs["args"]["ln_x"].float(), 1e-6)[0].double()
    rows = slice(N_TOK + 7 * 32, N_TOK + 8 * 32)                       # tile 7 of sequence 1
    got[output][1] -= (da[rows] if output == "dmod_shift" else da[rows] * n[rows]).sum(0)
    _rejected(cs, got, output)


@pytest.mark.parametrize("name,output", [("GELUBWD", "out"), ("LNBWD256", "dx"), ("FC2", "out")])
def test_rejects_swapped_halves_of_one_n_tile(name, output):
    """Accumulator register 4g + e of an n-tile is feature 32 nt + 8 g + 4 h + e: h and 1 - h exchanged in n-tile 3 of tile 1."""
    cs, got = _damaged(name)
    blk = got[output][32:64, 96:128].reshape(32, 4, 2, 4)
    got[output][32:64, 96:128] = blk.flip(2).reshape(32, 32)
    _rejected(cs, got, output)


@pytest.mark.parametrize("name", ["LNBWD256", "LNBWD384", "F_LN_MOD_BWD"])
def test_rejects_dx_overwritten_instead_of_accumulated(name):
    cs, got = _damaged(name)
    got["dx"][64:96] -= cs["args"]["dx"][64:96].double()
    _rejected(cs, got, "dx")


@pytest.mark.parametrize("name", ["QKV0", "QKV1"])
def test_rejects_q_left_unscaled(name):
    cs, got = _damaged(name)
    got["q"] = R.rb(cs["res"]["q"] / R.QS)
    _rejected(cs, got, "q")
