"""Host side of the long-series TS2Vec encoder (csrc/t2s_ts2vec_encode.hip): the C ABI's new symbols, the refusals and the
growth of t2s_ts2vec_encode_workspace_bytes, the mirror's routing and chunk planning (t2ms_amd.metrics), and the oracle
against the reference's long-series fixture.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import t2s_oracle as O
from t2ms_amd import _lib as L
from t2ms_amd import metrics as M
from t2ms_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "ts2vec_long.npz")
NEW = ("t2s_ts2vec_encode_workspace_bytes", "t2s_ts2vec_encode_long")


def _sizes(input_dims=1, hidden=64, output_dims=100, depth=10):
    w = L.Ts2vecWeights()
    w.input_dims, w.hidden, w.output_dims, w.depth = input_dims, hidden, output_dims, depth
    return w


def _bytes(w, B, T):
    return L.lib().t2s_ts2vec_encode_workspace_bytes(C.byref(w), B, T)


def test_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "t2s.h")).read(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.SYMBOLS["t2s_ts2vec_encode_workspace_bytes"][0] is C.c_uint64
    assert L.SYMBOLS["t2s_ts2vec_encode_long"][0] is C.c_int
    assert re.search(r"#define\s+T2S_TS2VEC_ENCODE_MAX_T\s+%d\b" % L.TS2VEC_ENCODE_MAX_T, header)
    assert L.TS2VEC_ENCODE_MAX_T == 4096
    assert "t2s_ts2vec_encode.hip" in open(os.path.join(REPO, "t2ms_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("kw,B,T,words", [
    ({}, 2, 0, "T=0"), ({}, 2, 4097, "T=4097"), ({}, 0, 96, "B=0"), ({"hidden": 129}, 2, 96, "hidden=129"),
    ({"output_dims": 321}, 2, 96, "output_dims=321"), ({"input_dims": 65}, 2, 96, "input_dims=65"),
    ({"depth": 16}, 2, 96, "depth=16")])
def test_workspace_bytes_refuses_with_the_offending_value(kw, B, T, words):
    assert _bytes(_sizes(**kw), B, T) == 0
    msg = L.lib().t2s_last_error().decode()
    assert "t2s_ts2vec_encode_workspace_bytes" in msg and words in msg, msg


def test_workspace_bytes_grows_with_B_and_T_and_equals_the_mirror_formula():
    w = _sizes()
    assert _bytes(w, 1, 1) > 0
    for T in (1, 96, 137, 4096):
        vals = [_bytes(w, B, T) for B in (1, 2, 3, 8, 64)]
        assert all(a < b for a, b in zip(vals, vals[1:])), vals
    for B in (1, 5):
        vals = [_bytes(w, B, T) for T in (1, 2, 31, 32, 33, 136, 137, 1025, 4096)]
        assert all(a < b for a, b in zip(vals, vals[1:])), vals
    # three (B, 128, T) fp32 planes dominate: the packed weights of the default sizes stay under 2 MiB
    assert 0 < _bytes(w, 4, 300) - 3 * 4 * 128 * 300 * 4 < 2 << 20
    for kw in ({}, {"hidden": 48, "output_dims": 36, "depth": 3, "input_dims": 3}, {"hidden": 128, "output_dims": 320, "depth": 15},
               {"hidden": 96, "output_dims": 7, "depth": 0}, {"hidden": 1, "output_dims": 1, "depth": 1}):
        s = _sizes(**kw)
        for B, T in ((1, 1), (3, 137), (7, 1025), (2, 4096)):
            assert _bytes(s, B, T) == M._encode_workspace_bytes(B, T, s.hidden, s.output_dims, s.depth), (kw, B, T)


def test_routing_table():
    # 3 planes x cmax x T x 4 bytes against the 160 KB of LDS: T <= 136 at 100 channels, T <= 213 at 64
    assert M._encode_path(136, 100) == "lds" and M._encode_path(137, 100) == "gemm"
    assert M._encode_path(213, 64) == "lds" and M._encode_path(214, 64) == "gemm"
    assert M._encode_path(1, 100) == "lds" and M._encode_path(4096, 100) == "gemm"
    for T, cmax in ((24, 100), (136, 100), (137, 100), (4096, 64)):
        assert M._encode_path(T, cmax, "lds") == "lds" and M._encode_path(T, cmax, "gemm") == "gemm"
        assert M._encode_path(T, cmax, None) == M._encode_path(T, cmax)
    for bad in ("torch", "", "LDS", 0):
        with pytest.raises(L.T2SError, match="path"):
            M._encode_path(96, 100, bad)


def test_chunk_planner_covers_every_row_once_under_the_cap():
    sizes = (64, 100, 10)
    for B, T, cap in ((1, 137, None), (512, 720, None), (2048, 4096, None), (7, 300, 3 << 20), (9, 300, 1 << 20),
                      (5, 4096, 1 << 20), (100, 137, 8 << 20)):
        chunks = M._encode_chunks(B, T, *sizes, cap=cap)
        rows = [r for r0, n in chunks for r in range(r0, r0 + n)]
        assert rows == list(range(B)), (B, T, cap)
        assert all(n >= 1 for _, n in chunks)
        limit = M.ENCODE_WORKSPACE_CAP if cap is None else cap
        one = M._encode_workspace_bytes(1, T, *sizes)
        if one > limit:                                   # a single row exceeds the cap: one row per chunk
            assert chunks == [(i, 1) for i in range(B)]
        else:
            biggest = max(n for _, n in chunks)
            assert M._encode_workspace_bytes(biggest, T, *sizes) <= limit
            assert biggest == B or M._encode_workspace_bytes(biggest + 1, T, *sizes) > limit   # and no smaller than needed
    assert M.ENCODE_WORKSPACE_CAP == 256 << 20
    assert M._encode_chunks(3, 137, *sizes) == [(0, 3)]
    assert M._encode_workspace_bytes(1, 4096, *sizes) > (1 << 20) and M._encode_chunks(5, 4096, *sizes, cap=1 << 20) == [(i, 1) for i in range(5)]
    assert M._encode_chunks(0, 137, *sizes) == []


def test_oracle_equals_reference_at_long_lengths():
    """oracle.ts2vec_encode against the reference's TSEncoder.forward at T = 137, 300 and 1025 (ts2vec_long.npz), held to
    the bar of test_ts2vec_encoder_restatement_equals_reference: 1e-5 of max|rep|."""
    g = np.load(GOLD, allow_pickle=False)
    assert [tuple(r) for r in g["cases"][:, :3]] == [(1, 137, 3), (10, 300, 3), (1, 1025, 2)]
    for k, (cin, T, B, stride) in enumerate(g["cases"]):
        x = g[f"x_{k}"]
        assert x.shape == (B, T, cin) and np.isnan(x[1]).any() and not np.isnan(x[0]).any()
        sd = synth.make_ts2vec_state_dict(2025, input_dims=int(cin))
        with torch.no_grad():
            rep, full = O.ts2vec_encode(sd, torch.from_numpy(x))
        assert tuple(rep.shape) == (B, T, 100)
        scale = float(np.abs(g[f"rep_{k}"]).max())
        assert scale > 0.1
        assert float(np.abs(rep[:, ::int(stride)].numpy() - g[f"rep_{k}"]).max()) <= 1e-5 * scale
        assert float(np.abs(full.numpy() - g[f"full_{k}"]).max()) <= 1e-5 * scale
