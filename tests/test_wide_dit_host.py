"""The wide-latent DiT without a GPU: the mirror class model.denoiser.mytransformer.Transformer(dim) against the key names and
shapes of the reference's module (recorded in tests/golden/wide_dit.npz by gen_golden_wide.py), the seeded weights, and the
header's new entries."""
import json
import os
import re

import numpy as np
import pytest
import torch

from t2ms_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan(golden_dir):
    return json.loads(str(np.load(os.path.join(golden_dir, "wide_dit.npz"))["plan"]))


@pytest.mark.parametrize("dim", [50, 64])
def test_mirror_state_dict_is_the_references(plan, dim):
    from model.denoiser.mytransformer import Transformer
    want = plan["state_dict"][str(dim)]
    got = {k: list(v.shape) for k, v in Transformer(dim).state_dict().items()}
    assert got == want
    assert got["pos_embed"] == [1, 16 * dim, 128]
    assert any(k.startswith("unpatch.") for k in got)        # the dead keys a reference checkpoint carries
    m = Transformer(dim)
    m.load_state_dict(synth.make_dit_state_dict(2025, width=dim), strict=True)
    assert (m.H, m.W, m.patch_count) == (dim, 64, 16 * dim)


def test_dim_30_is_the_existing_mirror():
    from model.denoiser import mytransformer, transformer
    a, b = mytransformer.Transformer(30).state_dict(), transformer.Transformer().state_dict()
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    assert issubclass(mytransformer.Transformer, transformer.Transformer)      # one class body
    for name in ("t2s_handle", "_forward_nograd", "set_pairing", "_weights_struct"):
        assert getattr(mytransformer.Transformer, name) is getattr(transformer.Transformer, name), name
    assert torch.equal(a["pos_embed"], b["pos_embed"])


def test_root_shim_and_pickle_module():
    import model.denoiser.mytransformer as shim
    import t2ms_amd.model.denoiser.mytransformer as real
    assert shim.Transformer is real.Transformer
    assert real.Transformer.__module__ == "model.denoiser.mytransformer"
    with pytest.raises(TypeError):
        shim.Transformer()                       # dim is required, as in the fork


def test_unsupported_dim_and_wide_math_are_refused_on_the_host():
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd import _lib as L
    with pytest.raises(L.T2SError, match="30, 50 or 64"):
        Transformer(40)
    m = Transformer(64)
    assert m.set_math("f32") is m
    for math in ("bf16x3", "bf16"):
        with pytest.raises(L.T2SError, match="f32"):
            m.set_math(math)
    Transformer(30).set_math("bf16x3")


def test_seeded_weights_do_not_move_with_the_width():
    base, w30, w64 = synth.make_dit_state_dict(2025), synth.make_dit_state_dict(2025, width=30), synth.make_dit_state_dict(2025, width=64)
    assert list(base) == list(w30) == list(w64)
    for k in base:
        assert torch.equal(base[k], w30[k]), k
        if k != "pos_embed":
            assert torch.equal(base[k], w64[k]), k
    assert tuple(base["pos_embed"].shape) == (1, 480, 128) and tuple(w64["pos_embed"].shape) == (1, 1024, 128)
    assert torch.equal(w64["pos_embed"][:, :480], base["pos_embed"])          # the sinusoid table, more rows of it
    assert tuple(synth.make_dit_state_dict(2025, width=50)["pos_embed"].shape) == (1, 800, 128)


def test_header_declares_the_wide_entries():
    text = open(os.path.join(REPO, "include", "t2s.h")).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int t2s_dit_create_w(const t2s_dit_weights* w, int latent_w, int max_seqs, t2s_dit** out);",
                 "int t2s_dit_weights_check_w(const t2s_dit_weights* w, int latent_w, const uint64_t* n_floats, int n_entries);",
                 "int t2s_dit_latent_w(const t2s_dit* h);",
                 "int t2s_attn_fwd_packed_n(const float* q, const float* k, const float* vT, float* o, int n_seq, int n_tok, void* stream);"):
        assert decl in flat, decl
    from t2ms_amd import _lib as L
    for name in ("t2s_dit_create_w", "t2s_dit_weights_check_w", "t2s_dit_latent_w", "t2s_attn_fwd_packed_n", "t2s_lms_step_n"):
        assert name in L.SYMBOLS, name
