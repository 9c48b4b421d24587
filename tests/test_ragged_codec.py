"""Ragged rows of the multichannel LA-VAE codec: t2s_vae_decode_mc_ragged / t2s_vae_encode_mc_ragged and the mirrors'
Encoder.encode_ragged / Decoder.decode_ragged (one launch, a length per row).

Every criterion is a BIT-EQUALITY against t2s_vae_encode_mc / t2s_vae_decode_mc, the uniform entries that tests/test_mvae.py
holds to the reference's outputs (tests/golden/mvae.npz, 1e-5): the ragged kernels are thin wrappers around the same per-series
body, so a row must come out as from the uniform entry run on that row alone.  No tolerance is involved.

Lengths of the one launch (synthetic weights, 2 residual layers): 8 the minimum; 11 resampled; 36; 41; 128 (L/4 = 32, the
last one-tile length); 131; 132 (L/4 = 33, the first tiled length); 203 (three tiles and resampled); 0 a skipped row.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from t2ms_amd import _lib as L
from t2ms_amd import synth

pytestmark = pytest.mark.gpu

LENGTHS = [8, 11, 36, 41, 128, 131, 132, 203, 0]
SENTINEL = 0x7FC0BEEF          # a NaN payload no kernel produces
E_INVALID = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


_MODELS = {}


def _model(ch, W, dev):
    from model.pretrained.myvqvae import vqvae
    if (ch, W) not in _MODELS:
        m = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64,
                                        flow_dim=W, input_dim=ch))
        m.load_state_dict(synth.make_mvae_state_dict(2025 + ch, ch, 128, 2, 256), strict=True)
        _MODELS[(ch, W)] = m.to(dev).eval()
    return _MODELS[(ch, W)]


def _rows(ch, lengths, dev, seed=5):
    """One series per row, (ch, L_b); an empty tensor for a 0 row."""
    return [synth.make_mseries(seed + 13 * b + Lb, 1, ch, Lb)[0].to(dev) if Lb else torch.empty(ch, 0, device=dev)
            for b, Lb in enumerate(lengths)]


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint64).view(np.int64)).to(dev)


def _tables(lengths, dev):
    lens = np.asarray(lengths, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    off4 = np.concatenate([[0], np.cumsum((lens // 4).astype(np.int64))])
    return torch.from_numpy(lens).to(dev), _i64(off, dev), _i64(off4, dev), off, off4


def _sentinel(n, dev):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _decode_ragged(m, z, lengths, dev, slack=64, max_L=None):
    """Raw entry over a sentinel-filled buffer -> (packed buffer with `slack` floats behind the rows, host offsets)."""
    ch = m.decoder.channels
    d_len, d_off, _, off, _ = _tables(lengths, dev)
    out = _sentinel(ch * int(off[-1]) + slack, dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_vae_decode_mc_ragged(m.decoder._handle(dev), z.data_ptr(), d_len.data_ptr(), d_off.data_ptr(),
                                                 out.data_ptr(), len(lengths), max_L or max(lengths), z.shape[2],
                                                 L.stream_ptr(dev)), "t2s_vae_decode_mc_ragged")
    torch.cuda.synchronize()
    return out, off


def _encode_ragged(m, rows, lengths, dev, slack=64, max_L=None):
    ch, W = m.encoder.channels, m.encoder._width()
    d_len, d_off, d_off4, off, off4 = _tables(lengths, dev)
    x = torch.cat([r.reshape(-1) for r in rows] + [torch.zeros(1, device=dev)])
    z = _sentinel(len(lengths) * 64 * W, dev).view(len(lengths), 64, W)
    before = _sentinel(64 * int(off4[-1]) + slack, dev)
    with torch.cuda.device(dev):
        L.check(L.lib().t2s_vae_encode_mc_ragged(m.encoder._handle(dev), x.data_ptr(), d_len.data_ptr(), d_off.data_ptr(),
                                                 d_off4.data_ptr(), z.data_ptr(), before.data_ptr(), len(lengths),
                                                 max_L or max(lengths), W, L.stream_ptr(dev)), "t2s_vae_encode_mc_ragged")
    torch.cuda.synchronize()
    return z, before, off4


def _is_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


@pytest.mark.parametrize("W", [8, 50, 64])
@pytest.mark.parametrize("ch", [3, 10])
def test_decode_rows_equal_the_uniform_entry(dev, ch, W):
    m = _model(ch, W, dev)
    z = synth.make_wide_latents(77 + W, len(LENGTHS), W).to(dev)
    out, off = _decode_ragged(m, z, LENGTHS, dev)
    with torch.no_grad():
        for b, Lb in enumerate(LENGTHS):
            got = out[ch * off[b]:ch * off[b + 1]].view(ch, Lb)
            if Lb:
                assert _same(got, m.decoder(z[b:b + 1], Lb)[0][0]), (b, Lb)
    assert _is_sentinel(out[ch * off[-1]:])                       # nothing behind the last span (the 0 row has no span)
    # the mirror returns the same rows
    rows = m.decoder.decode_ragged(z, LENGTHS)
    assert [tuple(r.shape) for r in rows] == [(ch, Lb) for Lb in LENGTHS]
    for b in range(len(LENGTHS)):
        assert _same(rows[b], out[ch * off[b]:ch * off[b + 1]].view(ch, LENGTHS[b]))


@pytest.mark.parametrize("W", [8, 50, 64])
@pytest.mark.parametrize("ch", [3, 10])
def test_encode_rows_equal_the_uniform_entry(dev, ch, W):
    m = _model(ch, W, dev)
    rows = _rows(ch, LENGTHS, dev)
    z, before, off4 = _encode_ragged(m, rows, LENGTHS, dev)
    with torch.no_grad():
        for b, Lb in enumerate(LENGTHS):
            if not Lb:
                assert _is_sentinel(z[b])                         # the skipped row's latent is untouched
                continue
            want_z, want_before = m.encoder(rows[b][None])
            assert _same(z[b], want_z[0]), (b, Lb)
            assert _same(before[64 * off4[b]:64 * off4[b + 1]].view(64, Lb // 4), want_before[0]), (b, Lb)
    assert _is_sentinel(before[64 * off4[-1]:])
    zm = m.encoder.encode_ragged(rows)
    keep = [b for b, Lb in enumerate(LENGTHS) if Lb]
    assert _same(zm[keep], z[keep]) and float(zm[LENGTHS.index(0)].abs().max()) == 0.0


@pytest.mark.parametrize("Ln", [36, 203])
@pytest.mark.parametrize("ch", [3, 10])
def test_equal_lengths_equal_the_uniform_launch(dev, ch, Ln):
    W, B = 50, 4
    m = _model(ch, W, dev)
    z = synth.make_wide_latents(9, B, W).to(dev)
    x = synth.make_mseries(9, B, ch, Ln).to(dev)
    out, off = _decode_ragged(m, z, [Ln] * B, dev)
    zr, before, off4 = _encode_ragged(m, list(x), [Ln] * B, dev)
    with torch.no_grad():
        assert _same(out[:ch * off[-1]].view(B, ch, Ln), m.decoder(z, Ln)[0])
        want_z, want_before = m.encoder(x)
        assert _same(zr, want_z) and _same(before[:64 * off4[-1]].view(B, 64, Ln // 4), want_before)


def test_permuting_the_rows_permutes_the_outputs(dev):
    ch, W = 10, 64
    m = _model(ch, W, dev)
    perm = [7, 2, 8, 0, 5, 3, 1, 6, 4]
    z = synth.make_wide_latents(31, len(LENGTHS), W).to(dev)
    rows = _rows(ch, LENGTHS, dev)
    out, off = _decode_ragged(m, z, LENGTHS, dev)
    enc, before, off4 = _encode_ragged(m, rows, LENGTHS, dev)
    lens_p = [LENGTHS[p] for p in perm]
    out_p, off_p = _decode_ragged(m, z[perm].contiguous(), lens_p, dev)
    enc_p, before_p, off4_p = _encode_ragged(m, [rows[p] for p in perm], lens_p, dev)
    for i, p in enumerate(perm):
        assert _same(out_p[ch * off_p[i]:ch * off_p[i + 1]], out[ch * off[p]:ch * off[p + 1]])
        assert _same(enc_p[i], enc[p])
        assert _same(before_p[64 * off4_p[i]:64 * off4_p[i + 1]], before[64 * off4[p]:64 * off4[p + 1]])


def test_rows_outside_the_range_are_skipped(dev):
    """A length of 5, one above max_L and a 0 row: their spans, their latents and everything behind keep the sentinel, and the
    valid rows between them are written as ever."""
    ch, W = 3, 8
    m = _model(ch, W, dev)
    lengths, max_L = [36, 5, 41, 150, 0, 11], 132
    z = synth.make_wide_latents(3, len(lengths), W).to(dev)
    rows = _rows(ch, lengths, dev)
    out, off = _decode_ragged(m, z, lengths, dev, max_L=max_L)
    enc, before, off4 = _encode_ragged(m, rows, lengths, dev, max_L=max_L)
    with torch.no_grad():
        for b, Lb in enumerate(lengths):
            span = out[ch * off[b]:ch * off[b + 1]]
            span4 = before[64 * off4[b]:64 * off4[b + 1]]
            if Lb in (36, 41, 11):
                want_z, want_before = m.encoder(rows[b][None])
                assert _same(span.view(ch, Lb), m.decoder(z[b:b + 1], Lb)[0][0])
                assert _same(enc[b], want_z[0]) and _same(span4.view(64, Lb // 4), want_before[0])
            else:
                assert _is_sentinel(span) and _is_sentinel(span4) and _is_sentinel(enc[b]), (b, Lb)
    assert _is_sentinel(out[ch * off[-1]:]) and _is_sentinel(before[64 * off4[-1]:])


def test_host_refusals(dev):
    """Each by its message, before any launch: the buffers keep their sentinel."""
    from model.pretrained.vqvae import vqvae as vqvae1
    ch, W = 3, 8
    m = _model(ch, W, dev)
    m1 = vqvae1(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
    m1.load_state_dict(synth.make_vae_state_dict(2025), strict=True)
    m1 = m1.to(dev).eval()
    lib, st = L.lib(), L.stream_ptr(dev)
    lengths = [36, 41]
    d_len, d_off, d_off4, off, off4 = _tables(lengths, dev)
    z = _sentinel(2 * 64 * W, dev)
    x = _sentinel(ch * 77, dev)
    rec = _sentinel(ch * 77, dev)
    before = _sentinel(64 * 19, dev)
    with torch.cuda.device(dev):
        hd, he = m.decoder._handle(dev), m.encoder._handle(dev)
        h1d, h1e = m1.decoder._handle(dev), m1.encoder._handle(dev)

        def dec(h=hd, zp=z.data_ptr(), lp=d_len.data_ptr(), op=d_off.data_ptr(), rp=rec.data_ptr(), B=2, max_L=41, w=W):
            return lib.t2s_vae_decode_mc_ragged(h, zp, lp, op, rp, B, max_L, w, st)

        def enc(h=he, xp=x.data_ptr(), lp=d_len.data_ptr(), op=d_off.data_ptr(), o4=d_off4.data_ptr(), zp=z.data_ptr(),
                bp=before.data_ptr(), B=2, max_L=41, w=W):
            return lib.t2s_vae_encode_mc_ragged(h, xp, lp, op, o4, zp, bp, B, max_L, w, st)

        def refused(rc, *words):
            msg = lib.t2s_last_error()
            assert rc == E_INVALID and all(w in msg for w in words), (rc, msg)

        for kw in ({"h": None}, {"zp": None}, {"lp": None}, {"op": None}, {"rp": None}):
            refused(dec(**kw), b"t2s_vae_decode_mc_ragged", b"NULL")
        for kw in ({"h": None}, {"xp": None}, {"lp": None}, {"op": None}, {"o4": None}, {"zp": None}):
            refused(enc(**kw), b"t2s_vae_encode_mc_ragged", b"NULL")
        refused(dec(h=h1d), b"t2s_vae_decode_mc_ragged", b"single-channel")
        refused(enc(h=h1e), b"t2s_vae_encode_mc_ragged", b"single-channel")
        refused(dec(max_L=7), b"L=7")
        refused(enc(max_L=7), b"L=7")
        refused(dec(max_L=(1 << 20) + 1), b"L=1048577")
        refused(dec(w=65), b"latent width 65")
        refused(enc(w=65), b"latent width 65")
        refused(enc(w=0), b"latent width 0")
        refused(dec(B=0), b"B=0")
        refused(enc(B=0), b"B=0")
        refused(enc(bp=None, max_L=132), b"max_L=132", b"before")      # tiled rows need `before`
    torch.cuda.synchronize()
    assert _is_sentinel(z) and _is_sentinel(rec) and _is_sentinel(before)
    # the mirrors refuse a single-channel codec themselves
    with pytest.raises(L.T2SError, match="single-channel"):
        m1.decoder.decode_ragged(torch.zeros(2, 64, 30, device=dev), lengths)
    with pytest.raises(L.T2SError, match="single-channel"):
        m1.encoder.encode_ragged([torch.zeros(1, 36, device=dev)])
