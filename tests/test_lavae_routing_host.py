"""Host-side logic of the LA-VAE codec mirror that both families share (t2ms_amd/model/pretrained/_lavae.py, no GPU): the
routing between the three forwards, the switches, the single-channel limits of the coverage predicate and the question the
Sampler asks a decoder."""
import itertools
import types

import pytest

from t2ms_amd import _lib as L
from t2ms_amd.model.pretrained import _lavae

# (g, p, i, c, t) -> route, written out per case: g grad enabled, p a parameter requires grad, i the input requires grad,
# c the shape is covered, t torch is forced.  Every combination that is not listed is "hip": nobody wants a gradient.
T, F = True, False
SINGLE_ENCODER = {            # wants = g and p (the input is not consulted: the kept oddity); "fn" if c and not i and not t
    (T, T, F, F, F): "autograd", (T, T, F, F, T): "autograd", (T, T, F, T, F): "fn", (T, T, F, T, T): "autograd",
    (T, T, T, F, F): "autograd", (T, T, T, F, T): "autograd", (T, T, T, T, F): "autograd", (T, T, T, T, T): "autograd",
}
MULTI_ENCODER = {             # wants = g and (p or i); "fn" if c and not i and not t
    **SINGLE_ENCODER,
    (T, F, T, F, F): "autograd", (T, F, T, F, T): "autograd", (T, F, T, T, F): "autograd", (T, F, T, T, T): "autograd",
}
DECODER = {                   # either family: wants = g and (p or i); "fn" if c and not t
    (T, T, F, F, F): "autograd", (T, T, F, F, T): "autograd", (T, T, F, T, F): "fn", (T, T, F, T, T): "autograd",
    (T, T, T, F, F): "autograd", (T, T, T, F, T): "autograd", (T, T, T, T, F): "fn", (T, T, T, T, T): "autograd",
    (T, F, T, F, F): "autograd", (T, F, T, F, T): "autograd", (T, F, T, T, F): "fn", (T, F, T, T, T): "autograd",
}
TABLE = {("encoder", False): SINGLE_ENCODER, ("encoder", True): MULTI_ENCODER, ("decoder", False): DECODER, ("decoder", True): DECODER}


@pytest.mark.parametrize("direction,multichannel", list(TABLE))
def test_routing_table(direction, multichannel):
    want = TABLE[direction, multichannel]
    cases = list(itertools.product((False, True), repeat=5))
    assert len(cases) == 32 and set(want) <= set(cases)
    for case in cases:
        assert _lavae._route(direction, multichannel, *case) == want.get(case, "hip"), (direction, multichannel, case)


def test_the_single_channel_encoder_ignores_a_series_that_requires_grad():
    """The oddity the table keeps: frozen parameters, a series that requires grad -> no graph; the other three build one."""
    assert _lavae._route("encoder", False, True, False, True, True, False) == "hip"
    assert _lavae._route("encoder", True, True, False, True, True, False) == "autograd"
    assert _lavae._route("decoder", False, True, False, True, True, False) == "fn"
    assert _lavae._route("decoder", True, True, False, True, True, False) == "fn"


def test_single_channel_switches(monkeypatch):
    names = {"encoder": "T2S_ENCODER_TORCH_AUTOGRAD", "decoder": "T2S_DECODER_TORCH_AUTOGRAD"}
    for name in (*names.values(), "T2S_MVAE_BACKWARD"):
        monkeypatch.delenv(name, raising=False)
    for direction, other in (("encoder", "decoder"), ("decoder", "encoder")):
        assert _lavae._torch_forced(direction, False) is False                  # unset
        for value, want in (("1", True), ("", False), ("0", False)):
            monkeypatch.setenv(names[direction], value)
            assert _lavae._torch_forced(direction, False) is want, (direction, value)
            assert _lavae._torch_forced(other, False) is False                  # its own direction only
            assert _lavae._torch_forced(direction, True) is False and _lavae._torch_forced(other, True) is False
        monkeypatch.delenv(names[direction])
    monkeypatch.setenv("T2S_MVAE_BACKWARD", "torch")                            # the other family's switch
    assert _lavae._torch_forced("encoder", False) is False and _lavae._torch_forced("decoder", False) is False


def test_multichannel_switch(monkeypatch):
    for name in ("T2S_ENCODER_TORCH_AUTOGRAD", "T2S_DECODER_TORCH_AUTOGRAD"):
        monkeypatch.setenv(name, "1")                                           # the other family's switches
    monkeypatch.delenv("T2S_MVAE_BACKWARD", raising=False)
    for direction in ("encoder", "decoder"):
        assert _lavae._torch_forced(direction, True) is False                   # unset
        for value, want in (("torch", True), ("", False), ("hip", False)):
            monkeypatch.setenv("T2S_MVAE_BACKWARD", value)
            assert _lavae._torch_forced(direction, True) is want, (direction, value)
        monkeypatch.setenv("T2S_MVAE_BACKWARD", "fast")
        with pytest.raises(L.T2SError, match="T2S_MVAE_BACKWARD"):
            _lavae._torch_forced(direction, True)
        monkeypatch.delenv("T2S_MVAE_BACKWARD")


def _single(**kw):
    from model.pretrained.vqvae import vqvae
    return vqvae(types.SimpleNamespace(**{**dict(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64),
                                          **kw}))


def test_single_channel_limits_of_the_predicate():
    m = _single()
    assert [m.encoder._hip_backward_ok(Ln) for Ln in (8, 24, 96, 128)] == [True] * 4
    assert [m.encoder._hip_backward_ok(Ln) for Ln in (4, 26, 132, 192)] == [False] * 4
    assert [m.decoder._hip_backward_ok(96, W) for W in (1, 24, 30, 32)] == [True] * 4
    assert m.decoder._hip_backward_ok(96, 33) is False
    for other in (_single(num_residual_layers=0), _single(block_hidden_size=64)):
        assert not any(other.encoder._hip_backward_ok(Ln) for Ln in (4, 8, 24, 26, 96, 128, 132, 192))
        assert not any(other.decoder._hip_backward_ok(96, W) for W in (1, 24, 30, 32, 33))


def test_channels_is_what_the_sampler_asks():
    from model.pretrained import myvqvae, vqvae
    assert vqvae.Decoder(64, 128, 2, 256).channels is None and vqvae.Encoder(1, 128, 2, 256, 64).channels is None
    assert myvqvae.Decoder(64, 128, 2, 256, out_channels=7).channels == 7
    assert myvqvae.Encoder(7, 128, 2, 256, 64, 50).channels == 7
