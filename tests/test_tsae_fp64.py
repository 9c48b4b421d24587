"""TSae kernels (csrc/t2s_tsae.hip) against the fp64 restatement (tests/_tsae_ref.py) over the kernels' own configuration space:
the case table of tests/_tsae_cases.py -- every d_ff chunking of tsae_ffn_kernel, 1..6 layers a side, 4 and 8 heads, F = 1, 5 and
16, the row-tile and key-chunk edges of T up to 2000 -- on weights whose softmax is peaked (q and k rows x 4), so the
online-softmax rescale of tsae_attn_kernel and the running softmax and merge of gen_attn carry the result.
tests/test_tsae_host.py holds the same cases' inputs to the conditioning and stress gates on the CPU.

The restatement runs on the LIBRARY's positional table (t2s_tsae_positional, cast to fp64): the table has its own test and bound
(test_tsae.py::test_positional_table_matches_reference), and a 1-ulp divisor difference would otherwise move the angle at position
2000 by 2.4e-4.  Bar, unchanged: 1e-5 * max(1, max|fp64 output|).  Every comparison prints a TSAEERR line (kernel error and the
fp32 restatement's error in units of the bar, largest |output|); profiles/tsae_errors.md holds a run's figures.

Measured on an MI355X (largest kernel error / bar over the 22 cases and the mirror's): memory 0.108 and teacher-forced prediction
0.122 (both T = 2000), generation 0.119, decode(generate) against generate 0.088; the fp32 restatement's own error on the same
inputs is at most 0.103.  No bar was moved.  Checked against nine arithmetic-only mutants of the kernels (a dropped rescale, a
softmax factor cut off below exp(-4), a tail-chunk bias from the wrong offset, ...): each fails here, four of them fail nothing
in tests/test_tsae.py (profiles/tsae_errors.md)."""
import ctypes as C
import functools
import types

import pytest
import torch

import _tsae_cases as TC
import _tsae_ref as R
from _tsae_handle import DEV, Handle
from t2ms_amd import _lib as L

pytestmark = pytest.mark.gpu
PATTERN, TAIL = 0xA5, 64 * 1024

_handles = {}


def handle(c, enc=True, dec=True):
    key = (c, enc, dec)
    if key not in _handles:
        k = dict(n_features=c.n_features, d_ff=c.d_ff, heads=c.heads, n_enc=c.n_enc, n_dec=c.n_dec)
        _handles[key] = Handle(k, TC.state_dict(c), enc=enc, dec=dec)
        assert _handles[key].rc == 0, L.lib().t2s_last_error()
    return _handles[key]


@functools.lru_cache(maxsize=None)
def table():
    """The library's positional table (a function of position and channel alone: any handle's), fp64 on the CPU."""
    return handle(TC.TABLE[0]).positional().double()


def _hold(c, entry, got, ref64, ref32, failures):
    """One TSAEERR line; a miss of the bar is collected, so a case prints all its figures before it fails."""
    got, b = got.detach().cpu(), TC.bar(ref64)
    err = float((got.double() - ref64.double()).abs().max())
    own = float((ref32.double() - ref64.double()).abs().max()) / b if ref32 is not None else float("nan")
    print(f"TSAEERR case={TC.case_id(c)} entry={entry} kernel={err / b:.3f} fp32={own:.3f} max={float(ref64.abs().max()):.3f}")
    if not (got.shape == ref64.shape and bool(torch.isfinite(got).all()) and err <= b):
        failures.append((entry, err, b))


@functools.lru_cache(maxsize=None)
def _teacher_forced(c):
    """(memory64, memory32, memory fed to decode, pred64, pred32) of the two restatements on the library's table."""
    x, pe = TC.series(c), table()
    sd64, sd32 = TC.state_dict_as(c, torch.float64), TC.state_dict(c)
    m64, m32 = R.encode(sd64, x, c.heads, pe=pe), R.encode(sd32, x, c.heads, pe=pe.float())
    fed = m64.float()                         # the kernel and both restatements decode from the same fp32 values
    return m64, m32, fed, R.decode(sd64, fed, x, c.heads, pe=pe), R.decode(sd32, fed, x, c.heads, pe=pe.float())


def _generated(c, memory):
    """Generation of the two restatements from the KERNEL's memory."""
    pe = table()
    return (R.generate(TC.state_dict_as(c, torch.float64), memory, c.heads, pe=pe),
            R.generate(TC.state_dict(c), memory, c.heads, pe=pe.float()))


@pytest.mark.parametrize("c", TC.TABLE, ids=TC.IDS)
def test_kernels_match_fp64_restatement(c):
    h, x = handle(c), TC.series(c).to(DEV)
    m64, m32, fed, p64, p32 = _teacher_forced(c)
    failures = []
    memory = h.encode(x)
    _hold(c, "memory", memory, m64, m32, failures)
    _hold(c, "pred", h.decode(fed.to(DEV), x), p64, p32, failures)
    gen = h.generate(memory)
    g64, g32 = _generated(c, memory.cpu())
    _hold(c, "gen", gen, g64, g32, failures)
    # generate's own output as the teacher-forced target reproduces it: the cache computes what the full causal pass computes
    _hold(c, "decode(gen)", h.decode(memory, gen), gen.cpu(), None, failures)
    assert not failures, failures


def _patterned(n_bytes):
    """(a device buffer of n_bytes + TAIL bytes, all PATTERN; its first n_bytes as fp32)."""
    buf = torch.full((n_bytes + TAIL,), PATTERN, dtype=torch.uint8, device=DEV)
    return buf, buf[:n_bytes].view(torch.float32)


def _tail_untouched(buf, n_bytes):
    return bool((buf[n_bytes:] == PATTERN).all())


F1, F5, SIX = TC.TABLE[10], TC.TABLE[11], TC.TABLE[7]


@pytest.mark.parametrize("c,enc,dec,floats_per_row", [(F1, True, False, 320), (F1, True, True, 448), (F5, True, True, 768),
                                                       (SIX, True, True, 1536)],
                         ids=["encoder_only", "n_dec1_F1", "n_dec3_F5", "n_dec6"])
def test_calls_stay_inside_workspace_and_outputs(c, enc, dec, floats_per_row):
    """Each entry with ws_bytes = the stated size exactly, the workspace and every output followed by 64 KiB of a byte pattern:
    the tails stay untouched and the results are bitwise those of an ordinary call.  The stated size is
    B * T * 4 * max(256, 320 + 128 n_dec, 256 n_dec); a handle without a decoder states 320 floats per row (its encode uses the
    first 256), n_dec = 1 the decode branch, n_dec >= 3 the generate branch."""
    assert (F1.n_features, F1.n_dec, F5.n_features, F5.n_dec, SIX.n_dec) == (1, 1, 5, 3, 6)
    h, x = handle(c, enc, dec), TC.series(c).to(DEV)
    B, T, F = c.B, c.T, c.n_features
    n_dec = c.n_dec if dec else 0
    need = int(L.lib().t2s_tsae_workspace_bytes(h.ptr, B, T))
    assert need == B * T * 4 * max(256, 320 + 128 * n_dec, 256 * n_dec) == B * T * 4 * floats_per_row
    ws, _ = _patterned(need)
    memory = h.encode(x)
    calls = [("t2s_tsae_encode", [x], 64, memory)]
    if dec:
        calls += [("t2s_tsae_decode", [memory, x], F, h.decode(memory, x)), ("t2s_tsae_generate", [memory], F, h.generate(memory))]
    for name, inputs, width, want in calls:
        n_out = B * T * width * 4
        out_buf, out = _patterned(n_out)
        assert h.call(name, inputs + [out], B, T, ws=ws, ws_bytes=need) == 0, (name, L.lib().t2s_last_error())
        torch.cuda.synchronize()
        assert _tail_untouched(out_buf, n_out), f"{name} wrote past its output"
        assert _tail_untouched(ws, need), f"{name} wrote past the stated workspace"
        assert torch.equal(out.view(B, T, width), want), name


def test_bitwise_properties_peaked():
    """d_ff 192 (a 64-column tail chunk), 2 + 1 layers, T = 129 (a fifth row tile of one row, a third key chunk of one key),
    B = 3, gain 4: a call repeats bit for bit; a series does not depend on the batch it sits in, nor on its place in it."""
    c = TC.TABLE[3]
    assert (c.d_ff, c.n_enc, c.n_dec, c.T, c.B, c.gain) == (192, 2, 1, 129, 3, 4.0)
    h, x = handle(c), TC.series(c).to(DEV)
    memory = h.encode(x)
    pred, gen = h.decode(memory, x), h.generate(memory)
    for name, first, again in (("encode", memory, h.encode(x)), ("decode", pred, h.decode(memory, x)), ("generate", gen, h.generate(memory))):
        assert torch.equal(first, again), name
    one = x[1:2].contiguous()
    m1 = h.encode(one)
    assert torch.equal(m1[0], memory[1])
    assert torch.equal(h.decode(m1, one)[0], pred[1])
    assert torch.equal(h.generate(m1)[0], gen[1])
    xr = x.flip(0).contiguous()
    mr = h.encode(xr)
    assert torch.equal(mr.flip(0), memory)
    assert torch.equal(h.decode(mr, xr).flip(0), pred)
    assert torch.equal(h.generate(mr).flip(0), gen)


def test_mirror_matches_fp64_restatement(monkeypatch):
    """model/pretrained/TSae.py at 6 + 6 layers, d_ff 512, F 16, T 65 on the HIP route: encoder, teacher-forced decoder and
    forward_inference against the same fp64 values the C ABI is held to."""
    from model.pretrained.TSae import AttentionSeq2SeqAutoencoder
    monkeypatch.delenv("T2S_TSAE", raising=False)
    c = TC.MIRROR
    assert (c.n_enc, c.n_dec, c.d_ff, c.n_features, c.T) == (6, 6, 512, 16, 65)
    m = AttentionSeq2SeqAutoencoder(types.SimpleNamespace(input_dim=c.n_features, flow_dim=64, num_encoder_layers=c.n_enc,
                                                          num_decoder_layers=c.n_dec, d_ff=c.d_ff, num_heads=c.heads))
    missing, unexpected = m.load_state_dict(TC.state_dict(c), strict=False)
    assert not unexpected and all(k.startswith("condition_fusion.") for k in missing), (missing, unexpected)
    m.condition_fusion = None
    m = m.to(DEV).eval()
    x = TC.series(c).to(DEV)
    m64, m32, fed, p64, p32 = _teacher_forced(c)
    failures = []
    with torch.no_grad():
        memory = m.encoder(x)
        _hold(c, "mirror memory", memory, m64, m32, failures)
        _hold(c, "mirror pred", m.decoder(fed.to(DEV), x), p64, p32, failures)
        g64, g32 = _generated(c, memory.cpu())
        _hold(c, "mirror gen", m.forward_inference(x, None), g64, g32, failures)
    assert "_t2s_h" in m.encoder.__dict__ and "_t2s_h" in m.decoder.__dict__           # the HIP entries ran
    assert isinstance(m.encoder.__dict__["_t2s_h"].ptr, C.c_void_p) and m.encoder.__dict__["_t2s_h"].ptr
    assert not failures, failures
