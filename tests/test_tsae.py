"""TSae codec on the GPU: t2s_tsae_encode / _decode / _generate through the C ABI and through the mirror
(model/pretrained/TSae.py) against the reference's recorded outputs (tests/golden/tsae.npz), at the bar
1e-5 * max(1, max|reference output|); the bitwise properties (repeat, batch independence, batch order), the workspace contract and
every refusal.

Measured on an MI355X (largest error / bar over the 17 cases): memory 0.30 (T 300; the positional divisors),
teacher-forced prediction 0.13, generation 0.12, decode(generate) against generate 0.05."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _tsae_fixture as FX
from _tsae_handle import DEV, Handle as _Handle
from t2ms_amd import _lib as L

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref, what):
    got = got.detach().cpu()
    err, b = float((got.double() - ref.double()).abs().max()), FX.bar(ref)
    print(f"{what}: max|err| {err:.3e} bar {b:.3e} ({err / b:.3f})")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and err <= b, (what, err, b)


def Handle(cfg, enc=True, dec=True, **override):
    """The shared handle (tests/_tsae_handle.py) on the configuration's seeded weights."""
    return _Handle(FX.golden()[1]["cfgs"][cfg], FX.state_dict(cfg), enc=enc, dec=dec, **override)


_handles = {}


def handle(cfg):
    if cfg not in _handles:
        _handles[cfg] = Handle(cfg)
        assert _handles[cfg].rc == 0, L.lib().t2s_last_error()
    return _handles[cfg]


def _err():
    return L.lib().t2s_last_error().decode()


@pytest.mark.parametrize("c", FX.cases(), ids=FX.case_ids())
def test_c_abi_matches_reference(c):
    h, x = handle(c["cfg"]), FX.case_input(c).to(DEV)
    memory = h.encode(x)
    _close(memory, FX.expected(c, "memory"), "memory")
    _close(h.decode(FX.expected(c, "memory").to(DEV), x), FX.expected(c, "pred"), "pred")
    gen = h.generate(memory)
    _close(gen, FX.expected(c, "gen"), "gen")
    # generate's own output as the teacher-forced target reproduces it: the cache computes what the full causal pass computes
    again = h.decode(memory, gen)
    _close(again, gen.cpu(), "decode(generate)")


@pytest.mark.parametrize("c", FX.cases(), ids=FX.case_ids())
def test_mirror_matches_reference(c, monkeypatch):
    monkeypatch.delenv("T2S_TSAE", raising=False)
    m, x = FX.mirror(c["cfg"], DEV), FX.case_input(c).to(DEV)
    with torch.no_grad():
        memory = m.encoder(x)
        _close(memory, FX.expected(c, "memory"), "memory")
        _close(m.decoder(FX.expected(c, "memory").to(DEV), x), FX.expected(c, "pred"), "pred")
        _close(m.forward_inference(x, None), FX.expected(c, "gen"), "gen")
    loss, recon = m.shared_eval(x, None, None, "test")
    _close(recon, FX.expected(c, "gen"), "shared_eval recon")
    want = float(FX.golden()[0][f"loss_{FX.case_key(c)}"])
    assert abs(float(loss) - want) <= 2e-5 * want, (float(loss), want)
    assert "_t2s_h" in m.encoder.__dict__ and "_t2s_h" in m.decoder.__dict__           # the HIP entries ran


def test_positional_table_matches_reference():
    """The library's table against the reference's buffer: pe[:, :8] and pe[:, 1999].  Bound: both form the angle p * w_i in
    fp32 from a divisor w_i = exp(.) that is correct to 1 ulp in either (relative 2^-23), so the angles differ by at most
    p * w_i * 2^-23, and sin / cos of them by that plus one rounding of the result (2^-24 each side)."""
    h, plan = handle("bp"), FX.golden()[1]
    pe = torch.empty(2000, 64, device=DEV)
    L.check(L.lib().t2s_tsae_positional(h.ptr, pe.data_ptr(), 0, 2000, L.stream_ptr(DEV)), "t2s_tsae_positional")
    pe = pe.cpu().double()
    w = torch.exp(torch.arange(0, 64, 2, dtype=torch.float64) * -(np.log(10000.0) / 64)).repeat_interleave(2)
    for rows, want in ((slice(0, 8), torch.tensor(plan["pe_head"])), (slice(1999, 2000), torch.tensor(plan["pe_last"]).unsqueeze(0))):
        p = torch.arange(2000, dtype=torch.float64)[rows].unsqueeze(1)
        bound = p * w * 2.0 ** -23 + 2.0 ** -23
        err = (pe[rows] - want).abs()
        print(f"pe rows {rows}: max err {float(err.max()):.3e}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("cfg,T", [("bp", 65), ("bp", 144), ("h4", 37)])
def test_bitwise_properties(cfg, T):
    """A call repeats bit for bit; a series' rows do not depend on the batch it sits in, nor on its place in it."""
    c = dict(cfg=cfg, T=T, B=3)
    h, x = handle(cfg), FX.case_input(c).to(DEV)
    memory, gen = h.encode(x), None
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


def test_workspace_contract():
    c = dict(cfg="bp", T=37, B=3)
    h, x = handle("bp"), FX.case_input(c).to(DEV)
    need = int(L.lib().t2s_tsae_workspace_bytes(h.ptr, 3, 37))
    assert need == 3 * 37 * 4 * max(256, 320 + 128 * 3, 256 * 3)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    memory = h.encode(x)
    sentinel = 12345.0
    for name, tensors in (("t2s_tsae_encode", [x, torch.full((3, 37, 64), sentinel, device=DEV)]),
                          ("t2s_tsae_decode", [memory, x, torch.full((3, 37, 10), sentinel, device=DEV)]),
                          ("t2s_tsae_generate", [memory, torch.full((3, 37, 10), sentinel, device=DEV)])):
        assert h.call(name, tensors, 3, 37, ws=ws, ws_bytes=need - 1) == -1, name
        assert "workspace" in _err() and str(need) in _err()
        torch.cuda.synchronize()
        assert bool((tensors[-1] == sentinel).all()), name                      # refused before any launch
        assert h.call(name, tensors, 3, 37, ws=ws, ws_bytes=need) == 0, (name, _err())   # exactly the stated size is enough
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tensors[-1]).all()) and not bool((tensors[-1] == sentinel).any()), name


def test_refusals_leave_outputs_untouched():
    h = handle("bp")
    x, memory = torch.rand(2, 8, 10, device=DEV), torch.rand(2, 8, 64, device=DEV)
    out64, out10 = torch.full((2, 8, 64), 7.0, device=DEV), torch.full((2, 8, 10), 7.0, device=DEV)
    entries = (("t2s_tsae_encode", [x, out64]), ("t2s_tsae_decode", [memory, x, out10]), ("t2s_tsae_generate", [memory, out10]))
    for name, tensors in entries:
        for B, T, word in ((2, 0, "T=0"), (2, 2001, "T=2001"), (0, 8, "B=0")):
            assert h.call(name, tensors, B, T) == -1, (name, B, T)
            assert word in _err(), (_err(), word)
        for i in range(len(tensors)):                                            # each NULL tensor
            holed = list(tensors)
            holed[i] = None
            assert h.call(name, holed, 2, 8) == -1 and "NULL" in _err(), (name, i)
        assert h.call(name, tensors, 2, 8, ws=False, ws_bytes=1 << 30) == -1 and "NULL" in _err()
        assert h.call(name, tensors, 2, 8, ptr=C.c_void_p()) == -1 and "NULL" in _err()   # NULL handle
    torch.cuda.synchronize()
    assert bool((out64 == 7.0).all()) and bool((out10 == 7.0).all())
    assert int(L.lib().t2s_tsae_workspace_bytes(h.ptr, 1, 2001)) == 0 and int(L.lib().t2s_tsae_workspace_bytes(None, 1, 8)) == 0


def test_one_sided_handles():
    enc, dec = Handle("h4", dec=False), Handle("h4", enc=False)
    try:
        assert enc.rc == 0 and dec.rc == 0, _err()
        c = dict(cfg="h4", T=8, B=2)
        x = FX.case_input(c).to(DEV)
        memory = enc.encode(x)
        _close(memory, FX.expected(c, "memory"), "memory")
        _close(dec.generate(memory), FX.expected(c, "gen"), "gen")
        out10, out64 = torch.full((2, 8, 10), 7.0, device=DEV), torch.full((2, 8, 64), 7.0, device=DEV)
        assert enc.call("t2s_tsae_generate", [memory, out10], 2, 8) == -1 and "without a decoder" in _err()
        assert enc.call("t2s_tsae_decode", [memory, x, out10], 2, 8) == -1 and "without a decoder" in _err()
        assert dec.call("t2s_tsae_encode", [x, out64], 2, 8) == -1 and "without an encoder" in _err()
        torch.cuda.synchronize()
        assert bool((out10 == 7.0).all()) and bool((out64 == 7.0).all())
    finally:
        enc.close()
        dec.close()


@pytest.mark.parametrize("field,value,word", [("d_model", 128, "d_model=128"), ("heads", 2, "heads=2"), ("d_ff", 96, "d_ff=96"),
                                              ("d_ff", 576, "d_ff=576"), ("n_features", 17, "n_features=17"),
                                              ("n_features", 0, "n_features=0")])
def test_create_refuses_uncovered_shapes(field, value, word):
    h = Handle("bp", **{field: value})
    assert h.rc == -1 and not h.ptr and word in _err(), _err()


def test_create_refuses_layer_counts_and_null():
    for enc, dec, word in ((7, 3, "n_enc=7"), (3, 7, "n_dec=7"), (0, 0, "n_enc=0 and n_dec=0")):
        h = Handle("bp")
        h.close()
        h.w.n_enc, h.w.n_dec = enc, dec
        p = C.c_void_p()
        assert L.lib().t2s_tsae_create(C.byref(h.w), C.byref(p)) == -1 and word in _err(), _err()
    h = Handle("bp")
    h.close()
    h.w.dec[1].norm3_w = None
    p = C.c_void_p()
    assert L.lib().t2s_tsae_create(C.byref(h.w), C.byref(p)) == -1 and "norm3" in _err() and "NULL" in _err(), _err()


def test_switch_and_default_route_agree(monkeypatch):
    c = dict(cfg="bp", T=37, B=3)
    m, x = FX.mirror("bp", DEV), FX.case_input(c).to(DEV)
    with torch.no_grad():
        monkeypatch.delenv("T2S_TSAE", raising=False)
        hip = (m.encoder(x), m.decoder(FX.expected(c, "memory").to(DEV), x), m.forward_inference(x, None))
        monkeypatch.setenv("T2S_TSAE", "torch")
        m.encoder.__dict__.pop("_t2s_h")                                         # a torch-route call builds no handle
        tor = (m.encoder(x), m.decoder(FX.expected(c, "memory").to(DEV), x), m.forward_inference(x, None))
        assert "_t2s_h" not in m.encoder.__dict__
    for name, a, b in zip(("memory", "pred", "gen"), hip, tor):
        _close(a, b.cpu(), f"hip vs torch {name}")
        _close(b, FX.expected(c, name), f"torch route {name}")


def test_long_series_runs():
    """T = 2000, the table's last row: every index stays in range and the cached generation agrees with the full causal pass."""
    h = handle("h4")
    x = torch.rand(1, 2000, 10, device=DEV)
    memory = h.encode(x)
    gen = h.generate(memory)
    assert bool(torch.isfinite(memory).all()) and bool(torch.isfinite(gen).all())
    _close(h.decode(memory, gen), gen.cpu(), "decode(generate) T=2000")


def test_reconstruct_tool(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tsae_reconstruct.py"), "--random_init", "1", "--synthetic", "4",
                        "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(report["groups"]) == {"synthetic_L36", "synthetic_L144"}
    for name, g in report["groups"].items():
        rec = np.load(tmp_path / f"{name}_recon.npy")
        assert rec.shape == (4, 10, g["length"]) and np.isfinite(rec).all() and g["finite"] and np.isfinite(g["mse"])
