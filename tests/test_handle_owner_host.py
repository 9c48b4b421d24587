"""Host-side policy of the mirrors' handle ownership (t2ms_amd/_handle.py, no GPU): when a cached handle is served, refreshed or
rebuilt, what a failed build leaves behind, what a pickle drops, and the grow-only workspace.  CPU tensors; the build, refresh
and close callables are fakes that record their calls."""
import contextlib
import copy
import ctypes as C
import pickle
import types

import pytest
import torch
import torch.nn as nn

from t2ms_amd import _handle as H
from t2ms_amd import _lib as L

CPU = torch.device("cpu")


class FakeHandle:
    def __init__(self, log, n):
        self.log, self.n = log, n

    def close(self):
        self.log.append(("close", self.n))


class Owner(H.HandleOwner, nn.Module):
    """A mirror in miniature: geometry = device + shapes, stamp = stamp_of the parameters."""

    def __init__(self, refreshable=True, fail_build=()):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self.__dict__["log"], self.__dict__["fail_build"], self.__dict__["refreshable"] = [], set(fail_build), refreshable

    def _build(self, tag):
        assert tag == "args"
        n = sum(1 for e in self.log if e[0] in ("build", "build-raises")) + 1
        if n in self.fail_build:
            self.log.append(("build-raises", n))
            raise L.T2SError(f"build {n} refused")
        self.log.append(("build", n))
        return FakeHandle(self.log, n)

    def _refresh(self, h, tag):
        assert tag == "args"
        self.log.append(("refresh", h.n))
        return ["sources of refresh", len(self.log)]

    def handle(self, extra=None):
        ts = list(self.parameters())
        geometry = (CPU, extra) + tuple(tuple(t.shape) for t in ts)
        return self._owned_handle(CPU, geometry, H.stamp_of(ts), self._build, self._refresh if self.refreshable else None, "args")


def test_stamp_of():
    a, b = torch.zeros(3), torch.zeros(2, 2)
    s = H.stamp_of([a, b])
    assert s == ((a.data_ptr(), a._version), (b.data_ptr(), b._version)) and H.stamp_of([a, b]) == s
    a.add_(1)
    assert H.stamp_of([a, b]) != s and H.stamp_of([a, b])[1] == s[1]
    with torch.inference_mode():
        c = torch.zeros(3)
    assert H.stamp_of([a, c]) is None and H.stamp_of([c, a]) is None and H.stamp_of([]) == ()

    def no_storage():
        raise RuntimeError("Cannot access data pointer of Tensor that doesn't have storage")

    odd = types.SimpleNamespace(data_ptr=no_storage, is_inference=lambda: False)
    with pytest.raises(RuntimeError, match="doesn't have storage"):          # not an inference tensor: not "never cache"
        H.stamp_of([a, odd])


def test_cached_needs_the_device_and_a_standing_stamp():
    o = types.SimpleNamespace()
    assert H.cached(o, "_k", CPU, (1,)) is None
    o.__dict__["_k"] = (CPU, (1,), "value")
    assert H.cached(o, "_k", CPU, (1,)) == "value"
    assert H.cached(o, "_k", CPU, (2,)) is None and H.cached(o, "_k", torch.device("meta"), (1,)) is None
    assert H.cached(o, "_k", CPU, None) is None          # inference tensors: never from the cache
    o.__dict__["_k"] = (CPU, None, "value")
    assert H.cached(o, "_k", CPU, None) is None


def test_first_call_builds_once_and_an_unchanged_owner_is_served_from_the_cache():
    o = Owner()
    h = o.handle()
    assert o.log == [("build", 1)] and o.__dict__["_t2s_h"] is h
    assert o.handle() is h and o.handle() is h and o.log == [("build", 1)]


def test_in_place_write_refreshes_and_keeps_the_handle():
    o = Owner()
    h = o.handle()
    with torch.no_grad():
        o.lin.weight.add_(1.0)
    assert o.handle() is h and o.log == [("build", 1), ("refresh", 1)]
    assert h.keep == ["sources of refresh", 2]          # the sources live on the handle until the next refresh
    assert o.handle() is h and o.log == [("build", 1), ("refresh", 1)]          # the new stamp was stored


def test_without_a_refresh_callable_an_in_place_write_rebuilds_closing_first():
    o = Owner(refreshable=False)
    h = o.handle()
    with torch.no_grad():
        o.lin.bias.zero_()
    h2 = o.handle()
    assert h2 is not h and o.log == [("build", 1), ("close", 1), ("build", 2)]          # closed once, before the build
    assert o.handle() is h2 and len(o.log) == 3


def test_reallocated_parameter_of_the_same_shape_refreshes():
    o = Owner()
    h = o.handle()
    old = o.lin.weight                                   # (held: the new storage cannot take the old one's address)
    o.lin.weight = nn.Parameter(torch.ones(2, 3))
    assert o.lin.weight.data_ptr() != old.data_ptr()
    assert o.handle() is h and o.log == [("build", 1), ("refresh", 1)]


@pytest.mark.parametrize("refreshable", [True, False])
def test_changed_shape_or_geometry_key_rebuilds(refreshable):
    o = Owner(refreshable=refreshable)
    h = o.handle()
    o.lin.weight = nn.Parameter(torch.ones(4, 3))
    h2 = o.handle()
    assert h2 is not h and o.log == [("build", 1), ("close", 1), ("build", 2)]
    h3 = o.handle(extra="a larger capacity")
    assert h3 is not h2 and o.log[3:] == [("close", 2), ("build", 3)]
    assert o.handle(extra="a larger capacity") is h3 and len(o.log) == 5


def test_inference_mode_parameters_are_never_served_from_the_cache():
    with torch.inference_mode():
        o, p = Owner(), Owner(refreshable=False)
    assert H.stamp_of(list(o.parameters())) is None
    h = o.handle()
    assert o.handle() is h and o.handle() is h and o.log == [("build", 1), ("refresh", 1), ("refresh", 1)]
    p.handle(), p.handle(), p.handle()
    assert p.log == [("build", 1), ("close", 1), ("build", 2), ("close", 2), ("build", 3)]


@pytest.mark.parametrize("refreshable", [True, False])
def test_a_build_that_raises_leaves_no_handle_behind(refreshable):
    """The old handle is closed before the new one is built (the free precedes the allocation), so a failed build must not
    leave the closed handle where the next call would find it and hand its freed pointer to the library."""
    o = Owner(refreshable=refreshable, fail_build={2})
    h = o.handle()
    with pytest.raises(L.T2SError, match="build 2 refused"):
        o.handle(extra="grow")
    assert "_t2s_h" not in o.__dict__ and "_t2s_stamp" not in o.__dict__
    assert o.log == [("build", 1), ("close", 1), ("build-raises", 2)]          # closed exactly once
    h3 = o.handle()                                      # the geometry the closed handle had: built again, not served
    assert h3 is not h and o.log[3:] == [("build", 3)] and o.__dict__["_t2s_h"] is h3
    assert o.handle() is h3 and len(o.log) == 4


def test_a_first_build_that_raises_is_tried_again():
    o = Owner(fail_build={1})
    with pytest.raises(L.T2SError):
        o.handle()
    assert "_t2s_h" not in o.__dict__ and o.handle().n == 2 and o.log == [("build-raises", 1), ("build", 2)]


# the keys each mirror drops from a pickle: this process's device state.  The settings stay.
OWNER_KEYS = ("_t2s_h", "_t2s_geom", "_t2s_stamp", "_t2s_ws")
DIT_KEYS = OWNER_KEYS + ("_t2s_math_applied", "_t2s_bucket", "_t2s_flat_grad", "_t2s_fwd_gen", "_t2s_wstruct", "_t2s_pair",
                         "_t2s_pairing")


def _mirrors():
    from model.denoiser.transformer import Transformer
    from model.pretrained.vqvae import Encoder
    from t2ms_amd.model.pretrained.tsae import TimeSeriesDecoder
    return [(Transformer(), DIT_KEYS), (Encoder(1, 128, 2, 256, 64), OWNER_KEYS),
            (TimeSeriesDecoder(4, num_layers=1, d_ff=64, num_heads=4, flow_dim=64), OWNER_KEYS)]


def test_getstate_drops_the_transient_keys_and_keeps_the_settings():
    for m, transient in _mirrors():
        assert set(m._t2s_transient) == set(transient), type(m)
        for k in transient:
            m.__dict__[k] = "device state"
        m.__dict__["_t2s_math"], m.__dict__["_t2s_train_dtype"] = "bf16x3", "bf16"
        before = dict(m.__dict__)
        state = m.__getstate__()
        assert not set(transient) & set(state), type(m)
        assert set(state) == set(before) - set(transient), type(m)
        assert state["_t2s_math"] == "bf16x3" and state["_t2s_train_dtype"] == "bf16"
        assert m.__dict__ == before                      # the live object keeps its handle
        back = pickle.loads(pickle.dumps(m))
        assert not set(transient) & set(back.__dict__) and back.__dict__["_t2s_math"] == "bf16x3"
        assert [k for k, _ in back.state_dict().items()] == [k for k, _ in m.state_dict().items()]


def test_deepcopy_does_not_share_the_handle():
    o = Owner()
    h = o.handle()
    twin = copy.deepcopy(o)
    assert "_t2s_h" not in twin.__dict__ and "_t2s_stamp" not in twin.__dict__ and o.__dict__["_t2s_h"] is h
    twin.__dict__["log"] = []
    assert twin.handle() is not h and twin.log == [("build", 1)] and o.log == [("build", 1)]


def test_workspace_grows_never_shrinks_and_follows_the_device():
    calls = []

    def alloc(n, dtype, device):
        calls.append((n, str(device)))
        return torch.empty(n, dtype=dtype, device=device)

    o = types.SimpleNamespace()
    ws = H.HandleOwner._workspace(o, 100, CPU, alloc)
    assert ws.dtype == torch.uint8 and ws.numel() == 100 and ws.device == CPU and o.__dict__["_t2s_ws"] is ws
    assert H.HandleOwner._workspace(o, 100, CPU, alloc) is ws and H.HandleOwner._workspace(o, 7, CPU, alloc) is ws
    assert calls == [(100, "cpu")]                       # large enough: the same tensor, no allocation
    big = H.HandleOwner._workspace(o, 101, CPU, alloc)
    assert big is not ws and big.numel() == 101 and calls == [(100, "cpu"), (101, "cpu")]
    assert H.HandleOwner._workspace(o, 50, CPU, alloc) is big and len(calls) == 2
    other = H.HandleOwner._workspace(o, 10, torch.device("meta"), alloc)          # a device change reallocates
    assert other.device.type == "meta" and other.numel() == 10 and calls[2:] == [(10, "meta")]
    assert H.HandleOwner._workspace(o, 10, torch.device("meta"), alloc) is other and len(calls) == 3


def test_workspace_asked_for_without_a_device_index_stays_grow_only():
    """A tensor's device always carries an index, a caller's "cuda" does not: that is the same device, not a change."""
    calls = []

    def alloc(n, dtype, device):          # (no GPU here: what a uint8 tensor on cuda:1 answers)
        calls.append((n, str(device)))
        return types.SimpleNamespace(numel=lambda: n, device=torch.device("cuda", 1))

    o = types.SimpleNamespace()
    ws = H.HandleOwner._workspace(o, 64, "cuda", alloc)
    assert H.HandleOwner._workspace(o, 64, "cuda", alloc) is ws and H.HandleOwner._workspace(o, 8, "cuda:1", alloc) is ws
    assert calls == [(64, "cuda")]
    assert H.HandleOwner._workspace(o, 8, "cuda:0", alloc) is not ws and calls[1:] == [(8, "cuda:0")]          # another index
    assert H.HandleOwner._workspace(o, 8, "cpu", alloc) is not ws and len(calls) == 3                          # another type


def test_workspace_allocation_that_raises_leaves_none_behind():
    def alloc(n, dtype, device):
        raise MemoryError("out of memory")

    o = types.SimpleNamespace()
    o.__dict__["_t2s_ws"] = torch.empty(4, dtype=torch.uint8)
    with pytest.raises(MemoryError):
        H.HandleOwner._workspace(o, 8, CPU, alloc)
    assert o.__dict__["_t2s_ws"] is None


class _Stack(C.Structure):
    _fields_ = [("conv3_w", C.c_void_p * 4), ("conv1_w", C.c_void_p * 4)]


class _Weights(C.Structure):
    _fields_ = [("a_w", C.c_void_p), ("a_b", C.c_void_p), ("stack", _Stack)]


def test_fill_writes_addresses_of_kept_fp32_contiguous_tensors():
    w, keep = _Weights(), []
    a = nn.Parameter(torch.arange(6.0).reshape(2, 3))
    half = torch.ones(4, dtype=torch.float16)
    strided = torch.arange(8.0).reshape(2, 4).t()
    H.fill(w, [("a_w", a), ("a_b", half)], keep)
    H.fill(w.stack, [(("conv3_w", 2), strided), (("conv1_w", 0), a)], keep)
    assert len(keep) == 4 and all(k.dtype == torch.float32 and k.is_contiguous() and not k.requires_grad for k in keep)
    assert w.a_w == a.data_ptr() == keep[0].data_ptr()          # fp32 contiguous: no copy
    assert w.a_b == keep[1].data_ptr() != half.data_ptr() and torch.equal(keep[1], half.float())
    assert w.stack.conv3_w[2] == keep[2].data_ptr() and torch.equal(keep[2], strided) and w.stack.conv1_w[0] == a.data_ptr()
    assert w.stack.conv3_w[0] is None and w.stack.conv1_w[1] is None
    with pytest.raises(L.T2SError, match="layers.3.mlp.0.weight must live on a GPU"):          # a name: through L.dev_ptr
        H.fill(w, [("a_w", a, "layers.3.mlp.0.weight")], keep)


def test_require_on_names_the_owner_and_the_devices():
    H.require_on([torch.zeros(1)], CPU, "LA-VAE")
    with pytest.raises(L.T2SError, match="^TSae parameters live on cpu but the input is on meta$"):
        H.require_on([torch.zeros(1)], torch.device("meta"), "TSae")
    with pytest.raises(L.T2SError, match="on meta; call model.to\\(device\\) first$"):
        H.require_on([torch.zeros(1)], torch.device("meta"), "MLP", "; call model.to(device) first")


def test_handle_creates_on_a_synchronised_device_and_destroys_once(monkeypatch):
    log = []

    def create(w, n, out):
        log.append(("create", w, n))
        C.cast(out, C.POINTER(C.c_void_p))[0] = 0x1000
        return 0

    def refuse(out):
        return 3

    fake = types.SimpleNamespace(t2s_x_create=create, t2s_x_refuse=refuse, t2s_x_destroy=lambda p: log.append(("destroy", p.value)),
                                 t2s_last_error=lambda: b"max_seqs > 65536")
    monkeypatch.setattr(L, "lib", lambda: fake)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda d: log.append(("sync", str(d))))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    h = H.Handle("meta", "t2s_x_create", "t2s_x_destroy", "weights", 7)
    g = H.Handle("meta", "t2s_x_create", "t2s_x_destroy", "weights", 8)
    assert log == [("sync", "meta"), ("create", "weights", 7), ("sync", "meta"), ("create", "weights", 8)]
    assert h.ptr.value == 0x1000 and h.device == torch.device("meta") and h.keep is None
    assert h.uid != g.uid                                # same address, two handles: users compare uids
    del log[:]
    h.close(), h.close()
    assert log == [("destroy", 0x1000)]
    del g                                                # an unreferenced handle is destroyed with the object
    assert log == [("destroy", 0x1000)] * 2
    with pytest.raises(L.T2SError, match="t2s_x_refuse failed \\(rc=3\\): max_seqs > 65536"):
        H.Handle("meta", "t2s_x_refuse", "t2s_x_destroy")
    assert log[2:] == [("sync", "meta")]                 # nothing was created: nothing to destroy
