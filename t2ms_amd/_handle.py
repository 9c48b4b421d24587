"""How the module mirrors own a C handle of libt2s_hip.so -- the one place that knows the policy.

A mirror (Transformer, the LA-VAE Encoder / Decoder, the TSae sides) caches a device handle against its parameters and has
to notice when they move.  The pieces, each written once:
  * stamp_of    what "the parameters did not change" means on the host: storage address and in-place version per tensor;
  * fill        detached fp32 contiguous tensors, kept alive, their addresses written into a ctypes struct;
  * Handle      the pointer, created on a synchronised device, destroyed under the device's lock by close() or with the object;
  * HandleOwner the cache policy (rebuild / refresh / serve), pickling without the device state, a grow-only workspace.
"""
import ctypes as C
import itertools
import weakref

import torch

from . import _lib as L


def stamp_of(ts):
    """(data_ptr, in-place version) per tensor: changes whenever one was written in place (optimizer step, load_state_dict)
    or re-allocated (.to()).  None when torch keeps no version counter for one of them (tensors created under
    torch.inference_mode(): `._version` raises): nothing can then be cached against the stamp -- see cached() and
    HandleOwner._owned_handle.  The tensors are asked is_inference() only once `._version` has raised: the class-API loop
    takes two stamps of 49 tensors per diffusion step, and asking all of them first lengthens each stamp
    (profiles/handle_owner.md).  Any other RuntimeError is the caller's."""
    try:
        return tuple([(t.data_ptr(), t._version) for t in ts])
    except RuntimeError:
        if any(t.is_inference() for t in ts):
            return None
        raise


def cached(owner, key, device, stamp):
    """The value stored as owner.__dict__[key] = (device, stamp, value) if it still stands, else None."""
    c = owner.__dict__.get(key)
    if c is not None and stamp is not None and c[0] == device and c[1] == stamp:
        return c[2]
    return None


def require_on(ts, device, who, hint=""):
    for t in ts:
        if t.device != device:
            raise L.T2SError(f"{who} parameters live on {t.device} but the input is on {device}{hint}")


def fill(dst, pairs, keep):
    """For each (field, tensor[, name]): append the detached fp32 contiguous tensor to `keep` and write its address into
    dst.field -- or into dst.field[i] for a field given as (field, i).  With a name the address is taken through L.dev_ptr
    (on a GPU, fp32, contiguous -- or a T2SError that carries the name)."""
    for field, t, *name in pairs:
        c = L.as_f32(t.detach())
        keep.append(c)
        addr = L.dev_ptr(c, *name) if name else c.data_ptr()
        if isinstance(field, tuple):
            getattr(dst, field[0])[field[1]] = addr
        else:
            setattr(dst, field, addr)


_UIDS = itertools.count(1)


class Handle:
    """Owns one object of the library on one device: `create` and `destroy` are entry names, create is called as
    create(*args, &ptr).  `uid` identifies THIS handle for the life of the process: a re-created handle often gets the freed
    one's address back, so users that cache state bound to a handle (Sampler's captured hipGraph, a pending backward) compare
    uids, never pointers.  Building synchronises the device, allocates and copies: the caller holds L.device_lock(device)."""

    def __init__(self, device, create, destroy, *args):
        self.uid, self.ptr, self.keep = next(_UIDS), C.c_void_p(), None
        self.device = torch.device(device)
        torch.cuda.synchronize(device)
        with torch.cuda.device(device):
            L.check(getattr(L.lib(), create)(*args, C.byref(self.ptr)), create)
        self._fin = weakref.finalize(self, L.destroy_locked, destroy, str(self.device), self.ptr)

    def close(self):
        self._fin()


class HandleOwner:
    """Mixin of the mirrors (and of TS2VecEncoder, for the workspace).  Everything lives in the instance's __dict__ under
    `_t2s_*` keys; a class lists in `_t2s_transient` the ones that describe this process's device state and stay out of a
    pickle or a deep copy."""

    _t2s_transient = ("_t2s_h", "_t2s_geom", "_t2s_stamp", "_t2s_ws")

    def _owned_handle(self, device, geometry, stamp, build, refresh, *args):
        """The cached handle for `geometry` (what the handle was sized for: a change forces a rebuild) and `stamp`
        (stamp_of the parameters: a change, or None, re-packs the weights); build(*args) makes a handle, refresh(h, *args)
        re-packs one and returns what has to stay alive meanwhile, or is None where the library has no such entry.
          * no handle or another geometry: rebuild under the device's lock (a device synchronisation, frees, allocations --
            never while another thread's sampler run has a capture open, _lib.device_lock).  The old handle is forgotten,
            then closed -- BEFORE the new one is built, the free precedes a multi-GB allocation -- and the new one is stored
            only once build() has returned: a build that raises leaves no handle behind, the next call builds again;
          * the stamp moved: h.keep = refresh(h, *args) -- stream-ordered copies, no lock, no allocation; the sources stay alive on
            the handle until the next refresh.  Without `refresh` the handle is rebuilt;
          * otherwise the cached handle, and nothing else happens."""
        d = self.__dict__
        h = d.get("_t2s_h")
        if h is not None and d.get("_t2s_geom") == geometry:
            if stamp is not None and d.get("_t2s_stamp") == stamp:
                return h
            if refresh is not None:
                h.keep = refresh(h, *args)
                d["_t2s_stamp"] = stamp
                return h
        with L.device_lock(device):
            for k in ("_t2s_h", "_t2s_geom", "_t2s_stamp"):
                d.pop(k, None)
            if h is not None:
                h.close()
            h = build(*args)
        d["_t2s_h"], d["_t2s_geom"], d["_t2s_stamp"] = h, geometry, stamp
        return h

    def _workspace(self, need, device, alloc=torch.empty):
        """Grow-only byte workspace on `device`: the same tensor while it is large enough, else a new one (the old one is
        released first) allocated under the device's lock.  A device given without an index ("cuda") is the one the
        workspace already lives on: a tensor's own device always carries one."""
        ws, dev = self.__dict__.get("_t2s_ws"), torch.device(device)
        if ws is None or ws.numel() < need or ws.device.type != dev.type or dev.index not in (None, ws.device.index):
            with L.device_lock(device):
                ws = self.__dict__["_t2s_ws"] = None
                ws = self.__dict__["_t2s_ws"] = alloc(need, dtype=torch.uint8, device=device)
        return ws

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in self._t2s_transient:
            state.pop(k, None)
        return state
