"""The LA-VAE codec mirror, once: what model/pretrained/vqvae.py (single-channel, latent width 30) and myvqvae.py (the
C-channel motion codec, latent width ``flow_dim``) share.  Both families run the same kernels of csrc/t2s_vae.hip over the
same handle; the single-channel codec is its C = 1 case.

Here: the handle's recipe (_Codec over _handle.HandleOwner), the weight and gradient lists, the HIP forwards with their autograd nodes
(_EncodeFn / _DecodeFn over _vae_backward), the torch-op forwards for what the HIP backward does not cover, the coverage
predicate (_backward_covers), the switches (_torch_forced) and the routing between the three forwards (_route).  A family
supplies its entries (_entries), the encoder's latent width (_width) and series layout (_series), the decoder's last torch-op
step (_recon_autograd), `channels`, and the ``forward`` front doors with the reference's argument rules.  Reference pickles
are unpickled without __init__: every hyper-parameter is read from the conv modules, never from an attribute set only here.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _handle as H
from ... import _lib as L


class Residual(nn.Module):
    """Parameter container: _block = [ReLU, Conv k3 no-bias, ReLU, Conv k1 no-bias]."""

    def __init__(self, in_channels, num_hiddens, num_residual_hiddens):
        super().__init__()
        self._block = nn.Sequential(
            nn.ReLU(True),
            nn.Conv1d(in_channels, num_residual_hiddens, kernel_size=3, stride=1, padding=1, bias=False),
            nn.ReLU(True),
            nn.Conv1d(num_residual_hiddens, num_hiddens, kernel_size=1, stride=1, bias=False))

    def forward(self, x):
        raise L.T2SError("Residual runs inside the fused LA-VAE kernels; call Encoder/Decoder.forward")


class ResidualStack(nn.Module):
    """`_residual`: the family's own Residual class (a pickle names each layer's class by its module)."""

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens):
        super().__init__()
        self._layers = nn.ModuleList([self._residual(in_channels, num_hiddens, num_residual_hiddens)
                                      for _ in range(num_residual_layers)])

    def forward(self, x):
        raise L.T2SError("ResidualStack runs inside the fused LA-VAE kernels; call Encoder/Decoder.forward")


def _stack_autograd(stack, h):
    """ResidualStack.forward plus the ReLU behind it as torch ops, from h = relu(the stack's input): nn.ReLU(True) of the
    reference's Residual mutates the block input, so the skip carries relu(x) (vqvae.py:10-21, myvqvae.py:9-17).  (The caller
    applies the first ReLU so that no frame holds on to the tensor in front of it while the stack runs.)"""
    for layer in stack._layers:
        h = F.relu(h + layer._block[3](F.relu(layer._block[1](h))))
    return h


def _backward_covers(hidden, emb, res_hidden, n_res, Ln, W, channels):
    """The shapes t2s_vae_encode_backward[_mc] / t2s_vae_decode_backward[_mc] take: the reference's default LA-VAE
    (pretrained_lavae_unified.py:119-122: hidden 128, res_hidden 128 / 256, emb 64, 1..4 residual layers; `res_hidden` None: a
    stack without layers).  `channels` None: the single-channel entries, on the BASELINE lengths; else the _mc ones."""
    max_len, len_step, max_w = (128, 4, 32) if channels is None else (192, 1, 64)
    return (hidden == 128 and emb == 64 and res_hidden is not None and res_hidden % 128 == 0 and 1 <= n_res <= 4
            and 8 <= Ln <= max_len and Ln % len_step == 0 and 1 <= W <= max_w and (channels is None or 1 <= channels <= 16))


def _backward_mode():
    """T2S_MVAE_BACKWARD = hip | torch, read at every call; unset: hip (profiles/mvae_train.json)."""
    mode = os.environ.get("T2S_MVAE_BACKWARD", "") or "hip"
    if mode not in ("hip", "torch"):
        raise L.T2SError(f"T2S_MVAE_BACKWARD={mode!r}: expected 'hip' or 'torch'")
    return mode


def _torch_forced(direction, multichannel):
    """Does the family's switch, read at every call, send a covered shape to the torch-op forward all the same?"""
    if multichannel:
        return _backward_mode() == "torch"
    switch = {"encoder": "T2S_ENCODER_TORCH_AUTOGRAD", "decoder": "T2S_DECODER_TORCH_AUTOGRAD"}[direction]
    return os.environ.get(switch, "0") not in ("", "0")          # unset / "" / "0": the HIP backward


def _route(direction, multichannel, g, p, i, c, t):
    """Which forward a call takes: "hip" (the kernel, nothing saved), "fn" (the kernel behind _EncodeFn / _DecodeFn) or
    "autograd" (torch ops).  g: grad is enabled; p: a parameter requires grad; i: the input requires grad; c: the shape is
    covered (_backward_covers); t: torch is forced (_torch_forced).  The encoder's backward entries produce parameter gradients
    only, so a series that asks for one takes the torch ops.
    KNOWN DIFFERENCE, kept: the single-channel encoder does not consult `i` when it asks whether anyone wants a gradient --
    with frozen parameters and a series that requires grad it returns a result without a graph."""
    if direction == "encoder":
        wants, fn = g and (p or (i and multichannel)), c and not i and not t
    else:
        wants, fn = g and (p or i), c and not t
    return "hip" if not wants else "fn" if fn else "autograd"


def _vae_backward(codec, struct, B, Ln, call):
    """What _EncodeFn.backward and _DecodeFn.backward share: fresh gradient tensors for codec._grad_params(), which lists
    them in the declared field order of `struct` (a residual-stack array takes one per layer), then
    `call(handle, byref(struct), stream)`; returns the gradients with None for a frozen parameter."""
    params = codec._grad_params()
    grads = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
    g, ptrs, n = struct(), iter(t.data_ptr() for t in grads), len(codec._residual_stack._layers)
    for name, ctype in struct._fields_:
        if ctype is C.c_void_p:
            setattr(g, name, next(ptrs))
        else:
            getattr(g, name)[:n] = [next(ptrs) for _ in range(n)]
    dev = params[0].device
    with torch.cuda.device(dev):
        ptr = codec._handle(dev)           # (the weights of the forward: no optimizer step happens between the two)
        h, rows = codec.__dict__["_t2s_h"], B * (Ln // 4)
        grows = rows > h.bwd_rows or B > h.bwd_series          # the C side's condition: vae_grow_rows, t2s_vae.hip
        # growing the row blocks frees / allocates device memory: under the device's lock, like building the handle
        with L.device_lock(dev) if grows else contextlib.nullcontext():
            call(ptr, C.byref(g), L.stream_ptr(dev))
        h.bwd_rows, h.bwd_series = max(h.bwd_rows, rows), max(h.bwd_series, B)
    return [gr if p.requires_grad else None for gr, p in zip(grads, params)]


class _Codec(H.HandleOwner, nn.Module):
    """What Encoder and Decoder share: the handle (cached against parameter storage + version) and the routing's inputs."""

    @property
    def channels(self):
        """None: the single-channel family; the multichannel classes answer C (what the Sampler asks a decoder)."""
        return None

    def _res_hidden(self):
        """num_residual_hiddens as the stack's first layer has it; None for a stack without layers."""
        layers = self._residual_stack._layers
        return layers[0]._block[1].out_channels if len(layers) else None

    def _stack_weights(self, w, stack, names):
        """The fields both directions fill the same way: the stack's, and `names` = ((field, tensor), ...)."""
        keep, layers = [], self._residual_stack._layers
        if len(layers) > 4:
            raise L.T2SError(f"LA-VAE: num_residual_layers={len(layers)} > 4 is not supported by the HIP codec")
        w.res_hidden, w.n_res_layers = self._res_hidden() or 1, len(layers)
        for i, layer in enumerate(layers):
            H.fill(stack, ((("conv3_w", i), layer._block[1].weight), (("conv1_w", i), layer._block[3].weight)), keep)
        H.fill(w, names, keep)
        return w, keep

    def _entry(self, k, *args):
        """The family's forward (k = 0) or backward (k = 1) entry."""
        name = self._entries[k]
        L.check(getattr(L.lib(), name)(*args), name)

    def _stack_params(self):
        layers = self._residual_stack._layers
        return [layer._block[1].weight for layer in layers] + [layer._block[3].weight for layer in layers]

    def _route_of(self, inputs, *shape):
        """_route for this call (`shape`: the arguments of _hip_backward_ok).  The shape and the switch are asked only where
        the result depends on them: a switch with a value it does not know raises for a covered shape that would take
        "fn", and for nothing else."""
        d, m, g, i = self._direction, self.channels is not None, torch.is_grad_enabled(), inputs.requires_grad
        p = g and any(q.requires_grad for q in self.parameters())
        route = _route(d, m, g, p, i, True, False)       # "fn" here: someone wants a gradient and c, t decide
        if route == "fn":
            c = self._hip_backward_ok(*shape)
            route = _route(d, m, g, p, i, c, c and _torch_forced(d, m))
        return route

    def _tensors(self):
        return [p for p in self.parameters()]

    def _build(self, device):
        """channels None: the single-channel codec (t2s_vae_create); C: the multichannel one (t2s_vae_create_mc)."""
        w, keep = self._weights_struct()          # (the library makes its own copies: `keep` ends with this call)
        if self.channels is None:
            h = H.Handle(device, "t2s_vae_create", "t2s_vae_destroy", C.byref(w))
        else:
            h = H.Handle(device, "t2s_vae_create_mc", "t2s_vae_destroy", C.byref(w), int(self.channels))
        # what the C handle's backward row blocks hold (a mirror handle serves one direction, an encoder's or a decoder's):
        # vae_grow_rows (t2s_vae.hip) grows them when rows > held rows or B > held series; _vae_backward repeats that condition
        h.bwd_rows = h.bwd_series = 0
        return h

    def _refresh(self, h, device):
        """Same shapes, new contents (an optimizer step on a trainable encoder, load_state_dict): re-copy into the handle's own
        buffers -- no allocation, stream-ordered (t2s_vae_update_weights)."""
        w, keep = self._weights_struct()
        with torch.cuda.device(device):
            L.check(L.lib().t2s_vae_update_weights(h.ptr, C.byref(w), L.stream_ptr(device)), "t2s_vae_update_weights")
        return keep

    def _handle(self, device):
        """The t2s_vae pointer (HandleOwner._owned_handle): rebuilt for another device or other shapes, refreshed for new
        contents."""
        device = torch.device(device)
        ts = self._tensors()
        H.require_on(ts, device, "LA-VAE")
        geometry = (device,) + tuple(tuple(t.shape) for t in ts)
        return self._owned_handle(device, geometry, H.stamp_of(ts), self._build, self._refresh, device).ptr


class Encoder(_Codec):
    """`_stack`: the family's own ResidualStack class."""

    _direction = "encoder"

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, embedding_dim):
        super().__init__()
        self._conv_1 = nn.Conv1d(in_channels, num_hiddens // 2, kernel_size=4, stride=2, padding=1)
        self._conv_2 = nn.Conv1d(num_hiddens // 2, num_hiddens, kernel_size=4, stride=2, padding=1)
        self._conv_3 = nn.Conv1d(num_hiddens, num_hiddens, kernel_size=3, stride=1, padding=1)
        self._residual_stack = self._stack(num_hiddens, num_hiddens, num_residual_layers, num_residual_hiddens)
        self._pre_vq_conv = nn.Conv1d(num_hiddens, embedding_dim, kernel_size=1, stride=1)

    def _weights_struct(self):
        w = L.VaeWeights()          # (only _conv_1's shape carries the channels)
        w.hidden = self._conv_2.out_channels
        w.emb = self._pre_vq_conv.out_channels
        return self._stack_weights(w, w.enc_stack, (
            ("enc_conv1_w", self._conv_1.weight), ("enc_conv1_b", self._conv_1.bias),
            ("enc_conv2_w", self._conv_2.weight), ("enc_conv2_b", self._conv_2.bias),
            ("enc_conv3_w", self._conv_3.weight), ("enc_conv3_b", self._conv_3.bias),
            ("enc_prevq_w", self._pre_vq_conv.weight), ("enc_prevq_b", self._pre_vq_conv.bias)))

    def _grad_params(self):
        """The encoder tensors in t2s_vae_enc_grads order (12 with two residual layers)."""
        ps = [self._conv_1.weight, self._conv_1.bias, self._conv_2.weight, self._conv_2.bias, self._conv_3.weight, self._conv_3.bias]
        return ps + self._stack_params() + [self._pre_vq_conv.weight, self._pre_vq_conv.bias]

    def _hip_backward_ok(self, Ln):
        return _backward_covers(self._conv_2.out_channels, self._pre_vq_conv.out_channels, self._res_hidden(),
                                len(self._residual_stack._layers), Ln, self._width(), self.channels)

    def _forward_autograd(self, inputs):
        """The same forward as torch ops UNDER AUTOGRAD: the training path for shapes the HIP backward does not cover
        (_backward_covers), for a series that itself asks for a gradient, and under the family's switch (_torch_forced) --
        host-level plumbing like the MLP denoiser, no throughput claim.  A covered shape runs forward AND backward in the
        HIP kernels (_EncodeFn)."""
        h = F.relu(self._conv_1(self._series(inputs.float())))
        h = F.relu(self._conv_2(h))
        before = self._pre_vq_conv(_stack_autograd(self._residual_stack, F.relu(self._conv_3(h))))
        return F.interpolate(before, size=self._width(), mode="linear", align_corners=True), before

    def _width_arg(self, W):
        """(the single-channel entries are built for the latent width 30 and take none)"""
        return () if self.channels is None else (W,)

    def _forward_hip(self, inputs):
        B, Ln, W = inputs.shape[0], inputs.shape[-1], self._width()
        x = self._series(L.as_f32(inputs))
        dev = x.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            emb = self._pre_vq_conv.out_channels
            z = torch.empty(B, emb, W, device=dev, dtype=torch.float32)
            before = torch.empty(B, emb, Ln // 4, device=dev, dtype=torch.float32)
            self._entry(0, h, L.dev_ptr(x, "inputs"), L.dev_ptr(z), L.dev_ptr(before), B, Ln, *self._width_arg(W),
                        L.stream_ptr(dev))
        return z, before

    def encode_ragged(self, series):
        """Clips of unequal length in ONE launch (t2s_vae_encode_mc_ragged): a list of (C, L_b) GPU tensors, each L_b >= 8 or
        0 -> z (B,64,flow_dim).  Row b equals forward(series[b][None])[0] bit for bit; the latent of an empty clip is zero.
        Multichannel codec only; under no_grad (inference: the ragged entries have no backward)."""
        what = "Encoder.encode_ragged"
        ch = self.channels
        if ch is None:
            raise L.T2SError(f"{what}: the single-channel codec has no ragged entries (model/pretrained/myvqvae.py has)")
        series = list(series)
        for b, t in enumerate(series):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != ch:
                raise L.T2SError(f"{what}: series[{b}] must be a ({ch},L) tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        lens, off, off4 = L.ragged_layout([t.shape[1] for t in series], None, what)
        if any(not t.is_cuda for t in series):
            raise L.T2SError(f"{what}: the series must live on a GPU; the HIP path has no CPU fallback")
        B, W, dev, max_L = len(series), self._width(), series[0].device, int(lens.max())
        emb = self._pre_vq_conv.out_channels
        with torch.no_grad(), torch.cuda.device(dev):
            z = torch.zeros(B, emb, W, device=dev, dtype=torch.float32)
            if max_L == 0:
                return z
            x = torch.cat([L.as_f32(t).reshape(-1) for t in series])
            before = torch.empty(emb * int(off4[-1]), device=dev, dtype=torch.float32)
            h = self._handle(dev)
            keep, p_len, p_off, p_off4 = L.ragged_device_tables(lens, off, off4, dev)
            L.check(L.lib().t2s_vae_encode_mc_ragged(h, L.dev_ptr(x, "series"), p_len, p_off, p_off4, L.dev_ptr(z), L.dev_ptr(before),
                                                     B, max_L, W, L.stream_ptr(dev)), "t2s_vae_encode_mc_ragged")
            keep.record_stream(torch.cuda.current_stream(dev))
        return z

    def _forward_kernel(self, route, inputs):
        """The "hip" and "fn" routes."""
        return _EncodeFn.apply(self, inputs, *self._grad_params()) if route == "fn" else self._forward_hip(inputs)


class _EncodeFn(torch.autograd.Function):
    """Encoder.forward under autograd, both directions in the HIP kernels: the encoder's _forward_hip now (t2s_vae_encode[_mc]),
    t2s_vae_encode_backward[_mc] for the parameter gradients (the forward is recomputed from x there; nothing but x is saved).
    The input series gets no gradient (it is data, train.py:104-106)."""

    @staticmethod
    def forward(ctx, enc, inputs, *params):
        with torch.no_grad():
            z, before = enc._forward_hip(inputs)
        ctx.enc, ctx.W = enc, z.shape[2]
        ctx.save_for_backward(enc._series(L.as_f32(inputs)))
        ctx.set_materialize_grads(False)      # train.py uses z only: `before` then arrives as None, not as a zero tensor
        return z, before

    @staticmethod
    def backward(ctx, dz, dbefore):
        (x,) = ctx.saved_tensors
        B, Ln, W = x.shape[0], x.shape[-1], ctx.W
        dzc = L.as_f32(dz) if dz is not None else torch.zeros(B, 64, W, device=x.device)
        dbc = L.as_f32(dbefore) if dbefore is not None else None
        out = _vae_backward(ctx.enc, L.VaeEncGrads, B, Ln, lambda h, g, st: ctx.enc._entry(
            1, h, L.dev_ptr(x), L.dev_ptr(dzc), L.dev_ptr(dbc), g, B, Ln, *ctx.enc._width_arg(W), st))
        return (None, None, *out)


class Decoder(_Codec):
    """`_stack`: the family's own ResidualStack class."""

    _direction = "decoder"

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, out_channels):
        super().__init__()
        self._conv_1 = nn.Conv1d(in_channels, num_hiddens, kernel_size=3, stride=1, padding=1)
        self._residual_stack = self._stack(num_hiddens, num_hiddens, num_residual_layers, num_residual_hiddens)
        self._conv_trans_1 = nn.ConvTranspose1d(num_hiddens, num_hiddens // 2, kernel_size=4, stride=2, padding=1)
        self._conv_trans_2 = nn.ConvTranspose1d(num_hiddens // 2, out_channels, kernel_size=4, stride=2, padding=1)

    def _weights_struct(self):
        w = L.VaeWeights()          # (only _conv_trans_2's shapes carry the channels)
        w.hidden = self._conv_1.out_channels
        w.emb = self._conv_1.in_channels
        return self._stack_weights(w, w.dec_stack, (
            ("dec_conv1_w", self._conv_1.weight), ("dec_conv1_b", self._conv_1.bias),
            ("dec_ct1_w", self._conv_trans_1.weight), ("dec_ct1_b", self._conv_trans_1.bias),
            ("dec_ct2_w", self._conv_trans_2.weight), ("dec_ct2_b", self._conv_trans_2.bias)))

    def _grad_params(self):
        """The decoder tensors in t2s_vae_dec_grads order (10 with two residual layers)."""
        return ([self._conv_1.weight, self._conv_1.bias] + self._stack_params()
                + [self._conv_trans_1.weight, self._conv_trans_1.bias, self._conv_trans_2.weight, self._conv_trans_2.bias])

    def _hip_backward_ok(self, Ln, W):
        return _backward_covers(self._conv_1.out_channels, self._conv_1.in_channels, self._res_hidden(),
                                len(self._residual_stack._layers), Ln, W, self.channels)

    def _forward_autograd(self, inputs, length):
        """The same forward as torch ops UNDER AUTOGRAD (see Encoder._forward_autograd).  A covered shape runs forward AND
        backward in the HIP kernels (_DecodeFn)."""
        after = F.interpolate(inputs.float(), size=int(length / 4), mode="linear", align_corners=True)
        h = _stack_autograd(self._residual_stack, F.relu(self._conv_1(after)))
        return self._recon_autograd(self._conv_trans_2(F.relu(self._conv_trans_1(h))), length), after

    def _forward_hip(self, z, Ln):
        B, W, dev, ch = z.shape[0], z.shape[2], z.device, self.channels
        with torch.cuda.device(dev):
            h = self._handle(dev)
            recon = torch.empty((B, Ln) if ch is None else (B, ch, Ln), device=dev, dtype=torch.float32)
            after = torch.empty(B, z.shape[1], Ln // 4, device=dev, dtype=torch.float32)
            self._entry(0, h, L.dev_ptr(z, "inputs"), L.dev_ptr(recon), L.dev_ptr(after), B, Ln, W, L.stream_ptr(dev))
        return recon, after

    def decode_ragged(self, z, lengths):
        """One launch, a length per row (t2s_vae_decode_mc_ragged): z (B,64,W), lengths = B integers, each 0 or >= 8 -> a list
        of (C, L_b) tensors, views of one packed buffer.  Row b equals forward(z[b:b+1], L_b)[0][0] bit for bit.  Multichannel
        codec only; under no_grad."""
        what = "Decoder.decode_ragged"
        ch = self.channels
        if ch is None:
            raise L.T2SError(f"{what}: the single-channel codec has no ragged entries (model/pretrained/myvqvae.py has)")
        if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[1] != self._conv_1.in_channels:
            raise L.T2SError(f"{what}: latent must be (B,{self._conv_1.in_channels},W), got "
                             f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__}")
        lens, off, off4 = L.ragged_layout(lengths, None, what, batch=z.shape[0])
        if not z.is_cuda:
            raise L.T2SError(f"{what}: latent must live on a GPU; the HIP path has no CPU fallback")
        B, W, dev, max_L = z.shape[0], z.shape[2], z.device, int(lens.max())
        with torch.no_grad(), torch.cuda.device(dev):
            packed = torch.empty(ch * int(off[-1]), device=dev, dtype=torch.float32)
            if max_L != 0:
                zc = L.as_f32(z)
                h = self._handle(dev)
                keep, p_len, p_off, _ = L.ragged_device_tables(lens, off, off4, dev)
                L.check(L.lib().t2s_vae_decode_mc_ragged(h, L.dev_ptr(zc, "latent"), p_len, p_off, L.dev_ptr(packed), B, max_L, W,
                                                         L.stream_ptr(dev)), "t2s_vae_decode_mc_ragged")
                keep.record_stream(torch.cuda.current_stream(dev))
        return [packed[ch * int(off[b]):ch * int(off[b + 1])].view(ch, int(lens[b])) for b in range(B)]

    def _forward_kernel(self, route, inputs, Ln):
        """The "hip" and "fn" routes: (recon, after) of the Ln samples the kernels write."""
        z = L.as_f32(inputs)
        return _DecodeFn.apply(self, z, Ln, *self._grad_params()) if route == "fn" else self._forward_hip(z, Ln)


class _DecodeFn(torch.autograd.Function):
    """Decoder.forward under autograd, both directions in the HIP kernels: the decoder's _forward_hip now (t2s_vae_decode_w /
    _mc), t2s_vae_decode_backward[_mc] for the parameter gradients and the latent's (the forward is recomputed from z there;
    nothing but z is saved)."""

    @staticmethod
    def forward(ctx, dec, z, Ln, *params):
        with torch.no_grad():
            recon, after = dec._forward_hip(z, Ln)
        ctx.dec, ctx.Ln, ctx.recon_shape = dec, Ln, recon.shape
        ctx.save_for_backward(z)
        ctx.set_materialize_grads(False)      # a loss on `recon` alone: `after` then arrives as None, not as a zero tensor
        return recon, after

    @staticmethod
    def backward(ctx, drecon, dafter):
        (z,) = ctx.saved_tensors
        B, W, Ln = z.shape[0], z.shape[2], ctx.Ln
        drc = L.as_f32(drecon).reshape(ctx.recon_shape) if drecon is not None else torch.zeros(ctx.recon_shape, device=z.device)
        dac = L.as_f32(dafter) if dafter is not None else None
        dz = torch.empty_like(z) if ctx.needs_input_grad[1] else None
        out = _vae_backward(ctx.dec, L.VaeDecGrads, B, Ln, lambda h, g, st: ctx.dec._entry(
            1, h, L.dev_ptr(z), L.dev_ptr(drc), L.dev_ptr(dac), g, L.dev_ptr(dz), B, Ln, W, st))
        return (None, dz, None, *out)
