"""Host-side mirror of the reference's multichannel LA-VAE codec (model/pretrained/myvqvae.py), the codec of the T2MS
motion models: C-channel series (7 deadlift, 10 bench press), latent width ``flow_dim``, any length L >= 8.

Class names, constructor signatures, attribute names and state-dict keys equal the reference's, so a plain state dict
(myinfer.py:126-128, mytrain.py:29-30) and a whole-module pickle both load.  Under no_grad ``Encoder.forward`` and
``Decoder.forward`` run the single-launch HIP kernels t2s_vae_encode_mc / t2s_vae_decode_mc (csrc/t2s_vae.hip): C <= 16,
flow_dim <= 64, hidden <= 128, res_hidden <= 256, <= 4 residual layers, embedding_dim 64.  No CPU fallback.

With grad enabled and a parameter or the latent asking for a gradient, a covered shape (``_mc_backward_covers``: hidden 128,
embedding_dim 64, res_hidden 128 / 256, 1..4 residual layers, 8 <= L <= 192, flow_dim <= 64, C <= 16) runs the same HIP forward
behind the single-channel mirror's autograd nodes (_EncodeFn, _DecodeFn), whose backward is t2s_vae_encode_backward_mc /
t2s_vae_decode_backward_mc: ``vqvae.shared_eval(..., 'train')`` and a trainable encoder grafted onto the DiT (mytrain.py:37-40)
train on HIP.  Everything else -- and everything under ``T2S_MVAE_BACKWARD=torch`` -- runs as torch ops under autograd
(``_forward_autograd``, host-level plumbing like the single-channel mirror's path for shapes its HIP backward does not cover).
The handle cache, version stamps, in-place weight refresh and the device lock are the single-channel mirror's (_Codec,
_VaeHandle).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib as L
from .core import BaseModel
from . import vqvae as _vq
from .vqvae import _Codec


class Residual(nn.Module):
    """myvqvae.py:6-17 (parameter container: _block = [ReLU, Conv k3 no-bias, ReLU, Conv k1 no-bias])."""

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
    """myvqvae.py:19-30."""

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens):
        super().__init__()
        self._layers = nn.ModuleList([Residual(in_channels, num_hiddens, num_residual_hiddens)
                                      for _ in range(num_residual_layers)])

    def forward(self, x):
        raise L.T2SError("ResidualStack runs inside the fused LA-VAE kernels; call Encoder/Decoder.forward")


def _stack_autograd(stack, h):
    """ResidualStack.forward as torch ops: nn.ReLU(True) mutates the block input, so the skip carries relu(x) (myvqvae.py:9-17)."""
    for layer in stack._layers:
        h = F.relu(h)
        h = h + layer._block[3](F.relu(layer._block[1](h)))
    return F.relu(h)


def _wants_grad(module, inputs):
    return torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in module.parameters()))


def _mc_backward_covers(hidden, emb, res_hidden, n_res, Ln, W, channels):
    """The shapes t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc take (`res_hidden` None: a stack without layers)."""
    return (hidden == 128 and emb == 64 and res_hidden is not None and res_hidden % 128 == 0 and 1 <= n_res <= 4
            and 8 <= Ln <= 192 and 1 <= W <= 64 and 1 <= channels <= 16)


def _backward_mode():
    """T2S_MVAE_BACKWARD = hip | torch, read at every call; unset: hip (profiles/mvae_train.json)."""
    mode = os.environ.get("T2S_MVAE_BACKWARD", "") or "hip"
    if mode not in ("hip", "torch"):
        raise L.T2SError(f"T2S_MVAE_BACKWARD={mode!r}: expected 'hip' or 'torch'")
    return mode


class Encoder(_Codec):
    """myvqvae.py:32-61."""

    _t2s_multichannel = True

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, embedding_dim, flow_dim):
        super().__init__()
        self.flow_dim = flow_dim
        self._conv_1 = nn.Conv1d(in_channels, num_hiddens // 2, kernel_size=4, stride=2, padding=1)
        self._conv_2 = nn.Conv1d(num_hiddens // 2, num_hiddens, kernel_size=4, stride=2, padding=1)
        self._conv_3 = nn.Conv1d(num_hiddens, num_hiddens, kernel_size=3, stride=1, padding=1)
        self._residual_stack = ResidualStack(num_hiddens, num_hiddens, num_residual_layers, num_residual_hiddens)
        self._pre_vq_conv = nn.Conv1d(num_hiddens, embedding_dim, kernel_size=1, stride=1)

    def _mc_channels(self):
        return self._conv_1.in_channels

    _weights_struct = _vq.Encoder._weights_struct      # the same attribute names; only _conv_1's shape carries the channels

    def _hip_backward_ok(self, Ln):
        return _mc_backward_covers(self._conv_2.out_channels, self._pre_vq_conv.out_channels, self._res_hidden(),
                                   len(self._residual_stack._layers), Ln, int(self.flow_dim), self._conv_1.in_channels)

    _grad_params = _vq.Encoder._grad_params            # the 12 encoder tensors in t2s_vae_enc_grads order

    def _forward_autograd(self, inputs):
        """The same forward as torch ops UNDER AUTOGRAD: the training path for shapes t2s_vae_encode_backward_mc does not
        cover, for a series that itself asks for a gradient, and under T2S_MVAE_BACKWARD=torch -- host-level plumbing, no
        throughput claim."""
        h = F.relu(self._conv_1(inputs.float()))
        h = F.relu(self._conv_2(h))
        before = self._pre_vq_conv(_stack_autograd(self._residual_stack, self._conv_3(h)))
        return F.interpolate(before, size=self.flow_dim, mode="linear", align_corners=True), before

    def forward(self, inputs):
        """x (B,C,L) -> (z (B,64,flow_dim), before (B,64,L//4)); myvqvae.py:49-61."""
        if not inputs.is_cuda:
            raise L.T2SError("Encoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        if inputs.dim() != 3 or inputs.shape[1] != self._conv_1.in_channels:
            raise L.T2SError(f"Encoder.forward: input must be (B,{self._conv_1.in_channels},L), got {tuple(inputs.shape)}")
        if _wants_grad(self, inputs):
            # (the backward entry produces parameter gradients only: a series that asks for one takes the torch ops)
            if self._hip_backward_ok(inputs.shape[2]) and not inputs.requires_grad and _backward_mode() == "hip":
                return _vq._EncodeFn.apply(self, inputs, *self._grad_params())
            return self._forward_autograd(inputs)
        return self._forward_hip(inputs)

    def _series(self, inputs):
        """The series as the kernels read it: (B,C,L) fp32."""
        return L.as_f32(inputs)

    def _backward_hip(self, h, x, dz, dbefore, g, B, Ln, W, st):
        L.check(L.lib().t2s_vae_encode_backward_mc(h, x, dz, dbefore, g, B, Ln, W, st), "t2s_vae_encode_backward_mc")

    def _forward_hip(self, inputs):
        B, Ln, W = inputs.shape[0], inputs.shape[2], int(self.flow_dim)
        x = self._series(inputs)
        dev = x.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            emb = self._pre_vq_conv.out_channels
            z = torch.empty(B, emb, W, device=dev, dtype=torch.float32)
            before = torch.empty(B, emb, Ln // 4, device=dev, dtype=torch.float32)
            L.check(L.lib().t2s_vae_encode_mc(h, L.dev_ptr(x, "inputs"), L.dev_ptr(z), L.dev_ptr(before), B, Ln, W,
                                              L.stream_ptr(dev)), "t2s_vae_encode_mc")
        return z, before


class Decoder(_Codec):
    """myvqvae.py:63-86."""

    _t2s_multichannel = True

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, out_channels=52):
        super().__init__()
        self._conv_1 = nn.Conv1d(in_channels, num_hiddens, kernel_size=3, stride=1, padding=1)
        self._residual_stack = ResidualStack(num_hiddens, num_hiddens, num_residual_layers, num_residual_hiddens)
        self._conv_trans_1 = nn.ConvTranspose1d(num_hiddens, num_hiddens // 2, kernel_size=4, stride=2, padding=1)
        self._conv_trans_2 = nn.ConvTranspose1d(num_hiddens // 2, out_channels, kernel_size=4, stride=2, padding=1)

    def _mc_channels(self):
        return self._conv_trans_2.out_channels

    _weights_struct = _vq.Decoder._weights_struct      # the same attribute names; only _conv_trans_2's shapes carry the channels

    def _hip_backward_ok(self, Ln, W):
        return _mc_backward_covers(self._conv_1.out_channels, self._conv_1.in_channels, self._res_hidden(),
                                   len(self._residual_stack._layers), Ln, W, self._conv_trans_2.out_channels)

    _grad_params = _vq.Decoder._grad_params            # the 10 decoder tensors in t2s_vae_dec_grads order

    def _forward_autograd(self, inputs, length):
        """The same forward as torch ops UNDER AUTOGRAD (see Encoder._forward_autograd)."""
        after = F.interpolate(inputs.float(), size=int(length / 4), mode="linear", align_corners=True)
        h = _stack_autograd(self._residual_stack, self._conv_1(after))
        h = self._conv_trans_2(F.relu(self._conv_trans_1(h)))
        return F.interpolate(h, size=length, mode="linear", align_corners=True), after

    def forward(self, inputs, length):
        """z (B,64,W) -> (recon (B,C,length), after (B,64,length//4)); myvqvae.py:76-86.  No squeeze: (B,C,length) also for
        B = 1 or C = 1."""
        if not inputs.is_cuda:
            raise L.T2SError("Decoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        if inputs.dim() != 3 or inputs.shape[1] != self._conv_1.in_channels:
            raise L.T2SError(f"Decoder.forward: latent must be (B,{self._conv_1.in_channels},W), got {tuple(inputs.shape)}")
        if _wants_grad(self, inputs):
            if self._hip_backward_ok(int(length), inputs.shape[2]) and _backward_mode() == "hip":
                return _vq._DecodeFn.apply(self, L.as_f32(inputs), int(length), *self._grad_params())
            return self._forward_autograd(inputs, length)
        return self._forward_hip(L.as_f32(inputs), int(length))

    def _backward_hip(self, h, z, drecon, dafter, g, dz, B, Ln, W, st):
        L.check(L.lib().t2s_vae_decode_backward_mc(h, z, drecon, dafter, g, dz, B, Ln, W, st), "t2s_vae_decode_backward_mc")

    def _forward_hip(self, z, Ln):
        B, W, dev = z.shape[0], z.shape[2], z.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            recon = torch.empty(B, self._conv_trans_2.out_channels, Ln, device=dev, dtype=torch.float32)
            after = torch.empty(B, z.shape[1], Ln // 4, device=dev, dtype=torch.float32)
            L.check(L.lib().t2s_vae_decode_mc(h, L.dev_ptr(z, "inputs"), L.dev_ptr(recon), L.dev_ptr(after), B, Ln, W,
                                              L.stream_ptr(dev)), "t2s_vae_decode_mc")
        return recon, after


class vqvae(BaseModel):
    """myvqvae.py:88-156 (no vector quantiser despite the name)."""

    def __init__(self, args):
        super().__init__()
        self.encoder = Encoder(in_channels=args.input_dim, num_hiddens=args.block_hidden_size,
                               num_residual_layers=args.num_residual_layers, num_residual_hiddens=args.res_hidden_size,
                               embedding_dim=args.embedding_dim, flow_dim=args.flow_dim)
        self.decoder = Decoder(in_channels=args.embedding_dim, num_hiddens=args.block_hidden_size,
                               num_residual_layers=args.num_residual_layers, num_residual_hiddens=args.res_hidden_size,
                               out_channels=args.input_dim)
        # the reference's Decoder takes any latent width; the codec was trained at one: the Sampler checks it against the DiT's
        self.decoder.flow_dim = int(args.flow_dim)

    def shared_eval(self, batch, optimizer, mode):  # pyright: ignore[reportIncompatibleMethodOverride]
        """myvqvae.py:116-136.  'train' is one optimisation step with the caller's optimizer: on a covered shape the HIP
        forwards and backwards (_EncodeFn / _DecodeFn on t2s_vae_*_backward_mc), otherwise the torch-op forwards under
        autograd; 'val' / 'test' run the HIP forwards under no_grad."""
        Ln = batch.shape[-1]
        if mode == "train":
            optimizer.zero_grad()
            z, before = self.encoder(batch)
            data_recon, after = self.decoder(z, length=Ln)
            recon_error = F.mse_loss(data_recon, batch)
            loss = recon_error + F.mse_loss(before, after)
            loss.backward()
            optimizer.step()
        else:
            with torch.no_grad():
                z, before = self.encoder(batch)
                data_recon, after = self.decoder(z, length=Ln)
                recon_error = F.mse_loss(data_recon, batch)
                loss = recon_error + F.mse_loss(before, after)
        return loss, recon_error, data_recon, z

    def forward(self, x):
        z, _ = self.encoder(x)
        out, _ = self.decoder(z, length=x.shape[-1])
        return out

    def custom_loss(self, x, y, lambda_smooth=0.1):
        """myvqvae.py:144-156: smooth-L1 plus lambda_smooth times the smooth-L1 of the first differences along time."""
        return F.smooth_l1_loss(x, y) + lambda_smooth * F.smooth_l1_loss(x[..., 1:] - x[..., :-1], y[..., 1:] - y[..., :-1])


for _cls in (Residual, ResidualStack, Encoder, Decoder, vqvae):
    _cls.__module__ = "model.pretrained.myvqvae"
