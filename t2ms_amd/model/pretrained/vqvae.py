"""Host-side mirror of the reference LA-VAE codec (model/pretrained/vqvae.py).

Class and attribute names equal the reference's, so its whole-module pickles (``final_model.pth``, loaded with
weights_only=False at infer.py:39 / train.py:22) resolve to these classes and their tensors are used as-is.  ``Encoder.forward``
and ``Decoder.forward`` run single-launch HIP kernels (t2s_vae.hip); the nn.Conv1d objects only hold weights.  The reference
freezes the VAE while training the DiT (train.py:31-33); with `usepretrainedvae` false the encoder trains and its backward is
t2s_vae_encode_backward.  LA-VAE pre-training (pretrained_lavae_unified.py, ``vqvae.shared_eval(..., "train")``) trains both
halves: the decoder's backward is t2s_vae_decode_backward (_DecodeFn), the losses are t2s_mse with its backward.  No CPU
fallback.  Everything but the reference's names, constructor signatures and argument rules is _lavae.py's, shared with the
multichannel myvqvae.py.
"""
import torch

from ... import _lib as L
from . import _lavae
from ._lavae import _DecodeFn, _EncodeFn  # noqa: F401  (the autograd nodes stay importable from here)
from .core import BaseModel


class Residual(_lavae.Residual):
    """vqvae.py:7-22."""


class ResidualStack(_lavae.ResidualStack):
    """vqvae.py:24-33."""

    _residual = Residual

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens):
        super().__init__(in_channels, num_hiddens, num_residual_layers, num_residual_hiddens)
        self._num_residual_layers = num_residual_layers


class Encoder(_lavae.Encoder):
    """vqvae.py:36-71 (the constructor is the shared one: the reference's signature)."""

    _stack, _entries = ResidualStack, ("t2s_vae_encode", "t2s_vae_encode_backward")

    def _width(self):
        return L.LAT_W

    def _series(self, x):
        """(B,L) or (B,1,L) in the codec's layout, (B,1,L): what the kernels and the torch ops read."""
        return x.reshape(x.shape[0], 1, x.shape[-1])

    def forward(self, inputs):
        """x (B,L) [or (B,1,L)] -> (z (B,64,30), before (B,64,L/4)); vqvae.py:57-71.  A trainable encoder (train.py:31-33 with
        `usepretrainedvae` false) on a covered shape runs forward and backward in the HIP kernels (_lavae._route)."""
        if not inputs.is_cuda:
            raise L.T2SError("Encoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        route = self._route_of(inputs, inputs.shape[-1])
        return self._forward_autograd(inputs) if route == "autograd" else self._forward_kernel(route, inputs)


class Decoder(_lavae.Decoder):
    """vqvae.py:74-105."""

    _stack, _entries = ResidualStack, ("t2s_vae_decode_w", "t2s_vae_decode_backward")

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens):
        super().__init__(in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, 1)

    def _recon_autograd(self, h, length):
        return torch.squeeze(h)

    def forward(self, inputs, length):
        """z (B,64,W) -> (recon, after (B,64,L/4)); vqvae.py:97-105 (W = 30 on the DiT path; any W <= 32, e.g. the L/4
        of the MLP-denoiser path, as F.interpolate accepts).  ``recon`` follows torch.squeeze's shape rule: (B,L), or
        (L,) when B == 1.  With grad enabled and a decoder parameter or the latent asking for a gradient (LA-VAE
        pre-training) the same forward kernel runs behind _DecodeFn, whose backward is t2s_vae_decode_backward; under
        no_grad or with everything frozen (infer.py, evaluation, the Sampler's C handle) nothing is saved."""
        if not inputs.is_cuda:
            raise L.T2SError("Decoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        if inputs.dim() != 3 or not 1 <= inputs.shape[2] <= 32:
            raise L.T2SError(f"Decoder.forward: latent must be (B,C,W) with W <= 32, got {tuple(inputs.shape)}")
        Ln = int(length / 4) * 4
        route = self._route_of(inputs, Ln, inputs.shape[2])
        if route == "autograd":
            return self._forward_autograd(inputs, length)
        recon, after = self._forward_kernel(route, inputs, Ln)
        return torch.squeeze(recon.unsqueeze(1)), after


class vqvae(BaseModel):
    """vqvae.py:108-142 (no vector quantiser despite the name)."""

    def __init__(self, args):
        super().__init__()
        self.encoder = Encoder(1, args.block_hidden_size, args.num_residual_layers, args.res_hidden_size,
                               args.embedding_dim)
        self.decoder = Decoder(args.embedding_dim, args.block_hidden_size, args.num_residual_layers,
                               args.res_hidden_size)

    def shared_eval(self, batch, optimizer, mode):  # pyright: ignore[reportIncompatibleMethodOverride]
        """vqvae.py:118-135.  'train' is one optimisation step of LA-VAE pre-training (pretrained_lavae_unified.py:142-174)
        entirely on the HIP kernels: encoder and decoder forward + backward (_EncodeFn, _DecodeFn), both MSE terms with their
        backward (_MseFn), and the caller's optimizer -- T2SAdamW in pretrain_lavae.py.  'val' / 'test' run under no_grad."""
        from ...train import mse_loss
        if mode == "train":
            optimizer.zero_grad()
            z, before = self.encoder(batch)
            data_recon, after = self.decoder(z, length=batch.shape[-1])
            recon_error = mse_loss(data_recon.reshape(batch.shape), batch)     # (B == 1: recon is (L,), torch.squeeze's rule)
            loss = recon_error + mse_loss(before, after)
            loss.backward()
            optimizer.step()
            return loss.detach(), recon_error.detach(), data_recon.detach(), z.detach()
        with torch.no_grad():
            z, before = self.encoder(batch)
            data_recon, after = self.decoder(z, length=batch.shape[-1])
            recon_error = mse_loss(data_recon.reshape(batch.shape), batch)
            loss = recon_error + mse_loss(before, after)
        return loss, recon_error, data_recon, z

    def forward(self, x):
        z, _ = self.encoder(x)
        return self.decoder(z, x.shape[-1])


for _cls in (Residual, ResidualStack, Encoder, Decoder, vqvae):
    _cls.__module__ = "model.pretrained.vqvae"
