"""Host-side mirror of the reference's multichannel LA-VAE codec (model/pretrained/myvqvae.py), the codec of the T2MS
motion models: C-channel series (7 deadlift, 10 bench press), latent width ``flow_dim``, any length L >= 8.

Class names, constructor signatures, attribute names and state-dict keys equal the reference's, so a plain state dict
(myinfer.py:126-128, mytrain.py:29-30) and a whole-module pickle both load.  Under no_grad ``Encoder.forward`` and
``Decoder.forward`` run the single-launch HIP kernels t2s_vae_encode_mc / t2s_vae_decode_mc (csrc/t2s_vae.hip): C <= 16,
flow_dim <= 64, hidden <= 128, res_hidden <= 256, <= 4 residual layers, embedding_dim 64.  No CPU fallback.
``Encoder.encode_ragged`` / ``Decoder.decode_ragged`` (_lavae.py) take clips of unequal length in one launch each
(t2s_vae_encode_mc_ragged / t2s_vae_decode_mc_ragged; inference only).

With grad enabled and a parameter or the latent asking for a gradient, a covered shape (``_mc_backward_covers``: hidden 128,
embedding_dim 64, res_hidden 128 / 256, 1..4 residual layers, 8 <= L <= 192, flow_dim <= 64, C <= 16) runs the same HIP forward
behind the autograd nodes (_EncodeFn, _DecodeFn), whose backward is t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc:
``vqvae.shared_eval(..., 'train')`` and a trainable encoder grafted onto the DiT (mytrain.py:37-40) train on HIP.  Everything
else -- and everything under ``T2S_MVAE_BACKWARD=torch`` -- runs as torch ops under autograd (``_forward_autograd``).
All but the reference's names, constructor signatures and argument rules is _lavae.py's, shared with the single-channel vqvae.py.
"""
import torch
import torch.nn.functional as F

from ... import _lib as L
from . import _lavae
from ._lavae import _backward_covers as _mc_backward_covers, _backward_mode  # noqa: F401  (this family's predicate and switch)
from .core import BaseModel


class Residual(_lavae.Residual):
    """myvqvae.py:6-17."""


class ResidualStack(_lavae.ResidualStack):
    """myvqvae.py:19-30."""

    _residual = Residual


class Encoder(_lavae.Encoder):
    """myvqvae.py:32-61."""

    _stack, _entries = ResidualStack, ("t2s_vae_encode_mc", "t2s_vae_encode_backward_mc")

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, embedding_dim, flow_dim):
        super().__init__(in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, embedding_dim)
        self.flow_dim = flow_dim

    @property
    def channels(self):
        return self._conv_1.in_channels

    def _width(self):
        return int(self.flow_dim)

    def _series(self, x):
        """(B,C,L) is the codec's layout already."""
        return x

    def forward(self, inputs):
        """x (B,C,L) -> (z (B,64,flow_dim), before (B,64,L//4)); myvqvae.py:49-61."""
        if not inputs.is_cuda:
            raise L.T2SError("Encoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        if inputs.dim() != 3 or inputs.shape[1] != self._conv_1.in_channels:
            raise L.T2SError(f"Encoder.forward: input must be (B,{self._conv_1.in_channels},L), got {tuple(inputs.shape)}")
        route = self._route_of(inputs, inputs.shape[2])
        return self._forward_autograd(inputs) if route == "autograd" else self._forward_kernel(route, inputs)


class Decoder(_lavae.Decoder):
    """myvqvae.py:63-86."""

    _stack, _entries = ResidualStack, ("t2s_vae_decode_mc", "t2s_vae_decode_backward_mc")

    def __init__(self, in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, out_channels=52):
        super().__init__(in_channels, num_hiddens, num_residual_layers, num_residual_hiddens, out_channels)

    @property
    def channels(self):
        return self._conv_trans_2.out_channels

    def _recon_autograd(self, h, length):
        return F.interpolate(h, size=length, mode="linear", align_corners=True)

    def forward(self, inputs, length):
        """z (B,64,W) -> (recon (B,C,length), after (B,64,length//4)); myvqvae.py:76-86.  No squeeze: (B,C,length) also for
        B = 1 or C = 1."""
        if not inputs.is_cuda:
            raise L.T2SError("Decoder.forward: input must live on a GPU; the HIP path has no CPU fallback")
        if inputs.dim() != 3 or inputs.shape[1] != self._conv_1.in_channels:
            raise L.T2SError(f"Decoder.forward: latent must be (B,{self._conv_1.in_channels},W), got {tuple(inputs.shape)}")
        route = self._route_of(inputs, int(length), inputs.shape[2])
        return self._forward_autograd(inputs, length) if route == "autograd" else self._forward_kernel(route, inputs, int(length))


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
