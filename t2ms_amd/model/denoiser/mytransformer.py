"""Host-side mirror of the T2MS fork's denoiser (model/denoiser/mytransformer.py): ``Transformer(dim)``.

The fork's network is the reference DiT with one change -- ``self.H = dim``, the latent width: the latent is (B,64,dim),
patchified 2x2 into 16 * dim tokens, and ``pos_embed`` has 16 * dim rows.  Its deadlift model uses dim 50 (800 tokens), its
bench-press model dim 64 (1024).  State-dict keys, block count, width and heads are those of
``model.denoiser.transformer.Transformer``, which is this class at dim 30: one class body (handle management, locking,
pairing, the no-grad forward) serves both, and ``forward`` runs the HIP kernels of libt2s_hip.so through a handle made by
t2s_dit_create_w.  Out of the box the wide widths run the f32 arithmetic and inference only; ``set_trainable(True)`` opts a
model into the fp32 training step, ``set_wide_math(True)`` into bf16x3 / bf16 inference.  Wide bf16 training
and a ragged backward stay refused.
"""
from __future__ import annotations

from . import transformer as _t
from .transformer import (InverseLatentEmbedding, LatentEmbedding, TimeEmbedding, Transformerlayer,  # noqa: F401
                          get_sinusoidal_positional_embeddings, modulate)

__all__ = ["Transformer", "Transformerlayer", "TimeEmbedding", "modulate",
           "get_sinusoidal_positional_embeddings", "InverseLatentEmbedding", "LatentEmbedding"]


class Transformer(_t.Transformer):
    """Drop-in for ``model.denoiser.mytransformer.Transformer`` (mytransformer.py:128-204): `dim` is required, as there."""

    def __init__(self, dim):
        super().__init__(dim)


Transformer.__module__ = "model.denoiser.mytransformer"   # pickles stay loadable by the fork and vice versa
