"""Host-side mirror of the reference's attention seq2seq codec (model/pretrained/TSae.py, AttentionSeq2SeqAutoencoder): the
codec the motion pipeline's ``vae:`` block configures (flow_dim 64, d_ff 128, 3 + 3 layers, 8 heads, input_dim 10) and
``pretrained_mylavae.py`` trains and reconstructs with.

Class names, constructor signatures, attribute names and state-dict keys equal the reference's (the two ``pe`` buffers and the
``condition_fusion.*`` tensors included), so a state dict the reference saved loads with ``strict=True``.

Routing (``_route``): eval mode, no gradient wanted, no masks and a covered shape (d_model 64, 4 or 8 heads, d_ff a multiple of
64 up to 512, 1..6 layers, 1..16 features, 1 <= T <= 2000) run the HIP entries of csrc/t2s_tsae.hip -- ``encoder(x)`` is
t2s_tsae_encode, ``decoder(memory, target)`` t2s_tsae_decode, ``decoder.generate(memory)`` t2s_tsae_generate (all steps in one
launch, key/value cached); a CPU tensor on that route is a T2SError.  Everything else -- training mode (dropout), a gradient
wanted (``shared_eval(..., 'train')``), masks, the text-fusion path of ``forward()``, uncovered shapes, and everything under
``T2S_TSAE=torch`` (read at call time) -- runs the ``_forward_torch`` methods: torch ops on the same parameters, plumbing with
no throughput claim.

Training (``shared_eval(..., 'train')``) has an opt-in HIP engine: ``T2S_TSAE_TRAIN=hip`` (read at call time; default ``torch``)
or ``AttentionSeq2SeqAutoencoder.set_train_engine("hip")`` sends the teacher-forced step through csrc/t2s_tsae_train.hip -- one
autograd node over the taking-part parameters, t2s_tsae_train_forward / _backward, dropout from the library's Philox rule -- when
``_train_route`` says the call is covered (T <= 192, a GPU input that wants no gradient, every parameter trainable, one common
dropout p, no ``T2S_TSAE=torch``); everything else runs the torch-op line as before.  The loss and the optimizer stay torch's.
"""
import ctypes as C
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _handle as H
from ... import _lib as L
from .core import BaseModel


def _torch_forced():
    v = os.environ.get("T2S_TSAE", "") or "hip"
    if v not in ("hip", "torch"):
        raise L.T2SError(f"T2S_TSAE must be 'hip' or 'torch' (got {v!r})")
    return v == "torch"


def _covered(n_features, d_model, d_ff, heads, layers, T, B=1):
    return (d_model == L.TSAE_D_MODEL and heads in (4, 8) and d_ff % 64 == 0 and 64 <= d_ff <= L.TSAE_MAX_D_FF
            and 1 <= layers <= L.TSAE_MAX_LAYERS and 1 <= n_features <= L.TSAE_MAX_FEATURES and 1 <= T <= L.TSAE_MAX_T
            and 1 <= B <= 65535)


def _train_engine_env():
    v = os.environ.get("T2S_TSAE_TRAIN", "") or "torch"
    if v not in ("hip", "torch"):
        raise L.T2SError(f"T2S_TSAE_TRAIN must be 'hip' or 'torch' (got {v!r})")
    return v


def _train_route(engine, forced, covered, on_gpu, input_grad, params_grad, common_p, masks=False):
    """'hip' or 'torch' for one shared_eval(..., 'train') call: the HIP node only when every condition holds."""
    ok = (engine == "hip" and not forced and covered and on_gpu and not input_grad and params_grad and common_p is not None
          and not masks)
    return "hip" if ok else "torch"


def _route(training, grad, masks, covered, forced):
    """'hip' or 'torch' for one call: each condition alone sends the call to the torch ops."""
    return "torch" if (training or grad or masks or not covered or forced) else "hip"


class PositionalEncoding(nn.Module):
    """x + pe[:, :T], then dropout; pe (1, max_len, d_model) is a buffer of the state dict."""

    def __init__(self, d_model, max_len=5000, dropout=0.1):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float) * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term[: d_model // 2])
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return self.dropout(x + self.pe[:, : x.size(1), :])


class AdaLN(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.ln = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(nn.Linear(d_model, d_model * 4), nn.GELU(), nn.Linear(d_model * 4, d_model * 2))

    def forward(self, x, condition):
        gamma, beta = self.mlp(condition).chunk(2, dim=1)
        return gamma.unsqueeze(1) * self.ln(x) + beta.unsqueeze(1)


class AdaptiveLinear(nn.Module):
    """A Linear that reads the first in_dim columns of a (out, max_in) weight.  The fusion block's is (64, 393216): drawn in one
    uniform_ pass at the xavier bound."""

    def __init__(self, out_features, max_in_features=2048):
        super().__init__()
        a = math.sqrt(6.0 / (out_features + max_in_features))
        self.weight = nn.Parameter(torch.empty(out_features, max_in_features).uniform_(-a, a))
        self.bias = nn.Parameter(torch.zeros(out_features))

    def forward(self, x):
        return F.linear(x, self.weight[:, : x.size(-1)], self.bias)


def _xavier_(linear, zero_bias=True):
    nn.init.xavier_uniform_(linear.weight)
    if zero_bias:
        nn.init.zeros_(linear.bias)


class ConditionFusionModule(nn.Module):
    """Text-condition fusion (torch ops only; the reference's live paths skip it)."""

    def __init__(self, flow_dim=128, max_text_length=512, text_embedding_dim=768, dropout=0.1):
        super().__init__()
        self.flow_dim = flow_dim
        self.text_projection = AdaptiveLinear(out_features=flow_dim, max_in_features=max_text_length * text_embedding_dim)
        self.condition_projection = nn.Linear(flow_dim, flow_dim)
        _xavier_(self.condition_projection)
        self.fusion = nn.Sequential(nn.Linear(flow_dim * 2, flow_dim * 4), nn.ReLU(), nn.Dropout(dropout),
                                    nn.Linear(flow_dim * 4, flow_dim))
        for layer in self.fusion:
            if isinstance(layer, nn.Linear):
                _xavier_(layer)
        self.fusion_ln = nn.LayerNorm(flow_dim)
        self.ada_ln = AdaLN(flow_dim)

    def forward(self, encoder_output, text_embedding):
        B, T, _ = encoder_output.shape
        text_cond = self.text_projection(text_embedding.reshape(B, -1))
        combined = torch.cat([encoder_output, text_cond.unsqueeze(1).expand(-1, T, -1)], dim=-1)
        fused = self.fusion_ln(self.fusion(combined) + encoder_output)
        return self.ada_ln(fused, self.condition_projection(text_cond))


def _wb(prefix, module):
    return [(prefix + "_w", module.weight), (prefix + "_b", module.bias)]


def _layer_ptrs(dst, layer, attns, norms, keep):
    """One transformer layer into its struct: the attention blocks, the feed-forward pair, the norms."""
    for a in attns:
        attn = getattr(layer, a)
        H.fill(getattr(dst, a), [("in_proj_w", attn.in_proj_weight), ("in_proj_b", attn.in_proj_bias),
                                 *_wb("out_proj", attn.out_proj)], keep)
    for n in ("linear1", "linear2") + norms:
        H.fill(dst, _wb(n, getattr(layer, n)), keep)


class _Side(H.HandleOwner, nn.Module):
    """What TimeSeriesEncoder and TimeSeriesDecoder share: a one-sided library handle cached against the parameters' storage and
    version, and the module-owned workspace (both _handle.HandleOwner's)."""

    def _layers(self):
        raise NotImplementedError

    def _shape(self):
        """(n_features, d_model, d_ff, heads, layers) as the modules hold them."""
        layers = self._layers()
        l0 = layers[0]
        return (int(self.n_features), int(self.flow_dim), int(l0.linear1.out_features), int(l0.self_attn.num_heads), len(layers))

    def _plain(self):
        """The layer options the kernels implement: pre-norm, ReLU, eps 1e-5 (what the constructors below set)."""
        return all(l.norm_first and l.norm1.eps == 1e-5 and getattr(l, "activation_relu_or_gelu", 1) == 1 for l in self._layers())

    def _route_of(self, x, T, masks, B=1):
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        F_, d, dff, heads, layers = self._shape()
        covered = x.dim() == 3 and self._plain() and _covered(F_, d, dff, heads, layers, T, B)
        return _route(self.training, grad, masks, covered, _torch_forced())

    def _build(self, device):
        w, keep = self._weights_struct()          # (the library packs its own copy: `keep` ends with this call)
        return H.Handle(device, "t2s_tsae_create", "t2s_tsae_destroy", C.byref(w))

    def _handle(self, device):
        """The handle object (HandleOwner._owned_handle).  Any change rebuilds: the one-sided handles serve inference; the
        refresh entry (t2s_tsae_update_weights) is the autoencoder's training handle's."""
        device = torch.device(device)
        ts = list(self.parameters())
        H.require_on(ts, device, "TSae")
        geometry = (device,) + tuple(tuple(t.shape) for t in ts)
        return self._owned_handle(device, geometry, H.stamp_of(ts), self._build, None, device)

    def _workspace_for(self, h, B, T, device):
        need = int(L.lib().t2s_tsae_workspace_bytes(h.ptr, B, T))
        if need == 0:
            raise L.T2SError("TSae: " + L.lib().t2s_last_error().decode("utf-8", "replace"))
        return self._workspace(need, device)

    def _gpu(self, who, *tensors):
        for t in tensors:
            if not t.is_cuda:
                raise L.T2SError(f"{who}: input must live on a GPU (got device {t.device}); the HIP path has no CPU fallback "
                                 f"(T2S_TSAE=torch selects the torch ops)")


class TimeSeriesEncoder(_Side):
    def __init__(self, n_features, flow_dim=128, num_layers=6, d_ff=2048, num_heads=8, dropout=0.1, max_seq_len=2000):
        super().__init__()
        self.num_layers, self.flow_dim, self.n_features = num_layers, flow_dim, n_features
        self.value_embedding = nn.Linear(n_features, flow_dim)
        _xavier_(self.value_embedding)
        self.embedding_dropout = nn.Dropout(p=dropout)
        self.embedding_ln = nn.LayerNorm(flow_dim)
        self.positional_encoding = PositionalEncoding(d_model=flow_dim, max_len=max_seq_len, dropout=dropout)
        layer = nn.TransformerEncoderLayer(d_model=flow_dim, nhead=num_heads, dim_feedforward=d_ff, dropout=dropout,
                                           batch_first=True, norm_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False)

    def _layers(self):
        return self.transformer_encoder.layers

    def _weights_struct(self):
        F_, d, dff, heads, n = self._shape()
        w, keep = L.TsaeWeights(), []
        w.n_features, w.d_model, w.d_ff, w.heads, w.n_enc, w.n_dec = F_, d, dff, heads, n, 0
        H.fill(w, _wb("value_embedding", self.value_embedding) + _wb("embedding_ln", self.embedding_ln), keep)
        for i, layer in enumerate(self._layers()):
            _layer_ptrs(w.enc[i], layer, ("self_attn",), ("norm1", "norm2"), keep)
        return w, keep

    def forward(self, time_series, src_key_padding_mask=None):
        """x (B,T,F) -> memory (B,T,flow_dim)."""
        T = time_series.shape[1] if time_series.dim() == 3 else 0
        B = time_series.shape[0] if time_series.dim() == 3 else 0
        if self._route_of(time_series, T, src_key_padding_mask is not None, B) == "torch":
            return self._forward_torch(time_series, src_key_padding_mask)
        self._gpu("TimeSeriesEncoder.forward", time_series)
        x = L.as_f32(time_series)
        dev = x.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            ws = self._workspace_for(h, B, T, dev)
            memory = torch.empty(B, T, L.TSAE_D_MODEL, dtype=torch.float32, device=dev)
            L.check(L.lib().t2s_tsae_encode(h.ptr, x.data_ptr(), memory.data_ptr(), B, T, ws.data_ptr(), ws.numel(),
                                            L.stream_ptr(dev)), "t2s_tsae_encode")
        return memory

    def _forward_torch(self, time_series, src_key_padding_mask=None):
        """The same forward as torch ops on the same parameters (autograd, dropout in training mode, masks)."""
        e = self.embedding_ln(self.embedding_dropout(self.value_embedding(time_series)))
        return self.transformer_encoder(self.positional_encoding(e), src_key_padding_mask=src_key_padding_mask)


class TimeSeriesDecoder(_Side):
    def __init__(self, n_features, num_layers=6, d_ff=2048, num_heads=8, dropout=0.1, max_seq_len=2000, flow_dim=128):
        super().__init__()
        self.max_seq_len, self.flow_dim, self.n_features = max_seq_len, flow_dim, n_features
        self.positional_encoding = PositionalEncoding(d_model=flow_dim, max_len=max_seq_len, dropout=dropout)
        layer = nn.TransformerDecoderLayer(d_model=flow_dim, nhead=num_heads, dim_feedforward=d_ff, dropout=dropout,
                                           batch_first=True, norm_first=True)
        self.transformer_decoder = nn.TransformerDecoder(layer, num_layers=num_layers)
        self.output_projection = nn.Linear(flow_dim, n_features)
        self.input_projection = nn.Linear(n_features, flow_dim)
        nn.init.xavier_uniform_(self.input_projection.weight)

    def _layers(self):
        return self.transformer_decoder.layers

    def _weights_struct(self):
        F_, d, dff, heads, n = self._shape()
        w, keep = L.TsaeWeights(), []
        w.n_features, w.d_model, w.d_ff, w.heads, w.n_enc, w.n_dec = F_, d, dff, heads, 0, n
        H.fill(w, _wb("input_projection", self.input_projection) + _wb("output_projection", self.output_projection), keep)
        for i, layer in enumerate(self._layers()):
            _layer_ptrs(w.dec[i], layer, ("self_attn", "multihead_attn"), ("norm1", "norm2", "norm3"), keep)
        return w, keep

    def _generate_causal_mask(self, size, device):
        return torch.triu(torch.ones(size, size, device=device), diagonal=1).bool()

    def _memory_ok(self, memory, T):
        return memory.dim() == 3 and memory.shape[1] == T and memory.shape[2] == L.TSAE_D_MODEL

    def forward(self, memory, target_seq, tgt_key_padding_mask=None):
        """Teacher forcing: memory (B,T,flow_dim), target (B,T,F) -> prediction (B,T,F)."""
        B, T = (target_seq.shape[0], target_seq.shape[1]) if target_seq.dim() == 3 else (0, 0)
        route = self._route_of(target_seq, T, tgt_key_padding_mask is not None, B)
        if route == "hip" and (memory.requires_grad and torch.is_grad_enabled() or not self._memory_ok(memory, T)
                               or memory.shape[0] != B):
            route = "torch"
        if route == "torch":
            return self._forward_torch(memory, target_seq, tgt_key_padding_mask)
        self._gpu("TimeSeriesDecoder.forward", memory, target_seq)
        mem, tgt = L.as_f32(memory), L.as_f32(target_seq)
        dev = tgt.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            ws = self._workspace_for(h, B, T, dev)
            pred = torch.empty(B, T, int(self.n_features), dtype=torch.float32, device=dev)
            L.check(L.lib().t2s_tsae_decode(h.ptr, mem.data_ptr(), tgt.data_ptr(), pred.data_ptr(), B, T, ws.data_ptr(),
                                            ws.numel(), L.stream_ptr(dev)), "t2s_tsae_decode")
        return pred

    def _forward_torch(self, memory, target_seq, tgt_key_padding_mask=None):
        B, T, _ = target_seq.shape
        emb = self.input_projection(target_seq)
        bos = torch.zeros(B, 1, self.flow_dim, device=target_seq.device, dtype=emb.dtype)
        tgt = self.positional_encoding(torch.cat([bos, emb[:, :-1, :]], dim=1))
        out = self.transformer_decoder(tgt, memory, tgt_mask=self._generate_causal_mask(T, target_seq.device),
                                       tgt_key_padding_mask=tgt_key_padding_mask)
        return self.output_projection(out)

    def generate(self, memory):
        """Autoregressive generation: memory (B,S,flow_dim) -> series (B,S,F)."""
        B, S = (memory.shape[0], memory.shape[1]) if memory.dim() == 3 else (0, 0)
        if self._route_of(memory, S, False, B) == "torch" or not self._memory_ok(memory, S):
            return self._generate_torch(memory)
        self._gpu("TimeSeriesDecoder.generate", memory)
        mem = L.as_f32(memory)
        dev = mem.device
        with torch.cuda.device(dev):
            h = self._handle(dev)
            ws = self._workspace_for(h, B, S, dev)
            series = torch.empty(B, S, int(self.n_features), dtype=torch.float32, device=dev)
            L.check(L.lib().t2s_tsae_generate(h.ptr, mem.data_ptr(), series.data_ptr(), B, S, ws.data_ptr(), ws.numel(),
                                              L.stream_ptr(dev)), "t2s_tsae_generate")
        return series

    def _generate_torch(self, memory):
        """The same generation as torch ops: the whole stack over the growing prefix at every step (no cache)."""
        B, S = memory.size(0), memory.size(1)
        dec_in = torch.zeros(B, 1, self.flow_dim, device=memory.device, dtype=memory.dtype)
        steps = []
        for _ in range(S):
            mask = self._generate_causal_mask(dec_in.size(1), memory.device)
            out = self.transformer_decoder(self.positional_encoding(dec_in), memory, tgt_mask=mask)
            pred = self.output_projection(out[:, -1:, :])
            steps.append(pred)
            dec_in = torch.cat([dec_in, self.input_projection(pred)], dim=1)
        return torch.cat(steps, dim=1)


def _two_sided_fields(w, enc, dec):
    """[(struct, field, parameter)] of every tensor that takes part in the teacher-forced step, in t2s_tsae_weights order."""
    out = [(w, f, p) for f, p in _wb("value_embedding", enc.value_embedding) + _wb("embedding_ln", enc.embedding_ln)]

    def layer(dst, mod, attns, norms):
        for a in attns:
            attn, d = getattr(mod, a), getattr(dst, a)
            out.extend([(d, "in_proj_w", attn.in_proj_weight), (d, "in_proj_b", attn.in_proj_bias),
                        (d, "out_proj_w", attn.out_proj.weight), (d, "out_proj_b", attn.out_proj.bias)])
        for n in ("linear1", "linear2") + norms:
            out.extend((dst, f, p) for f, p in _wb(n, getattr(mod, n)))

    for i, mod in enumerate(enc._layers()):
        layer(w.enc[i], mod, ("self_attn",), ("norm1", "norm2"))
    for i, mod in enumerate(dec._layers()):
        layer(w.dec[i], mod, ("self_attn", "multihead_attn"), ("norm1", "norm2", "norm3"))
    out.extend((w, f, p) for f, p in _wb("input_projection", dec.input_projection) + _wb("output_projection", dec.output_projection))
    return out


class _TrainStep(torch.autograd.Function):
    """prediction = decoder(encoder(x), x) on t2s_tsae_train_forward, its backward on t2s_tsae_train_backward.  The activations
    live in the model's workspace between the two: a backward after another forward of the same model is refused."""

    @staticmethod
    def forward(ctx, model, x, p, seed, *params):
        dev = x.device
        B, T, F_ = x.shape
        with torch.cuda.device(dev):
            h = model._train_handle(dev)
            need = int(L.lib().t2s_tsae_train_workspace_bytes(h.ptr, B, T))
            if need == 0:
                raise L.T2SError("TSae: " + L.lib().t2s_last_error().decode("utf-8", "replace"))
            ws = model._workspace(need, dev)
            pred = torch.empty(B, T, F_, dtype=torch.float32, device=dev)
            L.check(L.lib().t2s_tsae_train_forward(h.ptr, x.data_ptr(), pred.data_ptr(), B, T, p, seed, ws.data_ptr(), ws.numel(),
                                                   L.stream_ptr(dev)), "t2s_tsae_train_forward")
        model.__dict__["_t2s_train_token"] = token = model.__dict__.get("_t2s_train_token", 0) + 1
        ctx.model, ctx.x, ctx.p, ctx.seed, ctx.h, ctx.ws, ctx.token = model, x, p, seed, h, ws, token
        return pred

    @staticmethod
    def backward(ctx, d_pred):  # pyright: ignore[reportIncompatibleMethodOverride]
        model, x, h, ws = ctx.model, ctx.x, ctx.h, ctx.ws
        if model.__dict__.get("_t2s_train_token") != ctx.token or model.__dict__.get("_t2s_h") is not h:
            raise L.T2SError("TSae: backward of a training step whose workspace a later forward of the same model has overwritten")
        dev = x.device
        B, T, _ = x.shape
        d_pred = L.as_f32(d_pred)
        g, grads = L.TsaeWeights(), []
        for dst, field, prm in _two_sided_fields(g, model.encoder, model.decoder):
            grads.append(torch.empty(prm.shape, dtype=torch.float32, device=dev))
            setattr(dst, field, grads[-1].data_ptr())
        with torch.cuda.device(dev):
            L.check(L.lib().t2s_tsae_train_backward(h.ptr, x.data_ptr(), d_pred.data_ptr(), C.byref(g), B, T, ctx.p, ctx.seed,
                                                    ws.data_ptr(), ws.numel(), L.stream_ptr(dev)), "t2s_tsae_train_backward")
        return (None, None, None, None, *grads)


class AttentionSeq2SeqAutoencoder(H.HandleOwner, BaseModel):
    def __init__(self, args):
        super().__init__()
        self.n_features, self.flow_dim = args.input_dim, args.flow_dim
        self.encoder = TimeSeriesEncoder(n_features=args.input_dim, flow_dim=args.flow_dim, num_layers=args.num_encoder_layers,
                                         d_ff=args.d_ff, num_heads=args.num_heads)
        self.condition_fusion = ConditionFusionModule(flow_dim=args.flow_dim)
        self.decoder = TimeSeriesDecoder(n_features=args.input_dim, flow_dim=args.flow_dim, num_layers=args.num_decoder_layers,
                                         d_ff=args.d_ff, num_heads=args.num_heads)

    def forward(self, time_series, text_embedding, src_key_padding_mask=None, tgt_key_padding_mask=None):
        """Encoder, text fusion, teacher-forced decoder.  The fusion block is torch ops, so the whole path is."""
        x = self.encoder._forward_torch(time_series, src_key_padding_mask)
        x = self.condition_fusion(x, text_embedding)
        return self.decoder._forward_torch(x, time_series, tgt_key_padding_mask)

    def forward_inference(self, time_series, text_embedding, target_length=None, src_key_padding_mask=None):
        """Encoder, then autoregressive generation at the input's length (the text and target_length are not used)."""
        return self.decoder.generate(memory=self.encoder(time_series, src_key_padding_mask=src_key_padding_mask))

    # ---- the opt-in HIP training engine ----------------------------------------------------------------------------------
    def set_train_engine(self, engine):
        """'hip' or 'torch' for shared_eval(..., 'train'), overriding T2S_TSAE_TRAIN; None hands the choice back to it."""
        if engine not in ("hip", "torch", None):
            raise L.T2SError(f"set_train_engine: 'hip', 'torch' or None (got {engine!r})")
        self.__dict__["_t2s_train_engine"] = engine

    def _train_engine(self):
        return self.__dict__.get("_t2s_train_engine") or _train_engine_env()

    def _train_params(self):
        return [p for _, _, p in _two_sided_fields(L.TsaeWeights(), self.encoder, self.decoder)]

    def _common_dropout(self):
        """The one dropout probability of every nn.Dropout of the two sides and of their attention modules, or None."""
        ps = set()
        for side in (self.encoder, self.decoder):
            for m in side.modules():
                if isinstance(m, nn.Dropout):
                    ps.add(float(m.p))
                elif isinstance(m, nn.MultiheadAttention):
                    ps.add(float(m.dropout))
        return ps.pop() if len(ps) == 1 else None

    def _train_conditions(self, batch, masks=False):
        """What _train_route weighs for one 'train' call on `batch`, as its keyword arguments."""
        shapes = (self.encoder._shape(), self.decoder._shape())
        B, T = (batch.shape[0], batch.shape[1]) if batch.dim() == 3 else (0, 0)
        covered = (batch.dim() == 3 and shapes[0][:4] == shapes[1][:4] and self.encoder._plain() and self.decoder._plain()
                   and all(_covered(*s, T, B) for s in shapes) and T <= L.TSAE_TRAIN_MAX_T and batch.shape[2] == shapes[0][0]
                   and self.encoder.training == self.decoder.training == self.training)
        return dict(engine=self._train_engine(), forced=_torch_forced(), covered=covered, on_gpu=batch.is_cuda,
                    input_grad=batch.requires_grad, params_grad=torch.is_grad_enabled() and all(p.requires_grad for p in self._train_params()),
                    common_p=self._common_dropout(), masks=masks)

    def _weights_struct(self):
        F_, d, dff, heads, n_enc = self.encoder._shape()
        w, keep = L.TsaeWeights(), []
        w.n_features, w.d_model, w.d_ff, w.heads, w.n_enc, w.n_dec = F_, d, dff, heads, n_enc, self.decoder._shape()[4]
        for dst, field, prm in _two_sided_fields(w, self.encoder, self.decoder):
            H.fill(dst, [(field, prm)], keep)
        return w, keep

    def _build(self, device):
        w, keep = self._weights_struct()          # (the library packs its own copy: `keep` ends with this call)
        return H.Handle(device, "t2s_tsae_create", "t2s_tsae_destroy", C.byref(w))

    def _refresh(self, h, device):
        """The parameters moved (an optimizer step): one launch re-packs them on the caller's stream; the sources stay alive on
        the handle until the next refresh."""
        w, keep = self._weights_struct()
        with torch.cuda.device(device):
            L.check(L.lib().t2s_tsae_update_weights(h.ptr, C.byref(w), L.stream_ptr(device)), "t2s_tsae_update_weights")
        return keep

    def _train_handle(self, device):
        """The two-sided handle (HandleOwner._owned_handle): rebuilt when a shape changes, refreshed when only versions did."""
        device = torch.device(device)
        ts = self._train_params()
        H.require_on(ts, device, "TSae")
        geometry = (device, self.encoder._shape()[3]) + tuple(tuple(t.shape) for t in ts)
        return self._owned_handle(device, geometry, H.stamp_of(ts), self._build, self._refresh, device)

    def _train_forward_hip(self, batch):
        """One draw of torch's default CPU generator seeds the step's dropout: seed_everything governs a run, nothing synchronises."""
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        p = float(self._common_dropout()) if self.training else 0.0
        return _TrainStep.apply(self, L.as_f32(batch.detach()), p, seed, *self._train_params())

    def shared_eval(self, batch, text_embedding, optimizer, mode):  # pyright: ignore[reportIncompatibleMethodOverride]
        """'train': one teacher-forced optimisation step -- torch ops under autograd, or the HIP node where the training engine is
        'hip' and _train_route takes it; 'val' / 'test': eval mode, no_grad, encode + generate on the HIP entries.  Returns
        (loss, reconstruction)."""
        if mode == "train":
            optimizer.zero_grad()
            if _train_route(**self._train_conditions(batch)) == "hip":
                recon = self._train_forward_hip(batch)
            else:
                recon = self.decoder(memory=self.encoder(batch), target_seq=batch)
            loss = F.mse_loss(recon, batch)
            loss.backward()
            optimizer.step()
        elif mode in ("val", "test"):
            self.eval()
            with torch.no_grad():
                recon = self.forward_inference(batch, text_embedding)
                loss = F.mse_loss(recon, batch)
        else:
            raise L.T2SError(f"shared_eval: mode must be 'train', 'val' or 'test' (got {mode!r})")
        return loss, recon


for _cls in (PositionalEncoding, AdaLN, TimeSeriesEncoder, AdaptiveLinear, ConditionFusionModule, TimeSeriesDecoder,
             AttentionSeq2SeqAutoencoder):
    _cls.__module__ = "model.pretrained.TSae"
