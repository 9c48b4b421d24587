"""CPU restatement of the TSae codec's three computations in plain tensor ops (no nn.Transformer*): encode, the teacher-forced
decode, and generation with an EXPLICIT key/value cache -- the independent witness that caching is exact (in eval mode under a
causal mask an earlier position never changes once written).  Runs in the dtype of the state dict handed in (fp32 or fp64).

A state dict is the reference's (synth.make_tsae_state_dict); `heads` is not derivable from shapes and is passed."""
import math

import torch

EPS = 1e-5


def sinusoid_table(max_len, d_model=64, dtype=torch.float32):
    """pe[p, 2i] = sin(p * w_i), pe[p, 2i+1] = cos(p * w_i), w_i = exp(2i * -(ln 10000 / d_model)); the divisor and the angle are
    formed in fp32 (the reference's buffer is), the result is cast to `dtype`."""
    pos = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
    pe = torch.zeros(max_len, d_model)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.to(dtype)


def _ln(x, sd, name):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * sd[name + ".weight"] + sd[name + ".bias"]


def _lin(x, sd, name):
    return x @ sd[name + ".weight"].T + sd[name + ".bias"]


def _n_layers(sd, prefix):
    return len({k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)})


def _split_heads(t, heads):
    B, T, D = t.shape
    return t.reshape(B, T, heads, D // heads).transpose(1, 2)            # (B,H,T,dh)


def _attend(q, k, v, heads, causal):
    """q (B,Tq,64), k / v (B,Tk,64) already projected -> (B,Tq,64); causal: query i sees keys 0..i + (Tk - Tq)."""
    qh, kh, vh = (_split_heads(t, heads) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    if causal:
        Tq, Tk = s.shape[-2:]
        keep = torch.arange(Tk).unsqueeze(0) <= torch.arange(Tq).unsqueeze(1) + (Tk - Tq)
        s = s.masked_fill(~keep, float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(q.shape)


def _qkv(x, sd, name, rows):
    w, b = sd[name + ".in_proj_weight"], sd[name + ".in_proj_bias"]
    return x @ w[rows].T + b[rows]


Q, K, V = slice(0, 64), slice(64, 128), slice(128, 192)


def _table(pe, T, dt):
    """Rows 0..T-1 of the positional table: the caller's `pe` (at least T rows of 64), or the one formed here."""
    return sinusoid_table(T, 64, dt) if pe is None else pe[:T].to(dt)


def encode(sd, x, heads, pe=None):
    """x (B,T,F) -> memory (B,T,64).  `pe`: a positional table (rows >= T, 64) to use instead of sinusoid_table."""
    dt = sd["encoder.value_embedding.weight"].dtype
    x = x.to(dt)
    h = _ln(_lin(x, sd, "encoder.value_embedding"), sd, "encoder.embedding_ln") + _table(pe, x.shape[1], dt)
    for i in range(_n_layers(sd, "encoder.transformer_encoder.layers.")):
        p = f"encoder.transformer_encoder.layers.{i}."
        n = _ln(h, sd, p + "norm1")
        a = _attend(_qkv(n, sd, p + "self_attn", Q), _qkv(n, sd, p + "self_attn", K), _qkv(n, sd, p + "self_attn", V), heads, False)
        h = h + _lin(a, sd, p + "self_attn.out_proj")
        h = h + _lin(torch.relu(_lin(_ln(h, sd, p + "norm2"), sd, p + "linear1")), sd, p + "linear2")
    return h


def _dec_layers(sd):
    return _n_layers(sd, "decoder.transformer_decoder.layers.")


def _dec_rows(sd, rows, memory_kv, cache, heads):
    """Decoder stack on the NEW rows (B,n,64) given the cache of earlier rows' self-attention K / V per layer (list of (K, V),
    extended in place) and the memory's cross K / V per layer."""
    h = rows
    for i in range(_dec_layers(sd)):
        p = f"decoder.transformer_decoder.layers.{i}."
        n = _ln(h, sd, p + "norm1")
        k_new, v_new = _qkv(n, sd, p + "self_attn", K), _qkv(n, sd, p + "self_attn", V)
        k_all = k_new if cache[i] is None else torch.cat([cache[i][0], k_new], dim=1)
        v_all = v_new if cache[i] is None else torch.cat([cache[i][1], v_new], dim=1)
        cache[i] = (k_all, v_all)
        a = _attend(_qkv(n, sd, p + "self_attn", Q), k_all, v_all, heads, True)
        h = h + _lin(a, sd, p + "self_attn.out_proj")
        n = _ln(h, sd, p + "norm2")
        a = _attend(_qkv(n, sd, p + "multihead_attn", Q), memory_kv[i][0], memory_kv[i][1], heads, False)
        h = h + _lin(a, sd, p + "multihead_attn.out_proj")
        h = h + _lin(torch.relu(_lin(_ln(h, sd, p + "norm3"), sd, p + "linear1")), sd, p + "linear2")
    return _lin(h, sd, "decoder.output_projection")


def _memory_kv(sd, memory):
    return [(_qkv(memory, sd, f"decoder.transformer_decoder.layers.{i}.multihead_attn", K),
             _qkv(memory, sd, f"decoder.transformer_decoder.layers.{i}.multihead_attn", V)) for i in range(_dec_layers(sd))]


def decode(sd, memory, target, heads, pe=None):
    """Teacher forcing: memory (B,T,64), target (B,T,F) -> prediction (B,T,F); all rows at once (an empty cache)."""
    dt = sd["decoder.input_projection.weight"].dtype
    memory, target = memory.to(dt), target.to(dt)
    B, T, _ = target.shape
    rows = torch.cat([torch.zeros(B, 1, 64, dtype=dt), _lin(target, sd, "decoder.input_projection")[:, :-1]], dim=1)
    rows = rows + _table(pe, T, dt)
    return _dec_rows(sd, rows, _memory_kv(sd, memory), [None] * _dec_layers(sd), heads)


def generate(sd, memory, heads, pe=None):
    """Autoregressive generation with a key/value cache: memory (B,S,64) -> series (B,S,F); step t computes ONE new row."""
    dt = sd["decoder.input_projection.weight"].dtype
    memory = memory.to(dt)
    B, S, _ = memory.shape
    pe = _table(pe, S, dt)
    mkv, cache = _memory_kv(sd, memory), [None] * _dec_layers(sd)
    row, out = torch.zeros(B, 1, 64, dtype=dt), []
    for t in range(S):
        pred = _dec_rows(sd, row + pe[t], mkv, cache, heads)
        out.append(pred)
        row = _lin(pred, sd, "decoder.input_projection")
    return torch.cat(out, dim=1)
