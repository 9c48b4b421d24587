"""The TSae codec's teacher-forced TRAINING forward, prediction = decoder(memory = encoder(x), target_seq = x), restated in plain
tensor ops with an explicit keep-mask per dropout site, for tests/test_tsae_train_host.py and tests/test_tsae_train.py.  Runs in
the dtype of the state dict handed in, under torch autograd.

Holds the one site table (include/t2s.h has the same), the mask builder -- every site's mask for (seed, p, B, T, shape) from
oracle.t2s_oracle.device_uniform, i.e. the rule the kernels evaluate -- and the case table.  Nothing here is recorded."""
import collections
import functools
import math

import numpy as np
import torch

import _tsae_ref as R
from oracle import t2s_oracle as O
from t2ms_amd import synth

Case = collections.namedtuple("Case", "name n_features d_ff n_enc n_dec heads B T p")

CASES = (
    Case("A", 10, 128, 3, 3, 8, 3, 36, 0.0),
    Case("B", 10, 128, 3, 3, 8, 3, 36, 0.1),
    Case("C", 5, 64, 1, 1, 4, 2, 33, 0.1),       # a partial 32-row tile
    Case("D", 1, 64, 1, 1, 8, 1, 1, 0.0),        # the BOS row alone
    Case("E", 16, 512, 2, 2, 8, 2, 144, 0.1),    # the widest F and d_ff, at bench press's length
    Case("F", 7, 128, 3, 3, 8, 2, 192, 0.1),     # the ceiling
    Case("G", 3, 64, 6, 6, 4, 2, 31, 0.25),      # the deepest
    Case("H", 10, 128, 3, 3, 8, 5, 65, 0.1),     # one key past a 64-key chunk, an odd B
)
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

FWD_BAR = 1e-5          # forward: FWD_BAR * max(1, max|ref|)  (tests/_tsae_cases.py)
GRAD_BAR = 2e-4         # backward: GRAD_BAR * max|g_fp64| per tensor (tests/test_mvae_backward.py, the MLP backward)
LOSS_RTOL = 2e-5
MIN_GRAD = 1e-4         # every compared gradient tensor has at least this max|g| in fp64
KINK_MARGIN = 1e-6      # no FFN pre-activation of a case is nearer to zero than this in fp64 (min_preactivation below)

# ---- the site table -----------------------------------------------------------------------------------------------------------
ENC_EMB, ENC_POS, DEC_POS = 0, 1, 2


def enc_site(layer, k):
    """k: 0 attention probabilities, 1 after attention, 2 FFN hidden, 3 after FFN."""
    return 16 + 4 * layer + k


def dec_site(layer, k):
    """k: 0 self probabilities, 1 after self, 2 cross probabilities, 3 after cross, 4 FFN hidden, 5 after FFN."""
    return 64 + 6 * layer + k


def sites(d_ff, n_enc, n_dec, heads, T):
    """{site: shape of one series' mask}: a row site of width W is (T, W) (e = t * W + c), an attention site (H, T, T)
    (e = (h * T + i) * T + j)."""
    out = {ENC_EMB: (T, 64), ENC_POS: (T, 64), DEC_POS: (T, 64)}
    for i in range(n_enc):
        out.update({enc_site(i, 0): (heads, T, T), enc_site(i, 1): (T, 64), enc_site(i, 2): (T, d_ff), enc_site(i, 3): (T, 64)})
    for i in range(n_dec):
        out.update({dec_site(i, 0): (heads, T, T), dec_site(i, 1): (T, 64), dec_site(i, 2): (heads, T, T), dec_site(i, 3): (T, 64),
                    dec_site(i, 4): (T, d_ff), dec_site(i, 5): (T, 64)})
    return out


def keep_scale(p):
    """The fp32 1 / (1 - p) the kernels multiply kept values by, as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def build_masks(seed, p, B, d_ff, n_enc, n_dec, heads, T):
    """{site: bool (B, *shape)}: element e of series b at site s is kept iff device_uniform(seed, s, b)[e] >= fp32(p)."""
    out = {}
    for s, shape in sites(d_ff, n_enc, n_dec, heads, T).items():
        u = O.device_uniform(seed, s, 0, B, int(np.prod(shape)))
        out[s] = torch.from_numpy(u >= np.float32(p)).reshape((B,) + shape)
    return out


def ones_masks(B, d_ff, n_enc, n_dec, heads, T):
    return {s: torch.ones((B,) + shape, dtype=torch.bool) for s, shape in sites(d_ff, n_enc, n_dec, heads, T).items()}


# ---- the forward --------------------------------------------------------------------------------------------------------------
def _drop(x, masks, site, scale):
    return x * (masks[site].to(x.dtype) * scale)


def _attend(q, k, v, heads, causal, masks, site, scale):
    qh, kh, vh = (R._split_heads(t, heads) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    if causal:
        T = s.shape[-1]
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1), float("-inf"))
    prob = _drop(torch.softmax(s, dim=-1), masks, site, scale)          # nn.MultiheadAttention: no renormalisation
    return (prob @ vh).transpose(1, 2).reshape(q.shape)


_PRE = None             # min_preactivation()'s list, while it runs


def _ffn(h, sd, p, norm, masks, site_hidden, site_out, scale):
    pre = R._lin(R._ln(h, sd, p + norm), sd, p + "linear1")
    if _PRE is not None:
        _PRE.append(float(pre.detach().abs().min()))
    hid = _drop(torch.relu(pre), masks, site_hidden, scale)
    return h + _drop(R._lin(hid, sd, p + "linear2"), masks, site_out, scale)


def forward(sd, x, heads, masks, p, pe=None):
    """x (B,T,F) -> prediction (B,T,F) with the dropout the masks spell out (kept values times the fp32 1 / (1 - p))."""
    dt = sd["encoder.value_embedding.weight"].dtype
    x = x.to(dt)
    B, T, _ = x.shape
    scale = keep_scale(p)
    table = R._table(pe, T, dt)
    h = _drop(R._lin(x, sd, "encoder.value_embedding"), masks, ENC_EMB, scale)
    h = _drop(R._ln(h, sd, "encoder.embedding_ln") + table, masks, ENC_POS, scale)
    for i in range(R._n_layers(sd, "encoder.transformer_encoder.layers.")):
        q = f"encoder.transformer_encoder.layers.{i}."
        n = R._ln(h, sd, q + "norm1")
        a = _attend(R._qkv(n, sd, q + "self_attn", R.Q), R._qkv(n, sd, q + "self_attn", R.K), R._qkv(n, sd, q + "self_attn", R.V),
                    heads, False, masks, enc_site(i, 0), scale)
        h = h + _drop(R._lin(a, sd, q + "self_attn.out_proj"), masks, enc_site(i, 1), scale)
        h = _ffn(h, sd, q, "norm2", masks, enc_site(i, 2), enc_site(i, 3), scale)
    memory = h
    rows = torch.cat([torch.zeros(B, 1, 64, dtype=dt), R._lin(x, sd, "decoder.input_projection")[:, :-1]], dim=1)
    h = _drop(rows + table, masks, DEC_POS, scale)
    for i in range(R._dec_layers(sd)):
        q = f"decoder.transformer_decoder.layers.{i}."
        n = R._ln(h, sd, q + "norm1")
        a = _attend(R._qkv(n, sd, q + "self_attn", R.Q), R._qkv(n, sd, q + "self_attn", R.K), R._qkv(n, sd, q + "self_attn", R.V),
                    heads, True, masks, dec_site(i, 0), scale)
        h = h + _drop(R._lin(a, sd, q + "self_attn.out_proj"), masks, dec_site(i, 1), scale)
        n = R._ln(h, sd, q + "norm2")
        a = _attend(R._qkv(n, sd, q + "multihead_attn", R.Q), R._qkv(memory, sd, q + "multihead_attn", R.K),
                    R._qkv(memory, sd, q + "multihead_attn", R.V), heads, False, masks, dec_site(i, 2), scale)
        h = h + _drop(R._lin(a, sd, q + "multihead_attn.out_proj"), masks, dec_site(i, 3), scale)
        h = _ffn(h, sd, q, "norm3", masks, dec_site(i, 4), dec_site(i, 5), scale)
    return R._lin(h, sd, "decoder.output_projection")


def taking_part(sd):
    """The state-dict names the training step has a gradient for (98 at 3 + 3 layers): not the pe buffers, not condition_fusion.*"""
    return [k for k in sd if not k.endswith(".pe") and not k.startswith("condition_fusion.")]


def loss_and_grads(sd, x, heads, masks, p, pe=None):
    """(prediction, mse loss, {name: gradient}) of forward() in sd's dtype; sd is not modified."""
    leaves = {k: v.detach().clone().requires_grad_(k in set(taking_part(sd))) for k, v in sd.items()}
    pred = forward(leaves, x, heads, masks, p, pe)
    loss = torch.mean((pred - x.to(pred.dtype)) ** 2)
    names = taking_part(sd)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return pred.detach(), loss.detach(), dict(zip(names, grads))


# ---- the cases' weights and inputs --------------------------------------------------------------------------------------------
# A ReLU unit whose pre-activation is nearer to zero than an fp32 forward can resolve has no derivative to compare: fp32 and fp64
# then differentiate different functions (one flipped unit moved a linear1 gradient by 16 bars).  With ~3e5 hidden units of O(1)
# spread per case the nearest one sits around 4e-6; a case's seed is moved on until none is inside KINK_MARGIN, ten times the
# 1e-7 an O(1) pre-activation is off by in fp32.  F's first seed had one at 3.9e-8.
SEED_BUMP = {"F": 2000}


def case_seed(c):
    return 7000 + 13 * ord(c.name) + SEED_BUMP.get(c.name, 0)


def min_preactivation(c):
    """The smallest |FFN pre-activation| of the case's fp64 forward, over every layer, row and unit."""
    global _PRE
    _PRE = []
    try:
        forward(state_dict_as(c, torch.float64), series(c), c.heads, masks_of(c), c.p)
        return min(_PRE)
    finally:
        _PRE = None


@functools.lru_cache(maxsize=None)
def state_dict(c):
    """fp32 state dict of the case: the reference's initialisation scale, biases and LayerNorm parameters moved by 0.1 N(0,1) so
    that no gradient is trivially zero."""
    sd = synth.make_tsae_state_dict(case_seed(c), c.n_features, c.d_ff, c.n_enc, c.n_dec, c.heads)
    g = torch.Generator().manual_seed(case_seed(c) + 1)
    out = {}
    for k, v in sd.items():
        v = v.clone()
        if k in set(taking_part(sd)) and (k.endswith("bias") or ".norm" in k or "embedding_ln" in k):
            v += 0.1 * torch.randn(v.shape, generator=g)
        out[k] = v
    return out


def state_dict_as(c, dtype):
    return {k: v.to(dtype) for k, v in state_dict(c).items()}


def series(c):
    return synth.make_tsae_series(100 * c.T + 7 * c.B + case_seed(c), c.B, c.T, c.n_features)


def masks_of(c, seed=None):
    return build_masks(case_seed(c) if seed is None else seed, c.p, c.B, c.d_ff, c.n_enc, c.n_dec, c.heads, c.T)


_REFERENCE = {}


def reference(c, pe=None, key=None):
    """fp64 (prediction, loss, grads) of the case on its own masks, computed once per (case, key): `pe` a positional table to use
    (the library's own, on the GPU tests) instead of the one formed in tests/_tsae_ref.py, `key` what names it."""
    if (c, key) not in _REFERENCE:
        _REFERENCE[(c, key)] = loss_and_grads(state_dict_as(c, torch.float64), series(c), c.heads, masks_of(c), c.p, pe)
    return _REFERENCE[(c, key)]
