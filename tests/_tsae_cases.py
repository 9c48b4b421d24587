"""The TSae kernels' own branch points as a case table, shared by tests/test_tsae_host.py (the gates on the inputs) and
tests/test_tsae_fp64.py (the kernels against the fp64 restatement of tests/_tsae_ref.py).  Plain data and seeded builders only:
nothing here is recorded, everything is computed at test time.

A case is (n_features, d_ff, n_enc, n_dec, heads, B, T, gain, seed).  Weights: synth.make_tsae_state_dict(seed, ...) with the
q and k rows ([:128]) of every *.in_proj_weight multiplied by `gain`; inputs: synth.make_tsae_series.  At gain 1 the softmax is
nearly uniform (logit spread ~1); at gain 4 it is peaked (spread ~17, the running maximum moves between key chunks), and the
fp32 restatement still sits within a few hundredths of the bar of the fp64 one.  Gain 8 is out: generation turns chaotic."""
import collections
import functools
import math

import torch

import _tsae_ref as R
from t2ms_amd import synth

Case = collections.namedtuple("Case", "n_features d_ff n_enc n_dec heads B T gain seed")

BAR = 1e-5                        # the project's bar: BAR * max(1, max|fp64 output|)
MIN_SPREAD, MIN_RISING = 8.0, 0.25   # the stress gate of a gain-4 case (see stress())

BP_GAIN1 = Case(10, 128, 3, 3, 8, 2, 144, 1.0, 3101)      # the recorded `bp` weights as they are: fails the stress gate
TABLE = (
    BP_GAIN1,
    Case(10, 128, 3, 3, 8, 2, 144, 4.0, 3101),            # ... and peaked, side by side
    # d_ff: the 64-column tail chunk of tsae_ffn_kernel (64 alone, 128 + 64, 2 x 128 + 64), four chunks (512)
    Case(10, 64, 1, 1, 8, 1, 33, 4.0, 4101),
    Case(7, 192, 2, 1, 8, 3, 129, 4.0, 4102),             # also the bitwise-properties configuration
    Case(10, 320, 1, 2, 8, 1, 31, 4.0, 4103),
    Case(10, 512, 1, 1, 4, 1, 63, 4.0, 4104),
    # layers: six a side (LinBatch with six z-slices, the cache stride at l = 5), at the limits of d_ff and F; unequal sides;
    # four heads with more than one layer; B = 5 with the generate branch of the workspace size (n_dec >= 3)
    Case(16, 512, 6, 6, 8, 1, 257, 4.0, 4305),
    Case(10, 64, 6, 6, 4, 1, 32, 4.0, 4106),
    Case(10, 128, 3, 3, 4, 5, 37, 4.0, 4107),
    Case(3, 256, 2, 2, 4, 1, 128, 4.0, 4308),
    # features: gen_matvec at K = F = 1 and F = 5 (empty k quarters), ldy = F narrower than the 32-column tile
    Case(1, 64, 1, 1, 8, 3, 32, 4.0, 4109),
    Case(5, 128, 1, 3, 4, 3, 127, 4.0, 4110),
    # T: the last query block and key chunk of tsae_attn_kernel, the zero rows of load_tile
    Case(10, 128, 1, 1, 8, 3, 64, 4.0, 4111),
    Case(10, 192, 1, 1, 8, 3, 257, 4.0, 4112),
    Case(12, 448, 2, 2, 8, 3, 63, 4.0, 4113),
    Case(10, 128, 2, 2, 8, 1, 129, 4.0, 4414),
    Case(7, 128, 1, 1, 4, 3, 33, 4.0, 4115),
    Case(10, 128, 1, 1, 4, 1, 127, 4.0, 4416),
    Case(16, 256, 1, 1, 8, 3, 128, 4.0, 4117),
    Case(10, 128, 1, 1, 8, 3, 31, 4.0, 4118),
    # long: every key chunk up to the table's last row, and 600 rows with eight heads
    Case(10, 192, 2, 1, 4, 1, 2000, 4.0, 4119),
    Case(7, 128, 1, 2, 8, 1, 600, 4.0, 4120),
)
# The mirror's case (model/pretrained/TSae.py on the HIP route).  Not in TABLE: at T = 65 the second key chunk holds ONE key, so
# the share of rows whose running maximum rises there cannot reach MIN_RISING; it passes the conditioning and the spread gate.
MIRROR = Case(16, 512, 6, 6, 8, 2, 65, 4.0, 4121)


def case_id(c):
    return f"F{c.n_features}_ff{c.d_ff}_L{c.n_enc}x{c.n_dec}_h{c.heads}_B{c.B}_T{c.T}_g{c.gain:g}"


IDS = [case_id(c) for c in TABLE]


@functools.lru_cache(maxsize=None)
def state_dict(c):
    """fp32 state dict of the case (no `pe` scaling: only the q and k rows of the in-projections take the gain)."""
    sd = synth.make_tsae_state_dict(c.seed, c.n_features, c.d_ff, c.n_enc, c.n_dec, c.heads)
    out = {}
    for k, v in sd.items():
        v = v.clone()
        if k.endswith(".in_proj_weight"):
            v[:128] *= c.gain
        out[k] = v
    return out


def state_dict_as(c, dtype):
    return {k: v.to(dtype) for k, v in state_dict(c).items()}


def series(c):
    return synth.make_tsae_series(100 * c.T + 7 * c.B + c.seed, c.B, c.T, c.n_features)


def bar(ref):
    return BAR * max(1.0, float(ref.abs().max()))


def stress(c):
    """(median over query rows of max - min logit, share of rows whose running maximum over 64-key chunks rises by more than 1
    in some chunk after the first) of encoder layer 0's attention, from the fp64 restatement's own pieces."""
    sd = state_dict_as(c, torch.float64)
    x = series(c).double()
    h = R._ln(R._lin(x, sd, "encoder.value_embedding"), sd, "encoder.embedding_ln") + R.sinusoid_table(c.T, 64, torch.float64)
    p = "encoder.transformer_encoder.layers.0."
    n = R._ln(h, sd, p + "norm1")
    q, k = (R._split_heads(R._qkv(n, sd, p + "self_attn", rows), c.heads) for rows in (R.Q, R.K))
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])                         # (B,H,T,T)
    spread = float((s.max(-1).values - s.min(-1).values).median())
    chunk_max = torch.stack([s[..., j:j + 64].max(-1).values for j in range(0, c.T, 64)], dim=-1)
    running = torch.cummax(chunk_max, dim=-1).values
    rising = float(((running[..., 1:] - running[..., :-1]).max(-1).values > 1.0).double().mean()) if c.T > 64 else 0.0
    return spread, rising
