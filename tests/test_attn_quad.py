"""attn_fwd_persistent_quad_kernel (heads walked in fours, csrc/t2s_attn.hip) against attn_fwd_persistent_kernel, bit for bit.

The quad walk moves query tiles between waves and passes; every tile must still see key blocks 0..14 in order with the
sticky-reference decisions of the head-by-head walk, INCLUDING the coupling of the tiles (2i, 2i+1): the wave that holds
both re-references both when either is stale.  No tolerance can tell a wrong block order or a missed coupling from rounding,
so the check is bitwise equality of the same call under T2S_ATTN_QUAD=0 and =1.  The switches are read once per process:
each arm runs in a short child process with a timeout, and a child that fails ends the test there.

Shapes (T2S_ATTN_PERSIST_MIN=1, T2S_ATTN_GRID=4: four workgroups, head bh goes to workgroup bh % 4):
  n_seq 4 -> 16 heads, exactly one quad per workgroup;  9 -> 36 heads, two quads + one plain pass (ring and Q continuity
  across a quad boundary and into plain passes);  7 -> 28 heads, one quad + three plain passes;  3 -> 12 heads, three per
  workgroup: no quad, the launcher keeps the head-by-head kernel.
Spikes (in every head, so in heads A-D of every quad alike): the rows of test_attention_packed_kernel_vs_oracle (tiles 0, 3,
6, 14; the stale-reference branch fires in tile 0 at block 14 and tile 6 at block 12) and four more that fire it in
  tile 12 (wave 7's coupled pair of head D in pass 2; tile 13 must follow),  tile 14 (the uncoupled slots of wave 7),
  tile 8 (pass 4: its partner, tile 9, sits in another wave and follows through the exchanged flag),  tile 10 (the same
  between waves 6 and 7)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_INPUTS = r"""
import numpy as np, torch
def make_inputs(n_seq):
    rs = np.random.RandomState(2100 + n_seq)
    BH = n_seq * 4
    q, k, v = (torch.from_numpy(rs.randn(BH, 480, 32).astype(np.float32)) for _ in range(3))
    k[:, 333] = q[:, 100] * 5.0
    k[:, 5] = q[:, 479] * 4.0
    k[:, 479] = q[:, 0] * 4.0
    k[:, 410] = q[:, 200] * 12.0
    k[:, 0:32] = -q[:, 7:8] * 3.0 + 0.01 * k[:, 0:32]
    k[:, 448] = q[:, 7] * 10.0
    k[:, 440] = q[:, 390] * 12.0      # tile 12, block 13
    k[:, 400] = q[:, 470] * 12.0      # tile 14, block 12
    k[:, 425] = q[:, 270] * 12.0      # tile 8, block 13
    k[:, 300] = q[:, 345] * 12.0      # tile 10, block 9
    return q, k, v
"""

_KERNEL_CHILD = _INPUTS + r"""
import sys
sys.path.insert(0, {repo!r})
from t2ms_amd import _lib as L
n_seq = int(sys.argv[1])
dev = torch.device("cuda", 0)
q, k, v = make_inputs(n_seq)
BH = n_seq * 4
qd = q.reshape(BH, 15, 32, 4, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous().to(dev)
kd = k.reshape(BH, 15, 32, 4, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous().to(dev)
vd = v.reshape(BH, 15, 4, 2, 4, 32).permute(0, 1, 2, 3, 5, 4).contiguous().to(dev)
od = torch.full((n_seq * 480 * 128,), float("nan"), device=dev)
L.check(L.lib().t2s_attn_fwd_packed(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), n_seq, L.stream_ptr(dev)))
torch.cuda.synchronize()
np.save(sys.argv[2], od.cpu().numpy())
"""

_SAMPLER_CHILD = r"""
import sys, types
import numpy as np, torch
sys.path.insert(0, {repo!r})
from t2ms_amd import synth
from t2ms_amd.sampler import Sampler
from model.denoiser.transformer import Transformer
from model.pretrained.vqvae import vqvae
dev = torch.device("cuda", 0)
B, steps = 8, 10
m = Transformer(); m.load_state_dict(synth.make_dit_state_dict(31337, gain=0.7), strict=True); m = m.to(dev).eval()
v = vqvae(types.SimpleNamespace(block_hidden_size=128, num_residual_layers=2, res_hidden_size=256, embedding_dim=64))
v.load_state_dict(synth.make_vae_state_dict(2025), strict=True); v = v.to(dev).eval()
noises = torch.from_numpy(np.random.RandomState(2).randn(steps, B, 64, 30).astype(np.float32))
s = Sampler(m, v.decoder, "ddpm", steps, 7.0, B, 96, dev, use_graph=True, math="f32", lanes=2)
lat, series, _ = s.run(synth.make_text_embeddings(1, B), x_T=synth.make_latents(1, B), noise=noises)
torch.cuda.synchronize()
np.savez(sys.argv[1], lat=lat.cpu().numpy(), series=series.cpu().numpy())
"""


def _run_child(tmp_path, name, text, args, env):
    script = tmp_path / name
    script.write_text(text.format(repo=REPO))
    full = dict(os.environ, T2S_ATTN_PERSIST_MIN="1", **env)
    subprocess.run([sys.executable, str(script)] + [str(a) for a in args], check=True, env=full, cwd=REPO, timeout=120)


def _unpack(o, n_seq):
    # o: [tile = seq*15 + t][G = head*4 + g][h][i][e] = O[seq][head][32 t + i][8g + 4h + e]
    return torch.from_numpy(o).reshape(n_seq, 15, 4, 4, 2, 32, 4).permute(0, 2, 1, 5, 3, 4, 6).reshape(n_seq * 4, 480, 32)


@pytest.mark.parametrize("n_seq", [4, 9, 7, 3])
def test_quad_walk_is_the_head_walk_bit_for_bit(tmp_path, n_seq):
    outs = []
    for quad in ("0", "1"):
        dst = tmp_path / f"o_{quad}.npy"
        _run_child(tmp_path, "attn_child.py", _KERNEL_CHILD, [n_seq, dst], {"T2S_ATTN_GRID": "4", "T2S_ATTN_QUAD": quad})
        outs.append(np.load(dst))
    assert np.isfinite(outs[1]).all(), "the NaN pre-fill shows through: a tile was not written"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), \
        f"max |diff| {np.abs(outs[0] - outs[1]).max():.3e}"
    scope = {}
    exec(_INPUTS, scope)
    q, k, v = scope["make_inputs"](n_seq)
    ref = (torch.softmax((q.double() * 32 ** -0.5) @ k.double().transpose(-1, -2), dim=-1) @ v.double()).float()
    diff = float((_unpack(outs[1], n_seq).double() - ref.double()).abs().max())
    print(f"n_seq {n_seq}: max |quad - fp64 softmax| = {diff:.3e}")
    assert diff < 3e-5


def test_sampler_bits_do_not_depend_on_the_quad_walk(tmp_path):
    """10-step CFG DDPM at B = 8 on two lanes, persistent attention on a grid of 8 (every workgroup gets whole quads)."""
    outs = []
    for quad in ("0", "1"):
        dst = tmp_path / f"s_{quad}.npz"
        _run_child(tmp_path, "sampler_child.py", _SAMPLER_CHILD, [dst], {"T2S_ATTN_GRID": "8", "T2S_ATTN_QUAD": quad})
        outs.append(np.load(dst))
    for key in ("lat", "series"):
        assert np.isfinite(outs[1][key]).all()
        assert np.array_equal(outs[0][key].view(np.uint32), outs[1][key].view(np.uint32)), key
