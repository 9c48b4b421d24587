"""Plain-torch restatement of the motion denoiser's forward (model/denoiser/mytransformer.py Transformer(dim).forward) at any
dtype: oracle.t2s_oracle.dit_forward with N_TOK, 15 and LAT_W replaced by 16 * W, W / 2 and W.  Everything else (time
embedding, blocks, attention, MLP) is the oracle's own code, which follows the dtype of its arguments.

tests/test_wide_train_host.py anchors it to the reference project's recorded outputs (tests/golden/wide_dit.npz); the
wide training tests differentiate it with torch autograd in fp64."""
import torch
import torch.nn.functional as F

from oracle import t2s_oracle as O

NOGRAD = ("pos_embed", "unpatch.")      # state-dict keys that receive no gradient


def time_embedding(t, dtype):
    """O.time_embedding with the frequency table in `dtype` (the oracle builds it in fp32)."""
    t = (t * 100.0).to(dtype).unsqueeze(-1)
    freqs = torch.pow(torch.tensor(10000.0, dtype=dtype), torch.linspace(0, 1, O.D_MODEL // 2, dtype=dtype)).to(t.device)
    arg = t[:, None] / freqs
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1).squeeze(1)


def forward(sd, inp, t, text, temb=None):
    """inp (B,64,W) -> (B,64,W).  `temb`: a ready (B,128) time embedding (the fp64 runs take the fp32 one, as the fixture's
    generator does, so that both precisions differentiate the same function of the same conditioning)."""
    B, _, W = inp.shape
    x = inp.permute(0, 2, 1).unsqueeze(1)
    x = F.conv2d(x, sd["conv.weight"], sd["conv.bias"], stride=2)
    x = x.permute(0, 2, 3, 1)
    x = x.reshape(B, 16 * W, x.size(3))
    x = F.linear(x, sd["patch_emb.weight"], sd["patch_emb.bias"]) + sd["pos_embed"]
    c = time_embedding(t, inp.dtype) if temb is None else temb
    if text is not None:
        c = c + text
    for i in range(O.N_BLOCKS):
        x = O.dit_block(sd, i, x, c)
    x = F.layer_norm(x, (O.D_MODEL,), sd["ln.weight"], sd["ln.bias"], eps=1e-5)
    x = F.linear(x, sd["linear_emb_to_patch.weight"], sd["linear_emb_to_patch.bias"])
    x = x.view(B, W // 2, 32, 1, 2, 2).permute(0, 3, 1, 2, 4, 5).permute(0, 1, 2, 4, 3, 5)
    x = x.reshape(B, 1, W, O.LAT_C).squeeze(1)
    return x.permute(0, 2, 1)


def grads(sd32, x, t, text, target, dtype, input_grad=False):
    """Autograd through the restatement in `dtype` on the fp32 values sd32 / x / text / target and the fp32 time
    embedding: (pred, loss, {key: grad}, dx or None), all as fp64 tensors."""
    temb = time_embedding(t, torch.float32).to(dtype)
    sd = {k: v.detach().to(dtype).requires_grad_(not k.startswith(NOGRAD)) for k, v in sd32.items()}
    xin = x.detach().to(dtype).requires_grad_(input_grad)
    pred = forward(sd, xin, t, None if text is None else text.to(dtype), temb=temb)
    loss = F.mse_loss(pred, target.to(dtype))
    loss.backward()
    g = {k: v.grad.double() for k, v in sd.items() if v.grad is not None}
    return pred.detach().double(), loss.detach().double(), g, (xin.grad.double() if input_grad else None)


# ------------------------------------------------------------------------------------------------ shared cases
WEIGHT_SEED = 2025
_CASES = {}


def state_dict(W, seed=WEIGHT_SEED):
    from t2ms_amd import synth
    return synth.make_dit_state_dict(seed, width=W)


def batch_inputs(W, B, with_text):
    """(x, t, text or None, target) of a whole-model case: functions of (W, B, with_text) alone."""
    from t2ms_amd import synth
    x = synth.make_wide_latents(7100 + W, B, W)
    t = torch.tensor([5, 50, 99, 0, 73][:B])
    text = synth.make_text_embeddings(71, B) if with_text else None
    return x, t, text, synth.make_wide_latents(7200 + W, B, W)


def batch_case(W, B, with_text, dtype=torch.float64, input_grad=False):
    """Inputs and autograd through the restatement in `dtype`, computed once per case and left unchanged."""
    key = (W, B, with_text, dtype, input_grad)
    if key not in _CASES:
        ins = batch_inputs(W, B, with_text)
        _CASES[key] = ins + grads(state_dict(W), *ins, dtype=dtype, input_grad=input_grad)
    return _CASES[key]
