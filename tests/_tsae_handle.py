"""A TSae library handle through the C ABI, shared by tests/test_tsae.py and tests/test_tsae_fp64.py (GPU tests only)."""
import ctypes as C

import torch

from t2ms_amd import _lib as L

DEV = "cuda:0"


class Handle:
    """A two-sided (or one-sided) library handle on a state dict, with the entries as methods.  `k`: n_features, d_ff, heads,
    n_enc, n_dec (d_model 64 unless given) of the state dict `sd`; `override` replaces fields of what create is TOLD, the layers
    filled in stay those of `k`."""

    def __init__(self, k, sd, enc=True, dec=True, **override):
        layers = k
        k = dict(k, **override)
        sd = {n: t.to(DEV).contiguous() for n, t in sd.items()}
        self.keep, self.F = sd, k["n_features"]
        w = L.TsaeWeights()
        w.n_features, w.d_model, w.d_ff, w.heads = k["n_features"], k.get("d_model", 64), k["d_ff"], k["heads"]
        w.n_enc, w.n_dec = (k["n_enc"] if enc else 0), (k["n_dec"] if dec else 0)

        def p(name):
            return sd[name].data_ptr()

        def attn(dst, prefix):
            dst.in_proj_w, dst.in_proj_b = p(prefix + ".in_proj_weight"), p(prefix + ".in_proj_bias")
            dst.out_proj_w, dst.out_proj_b = p(prefix + ".out_proj.weight"), p(prefix + ".out_proj.bias")

        def layer(dst, prefix, norms):
            for n in ("linear1", "linear2") + norms:
                setattr(dst, n + "_w", p(f"{prefix}.{n}.weight"))
                setattr(dst, n + "_b", p(f"{prefix}.{n}.bias"))

        w.value_embedding_w, w.value_embedding_b = p("encoder.value_embedding.weight"), p("encoder.value_embedding.bias")
        w.embedding_ln_w, w.embedding_ln_b = p("encoder.embedding_ln.weight"), p("encoder.embedding_ln.bias")
        w.input_projection_w, w.input_projection_b = p("decoder.input_projection.weight"), p("decoder.input_projection.bias")
        w.output_projection_w, w.output_projection_b = p("decoder.output_projection.weight"), p("decoder.output_projection.bias")
        for i in range(layers["n_enc"]):
            attn(w.enc[i].self_attn, f"encoder.transformer_encoder.layers.{i}.self_attn")
            layer(w.enc[i], f"encoder.transformer_encoder.layers.{i}", ("norm1", "norm2"))
        for i in range(layers["n_dec"]):
            attn(w.dec[i].self_attn, f"decoder.transformer_decoder.layers.{i}.self_attn")
            attn(w.dec[i].multihead_attn, f"decoder.transformer_decoder.layers.{i}.multihead_attn")
            layer(w.dec[i], f"decoder.transformer_decoder.layers.{i}", ("norm1", "norm2", "norm3"))
        self.w, self.ptr = w, C.c_void_p()
        torch.cuda.synchronize()
        self.rc = L.lib().t2s_tsae_create(C.byref(w), C.byref(self.ptr))

    def close(self):
        if self.ptr:
            torch.cuda.synchronize()
            L.lib().t2s_tsae_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def ws(self, B, T):
        n = int(L.lib().t2s_tsae_workspace_bytes(self.ptr, B, T))
        assert n > 0
        return torch.empty(n, dtype=torch.uint8, device=DEV)

    def call(self, name, tensors, B, T, ws=None, ws_bytes=None, ptr=None):
        """rc of an entry; `tensors`: device tensors or None (NULL) in the entry's order."""
        ws = self.ws(max(B, 1), min(max(T, 1), L.TSAE_MAX_T)) if ws is None else ws
        args = [t.data_ptr() if t is not None else None for t in tensors]
        return getattr(L.lib(), name)(self.ptr if ptr is None else ptr, *args, B, T, ws.data_ptr() if ws is not False else None,
                                      ws.numel() if ws_bytes is None else ws_bytes, L.stream_ptr(DEV))

    def encode(self, x):
        B, T, _ = x.shape
        out = torch.empty(B, T, 64, device=DEV)
        L.check(self.call("t2s_tsae_encode", [x, out], B, T), "t2s_tsae_encode")
        return out

    def decode(self, memory, target):
        B, T, _ = target.shape
        out = torch.empty(B, T, self.F, device=DEV)
        L.check(self.call("t2s_tsae_decode", [memory, target, out], B, T), "t2s_tsae_decode")
        return out

    def generate(self, memory):
        B, S, _ = memory.shape
        out = torch.empty(B, S, self.F, device=DEV)
        L.check(self.call("t2s_tsae_generate", [memory, out], B, S), "t2s_tsae_generate")
        return out

    def positional(self, count=L.TSAE_MAX_T):
        """Rows 0 .. count-1 of the library's own positional table, on the CPU."""
        pe = torch.empty(count, 64, device=DEV)
        L.check(L.lib().t2s_tsae_positional(self.ptr, pe.data_ptr(), 0, count, L.stream_ptr(DEV)), "t2s_tsae_positional")
        return pe.cpu()
