"""TS2Vec for the C-FID metric (reference evaluate/ts2vec.py; evaluation.py:238-243): evaluation.py TRAINS this encoder on
the original series at evaluation time (`initialize_ts2vec`: 200 contrastive iterations from a random initialisation)
and then encodes original and generated series with it.

Split of labour here (the lowest-ranked remainder of the scope table):
  * `TS2Vec.encode(..., encoding_window='full_series')` -- what C-FID consumes -- runs the HIP encoder kernel
    (`t2s_ts2vec_encode`, csrc/t2s_eval.hip) on the averaged weights;
  * `TS2Vec.fit` trains a 0.6 M-parameter dilated-convolution stack for 200 steps of batch 8 on one of two engines.
    "torch" (the default): forward / backward are torch autograd ops, about 1,250 launches and one host sync per
    iteration.  "hip" (`engine="hip"`, or T2S_TS2VEC_FIT=hip): every draw of the fit is taken up front (`draw_plan`: none
    depends on a computed value), uploaded once, and each iteration is six launches on the parameter tensors in place --
    `t2s_ts2vec_train_step` (forward of both views, hierarchical contrastive loss, backward; csrc/t2s_ts2vec_train.hip),
    `t2s_adamw_step_multi`, `t2s_swa_update_multi` -- with the losses read once at the end.

The random draws follow the reference's ORDER and SOURCES so that a run is reproducible against it under the same seeds:
module initialisation and the loader shuffle from torch's CPU generator, crops and binomial masks from numpy's global
generator (ts2vec.py:120-126, 349-350), and the dropout masks of the two forward passes from torch's CPU generator with
the shape `nn.Dropout` sees on a CPU run (B, C_out, T) -- on the GPU they are applied as a multiplication.
tests/golden/ts2vec_fit.npz holds the reference's loss curve and representations for the fixture.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L


# ---------------------------------------------------------------------------- the encoder as a parameter container
class _SamePad(nn.Module):
    """ts2vec.py:401-418: Conv1d with 'same' length for any dilation (an even receptive field drops the last step)."""

    def __init__(self, cin, cout, k, dilation):
        super().__init__()
        rf = (k - 1) * dilation + 1
        self.conv = nn.Conv1d(cin, cout, k, padding=rf // 2, dilation=dilation)
        self.trim = 1 if rf % 2 == 0 else 0

    def forward(self, x):
        y = self.conv(x)
        return y[:, :, :-self.trim] if self.trim else y


class _Block(nn.Module):
    """ts2vec.py:420-433: GELU -> conv -> GELU -> conv, plus the (projected) input."""

    def __init__(self, cin, cout, k, dilation, final):
        super().__init__()
        self.conv1 = _SamePad(cin, cout, k, dilation)
        self.conv2 = _SamePad(cout, cout, k, dilation)
        self.projector = nn.Conv1d(cin, cout, 1) if (cin != cout or final) else None

    def forward(self, x):
        skip = x if self.projector is None else self.projector(x)
        return self.conv2(F.gelu(self.conv1(F.gelu(x)))) + skip


class _Dilated(nn.Module):
    def __init__(self, cin, channels, k):
        super().__init__()
        self.net = nn.Sequential(*[_Block(channels[i - 1] if i else cin, channels[i], k, 2 ** i, i == len(channels) - 1)
                                   for i in range(len(channels))])

    def forward(self, x):
        return self.net(x)


class TSEncoder(nn.Module):
    """ts2vec.py:352-399.  Same sub-module names (state-dict keys) and construction order (seeded initialisation) as the
    reference; `forward` is the TRAINING forward used by TS2Vec.fit (binomial mask, dropout mask handed in)."""

    def __init__(self, input_dims, output_dims, hidden_dims=64, depth=10):
        super().__init__()
        self.input_dims, self.output_dims, self.hidden_dims = input_dims, output_dims, hidden_dims
        self.input_fc = nn.Linear(input_dims, hidden_dims)
        self.feature_extractor = _Dilated(hidden_dims, [hidden_dims] * depth + [output_dims], 3)
        self.repr_dropout = nn.Dropout(p=0.1)

    def forward(self, x, mask, drop):
        """x (B,T,C_in) on the module's device, mask (B,T) bool (False = hidden time step), drop (B,C_out,T) the dropout
        multiplier (0 or 1/(1-p))."""
        valid = ~x.isnan().any(dim=-1)
        x = torch.where(valid.unsqueeze(-1), x, torch.zeros_like(x))
        h = self.input_fc(x)
        h = torch.where((mask & valid).unsqueeze(-1), h, torch.zeros_like(h))
        return (self.feature_extractor(h.transpose(1, 2)) * drop).transpose(1, 2)


# ---------------------------------------------------------------------------- loss (ts2vec.py:451-497)
def _pair_loss(sim, n):
    """-log-softmax of every row over all OTHER entries; mean over the positives (i, n + i) and (n + i, i)."""
    logits = torch.tril(sim, diagonal=-1)[..., :-1] + torch.triu(sim, diagonal=1)[..., 1:]
    logits = -F.log_softmax(logits, dim=-1)
    i = torch.arange(n, device=sim.device)
    return (logits[:, i, n + i - 1].mean() + logits[:, n + i, i].mean()) / 2


def instance_contrastive_loss(z1, z2):
    if z1.size(0) == 1:
        return z1.new_tensor(0.)
    z = torch.cat([z1, z2], dim=0).transpose(0, 1)                 # T x 2B x C
    return _pair_loss(torch.matmul(z, z.transpose(1, 2)), z1.size(0))


def temporal_contrastive_loss(z1, z2):
    if z1.size(1) == 1:
        return z1.new_tensor(0.)
    z = torch.cat([z1, z2], dim=1)                                  # B x 2T x C
    return _pair_loss(torch.matmul(z, z.transpose(1, 2)), z1.size(1))


def hierarchical_contrastive_loss(z1, z2, alpha=0.5, temporal_unit=0):
    loss, d = torch.zeros((), device=z1.device), 0
    while z1.size(1) > 1:
        if alpha != 0:
            loss = loss + alpha * instance_contrastive_loss(z1, z2)
        if d >= temporal_unit and 1 - alpha != 0:
            loss = loss + (1 - alpha) * temporal_contrastive_loss(z1, z2)
        d += 1
        z1 = F.max_pool1d(z1.transpose(1, 2), kernel_size=2).transpose(1, 2)
        z2 = F.max_pool1d(z2.transpose(1, 2), kernel_size=2).transpose(1, 2)
    if z1.size(1) == 1:
        if alpha != 0:
            loss = loss + alpha * instance_contrastive_loss(z1, z2)
        d += 1
    return loss / d


def _take_rows(x, starts, length):
    idx = torch.as_tensor(starts, device=x.device)[:, None] + torch.arange(length, device=x.device)[None, :]
    return x[torch.arange(x.size(0), device=x.device)[:, None], idx]


# ---------------------------------------------------------------------------- the model
ENGINES = ("torch", "hip")


def resolve_engine(engine):
    """None reads T2S_TS2VEC_FIT (default "torch"); there is never a silent switch between the two."""
    import os
    engine = os.environ.get("T2S_TS2VEC_FIT", "torch") if engine is None else engine
    if engine not in ENGINES:
        raise L.T2SError(f"TS2Vec: engine must be one of {ENGINES} (got {engine!r})")
    return engine


class FitDraw:
    """One iteration's draws: x (B, T, C_in) fp32 on the CPU (after the max_train_length window), crop_l, and per view
    (start (B) int, length, mask (B, length) bool, keep (B, C_out, length) fp32 dropout multiplier)."""
    __slots__ = ("x", "crop_l", "views")

    def __init__(self, x, crop_l, views):
        self.x, self.crop_l, self.views = x, crop_l, views


class TS2Vec:
    """ts2vec.py:23-330 as far as evaluation.py uses it: constructor arguments, fit, encode('full_series'), save / load."""

    def __init__(self, input_dims, output_dims=320, hidden_dims=64, depth=10, device="cuda", lr=0.001, batch_size=16,
                 max_train_length=None, temporal_unit=0, after_iter_callback=None, after_epoch_callback=None, engine=None):
        # fit() runs on one of two engines.  "torch" (the default): torch autograd, wherever the module lives (a CPU run
        # reproduces the reference's loss curve bit for bit: tests/test_ts2vec_fit.py).  "hip": the fused training step of
        # csrc/t2s_ts2vec_train.hip, GPU only.  engine=None reads T2S_TS2VEC_FIT.  encode() is the HIP kernel and needs a
        # GPU (no CPU fallback)
        self.device = torch.device(device)
        self.engine = resolve_engine(engine)
        if self.engine == "hip" and self.device.type != "cuda":
            raise L.T2SError(f"TS2Vec(engine='hip') needs a GPU (got device {self.device}); the HIP training step has no CPU fallback")
        self.lr, self.batch_size = lr, batch_size
        self.max_train_length, self.temporal_unit = max_train_length, temporal_unit
        self._net = TSEncoder(input_dims, output_dims, hidden_dims, depth).to(self.device)   # initialised on the CPU generator
        self.net = torch.optim.swa_utils.AveragedModel(self._net)
        self.net.update_parameters(self._net)
        self.after_iter_callback, self.after_epoch_callback = after_iter_callback, after_epoch_callback
        self.n_epochs = self.n_iters = 0
        self._hip = None

    # -- training (ts2vec.py:73-160)
    def _check_train_data(self, train_data, n_epochs, n_iters):
        train_data = np.asarray(train_data)
        assert train_data.ndim == 3
        if n_iters is None and n_epochs is None:
            n_iters = 200 if train_data.size <= 100000 else 600
        if self.max_train_length is not None and train_data.shape[1] // self.max_train_length >= 2:
            raise L.T2SError("TS2Vec.fit: series longer than 2 x max_train_length (the reference's NaN-padded sectioning) "
                             "are outside what evaluation.py feeds it")
        if np.isnan(train_data).any():
            raise L.T2SError("TS2Vec.fit: missing values (NaN) are outside what evaluation.py feeds it")
        return train_data, n_epochs, n_iters

    def _draw(self, train_data, n_epochs, n_iters):
        """Every random draw of fit, in the reference's loop order and from its sources, without touching the model: none
        of them depends on a computed value.  Yields ("iter", FitDraw) per iteration and ("epoch",) at the end of every
        completed epoch.  Lazy: the torch engine computes between two draws exactly where it always did."""
        from torch.utils.data import DataLoader, TensorDataset
        loader = DataLoader(TensorDataset(torch.from_numpy(train_data).to(torch.float)),
                            batch_size=min(self.batch_size, len(train_data)), shuffle=True, drop_last=True)
        p_drop = self._net.repr_dropout.p
        epochs, iters = self.n_epochs, self.n_iters
        while n_epochs is None or epochs < n_epochs:
            stopped = False
            for (x,) in loader:
                if n_iters is not None and iters >= n_iters:
                    stopped = True
                    break
                if self.max_train_length is not None and x.size(1) > self.max_train_length:
                    off = np.random.randint(x.size(1) - self.max_train_length + 1)
                    x = x[:, off: off + self.max_train_length]
                T = x.size(1)
                crop_l = np.random.randint(low=2 ** (self.temporal_unit + 1), high=T + 1)
                left = np.random.randint(T - crop_l + 1)
                right = left + crop_l
                eleft = np.random.randint(left + 1)
                eright = np.random.randint(low=right, high=T + 1)
                offs = np.random.randint(low=-eleft, high=T - eright + 1, size=x.size(0))
                views = []
                for start, length in ((offs + eleft, right - eleft), (offs + left, eright - left)):
                    mask = torch.from_numpy(np.random.binomial(1, 0.5, size=(x.size(0), length))).to(torch.bool)
                    keep = torch.empty(x.size(0), self._net.output_dims, length).bernoulli_(1 - p_drop).div_(1 - p_drop)
                    views.append((start, int(length), mask, keep))
                iters += 1
                yield "iter", FitDraw(x, int(crop_l), views)
            if stopped:
                break
            epochs += 1
            yield ("epoch",)

    def draw_plan(self, train_data, n_epochs=None, n_iters=None):
        """The whole fit's draws up front (a list of the events of `_draw`).  Leaves torch's CPU generator and numpy's
        global generator exactly where fit() on the torch engine leaves them."""
        train_data, n_epochs, n_iters = self._check_train_data(train_data, n_epochs, n_iters)
        return list(self._draw(train_data, n_epochs, n_iters))

    def fit(self, train_data, n_epochs=None, n_iters=None, verbose=False):
        train_data, n_epochs, n_iters = self._check_train_data(train_data, n_epochs, n_iters)
        self._hip = None
        if self.engine == "hip":
            return self._fit_hip(list(self._draw(train_data, n_epochs, n_iters)), verbose)
        opt = torch.optim.AdamW(self._net.parameters(), lr=self.lr)
        loss_log = []
        cum, n_in_epoch = 0.0, 0
        self.losses_ = []                       # the per-iteration losses of the last fit (either engine)
        for ev in self._draw(train_data, n_epochs, n_iters):
            if ev[0] == "iter":
                dr = ev[1]
                x = dr.x.to(self.device)
                opt.zero_grad()
                outs = []
                for start, length, mask, keep in dr.views:
                    outs.append(self._net(_take_rows(x, start, length), mask.to(self.device), keep.to(self.device)))
                loss = hierarchical_contrastive_loss(outs[0][:, -dr.crop_l:], outs[1][:, :dr.crop_l], temporal_unit=self.temporal_unit)
                loss.backward()
                opt.step()
                self.net.update_parameters(self._net)
                val = loss.item()
                self.losses_.append(val)
                cum += val
                n_in_epoch += 1
                self.n_iters += 1
                if self.after_iter_callback is not None:
                    self.after_iter_callback(self, val)
            else:
                loss_log.append(cum / n_in_epoch)
                cum, n_in_epoch = 0.0, 0
                if verbose:
                    print(f"Epoch #{self.n_epochs}: loss={loss_log[-1]}")
                self.n_epochs += 1
                if self.after_epoch_callback is not None:
                    self.after_epoch_callback(self, loss_log[-1])
        return loss_log

    # -- the same training on the fused HIP step (csrc/t2s_ts2vec_train.hip)
    def _hip_tables(self):
        """Pointer structs and device tables over the torch parameter tensors the step updates in place."""
        import ctypes as C
        net, avg = self._net, self.net.module
        blocks = list(net.feature_extractor.net)
        depth = len(blocks) - 1
        if depth >= L.TS2VEC_MAX_BLOCKS:
            raise L.T2SError(f"TS2Vec.fit(engine='hip'): depth {depth} exceeds {L.TS2VEC_MAX_BLOCKS - 1}")
        params = list(net.parameters())
        for p in params:
            L.dev_ptr(p.data, "TS2Vec parameter")
        grads = {id(p): torch.zeros_like(p.data) for p in params}
        w, g = L.Ts2vecWeights(), L.Ts2vecGrads()
        w.input_dims, w.hidden, w.output_dims, w.depth = net.input_dims, net.hidden_dims, net.output_dims, depth

        def put(field, p, i=None):
            for st, ptr in ((w, p.data.data_ptr()), (g, grads[id(p)].data_ptr())):
                if i is None:
                    setattr(st, field, ptr)
                else:
                    getattr(st, field)[i] = ptr
        put("fc_w", net.input_fc.weight), put("fc_b", net.input_fc.bias)
        for i, blk in enumerate(blocks):
            if (blk.projector is not None) != (i == depth):
                raise L.T2SError("TS2Vec.fit(engine='hip'): a projector inside the stack (unequal hidden widths) is not supported")
            put("conv1_w", blk.conv1.conv.weight, i), put("conv1_b", blk.conv1.conv.bias, i)
            put("conv2_w", blk.conv2.conv.weight, i), put("conv2_b", blk.conv2.conv.bias, i)
        put("proj_w", blocks[depth].projector.weight), put("proj_b", blocks[depth].projector.bias)
        moments = [(torch.zeros_like(p.data), torch.zeros_like(p.data)) for p in params]
        adam = [(p.data.data_ptr(), grads[id(p)].data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, (m, v) in zip(params, moments)]
        swa = [(a.data.data_ptr(), p.data.data_ptr(), 0, 0, p.numel()) for a, p in zip(avg.parameters(), params)]
        chunks = sum((r[4] + 1023) // 1024 for r in adam)
        tables = torch.tensor(adam + swa, dtype=torch.int64).to(self.device)          # 5 x 8 bytes = t2s_adamw_tensor
        return w, g, tables, len(params), chunks, (grads, moments)

    def _hip_plan(self, draws):
        """The draws of all iterations in three device arrays, uploaded once -- x, the view starts, and the masks / dropout
        draws as bytes -- and one t2s_ts2vec_step per iteration pointing into them."""
        dev = self.device
        B, T, cin = draws[0].x.shape
        keep_scale = float(torch.ones(()).div_(1 - self._net.repr_dropout.p))
        xs = torch.stack([d.x for d in draws]).contiguous().float()
        starts = torch.from_numpy(np.stack([np.stack([v[0] for v in d.views]) for d in draws]).astype(np.int32))
        parts, offs, pos = [], [], 0
        for d in draws:
            if tuple(d.x.shape) != (B, T, cin):
                raise L.T2SError("TS2Vec.fit(engine='hip'): every batch of a fit must have one shape")
            row = []
            for _, _, mask, keep in d.views:
                for t in (mask.to(torch.uint8), keep.ne(0).to(torch.uint8)):
                    row.append(pos)
                    parts.append(t.reshape(-1))
                    pos += t.numel()
            offs.append(row)
        xs, starts, blob = xs.to(dev), starts.to(dev), torch.cat(parts).to(dev)
        steps = []
        for i, d in enumerate(draws):
            s = L.Ts2vecStep()
            s.x, s.B, s.T, s.crop_l = xs.data_ptr() + 4 * i * B * T * cin, B, T, d.crop_l
            s.temporal_unit, s.alpha, s.keep_scale, s.x_nan_count = self.temporal_unit, 0.5, keep_scale, 0
            for v in range(2):
                s.view[v].start = starts.data_ptr() + 4 * (2 * i + v) * B
                s.view[v].mask = blob.data_ptr() + offs[i][2 * v]
                s.view[v].keep = blob.data_ptr() + offs[i][2 * v + 1]
                s.view[v].length = d.views[v][1]
            steps.append(s)
        return (xs, starts, blob), steps

    def _fit_hip(self, events, verbose):
        import ctypes as C
        dev, lib = self.device, L.lib()
        draws = [ev[1] for ev in events if ev[0] == "iter"]
        loss_log = []
        self.losses_ = []
        if not draws:
            return loss_log
        n, (B, T, _) = len(draws), draws[0].x.shape
        with torch.cuda.device(dev):
            w, g, tables, n_tensors, chunks, keepalive = self._hip_tables()
            ws_bytes = int(lib.t2s_ts2vec_train_workspace_bytes(C.byref(w), B, T))
            if ws_bytes == 0:
                raise L.T2SError("TS2Vec.fit(engine='hip'): " + lib.t2s_last_error().decode("utf-8", "replace"))
            plan_keep, steps = self._hip_plan(draws)
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            losses = torch.zeros(n, dtype=torch.float32, device=dev)
            stream = L.stream_ptr(dev)
            n_avg0 = int(self.net.n_averaged.item())
            adam_tab, swa_tab = tables.data_ptr(), tables.data_ptr() + 40 * n_tensors
            stepwise = self.after_iter_callback is not None or self.after_epoch_callback is not None
            vals, it, epoch_first = [], 0, 0
            # without callbacks every iteration is enqueued before the first loss is read; with one, each iteration is
            # synchronised so that the callback sees the model of that iteration.  The launches are the same either way.
            for ev in events:
                if ev[0] == "iter":
                    L.check(lib.t2s_ts2vec_train_step(C.byref(w), C.byref(g), C.byref(steps[it]), losses.data_ptr() + 4 * it,
                                                      workspace.data_ptr(), ws_bytes, stream), "t2s_ts2vec_train_step")
                    L.check(lib.t2s_adamw_step_multi(adam_tab, n_tensors, chunks, float(self.lr), 0.9, 0.999, 1e-8, 0.01, it + 1,
                                                     stream), "t2s_adamw_step_multi")
                    L.check(lib.t2s_swa_update_multi(swa_tab, n_tensors, chunks, n_avg0 + it, stream), "t2s_swa_update_multi")
                    it += 1
                    if stepwise:
                        vals.append(losses[it - 1].item())
                        self.net.n_averaged += 1
                        self.n_iters += 1
                        self._hip = None
                        if self.after_iter_callback is not None:
                            self.after_iter_callback(self, vals[-1])
                else:
                    if not stepwise:
                        loss_log.append((epoch_first, it))
                        epoch_first = it
                        continue
                    loss_log.append(sum(vals[epoch_first:it], 0.0) / (it - epoch_first))
                    epoch_first = it
                    if verbose:
                        print(f"Epoch #{self.n_epochs}: loss={loss_log[-1]}")
                    self.n_epochs += 1
                    if self.after_epoch_callback is not None:
                        self.after_epoch_callback(self, loss_log[-1])
            if not stepwise:
                vals = losses.cpu().tolist()
                self.net.n_averaged += n
                self.n_iters += n
                loss_log = [sum(vals[a:b], 0.0) / (b - a) for a, b in loss_log]
                for val in loss_log:
                    if verbose:
                        print(f"Epoch #{self.n_epochs}: loss={val}")
                    self.n_epochs += 1
            for p in list(self._net.parameters()) + list(self.net.module.parameters()):
                torch.autograd.graph.increment_version(p)          # written in place behind autograd's back
            del keepalive, plan_keep
        self._hip = None
        self.losses_ = vals
        return loss_log

    # -- inference on the HIP kernel (ts2vec.py:219-330, the 'full_series' / per-step windows)
    def _encoder(self):
        if self._hip is None:
            from .metrics import TS2VecEncoder
            self._hip = TS2VecEncoder(copy.deepcopy(self.net.module.state_dict()), self.device)
        return self._hip

    def encode(self, data, encoding_window=None, batch_size=None):
        """data (N, T, input_dims) -> the encoder's output, `batch_size` rows at a time.  Any T up to 4096: series whose
        activation planes fit LDS run on t2s_ts2vec_encode, longer ones on t2s_ts2vec_encode_long (TS2VecEncoder.encode)."""
        data = np.asarray(data)
        assert data.ndim == 3
        bs = batch_size or self.batch_size
        enc = self._encoder()
        outs = [enc.encode(torch.from_numpy(data[i:i + bs]).float(), encoding_window=encoding_window).cpu()
                for i in range(0, len(data), bs)]
        return torch.cat(outs, dim=0).numpy()

    def save(self, fn):
        torch.save(self.net.state_dict(), fn)

    def load(self, fn):
        self.net.load_state_dict(torch.load(fn, map_location=self.device))
        self._hip = None


def initialize_ts2vec(X_train, device="cuda", engine=None):
    """ts2vec.py:12-21: the configuration evaluation.py:238 trains for C-FID.  engine: see TS2Vec."""
    model = TS2Vec(input_dims=X_train.shape[-1], device=device, batch_size=8, lr=0.001, output_dims=100, max_train_length=3000,
                   engine=engine)
    model.fit(X_train, verbose=False)
    return model
