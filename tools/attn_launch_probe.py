#!/usr/bin/env python3
"""Time `t2s_attn_fwd_packed` alone at the headline's launch shapes (1024 heads: one of two sampler lanes; 2048: one lane),
on random data, and print a digest of the output.  The launch-form switches are read once per process, so one process is one
arm: alternate `T2S_ATTN_QUAD=0|1` (or `T2S_LIB=<other build>`) on one box and compare (profiles/r06_attn_quad_ab.txt).

    T2S_ATTN_QUAD=0 python tools/attn_launch_probe.py ; T2S_ATTN_QUAD=1 python tools/attn_launch_probe.py
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from t2ms_amd import _lib as L  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    out = []
    for n_seq in (256, 512):
        g = torch.Generator(device="cpu").manual_seed(n_seq)
        n = n_seq * 4 * 480 * 32
        q, k, v = (torch.randn(n, generator=g).to(dev) for _ in range(3))
        o = torch.full((n,), float("nan"), device=dev)
        st = L.stream_ptr(dev)

        def call():
            L.check(L.lib().t2s_attn_fwd_packed(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), n_seq, st))

        for _ in range(30):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 10.0)
        digest = hashlib.sha1(o.cpu().numpy().tobytes()).hexdigest()[:12]
        out.append(f"{n_seq * 4} heads: us/launch min {min(ts):.2f} median {sorted(ts)[2]:.2f} max {max(ts):.2f} sha1 {digest}")
    print(os.path.basename(os.environ.get("T2S_LIB", "in-tree")), "T2S_ATTN_QUAD=" + os.environ.get("T2S_ATTN_QUAD", "(unset)"),
          " | ".join(out))


if __name__ == "__main__":
    main()
