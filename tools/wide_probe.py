"""The wide-latent DiT's sampling rate and kernel efficiency at W = 30, 50, 64 (480, 800, 1024 tokens), f32 arithmetic, one MI355X.

    python tools/wide_probe.py [--steps 50] [--rounds 5] [--out profiles/wide_dit.json]

Per (W, B) in {30, 50, 64} x {256, 32}: the fused sampler (DDPM, CFG, Philox noise, whole-loop hipGraph, no decode) -- a
warm-up run of every configuration, then `--rounds` rounds in which the six configurations alternate (the order is reversed
every other round); a run is timed by the host clock between two device synchronisations.  Reported: median and spread
(max - min) of ms per step and series/s.  Then, per configuration, the average launch time of the attention and of the
row-chain kernels measured in situ (HIP events around every kernel of eager CFG forwards: bench.py time_kernels_in_situ) and
their fraction of the fp32 MFMA peak with bench.py's FLOP accounting at N = 16 W tokens: the row chain is linear in N, the
attention is 4 N^2 32 flops per head.

Next to each measured fraction stands what the 480-token figures predict for it (recorded, not gated): the
attention reaches 0.79 of the peak at 480 tokens with 15 of its 16 query-tile slots occupied, the rows 0.73.  At 1024 tokens
(32 tiles in 32 slots) the attention should not be lower than 0.79; at 800 (25 tiles in 32 slots) the idle slots bound it by
25/32 = 0.78, and the 480-token efficiency per occupied slot gives 0.79 x (25/32) / (15/16) = 0.66.  The row chain has no
per-sequence slots: 0.73 at every N.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WIDTHS, BATCHES = (30, 50, 64), (256, 32)
ATTN_FRAC_480, ROWS_FRAC_480 = 0.79, 0.73


def predicted_attention_frac(width):
    """From the 480-token figure: the same efficiency per occupied query-tile slot."""
    tiles = width // 2
    slots = {15: 16, 25: 32, 32: 32}[tiles]
    return ATTN_FRAC_480 * (tiles / slots) / (15 / 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_dit.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wide_probe: needs a GPU (a CPU timing says nothing about these kernels)")
    if a.rounds < 5:
        raise SystemExit("wide_probe: at least 5 rounds")
    import bench
    from model.denoiser.mytransformer import Transformer
    from t2ms_amd import synth
    from t2ms_amd.sampler import Sampler
    dev = torch.device("cuda:0")
    models = {}
    for W in WIDTHS:
        m = Transformer(W)
        m.load_state_dict(synth.make_dit_state_dict(2025, width=W), strict=True)
        models[W] = m.set_math("f32").to(dev).eval()
    configs = [(W, B) for B in BATCHES for W in WIDTHS]
    samplers, texts = {}, {}
    for W, B in configs:
        texts[B] = synth.make_text_embeddings(1, B).to(dev)
        s = Sampler(models[W], None, "ddpm", a.steps, 7.0, B, 96, dev, use_graph=True, loop_graph=1, math="f32")
        s.run(texts[B], decode=False)                                  # buffers, capture, warm-up
        samplers[(W, B)] = s

    def timed(s):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s.run_inplace(decode=False)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    for c in configs:
        timed(samplers[c])
    times = {c: [] for c in configs}
    for r in range(a.rounds):
        for c in (configs if r % 2 == 0 else configs[::-1]):
            times[c].append(timed(samplers[c]))
    rows = []
    for W, B in configs:
        t = times[(W, B)]
        med, n_tok = statistics.median(t), 16 * W
        x = synth.make_wide_latents(3, B, W).to(dev)
        kt = bench.time_kernels_in_situ(models[W], dev, x, texts[B])
        scale = n_tok / 480.0
        flop_attn = 2 * 2 * 4 * n_tok * n_tok * 32 * 2 * B              # per launch: QK^T + PV, 4 heads, 2 B sequences
        flop_rows = sum(f * mult for f, mult in zip(bench.FLOP_ROWS_PER_SEQ.values(), (1, 3, 1))) * scale * 2 * B   # per forward
        attn_frac = flop_attn / (kt["attn_us"] * 1e-6) / 1e12 / bench.PEAK_FP32_MFMA_TFLOPS
        rows_frac = flop_rows / (kt["rows_us"] * kt["rows_calls"] / 8 * 1e-6) / 1e12 / bench.PEAK_FP32_MFMA_TFLOPS
        attn_480 = bench.FLOP_ATTN_PER_SEQ_BLOCK * 4                     # the four attention blocks of a 480-token forward
        whole = (bench.FLOP_FORWARD_PER_SEQ - attn_480) * scale + attn_480 * scale * scale      # linear part, quadratic part
        rows.append({
            "latent_w": W, "tokens": n_tok, "batch": B, "steps": a.steps, "graph_lanes": samplers[(W, B)].graph_lanes,
            "ms_per_step": {"median": med / a.steps * 1e3, "spread": (max(t) - min(t)) / a.steps * 1e3},
            "series_per_s": {"median": B / med, "spread": B / min(t) - B / max(t)},
            "whole_path_frac_of_fp32_mfma_peak": whole * 2 * B * a.steps / med / 1e12 / bench.PEAK_FP32_MFMA_TFLOPS,
            "attention": {"avg_launch_us": kt["attn_us"], "frac_of_fp32_mfma_peak": attn_frac,
                          "predicted_from_480": predicted_attention_frac(W),
                          "occupied_tile_slots": f"{W // 2}/{ {15: 16, 25: 32, 32: 32}[W // 2] }"},
            "rows": {"avg_launch_us": kt["rows_us"], "frac_of_fp32_mfma_peak": rows_frac, "predicted_from_480": ROWS_FRAC_480},
        })
        print(json.dumps(rows[-1]))
    result = {"device": torch.cuda.get_device_name(0), "math": "f32", "backbone": "ddpm, CFG 7, Philox noise, whole-loop graph, no decode",
              "rounds": a.rounds, "peak_fp32_mfma_tflops": bench.PEAK_FP32_MFMA_TFLOPS,
              "prediction": "attention 0.79 and rows 0.73 of the fp32 MFMA peak at 480 tokens (B 256); attention scaled by the share of "
                            "occupied query-tile slots, rows unchanged", "configs": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
