/* libt2s_hip.so -- the evaluation of the T2MS motion runs (the reference's myevaluation.py): every clip of a test split, each
 * with its own length and its `runs` samples, scored in ONE call over the packed ragged layout of t2s_vae_decode_mc_ragged /
 * t2s_sampler_set_lengths.  An extension of t2s.h: that header's entry list stays as it is; t2ms_amd/_lib.py lists this entry
 * under SYMBOLS_EVAL_RUNS. */
#ifndef T2S_EVAL_RUNS_H
#define T2S_EVAL_RUNS_H

#include "t2s.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2S_EVAL_RUNS_MAX_CHANNELS 16   /* the multichannel codec's own limit */

/* myevaluation.py's per-clip scores.  For clip i with recording x_1 (channels, T_i) and samples x_t[r] (channels, T_i), r < runs:
 *   normalize(x) = (x - lo) / ((hi - lo) + 1e-8f) per channel row along time, lo / hi the row's min / max  (fp32, bit for bit
 *                  numpy's on float32 arrays: a NaN in a row makes lo and hi NaN as np.min / np.max do, Inf follows IEEE, a
 *                  constant row gives exact zeros).  One exception: a row whose minimum is zero and which holds zeros of BOTH
 *                  signs.  numpy takes the sign of lo from its reduction order there, which is not defined; this entry orders
 *                  the zeros (-0 < +0), so lo = -0 and every zero of that row normalises to +0, whatever the order of the
 *                  values, where numpy may give -0 for the row's -0 entries.  Values other than those zeros are not affected
 *                  (x - lo is the same for either sign of a zero lo when x != 0)
 *   a = normalize(x_t[r]), b = normalize(x_1); the reference hands the SAMPLES over as `ori` and reads the channel axis as time:
 *   mse[r]  = mean over (c, t) of (a - b)^2
 *   wape[r] = sum |a - b| / sum |a|                       (NaN when that denominator is exactly 0)
 *   ed[r]   = mean over t of sqrt(sum_c (a[c,t] - b[c,t])^2)
 *   dtw[r]  = sqrt of the minimal warping cost between the `channels` points a[i,:] and b[j,:] of T_i dimensions,
 *             cost[i][j] = sum_t (a[i,t] - b[j,t])^2, no window, no penalty (the recurrence of t2s_eval_dtw)
 * Every sum runs over the normalised fp32 values in fp64 in an order that depends on (channels, T_i) alone -- not on the grid,
 * the clip's place in the batch or `runs` -- and is rounded once to fp32; no floating-point atomics.  So a call repeats bit for
 * bit, a clip evaluated alone gives the bits it gives inside a batch, and runs never interact.
 *
 * Device arrays: x1 = `clips` packed rows, clip i is (channels, T_i) row-major at x1 + channels * offsets[i]; xt = (runs, the same
 * packing), run-major (run r at xt + r * channels * offsets[clips]); lengths (clips) int32; offsets (clips + 1) uint64, the
 * prefix sums of lengths.  Host: clips >= 1, runs >= 1, 1 <= channels <= T2S_EVAL_RUNS_MAX_CHANNELS, 1 <= max_T <=
 * T2S_EVAL_MOTION_MAX_LEN (every T_i <= max_T).
 * Outputs: per_run (clips, runs, 4) = [mse, wape, ed, dtw]; per_clip (clips, 4) = over the runs' fp32 values the mean, the
 * mean of those that are not NaN (NaN when none is left), the mean, the mean; out (4) = the plain mean of those per-clip
 * values (before their rounding) over the evaluated clips (a NaN clip value propagates; NaN when no clip was evaluated);
 * norm1 / normt = the normalised planes in the layout of x1 / xt (the entry's workspace, and the input of the feature
 * measures and C-FID).
 * A clip is SKIPPED -- nothing of it read, nothing of it written in per_run, per_clip, norm1, normt -- when T_i is outside
 * [1, max_T] or offsets[i + 1] - offsets[i] != T_i: a kernel never leaves the span a row's own offsets give it.
 * Three launches (normalise, score, reduce) whatever clips and runs; the caller's stream; no allocation, copy, synchronisation
 * or state: usable inside a captured graph.  T2S_E_INVALID with the entry's name and the offending value in t2s_last_error,
 * before any launch, for a NULL pointer or a host value outside the ranges above. */
int t2s_eval_runs(const float* x1, const float* xt, const int32_t* lengths, const uint64_t* offsets, float* per_run,
                  float* per_clip, float* out, float* norm1, float* normt, int clips, int runs, int channels, int max_T,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* T2S_EVAL_RUNS_H */
