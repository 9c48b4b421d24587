// t2s_eval_runs (include/t2s_eval_runs.h): the reference's myevaluation.py over every clip of a motion test split in one call.
// Clips have their own lengths, so the arrays are the packed ragged layout of t2s_vae_decode_mc_ragged: clip i is a
// (C, T_i) block at C * offsets[i]; the samples are `runs` such packings, run-major.
//
// Three launches, whatever the number of clips and runs:
//   runs_normalize_kernel   one workgroup per (plane, clip), plane 0 = the recording, 1 + r = run r; a wave per channel row:
//                           the row's min / max (a NaN stays, as in np.min / np.max), then (x - lo) / ((hi - lo) + 1e-8f) in fp32
//   runs_score_kernel       one workgroup per (clip, run): 64-step tiles of the two normalised (C, 64) planes in LDS; thread
//                           (i, j) adds cost[i][j] = sum_t (a[i,t] - b[j,t])^2 in fp64 in time order; the last wave's lane t
//                           takes column t of the tile for ED and WAPE; then wave 0 walks the C x C DTW table by anti-diagonals
//   runs_reduce_kernel      one workgroup: per clip the reductions over runs, then the mean over the evaluated clips
// Every sum is fp64 over the fp32 normalised values in an order fixed by (C, T_i) alone and rounded once; no atomics.
#include "t2s_common.h"
#include "../../include/t2s_eval_runs.h"

namespace t2s {
namespace {

constexpr int RUNS_MAX_C = T2S_EVAL_RUNS_MAX_CHANNELS;         // 16
constexpr int RUNS_MAX_T = T2S_EVAL_MOTION_MAX_LEN;            // 4096
constexpr int RUNS_TILE = 64;                                  // time steps staged at once
constexpr int RUNS_LD = RUNS_TILE + 1;                         // row stride of a staged plane: rows fall on distinct LDS banks
constexpr int RUNS_COL_WAVE = 3;                               // the wave that takes the tile's columns (ED, WAPE)

// the length of clip i, or 0 when the clip is skipped: T_i outside [1, max_T], or offsets that do not span it
__device__ __forceinline__ int runs_len(const int32_t* __restrict__ lengths, const uint64_t* __restrict__ offsets, int i, int max_T) {
    const int T = lengths[i];
    return (T >= 1 && T <= max_T && offsets[i + 1] - offsets[i] == (uint64_t)T) ? T : 0;
}

// np.minimum / np.maximum: a NaN on either side stays (fminf / fmaxf would drop it).  Zeros are ordered, -0 < +0, so the
// result does not depend on the order of the operands (numpy's own choice among zeros of both signs follows its reduction
// order; t2s_eval_runs.h states the one case where that shows)
__device__ __forceinline__ float runs_min(float a, float b) { return (a < b || a != a || (a == b && __builtin_signbit(a))) ? a : b; }
__device__ __forceinline__ float runs_max(float a, float b) { return (a > b || a != a || (a == b && !__builtin_signbit(a))) ? a : b; }

__global__ __launch_bounds__(256) void runs_normalize_kernel(const float* __restrict__ x1, const float* __restrict__ xt,
                                                             const int32_t* __restrict__ lengths, const uint64_t* __restrict__ offsets,
                                                             float* __restrict__ norm1, float* __restrict__ normt, int clips, int C,
                                                             int max_T) {
    const int plane = blockIdx.x / clips, clip = blockIdx.x - plane * clips;
    const int T = runs_len(lengths, offsets, clip, max_T);
    if (T == 0) return;
    const size_t at = (size_t)C * offsets[clip] + (plane == 0 ? 0 : (size_t)(plane - 1) * C * offsets[clips]);
    const float* src = (plane == 0 ? x1 : xt) + at;
    float* dst = (plane == 0 ? norm1 : normt) + at;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += 4) {
        const float* row = src + (size_t)c * T;
        float lo = row[0], hi = lo;                             // T >= 1
        for (int t = lane; t < T; t += 64) {
            const float v = row[t];
            lo = runs_min(lo, v);
            hi = runs_max(hi, v);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo = runs_min(lo, __shfl_xor(lo, o, 64));
            hi = runs_max(hi, __shfl_xor(hi, o, 64));
        }
        lo = __shfl(lo, 0, 64);
        hi = __shfl(hi, 0, 64);
        const float den = (hi - lo) + 1e-8f;
        for (int t = lane; t < T; t += 64) dst[(size_t)c * T + t] = (row[t] - lo) / den;
    }
}

__global__ __launch_bounds__(256) void runs_score_kernel(const float* __restrict__ norm1, const float* __restrict__ normt,
                                                         const int32_t* __restrict__ lengths, const uint64_t* __restrict__ offsets,
                                                         float* __restrict__ per_run, int clips, int runs, int C, int max_T) {
    __shared__ float sa[RUNS_MAX_C * RUNS_LD], sb[RUNS_MAX_C * RUNS_LD];
    __shared__ double table[RUNS_MAX_C * RUNS_MAX_C];
    __shared__ double cols[3];
    const int clip = blockIdx.x / runs, run = blockIdx.x - clip * runs;
    const int T = runs_len(lengths, offsets, clip, max_T);
    if (T == 0) return;
    const float* b = norm1 + (size_t)C * offsets[clip];                                        // the recording
    const float* a = normt + (size_t)run * C * offsets[clips] + (size_t)C * offsets[clip];     // the sample
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = tid >> 4, j = tid & 15;
    const bool cell = i < C && j < C;
    double cost = 0.0, ed = 0.0, num = 0.0, den = 0.0;
    for (int t0 = 0; t0 < T; t0 += RUNS_TILE) {
        const int n = T - t0 < RUNS_TILE ? T - t0 : RUNS_TILE;
        for (int e = tid; e < C * RUNS_TILE; e += 256) {
            const int c = e >> 6, t = e & 63;
            if (t < n) {
                sa[c * RUNS_LD + t] = a[(size_t)c * T + t0 + t];
                sb[c * RUNS_LD + t] = b[(size_t)c * T + t0 + t];
            }
        }
        __syncthreads();
        if (cell) {
            const float* pa = sa + i * RUNS_LD;
            const float* pb = sb + j * RUNS_LD;
            for (int t = 0; t < n; ++t) {
                const double d = (double)pa[t] - (double)pb[t];
                cost += d * d;
            }
        }
        if (wave == RUNS_COL_WAVE && lane < n) {
            double q = 0.0;
            for (int c = 0; c < C; ++c) {
                const double av = (double)sa[c * RUNS_LD + lane];
                const double d = av - (double)sb[c * RUNS_LD + lane];
                q += d * d;
                num += fabs(d);
                den += fabs(av);
            }
            ed += sqrt(q);
        }
        __syncthreads();
    }
    if (cell) table[i * RUNS_MAX_C + j] = cost;
    if (wave == RUNS_COL_WAVE) {                               // lane t holds the columns t, t + 64, ...: one fixed tree over the lanes
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ed += __shfl_xor(ed, o, 64);
            num += __shfl_xor(num, o, 64);
            den += __shfl_xor(den, o, 64);
        }
        if (lane == 0) { cols[0] = ed; cols[1] = num; cols[2] = den; }
    }
    __syncthreads();
    if (wave != 0) return;
    // DTW over the C x C table: lane i owns row i and takes cell (i, d - i) of anti-diagonal d; p1 / p2 are its cells on the
    // diagonals d - 1 / d - 2 (+inf where it has none), the row above comes by a lane shift.  eval_dtw_kernel's operations.
    const double INF = __builtin_inf();
    double p1 = INF, p2 = INF;
    for (int d = 0; d <= 2 * C - 2; ++d) {
        double up = __shfl_up(p1, 1, 64), dg = __shfl_up(p2, 1, 64);      // (i-1, j) and (i-1, j-1)
        if (lane == 0) { up = INF; dg = INF; }
        const int jj = d - lane;
        double cur = INF;
        if (lane < C && jj >= 0 && jj < C) {
            double best = 0.0;
            if (d != 0) {
                best = fmin(dg, fmin(up, p1));                            // p1: (i, j-1)
                if (up != up || p1 != p1 || dg != dg) best = __builtin_nan("");   // fmin drops a NaN: keep it
            }
            cur = table[lane * RUNS_MAX_C + jj] + best;
        }
        p2 = p1;
        p1 = cur;
    }
    if (lane == C - 1) {
        double diag = 0.0;
        for (int c = 0; c < C; ++c) diag += table[c * RUNS_MAX_C + c];
        float* o = per_run + ((size_t)clip * runs + run) * 4;
        o[0] = (float)(diag / ((double)C * (double)T));
        o[1] = cols[2] == 0.0 ? __builtin_nanf("") : (float)(cols[1] / cols[2]);
        o[2] = (float)(cols[0] / (double)T);
        o[3] = (float)sqrt(p1);
    }
}

// one workgroup.  Thread k takes the clips k, k + 256, ...: per clip the four reductions over the runs' fp32 values in run
// order, then its share of the sum over clips (of the clip means before their rounding); the shares are folded by one fixed tree.
__global__ __launch_bounds__(256) void runs_reduce_kernel(const float* __restrict__ per_run, const int32_t* __restrict__ lengths,
                                                          const uint64_t* __restrict__ offsets, float* __restrict__ per_clip,
                                                          float* __restrict__ out, int clips, int runs, int max_T) {
    __shared__ double red[5][256];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, count = 0.0;
    for (int clip = threadIdx.x; clip < clips; clip += 256) {
        if (runs_len(lengths, offsets, clip, max_T) == 0) continue;
        const float* v = per_run + (size_t)clip * runs * 4;
        double mse = 0.0, wape = 0.0, ed = 0.0, dtw = 0.0;
        int kept = 0;
        for (int r = 0; r < runs; ++r) {
            const float w = v[4 * r + 1];
            mse += (double)v[4 * r];
            if (w == w) { wape += (double)w; ++kept; }           // np.nanmean
            ed += (double)v[4 * r + 2];
            dtw += (double)v[4 * r + 3];
        }
        const double c0 = mse / (double)runs, c1 = kept == 0 ? __builtin_nan("") : wape / (double)kept;
        const double c2 = ed / (double)runs, c3 = dtw / (double)runs;
        float* o = per_clip + (size_t)clip * 4;
        o[0] = (float)c0; o[1] = (float)c1; o[2] = (float)c2; o[3] = (float)c3;
        s0 += c0; s1 += c1; s2 += c2; s3 += c3;                  // the summary is rounded once too: from the fp64 clip means
        count += 1.0;
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2; red[3][threadIdx.x] = s3;
    red[4][threadIdx.x] = count;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int m = 0; m < 5; ++m) red[m][threadIdx.x] += red[m][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) out[threadIdx.x] = red[4][0] == 0.0 ? __builtin_nanf("") : (float)(red[threadIdx.x][0] / red[4][0]);
}

}  // namespace
}  // namespace t2s

extern "C" int t2s_eval_runs(const float* x1, const float* xt, const int32_t* lengths, const uint64_t* offsets, float* per_run,
                             float* per_clip, float* out, float* norm1, float* normt, int clips, int runs, int channels, int max_T,
                             void* stream) {
    using namespace t2s;
    const char* who = "t2s_eval_runs";
    T2S_REQUIRE(x1 && xt && lengths && offsets, "%s: x1, xt, lengths and offsets must not be NULL", who);
    T2S_REQUIRE(per_run && per_clip && out && norm1 && normt, "%s: per_run, per_clip, out, norm1 and normt must not be NULL", who);
    T2S_REQUIRE(clips >= 1, "%s: clips=%d", who, clips);
    T2S_REQUIRE(runs >= 1, "%s: runs=%d", who, runs);
    T2S_REQUIRE(channels >= 1 && channels <= RUNS_MAX_C, "%s: channels=%d is outside [1, %d]", who, channels, RUNS_MAX_C);
    T2S_REQUIRE(max_T >= 1 && max_T <= RUNS_MAX_T, "%s: max_T=%d is outside [1, %d]", who, max_T, RUNS_MAX_T);
    T2S_REQUIRE((uint64_t)clips * ((uint64_t)runs + 1) <= 0x7fffffffull, "%s: clips=%d x runs=%d exceed one launch", who, clips, runs);
    hipStream_t st = (hipStream_t)stream;
    runs_normalize_kernel<<<(unsigned)clips * ((unsigned)runs + 1), 256, 0, st>>>(x1, xt, lengths, offsets, norm1, normt, clips,
                                                                                   channels, max_T);
    T2S_LAUNCH_CHECK();
    runs_score_kernel<<<(unsigned)clips * (unsigned)runs, 256, 0, st>>>(norm1, normt, lengths, offsets, per_run, clips, runs,
                                                                        channels, max_T);
    T2S_LAUNCH_CHECK();
    runs_reduce_kernel<<<1, 256, 0, st>>>(per_run, lengths, offsets, per_clip, out, clips, runs, max_T);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
