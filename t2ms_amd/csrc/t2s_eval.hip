// Reconstruction metrics of the generate -> evaluate loop on the GPU: MSE and WAPE exactly as
// evaluation.py:166-206 defines them on the (N, L, n_series) arrays infer.py writes (x_1.npy / x_t.npy).
//   mse_i  = mean over (L, series) of (ori - gen)^2              MSE  = mean_i mse_i
//   wape_i = sum |ori - gen| / sum |ori|   (NaN if the sum is 0)  WAPE = nanmean_i wape_i
// Deterministic: one wave per sample with a fixed summation order, then one workgroup over the samples.
//
// MRR as evaluation.py:21-45 defines it over the G generated runs of each sample (x_t.npy of run_0..run_{G-1}):
//   sim_g = <ori, gen_g> / (|ori| |gen_g|) over the flattened (L, series) values, 0 where that is not finite
//   (cosine_similarity, Dataset_Construction_Pipeline/Evaluate_Datasets.py:6-15 with nan_to_num);
//   the runs are visited by descending sim and the first one above the threshold ends the visit, so only the
//   best run can: score_i = 1 / (g* + 1) if sim_{g*} > threshold else 0, where g* is the RUN INDEX of the best
//   run (evaluation.py:37-41 take `idx + 1` of the argsort entry, not its position); ties go to the largest
//   index (reversed stable argsort).  MRR = mean_i score_i.
//
// Feature-based measures of evaluate/feature_based_measures.py on two SETS ori ("real") and gen ("fake") of shape
// (n, L, n_series); none of them pairs row i with row i.  Per channel c, over all n*L values x of the channel, centred by
// the channel mean (two passes: the mean first, then centred sums, fp64 throughout), N = n*L, K = min(64, L):
//   lag_k  = sum_{i, t >= k} x[i,t] x[i,t-k]            acf_k = (lag_k / (n (L-k))) / var_pop,  var_pop = lag_0 / N  (:98-109)
//   ACD    = mean_c sqrt(sum_k (acf_k(gen) - acf_k(ori))^2)                                                        (:155-161)
//   skew   = (sum x^3 / N) / std^3,  std^2 = lag_0 / (N-1)       SD = mean_c |skew(gen) - skew(ori)|     (:165-172,183-191)
//   kurt   = (sum x^4 / N) / var_pop^2 - 3                       KD = mean_c |kurt(gen) - kurt(ori)|     (:195-204,215-223)
// The samples are cut into P = min(n, 1024) chunks (a function of n alone); a workgroup sums one chunk in a fixed order
// and a fold kernel adds the P partials in index order: the grid never changes a bit of the result.
// MDD (HistoLoss + histogram_torch, :30-94), per column (t, c) = the n values ori[:, t, c]:
//   a = min, b = max of the real column (b = a + 1e-5 when b == a); 50 equal bins on [a, b], delta = (b - a) / 50 (fp64
//   here); real count: bin floor((x - a) / (b - a) 50), x == b in the last bin (torch.histc);
//   fake count of bin k: the fake values with delta/2 - |x - centre_k| > 0, which off a bin edge is the real side's
//   binning restricted to [a, b] -- the kernel bins both sides with that one rule (ON an edge the reference's own answer
//   hangs on the rounding of its fp32 centres; here the value goes to the upper bin, and b to the last);
//   loss(t, c) = mean_k |count_gen[k] - count_ori[k]| / (n delta);  MDD = mean over the L*n_series columns.
// Counts are integers added with LDS / global integer atomics: exact under any split of n over workgroups.
#include "t2s_common.h"

namespace t2s {
namespace {

__global__ __launch_bounds__(64) void eval_per_sample_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                             float* __restrict__ per_sample, int len) {
    const int i = blockIdx.x;
    const float* a = ori + (size_t)i * len;
    const float* b = gen + (size_t)i * len;
    float se = 0.f, ae = 0.f, av = 0.f;
    for (int k = threadIdx.x; k < len; k += 64) {
        const float d = a[k] - b[k];
        se += d * d;
        ae += fabsf(d);
        av += fabsf(a[k]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        se += __shfl_xor(se, o, 64);
        ae += __shfl_xor(ae, o, 64);
        av += __shfl_xor(av, o, 64);
    }
    if (threadIdx.x == 0) {
        per_sample[2 * i] = se / (float)len;
        per_sample[2 * i + 1] = av != 0.f ? ae / av : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void eval_reduce_kernel(const float* __restrict__ per_sample, float* __restrict__ out, int n) {
    __shared__ double red[3][256];
    double sm = 0.0, sw = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        sm += (double)per_sample[2 * i];
        const float w = per_sample[2 * i + 1];
        if (w == w) { sw += (double)w; cnt += 1.0; }
    }
    red[0][threadIdx.x] = sm; red[1][threadIdx.x] = sw; red[2][threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(red[0][0] / (double)n);
        out[1] = red[2][0] > 0.0 ? (float)(red[1][0] / red[2][0]) : __builtin_nanf("");
    }
}

// one wave per sample: double accumulation, so the only rounding is the final cast of each similarity
__global__ __launch_bounds__(64) void eval_mrr_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                      float* __restrict__ sims, float* __restrict__ score,
                                                      int n, int len, int runs, float threshold) {
    const int i = blockIdx.x;
    const float* a = ori + (size_t)i * len;
    double aa = 0.0;
    for (int k = threadIdx.x; k < len; k += 64) aa += (double)a[k] * (double)a[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) aa += __shfl_xor(aa, o, 64);
    float best = 0.f;
    int best_g = -1;
    for (int g = 0; g < runs; ++g) {
        const float* b = gen + ((size_t)g * n + i) * len;
        double ab = 0.0, bb = 0.0;
        for (int k = threadIdx.x; k < len; k += 64) {
            ab += (double)a[k] * (double)b[k];
            bb += (double)b[k] * (double)b[k];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ab += __shfl_xor(ab, o, 64);
            bb += __shfl_xor(bb, o, 64);
        }
        const double den = sqrt(aa) * sqrt(bb);
        float sf = den > 0.0 ? (float)(ab / den) : 0.f;         // 0/0 -> NaN -> nan_to_num -> 0 (a zero vector)
        if (!isfinite(sf)) sf = 0.f;                            // an Inf in either vector: inf/inf -> NaN -> 0, and it competes as 0
        if (best_g < 0 || sf >= best) { best = sf; best_g = g; }
        if (threadIdx.x == 0) sims[(size_t)i * runs + g] = sf;
    }
    if (threadIdx.x == 0) score[i] = (best_g >= 0 && best > threshold) ? 1.f / (float)(best_g + 1) : 0.f;
}

__global__ __launch_bounds__(256) void eval_mean_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(red[0] / (double)n);
}


// ---- ED (evaluation.py:137-150): per sample the mean over series of || ori[:, j] - gen[:, j] ||_2 over time
__global__ __launch_bounds__(64) void eval_ed_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                     float* __restrict__ per_sample, int L, int S) {
    const int i = blockIdx.x;
    const float* a = ori + (size_t)i * L * S;
    const float* b = gen + (size_t)i * L * S;
    double total = 0.0;
    for (int j = 0; j < S; ++j) {
        double ss = 0.0;
        for (int t = threadIdx.x; t < L; t += 64) {
            const double d = (double)a[t * S + j] - (double)b[t * S + j];
            ss += d * d;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
        total += sqrt(ss);
    }
    if (threadIdx.x == 0) per_sample[i] = (float)(total / (double)S);
}

// ---- CRPS (evaluation.py:51-83): per (sample, series, run) a Gaussian N(mean, std) fitted to the generated series over
// TIME (population std, 1e-8 when 0); mean over time of (1[obs >= mean] - Phi((obs - mean) / std))^2; then the mean over
// runs and series.  gen is run-major (runs, n, L, S).  One wave per sample, fp64 statistics.
__global__ __launch_bounds__(64) void eval_crps_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                       float* __restrict__ per_sample, int n, int L, int S, int runs) {
    const int i = blockIdx.x;
    const float* a = ori + (size_t)i * L * S;
    double total = 0.0;
    for (int j = 0; j < S; ++j) {
        double over_runs = 0.0;
        for (int k = 0; k < runs; ++k) {
            const float* g = gen + ((size_t)k * n + i) * L * S;
            double sm = 0.0;
            for (int t = threadIdx.x; t < L; t += 64) sm += (double)g[t * S + j];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sm += __shfl_xor(sm, o, 64);
            const double mean = sm / (double)L;
            double sv = 0.0;
            for (int t = threadIdx.x; t < L; t += 64) {
                const double d = (double)g[t * S + j] - mean;
                sv += d * d;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sv += __shfl_xor(sv, o, 64);
            // the reference takes mean / std of float32 data in float32 and compares float32 values
            const float meanf = (float)mean;
            float stdf = (float)sqrt(sv / (double)L);
            if (stdf == 0.f) stdf += 1e-8f;
            double acc = 0.0;
            for (int t = threadIdx.x; t < L; t += 64) {
                const float obs = a[t * S + j];
                const double step = obs < meanf ? 0.0 : 1.0;
                const double z = ((double)obs - (double)meanf) / (double)stdf;
                const double cdf = 0.5 * erfc(-z * 0.70710678118654752440);
                acc += (step - cdf) * (step - cdf);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
            over_runs += acc / (double)L;
        }
        total += over_runs / (double)runs;
    }
    if (threadIdx.x == 0) per_sample[i] = (float)(total / (double)S);
}

// ---- DTW (evaluation.py:152-163 = dtaidistance dtw_ndim.distance, no window / penalty): sqrt of the minimal warping-path
// cost with squared-Euclidean point costs between the (L, S) sequences.  One workgroup per sample walks the anti-diagonals
// of the L x L table (cells of a diagonal are independent); three diagonals of fp64 partial costs live in LDS.
__global__ __launch_bounds__(256) void eval_dtw_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                       float* __restrict__ per_sample, int L, int S) {
    extern __shared__ double diag[];          // [3][L]
    const int smp = blockIdx.x;
    const float* a = ori + (size_t)smp * L * S;
    const float* b = gen + (size_t)smp * L * S;
    const double INF = 1e300;
    for (int d = 0; d <= 2 * L - 2; ++d) {
        double* cur = diag + (d % 3) * L;
        const double* p1 = diag + ((d + 2) % 3) * L;    // diagonal d-1, indexed by row i
        const double* p2 = diag + ((d + 1) % 3) * L;    // diagonal d-2
        const int lo = d - (L - 1) > 0 ? d - (L - 1) : 0, hi = d < L - 1 ? d : L - 1;
        for (int i = lo + (int)threadIdx.x; i <= hi; i += 256) {
            const int j = d - i;
            double c = 0.0;
            for (int s = 0; s < S; ++s) {
                const double df = (double)a[i * S + s] - (double)b[j * S + s];
                c += df * df;
            }
            double best;
            if (i == 0 && j == 0) {
                best = 0.0;
            } else {
                const double up = i > 0 ? p1[i - 1] : INF;                 // (i-1, j)   on diagonal d-1
                const double left = j > 0 ? p1[i] : INF;                   // (i, j-1)   on diagonal d-1
                const double dg = (i > 0 && j > 0) ? p2[i - 1] : INF;      // (i-1, j-1) on diagonal d-2
                best = fmin(dg, fmin(up, left));
                if (up != up || left != left || dg != dg) best = __builtin_nan("");   // fmin drops a NaN: keep it, every path crosses its row
            }
            cur[i] = c + best;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) per_sample[smp] = (float)sqrt(diag[((2 * L - 2) % 3) * L + (L - 1)]);
}

// ---- feature-based measures (evaluate/feature_based_measures.py): see the head of this file
constexpr int FEAT_MAX_LAG = T2S_EVAL_MAX_LAG;     // 64: ACFLoss(max_lag=64)
constexpr int FEAT_BINS = T2S_EVAL_MDD_BINS;       // 50: calculate_mdd's n_bins
constexpr int FEAT_MAX_CHUNKS = 1024;
constexpr int FEAT_TILE = 64;                      // columns per MDD workgroup: one wave along the contiguous (t, c) axis

struct FeatLayout {          // byte offsets into the caller's workspace; a function of (n, L, n_series) alone
    int P, K;
    size_t cols;
    size_t mean_part, stat_part, chan, minmax, counts, col_loss, total;
};

__host__ __device__ inline int feat_lags(int L) { return L < FEAT_MAX_LAG ? L : FEAT_MAX_LAG; }

inline FeatLayout feat_layout(int n, int L, int S) {
    FeatLayout w{};
    w.P = n < FEAT_MAX_CHUNKS ? n : FEAT_MAX_CHUNKS;
    w.K = feat_lags(L);
    w.cols = (size_t)L * S;
    size_t o = 0;
    w.mean_part = o; o += (size_t)2 * w.P * S * sizeof(double);
    w.stat_part = o; o += (size_t)2 * w.P * S * (2 + w.K) * sizeof(double);
    w.chan = o;      o += (((size_t)3 * S * sizeof(float)) + 15) / 16 * 16;
    w.minmax = o;    o += (size_t)2 * w.cols * sizeof(unsigned);
    w.counts = o;    o += (size_t)2 * FEAT_BINS * w.cols * sizeof(unsigned);
    w.col_loss = o;  o += w.cols * sizeof(float);
    w.total = (o + 255) / 256 * 256;
    return w;
}

// sum of one double per thread of a 256-thread workgroup, the same tree on every call; every thread gets the sum
__device__ __forceinline__ double feat_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// the channel mean from the P chunk sums, folded the same way by whoever needs it
__device__ __forceinline__ double feat_mean(const double* __restrict__ part, int P, int S, int c, double count, double* red) {
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) s += part[(size_t)p * S + c];
    return feat_block_sum(s, red) / count;
}

// grid (P, 2): chunk p of set blockIdx.y -> mean_part[set][p][c] = sum of the chunk's values of channel c
__global__ __launch_bounds__(256) void feat_sum_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                       double* __restrict__ mean_part, int n, int L, int S) {
    __shared__ double red[256];
    const int P = gridDim.x, p = blockIdx.x, set = blockIdx.y;
    const size_t s0 = (size_t)p * n / P, s1 = (size_t)(p + 1) * n / P;
    const float* x = (set ? gen : ori) + s0 * L * S;
    const size_t cnt = (s1 - s0) * L;
    for (int c = 0; c < S; ++c) {
        double s = 0.0;
        for (size_t j = threadIdx.x; j < cnt; j += 256) s += (double)x[j * S + c];
        s = feat_block_sum(s, red);
        if (threadIdx.x == 0) mean_part[((size_t)set * P + p) * S + c] = s;
    }
}

// grid (P, 2), dynamic LDS = L doubles: per channel the chunk's centred sums [sum x^3, sum x^4, lag_0 .. lag_{K-1}].
// A series of one channel is staged centred in LDS; lane k of wave w adds x[t] x[t-k] for t = w, w+4, ...: x[t] is a
// broadcast and x[t-k] 64 consecutive doubles, so neither read conflicts.
__global__ __launch_bounds__(256) void feat_stats_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                         const double* __restrict__ mean_part, double* __restrict__ stat_part,
                                                         int n, int L, int S) {
    extern __shared__ double xs[];
    __shared__ double red[256];
    const int P = gridDim.x, p = blockIdx.x, set = blockIdx.y, K = feat_lags(L);
    const size_t s0 = (size_t)p * n / P, s1 = (size_t)(p + 1) * n / P;
    const float* x = set ? gen : ori;
    const int k = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = 0; c < S; ++c) {
        const double mean = feat_mean(mean_part + (size_t)set * P * S, P, S, c, (double)n * (double)L, red);
        double lag = 0.0, m3 = 0.0, m4 = 0.0;
        for (size_t i = s0; i < s1; ++i) {
            const float* row = x + i * L * S + c;
            for (int t = threadIdx.x; t < L; t += 256) {
                const double d = (double)row[(size_t)t * S] - mean, d2 = d * d;
                xs[t] = d;
                m3 += d2 * d;
                m4 += d2 * d2;
            }
            __syncthreads();
            if (k < K)
                for (int t = w; t < L; t += 4)
                    if (t >= k) lag += xs[t] * xs[t - k];
            __syncthreads();
        }
        double* dst = stat_part + (((size_t)set * P + p) * S + c) * (2 + K);
        m3 = feat_block_sum(m3, red);
        m4 = feat_block_sum(m4, red);
        red[threadIdx.x] = lag;                       // [wave][lag]
        __syncthreads();
        if ((int)threadIdx.x < K) dst[2 + k] = ((red[k] + red[64 + k]) + red[128 + k]) + red[192 + k];
        if (threadIdx.x == 0) { dst[0] = m3; dst[1] = m4; }
        __syncthreads();
    }
}

// grid (n_series): folds the P partials of channel c in index order, derives mean / var / skew / kurt / acf of both
// sets (-> stats[set][c][4 + K] when asked for) and the channel's three differences -> chan[3][S]
__global__ __launch_bounds__(256) void feat_fold_kernel(const double* __restrict__ mean_part, const double* __restrict__ stat_part,
                                                        float* __restrict__ stats, float* __restrict__ chan,
                                                        int n, int L, int S, int P) {
    __shared__ double red[256];
    __shared__ double tot[2][2 + FEAT_MAX_LAG];
    __shared__ double mean[2];
    const int c = blockIdx.x, K = feat_lags(L);
    const double N = (double)n * (double)L;
    for (int set = 0; set < 2; ++set) {
        const double m = feat_mean(mean_part + (size_t)set * P * S, P, S, c, N, red);
        if (threadIdx.x == 0) mean[set] = m;
    }
    if ((int)threadIdx.x < 2 * (2 + K)) {
        const int set = threadIdx.x / (2 + K), j = threadIdx.x - set * (2 + K);
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += stat_part[(((size_t)set * P + p) * S + c) * (2 + K) + j];
        tot[set][j] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double skew[2], kurt[2], var[2];
        for (int set = 0; set < 2; ++set) {
            var[set] = tot[set][2] / N;
            const double sd = sqrt(tot[set][2] / (N - 1.0));
            skew[set] = (tot[set][0] / N) / (sd * sd * sd);
            kurt[set] = (tot[set][1] / N) / (var[set] * var[set]) - 3.0;
        }
        double acd = 0.0;
        for (int j = 0; j < K; ++j) {
            double acf[2];
            for (int set = 0; set < 2; ++set) {
                acf[set] = (tot[set][2 + j] / ((double)n * (double)(L - j))) / var[set];
                if (stats != nullptr) stats[((size_t)set * S + c) * (4 + K) + 4 + j] = (float)acf[set];
            }
            acd += (acf[1] - acf[0]) * (acf[1] - acf[0]);
        }
        if (stats != nullptr)
            for (int set = 0; set < 2; ++set) {
                float* o = stats + ((size_t)set * S + c) * (4 + K);
                o[0] = (float)mean[set]; o[1] = (float)var[set]; o[2] = (float)skew[set]; o[3] = (float)kurt[set];
            }
        chan[c] = (float)sqrt(acd);
        chan[S + c] = (float)fabs(skew[1] - skew[0]);
        chan[2 * S + c] = (float)fabs(kurt[1] - kurt[0]);
    }
}

// grid (3): out[b] = mean over channels of chan[b][:]
__global__ __launch_bounds__(256) void feat_chan_mean_kernel(const float* __restrict__ chan, float* __restrict__ out, int S) {
    __shared__ double red[256];
    double s = 0.0;
    for (int c = threadIdx.x; c < S; c += 256) s += (double)chan[(size_t)blockIdx.x * S + c];
    s = feat_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s / (double)S);
}

// floats as unsigned keys of the same order, so that min / max across workgroups are integer atomics
__device__ __forceinline__ unsigned feat_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float feat_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void feat_mdd_init_kernel(unsigned* __restrict__ minmax, unsigned* __restrict__ counts, size_t cols) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cols) { minmax[i] = 0xffffffffu; minmax[cols + i] = 0u; }
    if (i < 2 * FEAT_BINS * cols) counts[i] = 0u;
}

// How a workgroup of the two MDD passes walks its tile: the lanes of a wave run along the contiguous column axis (tc
// columns, 64 in a full tile) and, where the tile is narrower than a wave, along 64 / tc samples as well; the four waves
// take different samples.  blockIdx.y owns the samples [s0, s1).
struct FeatWalk {
    size_t col, s0, s1, first, step;
    int lc;
    bool active;
};
__device__ __forceinline__ FeatWalk feat_walk(size_t cols, int n) {
    FeatWalk f;
    const size_t col0 = (size_t)blockIdx.x * FEAT_TILE;
    const int tc = cols - col0 < (size_t)FEAT_TILE ? (int)(cols - col0) : FEAT_TILE;
    const int spw = 64 / tc, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ls = lane / tc;
    f.lc = lane - ls * tc;
    f.active = ls < spw;
    f.col = col0 + f.lc;
    f.s0 = (size_t)blockIdx.y * n / gridDim.y;
    f.s1 = (size_t)(blockIdx.y + 1) * n / gridDim.y;
    f.first = f.s0 + (size_t)wave * spw + ls;
    f.step = (size_t)4 * spw;
    return f;
}

// grid (ceil(cols / 64), splits of n): min / max of every real column
__global__ __launch_bounds__(256) void feat_mdd_minmax_kernel(const float* __restrict__ ori, unsigned* __restrict__ minmax,
                                                              size_t cols, int n) {
    const FeatWalk f = feat_walk(cols, n);
    if (!f.active || f.first >= f.s1) return;
    float lo = ori[f.first * cols + f.col], hi = lo;
#pragma unroll 4
    for (size_t i = f.first + f.step; i < f.s1; i += f.step) {
        const float v = ori[i * cols + f.col];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    atomicMin(&minmax[f.col], feat_key(lo));
    atomicMax(&minmax[cols + f.col], feat_key(hi));
}

// the bin of x on [a, a + width], or -1 outside (and for a NaN)
__device__ __forceinline__ int feat_bin(float x, float a, float b, double width) {
    if (!(x >= a && x <= b)) return -1;
    const int k = (int)(((double)x - (double)a) / width * (double)FEAT_BINS);
    return k < FEAT_BINS ? k : FEAT_BINS - 1;
}

// b of a column: its max, or a + 1e-5 when the column is constant (histogram_torch, :32)
__device__ __forceinline__ void feat_range(const unsigned* __restrict__ minmax, size_t cols, size_t col, float& a, float& b,
                                           double& width) {
    a = feat_unkey(minmax[col]);
    b = feat_unkey(minmax[cols + col]);
    width = (double)b - (double)a;
    if (b == a) { width = 1e-5; b = (float)((double)a + 1e-5); if (!(b > a)) b = a; }
}

// same grid: counts[set][bin][col] += the tile's histogram of this workgroup's samples, gathered in LDS first
__global__ __launch_bounds__(256) void feat_mdd_count_kernel(const float* __restrict__ ori, const float* __restrict__ gen,
                                                             const unsigned* __restrict__ minmax, unsigned* __restrict__ counts,
                                                             size_t cols, int n) {
    __shared__ unsigned h[2 * FEAT_BINS * FEAT_TILE];            // [set][bin][column of the tile]
    for (int i = threadIdx.x; i < 2 * FEAT_BINS * FEAT_TILE; i += 256) h[i] = 0u;
    __syncthreads();
    const FeatWalk f = feat_walk(cols, n);
    if (f.active) {
        float a, b;
        double width;
        feat_range(minmax, cols, f.col, a, b, width);
#pragma unroll 4
        for (size_t i = f.first; i < f.s1; i += f.step) {
            const int ko = feat_bin(ori[i * cols + f.col], a, b, width);
            const int kg = feat_bin(gen[i * cols + f.col], a, b, width);
            if (ko >= 0) atomicAdd(&h[ko * FEAT_TILE + f.lc], 1u);
            if (kg >= 0) atomicAdd(&h[(FEAT_BINS + kg) * FEAT_TILE + f.lc], 1u);
        }
    }
    __syncthreads();
    const size_t col0 = (size_t)blockIdx.x * FEAT_TILE;
    for (int i = threadIdx.x; i < 2 * FEAT_BINS * FEAT_TILE; i += 256) {
        const int lc = i & (FEAT_TILE - 1), row = i / FEAT_TILE;      // row = set * 50 + bin
        if (h[i] != 0u && col0 + lc < cols) atomicAdd(&counts[(size_t)row * cols + col0 + lc], h[i]);
    }
}

// one thread per column: loss = mean_k |count_gen - count_ori| / (n delta)
__global__ __launch_bounds__(256) void feat_mdd_finish_kernel(const unsigned* __restrict__ minmax, const unsigned* __restrict__ counts,
                                                              float* __restrict__ col_loss, float* __restrict__ per_column,
                                                              size_t cols, int n) {
    const size_t col = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float a, b;
    double width;
    feat_range(minmax, cols, col, a, b, width);
    const double delta = width / (double)FEAT_BINS;
    double s = 0.0;
    for (int k = 0; k < FEAT_BINS; ++k) {
        const double co = (double)counts[(size_t)k * cols + col], cg = (double)counts[(size_t)(FEAT_BINS + k) * cols + col];
        s += fabs(cg / ((double)n * delta) - co / ((double)n * delta));
    }
    const float loss = (float)(s / (double)FEAT_BINS);
    col_loss[col] = loss;
    if (per_column != nullptr) per_column[col] = loss;
}

// ---- TS2Vec encoder forward (evaluate/ts2vec.py:366-399 in eval mode, mask 'all_true'): one workgroup per series, the
// three (channels x T) activation planes live in LDS; weights (< 1 MB) are read through L1 / L2.
struct Ts2vecDev {
    int cin, hidden, cout, depth, T;
    const float *fc_w, *fc_b;
    const float *c1w[T2S_TS2VEC_MAX_BLOCKS], *c1b[T2S_TS2VEC_MAX_BLOCKS], *c2w[T2S_TS2VEC_MAX_BLOCKS], *c2b[T2S_TS2VEC_MAX_BLOCKS];
    const float *pw, *pb;
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// out[co][t] = bias[co] + sum_ci sum_k w[co][ci][k] * gelu(in[ci][t + (k-1) dil]) (zero outside [0,T)) [+ res[co][t]]
__device__ void ts2vec_conv(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* out,
                            const float* res, int ci_n, int co_n, int T, int dil) {
    for (int idx = threadIdx.x; idx < co_n * T; idx += 256) {
        const int co = idx / T, t = idx - co * T;
        const float* wr = w + (size_t)co * ci_n * 3;
        const int tl = t - dil, tr = t + dil;
        float acc = bias[co];
        for (int ci = 0; ci < ci_n; ++ci) {
            const float* row = in + ci * T;
            float v = wr[3 * ci + 1] * row[t];
            if (tl >= 0) v += wr[3 * ci] * row[tl];
            if (tr < T) v += wr[3 * ci + 2] * row[tr];
            acc += v;
        }
        out[idx] = res != nullptr ? acc + res[idx] : acc;
    }
}

__global__ __launch_bounds__(256) void ts2vec_encode_kernel(const Ts2vecDev w, const float* __restrict__ x,
                                                            float* __restrict__ rep, float* __restrict__ full) {
    extern __shared__ float planes[];
    const int T = w.T, cmax = w.hidden > w.cout ? w.hidden : w.cout;
    float* H = planes;                        // current activation (C, T)
    float* G = planes + (size_t)cmax * T;     // gelu(.) / conv1 output
    float* R = planes + (size_t)2 * cmax * T; // projector output of the final block
    const float* xs = x + (size_t)blockIdx.x * T * w.cin;
    // input_fc with the NaN rule: a time step holding a NaN is zeroed before AND after the linear (:367-368,388-389)
    for (int idx = threadIdx.x; idx < w.hidden * T; idx += 256) {
        const int c = idx / T, t = idx - c * T;
        bool ok = true;
        float acc = w.fc_b[c];
        for (int k = 0; k < w.cin; ++k) {
            const float v = xs[t * w.cin + k];
            ok = ok && (v == v);
            acc += w.fc_w[c * w.cin + k] * v;
        }
        H[idx] = ok ? acc : 0.f;
    }
    __syncthreads();
    for (int blk = 0; blk <= w.depth; ++blk) {
        const bool last = blk == w.depth;
        const int ci_n = w.hidden, co_n = last ? w.cout : w.hidden;
        const int dil = blk < 30 ? (1 << blk) : (1 << 30);
        for (int idx = threadIdx.x; idx < ci_n * T; idx += 256) G[idx] = gelu_erf(H[idx]);
        if (last) {   // 1x1 projector of the raw (not activated) input
            for (int idx = threadIdx.x; idx < co_n * T; idx += 256) {
                const int co = idx / T, t = idx - co * T;
                float acc = w.pb[co];
                for (int ci = 0; ci < ci_n; ++ci) acc += w.pw[co * ci_n + ci] * H[ci * T + t];
                R[idx] = acc;
            }
        }
        __syncthreads();
        // conv1(gelu(h)) -> overwrite H is not possible in place for co != ci; H is dead once R / the residual is taken:
        // non-final blocks add the residual H element-wise at the very end, so conv1 goes to R's plane as scratch
        float* Y1 = last ? H : R;             // final block: H is dead after the projector; others: R is free
        ts2vec_conv(w.c1w[blk], w.c1b[blk], G, Y1, nullptr, ci_n, co_n, T, dil);
        __syncthreads();
        for (int idx = threadIdx.x; idx < co_n * T; idx += 256) G[idx] = gelu_erf(Y1[idx]);
        __syncthreads();
        if (last) {
            ts2vec_conv(w.c2w[blk], w.c2b[blk], G, H, R, co_n, co_n, T, dil);       // H = conv2 + projector
        } else {
            ts2vec_conv(w.c2w[blk], w.c2b[blk], G, R, H, co_n, co_n, T, dil);       // R = conv2 + H (element-wise residual)
            __syncthreads();
            for (int idx = threadIdx.x; idx < co_n * T; idx += 256) H[idx] = R[idx];
        }
        __syncthreads();
    }
    // outputs: rep (B, T, cout) time-major like the reference's transpose; full = max over time
    if (rep != nullptr)
        for (int idx = threadIdx.x; idx < w.cout * T; idx += 256) {
            const int t = idx / w.cout, c = idx - t * w.cout;
            rep[((size_t)blockIdx.x * T + t) * w.cout + c] = H[c * T + t];
        }
    for (int c = threadIdx.x; c < w.cout; c += 256) {
        float m = H[c * T];
        for (int t = 1; t < T; ++t) m = fmaxf(m, H[c * T + t]);
        full[(size_t)blockIdx.x * w.cout + c] = m;
    }
}

}  // namespace
}  // namespace t2s

extern "C" int t2s_eval_mrr(const float* ori, const float* gen, float* sims, float* score, float* out, int n, int len,
                            int runs, float threshold, void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && sims && score && out && n > 0 && len > 0 && runs > 0, "t2s_eval_mrr: bad argument");
    hipStream_t st = (hipStream_t)stream;
    eval_mrr_kernel<<<n, 64, 0, st>>>(ori, gen, sims, score, n, len, runs, threshold);
    T2S_LAUNCH_CHECK();
    eval_mean_kernel<<<1, 256, 0, st>>>(score, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_mse_wape(const float* ori, const float* gen, float* per_sample, float* out, int n, int len,
                                 void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && per_sample && out && n > 0 && len > 0, "t2s_eval_mse_wape: bad argument");
    hipStream_t st = (hipStream_t)stream;
    eval_per_sample_kernel<<<n, 64, 0, st>>>(ori, gen, per_sample, len);
    T2S_LAUNCH_CHECK();
    eval_reduce_kernel<<<1, 256, 0, st>>>(per_sample, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}


extern "C" int t2s_eval_ed(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                           void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && per_sample && out && n > 0 && L > 0 && n_series > 0, "t2s_eval_ed: bad argument");
    hipStream_t st = (hipStream_t)stream;
    eval_ed_kernel<<<n, 64, 0, st>>>(ori, gen, per_sample, L, n_series);
    T2S_LAUNCH_CHECK();
    eval_mean_kernel<<<1, 256, 0, st>>>(per_sample, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_crps(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                             int runs, void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && per_sample && out && n > 0 && L > 0 && n_series > 0 && runs > 0, "t2s_eval_crps: bad argument");
    hipStream_t st = (hipStream_t)stream;
    eval_crps_kernel<<<n, 64, 0, st>>>(ori, gen, per_sample, n, L, n_series, runs);
    T2S_LAUNCH_CHECK();
    eval_mean_kernel<<<1, 256, 0, st>>>(per_sample, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_dtw(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                            void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && per_sample && out && n > 0 && L > 0 && n_series > 0, "t2s_eval_dtw: bad argument");
    T2S_REQUIRE(L <= 4096, "t2s_eval_dtw: L=%d exceeds 4096 (three fp64 diagonals must fit in LDS)", L);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)3 * L * sizeof(double);
    if (lds > 48 * 1024)
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(eval_dtw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    eval_dtw_kernel<<<n, 256, lds, st>>>(ori, gen, per_sample, L, n_series);
    T2S_LAUNCH_CHECK();
    eval_mean_kernel<<<1, 256, 0, st>>>(per_sample, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

static int feat_check(const char* who, const void* ori, const void* gen, const void* out, int n, int L, int n_series,
                      const void* workspace, uint64_t workspace_bytes) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && out, "%s: ori, gen and out must not be NULL", who);
    T2S_REQUIRE(n >= 2, "%s: n=%d, the measures need at least 2 samples", who, n);
    T2S_REQUIRE(L >= 1 && L <= 4096, "%s: L=%d is outside [1, 4096]", who, L);
    T2S_REQUIRE(n_series >= 1 && (uint64_t)L * (uint64_t)n_series <= (1u << 24), "%s: n_series=%d (L * n_series must be in [1, 2^24])", who, n_series);
    const uint64_t need = feat_layout(n, L, n_series).total;
    T2S_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %llu bytes, t2s_eval_features_workspace_bytes asks for %llu",
                who, (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
    return T2S_OK;
}

extern "C" uint64_t t2s_eval_features_workspace_bytes(int n, int L, int n_series) {
    using namespace t2s;
    if (n < 2 || L < 1 || L > 4096 || n_series < 1 || (uint64_t)L * (uint64_t)n_series > (1u << 24)) {
        set_error("t2s_eval_features_workspace_bytes: unsupported n=%d, L=%d, n_series=%d (n >= 2, 1 <= L <= 4096, L * n_series <= 2^24)",
                  n, L, n_series);
        return 0;
    }
    return feat_layout(n, L, n_series).total;
}

extern "C" int t2s_eval_moments(const float* ori, const float* gen, float* stats, float* out, int n, int L, int n_series,
                                void* workspace, uint64_t workspace_bytes, void* stream) {
    using namespace t2s;
    if (int rc = feat_check("t2s_eval_moments", ori, gen, out, n, L, n_series, workspace, workspace_bytes)) return rc;
    const FeatLayout w = feat_layout(n, L, n_series);
    char* ws = (char*)workspace;
    double* mean_part = (double*)(ws + w.mean_part);
    double* stat_part = (double*)(ws + w.stat_part);
    float* chan = (float*)(ws + w.chan);
    hipStream_t st = (hipStream_t)stream;
    feat_sum_kernel<<<dim3(w.P, 2), 256, 0, st>>>(ori, gen, mean_part, n, L, n_series);
    T2S_LAUNCH_CHECK();
    feat_stats_kernel<<<dim3(w.P, 2), 256, (size_t)L * sizeof(double), st>>>(ori, gen, mean_part, stat_part, n, L, n_series);
    T2S_LAUNCH_CHECK();
    feat_fold_kernel<<<n_series, 256, 0, st>>>(mean_part, stat_part, stats, chan, n, L, n_series, w.P);
    T2S_LAUNCH_CHECK();
    feat_chan_mean_kernel<<<3, 256, 0, st>>>(chan, out, n_series);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_mdd(const float* ori, const float* gen, float* per_column, float* out, int n, int L, int n_series,
                            void* workspace, uint64_t workspace_bytes, void* stream) {
    using namespace t2s;
    if (int rc = feat_check("t2s_eval_mdd", ori, gen, out, n, L, n_series, workspace, workspace_bytes)) return rc;
    const FeatLayout w = feat_layout(n, L, n_series);
    char* ws = (char*)workspace;
    unsigned* minmax = (unsigned*)(ws + w.minmax);
    unsigned* counts = (unsigned*)(ws + w.counts);
    float* col_loss = (float*)(ws + w.col_loss);
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((w.cols + FEAT_TILE - 1) / FEAT_TILE);
    // at least 64 samples per workgroup, and about a thousand workgroups when n allows: L * n_series may be 24
    unsigned splits = 1024u / tiles > 0 ? 1024u / tiles : 1u;
    if (splits > (unsigned)(n + 63) / 64) splits = (unsigned)(n + 63) / 64;
    feat_mdd_init_kernel<<<(unsigned)((2 * FEAT_BINS * w.cols + 255) / 256), 256, 0, st>>>(minmax, counts, w.cols);
    T2S_LAUNCH_CHECK();
    feat_mdd_minmax_kernel<<<dim3(tiles, splits), 256, 0, st>>>(ori, minmax, w.cols, n);
    T2S_LAUNCH_CHECK();
    feat_mdd_count_kernel<<<dim3(tiles, splits), 256, 0, st>>>(ori, gen, minmax, counts, w.cols, n);
    T2S_LAUNCH_CHECK();
    feat_mdd_finish_kernel<<<(unsigned)((w.cols + 255) / 256), 256, 0, st>>>(minmax, counts, col_loss, per_column, w.cols, n);
    T2S_LAUNCH_CHECK();
    eval_mean_kernel<<<1, 256, 0, st>>>(col_loss, out, (int)w.cols);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_ts2vec_encode(const t2s_ts2vec_weights* w, const float* x, float* rep, float* full, int B, int T,
                                 void* stream) {
    using namespace t2s;
    T2S_REQUIRE(w && x && full && B > 0 && T > 0, "t2s_ts2vec_encode: bad argument");
    T2S_REQUIRE(w->depth >= 0 && w->depth < T2S_TS2VEC_MAX_BLOCKS && w->input_dims > 0 && w->hidden > 0 && w->output_dims > 0,
                "t2s_ts2vec_encode: unsupported sizes (depth=%d, max %d)", w->depth, T2S_TS2VEC_MAX_BLOCKS - 1);
    T2S_REQUIRE(w->fc_w && w->fc_b && w->proj_w && w->proj_b, "t2s_ts2vec_encode: NULL weight");
    Ts2vecDev d{};
    d.cin = w->input_dims; d.hidden = w->hidden; d.cout = w->output_dims; d.depth = w->depth; d.T = T;
    d.fc_w = w->fc_w; d.fc_b = w->fc_b; d.pw = w->proj_w; d.pb = w->proj_b;
    for (int i = 0; i <= w->depth; ++i) {
        T2S_REQUIRE(w->conv1_w[i] && w->conv1_b[i] && w->conv2_w[i] && w->conv2_b[i], "t2s_ts2vec_encode: NULL weight of block %d", i);
        d.c1w[i] = w->conv1_w[i]; d.c1b[i] = w->conv1_b[i]; d.c2w[i] = w->conv2_w[i]; d.c2b[i] = w->conv2_b[i];
    }
    const int cmax = d.hidden > d.cout ? d.hidden : d.cout;
    const size_t lds = (size_t)3 * cmax * T * sizeof(float);
    T2S_REQUIRE(lds <= 160 * 1024, "t2s_ts2vec_encode: 3 x %d channels x T=%d fp32 planes exceed the 160 KB LDS of a CU", cmax, T);
    T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ts2vec_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ts2vec_encode_kernel<<<B, 256, lds, (hipStream_t)stream>>>(d, x, rep, full);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
