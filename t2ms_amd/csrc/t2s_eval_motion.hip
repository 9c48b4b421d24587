// Motion measures of the T2MS evaluation (evaluate/metrics.py of the reference): what its __main__ (:290-370) computes on
// recordings of unequal length, next to the MSE / WAPE of t2s_eval.hip.
//
// Correlational score (calculate_correlation_matrix / calculate_correlational_score, :112-137) of two SETS of rows
// ori (rows_ori, S) and gen (rows_gen, S), the reference's reshape(N * T, D); as np.corrcoef(rowvar=False), all in fp64:
//   mean_c = sum x[:, c] / rows                  c_ij = sum_r (x[r, i] - mean_i) (x[r, j] - mean_j)
//   C_ij   = clip((c_ij / sqrt(c_ii)) / sqrt(c_jj), -1, 1)          (two divisions, as numpy does them; a NaN stays a NaN)
//   score  = 1 - sum |C_ori - C_gen| / sum |C_ori|                  (NaN when that denominator is exactly 0)
// The rows of a set are cut into P = min(rows, 1024) chunks (a function of rows alone); a workgroup sums one chunk in a
// fixed order and the partials are folded in index order, so the grid never changes a bit (feat_sum_kernel /
// feat_fold_kernel of t2s_eval.hip work the same way).  No floating-point atomics anywhere in this file.
//
// Sequence correlation (sequence_correlation, :219-266) of the pairs a_i (m, S), b_i (n', S) held in padded storage
// (n, La, S) / (n, Lb, S): for every shift s in -M .. M, M = min(m, n') - 1,
//   s >= 0: ov = min(m, n' - s), a[0:ov] against b[s:s+ov];     s < 0: ov = min(m + s, n'), a[-s:-s+ov] against b[0:ov]
//   dist_s = mean over the overlap of the Euclidean norm over the S channels   (fp64, rounded once to fp32)
// and the reference's left-to-right search min(keys, key=...) on the stored fp32 values.
//
// DTW of two sequences of unequal length (calculate_dtw(seq1, seq2), :139-170, default cost): the recurrence of
// eval_dtw_kernel (t2s_eval.hip) on an m x n' table -- the same fp64 operations per cell in the same order, so with
// m = n' = L the two kernels give the same bits.
#include "t2s_common.h"

namespace t2s {
namespace {

constexpr int MOTION_MAX_LEN = T2S_EVAL_MOTION_MAX_LEN;        // 4096
constexpr int CORR_MAX_SERIES = T2S_EVAL_CORR_MAX_SERIES;      // 64
constexpr int CORR_MAX_CHUNKS = 1024;
constexpr int SHIFT_BLOCK = 64;                                // consecutive shifts per workgroup

// a copy of eval_mean_kernel (t2s_eval.hip): out[0] = mean of v[0..n), fp64, one fixed tree
__global__ __launch_bounds__(256) void motion_mean_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
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

// a length from the caller's array (NULL: the full padded length), clamped into [1, cap]: nothing a caller stores there
// can take a read outside the arrays
__device__ __forceinline__ int motion_len(const int* __restrict__ len, int i, int cap) {
    int v = len != nullptr ? len[i] : cap;
    v = v < 1 ? 1 : v;
    return v > cap ? cap : v;
}

// ---- sequence correlation.  grid (n * ceil(W / 64)), pair-major: the four waves of a workgroup take the 64 columns of
// the block round robin; the 64 lanes of a wave stride the overlap and add their point norms in fp64 in that order; one xor
// shuffle tree, one division by ov, one rounding.  The order depends on (m, n', s) alone.
__global__ __launch_bounds__(256) void motion_shift_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const int* __restrict__ len_a, const int* __restrict__ len_b,
                                                           float* __restrict__ table, int La, int Lb, int S, int W,
                                                           int blocks) {
    const int pair = blockIdx.x / blocks, blk = blockIdx.x - pair * blocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = motion_len(len_a, pair, La), n = motion_len(len_b, pair, Lb);
    const int M = (m < n ? m : n) - 1, zero = (W - 1) / 2;                 // zero: the column of shift 0
    const float* pa = a + (size_t)pair * La * S;
    const float* pb = b + (size_t)pair * Lb * S;
    for (int k = wave; k < SHIFT_BLOCK; k += 4) {
        const int col = blk * SHIFT_BLOCK + k;
        if (col >= W) break;
        const int s = col - zero;
        float r = __builtin_nanf("");
        if (s >= -M && s <= M) {
            int ov, ia, ib;
            if (s >= 0) { ov = m < n - s ? m : n - s; ia = 0; ib = s; }
            else        { ov = m + s < n ? m + s : n; ia = -s; ib = 0; }
            const float* xa = pa + (size_t)ia * S;
            const float* xb = pb + (size_t)ib * S;
            double sum = 0.0;
            for (int t = lane; t < ov; t += 64) {
                double q = 0.0;
                for (int c = 0; c < S; ++c) {
                    const double d = (double)xa[(size_t)t * S + c] - (double)xb[(size_t)t * S + c];
                    q += d * d;
                }
                sum += sqrt(q);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
            r = (float)(sum / (double)ov);
        }
        if (lane == 0) table[(size_t)pair * W + col] = r;
    }
}

// the reference's search: min(distances.keys(), key=...) walks the shifts from -M upwards and a later one replaces the
// current one only if its value is strictly smaller.  So a NaN is never chosen unless it is the first value, which then
// stays (no comparison with a NaN is true); otherwise the smallest value wins, the most negative shift among equals.
// One wave per pair: lanes scan strided columns by that rule, then the (value, column) pairs are merged.
__global__ __launch_bounds__(64) void motion_scan_kernel(const float* __restrict__ table, const int* __restrict__ len_a,
                                                         const int* __restrict__ len_b, int* __restrict__ best_shift,
                                                         float* __restrict__ min_dist, int La, int Lb, int W) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int m = motion_len(len_a, pair, La), n = motion_len(len_b, pair, Lb);
    const int M = (m < n ? m : n) - 1, zero = (W - 1) / 2, first = zero - M, count = 2 * M + 1;
    const float* row = table + (size_t)pair * W;
    float bv = __builtin_inff();
    int bc = 0x7fffffff;                                        // no candidate yet
    for (int k = lane; k < count; k += 64) {
        const float v = row[first + k];
        if (v == v && (bc == 0x7fffffff || v < bv)) { bv = v; bc = first + k; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (oc != 0x7fffffff && (bc == 0x7fffffff || ov < bv || (ov == bv && oc < bc))) { bv = ov; bc = oc; }
    }
    if (lane == 0) {
        const float head = row[first];
        if (head != head || bc == 0x7fffffff) bc = first;       // a NaN at the first shift stays
        best_shift[pair] = bc - zero;
        min_dist[pair] = row[bc];
    }
}

// ---- ragged DTW: eval_dtw_kernel of t2s_eval.hip on an m x n table.  Three diagonals of La doubles, indexed by row.
__global__ __launch_bounds__(256) void motion_dtw_kernel(const float* __restrict__ sa, const float* __restrict__ sb,
                                                         const int* __restrict__ len_a, const int* __restrict__ len_b,
                                                         float* __restrict__ per_sample, int La, int Lb, int S) {
    extern __shared__ double diag[];          // [3][La]
    const int smp = blockIdx.x;
    const int m = motion_len(len_a, smp, La), n = motion_len(len_b, smp, Lb);
    const float* a = sa + (size_t)smp * La * S;
    const float* b = sb + (size_t)smp * Lb * S;
    const double INF = 1e300;
    for (int d = 0; d <= m + n - 2; ++d) {
        double* cur = diag + (d % 3) * La;
        const double* p1 = diag + ((d + 2) % 3) * La;   // diagonal d-1, indexed by row i
        const double* p2 = diag + ((d + 1) % 3) * La;   // diagonal d-2
        const int lo = d - (n - 1) > 0 ? d - (n - 1) : 0, hi = d < m - 1 ? d : m - 1;
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
                if (up != up || left != left || dg != dg) best = __builtin_nan("");   // fmin drops a NaN: keep it
            }
            cur[i] = c + best;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) per_sample[smp] = (float)sqrt(diag[((m + n - 2) % 3) * La + (m - 1)]);
}

// ---- correlational score
struct CorrLayout {          // byte offsets into the caller's workspace; a function of (rows_ori, rows_gen, S) alone
    int P[2], Pmax;
    size_t sum_part, co_part, c64, total;
};

inline CorrLayout corr_layout(int rows_ori, int rows_gen, int S) {
    CorrLayout w{};
    w.P[0] = rows_ori < CORR_MAX_CHUNKS ? rows_ori : CORR_MAX_CHUNKS;
    w.P[1] = rows_gen < CORR_MAX_CHUNKS ? rows_gen : CORR_MAX_CHUNKS;
    w.Pmax = w.P[0] > w.P[1] ? w.P[0] : w.P[1];
    size_t o = 0;
    w.sum_part = o; o += (size_t)2 * w.Pmax * S * sizeof(double);
    w.co_part = o;  o += (size_t)2 * w.Pmax * S * S * sizeof(double);
    w.c64 = o;      o += (size_t)2 * S * S * sizeof(double);
    w.total = (o + 255) / 256 * 256;
    return w;
}

struct CorrSets {
    const float* x[2];
    int rows[2], P[2];
};

__device__ __forceinline__ double corr_block_sum(double v, double* red) {
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

// grid (Pmax, 2): chunk p of set blockIdx.y -> sum_part[set][p][c] = the sum of the chunk's values of channel c
__global__ __launch_bounds__(256) void corr_sum_kernel(const CorrSets z, double* __restrict__ sum_part, int S, int Pmax) {
    __shared__ double red[256];
    const int set = blockIdx.y, p = blockIdx.x, P = z.P[set];
    if (p >= P) return;
    const size_t r0 = (size_t)p * z.rows[set] / P, r1 = (size_t)(p + 1) * z.rows[set] / P;
    const float* x = z.x[set] + r0 * S;
    for (int c = 0; c < S; ++c) {
        double s = 0.0;
        for (size_t r = threadIdx.x; r < r1 - r0; r += 256) s += (double)x[r * S + c];
        s = corr_block_sum(s, red);
        if (threadIdx.x == 0) sum_part[((size_t)set * Pmax + p) * S + c] = s;
    }
}

// grid (Pmax, 2): the channel means (the P chunk sums added in index order, by every workgroup alike), then thread (i, j)
// adds (x[r, i] - mean_i) (x[r, j] - mean_j) over the chunk's rows in row order -> co_part[set][p][i][j]
__global__ __launch_bounds__(256) void corr_comoment_kernel(const CorrSets z, const double* __restrict__ sum_part,
                                                            double* __restrict__ co_part, int S, int Pmax) {
    __shared__ double mean[CORR_MAX_SERIES];
    const int set = blockIdx.y, p = blockIdx.x, P = z.P[set];
    if (p >= P) return;
    if ((int)threadIdx.x < S) {
        double s = 0.0;
        for (int q = 0; q < P; ++q) s += sum_part[((size_t)set * Pmax + q) * S + threadIdx.x];
        mean[threadIdx.x] = s / (double)z.rows[set];
    }
    __syncthreads();
    const size_t r0 = (size_t)p * z.rows[set] / P, r1 = (size_t)(p + 1) * z.rows[set] / P;
    const float* x = z.x[set];
    double* dst = co_part + ((size_t)set * Pmax + p) * S * S;
    for (int e = threadIdx.x; e < S * S; e += 256) {
        const int i = e / S, j = e - i * S;
        const double mi = mean[i], mj = mean[j];
        double s = 0.0;
        for (size_t r = r0; r < r1; ++r) s += ((double)x[r * S + i] - mi) * ((double)x[r * S + j] - mj);
        dst[e] = s;
    }
}

// grid (S, 2): row i of set blockIdx.y.  Thread j folds c_ij, c_jj and c_ii over the P partials in index order, then
// C_ij = clip((c_ij / sqrt(c_ii)) / sqrt(c_jj)) -> c64 (fp64, for the score) and corr (fp32, may be NULL)
__global__ __launch_bounds__(64) void corr_fold_kernel(const CorrSets z, const double* __restrict__ co_part,
                                                       double* __restrict__ c64, float* __restrict__ corr, int S, int Pmax) {
    const int set = blockIdx.y, i = blockIdx.x, j = threadIdx.x, P = z.P[set];
    if (j >= S) return;
    const double* src = co_part + (size_t)set * Pmax * S * S;
    double cij = 0.0, cii = 0.0, cjj = 0.0;
    for (int p = 0; p < P; ++p) {
        const double* q = src + (size_t)p * S * S;
        cij += q[i * S + j];
        cii += q[i * S + i];
        cjj += q[j * S + j];
    }
    double r = cij / sqrt(cii);
    r = r / sqrt(cjj);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                  // np.clip: a NaN passes through
    const size_t e = ((size_t)set * S + i) * S + j;
    c64[e] = r;
    if (corr != nullptr) corr[e] = (float)r;
}

__global__ __launch_bounds__(256) void corr_score_kernel(const double* __restrict__ c64, float* __restrict__ out, int S) {
    __shared__ double red[256];
    double num = 0.0, den = 0.0;
    for (int e = threadIdx.x; e < S * S; e += 256) {
        num += fabs(c64[e] - c64[S * S + e]);
        den += fabs(c64[e]);
    }
    num = corr_block_sum(num, red);
    den = corr_block_sum(den, red);
    if (threadIdx.x == 0) out[0] = den == 0.0 ? __builtin_nanf("") : (float)(1.0 - num / den);
}

int corr_shape_ok(const char* who, int rows_ori, int rows_gen, int S) {
    T2S_REQUIRE(rows_ori >= 2, "%s: rows_ori=%d, a correlation needs at least 2 rows", who, rows_ori);
    T2S_REQUIRE(rows_gen >= 2, "%s: rows_gen=%d, a correlation needs at least 2 rows", who, rows_gen);
    T2S_REQUIRE(S >= 1 && S <= CORR_MAX_SERIES, "%s: n_series=%d is outside [1, %d]", who, S, CORR_MAX_SERIES);
    return T2S_OK;
}

int ragged_check(const char* who, const void* a, const void* b, int n, int La, int Lb, int S) {
    T2S_REQUIRE(a && b, "%s: a and b must not be NULL", who);
    T2S_REQUIRE(n >= 1, "%s: n=%d pairs", who, n);
    T2S_REQUIRE(La >= 1 && La <= MOTION_MAX_LEN, "%s: La=%d is outside [1, %d]", who, La, MOTION_MAX_LEN);
    T2S_REQUIRE(Lb >= 1 && Lb <= MOTION_MAX_LEN, "%s: Lb=%d is outside [1, %d]", who, Lb, MOTION_MAX_LEN);
    T2S_REQUIRE(S >= 1 && S <= (1 << 16), "%s: n_series=%d is outside [1, 65536]", who, S);
    return T2S_OK;
}

}  // namespace
}  // namespace t2s

extern "C" uint64_t t2s_eval_corr_workspace_bytes(int rows_ori, int rows_gen, int n_series) {
    using namespace t2s;
    if (corr_shape_ok("t2s_eval_corr_workspace_bytes", rows_ori, rows_gen, n_series) != T2S_OK) return 0;
    return corr_layout(rows_ori, rows_gen, n_series).total;
}

extern "C" int t2s_eval_corr(const float* ori, const float* gen, float* corr, float* out, int rows_ori, int rows_gen,
                             int n_series, void* workspace, uint64_t workspace_bytes, void* stream) {
    using namespace t2s;
    T2S_REQUIRE(ori && gen && out, "t2s_eval_corr: ori, gen and out must not be NULL");
    if (int rc = corr_shape_ok("t2s_eval_corr", rows_ori, rows_gen, n_series)) return rc;
    const CorrLayout w = corr_layout(rows_ori, rows_gen, n_series);
    T2S_REQUIRE(workspace && workspace_bytes >= w.total, "t2s_eval_corr: workspace of %llu bytes, t2s_eval_corr_workspace_bytes asks for %llu",
                (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)w.total);
    char* ws = (char*)workspace;
    double* sum_part = (double*)(ws + w.sum_part);
    double* co_part = (double*)(ws + w.co_part);
    double* c64 = (double*)(ws + w.c64);
    CorrSets z{};
    z.x[0] = ori; z.x[1] = gen;
    z.rows[0] = rows_ori; z.rows[1] = rows_gen;
    z.P[0] = w.P[0]; z.P[1] = w.P[1];
    hipStream_t st = (hipStream_t)stream;
    corr_sum_kernel<<<dim3(w.Pmax, 2), 256, 0, st>>>(z, sum_part, n_series, w.Pmax);
    T2S_LAUNCH_CHECK();
    corr_comoment_kernel<<<dim3(w.Pmax, 2), 256, 0, st>>>(z, sum_part, co_part, n_series, w.Pmax);
    T2S_LAUNCH_CHECK();
    corr_fold_kernel<<<dim3(n_series, 2), 64, 0, st>>>(z, co_part, c64, corr, n_series, w.Pmax);
    T2S_LAUNCH_CHECK();
    corr_score_kernel<<<1, 256, 0, st>>>(c64, out, n_series);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_shift(const float* a, const float* b, const int* len_a, const int* len_b, float* table,
                              int* best_shift, float* min_dist, float* out, int n, int La, int Lb, int n_series,
                              void* stream) {
    using namespace t2s;
    if (int rc = ragged_check("t2s_eval_shift", a, b, n, La, Lb, n_series)) return rc;
    T2S_REQUIRE(table && best_shift && min_dist && out, "t2s_eval_shift: table, best_shift, min_dist and out must not be NULL");
    const int W = 2 * (La < Lb ? La : Lb) - 1, blocks = (W + SHIFT_BLOCK - 1) / SHIFT_BLOCK;
    T2S_REQUIRE((uint64_t)n * (uint64_t)blocks <= 0x7fffffffull, "t2s_eval_shift: n=%d pairs of %d shifts exceed one launch", n, W);
    hipStream_t st = (hipStream_t)stream;
    motion_shift_kernel<<<(unsigned)n * (unsigned)blocks, 256, 0, st>>>(a, b, len_a, len_b, table, La, Lb, n_series, W, blocks);
    T2S_LAUNCH_CHECK();
    motion_scan_kernel<<<n, 64, 0, st>>>(table, len_a, len_b, best_shift, min_dist, La, Lb, W);
    T2S_LAUNCH_CHECK();
    motion_mean_kernel<<<1, 256, 0, st>>>(min_dist, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_eval_dtw_ragged(const float* a, const float* b, const int* len_a, const int* len_b, float* per_sample,
                                   float* out, int n, int La, int Lb, int n_series, void* stream) {
    using namespace t2s;
    if (int rc = ragged_check("t2s_eval_dtw_ragged", a, b, n, La, Lb, n_series)) return rc;
    T2S_REQUIRE(per_sample && out, "t2s_eval_dtw_ragged: per_sample and out must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)3 * La * sizeof(double);
    if (lds > 48 * 1024)
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(motion_dtw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    motion_dtw_kernel<<<n, 256, lds, st>>>(a, b, len_a, len_b, per_sample, La, Lb, n_series);
    T2S_LAUNCH_CHECK();
    motion_mean_kernel<<<1, 256, 0, st>>>(per_sample, out, n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
