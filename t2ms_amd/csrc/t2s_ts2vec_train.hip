// One training step of TS2Vec.fit (evaluate/ts2vec.py:113-140) and the AveragedModel update: include/t2s.h
// "t2s_ts2vec_train_step".  Four launches, no host round trip:
//   1. ts2vec_train_fwd_kernel   one workgroup per (view, series): the training forward with the three activation planes in
//                                LDS as ts2vec_encode_kernel keeps them; saves what the backward reads (block input, conv1
//                                output, and their GELUs) and the max-pool pyramid of the cropped, dropped-out output;
//   2. ts2vec_loss_kernel        one workgroup per (level, series) for the temporal term and per (level, time step) for the
//                                instance term: similarity matrix, row log-sum-exp, the loss part and d loss / d z;
//   3. ts2vec_train_bwd_kernel   one workgroup per (view, series): un-pools the pyramid's gradients, then the data gradients
//                                down the stack; saves d conv-output per convolution;
//   4. ts2vec_wgrad_kernel       one workgroup per (convolution, 8 output x 128 input channels): the weight gradient summed
//                                over (view, series, time) in that order by the thread that owns the weight.
// Nothing is accumulated with atomics, so a step is bit-reproducible.
#include "t2s_common.h"

namespace t2s {
namespace {

constexpr int MAXLEV = 9;       // crop_l <= 128 -> 128, 64, ..., 1: 8 levels
constexpr int PARTS = 128;      // loss parts per (level, kind): max(T, B)
constexpr int FB_THREADS = 512; // forward / backward / loss workgroup
constexpr int WG_CO = 8, WG_CI = 128;

struct TrainDev {
    int cin, hidden, cout, depth, cm;
    int B, T, crop_l, len[2];
    float keep_scale;
    const float *fc_w, *fc_b, *pw, *pb;
    const float *c1w[T2S_TS2VEC_MAX_BLOCKS], *c1b[T2S_TS2VEC_MAX_BLOCKS], *c2w[T2S_TS2VEC_MAX_BLOCKS], *c2b[T2S_TS2VEC_MAX_BLOCKS];
    const float* x;
    const int32_t* start[2];
    const uint8_t* mask[2];
    const uint8_t* keep[2];
    // workspace
    float *act, *dact, *zpyr, *dzI, *dzT, *simT, *simI, *losspart, *loss_out;
    // loss pyramid
    int nlev, L[MAXLEV], off[MAXLEV], instOn[MAXLEV], tempOn[MAXLEV];
    unsigned long long soffT[MAXLEV];
    float coefI[MAXLEV], coefT[MAXLEV];
};

struct GradDev {
    float *fc_w, *fc_b, *pw, *pb;
    float *c1w[T2S_TS2VEC_MAX_BLOCKS], *c1b[T2S_TS2VEC_MAX_BLOCKS], *c2w[T2S_TS2VEC_MAX_BLOCKS], *c2b[T2S_TS2VEC_MAX_BLOCKS];
};

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float dgelu_f(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}
__device__ __forceinline__ int clamp_start(int st, int T, int Tv) { return st < 0 ? 0 : (st > T - Tv ? T - Tv : st); }

// act: per (view-series s, block) four (cm x T)-strided planes: 0 block input H, 1 gelu(H), 2 conv1 output Y1, 3 gelu(Y1)
__device__ __forceinline__ float* act_plane(const TrainDev& d, int s, int blk, int which) {
    return d.act + ((size_t)(s * (d.depth + 1) + blk) * 4 + which) * d.cm * d.T;
}
// dact: per s: [2 blk] d conv1 output, [2 blk + 1] d block output, [2 (depth+1)] d block-0 input (masked)
__device__ __forceinline__ float* dact_plane(const TrainDev& d, int s, int idx) {
    return d.dact + ((size_t)s * (2 * (d.depth + 1) + 1) + idx) * d.cm * d.T;
}

// out[o][t] = bias[o] + sum_i sum_k W(o,i,k) in[i][t + (k-1) dil] + res[o][t], zero outside [0,T).
// Forward (TR = false): w is (n_out, n_in, 3), W(o,i,k) = w[o][i][k].
// Data gradient (TR = true): w is (n_in, n_out, 3), W(o,i,k) = w[i][o][2-k]: `in` is d conv-output, `out` d conv-input.
// A thread owns one output channel at four time steps TS apart; with dil >= T only the centre tap is evaluated.
template <bool TR>
__device__ void conv3(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* out, const float* res,
                      int n_in, int n_out, int T, int dil) {
    const int TS = (T + 3) >> 2;
    const bool outer = dil < T;
    for (int item = threadIdx.x; item < n_out * TS; item += FB_THREADS) {
        const int o = item / TS, tt = item - o * TS;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int tc[4], tl[4], tr[4];
        bool vl[4], vr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tt + j * TS;
            tc[j] = t < T ? t : T - 1;
            vl[j] = t < T && t - dil >= 0;
            vr[j] = t + dil < T;
            tl[j] = vl[j] ? t - dil : 0;
            tr[j] = vr[j] ? t + dil : 0;
        }
        const float* wp = TR ? w + (size_t)o * 3 : w + (size_t)o * n_in * 3;
        const int ws = TR ? n_out * 3 : 3;
        if (outer) {
#pragma unroll 2
            for (int i = 0; i < n_in; ++i) {
                const float w0 = wp[(size_t)i * ws + (TR ? 2 : 0)], w1 = wp[(size_t)i * ws + 1], w2 = wp[(size_t)i * ws + (TR ? 0 : 2)];
                const float* row = in + i * T;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float c = row[tc[j]];
                    const float l = vl[j] ? row[tl[j]] : 0.f;
                    const float r = vr[j] ? row[tr[j]] : 0.f;
                    acc[j] += w1 * c + w0 * l + w2 * r;
                }
            }
        } else {
#pragma unroll 4
            for (int i = 0; i < n_in; ++i) {
                const float w1 = wp[(size_t)i * ws + 1];
                const float* row = in + i * T;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += w1 * row[tc[j]];
            }
        }
        const float bv = bias != nullptr ? bias[o] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tt + j * TS;
            if (t < T) out[o * T + t] = acc[j] + bv + (res != nullptr ? res[o * T + t] : 0.f);
        }
    }
}

__global__ __launch_bounds__(FB_THREADS) void ts2vec_train_fwd_kernel(const TrainDev d) {
    extern __shared__ float planes[];
    const int s = blockIdx.x, v = s / d.B, b = s - v * d.B;
    const int T = d.len[v], C = d.cout;
    const size_t psz = (size_t)d.cm * d.T;
    float* H = planes;
    float* G = planes + psz;
    float* R = planes + 2 * psz;
    const int st = clamp_start(d.start[v][b], d.T, T);
    const float* xs = d.x + ((size_t)b * d.T + st) * d.cin;
    const uint8_t* mk = d.mask[v] + (size_t)b * T;
    for (int idx = threadIdx.x; idx < d.hidden * T; idx += FB_THREADS) {
        const int c = idx / T, t = idx - c * T;
        float acc = d.fc_b[c];
        for (int k = 0; k < d.cin; ++k) acc += d.fc_w[c * d.cin + k] * xs[t * d.cin + k];
        H[idx] = mk[t] ? acc : 0.f;
    }
    __syncthreads();
    for (int blk = 0; blk <= d.depth; ++blk) {
        const bool last = blk == d.depth;
        const int ci_n = d.hidden, co_n = last ? d.cout : d.hidden;
        const int dil = blk < 30 ? (1 << blk) : (1 << 30);
        float *aH = act_plane(d, s, blk, 0), *aG1 = act_plane(d, s, blk, 1), *aY1 = act_plane(d, s, blk, 2), *aG2 = act_plane(d, s, blk, 3);
        for (int idx = threadIdx.x; idx < ci_n * T; idx += FB_THREADS) {
            const float h = H[idx], g = gelu_f(h);
            G[idx] = g;
            aH[idx] = h;
            aG1[idx] = g;
        }
        if (last) {   // 1x1 projector of the raw input
            for (int idx = threadIdx.x; idx < co_n * T; idx += FB_THREADS) {
                const int co = idx / T, t = idx - co * T;
                float acc = d.pb[co];
                for (int ci = 0; ci < ci_n; ++ci) acc += d.pw[co * ci_n + ci] * H[ci * T + t];
                R[idx] = acc;
            }
        }
        __syncthreads();
        float* Y1 = last ? H : R;
        conv3<false>(d.c1w[blk], d.c1b[blk], G, Y1, nullptr, ci_n, co_n, T, dil);
        __syncthreads();
        for (int idx = threadIdx.x; idx < co_n * T; idx += FB_THREADS) {
            const float y = Y1[idx], g = gelu_f(y);
            G[idx] = g;
            aY1[idx] = y;
            aG2[idx] = g;
        }
        __syncthreads();
        if (last) {
            conv3<false>(d.c2w[blk], d.c2b[blk], G, H, R, co_n, co_n, T, dil);      // H = conv2 + projector
        } else {
            conv3<false>(d.c2w[blk], d.c2b[blk], G, R, H, co_n, co_n, T, dil);      // R = conv2 + H
            float* tmp = H; H = R; R = tmp;
        }
        __syncthreads();
    }
    // the cropped, dropped-out output and its max-pool pyramid: zpyr[s][off_l + i][c]; H is plane 0 or 2, so two
    // contiguous planes are free for the pyramid (2 crop_l C <= 2 cm T floats)
    float* ZP = (H == planes) ? planes + psz : planes;
    const int PT = 2 * d.T;
    float* zg = d.zpyr + (size_t)s * PT * C;
    const uint8_t* kp = d.keep[v] + (size_t)b * C * T;
    const int t0 = v == 0 ? T - d.crop_l : 0;
    for (int idx = threadIdx.x; idx < d.crop_l * C; idx += FB_THREADS) {
        const int i = idx / C, c = idx - i * C;
        const int t = t0 + i;
        const float z = kp[c * T + t] ? H[c * T + t] * d.keep_scale : 0.f;
        ZP[idx] = z;
        zg[idx] = z;
    }
    __syncthreads();
    for (int l = 1; l < d.nlev; ++l) {
        const float* src = ZP + (size_t)d.off[l - 1] * C;
        float* dst = ZP + (size_t)d.off[l] * C;
        for (int idx = threadIdx.x; idx < d.L[l] * C; idx += FB_THREADS) {
            const int i = idx / C, c = idx - i * C;
            const float a = src[(2 * i) * C + c], bq = src[(2 * i + 1) * C + c];
            const float m = a >= bq ? a : bq;
            dst[idx] = m;
            zg[(size_t)d.off[l] * C + idx] = m;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float wave_sum(float v) {   // butterfly: the same fixed tree in every run, all lanes get the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The pair loss of ts2vec.py:463-497 for M = 2n rows (positives r <-> r +- n): -log-softmax of every row over all OTHER
// rows at its positive.  kind 0: instance (rows = the 2B series at one time step); kind 1: temporal (rows = the 2n time
// steps of one series).  Writes the task's share of the loss and d loss / d z of its rows.
__global__ __launch_bounds__(FB_THREADS) void ts2vec_loss_kernel(const TrainDev d) {
    extern __shared__ float lds[];
    const int kind = blockIdx.z, l = blockIdx.y, task = blockIdx.x;
    const int n = d.L[l], C = d.cout, CP = C + 1, PT = 2 * d.T, B = d.B;
    int M, half;
    float* S;
    float coef;
    float* dz;
    if (kind == 0) {
        if (!d.instOn[l] || task >= n) return;
        M = 2 * B; half = B;
        S = d.simI + (size_t)(d.off[l] + task) * (4 * B * B);
        coef = d.coefI[l];
        dz = d.dzI;
    } else {
        if (!d.tempOn[l] || task >= B) return;
        M = 2 * n; half = n;
        S = d.simT + d.soffT[l] + (size_t)task * (4 * n * n);
        coef = d.coefT[l];
        dz = d.dzT;
    }
    float* Z = lds;                       // M x CP
    float* lse = lds + (size_t)M * CP;    // M
    float* rl = lse + M;                  // M
    auto goff = [&](int r) -> size_t {
        const int view = r >= half ? 1 : 0, q = r - view * half;
        return kind == 0 ? ((size_t)(view * B + q) * PT + d.off[l] + task) * C
                         : ((size_t)(view * B + task) * PT + d.off[l] + q) * C;
    };
    for (int e = threadIdx.x; e < M * C; e += FB_THREADS) {
        const int r = e / C, c = e - r * C;
        Z[r * CP + c] = d.zpyr[goff(r) + c];
    }
    __syncthreads();
    // similarities: four rows x one column per item
    const int RT = (M + 3) >> 2;
    for (int item = threadIdx.x; item < RT * M; item += FB_THREADS) {
        const int rt = item / M, j = item - rt * M;
        int rr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rr[q] = (rt * 4 + q < M ? rt * 4 + q : M - 1) * CP;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* zj = Z + j * CP;
        for (int c = 0; c < C; ++c) {
            const float zv = zj[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += Z[rr[q] + c] * zv;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (rt * 4 + q < M) S[(size_t)(rt * 4 + q) * M + j] = acc[q];
    }
    __threadfence_block();
    __syncthreads();
    // row log-sum-exp over the other rows, one wave per row
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wid; r < M; r += FB_THREADS / 64) {
        const float* sr = S + (size_t)r * M;
        float m = -INFINITY;
        for (int j = lane; j < M; j += 64)
            if (j != r) m = fmaxf(m, sr[j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < M; j += 64)
            if (j != r) sum += expf(sr[j] - m);
        sum = wave_sum(sum);
        if (lane == 0) {
            const float ls = m + logf(sum);
            lse[r] = ls;
            rl[r] = ls - sr[r >= half ? r - half : r + half];
        }
    }
    __syncthreads();
    if (wid == 0) {
        float part = 0.f;
        for (int r = lane; r < M; r += 64) part += rl[r];
        part = wave_sum(part);
        if (lane == 0) d.losspart[(l * 2 + kind) * PARTS + task] = coef * part;
    }
    // d loss / d sim, symmetrised: g[r][j] = coef (softmax_r[j] + softmax_j[r] - 2 [j positive of r]), 0 on the diagonal
    for (int e = threadIdx.x; e < M * M; e += FB_THREADS) {
        const int r = e / M, j = e - r * M;
        const float sv = S[e];
        const int p = r >= half ? r - half : r + half;
        const float g = r == j ? 0.f : expf(sv - lse[r]) + expf(sv - lse[j]) - (j == p ? 2.f : 0.f);
        S[e] = g * coef;
    }
    __threadfence_block();
    __syncthreads();
    // dz[r][c] = sum_j g[r][j] z[j][c]
    for (int item = threadIdx.x; item < RT * C; item += FB_THREADS) {
        const int rt = item / C, c = item - rt * C;
        const float* g4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) g4[q] = S + (size_t)(rt * 4 + q < M ? rt * 4 + q : M - 1) * M;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < M; ++j) {
            const float zv = Z[j * CP + c];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += g4[q][j] * zv;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (rt * 4 + q < M) dz[goff(rt * 4 + q) + c] = acc[q];
    }
}

__global__ __launch_bounds__(FB_THREADS) void ts2vec_train_bwd_kernel(const TrainDev d) {
    extern __shared__ float planes[];
    const int s = blockIdx.x, v = s / d.B, b = s - v * d.B;
    const int T = d.len[v], C = d.cout, PT = 2 * d.T, nb = d.depth + 1;
    const size_t psz = (size_t)d.cm * d.T;
    float* D = planes;
    float* A = planes + psz;
    float* Bp = planes + 2 * psz;
    // gradient of every pyramid level: its own loss terms, plus the un-pooled gradient of the level above
    float* PG = A;                         // planes 1 and 2: 2 crop_l C <= 2 cm T floats
    const int rows = d.off[d.nlev - 1] + d.L[d.nlev - 1];
    for (int e = threadIdx.x; e < rows * C; e += FB_THREADS) {
        const int row = e / C;
        int l = 0;
        while (l + 1 < d.nlev && row >= d.off[l + 1]) ++l;
        const size_t g = (size_t)s * PT * C + e;
        float val = d.instOn[l] ? d.dzI[g] : 0.f;
        if (d.tempOn[l]) val += d.dzT[g];
        PG[e] = val;
    }
    __syncthreads();
    const float* zg = d.zpyr + (size_t)s * PT * C;
    for (int l = d.nlev - 2; l >= 0; --l) {
        for (int e = threadIdx.x; e < d.L[l + 1] * C; e += FB_THREADS) {
            const int i = e / C, c = e - i * C;
            const float a = zg[(size_t)(d.off[l] + 2 * i) * C + c], bq = zg[(size_t)(d.off[l] + 2 * i + 1) * C + c];
            const int pick = a >= bq ? 2 * i : 2 * i + 1;      // a tie goes to the lower index
            PG[(d.off[l] + pick) * C + c] += PG[(d.off[l + 1] + i) * C + c];
        }
        __syncthreads();
    }
    const uint8_t* kp = d.keep[v] + (size_t)b * C * T;
    const int t0 = v == 0 ? T - d.crop_l : 0;
    for (int idx = threadIdx.x; idx < C * T; idx += FB_THREADS) {
        const int c = idx / T, t = idx - c * T, i = t - t0;
        D[idx] = (i >= 0 && i < d.crop_l && kp[idx]) ? PG[i * C + c] * d.keep_scale : 0.f;
    }
    __syncthreads();
    for (int blk = d.depth; blk >= 0; --blk) {
        const bool last = blk == d.depth;
        const int ci_n = d.hidden, co_n = last ? d.cout : d.hidden;
        const int dil = blk < 30 ? (1 << blk) : (1 << 30);
        const float *aH = act_plane(d, s, blk, 0), *aY1 = act_plane(d, s, blk, 2);
        float *gY1 = dact_plane(d, s, 2 * blk), *gOut = dact_plane(d, s, 2 * blk + 1);
        for (int idx = threadIdx.x; idx < co_n * T; idx += FB_THREADS) gOut[idx] = D[idx];
        conv3<true>(d.c2w[blk], nullptr, D, A, nullptr, co_n, co_n, T, dil);          // d gelu(Y1)
        __syncthreads();
        for (int idx = threadIdx.x; idx < co_n * T; idx += FB_THREADS) {
            const float g = A[idx] * dgelu_f(aY1[idx]);
            A[idx] = g;
            gY1[idx] = g;
        }
        __syncthreads();
        conv3<true>(d.c1w[blk], nullptr, A, Bp, nullptr, co_n, ci_n, T, dil);         // d gelu(H)
        __syncthreads();
        if (last) {
            for (int idx = threadIdx.x; idx < ci_n * T; idx += FB_THREADS) {
                const int ci = idx / T, t = idx - ci * T;
                float acc = 0.f;
                for (int co = 0; co < co_n; ++co) acc += d.pw[co * ci_n + ci] * D[co * T + t];
                Bp[idx] = Bp[idx] * dgelu_f(aH[idx]) + acc;
            }
            float* tmp = D; D = Bp; Bp = tmp;
        } else {
            for (int idx = threadIdx.x; idx < ci_n * T; idx += FB_THREADS) D[idx] = Bp[idx] * dgelu_f(aH[idx]) + D[idx];
        }
        __syncthreads();
    }
    const uint8_t* mk = d.mask[v] + (size_t)b * T;
    float* gIn = dact_plane(d, s, 2 * nb);
    for (int idx = threadIdx.x; idx < d.hidden * T; idx += FB_THREADS) {
        const int t = idx % T;
        gIn[idx] = mk[t] ? D[idx] : 0.f;
    }
    // the loss: parts in (level, kind, task) order, 64 interleaved partial sums and one butterfly
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        float acc = 0.f;
        for (int l = 0; l < d.nlev; ++l) {
            if (d.instOn[l])
                for (int i = threadIdx.x; i < d.L[l]; i += 64) acc += d.losspart[(l * 2) * PARTS + i];
            if (d.tempOn[l])
                for (int i = threadIdx.x; i < d.B; i += 64) acc += d.losspart[(l * 2 + 1) * PARTS + i];
        }
        acc = wave_sum(acc);
        if (threadIdx.x == 0) d.loss_out[0] = acc;
    }
}

// Weight gradients.  blockIdx.y: 2 blk + {0: conv1, 1: conv2}; 2 (depth+1): the projector; 2 (depth+1) + 1: input_fc.
// blockIdx.x: (tile of 8 output channels) x (tile of 128 input channels); for input_fc: the output channel.
__global__ __launch_bounds__(256) void ts2vec_wgrad_kernel(const TrainDev d, const GradDev g) {
    extern __shared__ float lds[];
    const int nb = d.depth + 1, q = blockIdx.y, S = 2 * d.B;
    if (q == 2 * nb + 1) {          // input_fc: dW[c][k] = sum_{s,t} dIn0[s][c][t] x[b][st+t][k], db[c] = sum dIn0
        const int c = blockIdx.x;
        if (c >= d.hidden) return;
        float* red = lds;
        for (int k = 0; k <= d.cin; ++k) {       // k == cin: the bias
            float acc = 0.f;
            for (int e = threadIdx.x; e < S * d.T; e += 256) {
                const int s = e / d.T, t = e - s * d.T, v = s / d.B, b = s - v * d.B;
                if (t >= d.len[v]) continue;
                const float gv = dact_plane(d, s, 2 * nb)[c * d.len[v] + t];
                const int st = clamp_start(d.start[v][b], d.T, d.len[v]);
                acc += k < d.cin ? gv * d.x[((size_t)b * d.T + st + t) * d.cin + k] : gv;
            }
            red[threadIdx.x] = acc;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (k < d.cin) g.fc_w[c * d.cin + k] = red[0];
                else g.fc_b[c] = red[0];
            }
            __syncthreads();
        }
        return;
    }
    const bool proj = q == 2 * nb;
    const int blk = proj ? d.depth : q >> 1, which = proj ? 0 : q & 1;
    const bool last = blk == d.depth;
    const int co_n = last ? d.cout : d.hidden;
    const int ci_n = (which == 1 && !proj) ? co_n : d.hidden;
    const int ncit = (d.cm + WG_CI - 1) / WG_CI;
    const int co0 = (blockIdx.x / ncit) * WG_CO, ci0 = (blockIdx.x % ncit) * WG_CI;
    if (co0 >= co_n || ci0 >= ci_n) return;
    const int dil = blk < 30 ? (1 << blk) : (1 << 30);
    const int Tp = d.T | 1;
    float* Gs = lds;                         // WG_CI x Tp
    float* dYs = lds + (size_t)WG_CI * Tp;   // WG_CO x T
    const int nci = ci_n - ci0 < WG_CI ? ci_n - ci0 : WG_CI;
    float accC[4] = {0.f, 0.f, 0.f, 0.f}, accL[4] = {0.f, 0.f, 0.f, 0.f}, accR[4] = {0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;
    for (int s = 0; s < S; ++s) {
        const int T = d.len[s / d.B];
        const float* gsrc = act_plane(d, s, blk, proj ? 0 : (which == 0 ? 1 : 3)) + (size_t)ci0 * T;
        const float* ysrc = dact_plane(d, s, (proj || which == 1) ? 2 * blk + 1 : 2 * blk);
        __syncthreads();
        for (int e = threadIdx.x; e < nci * T; e += 256) {
            const int ci = e / T, t = e - ci * T;
            Gs[ci * Tp + t] = gsrc[e];
        }
        for (int e = threadIdx.x; e < WG_CO * T; e += 256) {
            const int col = e / T, t = e - col * T;
            dYs[col * d.T + t] = co0 + col < co_n ? ysrc[(size_t)(co0 + col) * T + t] : 0.f;
        }
        __syncthreads();
        const bool outer = !proj && dil < T;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int item = threadIdx.x + 256 * u;       // (co_l, ci) with ci fastest
            const int col = item / WG_CI, ci = item - col * WG_CI;
            if (ci >= nci) continue;
            const float* gr = Gs + ci * Tp;
            const float* yr = dYs + col * d.T;
            float c = accC[u];
            for (int t = 0; t < T; ++t) c += yr[t] * gr[t];
            accC[u] = c;
            if (outer) {
                float lacc = accL[u], racc = accR[u];
                for (int t = dil; t < T; ++t) lacc += yr[t] * gr[t - dil];
                for (int t = 0; t < T - dil; ++t) racc += yr[t] * gr[t + dil];
                accL[u] = lacc;
                accR[u] = racc;
            }
        }
        if (ci0 == 0 && threadIdx.x < WG_CO) {
            const float* yr = dYs + threadIdx.x * d.T;
            for (int t = 0; t < T; ++t) bacc += yr[t];
        }
    }
    float* gw = proj ? g.pw : (which == 0 ? g.c1w[blk] : g.c2w[blk]);
    float* gb = proj ? g.pb : (which == 0 ? g.c1b[blk] : g.c2b[blk]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int item = threadIdx.x + 256 * u;
        const int col = item / WG_CI, ci = item - col * WG_CI;
        if (ci >= nci || co0 + col >= co_n) continue;
        const size_t wi = (size_t)(co0 + col) * ci_n + ci0 + ci;
        if (proj) {
            gw[wi] = accC[u];
        } else {
            gw[wi * 3] = accL[u];
            gw[wi * 3 + 1] = accC[u];
            gw[wi * 3 + 2] = accR[u];
        }
    }
    if (ci0 == 0 && threadIdx.x < WG_CO && co0 + (int)threadIdx.x < co_n) gb[co0 + threadIdx.x] = bacc;
}

__global__ __launch_bounds__(256) void swa_multi_kernel(const t2s_adamw_tensor* __restrict__ tab, int n_tensors, float inv) {
    __shared__ unsigned int first;
    __shared__ t2s_adamw_tensor ent;
    if (threadIdx.x == 0) {
        unsigned int acc = 0;
        int t = 0;
        for (; t < n_tensors; ++t) {
            const unsigned int nbk = (unsigned int)((tab[t].n + 1023) / 1024);
            if (blockIdx.x < acc + nbk) break;
            acc += nbk;
        }
        first = acc;
        ent = tab[t < n_tensors ? t : n_tensors - 1];
    }
    __syncthreads();
    const size_t base = (size_t)(blockIdx.x - first) * 1024;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const size_t i = base + threadIdx.x + 256 * u;
        if (i >= ent.n) return;
        const float a = ent.param[i];
        ent.param[i] = a + (ent.grad[i] - a) * inv;
    }
}

struct Layout {
    size_t act, dact, zpyr, dzI, dzT, simT, simI, losspart, total;   // offsets in floats; total in bytes
};

Layout layout(int cm, int C, int depth, int B, int T) {
    const size_t S = 2 * (size_t)B, nb = depth + 1, plane = (size_t)cm * T, pyr = S * 2 * T * C;
    Layout L{};
    size_t o = 0;
    L.act = o; o += S * nb * 4 * plane;
    L.dact = o; o += S * (2 * nb + 1) * plane;
    L.zpyr = o; o += pyr;
    L.dzI = o; o += pyr;
    L.dzT = o; o += pyr;
    L.simT = o; o += (size_t)B * 2 * (2 * T) * (2 * T);
    L.simI = o; o += (size_t)4 * B * B * 2 * T;
    L.losspart = o; o += (size_t)2 * MAXLEV * PARTS;
    L.total = o * sizeof(float);
    return L;
}

int check_model(const t2s_ts2vec_weights* w, int B, int T, const char* fn) {
    T2S_REQUIRE(w != nullptr, "%s: NULL weights", fn);
    T2S_REQUIRE(w->depth >= 0 && w->depth < T2S_TS2VEC_MAX_BLOCKS && w->input_dims > 0 && w->hidden > 0 && w->output_dims > 0,
                "%s: unsupported sizes (depth=%d, max %d)", fn, w->depth, T2S_TS2VEC_MAX_BLOCKS - 1);
    T2S_REQUIRE(B >= 1 && B <= T2S_TS2VEC_TRAIN_MAX_B, "%s: B=%d is outside 1..%d series per step", fn, B, T2S_TS2VEC_TRAIN_MAX_B);
    T2S_REQUIRE(T >= 1 && T <= T2S_TS2VEC_TRAIN_MAX_T, "%s: T=%d is outside 1..%d time steps", fn, T, T2S_TS2VEC_TRAIN_MAX_T);
    const int cm = w->hidden > w->output_dims ? w->hidden : w->output_dims;
    const size_t lds = (size_t)3 * cm * T * sizeof(float);
    T2S_REQUIRE(lds <= 160 * 1024, "%s: 3 x %d channels x T=%d fp32 planes exceed the 160 KB LDS of a CU", fn, cm, T);
    const size_t lds_loss = ((size_t)2 * (T > B ? T : B) * (w->output_dims + 3)) * sizeof(float);
    T2S_REQUIRE(lds_loss <= 160 * 1024, "%s: the loss tile of %d rows x output_dims=%d exceeds the 160 KB LDS of a CU", fn,
                2 * (T > B ? T : B), w->output_dims);
    return T2S_OK;
}

}  // namespace
}  // namespace t2s

extern "C" uint64_t t2s_ts2vec_train_workspace_bytes(const t2s_ts2vec_weights* w, int max_B, int max_T) {
    using namespace t2s;
    if (check_model(w, max_B, max_T, "t2s_ts2vec_train_workspace_bytes") != T2S_OK) return 0;
    const int cm = w->hidden > w->output_dims ? w->hidden : w->output_dims;
    return layout(cm, w->output_dims, w->depth, max_B, max_T).total;
}

extern "C" int t2s_ts2vec_train_step(const t2s_ts2vec_weights* w, const t2s_ts2vec_grads* grads, const t2s_ts2vec_step* step,
                                     float* loss_out, void* workspace, uint64_t ws_bytes, void* stream) {
    using namespace t2s;
    const char* fn = "t2s_ts2vec_train_step";
    T2S_REQUIRE(w && grads && step && loss_out && workspace, "%s: NULL argument", fn);
    if (int rc = check_model(w, step->B, step->T, fn)) return rc;
    T2S_REQUIRE(w->fc_w && w->fc_b && w->proj_w && w->proj_b, "%s: NULL weight", fn);
    T2S_REQUIRE(grads->fc_w && grads->fc_b && grads->proj_w && grads->proj_b, "%s: NULL pointer in grads (input_fc / projector)", fn);
    for (int i = 0; i <= w->depth; ++i) {
        T2S_REQUIRE(w->conv1_w[i] && w->conv1_b[i] && w->conv2_w[i] && w->conv2_b[i], "%s: NULL weight of block %d", fn, i);
        T2S_REQUIRE(grads->conv1_w[i] && grads->conv1_b[i] && grads->conv2_w[i] && grads->conv2_b[i],
                    "%s: NULL pointer in grads of block %d", fn, i);
    }
    const int B = step->B, T = step->T, C = w->output_dims;
    T2S_REQUIRE(step->x_nan_count == 0, "%s: x holds %d NaN values; the training step takes NaN-free input only", fn, step->x_nan_count);
    T2S_REQUIRE(step->x != nullptr, "%s: NULL x", fn);
    T2S_REQUIRE(step->crop_l >= 1 && step->crop_l <= T, "%s: crop_l=%d is outside 1..T=%d", fn, step->crop_l, T);
    T2S_REQUIRE(step->temporal_unit >= 0, "%s: temporal_unit=%d is negative", fn, step->temporal_unit);
    for (int v = 0; v < 2; ++v) {
        const t2s_ts2vec_view& vw = step->view[v];
        T2S_REQUIRE(vw.start && vw.mask && vw.keep, "%s: NULL pointer in view %d", fn, v);
        T2S_REQUIRE(vw.length >= step->crop_l && vw.length <= T, "%s: view %d length=%d is outside crop_l=%d..T=%d", fn, v, vw.length,
                    step->crop_l, T);
    }
    const int cm = w->hidden > C ? w->hidden : C;
    const Layout lay = layout(cm, C, w->depth, B, T);
    T2S_REQUIRE(ws_bytes >= lay.total, "%s: workspace of %llu bytes is smaller than the %llu that B=%d, T=%d need", fn,
                (unsigned long long)ws_bytes, (unsigned long long)lay.total, B, T);

    TrainDev d{};
    GradDev g{};
    d.cin = w->input_dims; d.hidden = w->hidden; d.cout = C; d.depth = w->depth; d.cm = cm;
    d.B = B; d.T = T; d.crop_l = step->crop_l; d.keep_scale = step->keep_scale;
    d.fc_w = w->fc_w; d.fc_b = w->fc_b; d.pw = w->proj_w; d.pb = w->proj_b;
    g.fc_w = grads->fc_w; g.fc_b = grads->fc_b; g.pw = grads->proj_w; g.pb = grads->proj_b;
    for (int i = 0; i <= w->depth; ++i) {
        d.c1w[i] = w->conv1_w[i]; d.c1b[i] = w->conv1_b[i]; d.c2w[i] = w->conv2_w[i]; d.c2b[i] = w->conv2_b[i];
        g.c1w[i] = grads->conv1_w[i]; g.c1b[i] = grads->conv1_b[i]; g.c2w[i] = grads->conv2_w[i]; g.c2b[i] = grads->conv2_b[i];
    }
    d.x = step->x;
    for (int v = 0; v < 2; ++v) {
        d.len[v] = step->view[v].length; d.start[v] = step->view[v].start; d.mask[v] = step->view[v].mask; d.keep[v] = step->view[v].keep;
    }
    float* ws = (float*)workspace;
    d.act = ws + lay.act; d.dact = ws + lay.dact; d.zpyr = ws + lay.zpyr; d.dzI = ws + lay.dzI; d.dzT = ws + lay.dzT;
    d.simT = ws + lay.simT; d.simI = ws + lay.simI; d.losspart = ws + lay.losspart; d.loss_out = loss_out;
    // the pyramid of hierarchical_contrastive_loss: levels crop_l, crop_l/2, ..., 1; the single-step level is instance-only
    int n = step->crop_l, off = 0, nlev = 0;
    unsigned long long so = 0;
    for (;;) {
        d.L[nlev] = n; d.off[nlev] = off; d.soffT[nlev] = so;
        d.instOn[nlev] = (step->alpha != 0.f && B > 1) ? 1 : 0;
        d.tempOn[nlev] = (n > 1 && nlev >= step->temporal_unit && 1.f - step->alpha != 0.f) ? 1 : 0;
        off += n; so += (unsigned long long)B * 4 * n * n;
        ++nlev;
        if (n == 1) break;
        n >>= 1;
    }
    d.nlev = nlev;
    for (int l = 0; l < nlev; ++l) {
        const float base = 1.0f / ((float)nlev * 2.0f * (float)B * (float)d.L[l]);
        d.coefI[l] = step->alpha * base;
        d.coefT[l] = (1.0f - step->alpha) * base;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t lds_fb = (size_t)3 * cm * T * sizeof(float);
    const int Mmax = 2 * (step->crop_l > B ? step->crop_l : B);
    const size_t lds_loss = ((size_t)Mmax * (C + 1) + 2 * Mmax) * sizeof(float);
    const size_t lds_wg = ((size_t)WG_CI * (T | 1) + (size_t)WG_CO * T + 256) * sizeof(float);
    {
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ts2vec_train_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ts2vec_train_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ts2vec_loss_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ts2vec_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    ts2vec_train_fwd_kernel<<<2 * B, FB_THREADS, lds_fb, st>>>(d);
    T2S_LAUNCH_CHECK();
    const int tasks = step->crop_l > B ? step->crop_l : B;
    ts2vec_loss_kernel<<<dim3(tasks, nlev, 2), FB_THREADS, lds_loss, st>>>(d);
    T2S_LAUNCH_CHECK();
    ts2vec_train_bwd_kernel<<<2 * B, FB_THREADS, lds_fb, st>>>(d);
    T2S_LAUNCH_CHECK();
    const int ntile = ((cm + WG_CO - 1) / WG_CO) * ((cm + WG_CI - 1) / WG_CI);
    ts2vec_wgrad_kernel<<<dim3(ntile > w->hidden ? ntile : w->hidden, 2 * (w->depth + 1) + 2), 256, lds_wg, st>>>(d, g);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_swa_update_multi(const t2s_adamw_tensor* table_dev, int n_tensors, uint64_t total_chunks, int64_t n_averaged,
                                    void* stream) {
    using namespace t2s;
    T2S_REQUIRE(table_dev && n_tensors > 0 && n_tensors <= 64 && total_chunks > 0 && n_averaged >= 1, "t2s_swa_update_multi: bad argument");
    swa_multi_kernel<<<(unsigned)total_chunks, 256, 0, (hipStream_t)stream>>>(table_dev, n_tensors, 1.0f / (float)(n_averaged + 1));
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
