// TSae training: the teacher-forced forward  prediction = decoder(memory = encoder(x), target_seq = x)  in training mode (dropout
// at every site of the torch modules) and its backward, for 1 <= T <= 192.  fp32 throughout (fma and v_mfma_f32_32x32x2_f32), no
// atomics, no scratch; every sum over (series, row) is taken in an order that depends on (B, T, shape) alone.
//
// Dropout masks are never stored: element e of series b at site s is kept iff the 24-bit Philox uniform of (seed, stream s, row b,
// element e) is >= p (include/t2s.h has the site table), and forward and backward evaluate that same rule.
//
// The forward keeps every layer's activations in the workspace (TrainWs below); LayerNorm statistics are recomputed from the saved
// layer inputs (the same instructions on the same data as the forward's), the softmax log-sum-exp is saved per (row, head).
//   tsae_train_embed_kernel      value embedding, dropout, LayerNorm, + position, dropout | shifted input projection, + position, dropout
//   tsae_train_rows_kernel       y = [res +] drop(act(Linear(drop([LayerNorm] x)))) on a 32-row tile of one series: every projection
//                                of the forward, and every data-gradient product of the backward (the weight as torch holds it),
//                                there optionally through the LayerNorm's backward and added onto the residual gradient
//   tsae_train_attn_kernel       one (head, series) per workgroup, K / V of the head in LDS, one query per lane, two passes
//   tsae_train_attn_bwd_kernel   dQ with the query on the lane, then dK / dV with the key on the lane: no sum crosses a workgroup
//   tsae_train_dw_kernel         dW (N,K) = sum over rows of dy (x) in, rows cut into S = min(tiles, 128) contiguous shares
//   tsae_train_reduce_kernel     the S partial sums (and the per-tile LayerNorm partials) added in a fixed tree
//   tsae_train_embed_bwd_kernel  the gradient at an embedding's output (encoder: through dropout, LayerNorm, dropout; decoder: shifted)
#include "t2s_tsae.h"

namespace t2s {
namespace {

using namespace tsae;

constexpr int TR_MAXT = T2S_TSAE_TRAIN_MAX_T;   // 192
constexpr int TR_MAXS = 128;                    // shares of the row range in a weight-gradient sum

enum { SITE_ENC_EMB = 0, SITE_ENC_POS = 1, SITE_DEC_POS = 2, SITE_NONE = -1 };
inline int enc_site(int layer, int k) { return 16 + 4 * layer + k; }   // k: 0 probabilities, 1 after attention, 2 FFN hidden, 3 after FFN
inline int dec_site(int layer, int k) { return 64 + 6 * layer + k; }   // k: 0 self probs, 1 after self, 2 cross probs, 3 after cross, 4 hidden, 5 after FFN

struct Drop { uint64_t seed; float p, scale; };   // scale = 1 / (1 - p); p == 0: no Philox work anywhere

__device__ __forceinline__ u32x4 drop_quad(const Drop& d, uint32_t site, uint32_t b, uint32_t quad) {
    return philox4x32_10(u32x4{quad, b, site, 0u}, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
}
__device__ __forceinline__ float drop_pick(const Drop& d, const u32x4& r, uint32_t e) {
    const uint32_t v = (e & 3) == 0 ? r.x : ((e & 3) == 1 ? r.y : ((e & 3) == 2 ? r.z : r.w));
    return ((float)(v >> 8) * (1.0f / 16777216.0f) >= d.p) ? d.scale : 0.f;
}
// what element e of series b is multiplied by at `site`: 1 / (1 - p) or 0; 1 where there is no dropout
__device__ __forceinline__ float drop_mul(const Drop& d, int site, uint32_t b, uint32_t e) {
    if (site < 0 || !(d.p > 0.f)) return 1.f;
    return drop_pick(d, drop_quad(d, (uint32_t)site, b, e >> 2), e);
}

// src (B,T,F) -> x (B*T,64), one wave per row, lane = channel.  Encoder (shift 0): drop1(LayerNorm(drop0(W src[i] + b)) + pe[i]);
// decoder (shift 1): drop2((i ? W src[i-1] + b : 0) + pe[i]).
__global__ __launch_bounds__(256) void tsae_train_embed_kernel(const float* __restrict__ src, float* __restrict__ x, Lin lin, Norm ln,
                                                               const float* __restrict__ pe, int F, int T, size_t rows, int shift, Drop d) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const uint32_t b = (uint32_t)(row / (size_t)T), i = (uint32_t)(row % (size_t)T);
    float v = 0.f;
    if (!(shift && i == 0)) {
        const float* s = src + (row - shift) * (size_t)F;
        v = lin.b[lane];
        for (int f = 0; f < F; ++f) v = fmaf(s[f], lin.w[f * TS_D + lane], v);
    }
    if (!shift) {
        v *= drop_mul(d, SITE_ENC_EMB, b, i * TS_D + lane);
        v = layer_norm_lane(v, ln.g[lane], ln.b[lane]);
    }
    v += pe[(size_t)i * TS_D + lane];
    x[row * TS_D + lane] = v * drop_mul(d, shift ? SITE_DEC_POS : SITE_ENC_POS, b, i * TS_D + lane);
}

// One product on a 32-row tile of one series (grid: tiles x B):
//   in  = drop_in([LayerNorm] x[row][0..K))                      K a multiple of 32, columns >= kvalid read as 0; LayerNorm: K = 64
//   v   = in . w[0..K)[0..N) (+ bias) (relu) (0 where gate <= 0)    N a multiple of 32; K <= 128 or N = 64
//   y   = (res +) drop_out(v)                                     columns < nvalid
// or, with lnx: y += LayerNorm_backward(v; lnx, lng) (N = 64), the tile's sums of v * xhat and v going to parts[tile][2][64].
struct RowOp {
    const float* x; int ldx, K, kvalid;
    Norm ln; int in_site, in_w;
    const float* w; int ldw; const float* bias; int N, nvalid;
    int relu; const float* gate; int out_site; const float* res; float* y; int ldy;
    const float* lnx; const float* lng; float* parts;
};

__global__ __launch_bounds__(256) void tsae_train_rows_kernel(RowOp o, int T, Drop d) {
    __shared__ float xs[32][128 + 1];
    __shared__ float red[2][16][64];
    __shared__ float ys[32][TS_D + 1];
    __shared__ float lnp[4][2][TS_D];
    const int b = blockIdx.y, t0 = blockIdx.x * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
    const size_t row0 = (size_t)b * T + t0;
    const bool one_chunk = o.K <= 128;
    const int kh = wave >> 1;   // the wave pairs {0,1} and {2,3} split every chunk's k range, added in that order
    for (int n0 = 0; n0 < o.N; n0 += 64) {
        const int ct = (n0 >> 5) + (wave & 1);
        const bool tile_ok = ct * 32 < o.N;
        f32x16 acc = {0};
        for (int c0 = 0; c0 < o.K; c0 += 128) {
            const int len = min(128, o.K - c0);
            if (!one_chunk || n0 == 0) {
                __syncthreads();
                float g = 1.f, be = 0.f;
                if (o.ln.g) {
                    g = o.ln.g[lane];
                    be = o.ln.b[lane];
                }
                for (int r = wave * 8; r < wave * 8 + 8; ++r) {
                    const int t = t0 + r;
                    for (int cc = 0; cc < len; cc += 64) {
                        const int col = c0 + cc + lane;
                        float v = (t < T && col < o.kvalid) ? o.x[(row0 + r) * (size_t)o.ldx + col] : 0.f;
                        if (o.ln.g) v = layer_norm_lane(v, g, be);
                        if (t < T) v *= drop_mul(d, o.in_site, b, (uint32_t)t * o.in_w + col);
                        xs[r][cc + lane] = v;
                    }
                }
                __syncthreads();
            }
            if (tile_ok) acc = tile_gemm(&xs[0][0], 128 + 1, o.w + (size_t)c0 * o.ldw, o.ldw, ct * 32, kh * (len >> 1), (kh + 1) * (len >> 1), acc);
        }
        __syncthreads();
        if (wave >= 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave - 2][r][lane] = acc[r];
        }
        __syncthreads();
        if (wave < 2 && tile_ok) {
            const int col = ct * 32 + (lane & 31);
            if (o.lnx) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ys[acc_row(r, half)][col] = acc[r] + red[wave][r][lane];
            } else if (col < o.nvalid) {
                const float bias = o.bias ? o.bias[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = acc_row(r, half), t = t0 + row;
                    if (t < T) {
                        const size_t gr = row0 + row;
                        float v = (acc[r] + red[wave][r][lane]) + bias;
                        if (o.relu) v = fmaxf(v, 0.f);
                        if (o.gate) v = o.gate[gr * o.N + col] > 0.f ? v : 0.f;
                        v *= drop_mul(d, o.out_site, b, (uint32_t)t * o.N + col);
                        if (o.res) v += o.res[gr * o.ldy + col];
                        o.y[gr * o.ldy + col] = v;
                    }
                }
            }
        }
    }
    if (!o.lnx) return;
    __syncthreads();
    const float g = o.lng[lane];
    float pg = 0.f, pb = 0.f;
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        const bool valid = t0 + r < T;
        const float x = valid ? o.lnx[(row0 + r) * TS_D + lane] : 0.f;
        const float mean = wave_sum(x) * (1.0f / TS_D);
        const float dd = x - mean;
        const float var = wave_sum(dd * dd) * (1.0f / TS_D);
        const float rstd = 1.0f / sqrtf(var + TS_EPS), xhat = dd * rstd;
        const float dn = valid ? ys[r][lane] : 0.f;
        const float dxh = dn * g;
        const float m1 = wave_sum(dxh) * (1.0f / TS_D), m2 = wave_sum(dxh * xhat) * (1.0f / TS_D);
        if (valid) o.y[(row0 + r) * TS_D + lane] += rstd * (dxh - m1 - xhat * m2);
        pg = fmaf(dn, xhat, pg);
        pb += dn;
    }
    lnp[wave][0][lane] = pg;
    lnp[wave][1][lane] = pb;
    __syncthreads();
    if (threadIdx.x < 2 * TS_D) {
        const int k = threadIdx.x >> 6;
        o.parts[((size_t)b * gridDim.x + blockIdx.x) * (2 * TS_D) + threadIdx.x] =
            (lnp[0][k][lane] + lnp[1][k][lane]) + (lnp[2][k][lane] + lnp[3][k][lane]);
    }
}

template <int DH>
__device__ __forceinline__ float dot_row(const float (&a)[DH], const float* b) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < DH; ++e) s = fmaf(a[e], b[e], s);
    return s;
}

// o[b, i, h*DH ..] = sum_j drop(softmax_j(q_i . k_j * scale)) v_j, j < T (causal: j <= i); lse[b, i, h] = ln sum_j exp(..).
// grid (H, B), 64 * ceil(T / 64) threads, one query per lane; the head's K and V rows in LDS.
template <int DH>
__global__ __launch_bounds__(TR_MAXT) void tsae_train_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int ldkv, float* __restrict__ o,
                                                                  float* __restrict__ lse, int T, int causal, float scale, int site, Drop d) {
    __shared__ __attribute__((aligned(16))) float ks[TR_MAXT][DH];
    __shared__ __attribute__((aligned(16))) float vs[TR_MAXT][DH];
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
    for (int j = tid; j < T; j += blockDim.x) {
        const size_t off = ((size_t)b * T + j) * ldkv + h * DH;
#pragma unroll
        for (int e = 0; e < DH; e += 4) {
            *(f32x4*)&ks[j][e] = *(const f32x4*)(k + off + e);
            *(f32x4*)&vs[j][e] = *(const f32x4*)(v + off + e);
        }
    }
    __syncthreads();
    const int i = tid;
    if (i >= T) return;
    float qr[DH], acc[DH];
    {
        const float* qp = q + ((size_t)b * T + i) * ldq + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            qr[e] = qp[e] * scale;
            acc[e] = 0.f;
        }
    }
    const int nk = causal ? i + 1 : T;
    float m = -INFINITY;
    for (int j = 0; j < nk; ++j) m = fmaxf(m, dot_row<DH>(qr, ks[j]));
    float l = 0.f;
    const uint32_t base = (uint32_t)(h * T + i) * (uint32_t)T;
    const bool dropping = site >= 0 && d.p > 0.f;
    u32x4 rnd = {0u, 0u, 0u, 0u};
    for (int j = 0; j < nk; ++j) {
        float p = expf(dot_row<DH>(qr, ks[j]) - m);
        l += p;
        if (dropping) {
            const uint32_t e = base + j;
            if (j == 0 || (e & 3) == 0) rnd = drop_quad(d, (uint32_t)site, b, e >> 2);
            p *= drop_pick(d, rnd, e);
        }
#pragma unroll
        for (int e = 0; e < DH; ++e) acc[e] = fmaf(p, vs[j][e], acc[e]);
    }
    const float inv = 1.0f / l;
    float* op = o + ((size_t)b * T + i) * TS_D + h * DH;
#pragma unroll
    for (int e = 0; e < DH; ++e) op[e] = acc[e] * inv;
    lse[((size_t)b * T + i) * H + h] = m + logf(l);
}

// The backward of the kernel above from (q, k, v, its output o, lse) and do = d loss / d o: dq, dk, dv.  Same grid and block; thread
// t first is query t (dq: a walk over the keys), then key t (dk, dv: a walk over the queries).  P is recomputed as exp(s - lse).
template <int DH>
__global__ __launch_bounds__(TR_MAXT) void tsae_train_attn_bwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                      const float* __restrict__ v, int ldkv, const float* __restrict__ o,
                                                                      const float* __restrict__ dout, const float* __restrict__ lse,
                                                                      float* __restrict__ dq, int lddq, float* __restrict__ dk,
                                                                      float* __restrict__ dv, int lddkv, int T, int causal, float scale,
                                                                      int site, Drop d) {
    __shared__ __attribute__((aligned(16))) float ks[TR_MAXT][DH];
    __shared__ __attribute__((aligned(16))) float vs[TR_MAXT][DH];
    __shared__ __attribute__((aligned(16))) float qs[TR_MAXT][DH];
    __shared__ __attribute__((aligned(16))) float dos[TR_MAXT][DH];
    __shared__ float lses[TR_MAXT], dels[TR_MAXT];
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
    for (int j = tid; j < T; j += blockDim.x) {
        const size_t row = (size_t)b * T + j;
        const size_t off = row * ldkv + h * DH;
        float del = 0.f;
#pragma unroll
        for (int e = 0; e < DH; e += 4) {
            *(f32x4*)&ks[j][e] = *(const f32x4*)(k + off + e);
            *(f32x4*)&vs[j][e] = *(const f32x4*)(v + off + e);
            const f32x4 q4 = *(const f32x4*)(q + row * ldq + h * DH + e);
            const f32x4 d4 = *(const f32x4*)(dout + row * TS_D + h * DH + e);
            const f32x4 o4 = *(const f32x4*)(o + row * TS_D + h * DH + e);
            *(f32x4*)&qs[j][e] = q4 * scale;
            *(f32x4*)&dos[j][e] = d4;
#pragma unroll
            for (int c = 0; c < 4; ++c) del = fmaf(d4[c], o4[c], del);
        }
        dels[j] = del;
        lses[j] = lse[row * H + h];
    }
    __syncthreads();
    const int t = tid;
    if (t >= T) return;
    const bool dropping = site >= 0 && d.p > 0.f;
    float kr[DH], vr[DH], ga[DH], gb[DH];
    {   // query t
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            kr[e] = qs[t][e];    // (the query and its do, in the registers the key phase reuses)
            vr[e] = dos[t][e];
            ga[e] = 0.f;
        }
        const float li = lses[t], di = dels[t];
        const int nk = causal ? t + 1 : T;
        const uint32_t base = (uint32_t)(h * T + t) * (uint32_t)T;
        u32x4 rnd = {0u, 0u, 0u, 0u};
        for (int j = 0; j < nk; ++j) {
            const float p = expf(dot_row<DH>(kr, ks[j]) - li);
            float dp = dot_row<DH>(vr, vs[j]);
            if (dropping) {
                const uint32_t e = base + j;
                if (j == 0 || (e & 3) == 0) rnd = drop_quad(d, (uint32_t)site, b, e >> 2);
                dp *= drop_pick(d, rnd, e);
            }
            const float ds = p * (dp - di);
#pragma unroll
            for (int e = 0; e < DH; ++e) ga[e] = fmaf(ds, ks[j][e], ga[e]);
        }
        float* qp = dq + ((size_t)b * T + t) * lddq + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) qp[e] = ga[e] * scale;
    }
    {   // key t
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            kr[e] = ks[t][e];
            vr[e] = vs[t][e];
            ga[e] = 0.f;
            gb[e] = 0.f;
        }
        for (int i = causal ? t : 0; i < T; ++i) {
            const float p = expf(dot_row<DH>(kr, qs[i]) - lses[i]);
            const float mul = dropping ? drop_mul(d, site, b, (uint32_t)(h * T + i) * (uint32_t)T + t) : 1.f;
            const float pm = p * mul;
            const float ds = p * (mul * dot_row<DH>(vr, dos[i]) - dels[i]);
#pragma unroll
            for (int e = 0; e < DH; ++e) {
                gb[e] = fmaf(pm, dos[i][e], gb[e]);
                ga[e] = fmaf(ds, qs[i][e], ga[e]);
            }
        }
        float* kp = dk + ((size_t)b * T + t) * lddkv + h * DH;
        float* vp = dv + ((size_t)b * T + t) * lddkv + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            kp[e] = ga[e];
            vp[e] = gb[e];
        }
    }
}

// Share s (of gridDim.x) of  dW[n][k] = sum_rows dy'[row][n] in'[row][k]  and  db[n] = sum_rows dy'[row][n]  for the 64 x 64 block
// (blockIdx.y, blockIdx.z) of (N, K): dy' = drop(dy) (width 64), in' = drop([LayerNorm] in).  The 32-row tiles of all series are cut
// into gridDim.x contiguous shares; a share's partial sum goes to pw[s][N][K] / pb[s][N] (an empty share writes zeros).
struct DwOp {
    const float* dy; int ldy, nvalid, dy_site;
    const float* in; int ldin, kvalid; Norm ln; int in_site, in_w;
    float* pw; float* pb; int N, K;
};

__global__ __launch_bounds__(256) void tsae_train_dw_kernel(DwOp o, int B, int T, Drop d) {
    __shared__ float dys[32][TS_D + 1];
    __shared__ float ins[32][TS_D + 1];
    const int s = blockIdx.x, n0 = blockIdx.y * 64, k0 = blockIdx.z * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
    const int tiles_t = (T + 31) / 32, n_tiles = B * tiles_t, per = (n_tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int first = s * per, last = min(n_tiles, first + per);
    const int nt = wave & 1, kt = wave >> 1;
    float g = 1.f, be = 0.f;
    if (o.ln.g) {
        g = o.ln.g[lane];
        be = o.ln.b[lane];
    }
    f32x16 acc = {0};
    float bsum = 0.f;
    for (int tile = first; tile < last; ++tile) {
        const int b = tile / tiles_t, t0 = (tile - b * tiles_t) * 32;
        const size_t row0 = (size_t)b * T + t0;
        __syncthreads();
        for (int r = wave * 8; r < wave * 8 + 8; ++r) {
            const int t = t0 + r, nc = n0 + lane, kc = k0 + lane;
            float dyv = (t < T && nc < o.nvalid) ? o.dy[(row0 + r) * (size_t)o.ldy + nc] : 0.f;
            float inv = (t < T && kc < o.kvalid) ? o.in[(row0 + r) * (size_t)o.ldin + kc] : 0.f;
            if (o.ln.g) inv = layer_norm_lane(inv, g, be);
            if (t < T) {
                dyv *= drop_mul(d, o.dy_site, b, (uint32_t)t * TS_D + nc);
                inv *= drop_mul(d, o.in_site, b, (uint32_t)t * o.in_w + kc);
            }
            dys[r][lane] = dyv;
            ins[r][lane] = inv;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 32; rr += 2) acc = mfma32(dys[rr + half][nt * 32 + j], ins[rr + half][kt * 32 + j], acc);
        if (k0 == 0 && threadIdx.x < 64) {
            for (int r = 0; r < 32; ++r) bsum += dys[r][threadIdx.x];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
        o.pw[((size_t)s * o.N + n0 + nt * 32 + acc_row(r, half)) * o.K + k0 + kt * 32 + j] = acc[r];
    if (k0 == 0 && threadIdx.x < 64) o.pb[(size_t)s * o.N + n0 + threadIdx.x] = bsum;
}

// ow[n][k] = sum_s pw[s * sw + n * K + k] (n < nvalid, k < kvalid; ow is (nvalid, kvalid)) and ob[n] = sum_s pb[s * sb + n]
// (n < nbvalid).  16 outputs x 16 strided partial sums per workgroup, the 16 added as a fixed tree.
struct RedOp {
    const float* pw; size_t sw; int N, K, nvalid, kvalid; float* ow;
    const float* pb; size_t sb; int NB, nbvalid; float* ob;
    int S;
};

__global__ __launch_bounds__(256) void tsae_train_reduce_kernel(RedOp o) {
    __shared__ float part[16][17];
    const int ol = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + ol, nw = o.N * o.K;
    const float* src = nullptr;
    float* dst = nullptr;
    size_t stride = 0;
    if (i < nw) {
        const int n = i / o.K, k = i - n * o.K;
        if (n < o.nvalid && k < o.kvalid) {
            src = o.pw + i;
            stride = o.sw;
            dst = o.ow + (size_t)n * o.kvalid + k;
        }
    } else if (i - nw < o.nbvalid) {
        src = o.pb + (i - nw);
        stride = o.sb;
        dst = o.ob + (i - nw);
    }
    float a = 0.f;
    if (dst)
        for (int s = sl; s < o.S; s += 16) a += src[(size_t)s * stride];
    part[ol][sl] = a;
    __syncthreads();
    if (sl == 0 && dst) {
        const float* p = part[ol];
        *dst = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) +
               (((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15])));
    }
}

// g (B*T,64) = d loss / d (an embedding kernel's output) -> demb (B*T,64) = d loss / d (W src + b), rows as the weight gradient
// pairs them with src.  Decoder (shift 1): demb[t] = drop2(g[t+1]), the last row 0.  Encoder: back through drop1, the LayerNorm
// (its tile sums to parts) and drop0.  grid (tiles, B), a wave per 8 rows, lane = channel.
__global__ __launch_bounds__(256) void tsae_train_embed_bwd_kernel(const float* __restrict__ src, const float* __restrict__ g,
                                                                   float* __restrict__ demb, Lin lin, Norm ln, float* __restrict__ parts,
                                                                   int F, int T, int shift, Drop d) {
    __shared__ float lnp[4][2][TS_D];
    const int b = blockIdx.y, t0 = blockIdx.x * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row0 = (size_t)b * T + t0;
    if (shift) {
        for (int r = wave * 8; r < wave * 8 + 8; ++r) {
            const int t = t0 + r;
            if (t < T)
                demb[(row0 + r) * TS_D + lane] =
                    t + 1 < T ? g[(row0 + r + 1) * TS_D + lane] * drop_mul(d, SITE_DEC_POS, b, (uint32_t)(t + 1) * TS_D + lane) : 0.f;
        }
        return;
    }
    const float gam = ln.g[lane];
    float pg = 0.f, pb = 0.f;
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        const int t = t0 + r;
        const bool valid = t < T;
        float x = 0.f, k0 = 1.f, dn = 0.f;
        if (valid) {
            const float* s = src + (row0 + r) * (size_t)F;
            x = lin.b[lane];
            for (int f = 0; f < F; ++f) x = fmaf(s[f], lin.w[f * TS_D + lane], x);
            k0 = drop_mul(d, SITE_ENC_EMB, b, (uint32_t)t * TS_D + lane);
            x *= k0;
            dn = g[(row0 + r) * TS_D + lane] * drop_mul(d, SITE_ENC_POS, b, (uint32_t)t * TS_D + lane);
        }
        const float mean = wave_sum(x) * (1.0f / TS_D);
        const float dd = x - mean;
        const float var = wave_sum(dd * dd) * (1.0f / TS_D);
        const float rstd = 1.0f / sqrtf(var + TS_EPS), xhat = dd * rstd;
        const float dxh = dn * gam;
        const float m1 = wave_sum(dxh) * (1.0f / TS_D), m2 = wave_sum(dxh * xhat) * (1.0f / TS_D);
        if (valid) demb[(row0 + r) * TS_D + lane] = rstd * (dxh - m1 - xhat * m2) * k0;
        pg = fmaf(dn, xhat, pg);
        pb += dn;
    }
    lnp[wave][0][lane] = pg;
    lnp[wave][1][lane] = pb;
    __syncthreads();
    if (threadIdx.x < 2 * TS_D) {
        const int k = threadIdx.x >> 6;
        parts[((size_t)b * gridDim.x + blockIdx.x) * (2 * TS_D) + threadIdx.x] =
            (lnp[0][k][lane] + lnp[1][k][lane]) + (lnp[2][k][lane] + lnp[3][k][lane]);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// The workspace: what the forward leaves for the backward (per layer), then the backward's own buffers.  x*[l] is layer l's input
// (x*[n] the stack's output), x1 / x2 the residual stream after the first / second sublayer, h the FFN hidden rows after the ReLU.
struct TrainWs {
    float *xe[TS_ML + 1], *qkve[TS_ML], *lsee[TS_ML], *atte[TS_ML], *x1e[TS_ML], *he[TS_ML];
    float *xd[TS_ML + 1], *qkvd[TS_ML], *lsed[TS_ML], *attd[TS_ML], *x1d[TS_ML], *cq[TS_ML], *ckv[TS_ML], *lse2[TS_ML], *att2[TS_ML],
        *x2d[TS_ML], *hd[TS_ML];
    float *g, *dmem, *datt, *dqkv, *dh, *pw, *pb, *pln;
    size_t floats;
};

inline int n_tiles_of(int B, int T) { return B * ((T + 31) / 32); }
inline int shares_of(int B, int T) { return n_tiles_of(B, T) < TR_MAXS ? n_tiles_of(B, T) : TR_MAXS; }

TrainWs carve(const t2s_tsae* h, int B, int T, float* base) {
    TrainWs w{};
    size_t off = 0;
    const size_t rows = (size_t)B * T;
    auto take = [&](size_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 63) & ~(size_t)63;
        return p;
    };
    for (int l = 0; l <= h->n_enc; ++l) w.xe[l] = take(rows * TS_D);
    for (int l = 0; l < h->n_enc; ++l) {
        w.qkve[l] = take(rows * 3 * TS_D), w.lsee[l] = take(rows * 8), w.atte[l] = take(rows * TS_D);
        w.x1e[l] = take(rows * TS_D), w.he[l] = take(rows * h->dff);
    }
    for (int l = 0; l <= h->n_dec; ++l) w.xd[l] = take(rows * TS_D);
    for (int l = 0; l < h->n_dec; ++l) {
        w.qkvd[l] = take(rows * 3 * TS_D), w.lsed[l] = take(rows * 8), w.attd[l] = take(rows * TS_D), w.x1d[l] = take(rows * TS_D);
        w.cq[l] = take(rows * TS_D), w.ckv[l] = take(rows * 2 * TS_D), w.lse2[l] = take(rows * 8), w.att2[l] = take(rows * TS_D);
        w.x2d[l] = take(rows * TS_D), w.hd[l] = take(rows * h->dff);
    }
    w.g = take(rows * TS_D), w.dmem = take(rows * TS_D), w.datt = take(rows * TS_D), w.dqkv = take(rows * 3 * TS_D);
    w.dh = take(rows * h->dff);
    const size_t S = shares_of(B, T), nmax = h->dff > 3 * TS_D ? h->dff : 3 * TS_D;
    w.pw = take(S * nmax * TS_D), w.pb = take(S * nmax), w.pln = take((size_t)n_tiles_of(B, T) * 2 * TS_D);
    w.floats = off;
    return w;
}

int check_train(const char* who, const t2s_tsae* h, int B, int T, float p, const void* ws, uint64_t ws_bytes) {
    T2S_REQUIRE(h != nullptr, "%s: handle is NULL", who);
    T2S_REQUIRE(h->n_enc >= 1 && h->n_dec >= 1, "%s: training needs a two-sided handle (n_enc=%d, n_dec=%d)", who, h->n_enc, h->n_dec);
    T2S_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d unsupported (1..65535)", who, B);
    T2S_REQUIRE(T >= 1 && T <= TR_MAXT, "%s: T=%d unsupported (1..%d, T2S_TSAE_TRAIN_MAX_T)", who, T, TR_MAXT);
    T2S_REQUIRE(p >= 0.f && p < 1.f, "%s: p_drop=%g unsupported (0 <= p < 1)", who, (double)p);   // false for a NaN
    T2S_REQUIRE(ws != nullptr, "%s: workspace is NULL", who);
    T2S_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const uint64_t need = (uint64_t)carve(h, B, T, nullptr).floats * sizeof(float);
    T2S_REQUIRE(ws_bytes >= need, "%s: workspace of %llu bytes is too small: B=%d T=%d needs %llu (t2s_tsae_train_workspace_bytes)", who,
                (unsigned long long)ws_bytes, B, T, (unsigned long long)need);
    return T2S_OK;
}

// One call's constants, and the launches in terms of them.
struct Run {
    const t2s_tsae* h;
    int B, T;
    Drop d;
    hipStream_t s;
    TrainWs w;

    dim3 tiles() const { return dim3((T + 31) / 32, B); }

    // y = [res +] drop_out(act(Linear(drop_in([ln] x)))): lin.w is (K, N)
    int rows(const float* x, int ldx, int K, Norm ln, int in_site, const float* wt, const float* bias, int N, int nvalid, int relu,
             int out_site, const float* res, float* y, int ldy) const {
        RowOp o{};
        o.x = x, o.ldx = ldx, o.K = K, o.kvalid = K, o.ln = ln, o.in_site = in_site, o.in_w = K;
        o.w = wt, o.ldw = N, o.bias = bias, o.N = N, o.nvalid = nvalid, o.relu = relu, o.out_site = out_site, o.res = res, o.y = y, o.ldy = ldy;
        tsae_train_rows_kernel<<<tiles(), 256, 0, s>>>(o, T, d);
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }
    // dx = drop_out(gate(drop_in(dy) . wt)), wt (K = the forward's outputs, N = its inputs) as torch holds the weight;
    // with lnx: g += LayerNorm_backward(dy . wt) and the norm's two gradients
    int back(const float* dy, int ldy_, int K, int kvalid, int in_site, const float* wt, int N, const float* gate, int out_site,
             const float* res, float* y, const float* lnx = nullptr, Norm ln = Norm{nullptr, nullptr}, float* gg = nullptr,
             float* gb = nullptr) const {
        RowOp o{};
        o.x = dy, o.ldx = ldy_, o.K = K, o.kvalid = kvalid, o.in_site = in_site, o.in_w = TS_D;
        o.w = wt, o.ldw = N, o.N = N, o.nvalid = N, o.gate = gate, o.out_site = out_site, o.res = res, o.y = y, o.ldy = N;
        o.lnx = lnx, o.lng = ln.g, o.parts = w.pln;
        tsae_train_rows_kernel<<<tiles(), 256, 0, s>>>(o, T, d);
        T2S_LAUNCH_CHECK();
        if (lnx) TS_TRY(norm_grads(gg, gb));
        return T2S_OK;
    }
    int norm_grads(float* gg, float* gb) const {
        RedOp r{};
        r.pw = w.pln, r.sw = 2 * TS_D, r.N = 1, r.K = TS_D, r.nvalid = 1, r.kvalid = TS_D, r.ow = gg;
        r.pb = w.pln + TS_D, r.sb = 2 * TS_D, r.NB = TS_D, r.nbvalid = TS_D, r.ob = gb, r.S = n_tiles_of(B, T);
        tsae_train_reduce_kernel<<<(2 * TS_D + 15) / 16, 256, 0, s>>>(r);
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }
    // gw (nvalid, kvalid) = sum_rows drop(dy)^T drop([ln] in), gb (nvalid) = sum_rows drop(dy)
    int dw(const float* dy, int ldy_, int nvalid, int dy_site, const float* in, int ldin, int kvalid, Norm ln, int in_site, float* gw,
           float* gb) const {
        DwOp o{};
        const int N = (nvalid + 63) & ~63, K = (kvalid + 63) & ~63, S = shares_of(B, T);
        o.dy = dy, o.ldy = ldy_, o.nvalid = nvalid, o.dy_site = dy_site, o.in = in, o.ldin = ldin, o.kvalid = kvalid, o.ln = ln;
        o.in_site = in_site, o.in_w = kvalid, o.pw = w.pw, o.pb = w.pb, o.N = N, o.K = K;
        tsae_train_dw_kernel<<<dim3(S, N / 64, K / 64), 256, 0, s>>>(o, B, T, d);
        T2S_LAUNCH_CHECK();
        RedOp r{};
        r.pw = w.pw, r.sw = (size_t)N * K, r.N = N, r.K = K, r.nvalid = nvalid, r.kvalid = kvalid, r.ow = gw;
        r.pb = w.pb, r.sb = N, r.NB = N, r.nbvalid = nvalid, r.ob = gb, r.S = S;
        tsae_train_reduce_kernel<<<(N * K + N + 15) / 16, 256, 0, s>>>(r);
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }
    int attn(const float* q, int ldq, const float* k, const float* v, int ldkv, float* o, float* lse, int causal, int site) const {
        const dim3 grid(h->heads, B);
        const int threads = 64 * ((T + 63) / 64);
        if (h->heads == 8)
            tsae_train_attn_kernel<8><<<grid, threads, 0, s>>>(q, ldq, k, v, ldkv, o, lse, T, causal, 1.0f / sqrtf(8.0f), site, d);
        else
            tsae_train_attn_kernel<16><<<grid, threads, 0, s>>>(q, ldq, k, v, ldkv, o, lse, T, causal, 1.0f / sqrtf(16.0f), site, d);
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }
    int attn_bwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* o, const float* dout, const float* lse,
                 float* dq, int lddq, float* dk, float* dv, int lddkv, int causal, int site) const {
        const dim3 grid(h->heads, B);
        const int threads = 64 * ((T + 63) / 64);
        if (h->heads == 8)
            tsae_train_attn_bwd_kernel<8><<<grid, threads, 0, s>>>(q, ldq, k, v, ldkv, o, dout, lse, dq, lddq, dk, dv, lddkv, T, causal,
                                                                   1.0f / sqrtf(8.0f), site, d);
        else
            tsae_train_attn_bwd_kernel<16><<<grid, threads, 0, s>>>(q, ldq, k, v, ldkv, o, dout, lse, dq, lddq, dk, dv, lddkv, T, causal,
                                                                    1.0f / sqrtf(16.0f), site, d);
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }

    // x_out = x_in + drop_out(W2 drop_hid(relu(W1 LayerNorm(x_in) + b1)) + b2)
    int ffn(const float* x_in, float* hid, float* x_out, Lin l1, Lin l2, Norm n, int site_hid, int site_out) const {
        const Norm none{nullptr, nullptr};
        TS_TRY(rows(x_in, TS_D, TS_D, n, SITE_NONE, l1.w, l1.b, h->dff, h->dff, 1, SITE_NONE, nullptr, hid, h->dff));
        return rows(hid, h->dff, h->dff, none, site_hid, l2.w, l2.b, TS_D, TS_D, 0, site_out, x_in, x_out, TS_D);
    }
    // w.g holds d loss / d x_out on entry and d loss / d x_in on return
    int ffn_bwd(const float* x_in, const float* hid, Lin l1, Lin l2, Norm n, int site_hid, int site_out, float* g_l1w, float* g_l1b,
                float* g_l2w, float* g_l2b, float* g_ng, float* g_nb) const {
        const Norm none{nullptr, nullptr};
        const int dff = h->dff;
        TS_TRY(dw(w.g, TS_D, TS_D, site_out, hid, dff, dff, none, site_hid, g_l2w, g_l2b));
        TS_TRY(back(w.g, TS_D, TS_D, TS_D, site_out, l2.t, dff, hid, site_hid, nullptr, w.dh));
        TS_TRY(dw(w.dh, dff, dff, SITE_NONE, x_in, TS_D, TS_D, n, SITE_NONE, g_l1w, g_l1b));
        return back(w.dh, dff, dff, dff, SITE_NONE, l1.t, TS_D, nullptr, SITE_NONE, nullptr, w.g, x_in, n, g_ng, g_nb);
    }
    // the out-projection of an attention sublayer, backwards: its two gradients, and w.datt = d loss / d (attention output)
    int out_proj_bwd(const float* att, Lin out, int site_out, float* g_w, float* g_b) const {
        const Norm none{nullptr, nullptr};
        TS_TRY(dw(w.g, TS_D, TS_D, site_out, att, TS_D, TS_D, none, SITE_NONE, g_w, g_b));
        return back(w.g, TS_D, TS_D, TS_D, site_out, out.t, TS_D, nullptr, SITE_NONE, nullptr, w.datt);
    }
    // a self-attention sublayer x_out = x_in + drop(out(attn(qkv(LayerNorm(x_in))))), backwards
    int self_bwd(const float* x_in, const float* qkv, const float* lse, const float* att, Lin lqkv, Lin lout, Norm n, int causal,
                 int site_p, int site_out, const t2s_tsae_attn_weights& ga, float* g_ng, float* g_nb) const {
        TS_TRY(out_proj_bwd(att, lout, site_out, (float*)ga.out_proj_w, (float*)ga.out_proj_b));
        TS_TRY(attn_bwd(qkv, 3 * TS_D, qkv + TS_D, qkv + 2 * TS_D, 3 * TS_D, att, w.datt, lse, w.dqkv, 3 * TS_D, w.dqkv + TS_D,
                        w.dqkv + 2 * TS_D, 3 * TS_D, causal, site_p));
        TS_TRY(dw(w.dqkv, 3 * TS_D, 3 * TS_D, SITE_NONE, x_in, TS_D, TS_D, n, SITE_NONE, (float*)ga.in_proj_w, (float*)ga.in_proj_b));
        return back(w.dqkv, 3 * TS_D, 3 * TS_D, 3 * TS_D, SITE_NONE, lqkv.t, TS_D, nullptr, SITE_NONE, nullptr, w.g, x_in, n, g_ng, g_nb);
    }
};

int make_run(Run& r, const char* who, const t2s_tsae* h, int B, int T, float p, uint64_t seed, void* ws, uint64_t ws_bytes, void* stream) {
    TS_TRY(check_train(who, h, B, T, p, ws, ws_bytes));
    r.h = h, r.B = B, r.T = T, r.s = (hipStream_t)stream;
    r.d = Drop{seed, p, 1.0f / (1.0f - p)};
    r.w = carve(h, B, T, (float*)ws);
    return T2S_OK;
}

}  // namespace
}  // namespace t2s

using namespace t2s;
using namespace t2s::tsae;

extern "C" uint64_t t2s_tsae_train_workspace_bytes(const t2s_tsae* h, int B, int T) {
    if (!h || h->n_enc < 1 || h->n_dec < 1 || B < 1 || B > 65535 || T < 1 || T > TR_MAXT) {
        set_error("t2s_tsae_train_workspace_bytes: handle NULL or one-sided, B=%d (1..65535) or T=%d (1..%d) out of range", B, T, TR_MAXT);
        return 0;
    }
    return (uint64_t)carve(h, B, T, nullptr).floats * sizeof(float);
}

extern "C" int t2s_tsae_train_forward(const t2s_tsae* h, const float* x, float* prediction, int B, int T, float p_drop, uint64_t seed,
                                      void* workspace, uint64_t workspace_bytes, void* stream) {
    Run r;
    TS_TRY(make_run(r, "t2s_tsae_train_forward", h, B, T, p_drop, seed, workspace, workspace_bytes, stream));
    T2S_REQUIRE(x != nullptr && prediction != nullptr, "t2s_tsae_train_forward: NULL tensor");
    const TrainWs& w = r.w;
    const size_t rows = (size_t)B * T;
    const Norm none{nullptr, nullptr};
    tsae_train_embed_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, r.s>>>(x, w.xe[0], h->emb, h->emb_ln, h->dec.pe, h->F, T, rows, 0, r.d);
    T2S_LAUNCH_CHECK();
    for (int l = 0; l < h->n_enc; ++l) {
        const EncLayerP& L = h->enc[l];
        TS_TRY(r.rows(w.xe[l], TS_D, TS_D, L.n1, SITE_NONE, L.qkv.w, L.qkv.b, 3 * TS_D, 3 * TS_D, 0, SITE_NONE, nullptr, w.qkve[l], 3 * TS_D));
        TS_TRY(r.attn(w.qkve[l], 3 * TS_D, w.qkve[l] + TS_D, w.qkve[l] + 2 * TS_D, 3 * TS_D, w.atte[l], w.lsee[l], 0, enc_site(l, 0)));
        TS_TRY(r.rows(w.atte[l], TS_D, TS_D, none, SITE_NONE, L.out.w, L.out.b, TS_D, TS_D, 0, enc_site(l, 1), w.xe[l], w.x1e[l], TS_D));
        TS_TRY(r.ffn(w.x1e[l], w.he[l], w.xe[l + 1], L.l1, L.l2, L.n2, enc_site(l, 2), enc_site(l, 3)));
    }
    const float* memory = w.xe[h->n_enc];
    tsae_train_embed_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, r.s>>>(x, w.xd[0], h->dec.inp, none, h->dec.pe, h->F, T, rows, 1, r.d);
    T2S_LAUNCH_CHECK();
    for (int l = 0; l < h->n_dec; ++l) {
        const DecLayerP& L = h->dec.L[l];
        TS_TRY(r.rows(w.xd[l], TS_D, TS_D, L.n1, SITE_NONE, L.qkv.w, L.qkv.b, 3 * TS_D, 3 * TS_D, 0, SITE_NONE, nullptr, w.qkvd[l], 3 * TS_D));
        TS_TRY(r.attn(w.qkvd[l], 3 * TS_D, w.qkvd[l] + TS_D, w.qkvd[l] + 2 * TS_D, 3 * TS_D, w.attd[l], w.lsed[l], 1, dec_site(l, 0)));
        TS_TRY(r.rows(w.attd[l], TS_D, TS_D, none, SITE_NONE, L.out.w, L.out.b, TS_D, TS_D, 0, dec_site(l, 1), w.xd[l], w.x1d[l], TS_D));
        TS_TRY(r.rows(w.x1d[l], TS_D, TS_D, L.n2, SITE_NONE, L.cq.w, L.cq.b, TS_D, TS_D, 0, SITE_NONE, nullptr, w.cq[l], TS_D));
        TS_TRY(r.rows(memory, TS_D, TS_D, none, SITE_NONE, L.ckv.w, L.ckv.b, 2 * TS_D, 2 * TS_D, 0, SITE_NONE, nullptr, w.ckv[l], 2 * TS_D));
        TS_TRY(r.attn(w.cq[l], TS_D, w.ckv[l], w.ckv[l] + TS_D, 2 * TS_D, w.att2[l], w.lse2[l], 0, dec_site(l, 2)));
        TS_TRY(r.rows(w.att2[l], TS_D, TS_D, none, SITE_NONE, L.cout.w, L.cout.b, TS_D, TS_D, 0, dec_site(l, 3), w.x1d[l], w.x2d[l], TS_D));
        TS_TRY(r.ffn(w.x2d[l], w.hd[l], w.xd[l + 1], L.l1, L.l2, L.n3, dec_site(l, 4), dec_site(l, 5)));
    }
    return r.rows(w.xd[h->n_dec], TS_D, TS_D, none, SITE_NONE, h->dec.outp.w, h->dec.outp.b, 32, h->F, 0, SITE_NONE, nullptr, prediction, h->F);
}

extern "C" int t2s_tsae_train_backward(const t2s_tsae* h, const float* x, const float* d_prediction, const t2s_tsae_grads* g, int B, int T,
                                       float p_drop, uint64_t seed, void* workspace, uint64_t workspace_bytes, void* stream) {
    Run r;
    TS_TRY(make_run(r, "t2s_tsae_train_backward", h, B, T, p_drop, seed, workspace, workspace_bytes, stream));
    T2S_REQUIRE(x != nullptr && d_prediction != nullptr && g != nullptr, "t2s_tsae_train_backward: NULL tensor");
    for (const PackItem& it : h->items)   // the items name exactly the tensors that take part
        T2S_REQUIRE(*(const float* const*)((const char*)g + it.w_field) != nullptr && *(const float* const*)((const char*)g + it.b_field) != nullptr,
                    "t2s_tsae_train_backward: a gradient pointer is NULL (pointer at byte %u / %u of t2s_tsae_grads)", it.w_field, it.b_field);
    const TrainWs& w = r.w;
    const int F = h->F;
    const Norm none{nullptr, nullptr};
    // output projection
    TS_TRY(r.dw(d_prediction, F, F, SITE_NONE, w.xd[h->n_dec], TS_D, TS_D, none, SITE_NONE, (float*)g->output_projection_w,
                (float*)g->output_projection_b));
    TS_TRY(r.back(d_prediction, F, 32, F, SITE_NONE, h->dec.outp.t, TS_D, nullptr, SITE_NONE, nullptr, w.g));
    for (int l = h->n_dec - 1; l >= 0; --l) {
        const DecLayerP& L = h->dec.L[l];
        const t2s_tsae_dec_layer& G = g->dec[l];
        TS_TRY(r.ffn_bwd(w.x2d[l], w.hd[l], L.l1, L.l2, L.n3, dec_site(l, 4), dec_site(l, 5), (float*)G.linear1_w, (float*)G.linear1_b,
                         (float*)G.linear2_w, (float*)G.linear2_b, (float*)G.norm3_w, (float*)G.norm3_b));
        // cross-attention: queries from LayerNorm2(x1), keys / values from the memory
        TS_TRY(r.out_proj_bwd(w.att2[l], L.cout, dec_site(l, 3), (float*)G.multihead_attn.out_proj_w, (float*)G.multihead_attn.out_proj_b));
        float* dcq = w.dqkv;
        float* dckv = w.dqkv + (size_t)B * T * TS_D;
        TS_TRY(r.attn_bwd(w.cq[l], TS_D, w.ckv[l], w.ckv[l] + TS_D, 2 * TS_D, w.att2[l], w.datt, w.lse2[l], dcq, TS_D, dckv, dckv + TS_D,
                          2 * TS_D, 0, dec_site(l, 2)));
        float* gin_w = (float*)G.multihead_attn.in_proj_w;
        float* gin_b = (float*)G.multihead_attn.in_proj_b;
        TS_TRY(r.dw(dcq, TS_D, TS_D, SITE_NONE, w.x1d[l], TS_D, TS_D, L.n2, SITE_NONE, gin_w, gin_b));
        TS_TRY(r.dw(dckv, 2 * TS_D, 2 * TS_D, SITE_NONE, w.xe[h->n_enc], TS_D, TS_D, none, SITE_NONE, gin_w + TS_D * TS_D, gin_b + TS_D));
        TS_TRY(r.back(dckv, 2 * TS_D, 2 * TS_D, 2 * TS_D, SITE_NONE, L.ckv.t, TS_D, nullptr, SITE_NONE, l == h->n_dec - 1 ? nullptr : w.dmem,
                      w.dmem));
        TS_TRY(r.back(dcq, TS_D, TS_D, TS_D, SITE_NONE, L.cq.t, TS_D, nullptr, SITE_NONE, nullptr, w.g, w.x1d[l], L.n2, (float*)G.norm2_w,
                      (float*)G.norm2_b));
        TS_TRY(r.self_bwd(w.xd[l], w.qkvd[l], w.lsed[l], w.attd[l], L.qkv, L.out, L.n1, 1, dec_site(l, 0), dec_site(l, 1), G.self_attn,
                          (float*)G.norm1_w, (float*)G.norm1_b));
    }
    // the shifted input projection (no gradient flows to x itself)
    tsae_train_embed_bwd_kernel<<<r.tiles(), 256, 0, r.s>>>(x, w.g, w.datt, h->dec.inp, none, w.pln, F, T, 1, r.d);
    T2S_LAUNCH_CHECK();
    TS_TRY(r.dw(w.datt, TS_D, TS_D, SITE_NONE, x, F, F, none, SITE_NONE, (float*)g->input_projection_w, (float*)g->input_projection_b));
    // the encoder, from the memory's gradient
    Run e = r;
    e.w.g = w.dmem;
    for (int l = h->n_enc - 1; l >= 0; --l) {
        const EncLayerP& L = h->enc[l];
        const t2s_tsae_enc_layer& G = g->enc[l];
        TS_TRY(e.ffn_bwd(w.x1e[l], w.he[l], L.l1, L.l2, L.n2, enc_site(l, 2), enc_site(l, 3), (float*)G.linear1_w, (float*)G.linear1_b,
                         (float*)G.linear2_w, (float*)G.linear2_b, (float*)G.norm2_w, (float*)G.norm2_b));
        TS_TRY(e.self_bwd(w.xe[l], w.qkve[l], w.lsee[l], w.atte[l], L.qkv, L.out, L.n1, 0, enc_site(l, 0), enc_site(l, 1), G.self_attn,
                          (float*)G.norm1_w, (float*)G.norm1_b));
    }
    tsae_train_embed_bwd_kernel<<<r.tiles(), 256, 0, r.s>>>(x, e.w.g, w.datt, h->emb, h->emb_ln, w.pln, F, T, 0, r.d);
    T2S_LAUNCH_CHECK();
    TS_TRY(r.norm_grads((float*)g->embedding_ln_w, (float*)g->embedding_ln_b));
    return r.dw(w.datt, TS_D, TS_D, SITE_NONE, x, F, F, none, SITE_NONE, (float*)g->value_embedding_w, (float*)g->value_embedding_b);
}
