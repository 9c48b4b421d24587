// LA-VAE codec (reference model/pretrained/vqvae.py:36-105) for MI355X.
//
// The codec runs once per batch (15-17 MFLOP per series against 1.95 TFLOP for the
// 1000-step loop), so it is a single launch with ONE workgroup per series and time tile: the
// activation stack of a tile (<= 256 channels x <= 32 positions at the L/4 resolution) stays in
// LDS from the latent to the decoded samples, weights (2.7 MB fp32) stream from L2.  Exact fp32 VALU.
// L <= 128 (BASELINE configs: 24 / 48 / 96) is one tile = the whole series.  Longer series (vqvae.py accepts any L;
// the reference's SUSHI set is 2048 long) are cut into tiles of 32 - 2 H core positions with a halo of H = the
// convolutions' receptive radius on either side, recomputed per tile: every kept value sums the same terms in the
// same order as the untiled computation, so the tiling is invisible in the results.
// One kernel per direction (vae_encode_kernel, vae_decode_kernel) serves the single-channel codec (vqvae.py) and the C-channel
// motion codec (myvqvae.py); vae_interp_rows_kernel finishes a tiled encode; the two backward kernels recompute the forward
// through the forward's own __device__ pieces (encode_stem, stage_latent, interp_linear_ac, the convolutions).
#include "t2s_arena.h"
#include "t2s_wgrad.h"

namespace t2s {

constexpr int VAE_TMAX = 32;   // positions after the stride-4 stem: L/4 <= 32  (L <= 128)
constexpr int VAE_CMAX = 256;  // res_hidden
constexpr int VAE_THREADS = 256;
constexpr int VAE_CO_PER_THREAD = 8;   // output channels per thread in conv1d_lds

struct VaeDev {  // device copies in the reference layouts
    int hidden, res_hidden, n_res, emb;
    const float *dec_conv1_w, *dec_conv1_b, *dec_ct1_w, *dec_ct1_b, *dec_ct2_w, *dec_ct2_b;
    const float *dec_c3[4], *dec_c1[4];
    const float *enc_conv1_w, *enc_conv1_b, *enc_conv2_w, *enc_conv2_b, *enc_conv3_w, *enc_conv3_b;
    const float *enc_c3[4], *enc_c1[4];
    const float *enc_prevq_w, *enc_prevq_b;
};

// out[co][t] (+)= b[co] + sum_{ci,kk} W[co][ci][kk] * in[ci][t*STRIDE + kk - pad]   (Conv1d)
// Buffers are LDS, row stride `ld`.  RELU_OUT applies to the final value; ACCUM adds into out.
// Windows: `in` holds global positions [in_g0, in_g0 + Tin), `out` global positions [out_g0, out_g0 + Tout); both are
// clipped to the series, so "outside the input window" is either true zero padding or a position whose influence
// stays inside the discarded halo.
template <int KS, int STRIDE, bool RELU_OUT, bool ACCUM>
__device__ void conv1d_lds(const float* in, int Cin, int Tin, float* out, int Cout, int Tout,
                           const float* __restrict__ W, const float* __restrict__ bias, int pad,
                           int ld_in, int ld_out, int in_g0 = 0, int out_g0 = 0) {
    // VAE_CO_PER_THREAD (8; measured 2: 21.3, 4: 19.1, 8: 17.9, 16: 17.8 ms per uncached bf16 train step) output channels per thread: the LDS activations are read once for four FMAs and four independent
    // accumulation chains are in flight (one chain per thread was latency-bound at 1.6 TFLOP/s); each output
    // still sums its (ci, kk) terms in the same order.  Cout is a multiple of 4 for every LA-VAE layer but the last.
    constexpr int CP = VAE_CO_PER_THREAD;
    if (Cout % CP == 0) {
        for (int o = threadIdx.x; o < (Cout / CP) * Tout; o += VAE_THREADS) {
            const int co = (o / Tout) * CP, t = o - (o / Tout) * Tout;
            float acc[CP];
#pragma unroll
            for (int u = 0; u < CP; ++u) acc[u] = bias ? bias[co + u] : 0.f;
            const float* w = W + (size_t)co * Cin * KS;
            const size_t ws = (size_t)Cin * KS;
#pragma unroll 2
            for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const int ti = (out_g0 + t) * STRIDE + kk - pad - in_g0;
                    if (ti >= 0 && ti < Tin) {
                        const float a = in[ci * ld_in + ti];
#pragma unroll
                        for (int u = 0; u < CP; ++u) acc[u] += w[u * ws + ci * KS + kk] * a;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < CP; ++u) {
                float r = acc[u];
                if (ACCUM) r += out[(co + u) * ld_out + t];
                if (RELU_OUT) r = fmaxf(r, 0.f);
                out[(co + u) * ld_out + t] = r;
            }
        }
        return;
    }
    for (int o = threadIdx.x; o < Cout * Tout; o += VAE_THREADS) {
        const int co = o / Tout, t = o - co * Tout;
        float acc = bias ? bias[co] : 0.f;
        const float* w = W + (size_t)co * Cin * KS;
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int ti = (out_g0 + t) * STRIDE + kk - pad - in_g0;
                if (ti >= 0 && ti < Tin) acc += w[ci * KS + kk] * in[ci * ld_in + ti];
            }
        }
        if (ACCUM) acc += out[co * ld_out + t];
        if (RELU_OUT) acc = fmaxf(acc, 0.f);
        out[co * ld_out + t] = acc;
    }
}

// ConvTranspose1d(k=4, stride=2, padding=1): W is (Cin, Cout, 4);
// out[co][t] = b[co] + sum_{ci,kk : t = 2 i - 1 + kk} in[ci][i] * W[ci][co][kk]
template <bool RELU_OUT>
__device__ void convT1d_k4s2_lds(const float* in, int Cin, int Tin, float* out, int Cout,
                                 const float* __restrict__ W, const float* __restrict__ bias,
                                 int ld_in, int ld_out) {
    const int Tout = 2 * Tin;
    for (int o = threadIdx.x; o < Cout * Tout; o += VAE_THREADS) {
        const int co = o / Tout, t = o - co * Tout;
        float acc = bias[co];
        // t+1-kk even  ->  kk has the parity of t+1
        const int k0 = (t + 1) & 1;
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
            for (int kk2 = 0; kk2 < 2; ++kk2) {
                const int kk = k0 + 2 * kk2;
                const int i = (t + 1 - kk) >> 1;
                if (t + 1 - kk >= 0 && i < Tin) acc += in[ci * ld_in + i] * W[((size_t)ci * Cout + co) * 4 + kk];
            }
        }
        if (RELU_OUT) acc = fmaxf(acc, 0.f);
        out[co * ld_out + t] = acc;
    }
}

// F.interpolate(mode='linear', align_corners=True) along the last axis maps Tin positions to Tout: output position t reads
// l0 * in[i0] + l1 * in[i1].  The ONE copy of that index arithmetic and of its rounding, shared by every forward site and the
// transpose.  The rounding sequence is the one of torch's CPU kernel, every named value rounded once:
//   real = scale * t;  l1 = real - (float)i0;  l0 = 1 - l1;  out = fma(l0, in[i0], round(l1 * in[i1]))
// so an interpolated value is torch's bit for bit, whichever loop iteration, tile or kernel computes it.  What pins it is
// `#pragma clang fp contract(off)` in the two bodies plus the one explicit fma: left to the compiler, `real - i0` fuses with the
// product in front of it in some iterations of a loop and not in others, and __fmul_rn / __fsub_rn do not stop that here.
struct InterpTap { int i0, i1; float l0, l1; };
__device__ inline float interp_scale_ac(int Tin, int Tout) { return Tout > 1 ? (float)(Tin - 1) / (float)(Tout - 1) : 0.f; }
__device__ inline InterpTap interp_tap_ac(float scale, int t, int Tin) {
#pragma clang fp contract(off)
    InterpTap p;
    const float real = scale * (float)t;
    p.i0 = (int)real;
    p.i1 = p.i0 + (p.i0 < Tin - 1 ? 1 : 0);
    p.l1 = real - (float)p.i0;
    p.l0 = 1.0f - p.l1;
    return p;
}
// the interpolated value from the two samples a0 = in[p.i0], a1 = in[p.i1]
__device__ inline float interp_apply(const InterpTap& p, float a0, float a1) {
#pragma clang fp contract(off)
    const float hi = p.l1 * a1;
    return __builtin_fmaf(p.l0, a0, hi);
}

// [C][Tin] -> [C][Tout] (`out` holds the global output positions [out_g0, out_g0 + Tw) of Tout)
__device__ void interp_linear_ac(const float* in, int C, int Tin, int ld_in, float* out, int Tout,
                                 int ld_out, int out_g0 = 0, int Tw = -1) {
    const float scale = interp_scale_ac(Tin, Tout);
    if (Tw < 0) Tw = Tout;
    for (int o = threadIdx.x; o < C * Tw; o += VAE_THREADS) {
        const int c = o / Tw, t = o - c * Tw;
        const InterpTap p = interp_tap_ac(scale, out_g0 + t, Tin);
        out[c * ld_out + t] = interp_apply(p, in[c * ld_in + p.i0], in[c * ld_in + p.i1]);
    }
}

// The transpose of interp_linear_ac: the forward maps Tin to Tout; this gathers the Tout gradients into Tin,
//   out[c][i] = (INIT ? init[c][i] : 0) + sum over t = 0 .. Tout - 1 of { l0(t) d[c][t] if i0(t) == i } + { l1(t) d[c][t] if i1(t) == i },
//   d[c][t] = g[c][t] (+ add[c][t] if ADD).
// Operands may live in LDS or global memory, each with its own row stride.  INIT and ADD are compile-time: an absent operand
// costs no floating-point operation, so every instantiation keeps one fixed expression (a run-time "+ 0" would not be the
// same bits as no addition for a negative zero).
template <bool INIT, bool ADD>
__device__ void interp_linear_ac_transposed(const float* g, int ld_g, const float* add, int ld_add, const float* init, int ld_init,
                                            float* out, int ld_out, int C, int Tin, int Tout) {
    const float scale = interp_scale_ac(Tin, Tout);
    for (int o = threadIdx.x; o < C * Tin; o += VAE_THREADS) {
        const int c = o / Tin, i = o - c * Tin;
        float acc = INIT ? init[c * ld_init + i] : 0.f;
        for (int t = 0; t < Tout; ++t) {
            const InterpTap p = interp_tap_ac(scale, t, Tin);
            float d = g[c * ld_g + t];
            if (ADD) d += add[c * ld_add + t];
            if (p.i0 == i) acc += p.l0 * d;
            if (p.i1 == i) acc += p.l1 * d;
        }
        out[c * ld_out + i] = acc;
    }
}

__device__ void relu_inplace(float* x, int C, int T, int ld) {
    for (int o = threadIdx.x; o < C * T; o += VAE_THREADS) {
        const int c = o / T, t = o - c * T;
        x[c * ld + t] = fmaxf(x[c * ld + t], 0.f);
    }
}

// ResidualStack (vqvae.py:7-33).  nn.ReLU(True) mutates the block input in place, so the skip
// path carries relu(x): x <- relu(x); x <- x + conv1x1(relu(conv3(x))); finally relu(x).
__device__ void residual_stack(float* x, float* tmp, int hidden, int res_hidden, int n_res, int T,
                               const float* const* c3, const float* const* c1, int ld) {
    for (int l = 0; l < n_res; ++l) {
        relu_inplace(x, hidden, T, ld);
        __syncthreads();
        conv1d_lds<3, 1, true, false>(x, hidden, T, tmp, res_hidden, T, c3[l], nullptr, 1, ld, ld);
        __syncthreads();
        conv1d_lds<1, 1, false, true>(tmp, res_hidden, T, x, hidden, T, c1[l], nullptr, 0, ld, ld);
        __syncthreads();
    }
    relu_inplace(x, hidden, T, ld);
    __syncthreads();
}

constexpr int LD = VAE_TMAX + 1;  // LDS row stride (floats)
constexpr int VAE_WIDE_T = 2 * VAE_TMAX + 2;   // positions at the L/2 resolution a tile's stride-2 convolutions touch
constexpr int VAE_LDS_FLOATS = 2 * VAE_CMAX * LD + 128 * 4 + 64 * VAE_WIDE_T;

// Time tiling at the L/4 resolution: tile `ti` keeps core positions [c0, c1) and computes the window [w0, w1) =
// core +- halo, clipped to [0, T).  One tile (T <= 32): the window is the series.
struct VaeTile {
    int c0, c1, w0, w1;
};
__host__ __device__ inline int vae_core(int T, int halo) { return T <= VAE_TMAX ? T : VAE_TMAX - 2 * halo; }
__host__ __device__ inline int vae_tiles(int T, int halo) { const int c = vae_core(T, halo); return (T + c - 1) / c; }
__device__ inline VaeTile vae_tile(int T, int halo, int ti) {
    const int core = vae_core(T, halo);
    VaeTile v;
    v.c0 = ti * core;
    v.c1 = v.c0 + core < T ? v.c0 + core : T;
    v.w0 = v.c0 - halo > 0 ? v.c0 - halo : 0;
    v.w1 = v.c1 + halo < T ? v.c1 + halo : T;
    return v;
}

// ------------------------------------------------------------------------------------------------ forward
// One codec, C channels.  The single-channel LA-VAE (vqvae.py:36-105) is C = 1 with L % 4 == 0 and a latent W <= 32 wide
// (30 on the DiT path, L/4 on the MLP-denoiser path); the T2MS motion codec (reference model/pretrained/myvqvae.py:32-86) is
// the same kernels at C channels -- _conv_1 reads C channels, _conv_trans_2 writes C -- with a latent up to 64 wide
// (flow_dim) and ANY length L >= 8: the stride-2 convolutions give L/2 and L/4 positions (floor; the last taps of an odd length
// are real samples), the decoder builds 4 T samples (T = L/4) and resamples them to L (myvqvae.py:85; the identity, skipped,
// when L % 4 == 0).  The channel count is a run-time argument: one instantiation, no atomics, exact fp32.
constexpr int VAE_MC_CMAX = 16;          // series channels
constexpr int VAE_MC_WMAX = 64;          // latent width
constexpr int LDZ = VAE_MC_WMAX + 1;     // LDS row stride of a staged latent wider than VAE_TMAX: 64 x 65 floats fit in bufB
constexpr int LDY = 4 * VAE_TMAX + 1;    // LDS row stride of a tile's samples in front of the final resampling
static_assert(T2S_LAT_C * LDZ <= VAE_CMAX * LD && VAE_MC_CMAX * LDY <= VAE_CMAX * LD, "staging rows exceed an LDS buffer");

// Encoder conv_1 (C -> hidden/2, k4 s2 p1, ReLU) of one series x (C, L), straight from global: the outputs at the
// L/2-resolution positions [u0, u1) -> wide [hidden/2][u1 - u0].  Output t reads x[2t-1 .. 2t+2] clipped to [0, L).
__device__ void encode_stem(const VaeDev& w, const float* __restrict__ x, int C, int L, int u0, int u1, float* wide) {
    const int Tu = u1 - u0;
    for (int o = threadIdx.x; o < (w.hidden / 2) * Tu; o += VAE_THREADS) {
        const int co = o / Tu, t = u0 + (o - co * Tu);
        float acc = w.enc_conv1_b[co];
        for (int ci = 0; ci < C; ++ci) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ti = 2 * t + kk - 1;
                if (ti >= 0 && ti < L) acc += w.enc_conv1_w[(co * C + ci) * 4 + kk] * x[(size_t)ci * L + ti];
            }
        }
        wide[co * Tu + (t - u0)] = fmaxf(acc, 0.f);
    }
}

// the latent z (emb, W) of one series -> buf[emb][ld]
__device__ void stage_latent(const float* __restrict__ z, int E, int W, float* buf, int ld) {
    for (int o = threadIdx.x; o < E * W; o += VAE_THREADS) {
        const int c = o / W, t = o - c * W;
        buf[c * ld + t] = z[o];
    }
}

// One sample of the decoder's last transposed convolution (hidden/2 -> C, k4 s2 p1): channel co at position t, from `wide`
// = the first transposed convolution's outputs at the L/2-resolution positions [i_g0, i_g0 + Tin), row stride ldw.
__device__ inline float decode_last_sample(const VaeDev& w, const float* wide, int ldw, int Tin, int i_g0, int C, int co, int t) {
    float acc = w.dec_ct2_b[co];
    const int k0 = (t + 1) & 1;      // t+1-kk even  ->  kk has the parity of t+1
    for (int ci = 0; ci < w.hidden / 2; ++ci) {
#pragma unroll
        for (int kk2 = 0; kk2 < 2; ++kk2) {
            const int kk = k0 + 2 * kk2;
            const int i = ((t + 1 - kk) >> 1) - i_g0;
            if (t + 1 - kk >= 0 && i >= 0 && i < Tin) acc += wide[ci * ldw + i] * w.dec_ct2_w[((size_t)ci * C + co) * 4 + kk];
        }
    }
    return acc;
}

// Decoder.forward (vqvae.py:97-105, myvqvae.py:76-86).  Receptive radius at the L/4 resolution: conv_1 1 + residual stack n_res
// + the two transposed convolutions 1 (the second one reads half a position beyond the first's window) = n_res + 2.
// The final resampling 4 T -> L: output position t reads samples i0(t) and i0(t) + 1; a tile owns the outputs whose i0 falls in
// its core [4 c0, 4 c1), and the one sample beyond, 4 c1, lies inside its halo window (it reads the same
// first-transposed-convolution outputs as the core sample 4 c1 - 1).  i0 is monotone in t, so every output has exactly one owner.
// The body works on ONE series -- z (emb, W), recon (C, L), after (emb, L/4) or NULL are that series' own rows -- and one time
// tile `ti` of it; the uniform and the ragged kernel below differ only in where a workgroup finds its rows and its L.
__device__ __forceinline__ void vae_decode_series(const VaeDev& w, const float* __restrict__ z, float* __restrict__ recon,
                                                  float* __restrict__ after, int L, int W, int C, int ti) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bufA = smem;                   // [<=256][LD]
    float* bufB = smem + VAE_CMAX * LD;   // [<=256][LD]
    float* wide = bufB + VAE_CMAX * LD;   // [hidden/2][2 Tw] for the first transposed conv
    const int T = L / 4, L4 = 4 * T;
    const VaeTile tl = vae_tile(T, w.n_res + 2, ti);
    const int Tw = tl.w1 - tl.w0;
    const int ldz = W <= VAE_TMAX ? LD : LDZ;
    stage_latent(z, w.emb, W, bufB, ldz);
    __syncthreads();
    interp_linear_ac(bufB, w.emb, W, ldz, bufA, T, LD, tl.w0, Tw);
    __syncthreads();
    if (after) {
        const int nc = tl.c1 - tl.c0;
        for (int o = threadIdx.x; o < w.emb * nc; o += VAE_THREADS) {
            const int c = o / nc, t = tl.c0 + (o - c * nc);
            after[(size_t)c * T + t] = bufA[c * LD + (t - tl.w0)];
        }
    }
    conv1d_lds<3, 1, false, false>(bufA, w.emb, Tw, bufB, w.hidden, Tw, w.dec_conv1_w, w.dec_conv1_b, 1, LD, LD);
    __syncthreads();
    residual_stack(bufB, bufA, w.hidden, w.res_hidden, w.n_res, Tw, w.dec_c3, w.dec_c1, LD);
    const int ldw = 2 * Tw;      // `wide` holds L/2-resolution positions [2 w0, 2 w1)
    convT1d_k4s2_lds<true>(bufB, w.hidden, Tw, wide, w.hidden / 2, w.dec_ct1_w, w.dec_ct1_b, LD, ldw);
    __syncthreads();
    // last transposed conv (hidden/2 -> C): the samples [y0, y1) go straight to global when L = 4 T, else to bufA [C][LDY]
    const bool resample = L != L4;
    const int y0 = 4 * tl.c0, yc = 4 * tl.c1;
    const int y1 = resample && yc < L4 ? yc + 1 : yc, Ty = y1 - y0;
    for (int o = threadIdx.x; o < C * Ty; o += VAE_THREADS) {
        const int co = o / Ty, t = y0 + (o - co * Ty);
        const float acc = decode_last_sample(w, wide, ldw, 2 * Tw, 2 * tl.w0, C, co, t);
        if (resample) bufA[co * LDY + (t - y0)] = acc;
        else recon[(size_t)co * L + t] = acc;
    }
    if (!resample) return;
    __syncthreads();
    // candidates: every t whose i0 = floor(scale * t) can fall in [y0, yc), two positions of slack for the fp32 division;
    // the ownership test itself is the tap's own arithmetic
    const float scale = interp_scale_ac(L4, L);
    int ta = (int)((float)y0 / scale) - 2, tb = (int)((float)yc / scale) + 3;
    ta = ta > 0 ? ta : 0;
    tb = tb < L ? tb : L;
    const int nt = tb - ta;
    for (int o = threadIdx.x; o < C * nt; o += VAE_THREADS) {
        const int co = o / nt, t = ta + (o - co * nt);
        const InterpTap p = interp_tap_ac(scale, t, L4);
        if (p.i0 < y0 || p.i0 >= yc) continue;
        recon[(size_t)co * L + t] = interp_apply(p, bufA[co * LDY + (p.i0 - y0)], bufA[co * LDY + (p.i1 - y0)]);
    }
}

__global__ __launch_bounds__(VAE_THREADS) void vae_decode_kernel(const VaeDev w, const float* __restrict__ z,
                                                                 float* __restrict__ recon, float* __restrict__ after,
                                                                 int L, int W, int C) {
    const size_t b = blockIdx.x;
    vae_decode_series(w, z + b * w.emb * W, recon + b * C * L, after ? after + b * w.emb * (L / 4) : nullptr, L, W, C, blockIdx.y);
}

// Ragged rows: series b has its own length lengths[b] and lies packed at channels * offsets[b] (offsets = the prefix sums of
// lengths, B + 1 entries).  A row is SKIPPED -- no read of z, no write -- unless 8 <= L_b <= max_L and offsets[b + 1] -
// offsets[b] == L_b (so a row never leaves the span its own offsets give it; L_b == 0 is the empty row), and a workgroup whose
// tile index is past its row's tile count (the grid is sized for max_L) returns: both before any barrier.
__device__ inline int vae_ragged_length(const int32_t* __restrict__ lengths, const uint64_t* __restrict__ offsets, int b, int max_L) {
    const int L = lengths[b];
    return (L >= 8 && L <= max_L && offsets[b + 1] - offsets[b] == (uint64_t)L) ? L : 0;
}

__global__ __launch_bounds__(VAE_THREADS) void vae_decode_ragged_kernel(const VaeDev w, const float* __restrict__ z,
                                                                        const int32_t* __restrict__ lengths,
                                                                        const uint64_t* __restrict__ offsets,
                                                                        float* __restrict__ recon, int max_L, int W, int C) {
    const int b = blockIdx.x;
    const int L = vae_ragged_length(lengths, offsets, b, max_L);
    if (L == 0 || (int)blockIdx.y >= vae_tiles(L / 4, w.n_res + 2)) return;
    vae_decode_series(w, z + (size_t)b * w.emb * W, recon + (size_t)C * offsets[b], nullptr, L, W, C, blockIdx.y);
}

// Encoder.forward (vqvae.py:57-71, myvqvae.py:49-61).  Receptive radius at the L/4 resolution behind conv_2: conv_3 1 + residual
// stack n_res.  The final interpolation to W positions needs the WHOLE `before` row: fused here when the series is one tile,
// otherwise vae_interp_rows_kernel reads the rows the tiles wrote.
// One series and one time tile `ti` of it, as vae_decode_series: x (C, L), z (emb, W), before (emb, L/4) or NULL are the
// series' own rows.
__device__ __forceinline__ void vae_encode_series(const VaeDev& w, const float* __restrict__ x, float* __restrict__ z,
                                                  float* __restrict__ before, int L, int W, int C, int ti) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bufA = smem;
    float* bufB = smem + VAE_CMAX * LD;
    float* wide = bufB + VAE_CMAX * LD;   // [hidden/2][Tu]: conv_1 outputs at L/2-resolution positions [u0, u1)
    const int T2 = L / 2, T = L / 4;
    const int half_c = w.hidden / 2;
    const VaeTile tl = vae_tile(T, w.n_res + 1, ti);
    const int Tw = tl.w1 - tl.w0;
    // conv_2 (k4 s2 p1) output t reads conv_1 outputs 2t-1 .. 2t+2
    const int u0 = 2 * tl.w0 - 1 > 0 ? 2 * tl.w0 - 1 : 0;
    const int u1 = 2 * (tl.w1 - 1) + 3 < T2 ? 2 * (tl.w1 - 1) + 3 : T2;
    const int Tu = u1 - u0;
    encode_stem(w, x, C, L, u0, u1, wide);
    __syncthreads();
    conv1d_lds<4, 2, true, false>(wide, half_c, Tu, bufA, w.hidden, Tw, w.enc_conv2_w, w.enc_conv2_b, 1, Tu, LD, u0, tl.w0);
    __syncthreads();
    conv1d_lds<3, 1, false, false>(bufA, w.hidden, Tw, bufB, w.hidden, Tw, w.enc_conv3_w, w.enc_conv3_b, 1, LD, LD);
    __syncthreads();
    residual_stack(bufB, bufA, w.hidden, w.res_hidden, w.n_res, Tw, w.enc_c3, w.enc_c1, LD);
    conv1d_lds<1, 1, false, false>(bufB, w.hidden, Tw, bufA, w.emb, Tw, w.enc_prevq_w, w.enc_prevq_b, 0, LD, LD);
    __syncthreads();
    if (before) {
        const int nc = tl.c1 - tl.c0;
        for (int o = threadIdx.x; o < w.emb * nc; o += VAE_THREADS) {
            const int c = o / nc, t = tl.c0 + (o - c * nc);
            before[(size_t)c * T + t] = bufA[c * LD + (t - tl.w0)];
        }
    }
    if (T > VAE_TMAX) return;             // tiled: the interpolation kernel finishes from `before`
    const float scale = interp_scale_ac(T, W);
    for (int o = threadIdx.x; o < w.emb * W; o += VAE_THREADS) {
        const int c = o / W, t = o - c * W;
        const InterpTap p = interp_tap_ac(scale, t, T);
        z[o] = interp_apply(p, bufA[c * LD + p.i0], bufA[c * LD + p.i1]);
    }
}

__global__ __launch_bounds__(VAE_THREADS) void vae_encode_kernel(const VaeDev w, const float* __restrict__ x,
                                                                 float* __restrict__ z, float* __restrict__ before,
                                                                 int L, int W, int C) {
    const size_t b = blockIdx.x;
    vae_encode_series(w, x + b * C * L, z + b * w.emb * W, before ? before + b * w.emb * (L / 4) : nullptr, L, W, C, blockIdx.y);
}

// Ragged rows, as vae_decode_ragged_kernel; `before` rows are packed (emb, L_b / 4) at emb * offsets4[b] (offsets4 = the prefix
// sums of L_b / 4), and a row whose offsets4 span is not L_b / 4 is skipped too.
__device__ inline int vae_ragged_length4(const int32_t* __restrict__ lengths, const uint64_t* __restrict__ offsets,
                                         const uint64_t* __restrict__ offsets4, int b, int max_L) {
    const int L = vae_ragged_length(lengths, offsets, b, max_L);
    return (L != 0 && offsets4[b + 1] - offsets4[b] == (uint64_t)(L / 4)) ? L : 0;
}

__global__ __launch_bounds__(VAE_THREADS) void vae_encode_ragged_kernel(const VaeDev w, const float* __restrict__ x,
                                                                        const int32_t* __restrict__ lengths,
                                                                        const uint64_t* __restrict__ offsets,
                                                                        const uint64_t* __restrict__ offsets4, float* __restrict__ z,
                                                                        float* __restrict__ before, int max_L, int W, int C) {
    const int b = blockIdx.x;
    const int L = vae_ragged_length4(lengths, offsets, offsets4, b, max_L);
    if (L == 0 || (int)blockIdx.y >= vae_tiles(L / 4, w.n_res + 1)) return;
    vae_encode_series(w, x + (size_t)C * offsets[b], z + (size_t)b * w.emb * W, before ? before + (size_t)w.emb * offsets4[b] : nullptr,
                      L, W, C, blockIdx.y);
}

// out (C,Tout) = F.interpolate(in (C,Tin), Tout, mode='linear', align_corners=True) of one series: the latent of a tiled encode
__device__ __forceinline__ void vae_interp_series(const float* __restrict__ src, float* __restrict__ out, int C, int Tin, int Tout) {
    const float scale = interp_scale_ac(Tin, Tout);
    for (int o = threadIdx.x; o < C * Tout; o += VAE_THREADS) {
        const int c = o / Tout, t = o - c * Tout;
        const InterpTap p = interp_tap_ac(scale, t, Tin);
        out[o] = interp_apply(p, src[(size_t)c * Tin + p.i0], src[(size_t)c * Tin + p.i1]);
    }
}

__global__ __launch_bounds__(VAE_THREADS) void vae_interp_rows_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      int C, int Tin, int Tout) {
    vae_interp_series(in + (size_t)blockIdx.x * C * Tin, out + (size_t)blockIdx.x * C * Tout, C, Tin, Tout);
}

// the rows of a ragged encode that ran in time tiles (L_b / 4 > 32); a one-tile row has its latent already
__global__ __launch_bounds__(VAE_THREADS) void vae_interp_rows_ragged_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                             const int32_t* __restrict__ lengths,
                                                                             const uint64_t* __restrict__ offsets,
                                                                             const uint64_t* __restrict__ offsets4, int max_L, int C,
                                                                             int Tout) {
    const int b = blockIdx.x;
    const int L = vae_ragged_length4(lengths, offsets, offsets4, b, max_L);
    if (L / 4 <= VAE_TMAX) return;
    vae_interp_series(in + (size_t)C * offsets4[b], out + (size_t)b * C * Tout, C, L / 4, Tout);
}

// ------------------------------------------------------------------------------------------------ encoder backward
// Backward of Encoder.forward: what trains the encoder (train.py:31-33 with `usepretrainedvae` false, LA-VAE pre-training) and,
// at C channels, the motion codec (myvqvae.py).  One scaffold, as the forward is one codec: the single-channel backward is its
// C = 1 case with L % 4 == 0, L <= 128 and the 30-wide latent.  Both backward kernels are templated on a tile bound TB (the whole
// series is ONE tile of T = L/4 <= TB positions): TB = 32 serves L <= 128 with the geometry the single-channel backward always
// had, TB = 48 serves 128 < L <= 192 (the motion models train at up to 4 x 48) in 139 / 150 KiB of the CU's 160 KiB of LDS.
// Two stages:
//   vae_encode_bwd_kernel   one workgroup per series: the forward is recomputed in LDS by the
//                           functions vae_encode_kernel calls, every layer's INPUT leaves as an im2col'd row block X (rows = b * T
//                           + t) and its ReLU pattern stays as one bit word per channel; then the data gradients walk back
//                           through the layers in LDS (transposed convolutions, fixed summation order) and every layer's
//                           OUTPUT gradient leaves as a row block dY.  conv_1 (C -> hidden/2, 4 taps: 64 (4 C + 1) values) is
//                           reduced per series into one partial row.
//   launch_wgrad32          dW = dY^T X per layer on the exact-fp32 MFMA (t2s_wgrad.h), deterministic two-stage reduction;
//                           vae_part_reduce_kernel adds the conv_1 partial rows in series order.
struct VaeStackBufs {   // per residual layer: the rows of r and m (inputs of c3 / c1), the output gradients of c1 / c3
    float *Xr3[4], *Xm[4], *dYc1[4], *dYc3[4];
};
struct VaeBwdBufs {
    float *Xc2, *Xc3, *Xp, *dYp, *dY3, *dY2, *part1;
    VaeStackBufs st;
};
// The LDS of a backward kernel at tile bound TB: the forward's two activation buffers, slack and `wide` at row stride TB + 1,
// then the ReLU bit words -- WT words per channel for a pattern over T positions, WT2 for one over the L/2 resolution -- and,
// in the decoder, the C x 4 T output-gradient samples (sized per launch).
template <int TB>
struct VaeBwdGeom {
    static constexpr int LD = TB + 1;
    static constexpr int WT = (TB + 31) / 32, WT2 = (2 * TB + 31) / 32;
    static constexpr int FLOATS = 2 * VAE_CMAX * LD + 128 * 4 + 64 * (2 * TB + 2);
    static constexpr int STACK_WORDS = 5 * 128 * WT + 4 * 256 * WT;
    static constexpr int ENC_BYTES = (FLOATS + 64 * WT2 + 128 * WT + STACK_WORDS) * 4;
    static constexpr int DEC_BYTES = (FLOATS + STACK_WORDS + 64 * WT2) * 4;        // + C * 4 T floats
    static constexpr int DEC_BYTES_MAX = DEC_BYTES + VAE_MC_CMAX * 4 * TB * 4;
};
static_assert(VaeBwdGeom<VAE_TMAX>::FLOATS == VAE_LDS_FLOATS, "TB = 32 is the forward's geometry");
static_assert(VaeBwdGeom<48>::ENC_BYTES <= 160 * 1024 && VaeBwdGeom<48>::DEC_BYTES_MAX <= 160 * 1024, "a backward tile exceeds the LDS of a CU");
__host__ __device__ inline int vae_p1(int C) { return 64 * (4 * C + 1); }   // conv_1 partial row: dW (hidden/2, C, 4) | db (64) at hidden = 128

// din[ci][t'] (+)= sum_{co, kk : t * STRIDE + kk - pad = t'} W[co][ci][kk] * dout[co][t]   -- data gradient of conv1d_lds --
// then zeroed where the layer input's ReLU was off (mask: one word per channel, bit = position; NULL: no ReLU in front).
template <int KS, int STRIDE, bool ACCUM>
__device__ void conv1d_dgrad_lds(const float* dout, int Cout, int Tout, float* din, int Cin, int Tin,
                                 const float* __restrict__ W, int pad, int ld_out, int ld_in, const unsigned* mask,
                                 int mask_words) {
    constexpr int CP = VAE_CO_PER_THREAD;
    for (int o = threadIdx.x; o < (Cin / CP) * Tin; o += VAE_THREADS) {
        const int ci = (o / Tin) * CP, tp = o - (o / Tin) * Tin;
        float acc[CP];
#pragma unroll
        for (int u = 0; u < CP; ++u) acc[u] = 0.f;
        for (int co = 0; co < Cout; ++co) {
            const float* w = W + ((size_t)co * Cin + ci) * KS;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int num = tp + pad - kk;
                if (num < 0 || (STRIDE == 2 && (num & 1))) continue;
                const int t = STRIDE == 2 ? num >> 1 : num;
                if (t >= Tout) continue;
                const float d = dout[co * ld_out + t];
#pragma unroll
                for (int u = 0; u < CP; ++u) acc[u] += w[u * KS + kk] * d;
            }
        }
#pragma unroll
        for (int u = 0; u < CP; ++u) {
            float r = acc[u];
            if (ACCUM) r += din[(ci + u) * ld_in + tp];
            if (mask != nullptr && !((mask[(ci + u) * mask_words + (tp >> 5)] >> (tp & 31)) & 1u)) r = 0.f;
            din[(ci + u) * ld_in + tp] = r;
        }
    }
}

// one bit per (channel, position): buf > 0   (T <= 32 * words)
__device__ void relu_mask(const float* buf, int C, int T, int ld, unsigned* mask, int words) {
    for (int o = threadIdx.x; o < C * words; o += VAE_THREADS) {
        const int c = o / words, wd = o - c * words;
        unsigned m = 0;
        for (int t = 32 * wd; t < T && t < 32 * wd + 32; ++t) m |= (buf[c * ld + t] > 0.f ? 1u : 0u) << (t & 31);
        mask[o] = m;
    }
}

// X[row0 + t][ci * KS + kk] = buf[ci][t * STRIDE + kk - pad] (0 outside): the im2col'd input rows of a convolution
template <int KS, int STRIDE>
__device__ void im2col_rows(const float* buf, int Cin, int Tin, int ld, float* __restrict__ X, size_t row0, int Tout, int pad) {
    const int K = Cin * KS;
    for (int o = threadIdx.x; o < Tout * K; o += VAE_THREADS) {
        const int t = o / K, col = o - t * K;
        const int ci = col / KS, kk = col - ci * KS;
        const int ti = t * STRIDE + kk - pad;
        X[(row0 + t) * K + col] = (ti >= 0 && ti < Tin) ? buf[ci * ld + ti] : 0.f;
    }
}

// Y[row0 + t][c] = buf[c][t] for c < C, 0 for C <= c < Cpad
__device__ void rows_out(const float* buf, int C, int T, int ld, float* __restrict__ Y, size_t row0, int Cpad) {
    for (int o = threadIdx.x; o < T * Cpad; o += VAE_THREADS) {
        const int t = o / Cpad, c = o - t * Cpad;
        Y[(row0 + t) * Cpad + c] = c < C ? buf[c * ld + t] : 0.f;
    }
}

// residual_stack for the backward kernels: the same arithmetic on x = bufB (tmp = bufA), and what the backward needs stays
// behind -- the ReLU patterns m_r [n_res + 1][128] (r_l = relu(h_l), then r_final) and m_m [n_res][256] (m_l), the rows of r_l
// (im2col'd) and m_l.  Ends behind the final relu_mask: the caller writes r_final's rows where its next layer wants them.
template <int TB>
__device__ void residual_stack_recompute(float* bufB, float* bufA, int H, int R, int n_res, int T, const float* const* c3,
                                         const float* const* c1, const VaeStackBufs& s, size_t row0, unsigned* m_r, unsigned* m_m) {
    constexpr int LD = VaeBwdGeom<TB>::LD, WT = VaeBwdGeom<TB>::WT;
    for (int l = 0; l < n_res; ++l) {
        relu_inplace(bufB, H, T, LD);
        __syncthreads();
        relu_mask(bufB, H, T, LD, m_r + l * 128 * WT, WT);     // r_l > 0  <=>  h_l > 0
        im2col_rows<3, 1>(bufB, H, T, LD, s.Xr3[l], row0, T, 1);
        conv1d_lds<3, 1, true, false>(bufB, H, T, bufA, R, T, c3[l], nullptr, 1, LD, LD);
        __syncthreads();
        relu_mask(bufA, R, T, LD, m_m + l * 256 * WT, WT);
        rows_out(bufA, R, T, LD, s.Xm[l], row0, R);
        conv1d_lds<1, 1, false, true>(bufA, R, T, bufB, H, T, c1[l], nullptr, 0, LD, LD);
        __syncthreads();
    }
    relu_inplace(bufB, H, T, LD);
    __syncthreads();
    relu_mask(bufB, H, T, LD, m_r + n_res * 128 * WT, WT);
}

// The way back through the stack: bufB holds dL/dh_out of the last layer on entry (already masked by r_final > 0) and
// dL/dh_in of the first on return; every layer's output gradients leave as the row blocks dYc1 / dYc3.
template <int TB>
__device__ void residual_stack_backward(float* bufB, float* bufA, int H, int R, int n_res, int T, const float* const* c3,
                                        const float* const* c1, const VaeStackBufs& s, size_t row0, const unsigned* m_r,
                                        const unsigned* m_m) {
    constexpr int LD = VaeBwdGeom<TB>::LD, WT = VaeBwdGeom<TB>::WT;
    for (int l = n_res - 1; l >= 0; --l) {
        // bufB = dL/dh_out, h_out = r + c1(m), m = relu(c3(r)), r = relu(h_in)
        rows_out(bufB, H, T, LD, s.dYc1[l], row0, H);
        conv1d_dgrad_lds<1, 1, false>(bufB, H, T, bufA, R, T, c1[l], 0, LD, LD, m_m + l * 256 * WT, WT);   // d(pre-ReLU of m)
        __syncthreads();
        rows_out(bufA, R, T, LD, s.dYc3[l], row0, R);
        conv1d_dgrad_lds<3, 1, true>(bufA, R, T, bufB, H, T, c3[l], 1, LD, LD, m_r + l * 128 * WT, WT);    // + skip, masked: dL/dh_in
        __syncthreads();
    }
}

template <int TB>
__global__ __launch_bounds__(VAE_THREADS) void vae_encode_bwd_kernel(const VaeDev w, const float* __restrict__ x,
                                                                     const float* __restrict__ dz,
                                                                     const float* __restrict__ dbefore, const VaeBwdBufs s, int L,
                                                                     int W, int C) {
    using G = VaeBwdGeom<TB>;
    constexpr int LD = G::LD, WT = G::WT, WT2 = G::WT2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bufA = smem;
    float* bufB = smem + VAE_CMAX * LD;
    float* wide = bufB + VAE_CMAX * LD;                            // [hidden/2][T2]
    unsigned* m_w1 = reinterpret_cast<unsigned*>(smem + G::FLOATS);        // [64][WT2]
    unsigned* m_a = m_w1 + 64 * WT2;                               // [128][WT]
    unsigned* m_r = m_a + 128 * WT;                                // [5][128][WT]: r_l = relu(h_l) for l < n_res, then r_final
    unsigned* m_m = m_r + 5 * 128 * WT;                            // [4][256][WT]
    const int b = blockIdx.x;
    const int T2 = L / 2, T = L / 4, H = w.hidden, R = w.res_hidden, half_c = H / 2;
    const size_t row0 = (size_t)b * T;
    const float* xb = x + (size_t)b * C * L;
    // ---------------- forward, recomputed with vae_encode_kernel's pieces (one tile: the window is the series, conv_1's
    // outputs [0, T2) -- an odd T2 = 2 T + 1 keeps the last one, which conv_2's last window reads)
    encode_stem(w, xb, C, L, 0, T2, wide);
    __syncthreads();
    relu_mask(wide, half_c, T2, T2, m_w1, WT2);
    im2col_rows<4, 2>(wide, half_c, T2, T2, s.Xc2, row0, T, 1);
    conv1d_lds<4, 2, true, false>(wide, half_c, T2, bufA, H, T, w.enc_conv2_w, w.enc_conv2_b, 1, T2, LD, 0, 0);
    __syncthreads();
    relu_mask(bufA, H, T, LD, m_a, WT);
    im2col_rows<3, 1>(bufA, H, T, LD, s.Xc3, row0, T, 1);
    conv1d_lds<3, 1, false, false>(bufA, H, T, bufB, H, T, w.enc_conv3_w, w.enc_conv3_b, 1, LD, LD);
    __syncthreads();
    residual_stack_recompute<TB>(bufB, bufA, H, R, w.n_res, T, w.enc_c3, w.enc_c1, s.st, row0, m_r, m_m);
    rows_out(bufB, H, T, LD, s.Xp, row0, H);
    __syncthreads();
    // ---------------- backward.  dbefore_total = dbefore (if given) + interp^T(dz)  -> bufA [emb][T]
    {
        const float* g = dz + (size_t)b * w.emb * W;
        if (dbefore != nullptr)
            interp_linear_ac_transposed<true, false>(g, W, nullptr, 0, dbefore + (size_t)b * w.emb * T, T, bufA, LD, w.emb, T, W);
        else
            interp_linear_ac_transposed<false, false>(g, W, nullptr, 0, nullptr, 0, bufA, LD, w.emb, T, W);
    }
    __syncthreads();
    rows_out(bufA, w.emb, T, LD, s.dYp, row0, 128);                // padded to 128 columns for the weight-gradient GEMM
    // d r_final = Wp^T dbefore, masked by r_final > 0: the gradient at the stack's output h
    conv1d_dgrad_lds<1, 1, false>(bufA, w.emb, T, bufB, H, T, w.enc_prevq_w, 0, LD, LD, m_r + w.n_res * 128 * WT, WT);
    __syncthreads();
    residual_stack_backward<TB>(bufB, bufA, H, R, w.n_res, T, w.enc_c3, w.enc_c1, s.st, row0, m_r, m_m);
    rows_out(bufB, H, T, LD, s.dY3, row0, H);                       // dL/d(conv_3 output)
    conv1d_dgrad_lds<3, 1, false>(bufB, H, T, bufA, H, T, w.enc_conv3_w, 1, LD, LD, m_a, WT);                    // dL/d(conv_2 pre-ReLU)
    __syncthreads();
    rows_out(bufA, H, T, LD, s.dY2, row0, H);
    conv1d_dgrad_lds<4, 2, false>(bufA, H, T, wide, half_c, T2, w.enc_conv2_w, 1, LD, T2, m_w1, WT2);            // dL/d(conv_1 pre-ReLU)
    __syncthreads();
    // conv_1: dW[co][c][kk] = sum_u d[co][u] x[c][2u + kk - 1], db[co] = sum_u d[co][u]: one partial row per series, torch's
    // (hidden/2, C, 4) layout and the bias behind it
    const int per_co = 4 * C + 1;
    for (int o = threadIdx.x; o < half_c * per_co; o += VAE_THREADS) {
        const int co = o / per_co, j = o - co * per_co;
        const int c = j >> 2, kk = j & 3;
        float acc = 0.f;
        for (int u = 0; u < T2; ++u) {
            const float d = wide[co * T2 + u];
            if (j == 4 * C) acc += d;
            else {
                const int ti = 2 * u + kk - 1;
                if (ti >= 0 && ti < L) acc += d * xb[(size_t)c * L + ti];
            }
        }
        s.part1[(size_t)b * vae_p1(C) + (j == 4 * C ? half_c * 4 * C + co : co * 4 * C + j)] = acc;
    }
}

// out[c] = sum_b part[b][c] in series order (deterministic): 32 columns x 8 row slices per workgroup, the 8 slice sums added
// in slice order
__global__ __launch_bounds__(256) void vae_part_reduce_kernel(const float* __restrict__ part, int B, int cols, float* __restrict__ dw,
                                                              int n_w, float* __restrict__ db) {
    __shared__ float red[8][32];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
    float acc = 0.f;
    if (c < cols)
        for (int r = sl; r < B; r += 8) acc += part[(size_t)r * cols + c];
    red[sl][threadIdx.x & 31] = acc;
    __syncthreads();
    if (sl != 0 || c >= cols) return;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += red[k][threadIdx.x & 31];
    if (c < n_w) dw[c] = v;
    else db[c - n_w] = v;
}

// ------------------------------------------------------------------------------------------------ decoder backward
// Backward of Decoder.forward (vqvae.py:97-105, myvqvae.py:76-86), what LA-VAE pre-training (pretrained_lavae_unified.py) adds to
// the encoder backward above; the same scaffold (C channels, tile bound TB) and the same two stages:
//   vae_decode_bwd_kernel   one workgroup per series: the forward is recomputed in LDS by the
//                           functions vae_decode_kernel calls up to the ReLU behind _conv_trans_1 (the samples themselves are not
//                           needed), layer inputs leave as row blocks and ReLU patterns stay as bit words; then the data
//                           gradients walk back from drecon to the latent.  When L != 4 T the way back starts with the transpose
//                           of the final resampling 4 T -> L (the forward's interp_tap_ac taps): either way C x 4 T sample
//                           gradients are staged in LDS.  _conv_trans_2 (hidden/2 x C x 4 values) and the two small biases are
//                           reduced per series into partial rows.
//   launch_wgrad32          dW = dY^T X per layer.  _conv_1: K = emb * 3 = 192, im2col rows padded to 256 columns.
//                           _conv_trans_1 (Cin, Cout * 4): the layer INPUT rows are the N operand, the gathered rows of the
//                           output gradient (column co * 4 + kk = d[co][2 i - 1 + kk]) the K operand.
struct VaeDecBwdBufs {
    float *Xc1, *dY1, *Xct1, *Gct1, *part2, *partb1;
    VaeStackBufs st;
};
__host__ __device__ inline int vae_p2(int C) { return 64 * 4 * C + C; }   // _conv_trans_2 partial row: dW (hidden/2, C, 4) | db (C) at hidden = 128
constexpr int VAE_PB1 = 64;   // _conv_trans_1 bias partial row (hidden/2)

// din[ci][i] = sum_{co, kk : 0 <= 2 i - 1 + kk < Tout} W[ci][co][kk] * dout[co][2 i - 1 + kk]   -- data gradient of
// convT1d_k4s2_lds (a stride-2 convolution of the output gradient) -- zeroed where the layer input's ReLU was off.
__device__ void convT1d_k4s2_dgrad_lds(const float* dout, int Cout, int Tout, float* din, int Cin, int Tin,
                                       const float* __restrict__ W, int ld_out, int ld_in, const unsigned* mask, int mask_words) {
    constexpr int CP = VAE_CO_PER_THREAD;
    for (int o = threadIdx.x; o < (Cin / CP) * Tin; o += VAE_THREADS) {
        const int ci = (o / Tin) * CP, i = o - (o / Tin) * Tin;
        float acc[CP];
#pragma unroll
        for (int u = 0; u < CP; ++u) acc[u] = 0.f;
        for (int co = 0; co < Cout; ++co) {
            const float* w = W + ((size_t)ci * Cout + co) * 4;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int t = 2 * i - 1 + kk;
                if (t < 0 || t >= Tout) continue;
                const float d = dout[co * ld_out + t];
#pragma unroll
                for (int u = 0; u < CP; ++u) acc[u] += w[(size_t)u * Cout * 4 + kk] * d;
            }
        }
#pragma unroll
        for (int u = 0; u < CP; ++u) {
            const bool on = mask == nullptr || ((mask[(ci + u) * mask_words + (i >> 5)] >> (i & 31)) & 1u);
            din[(ci + u) * ld_in + i] = on ? acc[u] : 0.f;
        }
    }
}

template <int TB>
__global__ __launch_bounds__(VAE_THREADS) void vae_decode_bwd_kernel(const VaeDev w, const float* __restrict__ z,
                                                                     const float* __restrict__ drecon,
                                                                     const float* __restrict__ dafter, float* __restrict__ dz,
                                                                     const VaeDecBwdBufs s, int L, int W, int C) {
    using G = VaeBwdGeom<TB>;
    constexpr int LD = G::LD, WT = G::WT, WT2 = G::WT2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bufA = smem;
    float* bufB = smem + VAE_CMAX * LD;
    float* wide = bufB + VAE_CMAX * LD;                            // [hidden/2][2 T]
    unsigned* m_r = reinterpret_cast<unsigned*>(smem + G::FLOATS);         // [5][128][WT]: r_l for l < n_res, then r_final
    unsigned* m_m = m_r + 5 * 128 * WT;                            // [4][256][WT]
    unsigned* m_w = m_m + 4 * 256 * WT;                            // [64][WT2]: the ReLU behind _conv_trans_1
    float* dr = reinterpret_cast<float*>(m_w + 64 * WT2);          // [C][4 T]: this series' gradient at the samples of _conv_trans_2
    const int b = blockIdx.x;
    const int T = L / 4, T2 = 2 * T, L4 = 4 * T, H = w.hidden, R = w.res_hidden, half_c = H / 2, E = w.emb;
    const size_t row0 = (size_t)b * T;
    const int ldz = W <= TB ? LD : LDZ;
    // ---------------- forward, recomputed with vae_decode_kernel's pieces (one tile)
    stage_latent(z + (size_t)b * E * W, E, W, bufB, ldz);
    {
        const float* g = drecon + (size_t)b * C * L;
        if (L == L4)
            for (int o = threadIdx.x; o < C * L; o += VAE_THREADS) dr[o] = g[o];
        else      // recon = interp(samples, 4 T -> L): the sample gradients are its transpose
            interp_linear_ac_transposed<false, false>(g, L, nullptr, 0, nullptr, 0, dr, L4, C, L4, L);
    }
    __syncthreads();
    interp_linear_ac(bufB, E, W, ldz, bufA, T, LD);
    __syncthreads();
    // _conv_1's im2col rows, K = emb * 3 = 192 padded to 256 columns
    for (int o = threadIdx.x; o < T * 256; o += VAE_THREADS) {
        const int t = o >> 8, col = o & 255;
        const int ci = col / 3, ti = t + (col - ci * 3) - 1;
        s.Xc1[(row0 + t) * 256 + col] = (col < E * 3 && ti >= 0 && ti < T) ? bufA[ci * LD + ti] : 0.f;
    }
    conv1d_lds<3, 1, false, false>(bufA, E, T, bufB, H, T, w.dec_conv1_w, w.dec_conv1_b, 1, LD, LD);
    __syncthreads();
    residual_stack_recompute<TB>(bufB, bufA, H, R, w.n_res, T, w.dec_c3, w.dec_c1, s.st, row0, m_r, m_m);
    rows_out(bufB, H, T, LD, s.Xct1, row0, H);
    convT1d_k4s2_lds<true>(bufB, H, T, wide, half_c, w.dec_ct1_w, w.dec_ct1_b, LD, T2);
    __syncthreads();
    relu_mask(wide, half_c, T2, T2, m_w, WT2);
    // ---------------- backward.  _conv_trans_2: y[c][t] = b[c] + sum_{ci,kk : t = 2 i - 1 + kk} wide[ci][i] W[ci][c][kk]
    // dW[ci][c][kk] = sum_i wide[ci][i] dy[c][2 i - 1 + kk], db[c] = sum_t dy[c][t]: one partial row per series
    for (int o = threadIdx.x; o < vae_p2(C); o += VAE_THREADS) {
        float acc = 0.f;
        if (o >= half_c * 4 * C) {
            const float* d = dr + (o - half_c * 4 * C) * L4;
            for (int t = 0; t < L4; ++t) acc += d[t];
        } else {
            const int ci = o / (4 * C), c = (o >> 2) - ci * C, kk = o & 3;
            for (int i = 0; i < T2; ++i) {
                const int t = 2 * i - 1 + kk;
                if (t >= 0 && t < L4) acc += wide[ci * T2 + i] * dr[c * L4 + t];
            }
        }
        s.part2[(size_t)b * vae_p2(C) + o] = acc;
    }
    __syncthreads();
    // d(_conv_trans_1 pre-ReLU)[ci][i] = sum_c sum_kk W[ci][c][kk] dy[c][2 i - 1 + kk], masked, in place of wide
    for (int o = threadIdx.x; o < half_c * T2; o += VAE_THREADS) {
        const int ci = o / T2, i = o - ci * T2;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int t = 2 * i - 1 + kk;
                if (t >= 0 && t < L4) acc += w.dec_ct2_w[(ci * C + c) * 4 + kk] * dr[c * L4 + t];
            }
        }
        wide[o] = ((m_w[ci * WT2 + (i >> 5)] >> (i & 31)) & 1u) ? acc : 0.f;
    }
    __syncthreads();
    for (int co = threadIdx.x; co < half_c; co += VAE_THREADS) {    // _conv_trans_1 bias: column sum of its output gradient
        float acc = 0.f;
        for (int t = 0; t < T2; ++t) acc += wide[co * T2 + t];
        s.partb1[(size_t)b * VAE_PB1 + co] = acc;
    }
    im2col_rows<4, 2>(wide, half_c, T2, T2, s.Gct1, row0, T, 1);    // column co * 4 + kk = d[co][2 i - 1 + kk]
    // d r_final, masked by r_final > 0: the gradient at the stack's output h (r_final itself left as Xct1)
    convT1d_k4s2_dgrad_lds(wide, half_c, T2, bufB, H, T, w.dec_ct1_w, T2, LD, m_r + w.n_res * 128 * WT, WT);
    __syncthreads();
    residual_stack_backward<TB>(bufB, bufA, H, R, w.n_res, T, w.dec_c3, w.dec_c1, s.st, row0, m_r, m_m);
    rows_out(bufB, H, T, LD, s.dY1, row0, H);                       // dL/d(_conv_1 output)
    if (dz == nullptr) return;
    conv1d_dgrad_lds<3, 1, false>(bufB, H, T, bufA, E, T, w.dec_conv1_w, 1, LD, LD, nullptr, 1);   // dL/d(after), decoder part
    __syncthreads();
    // dz = interp^T(d after + dafter)
    float* dzb = dz + (size_t)b * E * W;
    if (dafter != nullptr)
        interp_linear_ac_transposed<false, true>(bufA, LD, dafter + (size_t)b * E * T, T, nullptr, 0, dzb, W, E, W, T);
    else
        interp_linear_ac_transposed<false, false>(bufA, LD, nullptr, 0, nullptr, 0, dzb, W, E, W, T);
}

// dst (rows, cols) = the first `cols` columns of src (rows, ld)
__global__ __launch_bounds__(256) void vae_copy_cols_kernel(const float* __restrict__ src, int ld, float* __restrict__ dst, int rows,
                                                            int cols) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < rows * cols) dst[o] = src[(size_t)(o / cols) * ld + (o % cols)];
}

}  // namespace t2s

using namespace t2s;

struct t2s_vae {
    VaeDev dev{};
    float* arena = nullptr;
    bool has_encoder = false;
    bool has_decoder = false;
    int channels = 0;             // 0: the single-channel codec (t2s_vae_create); C: the multichannel one (t2s_vae_create_mc)
    // the two backwards (t2s_vae_encode_backward, t2s_vae_decode_backward): each its own row blocks, the weight-gradient
    // partial tiles `wg` shared; all grown on demand
    struct RowBuf {
        float* p = nullptr;
        size_t rows = 0;          // rows (= B * L / 4) the row blocks hold
        int series = 0;           // series the per-series partial rows hold
    } bwd, dbwd;
    float* wg = nullptr;
    size_t wg_floats = 0;
    int n_cu = 0;
};

namespace {
struct VaeItem { const float* src; size_t n; const float** dst; };

// every tensor of *w the handle keeps a device copy of, with the VaeDev slot that points at the copy
// (C = series channels: 1 for the single-channel codec)
int vae_items(const t2s_vae_weights* w, VaeDev& d, bool dec, bool enc, std::vector<VaeItem>& items, int C) {
    const int H = w->hidden, R = w->res_hidden, E = w->emb, NR = w->n_res_layers;
    if (dec)
        items = {{w->dec_conv1_w, (size_t)H * E * 3, &d.dec_conv1_w}, {w->dec_conv1_b, (size_t)H, &d.dec_conv1_b},
                 {w->dec_ct1_w, (size_t)H * (H / 2) * 4, &d.dec_ct1_w}, {w->dec_ct1_b, (size_t)H / 2, &d.dec_ct1_b},
                 {w->dec_ct2_w, (size_t)(H / 2) * C * 4, &d.dec_ct2_w}, {w->dec_ct2_b, (size_t)C, &d.dec_ct2_b}};
    for (int l = 0; dec && l < NR; ++l) {
        T2S_REQUIRE(w->dec_stack.conv3_w[l] && w->dec_stack.conv1_w[l], "t2s_vae: NULL decoder residual weight %d", l);
        items.push_back({w->dec_stack.conv3_w[l], (size_t)R * H * 3, &d.dec_c3[l]});
        items.push_back({w->dec_stack.conv1_w[l], (size_t)H * R, &d.dec_c1[l]});
    }
    if (enc) {
        items.push_back({w->enc_conv1_w, (size_t)(H / 2) * C * 4, &d.enc_conv1_w});
        items.push_back({w->enc_conv1_b, (size_t)H / 2, &d.enc_conv1_b});
        items.push_back({w->enc_conv2_w, (size_t)H * (H / 2) * 4, &d.enc_conv2_w});
        items.push_back({w->enc_conv2_b, (size_t)H, &d.enc_conv2_b});
        items.push_back({w->enc_conv3_w, (size_t)H * H * 3, &d.enc_conv3_w});
        items.push_back({w->enc_conv3_b, (size_t)H, &d.enc_conv3_b});
        items.push_back({w->enc_prevq_w, (size_t)E * H, &d.enc_prevq_w});
        items.push_back({w->enc_prevq_b, (size_t)E, &d.enc_prevq_b});
        for (int l = 0; l < NR; ++l) {
            T2S_REQUIRE(w->enc_stack.conv3_w[l] && w->enc_stack.conv1_w[l], "t2s_vae: NULL encoder residual weight %d", l);
            items.push_back({w->enc_stack.conv3_w[l], (size_t)R * H * 3, &d.enc_c3[l]});
            items.push_back({w->enc_stack.conv1_w[l], (size_t)H * R, &d.enc_c1[l]});
        }
    }
    return T2S_OK;
}
}

namespace { int vae_bwd_init(); }

// t2s_vae_create (channels 0) and t2s_vae_create_mc (channels 1..16), `who` = the entry's name
static int vae_create(const t2s_vae_weights* w, int channels, t2s_vae** out, const char* who) {
    T2S_REQUIRE(w && out, "%s: NULL argument", who);
    T2S_REQUIRE(w->hidden > 0 && w->hidden <= 128 && w->hidden % 2 == 0, "%s: hidden=%d unsupported (<=128, even)", who, w->hidden);
    T2S_REQUIRE(w->res_hidden > 0 && w->res_hidden <= VAE_CMAX, "%s: res_hidden=%d unsupported (<=256)", who, w->res_hidden);
    T2S_REQUIRE(w->n_res_layers >= 0 && w->n_res_layers <= 4, "%s: n_res_layers=%d unsupported (<=4)", who, w->n_res_layers);
    T2S_REQUIRE(w->emb == T2S_LAT_C, "%s: embedding_dim=%d must be 64", who, w->emb);
    const bool dec = w->dec_conv1_w != nullptr;
    const bool enc = w->enc_conv1_w != nullptr;
    T2S_REQUIRE(dec || enc, "%s: neither decoder nor encoder weights given", who);
    if (dec)
        T2S_REQUIRE(w->dec_conv1_b && w->dec_ct1_w && w->dec_ct1_b && w->dec_ct2_w && w->dec_ct2_b,
                    "%s: partial decoder weights", who);
    const int H = w->hidden, R = w->res_hidden, E = w->emb, NR = w->n_res_layers;
    if (enc)
        T2S_REQUIRE(w->enc_conv1_b && w->enc_conv2_w && w->enc_conv2_b && w->enc_conv3_w && w->enc_conv3_b &&
                        w->enc_prevq_w && w->enc_prevq_b,
                    "%s: partial encoder weights", who);
    t2s_vae* h = new t2s_vae();
    VaeDev& d = h->dev;
    d.hidden = H; d.res_hidden = R; d.n_res = NR; d.emb = E;
    std::vector<VaeItem> items;
    {
        const int rc_items = vae_items(w, d, dec, enc, items, channels ? channels : 1);
        if (rc_items != T2S_OK) {
            delete h;
            return rc_items;
        }
    }
    const std::string what = std::string(who) + ": a weight tensor (hyper-parameters vs tensor sizes)";
    for (auto& it : items) {      // sizes follow from hidden / res_hidden / emb (/ channels): a tensor of another shape is an error code
        const int rc_e = it.src ? check_device_extent(it.src, it.n * sizeof(float), what.c_str()) : T2S_OK;
        if (rc_e != T2S_OK) {
            delete h;
            return rc_e;
        }
    }
    size_t total = 0;
    for (auto& it : items) total += r64(it.n);
    hipError_t e = hipMalloc(&h->arena, total * sizeof(float));
    if (e != hipSuccess) {
        set_error("%s: hipMalloc failed: %s", who, hipGetErrorString(e));
        delete h;
        return T2S_E_HIP;
    }
    size_t off = 0;
    for (auto& it : items) {
        // (asynchronous on the default stream -- ordered behind whatever the caller's framework enqueued there to produce the
        // tensors -- and ONE synchronisation below; a synchronous hipMemcpy is what HIP refuses while another thread has a
        // stream capture open)
        e = hipMemcpyAsync(h->arena + off, it.src, it.n * sizeof(float), hipMemcpyDeviceToDevice, nullptr);
        if (e != hipSuccess) {
            set_error("%s: weight copy failed: %s", who, hipGetErrorString(e));
            t2s_vae_destroy(h);
            return T2S_E_HIP;
        }
        *it.dst = h->arena + off;
        off += r64(it.n);
    }
    e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        set_error("%s: weight copy failed: %s", who, hipGetErrorString(e));
        t2s_vae_destroy(h);
        return T2S_E_HIP;
    }
    h->has_encoder = enc;
    h->has_decoder = dec;
    h->channels = channels;
    static bool attr = false;
    if (!attr) {
        const int bytes = VAE_LDS_FLOATS * 4;
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vae_decode_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vae_encode_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vae_decode_ragged_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vae_encode_ragged_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attr = true;
    }
    (void)vae_bwd_init();         // (here, outside any stream capture; a refusal is reported by the backward entries)
    *out = h;
    return T2S_OK;
}

extern "C" int t2s_vae_create(const t2s_vae_weights* w, t2s_vae** out) { return vae_create(w, 0, out, "t2s_vae_create"); }

extern "C" int t2s_vae_create_mc(const t2s_vae_weights* w, int channels, t2s_vae** out) {
    T2S_REQUIRE(channels >= 1 && channels <= VAE_MC_CMAX, "t2s_vae_create_mc: channels=%d unsupported (1..%d)", channels, VAE_MC_CMAX);
    return vae_create(w, channels, out, "t2s_vae_create_mc");
}

extern "C" int t2s_vae_channels(const t2s_vae* h) { return h ? h->channels : 0; }

extern "C" void t2s_vae_destroy(t2s_vae* h) {
    if (!h) return;
    if (h->arena) (void)hipFree(h->arena);
    if (h->bwd.p) (void)hipFree(h->bwd.p);
    if (h->wg) (void)hipFree(h->wg);
    if (h->dbwd.p) (void)hipFree(h->dbwd.p);
    delete h;
}

extern "C" int t2s_vae_update_weights(t2s_vae* h, const t2s_vae_weights* w, void* stream) {
    T2S_REQUIRE(h && w, "t2s_vae_update_weights: NULL argument");
    T2S_REQUIRE(w->hidden == h->dev.hidden && w->res_hidden == h->dev.res_hidden && w->n_res_layers == h->dev.n_res && w->emb == h->dev.emb,
                "t2s_vae_update_weights: hyper-parameters differ from the handle's (hidden %d, res_hidden %d, layers %d, emb %d)",
                h->dev.hidden, h->dev.res_hidden, h->dev.n_res, h->dev.emb);
    T2S_REQUIRE((w->dec_conv1_w != nullptr) == h->has_decoder && (w->enc_conv1_w != nullptr) == h->has_encoder,
                "t2s_vae_update_weights: the handle was created with %s%s weights", h->has_encoder ? "encoder " : "", h->has_decoder ? "decoder" : "");
    VaeDev d = h->dev;                       // the slots keep pointing at the handle's copies: only the contents change
    std::vector<VaeItem> items;
    const int rc = vae_items(w, d, h->has_decoder, h->has_encoder, items, h->channels ? h->channels : 1);
    if (rc != T2S_OK) return rc;
    for (auto& it : items) {
        T2S_REQUIRE(it.src, "t2s_vae_update_weights: NULL weight pointer");
        const int rc_e = check_device_extent(it.src, it.n * sizeof(float), "t2s_vae_update_weights: a weight tensor");
        if (rc_e != T2S_OK) return rc_e;
        T2S_HIP_CHECK(hipMemcpyAsync(const_cast<float*>(*it.dst), it.src, it.n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return T2S_OK;
}

// ------------------------------------------------------------------------ what the forward entries share on the host
namespace {
// The handle's kind and the shape, `who` = the entry's name, `mc` = its family: the multichannel entries take a t2s_vae_create_mc
// handle, any L >= 8 and a latent up to 64 wide; the single-channel ones a t2s_vae_create handle, L a multiple of 4 and a latent
// up to 32 wide.
int vae_fwd_check(const char* who, const t2s_vae* h, bool mc, int B, int L, int W) {
    if (mc)
        T2S_REQUIRE(h->channels != 0, "%s: the handle is a single-channel one (t2s_vae_create); its entries are t2s_vae_encode / t2s_vae_decode[_w]", who);
    else
        T2S_REQUIRE(h->channels == 0, "%s: the handle is a multichannel one (t2s_vae_create_mc); its entries are t2s_vae_encode_mc / t2s_vae_decode_mc", who);
    T2S_REQUIRE(B > 0, "%s: B=%d", who, B);
    if (mc)
        T2S_REQUIRE(L >= 8 && L <= (1 << 20), "%s: L=%d unsupported (8 .. 2^20)", who, L);
    else
        T2S_REQUIRE(L >= 4 && L % 4 == 0 && L <= (1 << 20), "%s: L=%d unsupported (a multiple of 4)", who, L);
    const int wmax = mc ? VAE_MC_WMAX : VAE_TMAX;
    T2S_REQUIRE(W >= 1 && W <= wmax, "%s: latent width %d unsupported (1..%d)", who, W, wmax);
    return T2S_OK;
}

int vae_decode(const char* who, bool mc, t2s_vae* h, const float* z, float* recon, float* after, int B, int L, int W, void* stream) {
    T2S_REQUIRE(h && z && recon, "%s: NULL argument", who);
    T2S_REQUIRE(h->has_decoder, "%s: handle was created without decoder weights", who);
    int rc;
    if ((rc = vae_fwd_check(who, h, mc, B, L, W))) return rc;
    vae_decode_kernel<<<dim3(B, vae_tiles(L / 4, h->dev.n_res + 2)), VAE_THREADS, VAE_LDS_FLOATS * 4, (hipStream_t)stream>>>(
        h->dev, z, recon, after, L, W, h->channels ? h->channels : 1);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int vae_encode(const char* who, bool mc, t2s_vae* h, const float* x, float* z, float* before, int B, int L, int W, void* stream) {
    T2S_REQUIRE(h && x && z, "%s: NULL argument", who);
    T2S_REQUIRE(h->has_encoder, "%s: handle was created without encoder weights", who);
    int rc;
    if ((rc = vae_fwd_check(who, h, mc, B, L, W))) return rc;
    const int tiles = vae_tiles(L / 4, h->dev.n_res + 1);
    T2S_REQUIRE(tiles == 1 || before, "%s: L=%d (L/4 > 32) runs in time tiles and needs the `before` output buffer "
                                      "(the interpolation to the latent reads the whole row)", who, L);
    vae_encode_kernel<<<dim3(B, tiles), VAE_THREADS, VAE_LDS_FLOATS * 4, (hipStream_t)stream>>>(h->dev, x, z, before, L, W,
                                                                                              h->channels ? h->channels : 1);
    T2S_LAUNCH_CHECK();
    if (tiles > 1) {
        vae_interp_rows_kernel<<<B, VAE_THREADS, 0, (hipStream_t)stream>>>(before, z, h->dev.emb, L / 4, W);
        T2S_LAUNCH_CHECK();
    }
    return T2S_OK;
}
}

extern "C" int t2s_vae_decode(t2s_vae* h, const float* z, float* recon, float* after, int B, int L, void* stream) {
    return vae_decode("t2s_vae_decode", false, h, z, recon, after, B, L, LATW, stream);
}

extern "C" int t2s_vae_decode_w(t2s_vae* h, const float* z, float* recon, float* after, int B, int L, int latent_w, void* stream) {
    return vae_decode("t2s_vae_decode_w", false, h, z, recon, after, B, L, latent_w, stream);
}

extern "C" int t2s_vae_decode_mc(t2s_vae* h, const float* z, float* recon, float* after, int B, int L, int latent_w, void* stream) {
    return vae_decode("t2s_vae_decode_mc", true, h, z, recon, after, B, L, latent_w, stream);
}

extern "C" int t2s_vae_encode(t2s_vae* h, const float* x, float* z, float* before, int B, int L, void* stream) {
    return vae_encode("t2s_vae_encode", false, h, x, z, before, B, L, LATW, stream);
}

extern "C" int t2s_vae_encode_mc(t2s_vae* h, const float* x, float* z, float* before, int B, int L, int latent_w, void* stream) {
    return vae_encode("t2s_vae_encode_mc", true, h, x, z, before, B, L, latent_w, stream);
}

// Ragged rows (include/t2s.h): one launch over the rows' own lengths, the grid's tile dimension sized for max_L
extern "C" int t2s_vae_decode_mc_ragged(t2s_vae* h, const float* z, const int32_t* lengths, const uint64_t* offsets, float* recon,
                                        int B, int max_L, int latent_w, void* stream) {
    const char* who = "t2s_vae_decode_mc_ragged";
    T2S_REQUIRE(h && z && lengths && offsets && recon, "%s: NULL argument", who);
    T2S_REQUIRE(h->has_decoder, "%s: handle was created without decoder weights", who);
    int rc;
    if ((rc = vae_fwd_check(who, h, true, B, max_L, latent_w))) return rc;
    vae_decode_ragged_kernel<<<dim3(B, vae_tiles(max_L / 4, h->dev.n_res + 2)), VAE_THREADS, VAE_LDS_FLOATS * 4, (hipStream_t)stream>>>(
        h->dev, z, lengths, offsets, recon, max_L, latent_w, h->channels);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_vae_encode_mc_ragged(t2s_vae* h, const float* x, const int32_t* lengths, const uint64_t* offsets,
                                        const uint64_t* offsets4, float* z, float* before, int B, int max_L, int latent_w,
                                        void* stream) {
    const char* who = "t2s_vae_encode_mc_ragged";
    T2S_REQUIRE(h && x && lengths && offsets && offsets4 && z, "%s: NULL argument", who);
    T2S_REQUIRE(h->has_encoder, "%s: handle was created without encoder weights", who);
    int rc;
    if ((rc = vae_fwd_check(who, h, true, B, max_L, latent_w))) return rc;
    const int tiles = vae_tiles(max_L / 4, h->dev.n_res + 1);
    T2S_REQUIRE(tiles == 1 || before, "%s: max_L=%d (max_L/4 > 32) runs in time tiles and needs the `before` output buffer "
                                      "(the interpolation to the latent reads the whole row)", who, max_L);
    vae_encode_ragged_kernel<<<dim3(B, tiles), VAE_THREADS, VAE_LDS_FLOATS * 4, (hipStream_t)stream>>>(
        h->dev, x, lengths, offsets, offsets4, z, before, max_L, latent_w, h->channels);
    T2S_LAUNCH_CHECK();
    if (tiles > 1) {
        vae_interp_rows_ragged_kernel<<<B, VAE_THREADS, 0, (hipStream_t)stream>>>(before, z, lengths, offsets, offsets4, max_L,
                                                                                  h->dev.emb, latent_w);
        T2S_LAUNCH_CHECK();
    }
    return T2S_OK;
}

// ------------------------------------------------------------------------ what the backward entries share on the host
namespace {
// The handle's kind and shape and the batch, `who` = the entry's name, `mc` = its family, as vae_fwd_check: the multichannel
// entries take a t2s_vae_create_mc handle with at least one residual layer, any 8 <= L <= 192 and a latent up to 64 wide; the
// single-channel ones a t2s_vae_create handle, L <= 128 a multiple of 4 and a latent up to 32 wide.
int vae_bwd_check(const char* who, const t2s_vae* h, bool mc, bool enc, int B, int L, int W) {
    const VaeDev& d = h->dev;
    if (mc) {
        T2S_REQUIRE(h->channels != 0, "%s: the handle is a single-channel one (t2s_vae_create); its entries are t2s_vae_encode_backward / t2s_vae_decode_backward", who);
    } else {
        T2S_REQUIRE(h->channels == 0, "%s: the handle is a multichannel one (t2s_vae_create_mc); its entries are t2s_vae_encode_mc / t2s_vae_decode_mc and their backwards t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc", who);
    }
    T2S_REQUIRE(enc ? h->has_encoder : h->has_decoder, "%s: handle was created without %s weights", who, enc ? "encoder" : "decoder");
    if (mc) T2S_REQUIRE(d.n_res >= 1, "%s: n_res=0 unsupported (1..4 residual layers)", who);
    // the weight-gradient GEMMs work on 128-wide tiles: the reference's default LA-VAE (pretrained_lavae_unified.py:119-122)
    T2S_REQUIRE(d.hidden == 128 && d.res_hidden % 128 == 0 && d.emb == 64,
                "%s: hidden=%d res_hidden=%d emb=%d unsupported (hidden 128, res_hidden 128 / 256, emb 64)", who, d.hidden, d.res_hidden, d.emb);
    if (mc)
        T2S_REQUIRE(B > 0 && L >= 8 && L <= 4 * 48, "%s: B=%d L=%d unsupported (8 <= L <= 192)", who, B, L);
    else
        T2S_REQUIRE(B > 0 && L >= 8 && L % 4 == 0 && L <= 4 * VAE_TMAX, "%s: B=%d L=%d unsupported (8 <= L <= 128, a multiple of 4)", who, B, L);
    const int wmax = mc ? VAE_MC_WMAX : VAE_TMAX;
    T2S_REQUIRE(W >= 1 && W <= wmax, "%s: latent width %d unsupported (1..%d)", who, W, wmax);
    return T2S_OK;
}

// The dynamic-LDS caps of the four backward instantiations, requested once (the first backward call: training is never under a
// stream capture).  A refusal is remembered and returned by every later call too: nothing launches without its cap.
int vae_bwd_init() {
    static int state = -1;
    static std::string why;
    if (state < 0) {
        const struct { const void* k; int bytes; const char* name; } caps[4] = {
            {reinterpret_cast<const void*>(vae_encode_bwd_kernel<32>), VaeBwdGeom<32>::ENC_BYTES, "vae_encode_bwd_kernel<32>"},
            {reinterpret_cast<const void*>(vae_encode_bwd_kernel<48>), VaeBwdGeom<48>::ENC_BYTES, "vae_encode_bwd_kernel<48>"},
            {reinterpret_cast<const void*>(vae_decode_bwd_kernel<32>), VaeBwdGeom<32>::DEC_BYTES_MAX, "vae_decode_bwd_kernel<32>"},
            {reinterpret_cast<const void*>(vae_decode_bwd_kernel<48>), VaeBwdGeom<48>::DEC_BYTES_MAX, "vae_decode_bwd_kernel<48>"}};
        state = T2S_OK;
        for (auto& c : caps) {
            const hipError_t e = hipFuncSetAttribute(c.k, hipFuncAttributeMaxDynamicSharedMemorySize, c.bytes);
            if (e != hipSuccess) {
                why = std::string(c.name) + ": the runtime refused " + std::to_string(c.bytes) + " bytes of dynamic LDS: " + hipGetErrorString(e);
                state = T2S_E_HIP;
                break;
            }
        }
    }
    if (state != T2S_OK) set_error("t2s_vae backward: %s", why.c_str());
    return state;
}

int vae_cu_count(t2s_vae* h) {
    if (h->n_cu != 0) return T2S_OK;
    int dev = 0;
    hipDeviceProp_t prop;
    T2S_HIP_CHECK(hipGetDevice(&dev));
    T2S_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    h->n_cu = prop.multiProcessorCount;
    return T2S_OK;
}

// the weight-gradient partial tiles serve the largest of the caller's (N, K) shapes
template <int n>
int vae_ensure_wg(t2s_vae* h, const int (&shapes)[n][2]) {
    size_t need = 0;
    for (auto& sh : shapes) {
        const size_t f = wgrad16_shape_scratch_floats(sh[0], sh[1], h->n_cu);
        need = f > need ? f : need;
    }
    if (need <= h->wg_floats) return T2S_OK;
    if (h->wg) T2S_HIP_CHECK(hipFree(h->wg));
    h->wg = nullptr;
    h->wg_floats = 0;              // (a failed hipMalloc below must not leave a size that vouches for a NULL buffer)
    T2S_HIP_CHECK(hipMalloc((void**)&h->wg, need * sizeof(float)));
    h->wg_floats = need;
    return T2S_OK;
}

// `rb` holds `rows` row-block rows of per_row floats, B partial rows of per_series floats and `fixed` floats.  It grows when
// rows > rb.rows or B > rb.series, and never shrinks; growing frees and allocates, which the host mirror serialises under its
// per-device lock -- vqvae.py (_vae_backward) repeats exactly this condition to know when.
int vae_grow_rows(t2s_vae::RowBuf& rb, size_t rows, int B, size_t per_row, size_t per_series, size_t fixed) {
    if (rows <= rb.rows && B <= rb.series) return T2S_OK;
    const size_t r2 = rows > rb.rows ? rows : rb.rows;
    const int b2 = B > rb.series ? B : rb.series;
    if (rb.p) T2S_HIP_CHECK(hipFree(rb.p));
    rb = t2s_vae::RowBuf{};       // (a failed hipMalloc below must not leave sizes that vouch for a NULL buffer)
    T2S_HIP_CHECK(hipMalloc((void**)&rb.p, (r2 * per_row + (size_t)b2 * per_series + fixed) * sizeof(float)));
    rb.rows = r2;
    rb.series = b2;
    return T2S_OK;
}

// hands out the row blocks of a RowBuf in order
struct VaeTake {
    float* p;
    size_t rows;
    float* operator()(size_t cols) { float* q = p; p += rows * cols; return q; }
};

// the residual stack's share of a row buffer: floats per row and the hand-out in the same order; its weight gradients
size_t vae_stack_row_floats(int NR, int R) { return (size_t)NR * (384 + R + 128 + R); }
void vae_stack_take(VaeTake& take, VaeStackBufs& s, int NR, int R) {
    for (int l = 0; l < NR; ++l) { s.Xr3[l] = take(384); s.Xm[l] = take(R); s.dYc1[l] = take(128); s.dYc3[l] = take(R); }
}
int vae_stack_wgrad(t2s_vae* h, const VaeStackBufs& s, float* const* g_c3, float* const* g_c1, int M, hipStream_t st) {
    const int R = h->dev.res_hidden;
    int rc;
    for (int l = 0; l < h->dev.n_res; ++l) {
        if ((rc = launch_wgrad32(s.dYc3[l], s.Xr3[l], g_c3[l], nullptr, M, R, 384, h->wg, h->wg_floats, h->n_cu, st))) return rc;
        if ((rc = launch_wgrad32(s.dYc1[l], s.Xm[l], g_c1[l], nullptr, M, 128, R, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    }
    return T2S_OK;
}

// t2s_vae_encode_backward (C = 1, the 30-wide latent) and t2s_vae_encode_backward_mc
int vae_encode_backward(const char* who, bool mc, t2s_vae* h, const float* x, const float* dz, const float* dbefore,
                        const t2s_vae_enc_grads* g, int B, int L, int W, void* stream) {
    T2S_REQUIRE(h && x && dz && g, "%s: NULL argument", who);
    const VaeDev& d = h->dev;
    int rc;
    if ((rc = vae_bwd_check(who, h, mc, true, B, L, W))) return rc;
    T2S_REQUIRE(g->conv1_w && g->conv1_b && g->conv2_w && g->conv2_b && g->conv3_w && g->conv3_b && g->prevq_w && g->prevq_b,
                "%s: NULL gradient pointer", who);
    for (int l = 0; l < d.n_res; ++l)
        T2S_REQUIRE(g->stack_conv3_w[l] && g->stack_conv1_w[l], "%s: NULL gradient pointer of residual layer %d", who, l);
    if ((rc = vae_bwd_init())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = d.res_hidden, NR = d.n_res, M = B * (L / 4), C = h->channels ? h->channels : 1, P1 = vae_p1(C);
    if ((rc = vae_cu_count(h))) return rc;
    // row blocks: floats per row, in the order the pointers are handed out below; conv_1's partial rows; prevq padded to 128 outputs
    if ((rc = vae_grow_rows(h->bwd, (size_t)M, B, 256 + 384 + 128 + 128 + 128 + 128 + vae_stack_row_floats(NR, R), P1, 128 * 128 + 128)))
        return rc;
    const int shapes[5][2] = {{128, 256}, {128, 384}, {R, 384}, {128, R}, {128, 128}};
    if ((rc = vae_ensure_wg(h, shapes))) return rc;
    VaeBwdBufs s{};
    VaeTake take{h->bwd.p, h->bwd.rows};
    s.Xc2 = take(256); s.Xc3 = take(384); s.Xp = take(128); s.dYp = take(128); s.dY3 = take(128); s.dY2 = take(128);
    vae_stack_take(take, s.st, NR, R);
    s.part1 = take.p;
    float* tmp_w = s.part1 + (size_t)h->bwd.series * P1;           // (128,128) + (128): prevq padded to 128 outputs
    float* tmp_b = tmp_w + 128 * 128;
    if (L <= 4 * 32)
        vae_encode_bwd_kernel<32><<<B, VAE_THREADS, VaeBwdGeom<32>::ENC_BYTES, st>>>(d, x, dz, dbefore, s, L, W, C);
    else
        vae_encode_bwd_kernel<48><<<B, VAE_THREADS, VaeBwdGeom<48>::ENC_BYTES, st>>>(d, x, dz, dbefore, s, L, W, C);
    T2S_LAUNCH_CHECK();
    if ((rc = launch_wgrad32(s.dY2, s.Xc2, g->conv2_w, g->conv2_b, M, 128, 256, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    if ((rc = launch_wgrad32(s.dY3, s.Xc3, g->conv3_w, g->conv3_b, M, 128, 384, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    if ((rc = vae_stack_wgrad(h, s.st, g->stack_conv3_w, g->stack_conv1_w, M, st))) return rc;
    if ((rc = launch_wgrad32(s.dYp, s.Xp, tmp_w, tmp_b, M, 128, 128, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    T2S_HIP_CHECK(hipMemcpyAsync(g->prevq_w, tmp_w, (size_t)64 * 128 * sizeof(float), hipMemcpyDeviceToDevice, st));
    T2S_HIP_CHECK(hipMemcpyAsync(g->prevq_b, tmp_b, (size_t)64 * sizeof(float), hipMemcpyDeviceToDevice, st));
    vae_part_reduce_kernel<<<(P1 + 31) / 32, 256, 0, st>>>(s.part1, B, P1, g->conv1_w, 256 * C, g->conv1_b);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// t2s_vae_decode_backward (C = 1) and t2s_vae_decode_backward_mc
int vae_decode_backward(const char* who, bool mc, t2s_vae* h, const float* z, const float* drecon, const float* dafter,
                        const t2s_vae_dec_grads* g, float* dz, int B, int L, int W, void* stream) {
    T2S_REQUIRE(h && z && drecon && g, "%s: NULL argument", who);
    const VaeDev& d = h->dev;
    int rc;
    if ((rc = vae_bwd_check(who, h, mc, false, B, L, W))) return rc;
    T2S_REQUIRE(g->conv1_w && g->conv1_b && g->ct1_w && g->ct1_b && g->ct2_w && g->ct2_b, "%s: NULL gradient pointer", who);
    for (int l = 0; l < d.n_res; ++l)
        T2S_REQUIRE(g->stack_conv3_w[l] && g->stack_conv1_w[l], "%s: NULL gradient pointer of residual layer %d", who, l);
    if ((rc = vae_bwd_init())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = d.res_hidden, NR = d.n_res, M = B * (L / 4), C = h->channels ? h->channels : 1, P2 = vae_p2(C);
    if ((rc = vae_cu_count(h))) return rc;
    // row blocks: floats per row, in the order the pointers are handed out below; the two partial rows; _conv_1 with K padded to 256
    if ((rc = vae_grow_rows(h->dbwd, (size_t)M, B, 256 + 128 + 128 + 256 + vae_stack_row_floats(NR, R), P2 + VAE_PB1, 128 * 256))) return rc;
    const int shapes[3][2] = {{128, 256}, {R, 384}, {128, R}};
    if ((rc = vae_ensure_wg(h, shapes))) return rc;
    VaeDecBwdBufs s{};
    VaeTake take{h->dbwd.p, h->dbwd.rows};
    s.Xc1 = take(256); s.dY1 = take(128); s.Xct1 = take(128); s.Gct1 = take(256);
    vae_stack_take(take, s.st, NR, R);
    float* tmp_w = take.p;                                         // (128,256): _conv_1 with K padded from 192
    s.part2 = tmp_w + 128 * 256;
    s.partb1 = s.part2 + (size_t)h->dbwd.series * P2;
    const int dr_bytes = C * 4 * (L / 4) * (int)sizeof(float);     // the staged sample gradients
    if (L <= 4 * 32)
        vae_decode_bwd_kernel<32><<<B, VAE_THREADS, VaeBwdGeom<32>::DEC_BYTES + dr_bytes, st>>>(d, z, drecon, dafter, dz, s, L, W, C);
    else
        vae_decode_bwd_kernel<48><<<B, VAE_THREADS, VaeBwdGeom<48>::DEC_BYTES + dr_bytes, st>>>(d, z, drecon, dafter, dz, s, L, W, C);
    T2S_LAUNCH_CHECK();
    if ((rc = launch_wgrad32(s.dY1, s.Xc1, tmp_w, g->conv1_b, M, 128, 256, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    vae_copy_cols_kernel<<<(128 * 192 + 255) / 256, 256, 0, st>>>(tmp_w, 256, g->conv1_w, 128, 192);
    T2S_LAUNCH_CHECK();
    if ((rc = vae_stack_wgrad(h, s.st, g->stack_conv3_w, g->stack_conv1_w, M, st))) return rc;
    if ((rc = launch_wgrad32(s.Xct1, s.Gct1, g->ct1_w, nullptr, M, 128, 256, h->wg, h->wg_floats, h->n_cu, st))) return rc;
    vae_part_reduce_kernel<<<(P2 + 31) / 32, 256, 0, st>>>(s.part2, B, P2, g->ct2_w, 256 * C, g->ct2_b);
    T2S_LAUNCH_CHECK();
    vae_part_reduce_kernel<<<VAE_PB1 / 32, 256, 0, st>>>(s.partb1, B, VAE_PB1, g->ct1_b, VAE_PB1, nullptr);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
}

extern "C" int t2s_vae_encode_backward(t2s_vae* h, const float* x, const float* dz, const float* dbefore, const t2s_vae_enc_grads* g,
                                       int B, int L, void* stream) {
    return vae_encode_backward("t2s_vae_encode_backward", false, h, x, dz, dbefore, g, B, L, LATW, stream);
}

extern "C" int t2s_vae_encode_backward_mc(t2s_vae* h, const float* x, const float* dz, const float* dbefore, const t2s_vae_enc_grads* g,
                                          int B, int L, int latent_w, void* stream) {
    return vae_encode_backward("t2s_vae_encode_backward_mc", true, h, x, dz, dbefore, g, B, L, latent_w, stream);
}

extern "C" int t2s_vae_decode_backward(t2s_vae* h, const float* z, const float* drecon, const float* dafter,
                                       const t2s_vae_dec_grads* g, float* dz, int B, int L, int latent_w, void* stream) {
    return vae_decode_backward("t2s_vae_decode_backward", false, h, z, drecon, dafter, g, dz, B, L, latent_w, stream);
}

extern "C" int t2s_vae_decode_backward_mc(t2s_vae* h, const float* z, const float* drecon, const float* dafter,
                                          const t2s_vae_dec_grads* g, float* dz, int B, int L, int latent_w, void* stream) {
    return vae_decode_backward("t2s_vae_decode_backward_mc", true, h, z, drecon, dafter, g, dz, B, L, latent_w, stream);
}
