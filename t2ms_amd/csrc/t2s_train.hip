// Training step of the DiT for MI355X (reference train.py:101-127): forward that keeps the
// activations, hand-written backward for every trainable tensor, fused AdamW.
//
//   forward  (per block)  x_in -LN1,mod-> a1 -qkv-> q,k,v -attn-> o -proj-> p ; x_mid = x_in + g1 p
//                         x_mid -LN2,mod-> a2 -fc1-> u -gelu,fc2-> f ; x_out = x_mid + g2 f
//   backward (reverse)    gate/residual, fc2 (dgrad+wgrad), gelu', fc1, LN2/mod, proj, attention
//                         (dQ kernel + dK/dV kernel, P recomputed from the saved log-sum-exp), qkv,
//                         LN1/mod; then patchify, final layer and the adaLN linear.
//
// Round-1 design: correctness first, fp32 end to end, activations row-major.  Forward linears and
// every dgrad reuse gemm_rows_kernel (dgrad = the same kernel on transposed-packed weights);
// weight gradients are one MFMA kernel (A = dY^T, B = X straight from row-major global memory,
// contraction over token rows, fp32 atomics into the gradient); per-sequence reductions (adaLN
// shift / scale / gate gradients, LayerNorm backward) are deterministic one-workgroup-per-sequence
// kernels.  Parity: tests/test_hip_train.py against autograd through the CPU oracle and the
// reference-generated fixture tests/golden/train_step.npz.
#include <vector>

#include "t2s_wgrad.h"
#include "t2s_dit_internal.h"

using namespace t2s;

namespace t2s {
int attn_plain_train_fwd(const float* q, const float* k, const float* v, float* o_rows, float* lse, int BH, int n_tok,
                         hipStream_t st);
int attn_bwd(const float* q, const float* k, const float* v, const float* o_rows, const float* do_rows,
             const float* lse, float* dsum, float* dqkv_rows, int BH, int n_tok, hipStream_t st);
int attn16_train_fwd(const __bf16* q, const __bf16* k, const __bf16* v, __bf16* o_rows, float* lse, int BH, int n_tok, hipStream_t st);
int attn16_bwd(const __bf16* q, const __bf16* k, const __bf16* v, const __bf16* o_rows, const __bf16* do_rows,
               const float* lse, float* dsum, __bf16* dqkv_rows, int BH, int n_tok, hipStream_t st);
int f32_to_bf16(const float* src, __bf16* dst, size_t n, float scale, hipStream_t st);   // t2s_attn_bf16.hip
}

// ------------------------------------------------------------------ workspace
struct t2s_train_ws {
    int cap_seqs = 0;
    int dtype = 0;        // T2S_TRAIN_F32 / T2S_TRAIN_BF16 this workspace was laid out for
    int S = 0;            // sequences of the last forward
    int latw = LATW;      // the handle's latent width: a sequence is ntok() = 16 W tokens, a latent lat_elems() = 64 W values
    int ntok() const { return 16 * latw; }
    int lat_elems() const { return LATC * latw; }
    // ---- both arithmetics, all fp32, pieces of `act` (carve_act): the residual stream, the statistics, the conditioning and
    // what the backward keeps in fp32
    float* act = nullptr;
    float *x_in[NBLK + 1], *x_mid[NBLK], *lse[NBLK];
    float *silu_c = nullptr, *mod = nullptr, *c = nullptr, *lat = nullptr;   // (S,128) (S,3072) (S,128) (S,64 W)
    float *dx = nullptr, *dsum = nullptr, *dmod = nullptr;
    float* t1 = nullptr;           // (S,768) dense slice of dmod for the adaLN weight gradient; f32: also the block backward's (M,128) temporary
    float* wg_scratch = nullptr;   // partial weight-gradient tiles (wgrad16 stage 1 -> stage 2)
    float* colpart = nullptr;      // bf16: (M/32, 3, 128) column-sum partials of the fused LayerNorm backward (BEPI_LNBWD)
    size_t wg_scratch_floats = 0;
    int n_cu = 0;
    // ---- what one arithmetic owns; only the sub-struct of `dtype` is carved
    template <class T>
    struct Branch {   // saved branch activations of every block
        T *a1[NBLK], *q[NBLK], *k[NBLK], *v[NBLK], *o[NBLK], *p[NBLK], *a2[NBLK], *u[NBLK], *f[NBLK];
    };
    struct F32 : Branch<float> {    // T2S_TRAIN_F32: the activations and temporaries are further pieces of `act`
        float* warena = nullptr;    // training packs, refreshed by every t2s_dit_train_forward (the other forward packs are the handle's)
        f32x4* fc2_f[NBLK];         // forward: fc2 tile-major (the handle keeps it in chunk order)
        BlockMats<f32x4*> wt[NBLK]; // dgrad:   W^T (K,N)
        float *t2a = nullptr, *t2b = nullptr, *t3 = nullptr, *t4 = nullptr;   // (M,256) (M,256) (M,384) (M,128)
    } f32;
    struct BF16 : Branch<__bf16> {  // T2S_TRAIN_BF16: bf16 packs, activations and temporaries in arenas of their own
        __bf16* warena = nullptr;   // refreshed by every t2s_dit_train_forward
        BlockMats<bf16x8*> w[NBLK], wt[NBLK];   // forward: W (N,K); dgrad: W^T (K,N)
        __bf16* act = nullptr;
        __bf16 *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *t4 = nullptr;   // (M,128) (M,256) (M,384) (M,128)
    } bf;
};

namespace {

// W (N,K) row-major -> packed_index order of W (transpose=0) or of W^T (K,N) (transpose=1)
__global__ void pack_any_kernel(const float* __restrict__ W, float* __restrict__ P, int N, int K, int transpose) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * K) return;
    const int n = idx / K, k = idx - n * K;
    if (!transpose)
        P[packed_index(n, k, K)] = W[idx];
    else
        P[packed_index(k, n, N)] = W[idx];   // W^T is (K rows, N cols)
}

int pack_any(const float* W, f32x4* P, int N, int K, int transpose, hipStream_t st) {
    pack_any_kernel<<<(N * K + 255) / 256, 256, 0, st>>>(W, reinterpret_cast<float*>(P), N, K, transpose);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// ---------------------------------------------------------------- elementwise / per-sequence kernels
// float4-granular access to a branch tensor stored as fp32 (T2S_TRAIN_F32) or bf16 (T2S_TRAIN_BF16)
__device__ __forceinline__ f32x4 ld4(const float* p, size_t i4) { return reinterpret_cast<const f32x4*>(p)[i4]; }
__device__ __forceinline__ f32x4 ld4(const __bf16* p, size_t i4) { return unpack4(reinterpret_cast<const bf16x4*>(p)[i4]); }
__device__ __forceinline__ void st4(float* p, size_t i4, f32x4 v) { reinterpret_cast<f32x4*>(p)[i4] = v; }
__device__ __forceinline__ void st4(__bf16* p, size_t i4, f32x4 v) { reinterpret_cast<bf16x4*>(p)[i4] = pack4(v); }

// Geometry of the kernels below: W = 30 bakes the latent width in (the 480-token step), W = 0 takes it from latw_rt
// (800 / 1024 tokens).  Token n = hh * 32 + ww owns the 2x2 patch lat[2ww+j][2hh+i] at every width.
// x_out = x_in + gate[seq] * f      (rows of 128)
template <int W, typename T>
__global__ __launch_bounds__(256) void gate_res_kernel(const float* __restrict__ xin, const T* __restrict__ f,
                                                       const float* __restrict__ mod, int gate_off,
                                                       float* __restrict__ xout, int M, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // float4 index
    if (idx >= M * 32) return;
    const int row = idx >> 5, c4 = idx & 31;
    const int seq = row / ntok;
    const f32x4 g = *reinterpret_cast<const f32x4*>(mod + (size_t)seq * MODROW + gate_off + c4 * 4);
    const f32x4 a = reinterpret_cast<const f32x4*>(xin)[idx];
    const f32x4 b = ld4(f, idx);
    reinterpret_cast<f32x4*>(xout)[idx] = a + g * b;
}

// one workgroup per sequence: t = gate * dx ; dgate[seq] = sum_tok dx * f
template <int W, typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ dx, const T* __restrict__ f,
                                                       const float* __restrict__ mod, int gate_off,
                                                       T* __restrict__ t, float* __restrict__ dmod, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw;
    __shared__ f32x4 red[8][32];
    const int seq = blockIdx.x;
    const int c4 = threadIdx.x & 31, rg = threadIdx.x >> 5;   // 8 row groups
    const f32x4 g = *reinterpret_cast<const f32x4*>(mod + (size_t)seq * MODROW + gate_off + c4 * 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int tok = rg; tok < ntok; tok += 8) {
        const size_t idx = ((size_t)seq * ntok + tok) * 32 + c4;
        const f32x4 d = reinterpret_cast<const f32x4*>(dx)[idx];
        const f32x4 fv = ld4(f, idx);
        st4(t, idx, g * d);
        acc += d * fv;
    }
    red[rg][c4] = acc;
    __syncthreads();
    if (rg == 0) {
        f32x4 s = red[0][c4];
#pragma unroll
        for (int i = 1; i < 8; ++i) s += red[i][c4];
        *reinterpret_cast<f32x4*>(dmod + (size_t)seq * MODROW + gate_off + c4 * 4) = s;
    }
}

// one workgroup per sequence.  da = grad wrt modulate(LN(x)); computes
//   dshift = sum_tok da, dscale = sum_tok da * n, dn = da * (1 + scale),
//   dx += rstd * (dn - mean(dn) - n * mean(dn * n))          (LayerNorm backward, eps 1e-6, no affine)
// and, when f_next != NULL, the gate backward of the branch that is differentiated next
// (gate_bwd_kernel) on the dx it has just produced: t_next = gate_next * dx, dgate_next = sum_tok dx * f_next
// -- that saves one read of the fp32 gradient stream per branch.
template <int W, typename T>
__global__ __launch_bounds__(256) void ln_mod_bwd_kernel(const T* __restrict__ da, const float* __restrict__ x,
                                                         const float* __restrict__ mod, int shift_off, int scale_off,
                                                         float* __restrict__ dx, float* __restrict__ dmod,
                                                         const T* __restrict__ f_next, int gate_next_off,
                                                         T* __restrict__ t_next, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw;
    __shared__ f32x4 red[3][8][32];
    const int seq = blockIdx.x;
    const int c4 = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(mod + (size_t)seq * MODROW + scale_off + c4 * 4);
    f32x4 gn = {0.f, 0.f, 0.f, 0.f};
    if (f_next != nullptr) gn = *reinterpret_cast<const f32x4*>(mod + (size_t)seq * MODROW + gate_next_off + c4 * 4);
    f32x4 a_sh = {0.f, 0.f, 0.f, 0.f}, a_sc = {0.f, 0.f, 0.f, 0.f}, a_gt = {0.f, 0.f, 0.f, 0.f};
    for (int tok = rg; tok < ntok; tok += 8) {
        const size_t idx = ((size_t)seq * ntok + tok) * 32 + c4;
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
        const f32x4 g = ld4(da, idx);
        float s = (xv.x + xv.y) + (xv.z + xv.w);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s * (1.0f / 128.0f);
        const f32x4 d = xv - mean;
        float ss = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float rstd = rsqrtf(ss * (1.0f / 128.0f) + 1e-6f);
        const f32x4 n = d * rstd;
        a_sh += g;
        a_sc += g * n;
        const f32x4 dn = g * (1.0f + sc);
        float m1 = (dn.x + dn.y) + (dn.z + dn.w);
        float m2 = (dn.x * n.x + dn.y * n.y) + (dn.z * n.z + dn.w * n.w);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            m1 += __shfl_xor(m1, o, 64);
            m2 += __shfl_xor(m2, o, 64);
        }
        m1 *= (1.0f / 128.0f);
        m2 *= (1.0f / 128.0f);
        const f32x4 r = reinterpret_cast<const f32x4*>(dx)[idx] + (dn - m1 - n * m2) * rstd;
        reinterpret_cast<f32x4*>(dx)[idx] = r;
        if (f_next != nullptr) {
            st4(t_next, idx, gn * r);
            a_gt += r * ld4(f_next, idx);
        }
    }
    red[0][rg][c4] = a_sh;
    red[1][rg][c4] = a_sc;
    red[2][rg][c4] = a_gt;
    __syncthreads();
    if (rg < 3) {
        if (rg == 2 && f_next == nullptr) return;
        f32x4 s = red[rg][0][c4];
#pragma unroll
        for (int i = 1; i < 8; ++i) s += red[rg][i][c4];
        const int off = rg == 0 ? shift_off : (rg == 1 ? scale_off : gate_next_off);
        *reinterpret_cast<f32x4*>(dmod + (size_t)seq * MODROW + off + c4 * 4) = s;
    }
}

__global__ __launch_bounds__(256) void gelu_kernel(const float* __restrict__ u, float* __restrict__ out, size_t n4) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    f32x4 v = reinterpret_cast<const f32x4*>(u)[idx];
    v.x = gelu_tanh(v.x); v.y = gelu_tanh(v.y); v.z = gelu_tanh(v.z); v.w = gelu_tanh(v.w);
    reinterpret_cast<f32x4*>(out)[idx] = v;
}

__global__ __launch_bounds__(256) void silu_kernel(const float* __restrict__ c, float* __restrict__ out, int n) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float v = c[idx];
    out[idx] = v / (1.0f + __expf(-v));
}

// out[n] += sum_rows Y[row][n]   (N <= 3072, N % 4 == 0); slab of rows per workgroup, fp32 atomics
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ Y, float* __restrict__ out, int M, int N,
                                                     int rows_per_wg) {
    const int r0 = blockIdx.x * rows_per_wg;
    const int r1 = min(M, r0 + rows_per_wg);
    for (int n = threadIdx.x; n < N; n += 256) {
        float acc = 0.f;
        for (int r = r0; r < r1; ++r) acc += Y[(size_t)r * N + n];
        atomicAdd(out + n, acc);
    }
}

// Rows per workgroup of the two "tail" backward kernels below.  Their small gradients are reduced in the workgroup and
// written as ONE partial row per workgroup (FINAL_COLS / PATCH_COLS floats); tail_reduce_kernel then adds the partial
// rows in workgroup order -- deterministic, and without the ~800 K same-address fp32 atomics the round-1 kernels
// flushed with (they were most of these kernels' 0.3 ms each at B=1152).
constexpr int TAIL_ROWS = 256;
constexpr int FINAL_COLS = 772;   // ln.weight 128 | ln.bias 128 | linear_emb_to_patch.weight 4x128 | .bias 4
constexpr int PATCH_COLS = 660;   // patch_emb.weight 128x4 | .bias 128 | conv.weight 16 | conv.bias 4

struct TailDst { float* p[4]; int n[4]; };   // consecutive column ranges of a partial row -> gradient tensors
// grid = cols / 32 workgroups of 32 columns x 8 row slices: slice j adds partial rows j, j+8, ... (independent loads, many in
// flight), then the 8 slice sums are added in slice order.  (One thread per column walking all ~1000 rows serially paid a
// full memory latency per row: 260 us.)
__global__ __launch_bounds__(256) void tail_reduce_kernel(const float* __restrict__ part, int n_wg, int cols, int stride, const TailDst d) {
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s = 0.f;
    if (c < cols) {
#pragma unroll 8
        for (int w = sl; w < n_wg; w += 8) s += part[(size_t)w * stride + c];
    }
    red[sl][cl] = s;
    __syncthreads();
    if (sl != 0 || c >= cols) return;
#pragma unroll
    for (int j = 1; j < 8; ++j) s += red[j][cl];
    int off = c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (off < d.n[i]) { d.p[i][off] = s; return; }
        off -= d.n[i];
    }
}

// dgate of the last block's MLP branch from the fused final-layer backward: the workgroup partials of a sequence, added in
// workgroup order -- PPS = 3 of them at 480 tokens, PPS = 0: pps_rt (5 at 800, 8 at 1024; fused_rows below)
template <int PPS>
__global__ void final_gate_reduce_kernel(const float* __restrict__ part, int stride, float* __restrict__ dmod, int gate_off, int pps_rt) {
    const int pps = PPS ? PPS : pps_rt;
    const int seq = blockIdx.x, f = threadIdx.x;
    const float* p = part + (size_t)seq * pps * stride + FINAL_COLS + f;
    float s = p[0];
#pragma unroll
    for (int k = 1; k < pps; ++k) s += p[(size_t)k * stride];
    dmod[(size_t)seq * MODROW + gate_off + f] = s;
}
// Rows per workgroup of the fused final-layer backward: a whole fraction of a sequence (a workgroup reads ONE gate row and
// its dgate partial belongs to one sequence) and a multiple of 32 (final_bwd_kernel's row groups).  160 = 480 / 3 = 800 / 5;
// 1024 is no multiple of 160: 128 = 1024 / 8.
constexpr int fused_rows(int ntok) { return ntok % 160 == 0 ? 160 : 128; }
static_assert(NTOK % fused_rows(NTOK) == 0 && 800 % fused_rows(800) == 0 && 1024 % fused_rows(1024) == 0, "whole workgroups per sequence");

// final layer backward (transformer.py:182-191): dout (S,64,W) -> dx (M,128) and grads of
// ln.weight, ln.bias, linear_emb_to_patch.{weight,bias}.  32 lanes per token row.
// FUSED (bf16 training): the layer input x_mid + gate * f of the last block is formed here instead of being read back
// (the forward never writes it), and the gate backward of that MLP branch runs on the dx just produced: t = gate * dx
// (bf16 rows), dgate partial = sum over this workgroup's rows of dx * f in columns FINAL_COLS.. of its partial row.
// FUSED workgroups own ROWS = fused_rows(tokens) rows = a whole fraction of a sequence (160 = a third at 480 tokens), so that
// many consecutive partial rows make one sequence.
template <bool FUSED, int ROWS, int W>
__global__ __launch_bounds__(256) void final_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                        const float* __restrict__ lng, const float* __restrict__ lnb,
                                                        const float* __restrict__ ow, float* __restrict__ dx,
                                                        float* __restrict__ part, int M, const __bf16* __restrict__ f,
                                                        const float* __restrict__ mod, int gate_off, __bf16* __restrict__ t, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw, lat = LATC * latw;
    constexpr int PCOLS = FUSED ? FINAL_COLS + D : FINAL_COLS;
    __shared__ f32x4 red[FUSED ? 7 : 6][8][32];
    __shared__ float redb[8][4];
    const int c4 = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const f32x4 gam = *reinterpret_cast<const f32x4*>(lng + c4 * 4);
    const f32x4 bet = *reinterpret_cast<const f32x4*>(lnb + c4 * 4);
    f32x4 w[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) w[p] = *reinterpret_cast<const f32x4*>(ow + p * D + c4 * 4);
    f32x4 a_g = {0, 0, 0, 0}, a_b = {0, 0, 0, 0}, a_w[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    float a_ob[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 a_gt = {0, 0, 0, 0}, gt = {0, 0, 0, 0};
    const int row0 = blockIdx.x * ROWS;
    if constexpr (FUSED) gt = *reinterpret_cast<const f32x4*>(mod + (size_t)(row0 / ntok) * MODROW + gate_off + c4 * 4);
    static_assert(ROWS % 32 == 0, "8 row groups x 4 rows in flight");
    for (int it0 = 0; it0 < ROWS / 8; it0 += 4) {      // 4 rows per 32-lane group in flight: loads first, then the chains
        f32x4 xv4[4], fv4[4];
        float dl4[4][4];
        bool valid4[4];
        size_t idx4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = rg + 8 * (it0 + u);
            valid4[u] = row0 + rr < M;                      // rows past the end: clamped, their contributions masked
            const int row = valid4[u] ? row0 + rr : M - 1;
            idx4[u] = (size_t)row * 32 + c4;
            xv4[u] = reinterpret_cast<const f32x4*>(x)[idx4[u]];
            if constexpr (FUSED) {
                fv4[u] = ld4(f, idx4[u]);
                xv4[u] = xv4[u] + gt * fv4[u];              // the expression of gate_res_kernel
            }
            // gather d(lin)[p] from the unpatchified output gradient
            const int seq = row / ntok, tok = row - seq * ntok;
            const int hh = tok >> 5, ww = tok & 31;
            const float keep = valid4[u] ? 1.f : 0.f;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                dl4[u][p] = keep * dout[(size_t)seq * lat + (2 * ww + (p & 1)) * latw + 2 * hh + (p >> 1)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x4 xv = xv4[u];
            float s = (xv.x + xv.y) + (xv.z + xv.w);
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
            const float mean = s * (1.0f / 128.0f);
            const f32x4 d = xv - mean;
            float ss = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
            const float rstd = rsqrtf(ss * (1.0f / 128.0f) + 1e-5f);
            const f32x4 n = d * rstd;
            const f32x4 y = n * gam + bet;
            f32x4 dy = {0, 0, 0, 0};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                dy += w[p] * dl4[u][p];
                a_w[p] += y * dl4[u][p];
                a_ob[p] += dl4[u][p];
            }
            a_g += dy * n;
            a_b += dy;
            const f32x4 dn = dy * gam;
            float m1 = (dn.x + dn.y) + (dn.z + dn.w);
            float m2 = (dn.x * n.x + dn.y * n.y) + (dn.z * n.z + dn.w * n.w);
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) {
                m1 += __shfl_xor(m1, o, 64);
                m2 += __shfl_xor(m2, o, 64);
            }
            m1 *= (1.0f / 128.0f);
            m2 *= (1.0f / 128.0f);
            const f32x4 r = (dn - m1 - n * m2) * rstd;
            if (valid4[u]) reinterpret_cast<f32x4*>(dx)[idx4[u]] = r;
            if constexpr (FUSED) {
                if (valid4[u]) st4(t, idx4[u], gt * r);
                a_gt += (valid4[u] ? 1.f : 0.f) * (r * fv4[u]);
            }
        }
    }
    red[0][rg][c4] = a_g;
    red[1][rg][c4] = a_b;
#pragma unroll
    for (int p = 0; p < 4; ++p) red[2 + p][rg][c4] = a_w[p];
    if constexpr (FUSED) red[6][rg][c4] = a_gt;
    if (c4 == 0)
#pragma unroll
        for (int p = 0; p < 4; ++p) redb[rg][p] = a_ob[p];
    __syncthreads();
    if (rg < 6) {
        f32x4 s = red[rg][0][c4];
#pragma unroll
        for (int i = 1; i < 8; ++i) s += red[rg][i][c4];
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * PCOLS + rg * D + c4 * 4) = s;   // lnw | lnb | ow[p]
    } else if (rg == 6) {
        if (c4 < 4) {
            float s = 0.f;
            for (int i = 0; i < 8; ++i) s += redb[i][c4];
            part[(size_t)blockIdx.x * PCOLS + 6 * D + c4] = s;
        }
    } else if constexpr (FUSED) {
        f32x4 s = red[6][0][c4];
#pragma unroll
        for (int i = 1; i < 8; ++i) s += red[6][i][c4];
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * PCOLS + FINAL_COLS + c4 * 4) = s;   // dgate partial
    }
}

// patchify backward (transformer.py:166-172): dtok (M,128) -> grads of patch_emb.{weight,bias}, conv.{weight,bias}.
// With g = dtok row, px = the token's 2x2 latent patch, cv = conv(px):
//   d patch_emb.weight[d][c] = sum_rows g[d] cv[c] = sum_ij conv.w[c][ij] G[d][ij] + conv.b[c] PB[d]
//   d conv.weight[c][ij]     = sum_rows (sum_d g[d] Wpe[d][c]) px[ij] = sum_d Wpe[d][c] G[d][ij],   d conv.bias[c] = sum_d Wpe[d][c] PB[d]
// where G[d][ij] = sum_rows g[d] px[ij] and PB[d] = sum_rows g[d]: the row loop only accumulates G and PB (20 FMAs per
// lane and row, no cross-lane step) and the contractions with the weights run once per workgroup.
template <int W>
__global__ __launch_bounds__(256) void patchify_bwd_kernel(const float* __restrict__ dtok, const float* __restrict__ lat,
                                                           int B, const float* __restrict__ cw, const float* __restrict__ cb,
                                                           const float* __restrict__ pw, float* __restrict__ part, int M, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw, lat_n = LATC * latw;
    __shared__ f32x4 red[5][8][32];
    __shared__ float Gs[4][D], PBs[D];
    const int c4 = threadIdx.x & 31, rg = threadIdx.x >> 5;
    f32x4 G[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // [ij] over the lane's 4 features
    f32x4 a_pb = {0, 0, 0, 0};
    const int row0 = blockIdx.x * TAIL_ROWS;
    for (int it0 = 0; it0 < TAIL_ROWS / 8; it0 += 4) {
        f32x4 g4[4];
        float px4[4][4];   // [u][i*2+j] = in[2hh+i][2ww+j]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = rg + 8 * (it0 + u);
            const bool valid = row0 + rr < M;
            const int row = valid ? row0 + rr : M - 1;
            g4[u] = reinterpret_cast<const f32x4*>(dtok)[(size_t)row * 32 + c4];
            if (!valid) g4[u] = g4[u] * 0.f;
            const int seq = row / ntok, tok = row - seq * ntok;
            const int hh = tok >> 5, ww = tok & 31;
            const float* xin = lat + (size_t)(seq % B) * lat_n;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) px4[u][i * 2 + jj] = xin[(2 * ww + jj) * latw + 2 * hh + i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ij = 0; ij < 4; ++ij) G[ij] += g4[u] * px4[u][ij];
            a_pb += g4[u];
        }
    }
#pragma unroll
    for (int ij = 0; ij < 4; ++ij) red[ij][rg][c4] = G[ij];
    red[4][rg][c4] = a_pb;
    __syncthreads();
    if (rg < 5) {
        f32x4 s = red[rg][0][c4];
#pragma unroll
        for (int i = 1; i < 8; ++i) s += red[rg][i][c4];
        if (rg < 4) *reinterpret_cast<f32x4*>(&Gs[rg][c4 * 4]) = s;
        else *reinterpret_cast<f32x4*>(&PBs[c4 * 4]) = s;
    }
    __syncthreads();
    float* prow = part + (size_t)blockIdx.x * PATCH_COLS;
    if (rg < 4) {   // patch_emb.weight[d][c], d = 4*c4+e, c = rg
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = c4 * 4 + e;
            float acc = cw[rg * 4] * Gs[0][d];
            acc += cw[rg * 4 + 1] * Gs[1][d];
            acc += cw[rg * 4 + 2] * Gs[2][d];
            acc += cw[rg * 4 + 3] * Gs[3][d];
            prow[d * 4 + rg] = acc + cb[rg] * PBs[d];
        }
    } else if (rg == 4) {
        *reinterpret_cast<f32x4*>(prow + 512 + c4 * 4) = *reinterpret_cast<const f32x4*>(&PBs[c4 * 4]);
    } else if (rg == 5 && c4 < 20) {   // conv.weight[c][ij] (16) | conv.bias[c] (4): one thread per output, d in order
        const int c = c4 < 16 ? c4 >> 2 : c4 - 16;
        const float* src = c4 < 16 ? Gs[c4 & 3] : PBs;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += pw[d * 4 + c] * src[d];
        prow[640 + c4] = acc;
    }
}

// fused AdamW (torch.optim.AdamW semantics, decoupled weight decay, bias-corrected moments)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pv = p[i];
    const float gv = g[i];
    pv *= 1.0f - lr * wd;
    const float mv = b1 * m[i] + (1.0f - b1) * gv;
    const float vv = b2 * v[i] + (1.0f - b2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] = pv - (lr / bc1) * mv / denom;
}

// the same update for a whole parameter list in ONE launch: workgroup b handles chunk (b - first[t]) of tensor t,
// t found by a short scan of the (<= 64 entry) table staged in LDS
__global__ __launch_bounds__(256) void adamw_multi_kernel(const t2s_adamw_tensor* __restrict__ tab, int n_tensors, float lr,
                                                          float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
    __shared__ unsigned int first[65];
    __shared__ t2s_adamw_tensor ent;
    if (threadIdx.x == 0) {
        unsigned int acc = 0;
        int t = 0;
        for (; t < n_tensors; ++t) {
            const unsigned int nb = (unsigned int)((tab[t].n + 1023) / 1024);
            if (blockIdx.x < acc + nb) break;
            acc += nb;
        }
        first[0] = acc;
        ent = tab[t < n_tensors ? t : n_tensors - 1];
    }
    __syncthreads();
    const size_t base = (size_t)(blockIdx.x - first[0]) * 1024;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const size_t i = base + threadIdx.x + 256 * u;
        if (i >= ent.n) return;
        float pv = ent.param[i];
        const float gv = ent.grad[i];
        pv *= 1.0f - lr * wd;
        const float mv = b1 * ent.exp_avg[i] + (1.0f - b1) * gv;
        const float vv = b2 * ent.exp_avg_sq[i] + (1.0f - b2) * gv * gv;
        ent.exp_avg[i] = mv;
        ent.exp_avg_sq[i] = vv;
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        ent.param[i] = pv - (lr / bc1) * mv / denom;
    }
}

__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ gout, float* __restrict__ da, size_t n,
                                                      float sign) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    da[i] = sign * 2.0f * (a[i] - b[i]) * (gout[0] / (float)n);
}

// c = temb (+ text)   (transformer.py:176-178)
__global__ void cond_rows_kernel(float* __restrict__ c, const float* __restrict__ temb, int temb_rows,
                                 const float* __restrict__ text, int S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * D) return;
    const int s = idx >> 7, d = idx & 127;
    float val = temb[(size_t)(temb_rows == 1 ? 0 : s) * D + d];
    if (text) val += text[idx];
    c[idx] = val;
}

// patchify, row-major output (transformer.py:166-172)
template <int W>
__global__ __launch_bounds__(256) void patchify_rows_kernel(const float* __restrict__ x, float* __restrict__ h, int S,
                                                            const float* __restrict__ cw, const float* __restrict__ cb,
                                                            const float* __restrict__ pw, const float* __restrict__ pb,
                                                            const float* __restrict__ pos, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw, lat = LATC * latw;
    // one thread = 4 features of token n for FOUR series: the weights, bias and position row are loaded once per thread
    // and the four 16-byte stores are independent (one series per thread ran at 2.6 TB/s of pure stores)
    constexpr int SPT = 4;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = gid & 31, rest = gid >> 5;
    const int sg = rest / ntok, n = rest - sg * ntok;
    if (sg * SPT >= S) return;
    const int hh = n >> 5, ww = n & 31;
    f32x4 w[4], bias, posr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int d = c4 * 4 + e;
        w[e] = *reinterpret_cast<const f32x4*>(pw + d * 4);
        bias[e] = pb[d];
        posr[e] = pos[n * D + d];
    }
    float px[SPT][4];
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const int s = sg * SPT + u < S ? sg * SPT + u : S - 1;
        const float* xin = x + (size_t)s * lat;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) px[u][i * 2 + j] = xin[(2 * ww + j) * latw + 2 * hh + i];
    }
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const int s = sg * SPT + u;
        float cv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float acc = cw[c * 4 + 0] * px[u][0];
            acc += cw[c * 4 + 1] * px[u][1];
            acc += cw[c * 4 + 2] * px[u][2];
            acc += cw[c * 4 + 3] * px[u][3];
            cv[c] = acc + cb[c];
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = w[e].x * cv[0];
            acc += w[e].y * cv[1];
            acc += w[e].z * cv[2];
            acc += w[e].w * cv[3];
            o[e] = acc + bias[e] + posr[e];
        }
        if (s < S) reinterpret_cast<f32x4*>(h)[((size_t)s * ntok + n) * 32 + c4] = o;
    }
}

// gradient of patchify with respect to the LATENT (transformer.py:166-172 backwards): token n = hh*32 + ww owns the 2x2 patch
// lat[2ww+j][2hh+i]; dcv[c] = sum_d dx[tok][d] patch_w[d][c]; dlat[2ww+j][2hh+i] = sum_c conv_w[c][i][j] dcv[c].  Every latent
// element belongs to exactly one token: plain stores.  Needed only when something upstream of the latent trains
// (train.py:31-33 with the LA-VAE encoder un-frozen).
template <int W>
__global__ __launch_bounds__(256) void patchify_input_grad_kernel(const float* __restrict__ dx, float* __restrict__ dlat, int S,
                                                                  const float* __restrict__ cw, const float* __restrict__ pw, int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw, lat = LATC * latw;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= S * ntok) return;
    const int s = gid / ntok, n = gid - s * ntok;
    const int hh = n >> 5, ww = n & 31;
    const f32x4* row = reinterpret_cast<const f32x4*>(dx + (size_t)gid * D);
    float dcv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int d4 = 0; d4 < D / 4; ++d4) {
        const f32x4 g = row[d4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(pw + (d4 * 4 + e) * 4);
            dcv[0] += g[e] * w.x; dcv[1] += g[e] * w.y; dcv[2] += g[e] * w.z; dcv[3] += g[e] * w.w;
        }
    }
    float* out = dlat + (size_t)s * lat;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc += cw[c * 4 + i * 2 + j] * dcv[c];
            out[(2 * ww + j) * latw + 2 * hh + i] = acc;
        }
}

// final layer, row-major input (transformer.py:182-191)
// f != NULL (bf16 training): the layer input is x_mid + gate * f of the last block, formed here (gate_res_kernel's expression)
template <int W>
__global__ __launch_bounds__(256) void final_rows_kernel(const float* __restrict__ h, int S, const float* __restrict__ lnw,
                                                         const float* __restrict__ lnb, const float* __restrict__ ow,
                                                         const float* __restrict__ ob, float* __restrict__ out,
                                                         const __bf16* __restrict__ f, const float* __restrict__ mod, int gate_off,
                                                         int latw_rt) {
    const int latw = W ? W : latw_rt, ntok = 16 * latw, lat = LATC * latw;
    // 32 lanes per token row, FOUR rows per group in flight: a row is 3 dependent butterfly reductions (mean, variance,
    // the four output dots) and one row per group left the kernel latency-bound at 2.7 TB/s
    constexpr int RPG = 4;
    const int c4 = threadIdx.x & 31;
    const int grp = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const int M = S * ntok;
    const f32x4 gam = *reinterpret_cast<const f32x4*>(lnw + c4 * 4), bet = *reinterpret_cast<const f32x4*>(lnb + c4 * 4);
    f32x4 w[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) w[p] = *reinterpret_cast<const f32x4*>(ow + p * D + c4 * 4);
    f32x4 v[RPG];
    int tok[RPG];
#pragma unroll
    for (int u = 0; u < RPG; ++u) {
        tok[u] = grp * RPG + u;
        const int tk = tok[u] < M ? tok[u] : M - 1;
        v[u] = reinterpret_cast<const f32x4*>(h)[(size_t)tk * 32 + c4];
        if (f != nullptr) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(mod + (size_t)(tk / ntok) * MODROW + gate_off + c4 * 4);
            v[u] = v[u] + g * ld4(f, (size_t)tk * 32 + c4);
        }
    }
#pragma unroll
    for (int u = 0; u < RPG; ++u) {
        float s1 = (v[u].x + v[u].y) + (v[u].z + v[u].w);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) s1 += __shfl_xor(s1, o, 64);
        const float mean = s1 * (1.0f / 128.0f);
        const f32x4 d = v[u] - mean;
        float s2 = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) s2 += __shfl_xor(s2, o, 64);
        const float rstd = rsqrtf(s2 * (1.0f / 128.0f) + 1e-5f);
        const f32x4 y = (d * rstd) * gam + bet;
        float acc[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float a = (y.x * w[p].x + y.y * w[p].y) + (y.z * w[p].z + y.w * w[p].w);
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
            acc[p] = a + ob[p];
        }
        if (tok[u] < M && c4 < 4) {
            const int s = tok[u] / ntok, n = tok[u] - s * ntok;
            const int hh = n >> 5, ww = n & 31;
            out[(size_t)s * lat + (2 * ww + (c4 & 1)) * latw + 2 * hh + (c4 >> 1)] = acc[c4];
        }
    }
}

// ---------------------------------------------------------------- workspace management
// The layouts of the three training arenas (t2s_arena.h: written once, run to measure and to bind).
template <class Take>
void carve_weights(t2s_train_ws::F32& f, Take&& take) {
    for (int i = 0; i < NBLK; ++i)
        for (int j = 0; j < NMAT; ++j) {
            if (j == FC2) take(f.fc2_f[i], mat_elems(j));
            take(f.wt[i][j], mat_elems(j));
        }
}
template <class Take>
void carve_weights(t2s_train_ws::BF16& b, Take&& take) {
    for (int i = 0; i < NBLK; ++i)
        for (int j = 0; j < NMAT; ++j) { take(b.w[i][j], mat_elems(j)); take(b.wt[i][j], mat_elems(j)); }
}
template <class T, class Take>
void carve_branch(t2s_train_ws::Branch<T>& a, int i, size_t M, Take&& take) {
    take(a.a1[i], M * D); take(a.q[i], M * D); take(a.k[i], M * D); take(a.v[i], M * D); take(a.o[i], M * D);
    take(a.p[i], M * D); take(a.a2[i], M * D); take(a.u[i], M * 2 * D); take(a.f[i], M * D);
}
// the fp32 arena: residual stream and statistics always; branch activations and temporaries only in fp32 mode
template <class Take>
void carve_act(t2s_train_ws* w, Take&& take) {
    const size_t S = (size_t)w->cap_seqs, M = S * w->ntok(), lat_n = w->lat_elems();
    const bool bf = w->dtype == T2S_TRAIN_BF16;
    for (int i = 0; i <= NBLK; ++i) take(w->x_in[i], M * D);
    for (int i = 0; i < NBLK; ++i) {
        take(w->x_mid[i], M * D);
        take(w->lse[i], M * NH);
        if (!bf) carve_branch(w->f32, i, M, take);
    }
    take(w->silu_c, S * D); take(w->mod, S * MODROW); take(w->c, S * D); take(w->lat, S * lat_n); take(w->dx, M * D);
    take(w->dsum, M * NH); take(w->dmod, S * MODROW);
    take(w->t1, bf ? S * MODW : M * D);
    take(w->wg_scratch, w->wg_scratch_floats);
    take(w->colpart, bf ? M / 32 * 384 : 64);
    if (!bf) { take(w->f32.t2a, M * 2 * D); take(w->f32.t2b, M * 2 * D); take(w->f32.t3, M * 3 * D); take(w->f32.t4, M * D); }
}
template <class Take>
void carve_act16(t2s_train_ws* w, Take&& take) {
    const size_t M = (size_t)w->cap_seqs * w->ntok();
    for (int i = 0; i < NBLK; ++i) carve_branch(w->bf, i, M, take);
    take(w->bf.t1, M * D); take(w->bf.t2, M * 2 * D); take(w->bf.t3, M * 3 * D); take(w->bf.t4, M * D);
}

// everything of a workspace laid out for w->cap_seqs sequences of w->dtype; a failure leaves what it allocated to train_free
int build_ws(t2s_train_ws* w) {
    auto oom = [](const char* what, size_t bytes) {
        set_error("t2s train: hipMalloc(%s, %.1f MB) failed", what, bytes / 1e6);
        return T2S_E_HIP;
    };
    const bool bf = w->dtype == T2S_TRAIN_BF16;
    size_t n = 0;
    // ---- packed weights (fp32 packs: fc2 tile-major + all W^T; bf16 packs: W and W^T of every linear)
    if (!bf) {
        if (carve_alloc(w->f32.warena, [&](auto& take) { carve_weights(w->f32, take); }, &n) != hipSuccess) return oom("packed weights", n * 4);
    } else {
        if (carve_alloc(w->bf.warena, [&](auto& take) { carve_weights(w->bf, take); }, &n) != hipSuccess) return oom("packed bf16 weights", n * 2);
    }
    {
        const int S = w->cap_seqs;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return oom("device query", 0);
        w->n_cu = prop.multiProcessorCount;
        w->wg_scratch_floats = wgrad16_scratch_floats(S * w->ntok(), w->n_cu);
        int rows, gx;                                            // the adaLN linear: M = S rows, (768,128)
        wgrad16_plan(S, MODW, D, w->n_cu, &rows, &gx);
        const size_t ada = (size_t)gx * (MODW / 128) * (128 * 128 + 128);
        if (ada > w->wg_scratch_floats) w->wg_scratch_floats = ada;
    }
    if (carve_alloc(w->act, [&](auto& take) { carve_act(w, take); }, &n) != hipSuccess) return oom("activations", n * 4);
    if (bf && carve_alloc(w->bf.act, [&](auto& take) { carve_act16(w, take); }, &n) != hipSuccess) return oom("bf16 activations", n * 2);
    return T2S_OK;
}

int ensure_ws(t2s_dit* h, int S) {
    const int dtype = h->train_dtype;
    if (h->train && h->train->cap_seqs >= S && h->train->dtype == dtype) return T2S_OK;
    t2s::train_free(h);
    t2s_train_ws* w = h->train = new t2s_train_ws();
    // Grow with 12.5 % headroom (within the handle's capacity): the length groups of a mix-train batch fluctuate by a few
    // per cent from step to step (train.py:60-87), and a workspace rebuilt at every new maximum costs a device-wide
    // hipFree + a multi-GB hipMalloc each time -- seconds in a long-lived process (found in round 4: train.py's loop at
    // 65-180 ms per 28 ms step).  Everything is sized for the capacity.
    const int want = (S + S / 8 + 63) / 64 * 64;
    w->cap_seqs = want < h->max_seqs ? want : (S > h->max_seqs ? S : h->max_seqs);
    w->dtype = dtype;
    w->latw = h->latw;
    const int rc = build_ws(w);
    if (rc != T2S_OK) t2s::train_free(h);
    return rc;
}

// the 32 bf16 weight packs of a training forward (4 blocks x 4 matrices x 2 orientations) in one launch: job table
// as a kernel argument, blockIdx.y = job (each single launch costs ~3 us against ~1 us of work)
struct Pack16Job {
    const float* W;
    __bf16* P;
    int N, K, transpose;
};
struct Pack16Table {
    Pack16Job j[8 * NBLK];
};
__global__ void pack16_multi_kernel(const Pack16Table t) {
    const Pack16Job& j = t.j[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= j.N * j.K) return;
    const int n = idx / j.K, k = idx - n * j.K;
    const size_t dst = j.transpose ? packed16_index(k, n, j.N) : packed16_index(n, k, j.K);
    j.P[dst] = (__bf16)j.W[idx];
}

// TOK: the tile -> (sequence, token) map of the kernels that need one (LayerNorm prologues, q / k / v heads), NTOK or 0 with
// `ntok` at run time -- as gemm<..., TOK> below
template <int K, int N, int PRO, int EPI, int TOK = NTOK>
int bgemm(const void* A, const bf16x8* Wp, const float* bias, __bf16* out, int M, int n_out, hipStream_t st,
          const float* mod = nullptr, int shift_off = 0, int scale_off = 0, __bf16* save_A = nullptr,
          const __bf16* aux = nullptr, __bf16* q = nullptr, __bf16* k = nullptr, __bf16* v = nullptr,
          const __bf16* res = nullptr, int gate_off = 0, float* x_out = nullptr, int ntok = NTOK) {
    BGemmArgs a{};
    a.A = A; a.Wp = Wp; a.bias = bias; a.out = out; a.M = M; a.N = n_out; a.mod = mod; a.shift_off = shift_off;
    a.scale_off = scale_off; a.save_A = save_A; a.aux = aux; a.q = q; a.k = k; a.v = v;
    a.res = res; a.gate_off = gate_off; a.x_out = x_out; a.tps = ntok / 32;
    return launch_bgemm<K, N, PRO, EPI, TOK>(a, st);
}

// data-gradient GEMM (M,K) x W^T -> (M,128) whose epilogue is the LayerNorm + modulate backward (BEPI_LNBWD), then the
// per-sequence column sums of its partials into dmod
template <int K, int TOK = NTOK>
int bgemm_lnbwd(t2s_train_ws* ws, const __bf16* dY, const bf16x8* Wt, const float* ln_x, int shift_off, int scale_off,
                const __bf16* f_next, int gate_next_off, __bf16* t_next, int M, hipStream_t st) {
    const int ntok = ws->ntok();
    BGemmArgs a{};
    a.A = dY; a.Wp = Wt; a.M = M; a.N = D; a.mod = ws->mod; a.shift_off = shift_off; a.scale_off = scale_off;
    a.res = f_next; a.gate_off = gate_next_off; a.out = t_next; a.ln_x = ln_x; a.dx = ws->dx; a.colpart = ws->colpart;
    a.tps = ntok / 32;
    int rc;
    if ((rc = launch_bgemm<K, 128, BPRO_BF16, BEPI_LNBWD, TOK>(a, st))) return rc;
    lnbwd_colsum_reduce_kernel<TOK / 32><<<M / ntok, f_next != nullptr ? 384 : 256, 0, st>>>(ws->colpart, ws->dmod, shift_off, scale_off, gate_next_off,
                                                                                              ntok / 32);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

template <int K, int NT, int PRO, int EPI, int TOK = NTOK>
int gemm(const float* A, const f32x4* Wp, const float* bias, float* out, int M, int N, hipStream_t st,
         const float* mod = nullptr, int shift_off = 0, int scale_off = 0, float* save_A = nullptr,
         const float* aux = nullptr, float* q = nullptr, float* k = nullptr, float* v = nullptr, int ntok = NTOK) {
    GemmArgs a{};
    a.ntok = ntok;
    a.A = A; a.Wp = Wp; a.bias = bias; a.out = out; a.M = M; a.N = N; a.mod = mod; a.shift_off = shift_off;
    a.scale_off = scale_off; a.save_A = save_A; a.aux = aux; a.q = q; a.k = k; a.v = v;
    return launch_gemm_rows<K, NT, PRO, EPI, TOK>(a, st);
}

// weight (and, if db != NULL, bias) gradient of a linear layer
int wgrad(t2s_train_ws* ws, const float* dY, const float* X, float* dW, float* db, int M, int N, int K, hipStream_t st) {
    return launch_wgrad32(dY, X, dW, db, M, N, K, ws->wg_scratch, ws->wg_scratch_floats, ws->n_cu, st);
}

int colsum(const float* Y, float* out, int M, int N, hipStream_t st) {
    const int rows_per_wg = 512;
    colsum_kernel<<<(M + rows_per_wg - 1) / rows_per_wg, 256, 0, st>>>(Y, out, M, N, rows_per_wg);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// A statement that names a kernel template's width parameter W, once per form: W = 30 for a width-30 handle (the compile-time
// 480-token step), W = 0 for any other (the width goes in as the kernel's last argument)
#define T2S_BY_WIDTH(latw_, ...)                                                               \
    do {                                                                                       \
        if ((latw_) == LATW) { constexpr int W = LATW; __VA_ARGS__; }                          \
        else { constexpr int W = 0; __VA_ARGS__; }                                             \
    } while (0)

// ---------------------------------------------------------------- the block recipes, one per arithmetic and direction
// (every launch is one timed interval: the class names what bench.py reports per step)
// Declared here and defined behind the entry point each was cut from: the compiler emits a template kernel where the source
// first asks for it, and the order of the kernels in the code object is part of what is measured.
int forward_blocks_bf16(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st);
int forward_blocks_f32(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st);
int backward_blocks_bf16(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st);
int backward_blocks_f32(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st);
// The run-time (800 / 1024-token) forms of the bf16 recipes and of the fused final-layer backward are first asked for at the
// END of this file, so that their kernels follow every kernel of the 480-token step in the code object.
int forward_blocks_bf16_wide(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st);
int backward_blocks_bf16_wide(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st);
int final_bwd_fused_wide(t2s_dit* h, t2s_train_ws* ws, const float* dout, int M, int S, int goff, int final_wgs, int final_stride, hipStream_t st);

}  // namespace

namespace t2s {
void train_free(t2s_dit* h) {
    if (!h || !h->train) return;
    t2s_train_ws* w = h->train;
    for (void* arena : {(void*)w->f32.warena, (void*)w->bf.warena, (void*)w->act, (void*)w->bf.act})   // (a half-built one too)
        if (arena) (void)hipFree(arena);
    delete w;
    h->train = nullptr;
}
}  // namespace t2s

// ------------------------------------------------------------------ C ABI
extern "C" {

int t2s_dit_set_train_dtype(t2s_dit* h, int dtype) {
    T2S_REQUIRE(h, "t2s_dit_set_train_dtype: NULL handle");
    T2S_REQUIRE(h->latw == LATW || h->trainable, "t2s_dit_set_train_dtype: training runs at latent width 30 only, this handle has %d", h->latw);
    T2S_REQUIRE(dtype == T2S_TRAIN_F32 || dtype == T2S_TRAIN_BF16, "t2s_dit_set_train_dtype: unknown dtype %d", dtype);
    T2S_REQUIRE(h->latw == LATW || dtype == T2S_TRAIN_F32 || h->wide_train_bf16,
                "t2s_dit_set_train_dtype: a handle of latent width %d trains in T2S_TRAIN_F32 only (T2S_TRAIN_BF16 exists at width 30)", h->latw);
    h->train_dtype = dtype;
    return T2S_OK;
}

// include/t2s_wide_train_bf16.h
int t2s_dit_set_wide_train_bf16(t2s_dit* h, int on) {
    T2S_REQUIRE(h, "t2s_dit_set_wide_train_bf16: NULL handle");
    if (h->latw == LATW) return T2S_OK;   // (a width-30 handle has always had both arithmetics)
    h->wide_train_bf16 = on != 0;
    if (!h->wide_train_bf16 && h->train_dtype == T2S_TRAIN_BF16) h->train_dtype = T2S_TRAIN_F32;   // (ensure_ws rebuilds on the dtype change)
    return T2S_OK;
}

int t2s_dit_set_trainable(t2s_dit* h, int on) {
    T2S_REQUIRE(h, "t2s_dit_set_trainable: NULL handle");
    if (h->latw != LATW) h->trainable = on != 0;   // (a width-30 handle always trains)
    return T2S_OK;
}

int t2s_dit_train_forward(t2s_dit* h, const t2s_dit_weights* w, const float* x, const float* temb, int temb_rows,
                          const float* text, float* out, int B, void* stream) {
    t2s::reset_tile_dir();
    T2S_REQUIRE(h && w && x && temb && out, "t2s_dit_train_forward: NULL argument");
    T2S_REQUIRE(h->latw == LATW || h->trainable, "t2s_dit_train_forward: training runs at latent width 30 only, this handle has %d", h->latw);
    T2S_REQUIRE(B > 0 && B <= h->max_seqs, "t2s_dit_train_forward: B=%d exceeds max_seqs=%d", B, h->max_seqs);
    T2S_REQUIRE(temb_rows == 1 || temb_rows == B, "t2s_dit_train_forward: temb_rows=%d", temb_rows);
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_ws(h, B);
    if (rc != T2S_OK) return rc;
    t2s_train_ws* ws = h->train;
    const int ntok = h->ntok();
    const int S = B, M = S * ntok;
    T2S_REQUIRE(ws->dtype == T2S_TRAIN_F32 || h->latw == LATW || h->wide_train_bf16,
                "t2s_dit_train_forward: a handle of latent width %d trains in T2S_TRAIN_F32 only", h->latw);
    ws->S = S;
    // the handle's own parameter copies / forward packs must be current: the caller refreshes them
    // with t2s_dit_update_weights; here only the training-specific packs
    const bool bf = ws->dtype == T2S_TRAIN_BF16;
    if (!bf) {       // fc2 tile-major, all W^T
        for (int i = 0; i < NBLK; ++i)
            for (int j = 0; j < NMAT; ++j) {
                const float* W = mat_w(w->blk[i], j);
                if (j == FC2 && (rc = pack_any(W, ws->f32.fc2_f[i], MAT_N[j], MAT_K[j], 0, st))) return rc;
                if ((rc = pack_any(W, ws->f32.wt[i][j], MAT_N[j], MAT_K[j], 1, st))) return rc;
            }
    } else {         // bf16 copies of the fp32 master weights, both orientations
        Pack16Table pt{};
        int np = 0;
        for (int i = 0; i < NBLK; ++i)
            for (int j = 0; j < NMAT; ++j) {
                pt.j[np++] = Pack16Job{mat_w(w->blk[i], j), reinterpret_cast<__bf16*>(ws->bf.w[i][j]), MAT_N[j], MAT_K[j], 0};
                pt.j[np++] = Pack16Job{mat_w(w->blk[i], j), reinterpret_cast<__bf16*>(ws->bf.wt[i][j]), MAT_N[j], MAT_K[j], 1};
            }
        T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st, pack16_multi_kernel<<<dim3((3 * D * D + 255) / 256, np), 256, 0, st>>>(pt));
    }
    T2S_HIP_CHECK(hipMemcpyAsync(ws->lat, x, (size_t)S * h->lat() * sizeof(float), hipMemcpyDeviceToDevice, st));
    T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st, cond_rows_kernel<<<(S * D + 255) / 256, 256, 0, st>>>(ws->c, temb, temb_rows, text, S));
    T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st, silu_kernel<<<(S * D + 255) / 256, 256, 0, st>>>(ws->c, ws->silu_c, S * D));
    T2S_TIMED(h, TC_TR_TAIL, st, gemm<128, 3, PRO_PLAIN, EPI_BIAS>(ws->silu_c, h->ada_p, h->ada_b, ws->mod, S, MODROW, st));
    T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st,
                     T2S_BY_WIDTH(h->latw, patchify_rows_kernel<W><<<((S + 3) / 4 * ntok * 32 + 255) / 256, 256, 0, st>>>(
                                                   x, ws->x_in[0], S, h->conv_w, h->conv_b, h->patch_w, h->patch_b, h->pos, h->latw)));
    if ((rc = bf ? forward_blocks_bf16(h, ws, S, st) : forward_blocks_f32(h, ws, S, st))) return rc;
    if (bf)   // (the last block's x_mid + g2 * f is formed here)
        T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st,
                         T2S_BY_WIDTH(h->latw, final_rows_kernel<W><<<((M + 3) / 4 * 32 + 255) / 256, 256, 0, st>>>(
                                                   ws->x_mid[NBLK - 1], S, h->ln_w, h->ln_b, h->out_w, h->out_b, out, ws->bf.f[NBLK - 1], ws->mod,
                                                   (NBLK - 1) * MODW + 5 * D, h->latw)));
    else
        T2S_TIMED_LAUNCH(h, TC_TR_TAIL, st,
                         T2S_BY_WIDTH(h->latw, final_rows_kernel<W><<<((M + 3) / 4 * 32 + 255) / 256, 256, 0, st>>>(
                                                   ws->x_in[NBLK], S, h->ln_w, h->ln_b, h->out_w, h->out_b, out, nullptr, nullptr, 0, h->latw)));
    return T2S_OK;
}

}  // extern "C"

namespace {
template <int W>
int forward_blocks_bf16_w(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st) {
    constexpr int TOK = W ? 16 * W : 0;   // the GEMMs' tile -> sequence maps
    t2s_train_ws::BF16& a = ws->bf;
    const int ntok = h->ntok();
    const int M = S * ntok;
    for (int i = 0; i < NBLK; ++i) {
        const int base = i * MODW;
        // The gate / residual adds have no kernel of their own: the GEMM that consumes a residual-stream tensor forms it
        // in its prologue (x = x_prev + gate * branch), writes it out for the backward pass and LayerNorm-modulates it.
        // a1 = mod(LN1(x_in)) -> bf16; q,k,v = a1 Wqkv^T + b -> bf16 heads; for i > 0, x_in[i] = x_mid[i-1] + g2 f[i-1]
        T2S_TIMED(h, TC_TR_GEMM, st,
                  i == 0 ? bgemm<128, 384, BPRO_LN, BEPI_QKV, TOK>(ws->x_in[i], a.w[i][QKV], h->bias[i][QKV], nullptr, M, 3 * D, st, ws->mod,
                                                                   base + 0 * D, base + 1 * D, a.a1[i], nullptr, a.q[i], a.k[i], a.v[i], nullptr, 0,
                                                                   nullptr, ntok)
                         : bgemm<128, 384, BPRO_LN_RES, BEPI_QKV, TOK>(ws->x_mid[i - 1], a.w[i][QKV], h->bias[i][QKV], nullptr, M, 3 * D, st, ws->mod,
                                                                       base + 0 * D, base + 1 * D, a.a1[i], nullptr, a.q[i], a.k[i], a.v[i],
                                                                       a.f[i - 1], (i - 1) * MODW + 5 * D, ws->x_in[i], ntok));
        T2S_TIMED(h, TC_TR_ATTN_FWD, st, attn16_train_fwd(a.q[i], a.k[i], a.v[i], a.o[i], ws->lse[i], S * NH, ntok, st));
        // p = o Wp^T + b
        T2S_TIMED(h, TC_TR_GEMM, st, bgemm<128, 128, BPRO_BF16, BEPI_BF16>(a.o[i], a.w[i][PROJ], h->bias[i][PROJ], a.p[i], M, D, st));
        // x_mid = x_in + g1 * p; a2 = mod(LN2(x_mid)); u = a2 W1^T + b1
        T2S_TIMED(h, TC_TR_GEMM, st,
                  bgemm<128, 256, BPRO_LN_RES, BEPI_BF16, TOK>(ws->x_in[i], a.w[i][FC1], h->bias[i][FC1], a.u[i], M, 2 * D, st, ws->mod, base + 3 * D,
                                                               base + 4 * D, a.a2[i], nullptr, nullptr, nullptr, nullptr, a.p[i], base + 2 * D,
                                                               ws->x_mid[i], ntok));
        // f = gelu(u) W2^T + b2   (gelu(u) is not saved: the fc2 weight gradient re-applies it to u)
        T2S_TIMED(h, TC_TR_GEMM, st, bgemm<256, 128, BPRO_GELU, BEPI_BF16>(a.u[i], a.w[i][FC2], h->bias[i][FC2], a.f[i], M, D, st));
        // (the last block's x_mid + g2 * f is formed inside the final-layer kernels, forward and backward: never written)
    }
    return T2S_OK;
}
int forward_blocks_bf16(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st) {
    return h->latw == LATW ? forward_blocks_bf16_w<LATW>(h, ws, S, st) : forward_blocks_bf16_wide(h, ws, S, st);
}

template <int W>
int forward_blocks_f32_w(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st) {
    constexpr int TOK = W ? 16 * W : 0;   // the GEMMs' row -> sequence maps
    t2s_train_ws::F32& a = ws->f32;
    const int ntok = h->ntok();
    const int M = S * ntok;
    for (int i = 0; i < NBLK; ++i) {
        const int base = i * MODW;
        // a1 = mod(LN1(x_in)); q,k,v = a1 Wqkv^T + b
        T2S_TIMED(h, TC_TR_GEMM, st,
                  gemm<128, 3, PRO_LNMOD, EPI_QKV, TOK>(ws->x_in[i], h->p32[i][QKV], h->bias[i][QKV], nullptr, M, 3 * D, st, ws->mod, base + 0 * D,
                                                        base + 1 * D, a.a1[i], nullptr, a.q[i], a.k[i], a.v[i], ntok));
        T2S_TIMED(h, TC_TR_ATTN_FWD, st, attn_plain_train_fwd(a.q[i], a.k[i], a.v[i], a.o[i], ws->lse[i], S * NH, ntok, st));
        T2S_TIMED(h, TC_TR_GEMM, st, gemm<128, 1, PRO_PLAIN, EPI_BIAS>(a.o[i], h->p32[i][PROJ], h->bias[i][PROJ], a.p[i], M, D, st));
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st,
                         gate_res_kernel<W><<<(M * 32 + 255) / 256, 256, 0, st>>>(ws->x_in[i], a.p[i], ws->mod, base + 2 * D, ws->x_mid[i], M, h->latw));
        // a2 = mod(LN2(x_mid)); u = a2 W1^T + b1; f = gelu(u) W2^T + b2
        T2S_TIMED(h, TC_TR_GEMM, st,
                  gemm<128, 2, PRO_LNMOD, EPI_BIAS, TOK>(ws->x_mid[i], h->p32[i][FC1], h->bias[i][FC1], a.u[i], M, 2 * D, st, ws->mod, base + 3 * D,
                                                         base + 4 * D, a.a2[i], nullptr, nullptr, nullptr, nullptr, ntok));
        T2S_TIMED(h, TC_TR_GEMM, st, gemm<256, 1, PRO_GELU, EPI_BIAS>(a.u[i], a.fc2_f[i], h->bias[i][FC2], a.f[i], M, D, st));
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st,
                         gate_res_kernel<W><<<(M * 32 + 255) / 256, 256, 0, st>>>(ws->x_mid[i], a.f[i], ws->mod, base + 5 * D, ws->x_in[i + 1], M, h->latw));
    }
    return T2S_OK;
}
int forward_blocks_f32(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st) {
    return h->latw == LATW ? forward_blocks_f32_w<LATW>(h, ws, S, st) : forward_blocks_f32_w<0>(h, ws, S, st);
}
}  // namespace

extern "C" {

int t2s_dit_train_backward(t2s_dit* h, const float* dout, const t2s_dit_grads* g, int B, void* stream) {
    t2s::reset_tile_dir();
    T2S_REQUIRE(h && dout && g, "t2s_dit_train_backward: NULL argument");
    T2S_REQUIRE(h->latw == LATW || h->trainable, "t2s_dit_train_backward: training runs at latent width 30 only, this handle has %d", h->latw);
    T2S_REQUIRE(h->train && h->train->S == B, "t2s_dit_train_backward: no matching t2s_dit_train_forward (B=%d)", B);
    T2S_REQUIRE(h->train->dtype == h->train_dtype, "t2s_dit_train_backward: training dtype changed since the forward");
    hipStream_t st = (hipStream_t)stream;
    t2s_train_ws* ws = h->train;
    const int S = B, M = S * h->ntok();
    int rc;
    // ---- zero every gradient (the kernels accumulate with atomics)
    struct Z { float* p; size_t n; };
    std::vector<Z> zs = {{g->conv_w, 16}, {g->conv_b, 4}, {g->patch_w, 512}, {g->patch_b, 128}, {g->ln_w, 128},
                         {g->ln_b, 128}, {g->out_w, 512}, {g->out_b, 4}};
    for (int i = 0; i < NBLK; ++i) {
        const t2s_dit_block_grads& b = g->blk[i];
        zs.insert(zs.end(), {{b.qkv_w, 3 * D * D}, {b.qkv_b, 3 * D}, {b.proj_w, D * D}, {b.proj_b, D}, {b.fc1_w, 2 * D * D},
                             {b.fc1_b, 2 * D}, {b.fc2_w, 2 * D * D}, {b.fc2_b, D}, {b.ada_w, MODW * D}, {b.ada_b, MODW}});
    }
    // adjacent ranges are merged: the host mirror carves all of them out of one flat bucket (what the data-parallel
    // all-reduce sends), so this is normally ONE memset instead of 48
    for (size_t i = 0; i < zs.size();) {
        T2S_REQUIRE(zs[i].p, "t2s_dit_train_backward: NULL gradient pointer");
        float* p = zs[i].p;
        size_t n = zs[i].n;
        size_t k = i + 1;
        while (k < zs.size() && zs[k].p == p + n) n += zs[k++].n;
        T2S_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(float), st));
        i = k;
    }
    // ---- final layer
    const bool bf = ws->dtype == T2S_TRAIN_BF16;
    T2S_REQUIRE(!bf || h->latw == LATW || h->wide_train_bf16,
                "t2s_dit_train_backward: a handle of latent width %d trains in T2S_TRAIN_F32 only", h->latw);
    const int tail_wgs = (M + TAIL_ROWS - 1) / TAIL_ROWS;
    const int ntok = h->ntok(), frows = fused_rows(ntok);      // bf16: 160 (128 at 1024 tokens) rows = a whole fraction of a sequence
    T2S_REQUIRE(!bf || (ntok % frows == 0 && M % frows == 0), "t2s_dit_train_backward: %d tokens are no whole number of %d-row workgroups", ntok, frows);
    const int final_wgs = bf ? M / frows : tail_wgs, final_stride = bf ? FINAL_COLS + D : FINAL_COLS;
    T2S_REQUIRE((size_t)final_wgs * final_stride <= ws->wg_scratch_floats && (size_t)tail_wgs * PATCH_COLS <= ws->wg_scratch_floats,
                "t2s_dit_train_backward: scratch too small for the tail partials");
    { TimeScope ts(h, TC_TR_TAIL, st);
    if (bf) {   // + the gate backward of the last block's MLP branch: t1 = df = g2 * dx, dgate2
        const int goff = (NBLK - 1) * MODW + 5 * D;
        if (h->latw == LATW) {
            final_bwd_kernel<true, fused_rows(NTOK), LATW><<<final_wgs, 256, 0, st>>>(ws->x_mid[NBLK - 1], dout, h->ln_w, h->ln_b, h->out_w, ws->dx,
                                                                                      ws->wg_scratch, M, ws->bf.f[NBLK - 1], ws->mod, goff, ws->bf.t1, LATW);
            T2S_LAUNCH_CHECK();
            final_gate_reduce_kernel<NTOK / fused_rows(NTOK)><<<S, D, 0, st>>>(ws->wg_scratch, final_stride, ws->dmod, goff, 0);
        } else if ((rc = final_bwd_fused_wide(h, ws, dout, M, S, goff, final_wgs, final_stride, st))) {
            return rc;
        }
    } else {
        T2S_BY_WIDTH(h->latw, final_bwd_kernel<false, TAIL_ROWS, W><<<final_wgs, 256, 0, st>>>(ws->x_in[NBLK], dout, h->ln_w, h->ln_b, h->out_w, ws->dx,
                                                                                              ws->wg_scratch, M, nullptr, nullptr, 0, nullptr, h->latw));
    }
    T2S_LAUNCH_CHECK();
    tail_reduce_kernel<<<(FINAL_COLS + 31) / 32, 256, 0, st>>>(ws->wg_scratch, final_wgs, FINAL_COLS, final_stride,
                                                                 TailDst{{g->ln_w, g->ln_b, g->out_w, g->out_b}, {D, D, 4 * D, 4}});
    T2S_LAUNCH_CHECK();
    }
    if ((rc = bf ? backward_blocks_bf16(h, ws, g, S, st) : backward_blocks_f32(h, ws, g, S, st))) return rc;
    // ---- patchify
    { TimeScope ts(h, TC_TR_TAIL, st);
    T2S_BY_WIDTH(h->latw, patchify_bwd_kernel<W><<<tail_wgs, 256, 0, st>>>(ws->dx, ws->lat, S, h->conv_w, h->conv_b, h->patch_w, ws->wg_scratch, M, h->latw));
    T2S_LAUNCH_CHECK();
    tail_reduce_kernel<<<(PATCH_COLS + 31) / 32, 256, 0, st>>>(ws->wg_scratch, tail_wgs, PATCH_COLS, PATCH_COLS,
                                                                 TailDst{{g->patch_w, g->patch_b, g->conv_w, g->conv_b}, {4 * D, D, 16, 4}});
    T2S_LAUNCH_CHECK();
    }
    // ---- adaLN linear: mod = silu(c) W_ada^T + b_ada  (per block rows [768 i, 768 i + 768) of the (3072,128) stack)
    for (int i = 0; i < NBLK; ++i) {
        // dmod block slice is strided (row stride MODROW): copy to a dense (S,768) temp first
        T2S_HIP_CHECK(hipMemcpy2DAsync(ws->t1, MODW * sizeof(float), ws->dmod + i * MODW, MODROW * sizeof(float),
                                       MODW * sizeof(float), S, hipMemcpyDeviceToDevice, st));
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad(ws, ws->t1, ws->silu_c, g->blk[i].ada_w, g->blk[i].ada_b, S, MODW, D, st));
    }
    return T2S_OK;
}

}  // extern "C"

namespace {
// (Measured and dropped in round 2: the four weight gradients of a block on a side stream.  Issued as soon as their
// operands exist they only share the HBM bandwidth with the GEMM / LayerNorm kernels they run beside (13.42 ms per step,
// the same as in order); issued beside the VALU-bound attention backward they slow it by more than they take alone
// (attention backward 3.0 -> 4.4 ms per step, 14.1 ms per step): the attention workgroups fill the CUs.
// Round 3 repeated both as timing-only builds on a stream CALIBRATED to run concurrently (t2s_sampler.hip lane_streams:
// HIP streams that share a hardware queue serialise, which may have been the "same as in order" of round 2): without any
// dependency waits 10.92 vs 11.10 ms in order, issued beside the attention backward 11.08 -- the attention backward then
// takes 3.1-3.7 instead of 2.2 ms: it is bound by vector issue, but its 16 waves per CU leave the other kernel no slot.)
template <int W>
int backward_blocks_bf16_w(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st) {
    constexpr int TOK = W ? 16 * W : 0;
    t2s_train_ws::BF16& a = ws->bf;
    const int ntok = h->ntok();
    const int M = S * ntok;
    auto wgrad16 = [&](auto gelu, const __bf16* dY, const __bf16* X, float* dW, float* db, int N, int K) {
        return launch_wgrad16<decltype(gelu)::value>(dY, X, dW, db, M, N, K, ws->wg_scratch, ws->wg_scratch_floats, ws->n_cu, st);
    };
    constexpr std::true_type gelu_x{};
    constexpr std::false_type plain{};
    for (int i = NBLK - 1; i >= 0; --i) {
        const int base = i * MODW;
        const t2s_dit_block_grads& b = g->blk[i];
        // ---- MLP branch: x_out = x_mid + g2 * f.  t1 = df = g2 * dx and dgate2 come from the kernel that produced dx: the
        // next block's LN1 backward epilogue, or the final-layer backward for the last block
        // dW2 = df^T gelu(u): gelu applied to the fetched u chunks (not saved)
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad16(gelu_x, a.t1, a.u[i], b.fc2_w, b.fc2_b, D, 2 * D));
        // du = (df W2) * gelu'(u)
        T2S_TIMED(h, TC_TR_GEMM, st,
                  bgemm<128, 256, BPRO_BF16, BEPI_GELUBWD>(a.t1, a.wt[i][FC2], nullptr, a.t2, M, 2 * D, st, nullptr, 0, 0, nullptr, a.u[i]));
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad16(plain, a.t2, a.a2[i], b.fc1_w, b.fc1_b, 2 * D, D));
        // da2 = du W1, consumed in the accumulators: LN2 backward into dx merged with the attention branch's gate
        // backward (t1 = dp = g1 * dx, dgate1) -- the epilogue of the data-gradient GEMM (BEPI_LNBWD; da2 never reaches HBM)
        T2S_TIMED(h, TC_TR_GEMM, st,
                  bgemm_lnbwd<256, TOK>(ws, a.t2, a.wt[i][FC1], ws->x_mid[i], base + 3 * D, base + 4 * D, a.p[i], base + 2 * D, a.t1, M, st));
        // ---- attention branch: x_mid = x_in + g1 * p
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad16(plain, a.t1, a.o[i], b.proj_w, b.proj_b, D, D));
        T2S_TIMED(h, TC_TR_GEMM, st, bgemm<128, 128, BPRO_BF16, BEPI_BF16>(a.t1, a.wt[i][PROJ], nullptr, a.t4, M, D, st));   // do
        T2S_TIMED(h, TC_TR_ATTN_BWD, st, attn16_bwd(a.q[i], a.k[i], a.v[i], a.o[i], a.t4, ws->lse[i], ws->dsum, a.t3, S * NH, ntok, st));
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad16(plain, a.t3, a.a1[i], b.qkv_w, b.qkv_b, 3 * D, D));
        // da1 = dqkv Wqkv with LN1 backward into dx as its epilogue, merged with the gate backward of block i-1's MLP branch
        T2S_TIMED(h, TC_TR_GEMM, st,
                  bgemm_lnbwd<384, TOK>(ws, a.t3, a.wt[i][QKV], ws->x_in[i], base + 0 * D, base + 1 * D,
                                   i > 0 ? a.f[i - 1] : (const __bf16*)nullptr, (i - 1) * MODW + 5 * D, a.t1, M, st));
    }
    return T2S_OK;
}
int backward_blocks_bf16(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st) {
    return h->latw == LATW ? backward_blocks_bf16_w<LATW>(h, ws, g, S, st) : backward_blocks_bf16_wide(h, ws, g, S, st);
}

template <int W>
int backward_blocks_f32_w(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st) {
    t2s_train_ws::F32& a = ws->f32;
    const int ntok = h->ntok();
    const int M = S * ntok;
    for (int i = NBLK - 1; i >= 0; --i) {
        const int base = i * MODW;
        const t2s_dit_block_grads& b = g->blk[i];
        // ---- MLP branch: x_out = x_mid + g2 * f
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st, gate_bwd_kernel<W><<<S, 256, 0, st>>>(ws->dx, a.f[i], ws->mod, base + 5 * D, ws->t1, ws->dmod, h->latw));   // t1 = df
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st,
                         gelu_kernel<<<((size_t)M * 64 + 255) / 256, 256, 0, st>>>(a.u[i], a.t2a, (size_t)M * 64));   // t2a = gelu(u)
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad(ws, ws->t1, a.t2a, b.fc2_w, b.fc2_b, M, D, 2 * D, st));
        // du = (df W2) * gelu'(u)      (dgrad = row GEMM on W2^T: out 256 <- in 128)
        T2S_TIMED(h, TC_TR_GEMM, st,
                  gemm<128, 2, PRO_PLAIN, EPI_GELUBWD>(ws->t1, a.wt[i][FC2], nullptr, a.t2b, M, 2 * D, st, nullptr, 0, 0, nullptr, a.u[i]));
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad(ws, a.t2b, a.a2[i], b.fc1_w, b.fc1_b, M, 2 * D, D, st));
        // da2 = du W1 (out 128 <- in 256)
        T2S_TIMED(h, TC_TR_GEMM, st, gemm<256, 1, PRO_PLAIN, EPI_BIAS>(a.t2b, a.wt[i][FC1], nullptr, ws->t1, M, D, st));
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st,
                         ln_mod_bwd_kernel<W><<<S, 256, 0, st>>>(ws->t1, ws->x_mid[i], ws->mod, base + 3 * D, base + 4 * D, ws->dx, ws->dmod,
                                                                 (const float*)nullptr, 0, (float*)nullptr, h->latw));
        // ---- attention branch: x_mid = x_in + g1 * p
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st, gate_bwd_kernel<W><<<S, 256, 0, st>>>(ws->dx, a.p[i], ws->mod, base + 2 * D, ws->t1, ws->dmod, h->latw));   // t1 = dp
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad(ws, ws->t1, a.o[i], b.proj_w, b.proj_b, M, D, D, st));
        T2S_TIMED(h, TC_TR_GEMM, st, gemm<128, 1, PRO_PLAIN, EPI_BIAS>(ws->t1, a.wt[i][PROJ], nullptr, a.t4, M, D, st));   // do
        T2S_TIMED(h, TC_TR_ATTN_BWD, st, attn_bwd(a.q[i], a.k[i], a.v[i], a.o[i], a.t4, ws->lse[i], ws->dsum, a.t3, S * NH, ntok, st));
        T2S_TIMED(h, TC_TR_WGRAD, st, wgrad(ws, a.t3, a.a1[i], b.qkv_w, b.qkv_b, M, 3 * D, D, st));
        // da1 = dqkv Wqkv (out 128 <- in 384)
        T2S_TIMED(h, TC_TR_GEMM, st, gemm<384, 1, PRO_PLAIN, EPI_BIAS>(a.t3, a.wt[i][QKV], nullptr, ws->t1, M, D, st));
        T2S_TIMED_LAUNCH(h, TC_TR_ELEM, st,
                         ln_mod_bwd_kernel<W><<<S, 256, 0, st>>>(ws->t1, ws->x_in[i], ws->mod, base + 0 * D, base + 1 * D, ws->dx, ws->dmod,
                                                                 (const float*)nullptr, 0, (float*)nullptr, h->latw));
    }
    return T2S_OK;
}
int backward_blocks_f32(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st) {
    return h->latw == LATW ? backward_blocks_f32_w<LATW>(h, ws, g, S, st) : backward_blocks_f32_w<0>(h, ws, g, S, st);
}
}  // namespace

extern "C" {

int t2s_dit_train_input_grad(t2s_dit* h, float* dinput, int B, void* stream) {
    T2S_REQUIRE(h && dinput, "t2s_dit_train_input_grad: NULL argument");
    T2S_REQUIRE(h->latw == LATW || h->trainable, "t2s_dit_train_input_grad: training runs at latent width 30 only, this handle has %d", h->latw);
    T2S_REQUIRE(h->train && h->train->S == B, "t2s_dit_train_input_grad: no matching t2s_dit_train_backward (B=%d)", B);
    t2s_train_ws* ws = h->train;
    TimeScope ts(h, TC_TR_TAIL, (hipStream_t)stream);
    T2S_BY_WIDTH(h->latw, patchify_input_grad_kernel<W><<<(B * h->ntok() + 255) / 256, 256, 0, (hipStream_t)stream>>>(ws->dx, dinput, B, h->conv_w,
                                                                                                                    h->patch_w, h->latw));
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int t2s_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, void* stream) {
    T2S_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step > 0, "t2s_adamw_step: bad argument");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = 1.0f - powf(beta2, (float)step);
    adamw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, (size_t)n, lr,
                                                                                beta1, beta2, eps, weight_decay, bc1,
                                                                                sqrtf(bc2));
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int t2s_adamw_step_multi(const t2s_adamw_tensor* table_dev, int n_tensors, uint64_t total_chunks, float lr, float beta1,
                         float beta2, float eps, float weight_decay, int step, void* stream) {
    T2S_REQUIRE(table_dev && n_tensors > 0 && n_tensors <= 64 && total_chunks > 0 && step > 0, "t2s_adamw_step_multi: bad argument");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = 1.0f - powf(beta2, (float)step);
    adamw_multi_kernel<<<(unsigned)total_chunks, 256, 0, (hipStream_t)stream>>>(table_dev, n_tensors, lr, beta1, beta2, eps,
                                                                                weight_decay, bc1, sqrtf(bc2));
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int t2s_mse_backward(const float* a, const float* b, const float* grad_out, float* da, float* db, uint64_t n, void* stream) {
    T2S_REQUIRE(a && b && grad_out && n > 0 && (da || db), "t2s_mse_backward: bad argument");
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (da) mse_bwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(a, b, grad_out, da, (size_t)n, 1.0f);
    if (db) mse_bwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(a, b, grad_out, db, (size_t)n, -1.0f);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int t2s_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, int dtype, int flags, void* stream) {
    T2S_REQUIRE(dY && X && dW, "t2s_wgrad: NULL argument");
    T2S_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 128 == 0, "t2s_wgrad: unsupported shape M=%d N=%d K=%d", M, N, K);
    T2S_REQUIRE(dtype == T2S_TRAIN_F32 || dtype == T2S_TRAIN_BF16, "t2s_wgrad: unknown dtype %d", dtype);
    T2S_REQUIRE((flags & ~3) == 0, "t2s_wgrad: unknown flags %d", flags);
    T2S_REQUIRE(!(flags & 1) || dtype == T2S_TRAIN_BF16, "t2s_wgrad: gelu on the X operand (flags bit 0) is a bf16 kernel only");
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    hipDeviceProp_t prop;
    T2S_HIP_CHECK(hipGetDevice(&dev));
    T2S_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    const int n_cu = prop.multiProcessorCount;
    const size_t scratch_floats = wgrad16_shape_scratch_floats(N, K, n_cu);
    float* scratch = nullptr;
    __bf16* buf = nullptr;                                  // bf16: dY (M,N) | X (M,K)
    T2S_HIP_CHECK(hipMalloc(&scratch, scratch_floats * sizeof(float)));
    t2s::g_tile_flip = (flags & 2) ? 1u : 0u;               // the direction next_tile_dir() hands the launch
    int rc = T2S_OK;
    if (dtype == T2S_TRAIN_F32) {
        rc = launch_wgrad32(dY, X, dW, db, M, N, K, scratch, scratch_floats, n_cu, st);
    } else if (hipMalloc(&buf, (size_t)M * (N + K) * sizeof(__bf16)) != hipSuccess) {
        set_error("t2s_wgrad: out of memory for %zu bf16 values", (size_t)M * (N + K));
        rc = T2S_E_HIP;
    } else {
        __bf16 *yh = buf, *xh = buf + (size_t)M * N;
        rc = f32_to_bf16(dY, yh, (size_t)M * N, 1.0f, st);
        if (rc == T2S_OK) rc = f32_to_bf16(X, xh, (size_t)M * K, 1.0f, st);
        if (rc == T2S_OK)
            rc = (flags & 1) ? launch_wgrad16<true>(yh, xh, dW, db, M, N, K, scratch, scratch_floats, n_cu, st)
                             : launch_wgrad16<false>(yh, xh, dW, db, M, N, K, scratch, scratch_floats, n_cu, st);
    }
    (void)hipStreamSynchronize(st);
    if (buf) (void)hipFree(buf);
    (void)hipFree(scratch);
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ the run-time forms of the bf16 step (see their declarations)
namespace {
int forward_blocks_bf16_wide(t2s_dit* h, t2s_train_ws* ws, int S, hipStream_t st) { return forward_blocks_bf16_w<0>(h, ws, S, st); }
int backward_blocks_bf16_wide(t2s_dit* h, t2s_train_ws* ws, const t2s_dit_grads* g, int S, hipStream_t st) {
    return backward_blocks_bf16_w<0>(h, ws, g, S, st);
}
int final_bwd_fused_wide(t2s_dit* h, t2s_train_ws* ws, const float* dout, int M, int S, int goff, int final_wgs, int final_stride, hipStream_t st) {
    const int ntok = h->ntok(), frows = fused_rows(ntok);
    if (frows == 160)
        final_bwd_kernel<true, 160, 0><<<final_wgs, 256, 0, st>>>(ws->x_mid[NBLK - 1], dout, h->ln_w, h->ln_b, h->out_w, ws->dx, ws->wg_scratch, M,
                                                                  ws->bf.f[NBLK - 1], ws->mod, goff, ws->bf.t1, h->latw);
    else
        final_bwd_kernel<true, 128, 0><<<final_wgs, 256, 0, st>>>(ws->x_mid[NBLK - 1], dout, h->ln_w, h->ln_b, h->out_w, ws->dx, ws->wg_scratch, M,
                                                                  ws->bf.f[NBLK - 1], ws->mod, goff, ws->bf.t1, h->latw);
    T2S_LAUNCH_CHECK();
    final_gate_reduce_kernel<0><<<S, D, 0, st>>>(ws->wg_scratch, final_stride, ws->dmod, goff, ntok / frows);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
}  // namespace

// ------------------------------------------------------------------ include/t2s_train_rows.h: one launch form of the step alone
// Host code only, and LAST in this file: every kernel it names is an instantiation the recipes above have already asked for, so
// the code object keeps its kernels and their order.
namespace t2s {
int bf16_to_f32(const __bf16* src, float* dst, size_t n, hipStream_t st);   // t2s_attn_bf16.hip
}
namespace {
struct RowsBufs {   // the entry's temporaries: freed when it returns
    std::vector<void*> all;
    struct Widen { const __bf16* src; float* dst; size_t n; };
    std::vector<Widen> widen;
    bool oom = false;
    ~RowsBufs() { for (void* p : all) (void)hipFree(p); }
    template <class T>
    T* get(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { oom = true; return nullptr; }
        all.push_back(p);
        return static_cast<T*>(p);
    }
    // a bf16 copy of an fp32 operand (NULL stays NULL)
    const __bf16* in16(const float* src, size_t n, hipStream_t st, int* rc) {
        if (src == nullptr || *rc != T2S_OK) return nullptr;
        __bf16* d = get<__bf16>(n);
        if (d == nullptr) return nullptr;
        *rc = f32_to_bf16(src, d, n, 1.0f, st);
        return d;
    }
    // a bf16 result, widened into dst by finish()
    __bf16* out16(float* dst, size_t n) {
        if (dst == nullptr) return nullptr;
        __bf16* d = get<__bf16>(n);
        if (d != nullptr) widen.push_back({d, dst, n});
        return d;
    }
    int finish(hipStream_t st) {
        for (const Widen& w : widen)
            if (const int rc = bf16_to_f32(w.src, w.dst, w.n, st)) return rc;
        return T2S_OK;
    }
};

// what a launch form needs of t2s_train_rows_args
enum : unsigned { RA = 1, RW = 2, RMOD = 4, RRES = 8, RAUX = 16, RLNX = 32, RFIN = 64, ROUT = 128, RSAVE = 256, RXOUT = 512,
                  RQKV = 1024, RDX = 2048, RDMOD = 4096, RSHIFT = 8192, RSCALE = 16384, RGATE = 32768 };
struct RowsForm { int op, dtype; unsigned need; };
constexpr RowsForm ROWS_FORMS[] = {
    {T2S_ROWS_QKV0, T2S_TRAIN_BF16, RA | RW | RMOD | RSHIFT | RSCALE | RSAVE | RQKV},
    {T2S_ROWS_QKV1, T2S_TRAIN_BF16, RA | RW | RMOD | RSHIFT | RSCALE | RGATE | RRES | RXOUT | RSAVE | RQKV},
    {T2S_ROWS_FC1, T2S_TRAIN_BF16, RA | RW | RMOD | RSHIFT | RSCALE | RGATE | RRES | RXOUT | RSAVE | ROUT},
    {T2S_ROWS_FC2, T2S_TRAIN_BF16, RA | RW | ROUT},
    {T2S_ROWS_LIN128, T2S_TRAIN_BF16, RA | RW | ROUT},
    {T2S_ROWS_GELUBWD, T2S_TRAIN_BF16, RA | RW | RAUX | ROUT},
    {T2S_ROWS_LNBWD256, T2S_TRAIN_BF16, RA | RW | RLNX | RMOD | RSHIFT | RSCALE | RDX | RDMOD},
    {T2S_ROWS_LNBWD384, T2S_TRAIN_BF16, RA | RW | RLNX | RMOD | RSHIFT | RSCALE | RDX | RDMOD},
    {T2S_ROWS_FINAL_FUSED, T2S_TRAIN_BF16, RA | RW | RRES | RMOD | RGATE | RFIN | RDX | ROUT | RDMOD},
    {T2S_ROWS_F_QKV, T2S_TRAIN_F32, RA | RW | RMOD | RSHIFT | RSCALE | RSAVE | RQKV},
    {T2S_ROWS_F_FC1, T2S_TRAIN_F32, RA | RW | RMOD | RSHIFT | RSCALE | RSAVE | ROUT},
    {T2S_ROWS_F_FC2, T2S_TRAIN_F32, RA | RW | ROUT},
    {T2S_ROWS_F_LIN128, T2S_TRAIN_F32, RA | RW | ROUT},
    {T2S_ROWS_F_LIN256, T2S_TRAIN_F32, RA | RW | ROUT},
    {T2S_ROWS_F_LIN384, T2S_TRAIN_F32, RA | RW | ROUT},
    {T2S_ROWS_F_GELUBWD, T2S_TRAIN_F32, RA | RW | RAUX | ROUT},
    {T2S_ROWS_F_GATE_RES, T2S_TRAIN_F32, RA | RRES | RMOD | RGATE | RXOUT},
    {T2S_ROWS_F_GATE_BWD, T2S_TRAIN_F32, RDX | RRES | RMOD | RGATE | ROUT | RDMOD},
    {T2S_ROWS_F_LN_MOD_BWD, T2S_TRAIN_F32, RA | RLNX | RMOD | RSHIFT | RSCALE | RDX | RDMOD},
    {T2S_ROWS_F_GELU, T2S_TRAIN_F32, RA | ROUT},
    {T2S_ROWS_F_FINAL, T2S_TRAIN_F32, RA | RW | RFIN | RDX},
};

// weight (N,K) row-major -> the pack of its arithmetic, by the step's own packing kernels
int rows_pack32(const float* W, int N, int K, RowsBufs& b, f32x4** P, hipStream_t st) {
    *P = b.get<f32x4>((size_t)N * K / 4);
    if (*P == nullptr) return T2S_OK;   // (b.oom is reported by the caller)
    return pack_any(W, *P, N, K, 0, st);
}
int rows_pack16(const float* W, int N, int K, RowsBufs& b, bf16x8** P, hipStream_t st) {
    *P = b.get<bf16x8>((size_t)N * K / 8);
    if (*P == nullptr) return T2S_OK;
    pack16_kernel<<<(N * K + 255) / 256, 256, 0, st>>>(W, reinterpret_cast<__bf16*>(*P), N, K, 0);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

template <int TOK>
int rows_bf16(int op, int n_tok, int n_seq, const t2s_train_rows_args& p, RowsBufs& b, hipStream_t st) {
    const int M = n_seq * n_tok;
    const size_t MD = (size_t)M * D;
    int rc = T2S_OK;
    bf16x8* Wp = nullptr;
    const size_t hd = MD;   // elements of each of q, k, v: (n_seq * 4, n_tok, 32)
    switch (op) {
    case T2S_ROWS_QKV0:
    case T2S_ROWS_QKV1: {
        if ((rc = rows_pack16(p.w, 3 * D, D, b, &Wp, st))) return rc;
        const __bf16* res = op == T2S_ROWS_QKV1 ? b.in16(p.res, MD, st, &rc) : nullptr;
        __bf16 *a1 = b.out16(p.save_a, MD), *q = b.out16(p.q, hd), *k = b.out16(p.k, hd), *v = b.out16(p.v, hd);
        if (rc != T2S_OK || b.oom) return rc;
        return op == T2S_ROWS_QKV0
                   ? bgemm<128, 384, BPRO_LN, BEPI_QKV, TOK>(p.a, Wp, p.bias, nullptr, M, 3 * D, st, p.mod, p.shift_off, p.scale_off, a1, nullptr, q, k, v,
                                                             nullptr, 0, nullptr, n_tok)
                   : bgemm<128, 384, BPRO_LN_RES, BEPI_QKV, TOK>(p.a, Wp, p.bias, nullptr, M, 3 * D, st, p.mod, p.shift_off, p.scale_off, a1, nullptr, q, k,
                                                                 v, res, p.gate_off, p.x_out, n_tok);
    }
    case T2S_ROWS_FC1: {
        if ((rc = rows_pack16(p.w, 2 * D, D, b, &Wp, st))) return rc;
        const __bf16* res = b.in16(p.res, MD, st, &rc);
        __bf16 *a2 = b.out16(p.save_a, MD), *u = b.out16(p.out, 2 * MD);
        if (rc != T2S_OK || b.oom) return rc;
        return bgemm<128, 256, BPRO_LN_RES, BEPI_BF16, TOK>(p.a, Wp, p.bias, u, M, 2 * D, st, p.mod, p.shift_off, p.scale_off, a2, nullptr, nullptr, nullptr,
                                                            nullptr, res, p.gate_off, p.x_out, n_tok);
    }
    case T2S_ROWS_FC2: {
        if ((rc = rows_pack16(p.w, D, 2 * D, b, &Wp, st))) return rc;
        const __bf16* u = b.in16(p.a, 2 * MD, st, &rc);
        __bf16* f = b.out16(p.out, MD);
        if (rc != T2S_OK || b.oom) return rc;
        return bgemm<256, 128, BPRO_GELU, BEPI_BF16>(u, Wp, p.bias, f, M, D, st);
    }
    case T2S_ROWS_LIN128: {
        if ((rc = rows_pack16(p.w, D, D, b, &Wp, st))) return rc;
        const __bf16* a = b.in16(p.a, MD, st, &rc);
        __bf16* o = b.out16(p.out, MD);
        if (rc != T2S_OK || b.oom) return rc;
        return bgemm<128, 128, BPRO_BF16, BEPI_BF16>(a, Wp, p.bias, o, M, D, st);
    }
    case T2S_ROWS_GELUBWD: {
        if ((rc = rows_pack16(p.w, 2 * D, D, b, &Wp, st))) return rc;
        const __bf16* a = b.in16(p.a, MD, st, &rc);
        const __bf16* u = b.in16(p.aux, 2 * MD, st, &rc);
        __bf16* o = b.out16(p.out, 2 * MD);
        if (rc != T2S_OK || b.oom) return rc;
        return bgemm<128, 256, BPRO_BF16, BEPI_GELUBWD>(a, Wp, p.bias, o, M, 2 * D, st, nullptr, 0, 0, nullptr, u);
    }
    case T2S_ROWS_LNBWD256:
    case T2S_ROWS_LNBWD384: {
        const int K = op == T2S_ROWS_LNBWD256 ? 2 * D : 3 * D;
        if ((rc = rows_pack16(p.w, D, K, b, &Wp, st))) return rc;
        const __bf16* dY = b.in16(p.a, (size_t)M * K, st, &rc);
        const __bf16* f_next = b.in16(p.res, MD, st, &rc);
        __bf16* t_next = p.res != nullptr ? b.out16(p.out, MD) : nullptr;
        t2s_train_ws ws;             // what bgemm_lnbwd reads of a workspace
        ws.latw = n_tok / 16;
        ws.mod = const_cast<float*>(p.mod);
        ws.dx = p.dx;
        ws.dmod = p.dmod;
        ws.colpart = b.get<float>((size_t)M / 32 * 384);
        if (rc != T2S_OK || b.oom) return rc;
        return op == T2S_ROWS_LNBWD256 ? bgemm_lnbwd<256, TOK>(&ws, dY, Wp, p.ln_x, p.shift_off, p.scale_off, f_next, p.gate_off, t_next, M, st)
                                       : bgemm_lnbwd<384, TOK>(&ws, dY, Wp, p.ln_x, p.shift_off, p.scale_off, f_next, p.gate_off, t_next, M, st);
    }
    default: {   // T2S_ROWS_FINAL_FUSED, as t2s_dit_train_backward launches it
        const int frows = fused_rows(n_tok), final_wgs = M / frows, final_stride = FINAL_COLS + D;
        const __bf16* f = b.in16(p.res, MD, st, &rc);
        __bf16* t = b.out16(p.out, MD);
        float* part = b.get<float>((size_t)final_wgs * final_stride);
        if (rc != T2S_OK || b.oom) return rc;
        if (TOK == NTOK) {
            final_bwd_kernel<true, fused_rows(NTOK), LATW><<<final_wgs, 256, 0, st>>>(p.a, p.dout, p.ln_w, p.ln_b, p.w, p.dx, part, M, f, p.mod, p.gate_off, t, LATW);
            T2S_LAUNCH_CHECK();
            final_gate_reduce_kernel<NTOK / fused_rows(NTOK)><<<n_seq, D, 0, st>>>(part, final_stride, p.dmod, p.gate_off, 0);
        } else {
            t2s_dit hd;              // what final_bwd_fused_wide reads of a handle and a workspace
            hd.latw = n_tok / 16;
            hd.ln_w = const_cast<float*>(p.ln_w); hd.ln_b = const_cast<float*>(p.ln_b); hd.out_w = const_cast<float*>(p.w);
            t2s_train_ws ws;
            ws.latw = hd.latw;
            ws.x_mid[NBLK - 1] = const_cast<float*>(p.a);
            ws.dx = p.dx; ws.wg_scratch = part; ws.mod = const_cast<float*>(p.mod); ws.dmod = p.dmod;
            ws.bf.f[NBLK - 1] = const_cast<__bf16*>(f);
            ws.bf.t1 = t;
            if ((rc = final_bwd_fused_wide(&hd, &ws, p.dout, M, n_seq, p.gate_off, final_wgs, final_stride, st))) return rc;
        }
        T2S_LAUNCH_CHECK();
        tail_reduce_kernel<<<(FINAL_COLS + 31) / 32, 256, 0, st>>>(part, final_wgs, FINAL_COLS, final_stride,
                                                                     TailDst{{p.g_ln_w, p.g_ln_b, p.g_out_w, p.g_out_b}, {D, D, 4 * D, 4}});
        T2S_LAUNCH_CHECK();
        return T2S_OK;
    }
    }
}

template <int W>
int rows_f32(int op, int n_tok, int n_seq, const t2s_train_rows_args& p, RowsBufs& b, hipStream_t st) {
    constexpr int TOK = W ? 16 * W : 0;
    const int M = n_seq * n_tok, latw = n_tok / 16;
    int rc = T2S_OK;
    f32x4* Wp = nullptr;
    switch (op) {
    case T2S_ROWS_F_QKV:
        if ((rc = rows_pack32(p.w, 3 * D, D, b, &Wp, st)) || b.oom) return rc;
        return gemm<128, 3, PRO_LNMOD, EPI_QKV, TOK>(p.a, Wp, p.bias, nullptr, M, 3 * D, st, p.mod, p.shift_off, p.scale_off, p.save_a, nullptr, p.q, p.k,
                                                     p.v, n_tok);
    case T2S_ROWS_F_FC1:
        if ((rc = rows_pack32(p.w, 2 * D, D, b, &Wp, st)) || b.oom) return rc;
        return gemm<128, 2, PRO_LNMOD, EPI_BIAS, TOK>(p.a, Wp, p.bias, p.out, M, 2 * D, st, p.mod, p.shift_off, p.scale_off, p.save_a, nullptr, nullptr,
                                                      nullptr, nullptr, n_tok);
    case T2S_ROWS_F_FC2:
        if ((rc = rows_pack32(p.w, D, 2 * D, b, &Wp, st)) || b.oom) return rc;
        return gemm<256, 1, PRO_GELU, EPI_BIAS>(p.a, Wp, p.bias, p.out, M, D, st);
    case T2S_ROWS_F_LIN128:
        if ((rc = rows_pack32(p.w, D, D, b, &Wp, st)) || b.oom) return rc;
        return gemm<128, 1, PRO_PLAIN, EPI_BIAS>(p.a, Wp, p.bias, p.out, M, D, st);
    case T2S_ROWS_F_LIN256:
        if ((rc = rows_pack32(p.w, D, 2 * D, b, &Wp, st)) || b.oom) return rc;
        return gemm<256, 1, PRO_PLAIN, EPI_BIAS>(p.a, Wp, p.bias, p.out, M, D, st);
    case T2S_ROWS_F_LIN384:
        if ((rc = rows_pack32(p.w, D, 3 * D, b, &Wp, st)) || b.oom) return rc;
        return gemm<384, 1, PRO_PLAIN, EPI_BIAS>(p.a, Wp, p.bias, p.out, M, D, st);
    case T2S_ROWS_F_GELUBWD:
        if ((rc = rows_pack32(p.w, 2 * D, D, b, &Wp, st)) || b.oom) return rc;
        return gemm<128, 2, PRO_PLAIN, EPI_GELUBWD>(p.a, Wp, p.bias, p.out, M, 2 * D, st, nullptr, 0, 0, nullptr, p.aux);
    case T2S_ROWS_F_GATE_RES:
        gate_res_kernel<W><<<(M * 32 + 255) / 256, 256, 0, st>>>(p.a, p.res, p.mod, p.gate_off, p.x_out, M, latw);
        break;
    case T2S_ROWS_F_GATE_BWD:
        gate_bwd_kernel<W><<<n_seq, 256, 0, st>>>(p.dx, p.res, p.mod, p.gate_off, p.out, p.dmod, latw);
        break;
    case T2S_ROWS_F_LN_MOD_BWD:
        ln_mod_bwd_kernel<W><<<n_seq, 256, 0, st>>>(p.a, p.ln_x, p.mod, p.shift_off, p.scale_off, p.dx, p.dmod, (const float*)nullptr, 0, (float*)nullptr,
                                                    latw);
        break;
    case T2S_ROWS_F_GELU:
        gelu_kernel<<<((size_t)M * 64 + 255) / 256, 256, 0, st>>>(p.a, p.out, (size_t)M * 64);
        break;
    default: {   // T2S_ROWS_F_FINAL
        const int final_wgs = (M + TAIL_ROWS - 1) / TAIL_ROWS;
        float* part = b.get<float>((size_t)final_wgs * FINAL_COLS);
        if (b.oom) return T2S_OK;
        final_bwd_kernel<false, TAIL_ROWS, W><<<final_wgs, 256, 0, st>>>(p.a, p.dout, p.ln_w, p.ln_b, p.w, p.dx, part, M, nullptr, nullptr, 0, nullptr, latw);
        T2S_LAUNCH_CHECK();
        tail_reduce_kernel<<<(FINAL_COLS + 31) / 32, 256, 0, st>>>(part, final_wgs, FINAL_COLS, FINAL_COLS,
                                                                     TailDst{{p.g_ln_w, p.g_ln_b, p.g_out_w, p.g_out_b}, {D, D, 4 * D, 4}});
        break;
    }
    }
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
}  // namespace

extern "C" int t2s_train_rows(int op, int dtype, int n_tok, int n_seq, int flags, const t2s_train_rows_args* args, void* stream) {
    T2S_REQUIRE(args, "t2s_train_rows: args is NULL");
    T2S_REQUIRE(dtype == T2S_TRAIN_F32 || dtype == T2S_TRAIN_BF16, "t2s_train_rows: unknown dtype %d", dtype);
    const RowsForm* form = nullptr;
    for (const RowsForm& f : ROWS_FORMS)
        if (f.op == op) form = &f;
    T2S_REQUIRE(form, "t2s_train_rows: unknown op %d", op);
    T2S_REQUIRE(form->dtype == dtype, "t2s_train_rows: op %d is a %s launch form, dtype %d was asked", op,
                form->dtype == T2S_TRAIN_BF16 ? "T2S_TRAIN_BF16" : "T2S_TRAIN_F32", dtype);
    T2S_REQUIRE(n_tok == NTOK || n_tok == 800 || n_tok == 1024, "t2s_train_rows: n_tok=%d (480, 800 and 1024 tokens are built)", n_tok);
    T2S_REQUIRE(n_seq > 0 && n_seq <= (1 << 20) / (n_tok / 32), "t2s_train_rows: n_seq=%d", n_seq);
    T2S_REQUIRE((flags & ~2) == 0, "t2s_train_rows: unknown flags %d", flags);
    const t2s_train_rows_args& p = *args;
    const unsigned need = form->need;
    T2S_REQUIRE(!(need & RA) || p.a, "t2s_train_rows: op %d needs a", op);
    T2S_REQUIRE(!(need & RW) || p.w, "t2s_train_rows: op %d needs w", op);
    T2S_REQUIRE(!(need & RMOD) || p.mod, "t2s_train_rows: op %d needs mod", op);
    T2S_REQUIRE(!(need & RRES) || p.res, "t2s_train_rows: op %d needs res", op);
    T2S_REQUIRE(!(need & RAUX) || p.aux, "t2s_train_rows: op %d needs aux", op);
    T2S_REQUIRE(!(need & RLNX) || p.ln_x, "t2s_train_rows: op %d needs ln_x", op);
    T2S_REQUIRE(!(need & RFIN) || (p.dout && p.ln_w && p.ln_b && p.g_ln_w && p.g_ln_b && p.g_out_w && p.g_out_b),
                "t2s_train_rows: op %d needs dout, ln_w, ln_b, g_ln_w, g_ln_b, g_out_w and g_out_b", op);
    T2S_REQUIRE(!(need & ROUT) || p.out, "t2s_train_rows: op %d needs out", op);
    T2S_REQUIRE(!(need & RSAVE) || p.save_a, "t2s_train_rows: op %d needs save_a", op);
    T2S_REQUIRE(!(need & RXOUT) || p.x_out, "t2s_train_rows: op %d needs x_out", op);
    T2S_REQUIRE(!(need & RQKV) || (p.q && p.k && p.v), "t2s_train_rows: op %d needs q, k and v", op);
    T2S_REQUIRE(!(need & RDX) || p.dx, "t2s_train_rows: op %d needs dx", op);
    T2S_REQUIRE(!(need & RDMOD) || p.dmod, "t2s_train_rows: op %d needs dmod", op);
    const bool lnbwd = op == T2S_ROWS_LNBWD256 || op == T2S_ROWS_LNBWD384;
    T2S_REQUIRE(!lnbwd || !p.res || p.out, "t2s_train_rows: op %d with res (f_next) needs out (t_next)", op);
    auto off_ok = [](int off) { return off >= 0 && off <= MODROW - D && off % 4 == 0; };
    T2S_REQUIRE(!(need & RSHIFT) || off_ok(p.shift_off), "t2s_train_rows: shift_off=%d", p.shift_off);
    T2S_REQUIRE(!(need & RSCALE) || off_ok(p.scale_off), "t2s_train_rows: scale_off=%d", p.scale_off);
    T2S_REQUIRE(!((need & RGATE) || (lnbwd && p.res)) || off_ok(p.gate_off), "t2s_train_rows: gate_off=%d", p.gate_off);
    hipStream_t st = (hipStream_t)stream;
    RowsBufs bufs;
    t2s::g_tile_flip = (flags & 2) ? 1u : 0u;               // the direction next_tile_dir() hands the launch (as t2s_wgrad)
    int rc;
    if (dtype == T2S_TRAIN_BF16) {
        rc = n_tok == NTOK ? rows_bf16<NTOK>(op, n_tok, n_seq, p, bufs, st) : rows_bf16<0>(op, n_tok, n_seq, p, bufs, st);
        if (rc == T2S_OK && !bufs.oom) rc = bufs.finish(st);
    } else {
        rc = n_tok == NTOK ? rows_f32<LATW>(op, n_tok, n_seq, p, bufs, st) : rows_f32<0>(op, n_tok, n_seq, p, bufs, st);
    }
    (void)hipStreamSynchronize(st);
    if (rc == T2S_OK && bufs.oom) {
        set_error("t2s_train_rows: out of device memory for the temporaries of op %d at n_seq=%d", op, n_seq);
        rc = T2S_E_HIP;
    }
    return rc;
}
