// TSae: the attention seq2seq codec of the motion models (reference model/pretrained/TSae.py, AttentionSeq2SeqAutoencoder):
// a pre-norm transformer encoder (x (B,T,F) -> memory (B,T,64)), the teacher-forced pre-norm decoder, and the autoregressive
// generation with a key/value cache.  d_model 64, fp32 throughout (fma and v_mfma_f32_32x32x2_f32), no atomics.
//
// Teacher-forced entries (encode, decode) are chains of four row kernels over 32-row tiles of ONE series (grid: tiles x B), so a
// row's value never depends on the batch:
//   tsae_embed_kernel    value embedding + LayerNorm + position | input_projection(target[i-1]) + position (row 0: BOS)
//   tsae_linear_kernel   y (=|+=) Linear([LayerNorm] x): in-projections, out-projections (+ residual), cross K/V, output projection
//   tsae_attn_kernel     softmax(q k^T / sqrt(dh)) v per (64 queries, head, series), keys staged through LDS 64 at a time
//   tsae_ffn_kernel      x += W2 relu(W1 LayerNorm(x) + b1) + b2, the hidden row tile kept in LDS 128 columns at a time
// Generation is one launch of tsae_generate_kernel, one workgroup per series, all S steps inside (after one tsae_linear_kernel
// launch that projects the memory to every layer's cross-attention K / V): the current row lives in LDS, the self-attention K / V
// of the rows written so far in a global cache, the weights are streamed from L2.
// t2s_tsae_update_weights replays the create-time packing (a table of PackItems kept with the blob) in one launch of
// tsae_pack_kernel.  The training entries are t2s_tsae_train.hip; what the two files share is t2s_tsae.h.
#include "t2s_tsae.h"

#include <stddef.h>
#include <string.h>

namespace t2s {
namespace {

using namespace tsae;

struct LinBatch { Lin lin[TS_ML]; };   // blockIdx.z picks one (the cross K / V of every decoder layer in one launch)

// rows of one series, 32 per block: wave w loads rows 8w .. 8w+7 (lane = channel), normalised if ln.g
__device__ __forceinline__ void load_tile(float (*xs)[TS_D + 1], const float* x, int ldx, size_t row0, int t0, int T, Norm ln) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float g = 1.f, be = 0.f;
    if (ln.g) {
        g = ln.g[lane];
        be = ln.b[lane];
    }
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        float v = (t0 + r < T) ? x[(row0 + r) * (size_t)ldx + lane] : 0.f;
        if (ln.g) v = layer_norm_lane(v, g, be);
        xs[r][lane] = v;
    }
}

// src (B,T,F) -> x (B*T,64).  Encoder (shift 0): LayerNorm(W src[i] + b) + pe[i].  Decoder (shift 1): row 0 is the zero BOS row,
// row i > 0 is W src[i-1] + b; + pe[i].  One wave per row, lane = channel.
__global__ __launch_bounds__(256) void tsae_embed_kernel(const float* __restrict__ src, float* __restrict__ x, Lin lin, Norm ln,
                                                         const float* __restrict__ pe, int F, int T, size_t rows, int shift) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int i = (int)(row % (size_t)T);
    float v = 0.f;
    if (!(shift && i == 0)) {
        const float* s = src + (row - shift) * (size_t)F;
        v = lin.b[lane];
        for (int f = 0; f < F; ++f) v = fmaf(s[f], lin.w[f * TS_D + lane], v);
    }
    if (ln.g) v = layer_norm_lane(v, ln.g[lane], ln.b[lane]);
    x[row * TS_D + lane] = v + pe[(size_t)i * TS_D + lane];
}

// y[row][0..nvalid) (= | +=) Linear([LayerNorm] x[row][0..64)), weights (64, N) packed, N a multiple of 32.  grid (tiles, B, nz).
__global__ __launch_bounds__(256) void tsae_linear_kernel(const float* __restrict__ x, int ldx, float* y, int ldy, size_t y_zstride,
                                                          LinBatch lb, Norm ln, int N, int nvalid, int accumulate, int T) {
    __shared__ float xs[32][TS_D + 1];
    const int b = blockIdx.y, t0 = blockIdx.x * 32, z = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
    const size_t row0 = (size_t)b * T + t0;
    load_tile(xs, x, ldx, row0, t0, T, ln);
    __syncthreads();
    const Lin lin = lb.lin[z];
    y += (size_t)z * y_zstride;
    for (int ct = wave; ct < (N >> 5); ct += 4) {
        f32x16 acc = {0};
        acc = tile_gemm(&xs[0][0], TS_D + 1, lin.w, N, ct * 32, 0, TS_D, acc);
        const int col = ct * 32 + (lane & 31);
        if (col >= nvalid) continue;
        const float bias = lin.b[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, half);
            if (t0 + row < T) {
                float* p = y + (row0 + row) * (size_t)ldy + col;
                const float v = acc[r] + bias;
                *p = accumulate ? *p + v : v;
            }
        }
    }
}

// x[row] += W2 relu(W1 LayerNorm(x[row]) + b1) + b2 for the 32 rows of a tile.  The hidden tile goes through LDS 128 columns at a
// time; the second product splits each chunk's k range over the wave pairs {0,1} and {2,3}, added in that order at the end.
__global__ __launch_bounds__(256) void tsae_ffn_kernel(float* x, Lin l1, Lin l2, Norm ln, int dff, int T) {
    __shared__ float xs[32][TS_D + 1];
    __shared__ float hs[32][128 + 1];
    __shared__ float red[2][16][64];
    const int b = blockIdx.y, t0 = blockIdx.x * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
    const size_t row0 = (size_t)b * T + t0;
    load_tile(xs, x, TS_D, row0, t0, T, ln);
    __syncthreads();
    f32x16 acc2 = {0};
    const int ct2 = wave & 1, kh = wave >> 1;
    for (int c0 = 0; c0 < dff; c0 += 128) {
        const int len = min(128, dff - c0);   // 128, or 64 in the last chunk
        if (wave < (len >> 5)) {
            f32x16 h = {0};
            h = tile_gemm(&xs[0][0], TS_D + 1, l1.w, dff, c0 + wave * 32, 0, TS_D, h);
            const int col = wave * 32 + (lane & 31);
            const float bias = l1.b[c0 + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) hs[acc_row(r, half)][col] = fmaxf(h[r] + bias, 0.f);
        }
        __syncthreads();
        acc2 = tile_gemm(&hs[0][0], 128 + 1, l2.w + (size_t)c0 * TS_D, TS_D, ct2 * 32, kh * (len >> 1), (kh + 1) * (len >> 1), acc2);
        __syncthreads();
    }
    if (wave >= 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 2][r][lane] = acc2[r];
    }
    __syncthreads();
    if (wave < 2) {
        const int col = ct2 * 32 + (lane & 31);
        const float bias = l2.b[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, half);
            if (t0 + row < T) {
                float* p = x + (row0 + row) * TS_D + col;
                *p = *p + ((acc2[r] + red[wave][r][lane]) + bias);
            }
        }
    }
}

// o[b, i, h*DH ..] = softmax_j(q_i . k_j * scale) v_j, j < Tk (causal: j <= i).  grid (ceil(Tq/64), H, B), one query per lane;
// 64 keys at a time go through LDS, the running maximum moves once per chunk.
template <int DH>
__global__ __launch_bounds__(64) void tsae_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                       const float* __restrict__ v, int ldkv, float* __restrict__ o, int Tq, int Tk,
                                                       int causal, float scale) {
    __shared__ __attribute__((aligned(16))) float ks[64][DH];
    __shared__ __attribute__((aligned(16))) float vs[64][DH];
    const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int i = blockIdx.x * 64 + lane, ii = min(i, Tq - 1);
    float qr[DH], acc[DH];
    {
        const float* qp = q + ((size_t)b * Tq + ii) * ldq + h * DH;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            qr[d] = qp[d];
            acc[d] = 0.f;
        }
    }
    float m = -INFINITY, l = 0.f;
    const int nk = causal ? min(Tk, blockIdx.x * 64 + 64) : Tk;
    for (int j0 = 0; j0 < nk; j0 += 64) {
        __syncthreads();
        {
            const int jj = j0 + lane;
            const size_t off = ((size_t)b * Tk + min(jj, Tk - 1)) * ldkv + h * DH;
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                *(f32x4*)&ks[lane][d] = *(const f32x4*)(k + off + d);
                *(f32x4*)&vs[lane][d] = *(const f32x4*)(v + off + d);
            }
        }
        __syncthreads();
        float s[64];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) dot = fmaf(qr[d], ks[j][d], dot);
            const bool valid = (j0 + j < Tk) && (!causal || j0 + j <= ii);
            s[j] = valid ? dot * scale : -INFINITY;
            mx = fmaxf(mx, s[j]);
        }
        if (mx > -INFINITY) {
            const float mn = fmaxf(m, mx), c = expf(m - mn);
            l *= c;
#pragma unroll
            for (int d = 0; d < DH; ++d) acc[d] *= c;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const float p = expf(s[j] - mn);
                l += p;
#pragma unroll
                for (int d = 0; d < DH; ++d) acc[d] = fmaf(p, vs[j][d], acc[d]);
            }
            m = mn;
        }
    }
    if (i < Tq) {
        float* op = o + ((size_t)b * Tq + i) * TS_D + h * DH;
        const float inv = 1.0f / l;
#pragma unroll
        for (int d = 0; d < DH; ++d) op[d] = acc[d] * inv;
    }
}

// ---- generation: one workgroup (256 threads) per series -------------------------------------------------------------------
enum { MV_STORE = 0, MV_RELU = 1, MV_ADD = 2 };

// out[n] (= | relu | +=) sum_k in[k] w[k][n] + b[n], in / out in LDS.  Every output's k range is cut in four, the four partial
// sums added as (p0 + p1) + (p2 + p3): the order is a function of (N, K) alone.  Ends with a barrier; `in` must be settled on entry.
__device__ __forceinline__ void gen_matvec(const float* in, float* out, Lin lin, int N, int ldw, int K, int mode, float* part) {
    const int tid = threadIdx.x;
    const int kc = (K + 3) >> 2;
    for (int i = tid; i < 4 * N; i += 256) {
        const int kq = i / N, n = i - kq * N;
        const int k0 = kq * kc, k1 = min(K, k0 + kc);
        const float* w = lin.w + (size_t)k0 * ldw + n;
        float s = 0.f;
#pragma unroll 4
        for (int k = k0; k < k1; ++k, w += ldw) s = fmaf(in[k], *w, s);
        part[kq * N + n] = s;
    }
    __syncthreads();
    for (int n = tid; n < N; n += 256) {
        float s = ((part[n] + part[N + n]) + (part[2 * N + n] + part[3 * N + n])) + lin.b[n];
        if (mode == MV_RELU) s = fmaxf(s, 0.f);
        if (mode == MV_ADD) s += out[n];
        out[n] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void gen_ln(const float* x, float* xn, Norm n) {
    const int tid = threadIdx.x;
    if (tid < 64) xn[tid] = layer_norm_lane(x[tid], n.g[tid], n.b[tid]);
    __syncthreads();
}

// att[h*DH + d] = softmax over rows 0 .. n-1 of (kc, vc) (global, row stride ld) for the query q (LDS).  Thread (h, p) walks rows
// p, p + P, ... with a running softmax; the P partial results of a head are merged in p order.  Ends with a barrier.
template <int DH>
__device__ __forceinline__ void gen_attn(const float* q, const float* kc, const float* vc, int ld, int n, float scale, float* att,
                                         float* pm, float* pl, float* pacc) {
    constexpr int H = TS_D / DH, P = 256 / H;
    const int tid = threadIdx.x, h = tid / P, p = tid % P;
    float qr[DH], acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        qr[d] = q[h * DH + d];
        acc[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = p; j < n; j += P) {
        const size_t off = (size_t)j * ld + h * DH;
        float kr[DH], vr[DH];
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const f32x4 k4 = *(const f32x4*)(kc + off + d), v4 = *(const f32x4*)(vc + off + d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kr[d + e] = k4[e];
                vr[d + e] = v4[e];
            }
        }
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) s = fmaf(qr[d], kr[d], s);
        s *= scale;
        const float mn = fmaxf(m, s), c = expf(m - mn), e = expf(s - mn);
        l = l * c + e;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] = fmaf(e, vr[d], acc[d] * c);
        m = mn;
    }
    pm[tid] = m;
    pl[tid] = l;
#pragma unroll
    for (int d = 0; d < DH; ++d) pacc[tid * 17 + d] = acc[d];
    __syncthreads();
    if (tid < TS_D) {
        const int hh = tid / DH, d = tid % DH;
        float M = -INFINITY;
        for (int pp = 0; pp < P; ++pp) M = fmaxf(M, pm[hh * P + pp]);
        float L = 0.f, O = 0.f;
        for (int pp = 0; pp < P; ++pp) {
            const float e = expf(pm[hh * P + pp] - M);   // 0 for a thread that had no row (m = -inf)
            L = fmaf(pl[hh * P + pp], e, L);
            O = fmaf(pacc[(hh * P + pp) * 17 + d], e, O);
        }
        att[tid] = O / L;
    }
    __syncthreads();
}

// ckv / skv: [layer][series][row][128] (K in columns 0..63, V in 64..127); ckv is read, skv is this kernel's cache: series b's
// workgroup writes row t of every layer at step t and reads rows 0 .. t.  out (B,S,F).
template <int DH>
__global__ __launch_bounds__(256) void tsae_generate_kernel(GenP P, const float* ckv, float* skv, float* __restrict__ out, int S, int B) {
    __shared__ float x[TS_D], xn[TS_D], att[TS_D], o[32];
    __shared__ float buf[TS_MAXFF];
    __shared__ float part[4 * TS_MAXFF];
    __shared__ float pm[256], pl[256], pacc[256 * 17];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float scale = 1.0f / sqrtf((float)DH);
    if (tid < TS_D) x[tid] = P.pe[tid];   // the zero BOS row + position 0
    __syncthreads();
    for (int t = 0; t < S; ++t) {
        for (int l = 0; l < P.n_dec; ++l) {
            const DecLayerP& Lp = P.L[l];
            const size_t base = ((size_t)l * B + b) * (size_t)S * 128;
            float* kv = skv + base;
            const float* ck = ckv + base;
            gen_ln(x, xn, Lp.n1);
            gen_matvec(xn, buf, Lp.qkv, 3 * TS_D, 3 * TS_D, TS_D, MV_STORE, part);
            if (tid >= TS_D && tid < 3 * TS_D) kv[(size_t)t * 128 + tid - TS_D] = buf[tid];
            __threadfence_block();
            __syncthreads();
            gen_attn<DH>(buf, kv, kv + TS_D, 128, t + 1, scale, att, pm, pl, pacc);
            gen_matvec(att, x, Lp.out, TS_D, TS_D, TS_D, MV_ADD, part);
            gen_ln(x, xn, Lp.n2);
            gen_matvec(xn, buf, Lp.cq, TS_D, TS_D, TS_D, MV_STORE, part);
            gen_attn<DH>(buf, ck, ck + TS_D, 128, S, scale, att, pm, pl, pacc);
            gen_matvec(att, x, Lp.cout, TS_D, TS_D, TS_D, MV_ADD, part);
            gen_ln(x, xn, Lp.n3);
            gen_matvec(xn, buf, Lp.l1, P.dff, P.dff, TS_D, MV_RELU, part);
            gen_matvec(buf, x, Lp.l2, TS_D, TS_D, P.dff, MV_ADD, part);
        }
        gen_matvec(x, o, P.outp, P.F, 32, TS_D, MV_STORE, part);
        if (tid < P.F) out[((size_t)b * S + t) * P.F + tid] = o[tid];
        if (t + 1 < S) {
            gen_matvec(o, x, P.inp, TS_D, TS_D, P.F, MV_STORE, part);
            if (tid < TS_D) x[tid] += P.pe[(size_t)(t + 1) * TS_D + tid];
            __syncthreads();
        }
    }
}

// One workgroup per PackItem: the create-time packing of one tensor pair, from the caller's tensors as they are now.
__global__ __launch_bounds__(256) void tsae_pack_kernel(t2s_tsae_weights w, const PackItem* __restrict__ items, float* __restrict__ blob) {
    const PackItem it = items[blockIdx.x];
    const float* sw = *(const float* const*)((const char*)&w + it.w_field);
    const float* sb = *(const float* const*)((const char*)&w + it.b_field);
    for (int i = threadIdx.x; i < it.N * it.K; i += 256) {
        const int n = i / it.K, k = i - n * it.K;
        const float v = sw[(size_t)it.r0 * it.K + i];
        blob[it.off_w + (size_t)k * it.Npad + n] = v;
        if (it.off_t) blob[it.off_t + i] = v;
    }
    for (int n = threadIdx.x; n < it.N; n += 256) blob[it.off_b + n] = sb[it.r0 + n];
}

}  // namespace
}  // namespace t2s

using namespace t2s;
using namespace t2s::tsae;

namespace {

// Host-side packing: tensors are read back once, transposed into one blob (offsets in floats, every item 64-float aligned).
struct Packer {
    const t2s_tsae_weights* W;
    std::vector<float> blob;
    std::vector<float> tmp;
    std::vector<PackItem> items;
    int rc = T2S_OK;

    uint32_t field(const float* const& p) const { return (uint32_t)((const char*)&p - (const char*)W); }

    size_t reserve(size_t n) {
        const size_t off = blob.size();
        blob.resize(off + ((n + 63) & ~(size_t)63), 0.f);
        return off;
    }
    bool fetch(const float* p, size_t n, const char* name) {
        if (rc != T2S_OK) return false;
        if (!p) {
            set_error("t2s_tsae_create: %s is NULL", name);
            rc = T2S_E_INVALID;
            return false;
        }
        if (check_device_extent(p, n * sizeof(float), name) != T2S_OK) {
            rc = T2S_E_INVALID;
            return false;
        }
        tmp.resize(n);
        const hipError_t e = hipMemcpy(tmp.data(), p, n * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("t2s_tsae_create: reading %s failed: %s", name, hipGetErrorString(e));
            rc = T2S_E_HIP;
            return false;
        }
        return true;
    }
    // rows [r0, r0 + N) of a torch Linear weight (Nall, K) and its bias -> (K, Npad) + (Npad) and, if want_t, the rows as they are
    // (N rounded up to 32, K); offsets returned as w, b, t.  w and b are MEMBERS of *W: their place in the struct goes into the item.
    void lin(const float* const& w, const float* const& b, int Nall, int r0, int N, int K, int Npad, bool want_t, const char* name,
             size_t off[3]) {
        off[0] = off[1] = off[2] = 0;
        if (!fetch(w, (size_t)Nall * K, name)) return;
        off[0] = reserve((size_t)K * Npad);
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) blob[off[0] + (size_t)k * Npad + n] = tmp[(size_t)(r0 + n) * K + k];
        if (want_t) {
            off[2] = reserve((size_t)((N + 31) & ~31) * K);
            memcpy(&blob[off[2]], &tmp[(size_t)r0 * K], (size_t)N * K * sizeof(float));
        }
        if (!fetch(b, (size_t)Nall, name)) return;
        off[1] = reserve(Npad);
        for (int n = 0; n < N; ++n) blob[off[1] + n] = tmp[r0 + n];
        items.push_back(PackItem{field(w), field(b), r0, N, K, Npad, (uint32_t)off[0], (uint32_t)off[1], (uint32_t)off[2]});
    }
    void norm(const float* const& g, const float* const& b, const char* name, size_t off[3]) {
        lin(g, b, TS_D, 0, TS_D, 1, TS_D, false, name, off);
    }
};

struct OffLayer { size_t qkv[3], out[3], cq[3], ckv[3], cout[3], l1[3], l2[3], n1[3], n2[3], n3[3]; };

inline Lin mk_lin(const float* base, const size_t off[3]) { return Lin{base + off[0], base + off[1], off[2] ? base + off[2] : nullptr}; }
inline Norm mk_norm(const float* base, const size_t off[3]) { return Norm{base + off[0], base + off[1]}; }

// floats of workspace per (series x row): encode needs qkv + attention output, decode x + qkv + attention output + every layer's
// cross K / V, generate every layer's cross K / V and self K / V cache
inline size_t ws_floats_per_row(const t2s_tsae* h) {
    const size_t enc = 3 * TS_D + TS_D, dec = TS_D + 3 * TS_D + TS_D + (size_t)h->n_dec * 128, gen = (size_t)h->n_dec * 256;
    return enc > dec ? (enc > gen ? enc : gen) : (dec > gen ? dec : gen);
}

int check_call(const char* who, const t2s_tsae* h, int B, int T, const void* ws, uint64_t ws_bytes) {
    T2S_REQUIRE(h != nullptr, "%s: handle is NULL", who);
    T2S_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d unsupported (1..65535)", who, B);
    T2S_REQUIRE(T >= 1 && T <= TS_MAXT, "%s: T=%d unsupported (1..%d, the positional table)", who, T, TS_MAXT);
    T2S_REQUIRE(ws != nullptr, "%s: workspace is NULL", who);
    T2S_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const uint64_t need = (uint64_t)B * T * ws_floats_per_row(h) * sizeof(float);
    T2S_REQUIRE(ws_bytes >= need, "%s: workspace of %llu bytes is too small: B=%d T=%d needs %llu (t2s_tsae_workspace_bytes)", who,
                (unsigned long long)ws_bytes, B, T, (unsigned long long)need);
    return T2S_OK;
}

int launch_linear(const float* x, int ldx, float* y, int ldy, size_t zstride, const LinBatch& lb, int nz, Norm ln, int N, int nvalid,
                  int accumulate, int B, int T, hipStream_t s) {
    tsae_linear_kernel<<<dim3((T + 31) / 32, B, nz), 256, 0, s>>>(x, ldx, y, ldy, zstride, lb, ln, N, nvalid, accumulate, T);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
int launch_linear1(const float* x, int ldx, float* y, int ldy, Lin lin, Norm ln, int N, int nvalid, int accumulate, int B, int T,
                   hipStream_t s) {
    LinBatch lb{};
    lb.lin[0] = lin;
    return launch_linear(x, ldx, y, ldy, 0, lb, 1, ln, N, nvalid, accumulate, B, T, s);
}

int launch_attn(int heads, const float* q, int ldq, const float* k, const float* v, int ldkv, float* o, int B, int Tq, int Tk, int causal,
                hipStream_t s) {
    const dim3 grid((Tq + 63) / 64, heads, B);
    if (heads == 8)
        tsae_attn_kernel<8><<<grid, 64, 0, s>>>(q, ldq, k, v, ldkv, o, Tq, Tk, causal, 1.0f / sqrtf(8.0f));
    else
        tsae_attn_kernel<16><<<grid, 64, 0, s>>>(q, ldq, k, v, ldkv, o, Tq, Tk, causal, 1.0f / sqrtf(16.0f));
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int launch_cross_kv(const t2s_tsae* h, const float* memory, float* ckv, int B, int T, hipStream_t s) {
    LinBatch lb{};
    for (int l = 0; l < h->n_dec; ++l) lb.lin[l] = h->dec.L[l].ckv;
    return launch_linear(memory, TS_D, ckv, 128, (size_t)B * T * 128, lb, h->n_dec, Norm{nullptr, nullptr}, 128, 128, 0, B, T, s);
}

}  // namespace

extern "C" int t2s_tsae_create(const t2s_tsae_weights* w, t2s_tsae** out) {
    T2S_REQUIRE(w != nullptr && out != nullptr, "t2s_tsae_create: NULL argument");
    *out = nullptr;
    T2S_REQUIRE(w->d_model == TS_D, "t2s_tsae_create: d_model=%d unsupported (64)", w->d_model);
    T2S_REQUIRE(w->heads == 4 || w->heads == 8, "t2s_tsae_create: heads=%d unsupported (4 or 8)", w->heads);
    T2S_REQUIRE(w->d_ff >= 64 && w->d_ff <= TS_MAXFF && w->d_ff % 64 == 0,
                "t2s_tsae_create: d_ff=%d unsupported (a multiple of 64, at most %d)", w->d_ff, TS_MAXFF);
    // a one-sided handle (an encoder alone: n_dec 0; a decoder alone: n_enc 0) reads that side's tensors only
    T2S_REQUIRE(w->n_enc >= 0 && w->n_enc <= TS_ML, "t2s_tsae_create: n_enc=%d unsupported (1..%d, or 0 for a decoder alone)", w->n_enc, TS_ML);
    T2S_REQUIRE(w->n_dec >= 0 && w->n_dec <= TS_ML, "t2s_tsae_create: n_dec=%d unsupported (1..%d, or 0 for an encoder alone)", w->n_dec, TS_ML);
    T2S_REQUIRE(w->n_enc + w->n_dec >= 1, "t2s_tsae_create: n_enc=0 and n_dec=0: a handle needs at least one side");
    T2S_REQUIRE(w->n_features >= 1 && w->n_features <= TS_MAXF, "t2s_tsae_create: n_features=%d unsupported (1..%d)", w->n_features,
                TS_MAXF);
    const int F = w->n_features, dff = w->d_ff;
    Packer pk;
    pk.W = w;
    size_t emb[3] = {0, 0, 0}, emb_ln[3] = {0, 0, 0}, inp[3] = {0, 0, 0}, outp[3] = {0, 0, 0};
    OffLayer eo[TS_ML], dol[TS_ML];
    pk.reserve(64);   // offset 0 stays unused
    if (w->n_enc) {
        pk.lin(w->value_embedding_w, w->value_embedding_b, TS_D, 0, TS_D, F, TS_D, false, "encoder.value_embedding", emb);
        pk.norm(w->embedding_ln_w, w->embedding_ln_b, "encoder.embedding_ln", emb_ln);
    }
    for (int l = 0; l < w->n_enc; ++l) {
        const t2s_tsae_enc_layer& L = w->enc[l];
        pk.lin(L.self_attn.in_proj_w, L.self_attn.in_proj_b, 3 * TS_D, 0, 3 * TS_D, TS_D, 3 * TS_D, true, "encoder self_attn.in_proj", eo[l].qkv);
        pk.lin(L.self_attn.out_proj_w, L.self_attn.out_proj_b, TS_D, 0, TS_D, TS_D, TS_D, true, "encoder self_attn.out_proj", eo[l].out);
        pk.lin(L.linear1_w, L.linear1_b, dff, 0, dff, TS_D, dff, true, "encoder linear1", eo[l].l1);
        pk.lin(L.linear2_w, L.linear2_b, TS_D, 0, TS_D, dff, TS_D, true, "encoder linear2", eo[l].l2);
        pk.norm(L.norm1_w, L.norm1_b, "encoder norm1", eo[l].n1);
        pk.norm(L.norm2_w, L.norm2_b, "encoder norm2", eo[l].n2);
    }
    for (int l = 0; l < w->n_dec; ++l) {
        const t2s_tsae_dec_layer& L = w->dec[l];
        pk.lin(L.self_attn.in_proj_w, L.self_attn.in_proj_b, 3 * TS_D, 0, 3 * TS_D, TS_D, 3 * TS_D, true, "decoder self_attn.in_proj", dol[l].qkv);
        pk.lin(L.self_attn.out_proj_w, L.self_attn.out_proj_b, TS_D, 0, TS_D, TS_D, TS_D, true, "decoder self_attn.out_proj", dol[l].out);
        pk.lin(L.multihead_attn.in_proj_w, L.multihead_attn.in_proj_b, 3 * TS_D, 0, TS_D, TS_D, TS_D, true, "decoder multihead_attn.in_proj",
               dol[l].cq);
        pk.lin(L.multihead_attn.in_proj_w, L.multihead_attn.in_proj_b, 3 * TS_D, TS_D, 2 * TS_D, TS_D, 2 * TS_D, true,
               "decoder multihead_attn.in_proj", dol[l].ckv);
        pk.lin(L.multihead_attn.out_proj_w, L.multihead_attn.out_proj_b, TS_D, 0, TS_D, TS_D, TS_D, true, "decoder multihead_attn.out_proj",
               dol[l].cout);
        pk.lin(L.linear1_w, L.linear1_b, dff, 0, dff, TS_D, dff, true, "decoder linear1", dol[l].l1);
        pk.lin(L.linear2_w, L.linear2_b, TS_D, 0, TS_D, dff, TS_D, true, "decoder linear2", dol[l].l2);
        pk.norm(L.norm1_w, L.norm1_b, "decoder norm1", dol[l].n1);
        pk.norm(L.norm2_w, L.norm2_b, "decoder norm2", dol[l].n2);
        pk.norm(L.norm3_w, L.norm3_b, "decoder norm3", dol[l].n3);
    }
    if (w->n_dec) {
        pk.lin(w->input_projection_w, w->input_projection_b, TS_D, 0, TS_D, F, TS_D, false, "decoder.input_projection", inp);
        pk.lin(w->output_projection_w, w->output_projection_b, F, 0, F, TS_D, 32, true, "decoder.output_projection", outp);
    }
    if (pk.rc != T2S_OK) return pk.rc;
    // The sinusoidal table, a function of (position, channel): the divisor 10000^(-2i/64) and the angle are formed in fp32 as the
    // reference forms them, exp / sin / cos are evaluated in double and rounded once.
    const size_t pe = pk.reserve((size_t)TS_MAXT * TS_D);
    const float step = (float)(-(log(10000.0) / TS_D));
    for (int i = 0; i < TS_D / 2; ++i) {
        const float div = (float)exp((double)((float)(2 * i) * step));
        for (int p = 0; p < TS_MAXT; ++p) {
            const float ang = (float)p * div;
            pk.blob[pe + (size_t)p * TS_D + 2 * i] = (float)sin((double)ang);
            pk.blob[pe + (size_t)p * TS_D + 2 * i + 1] = (float)cos((double)ang);
        }
    }
    // the items ride behind the table, for the device replay of this packing (t2s_tsae_update_weights)
    const size_t items_off = pk.reserve((pk.items.size() * sizeof(PackItem) + sizeof(float) - 1) / sizeof(float));
    memcpy(&pk.blob[items_off], pk.items.data(), pk.items.size() * sizeof(PackItem));
    t2s_tsae* h = new t2s_tsae();
    hipError_t e = hipMalloc((void**)&h->blob, pk.blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->blob, pk.blob.data(), pk.blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("t2s_tsae_create: uploading the packed weights failed: %s", hipGetErrorString(e));
        if (h->blob) (void)hipFree(h->blob);
        delete h;
        return T2S_E_HIP;
    }
    const float* base = h->blob;
    h->F = F, h->dff = dff, h->heads = w->heads, h->n_enc = w->n_enc, h->n_dec = w->n_dec;
    h->emb = mk_lin(base, emb);
    h->emb_ln = mk_norm(base, emb_ln);
    for (int l = 0; l < h->n_enc; ++l)
        h->enc[l] = EncLayerP{mk_lin(base, eo[l].qkv), mk_lin(base, eo[l].out), mk_lin(base, eo[l].l1), mk_lin(base, eo[l].l2),
                              mk_norm(base, eo[l].n1), mk_norm(base, eo[l].n2)};
    for (int l = 0; l < h->n_dec; ++l)
        h->dec.L[l] = DecLayerP{mk_lin(base, dol[l].qkv), mk_lin(base, dol[l].out), mk_lin(base, dol[l].cq), mk_lin(base, dol[l].ckv),
                                mk_lin(base, dol[l].cout), mk_lin(base, dol[l].l1), mk_lin(base, dol[l].l2), mk_norm(base, dol[l].n1),
                                mk_norm(base, dol[l].n2), mk_norm(base, dol[l].n3)};
    h->dec.inp = mk_lin(base, inp);
    h->dec.outp = mk_lin(base, outp);
    h->dec.pe = base + pe;
    h->items = pk.items;
    h->items_dev = (PackItem*)(h->blob + items_off);
    h->dec.n_dec = h->n_dec, h->dec.dff = dff, h->dec.F = F;
    *out = h;
    return T2S_OK;
}

extern "C" int t2s_tsae_update_weights(t2s_tsae* h, const t2s_tsae_weights* w, void* stream) {
    T2S_REQUIRE(h != nullptr && w != nullptr, "t2s_tsae_update_weights: NULL argument");
    T2S_REQUIRE(w->n_features == h->F && w->d_model == TS_D && w->d_ff == h->dff && w->heads == h->heads && w->n_enc == h->n_enc &&
                    w->n_dec == h->n_dec,
                "t2s_tsae_update_weights: the shape (n_features=%d d_model=%d d_ff=%d heads=%d n_enc=%d n_dec=%d) is not the handle's "
                "(%d %d %d %d %d %d): create a new handle",
                w->n_features, w->d_model, w->d_ff, w->heads, w->n_enc, w->n_dec, h->F, TS_D, h->dff, h->heads, h->n_enc, h->n_dec);
    for (const PackItem& it : h->items) {
        const float* sw = *(const float* const*)((const char*)w + it.w_field);
        const float* sb = *(const float* const*)((const char*)w + it.b_field);
        T2S_REQUIRE(sw != nullptr && sb != nullptr, "t2s_tsae_update_weights: a tensor is NULL (pointer at byte %u / %u of t2s_tsae_weights)",
                    it.w_field, it.b_field);
        TS_TRY(check_device_extent(sw, (size_t)(it.r0 + it.N) * it.K * sizeof(float), "t2s_tsae_update_weights: a weight"));
        TS_TRY(check_device_extent(sb, (size_t)(it.r0 + it.N) * sizeof(float), "t2s_tsae_update_weights: a bias"));
    }
    tsae_pack_kernel<<<(unsigned)h->items.size(), 256, 0, (hipStream_t)stream>>>(*w, h->items_dev, h->blob);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" void t2s_tsae_destroy(t2s_tsae* h) {
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

extern "C" int t2s_tsae_positional(const t2s_tsae* h, float* pe, int first, int count, void* stream) {
    T2S_REQUIRE(h != nullptr && pe != nullptr, "t2s_tsae_positional: NULL argument");
    T2S_REQUIRE(first >= 0 && count >= 1 && first + count <= TS_MAXT, "t2s_tsae_positional: rows [%d, %d) outside 0..%d", first,
                first + count, TS_MAXT);
    T2S_HIP_CHECK(hipMemcpyAsync(pe, h->dec.pe + (size_t)first * TS_D, (size_t)count * TS_D * sizeof(float), hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
    return T2S_OK;
}

extern "C" uint64_t t2s_tsae_workspace_bytes(const t2s_tsae* h, int B, int T) {
    if (!h || B < 1 || T < 1 || T > TS_MAXT) {
        set_error("t2s_tsae_workspace_bytes: handle NULL, B=%d or T=%d out of range (T 1..%d)", B, T, TS_MAXT);
        return 0;
    }
    return (uint64_t)B * T * ws_floats_per_row(h) * sizeof(float);
}

extern "C" int t2s_tsae_encode(const t2s_tsae* h, const float* x, float* memory, int B, int T, void* workspace, uint64_t workspace_bytes,
                               void* stream) {
    TS_TRY(check_call("t2s_tsae_encode", h, B, T, workspace, workspace_bytes));
    T2S_REQUIRE(h->n_enc >= 1, "t2s_tsae_encode: the handle was created without an encoder (n_enc=0)");
    T2S_REQUIRE(x != nullptr && memory != nullptr, "t2s_tsae_encode: NULL tensor");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * T;
    float* qkv = (float*)workspace;
    float* att = qkv + rows * 3 * TS_D;
    const Norm none{nullptr, nullptr};
    tsae_embed_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(x, memory, h->emb, h->emb_ln, h->dec.pe, h->F, T, rows, 0);
    T2S_LAUNCH_CHECK();
    for (int l = 0; l < h->n_enc; ++l) {
        const EncLayerP& L = h->enc[l];
        TS_TRY(launch_linear1(memory, TS_D, qkv, 3 * TS_D, L.qkv, L.n1, 3 * TS_D, 3 * TS_D, 0, B, T, s));
        TS_TRY(launch_attn(h->heads, qkv, 3 * TS_D, qkv + TS_D, qkv + 2 * TS_D, 3 * TS_D, att, B, T, T, 0, s));
        TS_TRY(launch_linear1(att, TS_D, memory, TS_D, L.out, none, TS_D, TS_D, 1, B, T, s));
        tsae_ffn_kernel<<<dim3((T + 31) / 32, B), 256, 0, s>>>(memory, L.l1, L.l2, L.n2, h->dff, T);
        T2S_LAUNCH_CHECK();
    }
    return T2S_OK;
}

extern "C" int t2s_tsae_decode(const t2s_tsae* h, const float* memory, const float* target, float* prediction, int B, int T,
                               void* workspace, uint64_t workspace_bytes, void* stream) {
    TS_TRY(check_call("t2s_tsae_decode", h, B, T, workspace, workspace_bytes));
    T2S_REQUIRE(h->n_dec >= 1, "t2s_tsae_decode: the handle was created without a decoder (n_dec=0)");
    T2S_REQUIRE(memory != nullptr && target != nullptr && prediction != nullptr, "t2s_tsae_decode: NULL tensor");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * T;
    float* x = (float*)workspace;
    float* qkv = x + rows * TS_D;
    float* att = qkv + rows * 3 * TS_D;
    float* ckv = att + rows * TS_D;
    const Norm none{nullptr, nullptr};
    tsae_embed_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(target, x, h->dec.inp, none, h->dec.pe, h->F, T, rows, 1);
    T2S_LAUNCH_CHECK();
    TS_TRY(launch_cross_kv(h, memory, ckv, B, T, s));
    for (int l = 0; l < h->n_dec; ++l) {
        const DecLayerP& L = h->dec.L[l];
        const float* ck = ckv + (size_t)l * rows * 128;
        TS_TRY(launch_linear1(x, TS_D, qkv, 3 * TS_D, L.qkv, L.n1, 3 * TS_D, 3 * TS_D, 0, B, T, s));
        TS_TRY(launch_attn(h->heads, qkv, 3 * TS_D, qkv + TS_D, qkv + 2 * TS_D, 3 * TS_D, att, B, T, T, 1, s));
        TS_TRY(launch_linear1(att, TS_D, x, TS_D, L.out, none, TS_D, TS_D, 1, B, T, s));
        TS_TRY(launch_linear1(x, TS_D, qkv, TS_D, L.cq, L.n2, TS_D, TS_D, 0, B, T, s));
        TS_TRY(launch_attn(h->heads, qkv, TS_D, ck, ck + TS_D, 128, att, B, T, T, 0, s));
        TS_TRY(launch_linear1(att, TS_D, x, TS_D, L.cout, none, TS_D, TS_D, 1, B, T, s));
        tsae_ffn_kernel<<<dim3((T + 31) / 32, B), 256, 0, s>>>(x, L.l1, L.l2, L.n3, h->dff, T);
        T2S_LAUNCH_CHECK();
    }
    TS_TRY(launch_linear1(x, TS_D, prediction, h->F, h->dec.outp, none, 32, h->F, 0, B, T, s));
    return T2S_OK;
}

extern "C" int t2s_tsae_generate(const t2s_tsae* h, const float* memory, float* series, int B, int S, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    TS_TRY(check_call("t2s_tsae_generate", h, B, S, workspace, workspace_bytes));
    T2S_REQUIRE(h->n_dec >= 1, "t2s_tsae_generate: the handle was created without a decoder (n_dec=0)");
    T2S_REQUIRE(memory != nullptr && series != nullptr, "t2s_tsae_generate: NULL tensor");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * S;
    float* ckv = (float*)workspace;
    float* skv = ckv + (size_t)h->n_dec * rows * 128;
    TS_TRY(launch_cross_kv(h, memory, ckv, B, S, s));
    if (h->heads == 8)
        tsae_generate_kernel<8><<<B, 256, 0, s>>>(h->dec, ckv, skv, series, S, B);
    else
        tsae_generate_kernel<16><<<B, 256, 0, s>>>(h->dec, ckv, skv, series, S, B);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
