// Attention for the TRAINING path (plain layouts, fp32 MFMA): forward that also emits the row
// log-sum-exp, and the flash-style backward (timm 1.0.11 Attention core; reference call site
// model/denoiser/transformer.py:116 under autograd, train.py:123-125).
//
// With n = tokens per sequence (480; 800 / 1024 at the wide latent widths):
// q, k, v: (BH, n, 32) with bh = seq*4 + head.  o, do: token rows (S*n, 128), head h at
// columns 32h..32h+31.  dqkv: token rows (S*n, 384) = [dq | dk | dv] x heads, i.e. the gradient
// of the qkv linear's output.  lse: (BH, n) in the log2 domain: m + log2(sum 2^(s - m)) with
// s = q.k * 32^-0.5 * log2(e).
//
// Backward, with P recomputed from lse (no N x N tensor is stored):
//   D_i   = sum_d dO[i][d] O[i][d]
//   dS    = P o (dP - D_i),  dP = dO V^T
//   dQ    = scale * dS K          (kernel A: queries on the lanes, transposed tiles as in forward)
//   dK    = scale * dS^T Q,  dV = P^T dO   (kernel B: keys on the lanes)
// Each kernel keeps two (n x 32) operands of its (sequence, head) in LDS (row stride 36) and the
// other two in registers / streams them; the f32 accumulator layout is reused directly as the next
// MFMA's B operand (one register per lane), exactly as in the forward kernels.
//
// Token counts.  NT = 480 (compile time): the two operands are staged whole (142,080 B), one workgroup per (sequence, head),
// its 8 waves walk the 15 tiles.  NT = 0 (run time, n_tok a multiple of 32; 800 and 1024 are used): two whole operands no
// longer fit a CU's 160 KB, so the LDS pair is staged in chunks of CHB = 16 blocks (512 rows, 151,552 B with the two row
// vectors) and the block loop runs inside a loop over chunks.  The accumulators stay in registers across chunks (the
// forward's running max / sum / O by the online-softmax step the block loop already takes; dq, dk, dv additively, P being
// recomputed from the lse), so a wave owns ONE tile: a head's tiles are dealt over gridDim.y workgroups, tile = y +
// gridDim.y * wave (25 tiles at 800 tokens over 4 workgroups: 7, 6, 6, 6).  The per-block arithmetic and its order are
// the same functions in both forms.  No atomics; every output element has one writer and one fixed summation order.
#include "t2s_common.h"

namespace t2s {

namespace {
constexpr int STR = 36;            // padded LDS row stride (floats)
constexpr int LDS2 = 2 * NTOK * STR * 4 + 2 * NTOK * 4;   // two operands + two per-row vectors = 142,080 B
constexpr int CHB = 16;            // run-time token count: blocks of 32 rows per LDS chunk
constexpr int CHR = CHB * 32;      // 512 rows
constexpr int LDSW = 2 * CHR * STR * 4 + 2 * CHR * 4;     // 151,552 B
static_assert(LDSW <= 160 * 1024, "a chunk pair must fit a CU's LDS");
constexpr float SCALE = 0.17677669529663687f;
constexpr float QS = SCALE * 1.4426950408889634f;

__device__ __forceinline__ float pair_max_f(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pair_sum_f(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// stage `rows` rows of a (.,32) row-major matrix into LDS with row stride STR
__device__ __forceinline__ void stage_rows(float* dst, const float* src, int src_row_stride, int rows, int tid, int nthreads) {
    for (int idx = tid; idx < rows * 8; idx += nthreads) {
        const int row = idx >> 3, c4 = idx & 7;
        *reinterpret_cast<f32x4*>(dst + row * STR + c4 * 4) =
            *reinterpret_cast<const f32x4*>(src + (size_t)row * src_row_stride + c4 * 4);
    }
}

// ---- forward: one 32-query tile of a wave against the nb key blocks staged at Ks / Vs (online softmax)
struct FwdTile {
    f32x4 qf[4];
    f32x16 ot;
    float m_run, l_lane;
};
__device__ __forceinline__ void fwd_tile_begin(FwdTile& t, const float* qrow) {   // qrow: this lane's query row + 4 * half
#pragma unroll
    for (int g = 0; g < 4; ++g) t.qf[g] = *reinterpret_cast<const f32x4*>(qrow + 8 * g) * QS;
#pragma unroll
    for (int r = 0; r < 16; ++r) t.ot[r] = 0.f;
    t.m_run = -INFINITY;
    t.l_lane = 0.f;
}
__device__ __forceinline__ void fwd_tile_blocks(FwdTile& t, const float* Ks, const float* Vs, int nb, int half, int i) {
    for (int jb = 0; jb < nb; ++jb) {
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
        const float* krow = Ks + (jb * 32 + i) * STR + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kf = *reinterpret_cast<const f32x4*>(krow + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) st = mfma32(kf[e], t.qf[g][e], st);
        }
        float mloc = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, st[r]);
        mloc = pair_max_f(mloc);
        const float m_new = fmaxf(t.m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f(t.m_run - m_new);
        t.m_run = m_new;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            st[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
            ps += st[r];
            t.ot[r] *= alpha;
        }
        t.l_lane = t.l_lane * alpha + ps;
        const float* vrow = Vs + (jb * 32 + 4 * half) * STR + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) t.ot = mfma32(vrow[((r & 3) + 8 * (r >> 2)) * STR], st[r], t.ot);
    }
}
__device__ __forceinline__ void fwd_tile_end(const FwdTile& t, float* orow, float* lse_tok, int half) {   // orow: + 4 * half
    const float l_tot = pair_sum_f(t.l_lane);
    const float inv = 1.0f / l_tot;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 w = {t.ot[4 * g] * inv, t.ot[4 * g + 1] * inv, t.ot[4 * g + 2] * inv, t.ot[4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 8 * g) = w;
    }
    if (half == 0) *lse_tok = t.m_run + __builtin_amdgcn_logf(l_tot);   // v_log_f32 = log2
}

// ---- dQ: one 32-query tile against the nb key blocks staged at Ks / Vs
struct DqTile {
    f32x4 qf[4], dof[4];   // B operands: Q^T (pre-scaled, log2 domain) and dO^T of this lane's query
    float lse_i, d_i;
    f32x16 dq;
};
__device__ __forceinline__ void dq_tile_begin(DqTile& t, const float* qrow, const float* dorow, float lse_i, float d_i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        t.qf[g] = *reinterpret_cast<const f32x4*>(qrow + 8 * g) * QS;
        t.dof[g] = *reinterpret_cast<const f32x4*>(dorow + 8 * g);
    }
    t.lse_i = lse_i;
    t.d_i = d_i;
#pragma unroll
    for (int r = 0; r < 16; ++r) t.dq[r] = 0.f;
}
__device__ __forceinline__ void dq_tile_blocks(DqTile& t, const float* Ks, const float* Vs, int nb, int half, int i) {
    for (int jb = 0; jb < nb; ++jb) {
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
        const float* krow = Ks + (jb * 32 + i) * STR + 4 * half;
        const float* vrw = Vs + (jb * 32 + i) * STR + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kf = *reinterpret_cast<const f32x4*>(krow + 8 * g);
            const f32x4 vf = *reinterpret_cast<const f32x4*>(vrw + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                st = mfma32(kf[e], t.qf[g][e], st);     // S^T[key][query]  (log2 domain)
                dp = mfma32(vf[e], t.dof[g][e], dp);    // dP^T[key][query] = V dO^T
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(st[r] - t.lse_i);
            st[r] = p * (dp[r] - t.d_i);                // dS^T
        }
        // dQ^T[d][query] += K^T[d][key] dS^T[key][query]: A = K column d over the key pair of step r
        const float* kcol = Ks + (jb * 32 + 4 * half) * STR + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) t.dq = mfma32(kcol[((r & 3) + 8 * (r >> 2)) * STR], st[r], t.dq);
    }
}
__device__ __forceinline__ void dq_tile_end(const DqTile& t, float* dst) {   // dst: the dq block of this lane's row + 4 * half
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 w = {t.dq[4 * g] * SCALE, t.dq[4 * g + 1] * SCALE, t.dq[4 * g + 2] * SCALE, t.dq[4 * g + 3] * SCALE};
        *reinterpret_cast<f32x4*>(dst + 8 * g) = w;
    }
}

// ---- dK, dV: one 32-key tile against the nb query blocks staged at Qs / Os / Ls / Ds
struct DkvTile {
    f32x4 kf[4], vf[4];   // B operands: K^T (pre-scaled to the log2 domain) and V^T of this lane's key
    f32x16 dk, dv;
};
__device__ __forceinline__ void dkv_tile_begin(DkvTile& t, const float* krow, const float* vrow) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        t.kf[g] = *reinterpret_cast<const f32x4*>(krow + 8 * g) * QS;
        t.vf[g] = *reinterpret_cast<const f32x4*>(vrow + 8 * g);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) t.dk[r] = t.dv[r] = 0.f;
}
__device__ __forceinline__ void dkv_tile_blocks(DkvTile& t, const float* Qs, const float* Os, const float* Ls, const float* Ds,
                                                int nb, int half, int j) {
    for (int qb = 0; qb < nb; ++qb) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
        const float* qrow = Qs + (qb * 32 + j) * STR + 4 * half;    // A operand row = query (lane index j)
        const float* orow = Os + (qb * 32 + j) * STR + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 qa = *reinterpret_cast<const f32x4*>(qrow + 8 * g);
            const f32x4 oa = *reinterpret_cast<const f32x4*>(orow + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s = mfma32(qa[e], t.kf[g][e], s);      // S[query][key]   (registers = queries, lane = key)
                dp = mfma32(oa[e], t.vf[g][e], dp);    // dP[query][key] = dO V^T
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;   // query of register r in this half
            const float p = __builtin_amdgcn_exp2f(s[r] - Ls[qi]);
            dp[r] = p * (dp[r] - Ds[qi]);   // dS[query][key]
            s[r] = p;                       // P[query][key]
        }
        // dV^T[d][key] += dO^T[d][query] P[query][key] ; dK^T[d][key] += Q^T[d][query] dS[query][key]
        const float* ocol = Os + (qb * 32 + 4 * half) * STR + j;    // lane index j = feature d here
        const float* qcol = Qs + (qb * 32 + 4 * half) * STR + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ro = ((r & 3) + 8 * (r >> 2)) * STR;
            t.dv = mfma32(ocol[ro], s[r], t.dv);
            t.dk = mfma32(qcol[ro], dp[r], t.dk);
        }
    }
}
__device__ __forceinline__ void dkv_tile_end(const DkvTile& t, float* dst) {   // dst: the dq block of this lane's row + 4 * half
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 wk = {t.dk[4 * g] * SCALE, t.dk[4 * g + 1] * SCALE, t.dk[4 * g + 2] * SCALE, t.dk[4 * g + 3] * SCALE};
        const f32x4 wv = {t.dv[4 * g], t.dv[4 * g + 1], t.dv[4 * g + 2], t.dv[4 * g + 3]};
        *reinterpret_cast<f32x4*>(dst + D + 8 * g) = wk;
        *reinterpret_cast<f32x4*>(dst + 2 * D + 8 * g) = wv;
    }
}
}  // namespace

// ------------------------------------------------------------------ forward with lse
// NT = NTOK: grid (BH), n_tok unused.  NT = 0: grid (BH, ceil(n_tok / 256)), n_tok a multiple of 32.
template <int NT>
__global__ __launch_bounds__(512) void attn_train_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, float* __restrict__ o_rows,
                                                             float* __restrict__ lse, int n_tok) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ntok = NT ? NT : n_tok;
    float* Ks = smem;
    float* Vs = smem + (NT ? NT : CHR) * STR;
    const int bh = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, i = lane & 31;
    const int seq = bh / NH, head = bh % NH;
    const float* kg = k + (size_t)bh * ntok * DH;
    const float* vg = v + (size_t)bh * ntok * DH;
    const float* qg = q + (size_t)bh * ntok * DH;
    if constexpr (NT != 0) {
        stage_rows(Ks, kg, DH, NT, tid, 512);
        stage_rows(Vs, vg, DH, NT, tid, 512);
        __syncthreads();
        for (int qt = wave; qt < NT / 32; qt += 8) {
            const int tok = qt * 32 + i;
            FwdTile t;
            fwd_tile_begin(t, qg + (size_t)tok * DH + 4 * half);
            fwd_tile_blocks(t, Ks, Vs, NT / 32, half, i);
            fwd_tile_end(t, o_rows + ((size_t)seq * NT + tok) * D + head * DH + 4 * half, lse + (size_t)bh * NT + tok, half);
        }
    } else {
        const int nkb = ntok >> 5;
        const int qt = blockIdx.y + gridDim.y * wave;      // this wave's only tile
        const bool active = qt < nkb;
        const int tok = (active ? qt : 0) * 32 + i;
        FwdTile t;
        fwd_tile_begin(t, qg + (size_t)tok * DH + 4 * half);
        for (int c0 = 0; c0 < nkb; c0 += CHB) {
            const int nb = min(CHB, nkb - c0);
            if (c0 != 0) __syncthreads();                  // every wave is done with the chunk before
            stage_rows(Ks, kg + (size_t)c0 * 32 * DH, DH, nb * 32, tid, 512);
            stage_rows(Vs, vg + (size_t)c0 * 32 * DH, DH, nb * 32, tid, 512);
            __syncthreads();
            if (active) fwd_tile_blocks(t, Ks, Vs, nb, half, i);
        }
        if (active)
            fwd_tile_end(t, o_rows + ((size_t)seq * ntok + tok) * D + head * DH + 4 * half, lse + (size_t)bh * ntok + tok, half);
    }
}

// ------------------------------------------------------------------ D_i = sum_d dO[i][d] * O[i][d]
template <int NT>
__global__ __launch_bounds__(256) void attn_dsum_kernel(const float* __restrict__ o_rows, const float* __restrict__ do_rows,
                                                        float* __restrict__ dsum, int M, int n_tok) {
    // one thread per (token row, head): 32 contiguous floats
    const int ntok = NT ? NT : n_tok;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * NH) return;
    const int row = idx >> 2, head = idx & 3;
    const f32x4* a = reinterpret_cast<const f32x4*>(o_rows + (size_t)row * D + head * DH);
    const f32x4* b = reinterpret_cast<const f32x4*>(do_rows + (size_t)row * D + head * DH);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const f32x4 x = a[c], y = b[c];
        s += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
    }
    const int seq = row / ntok, tok = row - seq * ntok;
    dsum[((size_t)seq * NH + head) * ntok + tok] = s;
}

// ------------------------------------------------------------------ kernel A: dQ (queries on lanes)
template <int NT>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, const float* __restrict__ do_rows,
                                                          const float* __restrict__ lse, const float* __restrict__ dsum,
                                                          float* __restrict__ dqkv, int n_tok) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ntok = NT ? NT : n_tok;
    float* Ks = smem;
    float* Vs = smem + (NT ? NT : CHR) * STR;
    const int bh = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, i = lane & 31;
    const int seq = bh / NH, head = bh % NH;
    const float* kg = k + (size_t)bh * ntok * DH;
    const float* vg = v + (size_t)bh * ntok * DH;
    const float* qg = q + (size_t)bh * ntok * DH;
    if constexpr (NT != 0) {
        stage_rows(Ks, kg, DH, NT, tid, 512);
        stage_rows(Vs, vg, DH, NT, tid, 512);
        __syncthreads();
        for (int qt = wave; qt < NT / 32; qt += 8) {
            const int tok = qt * 32 + i;
            DqTile t;
            dq_tile_begin(t, qg + (size_t)tok * DH + 4 * half, do_rows + ((size_t)seq * NT + tok) * D + head * DH + 4 * half,
                          lse[(size_t)bh * NT + tok], dsum[(size_t)bh * NT + tok]);
            dq_tile_blocks(t, Ks, Vs, NT / 32, half, i);
            dq_tile_end(t, dqkv + ((size_t)seq * NT + tok) * (3 * D) + head * DH + 4 * half);
        }
    } else {
        const int nkb = ntok >> 5;
        const int qt = blockIdx.y + gridDim.y * wave;
        const bool active = qt < nkb;
        const int tok = (active ? qt : 0) * 32 + i;
        DqTile t;
        dq_tile_begin(t, qg + (size_t)tok * DH + 4 * half, do_rows + ((size_t)seq * ntok + tok) * D + head * DH + 4 * half,
                      lse[(size_t)bh * ntok + tok], dsum[(size_t)bh * ntok + tok]);
        for (int c0 = 0; c0 < nkb; c0 += CHB) {
            const int nb = min(CHB, nkb - c0);
            if (c0 != 0) __syncthreads();
            stage_rows(Ks, kg + (size_t)c0 * 32 * DH, DH, nb * 32, tid, 512);
            stage_rows(Vs, vg + (size_t)c0 * 32 * DH, DH, nb * 32, tid, 512);
            __syncthreads();
            if (active) dq_tile_blocks(t, Ks, Vs, nb, half, i);
        }
        if (active) dq_tile_end(t, dqkv + ((size_t)seq * ntok + tok) * (3 * D) + head * DH + 4 * half);
    }
}

// ------------------------------------------------------------------ kernel B: dK, dV (keys on lanes)
template <int NT>
__global__ __launch_bounds__(512) void attn_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ do_rows,
                                                           const float* __restrict__ lse, const float* __restrict__ dsum,
                                                           float* __restrict__ dqkv, int n_tok) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ntok = NT ? NT : n_tok;
    constexpr int ROWS = NT ? NT : CHR;
    float* Qs = smem;                       // (ROWS, STR) unscaled Q
    float* Os = smem + ROWS * STR;          // (ROWS, STR) dO of this head
    float* Ls = smem + 2 * ROWS * STR;      // lse (log2 domain)
    float* Ds = Ls + ROWS;                  // D_i
    const int bh = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int seq = bh / NH, head = bh % NH;
    const float* qg = q + (size_t)bh * ntok * DH;
    const float* og = do_rows + (size_t)seq * ntok * D + head * DH;
    const float* kg = k + (size_t)bh * ntok * DH;
    const float* vg = v + (size_t)bh * ntok * DH;
    if constexpr (NT != 0) {
        stage_rows(Qs, qg, DH, NT, tid, 512);
        stage_rows(Os, og, D, NT, tid, 512);
        for (int t = tid; t < NT; t += 512) {
            Ls[t] = lse[(size_t)bh * NT + t];
            Ds[t] = dsum[(size_t)bh * NT + t];
        }
        __syncthreads();
        for (int kb = wave; kb < NT / 32; kb += 8) {
            const int key = kb * 32 + j;
            DkvTile t;
            dkv_tile_begin(t, kg + (size_t)key * DH + 4 * half, vg + (size_t)key * DH + 4 * half);
            dkv_tile_blocks(t, Qs, Os, Ls, Ds, NT / 32, half, j);
            dkv_tile_end(t, dqkv + ((size_t)seq * NT + key) * (3 * D) + head * DH + 4 * half);
        }
    } else {
        const int nkb = ntok >> 5;
        const int kb = blockIdx.y + gridDim.y * wave;
        const bool active = kb < nkb;
        const int key = (active ? kb : 0) * 32 + j;
        DkvTile t;
        dkv_tile_begin(t, kg + (size_t)key * DH + 4 * half, vg + (size_t)key * DH + 4 * half);
        for (int c0 = 0; c0 < nkb; c0 += CHB) {
            const int nb = min(CHB, nkb - c0);
            if (c0 != 0) __syncthreads();
            stage_rows(Qs, qg + (size_t)c0 * 32 * DH, DH, nb * 32, tid, 512);
            stage_rows(Os, og + (size_t)c0 * 32 * D, D, nb * 32, tid, 512);
            for (int r = tid; r < nb * 32; r += 512) {
                Ls[r] = lse[(size_t)bh * ntok + c0 * 32 + r];
                Ds[r] = dsum[(size_t)bh * ntok + c0 * 32 + r];
            }
            __syncthreads();
            if (active) dkv_tile_blocks(t, Qs, Os, Ls, Ds, nb, half, j);
        }
        if (active) dkv_tile_end(t, dqkv + ((size_t)seq * ntok + key) * (3 * D) + head * DH + 4 * half);
    }
}

static int attn_train_init() {
    static bool done = false;
    if (!done) {
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_train_fwd_kernel<NTOK>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS2));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_dq_kernel<NTOK>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS2));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_dkv_kernel<NTOK>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS2));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_train_fwd_kernel<0>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDSW));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_dq_kernel<0>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDSW));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_dkv_kernel<0>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, LDSW));
        done = true;
    }
    return T2S_OK;
}

// the run-time form: a wave owns one tile, so a head takes ceil(tiles / 8) workgroups
static int wide_split(int n_tok, int* split) {
    if (n_tok <= 0 || n_tok % 32 != 0) {
        set_error("training attention: n_tok=%d is not a positive multiple of 32", n_tok);
        return T2S_E_INVALID;
    }
    *split = (n_tok / 32 + 7) / 8;
    return T2S_OK;
}

int attn_plain_train_fwd(const float* q, const float* k, const float* v, float* o_rows, float* lse, int BH, int n_tok,
                         hipStream_t st) {
    if (int rc = attn_train_init()) return rc;
    if (n_tok == NTOK) {
        attn_train_fwd_kernel<NTOK><<<BH, 512, LDS2, st>>>(q, k, v, o_rows, lse, NTOK);
    } else {
        int split;
        if (int rc = wide_split(n_tok, &split)) return rc;
        attn_train_fwd_kernel<0><<<dim3(BH, split), 512, LDSW, st>>>(q, k, v, o_rows, lse, n_tok);
    }
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int attn_bwd(const float* q, const float* k, const float* v, const float* o_rows, const float* do_rows,
             const float* lse, float* dsum, float* dqkv_rows, int BH, int n_tok, hipStream_t st) {
    if (int rc = attn_train_init()) return rc;
    const int M = (BH / NH) * n_tok;
    if (n_tok == NTOK) {
        attn_dsum_kernel<NTOK><<<(M * NH + 255) / 256, 256, 0, st>>>(o_rows, do_rows, dsum, M, NTOK);
        T2S_LAUNCH_CHECK();
        attn_bwd_dq_kernel<NTOK><<<BH, 512, LDS2, st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, NTOK);
        T2S_LAUNCH_CHECK();
        attn_bwd_dkv_kernel<NTOK><<<BH, 512, LDS2, st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, NTOK);
        T2S_LAUNCH_CHECK();
    } else {
        int split;
        if (int rc = wide_split(n_tok, &split)) return rc;
        attn_dsum_kernel<0><<<(M * NH + 255) / 256, 256, 0, st>>>(o_rows, do_rows, dsum, M, n_tok);
        T2S_LAUNCH_CHECK();
        attn_bwd_dq_kernel<0><<<dim3(BH, split), 512, LDSW, st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, n_tok);
        T2S_LAUNCH_CHECK();
        attn_bwd_dkv_kernel<0><<<dim3(BH, split), 512, LDSW, st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, n_tok);
        T2S_LAUNCH_CHECK();
    }
    return T2S_OK;
}

}  // namespace t2s
