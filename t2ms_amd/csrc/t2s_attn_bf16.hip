// Attention of the bf16 TRAINING path: forward with log-sum-exp and the flash-style backward, all
// contractions on v_mfma_f32_32x32x16_bf16 (fp32 accumulate), softmax statistics in fp32.
// Same mathematics as t2s_attn_bwd.hip (timm 1.0.11 Attention core; reference call site
// model/denoiser/transformer.py:116 under autograd, train.py:123-125).
//
// q, k, v: bf16 (BH, N, 32), N = 480 tokens (800 / 1024 for a wide handle), bh = seq*4 + head; q is PRE-SCALED by
// log2(e)/sqrt(32) (ATT_QS, applied by the qkv GEMM's epilogue), so q.k is the score in the log2 domain and the softmax
// reference / log-sum-exp / D_i are subtracted for free as the C operand of the score MFMAs (mfma16_from).  o, do: bf16
// token rows (S*N, 128), head h at columns 32h..32h+31.  dqkv: bf16 token rows (S*N, 384) = [dq | dk | dv] x heads.
// lse: fp32 (BH, N) in the log2 domain of the scaled scores.
//
// One workgroup (8 waves; 16 at 800 / 1024 tokens) per (sequence, head); two whole (tokens x 32) operands live in LDS as bf16
// "images" with 64-byte rows whose 16-byte chunks are XOR-swizzled by (row>>2)&3.  That one image
// serves both kinds of read without bank conflicts:
//   row read  (ds_read_b128)        -> MFMA operand with the image ROW on the lane     (K, Q, dO, V)
//   col read  (ds_read_b64_tr_b16)  -> MFMA operand with the image COLUMN on the lane  (K^T, V^T, Q^T, dO^T)
// The 32x32 score tile never leaves registers: the fp32 accumulator, converted pairwise to bf16,
// is the next MFMA's operand (acc_frag; its permuted k order is matched by the column reads).
#include "t2s_x3.h"   // T2S_X3_KERNEL (no packed fp32: it serialises with bf16 MFMAs), wg_sync; includes t2s_bf16.h

namespace t2s {

namespace {
// The three kernels are templates on the token count NT, as t2s_attn_bwd.hip's: NT = NTOK is the 480-token form (15 tiles,
// static LDS), NT = 0 takes n_tok from {800, 1024} at run time (25 / 32 tiles, never a partial one; dynamic LDS, raised
// by attn16_wide_check).  As bf16 images of 64-byte rows the whole operand pair still fits the 160 KiB LDS at the wide counts:
// 2 x 51,200 B / 2 x 65,536 B, + 2 n_tok fp32 statistics in the dK/dV kernel = 108,800 B / 139,264 B at most.  The algorithm
// is the same; one such workgroup owns its CU.  WAVES waves walk the tiles (8 at 480 tokens, WW below at the wide counts).
constexpr float SCALE = 0.17677669529663687f;  // 32^-0.5
constexpr float LN2 = 0.6931471805599453f;     // SCALE / ATT_QS: dK = dS^T q SCALE = dS^T (q ATT_QS) ln 2

__device__ __forceinline__ int img_off(int row, int chunk) { return row * 64 + 16 * (chunk ^ ((row >> 2) & 3)); }

__device__ __forceinline__ float pair_max_f(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pair_sum_f(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Store the 32 features of this lane pair's row (accumulator layout: the lane of half h holds features 8g + 4h + e) as
// bf16 in TWO 16-byte pieces per lane: the halves first trade pieces with v_permlane32_swap so that half 0 owns features
// 0..15 and half 1 features 16..31 -- a contiguous 64 bytes per row instead of eight scattered 8-byte pieces (which reach
// HBM as partial lines at less than half the store rate).  `row32` points at feature 0 of the row.
__device__ __forceinline__ void store_row32(__bf16* row32, const f32x16& acc, float scale, int half) {
    uint32_t d[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 w = {acc[4 * g] * scale, acc[4 * g + 1] * scale, acc[4 * g + 2] * scale, acc[4 * g + 3] * scale};
        const bf16x4 pk = pack4(w);
        d[g][0] = __builtin_bit_cast(uint2, pk).x;
        d[g][1] = __builtin_bit_cast(uint2, pk).y;
    }
    uint4 lo, hi;   // after the swaps: [features 8G..8G+3 | 8G+4..8G+7] for G = 2 half (lo) and 2 half + 1 (hi)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const auto a = __builtin_amdgcn_permlane32_swap(d[0][w], d[2][w], false, false);   // pieces g = 0 and 2
        const auto b = __builtin_amdgcn_permlane32_swap(d[1][w], d[3][w], false, false);   // pieces g = 1 and 3
        (&lo.x)[w] = a[0];
        (&lo.x)[2 + w] = a[1];
        (&hi.x)[w] = b[0];
        (&hi.x)[2 + w] = b[1];
    }
    uint4* dst = reinterpret_cast<uint4*>(row32 + 16 * half);
    dst[0] = lo;
    dst[1] = hi;
}

// The same image filled by LDS-DMA (no registers, asynchronous): piece p of 30 = rows [16p, 16p+16) = 1 KiB; lane l writes
// LDS bytes [16 l, 16 l + 16) of the piece = row 16p + (l>>2), swizzled chunk l&3, so it FETCHES chunk (l&3) ^ ((row>>2)&3).
// hipcc compiled stage_img's loop as load -> s_waitcnt vmcnt(0) -> ds_write per iteration: eight serialized HBM round trips
// per workgroup before its first MFMA (a forward kernel run with ONE key block instead of 15 still took 63 % of the time).
__device__ __forceinline__ void dma_img_piece(char* img, const __bf16* src, int src_stride, int p, int lane) {
    const int row = 16 * p + (lane >> 2);
    const int chunk = (lane & 3) ^ ((row >> 2) & 3);
    glds16(reinterpret_cast<const f32x4*>(src + (size_t)row * src_stride + chunk * 8), reinterpret_cast<f32x4*>(img + p * 1024));
}
// (With the staging by DMA the forward kernel is, per launch, ~145 us of "skeleton" -- K / V / Q in, O out: 566 MB = 113 us at
// 5 TB/s -- plus ~90 us of key-block compute that the two workgroups a CU holds overlap only partly.  Prefetching the K / V
// of the head that takes the slot next into the caches while this one computes: no gain, 0.91 vs 0.89 ms per step.)
// two images (2 x np pieces, np = n_tok / 16: 30 at 480 tokens) over the waves of a workgroup; complete after
// s_waitcnt vmcnt(0) + barrier
template <int WAVES>
__device__ __forceinline__ void dma_two_images(char* img_a, const __bf16* src_a, int stride_a, char* img_b, const __bf16* src_b,
                                               int stride_b, int wave, int lane, int np) {
    for (int p = wave; p < 2 * np; p += WAVES) {
        if (p < np) dma_img_piece(img_a, src_a, stride_a, p, lane);
        else dma_img_piece(img_b, src_b, stride_b, p - np, lane);
    }
}

// the workgroup's LDS: static at a compile-time token count, the launch's dynamic allocation otherwise
#define T2S_ATTN16_SMEM(smem, NT, EXTRA)                                                          \
    char* smem;                                                                                   \
    if constexpr ((NT) != 0) {                                                                    \
        __shared__ __attribute__((aligned(16))) char smem_static[2 * (NT) * 64 + (EXTRA)];        \
        smem = smem_static;                                                                       \
    } else {                                                                                      \
        extern __shared__ __attribute__((aligned(16))) char smem_dynamic[];                       \
        smem = smem_dynamic;                                                                      \
    }

// operand with the image row (token base + lane&31) on the lane: k = feature 16s + 8h + 0..7
__device__ __forceinline__ bf16x8 row_frag(const char* img, int base, int lane, int s) {
    return *reinterpret_cast<const bf16x8*>(img + img_off(base + (lane & 31), 2 * s + (lane >> 5)));
}

// operand with the image column (feature lane&31) on the lane: k = token base + 16s + 8(j>>2) + 4h + (j&3)
__device__ __forceinline__ bf16x8 col_frag(const char* img, int base, int lane, int s) {
    const int grp = (lane >> 4) & 3, dhalf = grp & 1, h = grp >> 1, q = (lane & 15) >> 2, p = lane & 3;
    const int row = base + 16 * s + 4 * h + q;                 // (row >> 2) & 3 is the same for the 4 rows of the block
    const int chunk = 2 * dhalf + (p >> 1);
    const char* a0 = img + img_off(row, chunk) + 8 * (p & 1);
    const char* a1 = img + img_off(row + 8, chunk) + 8 * (p & 1);
    return join_tr(lds_tr16(a0), lds_tr16(a1));
}
}  // namespace

// ------------------------------------------------------------------ forward with lse
template <int NT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) T2S_X3_KERNEL void attn16_fwd_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                         const __bf16* __restrict__ v, __bf16* __restrict__ o_rows,
                                                         float* __restrict__ lse, int reverse, int n_tok) {
    const int ntok = NT ? NT : n_tok, nkb = ntok / 32, img = ntok * 64;
    T2S_ATTN16_SMEM(smem, NT, 0)
    char* Ks = smem;
    char* Vs = smem + img;
    const int bh = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = bh / NH, head = bh % NH;
    dma_two_images<WAVES>(Ks, k + (size_t)bh * ntok * DH, DH, Vs, v + (size_t)bh * ntok * DH, DH, wave, lane, ntok / 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_sync();
    const __bf16* qg = q + (size_t)bh * ntok * DH;
    for (int qt = wave; qt < nkb; qt += WAVES) {
        const int tok = qt * 32 + i;
        bf16x8 qf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qg + (size_t)tok * DH + 16 * s + 8 * half);
        f32x16 ot;
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[r] = 0.f;
        // Sticky-reference softmax: the reference m_ref is the row max of the FIRST key block; later blocks
        // are exponentiated against it without a max or an output rescale (the kernel is VALU-bound:
        // that is a third of its vector work).  A block whose row sum shows the reference is stale by
        // more than 2^40 re-references the running state (classic online-softmax step), wave-uniformly.
        // (Round 2 measured hand-pipelined LDS reads here -- K fragments of block jb+1 fetched behind the score MFMAs of
        // block jb, V^T fragments before the exponentials, four independent row-sum chains: no gain, 0.96 vs 0.94 ms per
        // step in a same-box A/B; the other waves of the SIMD already cover those round trips.  PMC view of this kernel
        // (tools/pmc_train.sh): VALU busy 56 %, matrix pipe 24 % (half of it co-executing), 31 % of the cycles neither,
        // 2.7 of 4 wave slots occupied on average -- the per-workgroup K / V staging and the 15-tiles-over-8-waves tail.
        // A persistent variant was built to remove exactly that (one 16-wave workgroup per CU walking 18 heads, the next
        // head's K / V images arriving by LDS-DMA into a second buffer, Q fetched a head ahead, counted vmcnt so the
        // output stores stay in flight across the per-head barrier): 1.01 vs 0.93 ms per step -- SLOWER; the barrier puts the
        // 16 waves back into lockstep at every head (offsetting them with s_sleep changed nothing).  Dropped.
        // Also without effect: a one-time half-block s_sleep offset between the two waves a SIMD holds of a workgroup, and a
        // software pipeline that issues the score MFMAs of block jb+1 before the exponentials of block jb (two alternating
        // accumulators; 0.91 vs 0.91 ms), and a staged arrival of the images (four 16 KiB stages, the first query tile gated per
        // stage with counted vmcnt + s_barrier so that it starts on the first 128 keys: 0.98 vs 0.89 ms -- every extra barrier
        // re-aligns the eight waves, whose drift apart is what overlaps their exp and MFMA phases).  What is left is the exponential itself: 16 v_exp per 4 MFMAs at head_dim 32 --
        // the kernel does 4.7 T exp/s, the chip's v_exp issue rate is ~20 T/s only if nothing else used the port.)
        float m_run = 0.f, l_lane = 0.f;    // m_run: the reference, in the log2 domain of the (pre-scaled) scores
        f32x16 negm;                        // -m_run in all 16 registers: the C operand of every score MFMA
        for (int jb = 0; jb < nkb; ++jb) {
            if (jb == 0) {                  // reference = row max of the first key block (two extra MFMAs per tile)
                f32x16 raw;
#pragma unroll
                for (int r = 0; r < 16; ++r) raw[r] = 0.f;
#pragma unroll
                for (int s = 0; s < 2; ++s) raw = mfma16(row_frag(Ks, 0, lane, s), qf[s], raw);
                float mloc = raw[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, raw[r]);
                m_run = pair_max_f(mloc);
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[r] = -m_run;
            }
            f32x16 st = mfma16_from(row_frag(Ks, jb * 32, lane, 0), qf[0], negm);   // S^T[key][query] - m_run
            st = mfma16(row_frag(Ks, jb * 32, lane, 1), qf[1], st);
            f32x16 pt;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pt[r] = __builtin_amdgcn_exp2f(st[r]);
                ps += pt[r];
            }
            if (__builtin_amdgcn_ballot_w64(!(ps < 1.0995116e12f)) != 0) {      // 2^40; also catches inf / NaN
                float mloc = st[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, st[r]);
                const float up = fmaxf(0.f, pair_max_f(mloc));                  // the new reference is m_run + up
                const float alpha = __builtin_amdgcn_exp2f(-up);
                m_run += up;
                ps = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    negm[r] = -m_run;
                    pt[r] = __builtin_amdgcn_exp2f(st[r] - up);
                    ps += pt[r];
                    ot[r] *= alpha;
                }
                l_lane *= alpha;
            }
            l_lane += ps;
#pragma unroll
            for (int s = 0; s < 2; ++s) ot = mfma16(col_frag(Vs, jb * 32, lane, s), acc_frag(pt, s), ot);   // O^T += V^T P^T
        }
        const float l_tot = pair_sum_f(l_lane);
        const float inv = 1.0f / l_tot;
        store_row32(o_rows + ((size_t)seq * ntok + tok) * D + head * DH, ot, inv, half);
        if (half == 0) lse[(size_t)bh * ntok + tok] = m_run + __builtin_amdgcn_logf(l_tot);   // v_log_f32 = log2
    }
}

// ------------------------------------------------------------------ kernel A: dQ (queries on lanes)
template <int NT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) T2S_X3_KERNEL void attn16_bwd_dq_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                            const __bf16* __restrict__ v, const __bf16* __restrict__ o_rows,
                                                            const __bf16* __restrict__ do_rows,
                                                            const float* __restrict__ lse, float* __restrict__ dsum,
                                                            __bf16* __restrict__ dqkv, int reverse, int n_tok) {
    const int ntok = NT ? NT : n_tok, nkb = ntok / 32, img = ntok * 64;
    T2S_ATTN16_SMEM(smem, NT, 0)
    char* Ks = smem;
    char* Vs = smem + img;
    const int bh = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = bh / NH, head = bh % NH;
    dma_two_images<WAVES>(Ks, k + (size_t)bh * ntok * DH, DH, Vs, v + (size_t)bh * ntok * DH, DH, wave, lane, ntok / 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_sync();
    const __bf16* qg = q + (size_t)bh * ntok * DH;
    for (int qt = wave; qt < nkb; qt += WAVES) {
        const int tok = qt * 32 + i;
        const __bf16* dorow = do_rows + ((size_t)seq * ntok + tok) * D + head * DH + 8 * half;
        bf16x8 qf[2], dof[2];   // B operands: Q^T and dO^T of this lane's query
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            qf[s] = *reinterpret_cast<const bf16x8*>(qg + (size_t)tok * DH + 16 * s + 8 * half);
            dof[s] = *reinterpret_cast<const bf16x8*>(dorow + 16 * s);
        }
        const float lse_i = lse[(size_t)bh * ntok + tok];
        // D_i = sum_d dO[i][d] O[i][d]: each lane half holds 16 of the query's 32 features; published for the dK/dV
        // kernel (which runs next on the same stream) instead of a separate pass over o and do
        float d_i = 0.f;
        {
            const __bf16* orow = o_rows + ((size_t)seq * ntok + tok) * D + head * DH + 8 * half;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f32x8 ov = unpack8(*reinterpret_cast<const bf16x8*>(orow + 16 * s)), dv8 = unpack8(dof[s]);
#pragma unroll
                for (int e = 0; e < 8; ++e) d_i += ov[e] * dv8[e];
            }
            d_i = pair_sum_f(d_i);
            if (half == 0) dsum[(size_t)bh * ntok + tok] = d_i;
        }
        f32x16 dq, nl, nd;     // nl / nd: -lse_i / -D_i in all 16 registers, the C operands of the score / dP MFMAs
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dq[r] = 0.f;
            nl[r] = -lse_i;
            nd[r] = -d_i;
        }
        for (int jb = 0; jb < nkb; ++jb) {
            f32x16 st = mfma16_from(row_frag(Ks, jb * 32, lane, 0), qf[0], nl);    // S^T[key][query] - lse (log2 domain)
            f32x16 dp = mfma16_from(row_frag(Vs, jb * 32, lane, 0), dof[0], nd);   // dP^T[key][query] - D = V dO^T - D
            st = mfma16(row_frag(Ks, jb * 32, lane, 1), qf[1], st);
            dp = mfma16(row_frag(Vs, jb * 32, lane, 1), dof[1], dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r]) * dp[r];   // dS^T = P (dP - D)
#pragma unroll
            for (int s = 0; s < 2; ++s) dq = mfma16(col_frag(Ks, jb * 32, lane, s), acc_frag(st, s), dq);   // dQ^T += K^T dS^T
        }
        store_row32(dqkv + ((size_t)seq * ntok + tok) * (3 * D) + head * DH, dq, SCALE, half);   // dq block
    }
}

// ------------------------------------------------------------------ kernel B: dK, dV (keys on lanes)
template <int NT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) T2S_X3_KERNEL void attn16_bwd_dkv_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                             const __bf16* __restrict__ v, const __bf16* __restrict__ do_rows,
                                                             const float* __restrict__ lse, const float* __restrict__ dsum,
                                                             __bf16* __restrict__ dqkv, int reverse, int n_tok) {
    const int ntok = NT ? NT : n_tok, nkb = ntok / 32, img = ntok * 64;
    T2S_ATTN16_SMEM(smem, NT, 2 * NT * 4)
    char* Qs = smem;                                              // Q image
    char* Os = smem + img;                                        // dO image (this head)
    float* Ls = reinterpret_cast<float*>(smem + 2 * img);         // lse (log2 domain)
    float* Ds = Ls + ntok;                                        // D_i
    const int bh = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, half = lane >> 5, j = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = bh / NH, head = bh % NH;
    dma_two_images<WAVES>(Qs, q + (size_t)bh * ntok * DH, DH, Os, do_rows + (size_t)seq * ntok * D + head * DH, D, wave, lane, ntok / 16);
    for (int t = tid; t < ntok; t += WAVES * 64) {
        Ls[t] = -lse[(size_t)bh * ntok + t];      // negated: they initialise the accumulators (C operands) below
        Ds[t] = -dsum[(size_t)bh * ntok + t];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_sync();
    const __bf16* kg = k + (size_t)bh * ntok * DH;
    const __bf16* vg = v + (size_t)bh * ntok * DH;
    for (int kb = wave; kb < nkb; kb += WAVES) {
        const int key = kb * 32 + j;
        bf16x8 kf[2], vf[2];   // B operands: K^T and V^T of this lane's key
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            kf[s] = *reinterpret_cast<const bf16x8*>(kg + (size_t)key * DH + 16 * s + 8 * half);
            vf[s] = *reinterpret_cast<const bf16x8*>(vg + (size_t)key * DH + 16 * s + 8 * half);
        }
        f32x16 dk, dv;
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
        for (int qb = 0; qb < nkb; ++qb) {
            // accumulators start at the per-register query statistics (queries 8g + 4 half + 0..3 of this block):
            // sc = S - lse, dp = dP - D come straight out of the MFMAs
            f32x16 sc, dp;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qb * 32 + 8 * g + 4 * half);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + qb * 32 + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sc[4 * g + e] = l4[e];
                    dp[4 * g + e] = d4[e];
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                sc = mfma16(row_frag(Qs, qb * 32, lane, s), kf[s], sc);    // S[query][key] - lse (registers = queries)
                dp = mfma16(row_frag(Os, qb * 32, lane, s), vf[s], dp);    // dP[query][key] - D = dO V^T - D
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(sc[r]);
                dp[r] = p * dp[r];             // dS[query][key]
                sc[r] = p;                     // P[query][key]
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                dv = mfma16(col_frag(Os, qb * 32, lane, s), acc_frag(sc, s), dv);   // dV^T += dO^T P
                dk = mfma16(col_frag(Qs, qb * 32, lane, s), acc_frag(dp, s), dk);   // dK^T += Q^T dS
            }
        }
        __bf16* dst = dqkv + ((size_t)seq * ntok + key) * (3 * D) + head * DH;
        store_row32(dst + D, dk, LN2, half);        // Qs holds q ATT_QS: dK = dS^T (q ATT_QS) ln 2
        store_row32(dst + 2 * D, dv, 1.0f, half);
    }
}

// the 480-token launches; the run-time form's launchers (attn16_*_wide) follow them, so that in the code object the wide
// kernels follow the 480-token ones
static int attn16_train_fwd_wide(const __bf16* q, const __bf16* k, const __bf16* v, __bf16* o_rows, float* lse, int BH, int n_tok, hipStream_t st);
static int attn16_bwd_wide(const __bf16* q, const __bf16* k, const __bf16* v, const __bf16* o_rows, const __bf16* do_rows,
                           const float* lse, float* dsum, __bf16* dqkv_rows, int BH, int n_tok, hipStream_t st);

int attn16_train_fwd(const __bf16* q, const __bf16* k, const __bf16* v, __bf16* o_rows, float* lse, int BH, int n_tok, hipStream_t st) {
    if (n_tok != NTOK) return attn16_train_fwd_wide(q, k, v, o_rows, lse, BH, n_tok, st);
    attn16_fwd_kernel<NTOK, 8><<<BH, 512, 0, st>>>(q, k, v, o_rows, lse, next_tile_dir(), NTOK);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int attn16_bwd(const __bf16* q, const __bf16* k, const __bf16* v, const __bf16* o_rows, const __bf16* do_rows,
               const float* lse, float* dsum, __bf16* dqkv_rows, int BH, int n_tok, hipStream_t st) {
    if (n_tok != NTOK) return attn16_bwd_wide(q, k, v, o_rows, do_rows, lse, dsum, dqkv_rows, BH, n_tok, st);
    attn16_bwd_dq_kernel<NTOK, 8><<<BH, 512, 0, st>>>(q, k, v, o_rows, do_rows, lse, dsum, dqkv_rows, next_tile_dir(), NTOK);   // also writes D_i -> dsum
    T2S_LAUNCH_CHECK();
    attn16_bwd_dkv_kernel<NTOK, 8><<<BH, 512, 0, st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, next_tile_dir(), NTOK);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// Waves per workgroup of the run-time (800 / 1024-token) form.  One such workgroup has its CU to itself (two image pairs do
// not fit the LDS), so 8 waves would be half the 480-token form's wave occupancy: 16 waves share the one image pair (32
// tiles = 2 per wave at 1024 tokens, 25 tiles over 16 waves at 800) within the 128 registers a lane that leaves them (96 /
// 124 / 121 VGPRs, no scratch).  Measured against the 8-wave form, one whole step at B = 128: 4.13 vs 4.37 ms at W 64, 3.40 vs
// 3.52 ms at W 50 (profiles/EXPERIMENTS.md).
constexpr int WW = 16;
constexpr int attn16_lds(int n_tok, bool dkv) { return 2 * n_tok * 64 + (dkv ? 2 * n_tok * 4 : 0); }
static_assert(attn16_lds(1024, true) <= 160 * 1024, "two bf16 images and the statistics of 1024 tokens fit the LDS");

// whole 32-token tiles and whole 16-row DMA pieces (800 = 25 x 32, 1024 = 32 x 32), and an LDS request the runtime has granted
static int attn16_wide_check(int n_tok) {
    if (n_tok != 800 && n_tok != 1024) {
        set_error("bf16 training attention: n_tok=%d (480, 800 and 1024 tokens are built)", n_tok);
        return T2S_E_INVALID;
    }
    static bool done = false;
    if (!done) {
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn16_fwd_kernel<0, WW>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, attn16_lds(1024, false)));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn16_bwd_dq_kernel<0, WW>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, attn16_lds(1024, false)));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn16_bwd_dkv_kernel<0, WW>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, attn16_lds(1024, true)));
        done = true;
    }
    return T2S_OK;
}

static int attn16_train_fwd_wide(const __bf16* q, const __bf16* k, const __bf16* v, __bf16* o_rows, float* lse, int BH, int n_tok, hipStream_t st) {
    if (int rc = attn16_wide_check(n_tok)) return rc;
    attn16_fwd_kernel<0, WW><<<BH, WW * 64, attn16_lds(n_tok, false), st>>>(q, k, v, o_rows, lse, next_tile_dir(), n_tok);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

static int attn16_bwd_wide(const __bf16* q, const __bf16* k, const __bf16* v, const __bf16* o_rows, const __bf16* do_rows,
                           const float* lse, float* dsum, __bf16* dqkv_rows, int BH, int n_tok, hipStream_t st) {
    if (int rc = attn16_wide_check(n_tok)) return rc;
    attn16_bwd_dq_kernel<0, WW><<<BH, WW * 64, attn16_lds(n_tok, false), st>>>(q, k, v, o_rows, do_rows, lse, dsum, dqkv_rows, next_tile_dir(), n_tok);
    T2S_LAUNCH_CHECK();
    attn16_bwd_dkv_kernel<0, WW><<<BH, WW * 64, attn16_lds(n_tok, true), st>>>(q, k, v, do_rows, lse, dsum, dqkv_rows, next_tile_dir(), n_tok);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

int attn_plain_train_fwd(const float* q, const float* k, const float* v, float* o_rows, float* lse, int BH, int n_tok,
                         hipStream_t st);                                                       // t2s_attn_bwd.hip
int attn_bwd(const float* q, const float* k, const float* v, const float* o_rows, const float* do_rows,
             const float* lse, float* dsum, float* dqkv_rows, int BH, int n_tok, hipStream_t st);

}  // namespace t2s

// ------------------------------------------------------------------ C ABI: stand-alone training attention (tests, benchmarking)
namespace {
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, size_t n4, float scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) reinterpret_cast<t2s::bf16x4*>(dst)[i] = t2s::pack4(reinterpret_cast<const t2s::f32x4*>(src)[i] * scale);
}
__global__ void bf16_to_f32_kernel(const __bf16* __restrict__ src, float* __restrict__ dst, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) reinterpret_cast<t2s::f32x4*>(dst)[i] = t2s::unpack4(reinterpret_cast<const t2s::bf16x4*>(src)[i]);
}
}  // namespace

namespace t2s {
// fp32 <-> bf16 copies of the stand-alone doors (n % 4 == 0); also used by t2s_wgrad (t2s_train.hip)
int f32_to_bf16(const float* src, __bf16* dst, size_t n, float scale, hipStream_t st) {
    f32_to_bf16_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, st>>>(src, dst, n / 4, scale);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
int bf16_to_f32(const __bf16* src, float* dst, size_t n, hipStream_t st) {
    bf16_to_f32_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, st>>>(src, dst, n / 4);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}
}  // namespace t2s

extern "C" int t2s_attn_fwd_bf16(const float* q, const float* k, const float* v, float* o_rows, float* lse, int n_seq,
                                 void* stream) {
    using namespace t2s;
    T2S_REQUIRE(q && k && v && o_rows && lse && n_seq > 0, "t2s_attn_fwd_bf16: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)n_seq * NH * NTOK * DH;      // elements of each of q, k, v, o
    __bf16* buf = nullptr;
    T2S_HIP_CHECK(hipMalloc(&buf, 4 * n * sizeof(__bf16)));
    const unsigned blocks = (unsigned)((n / 4 + 255) / 256);
    f32_to_bf16_kernel<<<blocks, 256, 0, st>>>(q, buf, n / 4, ATT_QS);   // the kernels take q pre-scaled (as the qkv GEMM stores it)
    f32_to_bf16_kernel<<<blocks, 256, 0, st>>>(k, buf + n, n / 4, 1.0f);
    f32_to_bf16_kernel<<<blocks, 256, 0, st>>>(v, buf + 2 * n, n / 4, 1.0f);
    int rc = attn16_train_fwd(buf, buf + n, buf + 2 * n, buf + 3 * n, lse, n_seq * NH, NTOK, st);
    if (rc == T2S_OK) {
        bf16_to_f32_kernel<<<blocks, 256, 0, st>>>(buf + 3 * n, o_rows, n / 4);
        if (hipGetLastError() != hipSuccess) rc = T2S_E_HIP;
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(buf);
    return rc;
}

// t2s_attn_train / t2s_attn_train_n: the launchers of the training step on caller tensors, n_tok tokens per sequence
static int attn_train_any(const char* who, const float* q, const float* k, const float* v, const float* do_rows, float* o_rows,
                          float* lse, float* dqkv_rows, int n_seq, int n_tok, int dtype, void* stream, bool wide_bf16 = false) {
    using namespace t2s;
    T2S_REQUIRE(q && k && v && do_rows && o_rows && lse && dqkv_rows && n_seq > 0, "%s: bad argument", who);
    T2S_REQUIRE(dtype == T2S_TRAIN_F32 || dtype == T2S_TRAIN_BF16, "%s: unknown dtype %d", who, dtype);
    T2S_REQUIRE(n_tok == NTOK || n_tok == 800 || n_tok == 1024, "%s: n_tok=%d (480, 800 and 1024 tokens are built)", who, n_tok);
    T2S_REQUIRE(dtype == T2S_TRAIN_F32 || n_tok == NTOK || wide_bf16, "%s: T2S_TRAIN_BF16 runs at 480 tokens only, not %d", who, n_tok);
    hipStream_t st = (hipStream_t)stream;
    const int BH = n_seq * NH;
    const size_t n = (size_t)BH * n_tok * DH;              // elements of each of q, k, v, o, do; dqkv has 3 n
    float* dsum = nullptr;                                 // D_i (BH, n_tok)
    __bf16* buf = nullptr;                                 // bf16: q | k | v | o | do | dqkv
    T2S_HIP_CHECK(hipMalloc(&dsum, (size_t)BH * n_tok * sizeof(float)));
    reset_tile_dir();                                      // as at the top of a training forward
    int rc = T2S_OK;
    if (dtype == T2S_TRAIN_F32) {
        rc = attn_plain_train_fwd(q, k, v, o_rows, lse, BH, n_tok, st);
        if (rc == T2S_OK) rc = attn_bwd(q, k, v, o_rows, do_rows, lse, dsum, dqkv_rows, BH, n_tok, st);
    } else if (hipMalloc(&buf, 8 * n * sizeof(__bf16)) != hipSuccess) {
        set_error("%s: out of memory for %zu bf16 values", who, 8 * n);
        rc = T2S_E_HIP;
    } else {
        __bf16 *qh = buf, *kh = buf + n, *vh = buf + 2 * n, *oh = buf + 3 * n, *doh = buf + 4 * n, *dh = buf + 5 * n;
        rc = f32_to_bf16(q, qh, n, ATT_QS, st);            // the kernels take q pre-scaled (as the qkv GEMM stores it)
        if (rc == T2S_OK) rc = f32_to_bf16(k, kh, n, 1.0f, st);
        if (rc == T2S_OK) rc = f32_to_bf16(v, vh, n, 1.0f, st);
        if (rc == T2S_OK) rc = f32_to_bf16(do_rows, doh, n, 1.0f, st);
        if (rc == T2S_OK) rc = attn16_train_fwd(qh, kh, vh, oh, lse, BH, n_tok, st);
        if (rc == T2S_OK) rc = attn16_bwd(qh, kh, vh, oh, doh, lse, dsum, dh, BH, n_tok, st);
        if (rc == T2S_OK) rc = bf16_to_f32(oh, o_rows, n, st);
        if (rc == T2S_OK) rc = bf16_to_f32(dh, dqkv_rows, 3 * n, st);
    }
    (void)hipStreamSynchronize(st);
    if (buf) (void)hipFree(buf);
    (void)hipFree(dsum);
    return rc;
}

extern "C" int t2s_attn_train(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows, float* lse,
                              float* dqkv_rows, int n_seq, int dtype, void* stream) {
    return attn_train_any("t2s_attn_train", q, k, v, do_rows, o_rows, lse, dqkv_rows, n_seq, t2s::NTOK, dtype, stream);
}

extern "C" int t2s_attn_train_n(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows, float* lse,
                                float* dqkv_rows, int n_seq, int n_tok, int dtype, void* stream) {
    return attn_train_any("t2s_attn_train_n", q, k, v, do_rows, o_rows, lse, dqkv_rows, n_seq, n_tok, dtype, stream);
}

// include/t2s_wide_train_bf16.h
extern "C" int t2s_attn_train_bf16_n(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows, float* lse,
                                     float* dqkv_rows, int n_seq, int n_tok, void* stream) {
    return attn_train_any("t2s_attn_train_bf16_n", q, k, v, do_rows, o_rows, lse, dqkv_rows, n_seq, n_tok, T2S_TRAIN_BF16, stream, true);
}
