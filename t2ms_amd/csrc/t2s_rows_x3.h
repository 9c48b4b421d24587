// The row-local chain of a DiT block (t2s_rows.h) in "bf16x3" arithmetic (t2s_x3.h): the same
// register-resident chain, chunk order and LDS-DMA weight ring, with every fp32 product evaluated
// as six bf16 MFMAs (fp32-accurate) -- 48 v_mfma_f32_32x32x16_bf16 per chunk instead of 64
// v_mfma_f32_32x32x2_f32 at half the cycles each.  T2S_MATH_BF16X3: what infer.py / Sampler select by default since round 5
// (the bench headline stays on the f32 kernels).
//
// Operand flow.  The 32x32 fp32 accumulator layout (lane = token, registers = features) is still the
// next product's B operand: registers 8s..8s+7 of feature tile nt are k-step 2nt+s, split into three
// bf16 planes in registers (split3_acc).  Where the register budget allows the planes stay resident
// for the whole GEMM (attention output for proj, LayerNorm outputs for fc1 and qkv: 96 registers; the
// fp32 copy is dead by then, and the residual stream is parked in HBM during the MLP loop).
//
// Weights: three bf16 planes in chunk order, 24 KiB per chunk = 24 LDS-DMA pieces of 1 KiB:
//   K = 128 chunks (proj / fc1 / qkv tile of 32 outputs): piece (ks, p), ks = k-step 0..7, p = plane,
//     lane (n & 31, h) holds W[n][32 (ks>>1) + 16 (ks&1) + 8 (j>>2) + 4 h + (j&3)], j = 0..7;
//   fc2 chunk c (the 32 hidden units of fc1 chunk c):  piece (nt, s, p), lane holds
//     W2[32 nt + (n & 31)][32 c + 16 s + 8 (j>>2) + 4 h + (j&3)].
//
// One-plane form ("bf16" arithmetic, T2S_MATH_BF16; dit_rows_bf16p_kernel below): the same body instantiated on Split1
// (t2s_x3.h).  Weight pieces carry the h plane only -- 8 KiB per chunk = 8 pieces, two per wave -- activation fragments
// are rounded once, and k / V^T leave as one bf16 plane per tile (2 KiB); 8 MFMAs per chunk instead of 48.
#pragma once
#include <type_traits>

#include "t2s_rows.h"
#include "t2s_x3.h"

namespace t2s {

// Raise the wave's issue priority for its VALU-heavy sections (LayerNorm, GELU, operand splits): the two
// waves of a SIMD are arbitrated by priority, then age, and a partner in an MFMA section needs the issue
// port for only 8 of every 32 cycles (measured: 375 -> 364 us average per launch).
#define X3_PRIO(p) __builtin_amdgcn_s_setprio(p);

// (explicit vmcnt(0): every weight DMA of this kernel is issued by untracked inline asm, the fence inside wg_sync() only covers
// what hipcc tracks -- as ROWS_SYNC in t2s_rows.h)
#define X3_SYNC() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); wg_sync(); }
// the same, but the 16 YOUNGEST vector-memory operations of the wave may still be in flight (the tile's residual stream, issued
// last on purpose: it is first needed after the proj chunks).  Not wg_sync(): its release fence waits for vmcnt(0).
#define X3_SYNC_BUT16() { asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
template <int NP> constexpr int XN_CHUNK_UNITS = 8 * NP * 64;   // 16-byte units per chunk: 8 k-steps x NP planes
constexpr int X3_CHUNK_UNITS = XN_CHUNK_UNITS<3>;          // 24 KiB
template <int NP> constexpr int ROWS_XN_LDS_BYTES = 2 * XN_CHUNK_UNITS<NP> * 16 + (ROWS_CB_FLOATS + 4 * ROWS_CM_FLOATS) * 4;
constexpr int ROWS_X3_LDS_BYTES = ROWS_XN_LDS_BYTES<3>;
constexpr int ROWS_P1_LDS_BYTES = ROWS_XN_LDS_BYTES<1>;

struct RowArgsX3 {
    float* x;          // (M,128) residual stream, fragment-major, in place
    const float* x_in; // where the stream is READ at kernel entry: x itself, or (block 0 of a CFG pass) the patchified
    int in_seqs;       //   tokens of the in_seqs distinct sequences, sequence s reading slot s % in_seqs
    // <qkv only> kernel of block 0 with p_lat != NULL: the tokens are GENERATED in the prologue from the latent (patchify,
    // exactly as in t2s_rows.h: same helpers, same bits as patchify_kernel) and written to x_in for block 0's <proj + MLP> kernel
    const float* p_lat;
    int p_B;
    const float *p_cw, *p_cb, *p_pw, *p_pb, *p_pos;
    // last block only (DO_MLP && !DO_QKV): fused final layer when out0 != NULL; sequences [0,split) -> out0, rest -> out1;
    // keep_x = 0 skips the store of the final residual stream (only the t2s_dit_read_stream tap reads it)
    const float *f_lnw, *f_lnb, *f_ow, *f_ob;
    float *out0, *out1;
    int split, keep_x;
    const float* ao;   // (M,128) attention output (pre-proj), fragment-major
    const float* mod;  // (S,MODROW), or the sampler's whole-run table when mod_step != NULL (see RowArgs, t2s_rows.h)
    const int* mod_step;
    int mod_rows, mod_uncond, mod_row0;
    int M;
    int blk;
    int qkv_blk;
    const bf16x8 *Wp, *W1, *W2c, *Wq;   // split weights in chunk order (see above)
    const float *bp, *b1, *b2, *bq;
    float* q;          // q fragment-major fp32 (the attention scales and splits it once per head)
    __bf16 *k3, *v3;   // k, V^T split planes (t2s_x3.h); ONE plane each for the one-plane kernels
    int tps;           // wide kernels only: 32-token tiles per sequence, 25 or 32 (latent width 2 tps: 800 / 1024 tokens); M = S * 32 * tps
};

// fp32 packed weights (packed_index order, or the fc2 chunk order of pack_weight_kernel mode 1) ->
// split planes in the chunk order above.  One thread per (chunk, piece-without-plane, lane).
template <int NP>
static __global__ void pack_rows_xn_kernel(const float* __restrict__ P, bf16x8* __restrict__ dst, int N, int K, int fc2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_chunks = fc2 ? K / 32 : N / 32;
    if (idx >= n_chunks * 8 * 64) return;
    const int lane = idx & 63, piece = (idx >> 6) & 7, chunk = idx >> 9;
    const int i = lane & 31, h = lane >> 5;
    f32x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int n, k;
        if (!fc2) {
            n = chunk * 32 + i;
            k = 32 * (piece >> 1) + 16 * (piece & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
            v[j] = P[packed_index(n, k, K)];
        } else {
            const int nt = piece >> 1, s = piece & 1;
            n = 32 * nt + i;
            k = 32 * chunk + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
            const int G = k >> 3, hh = (k >> 2) & 1, e = k & 3, c = G >> 2, g = G & 3;
            v[j] = P[((((size_t)(c * (N >> 5) + (n >> 5)) * 4 + g) * 64) + (hh * 32 + (n & 31))) * 4 + e];
        }
    }
    const Split3 sp = split3(v);   // (NP == 1 keeps h = rn_bf16(v) only)
    bf16x8* d = dst + ((size_t)(chunk * 8 + piece) * NP) * 64 + lane;
    d[0] = sp.h;
    if constexpr (NP == 3) {
        d[64] = sp.m;
        d[128] = sp.l;
    }
}

// np = 3: all three planes; np = 1: the h plane alone, in the same chunk order (a third of the bytes)
inline int pack_rows_xn(int np, const float* P, bf16x8* dst, int N, int K, int fc2, hipStream_t st) {
    const int n = (fc2 ? K / 32 : N / 32) * 8 * 64;
    (np == 3 ? pack_rows_xn_kernel<3> : pack_rows_xn_kernel<1>)<<<(n + 255) / 256, 256, 0, st>>>(P, dst, N, K, fc2);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// the planes of weight piece `pc` of the chunk in ring slot `wb` (wb already offset by lane)
template <class SP>
__device__ __forceinline__ SP ldwp(const bf16x8* wb, int pc) {
    constexpr int NP = planes_of<SP>::n;
    SP w;
    w.h = wb[(pc * NP + 0) * 64];
    if constexpr (NP == 3) {
        w.m = wb[(pc * 3 + 1) * 64];
        w.l = wb[(pc * 3 + 2) * 64];
    }
    return w;
}

// One chunk's eight k-steps with the NEXT k-step's three weight fragments requested before the current k-step's six MFMAs
// (sched_barrier pins that order; the waitcnt pass then emits counted lgkmcnt waits instead of `3 ds_read, lgkmcnt(0), 6 MFMA`
// per k-step): rows -1.5 %, sampler +1.1 % in a same-box A/B (profiles/r05_x3_pingpong_ab.txt).  `hook(ks)` runs between the
// k-steps (the LDS-DMA piece of the next chunk).
template <bool SWAP, class SP, typename BOP, typename HOOK>
__device__ __forceinline__ void ktile_x3(const bf16x8* wb, BOP&& bop, f32x16& acc, HOOK&& hook) {
    SP w = ldwp<SP>(wb, 0);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        SP wn = w;
        if (ks + 1 < 8) wn = ldwp<SP>(wb, ks + 1);
        __builtin_amdgcn_sched_barrier(0);
        acc = SWAP ? mfma_x3(bop(ks), w, acc) : mfma_x3(w, bop(ks), acc);
        hook(ks);
        __builtin_amdgcn_sched_barrier(0);
        w = wn;
    }
}

// SP = Split3 (bf16x3) or Split1 (one plane); wring3 = the kernel's dynamic LDS, [2][CHUNK_UNITS] + constants
// TPS = 32-token tiles per sequence, as in t2s_rows.h: 15 (480 tokens, compile-time index arithmetic) or 0 = RowArgsX3::tps at
// run time (the wide kernels).  The latent width is 2 TPS.  It enters the prologue's and the stores' addresses only.
template <bool DO_MLP, bool DO_QKV, class SP, int TPS>
__device__ __forceinline__ void dit_rows_xn_body(const RowArgsX3 a, bf16x8* wring3) {
    constexpr int NP = planes_of<SP>::n;
    constexpr int CHUNK_UNITS = XN_CHUNK_UNITS<NP>;
    constexpr int WAVE_PIECES = 2 * NP;           // LDS-DMA pieces per wave and chunk: 8 NP pieces over four waves
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;
    const int n_tiles = a.M >> 5;
    int tile = blockIdx.x * 4 + wave;             // 32-token tile of this wave
    const bool active = tile < n_tiles;           // tail waves compute on a clamped tile, store nothing
    if (!active) tile = n_tiles - 1;
    const int tps = TPS ? TPS : a.tps, latw = 2 * tps;
    const int seq = (tile * 32) / (32 * tps);     // 16 W tokens = W / 2 tiles: a tile never straddles sequences (tokens over
                                                  // tokens, not tile / tps: the 480-token kernels keep their instructions)
    const float* __restrict__ modrow = a.mod + (size_t)seq * MODROW;
    if (a.mod_step != nullptr)      // (spelled out here: a helper without this kernel's target attribute would not inline)
        modrow = a.mod + ((size_t)(*a.mod_step) * a.mod_rows + (seq < a.mod_uncond ? 0 : 1 + a.mod_row0 + (seq - a.mod_uncond))) * MODROW;

    constexpr int N_CHUNKS = (DO_MLP ? 20 : 0) + (DO_QKV ? 12 : 0);
    auto chunk_src = [&](int ci) T2S_X3_KERNEL -> const bf16x8* {
        if constexpr (DO_MLP) {
            if (ci < 4) return a.Wp + (size_t)ci * CHUNK_UNITS;
            if (ci < 20) {
                const int j = ci - 4;
                return ((j & 1) ? a.W2c : a.W1) + (size_t)(j >> 1) * CHUNK_UNITS;
            }
            ci -= 20;
        }
        return a.Wq + (size_t)ci * CHUNK_UNITS;
    };
    // each wave DMAs pieces {wave, wave+4, ..., wave+20} of the chunk (one plane: {wave, wave+4})
    auto fill = [&](int ci) T2S_X3_KERNEL {
        const bf16x8* src = chunk_src(ci) + lane;
        bf16x8* dst = wring3 + (ci & 1) * CHUNK_UNITS;
#pragma unroll
        for (int p = 0; p < WAVE_PIECES; ++p)      // untracked (glds16_asm), like the pieces below: with a TRACKED LDS-DMA pending hipcc turns
            glds16_asm(reinterpret_cast<const f32x4*>(src + (wave + 4 * p) * 64),      // every wait of the prologue into vmcnt(0) --
                       reinterpret_cast<f32x4*>(dst + (wave + 4 * p) * 64));           // one full round trip per constant load
    };

    // The next chunk's six LDS-DMA pieces are issued BETWEEN the k-steps of the current chunk's MFMA group, one per k-step:
    // an LDS-DMA instruction costs ~100 issue cycles in an MFMA gap against ~150 in front of the group, where nothing covers
    // the wave's vector-memory issue (a cycle-stamped build put 14 % of a wave's cycles into the six-instruction burst; spread out
    // they cost 10 %: rows -1.0 %, sampler +0.7 % in a same-box A/B, profiles/r05_x3_dma_mix_ab.txt).  Untracked inline asm
    // (glds16_asm) so hipcc keeps its counted lgkmcnt waits for the fragment reads: every chunk therefore ends with an
    // explicit vmcnt wait in front of its barrier.
    auto fill_piece = [&](int ci, int p) T2S_X3_KERNEL {
        const bf16x8* src = chunk_src(ci) + lane + (wave + 4 * p) * 64;
        bf16x8* dst = wring3 + (ci & 1) * CHUNK_UNITS + (wave + 4 * p) * 64;
        glds16_asm(reinterpret_cast<const f32x4*>(src), reinterpret_cast<f32x4*>(dst));
    };
#define X3_FILL_MIX(ci, step) if ((step) >= 1 && (step) <= WAVE_PIECES) fill_piece(ci, (step) - 1);
#define X3_DMA_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    fill(0);
    // The attention output of the tile is requested FIRST, in front of the constants below (whose loads the compiler waits for
    // one by one before their ds_writes): its round trip then runs under theirs instead of after them.
    f32x4 araw[DO_MLP ? 16 : 1];
    if constexpr (DO_MLP) {
        const f32x4* ar = reinterpret_cast<const f32x4*>(a.ao) + (size_t)tile * 16 * 64 + lane;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            araw[g] = ar[g * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- per-feature constants in LDS (visible after the first barrier), as in t2s_rows.h ----
    float* cb = reinterpret_cast<float*>(wring3 + 2 * CHUNK_UNITS);
    float* cm = cb + ROWS_CB_FLOATS + wave * ROWS_CM_FLOATS;
    {   // every load first, then every ds_write: written as load -> store pairs each pair cost its own L2 round trip
        const int t0 = threadIdx.x, t1 = t0 + 256;
        float c0 = 0.f, c1 = 0.f, q0 = 0.f, q1 = 0.f;
        f32x4 m0 = {}, m1 = {}, m2 = {}, mq = {};
        if constexpr (DO_MLP) {
            c0 = t0 < 128 ? a.bp[t0] : a.b1[t0 - 128];                  // i = t0 < 256
            c1 = t1 < 384 ? a.b1[t1 - 128] : a.b2[t1 - 384];            // i = t1 in [256, 512)
            const float* src = modrow + a.blk * MODW;
            m0 = *reinterpret_cast<const f32x4*>(src + lane * 4);
            m1 = *reinterpret_cast<const f32x4*>(src + (64 + lane) * 4);
            m2 = *reinterpret_cast<const f32x4*>(src + (128 + lane) * 4);
        }
        if constexpr (DO_QKV) {
            q0 = a.bq[t0];
            if (t1 < 384) q1 = a.bq[t1];
            mq = *reinterpret_cast<const f32x4*>(modrow + a.qkv_blk * MODW + lane * 4);   // shift_msa | scale_msa
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (DO_MLP) {
            cb[t0] = c0;
            cb[t1] = c1;
            *reinterpret_cast<f32x4*>(cm + lane * 4) = m0;
            *reinterpret_cast<f32x4*>(cm + (64 + lane) * 4) = m1;
            *reinterpret_cast<f32x4*>(cm + (128 + lane) * 4) = m2;
        }
        if constexpr (DO_QKV) {
            cb[512 + t0] = q0;
            if (t1 < 384) cb[512 + t1] = q1;
            *reinterpret_cast<f32x4*>(cm + 768 + lane * 4) = mq;
        }
    }
    const float* c_bp = cb;
    const float* c_b1 = cb + 128;
    const float* c_b2 = cb + 384;
    const float* c_bq = cb + 512;

    // residual stream of this lane's token, accumulator layout: x[nt][4g+e] = X[row][32nt+8g+4half+e]
    f32x16 x[4];
    const int tile_src = tile - (seq - seq % a.in_seqs) * tps;   // same tile of sequence seq % in_seqs
    bool generated = false;
    if constexpr (!DO_MLP) {
        if (a.p_lat != nullptr) {
            // patchify in the prologue (as t2s_rows.h): patch_emb weight in the (unused) proj / MLP bias slots of LDS, bias in the
            // wave's (unused) MLP adaLN slots; visible after this barrier
            for (int i = threadIdx.x; i < 512; i += 256) cb[i] = a.p_pw[i];
            *reinterpret_cast<f32x4*>(cm + 256 + (lane & 31) * 4) = *reinterpret_cast<const f32x4*>(a.p_pb + (lane & 31) * 4);
            wg_sync();
            const int n = (tile - seq * tps) * 32 + (lane & 31);
            float cv[4];
            patch_conv(a, seq, n, cv, latw);
            const float* posrow = a.p_pos + (size_t)n * D;
#pragma unroll
            for (int G = 0; G < 16; ++G) {
                const int d0 = 8 * G + 4 * half;
                const f32x4 pos4 = *reinterpret_cast<const f32x4*>(posrow + d0);
                const f32x4 pb4 = *reinterpret_cast<const f32x4*>(cm + 256 + d0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    x[G >> 2][4 * (G & 3) + e] = patch_feature(cv, *reinterpret_cast<const f32x4*>(cb + (d0 + e) * 4), pb4[e], pos4[e]);
            }
            if (active && seq < a.in_seqs) {   // block 0's <proj + MLP> kernel reads the tokens of sequence s % in_seqs
                f32x4* xo = const_cast<f32x4*>(reinterpret_cast<const f32x4*>(a.x_in)) + (size_t)tile_src * 16 * 64 + lane;
#pragma unroll
                for (int G = 0; G < 16; ++G) {
                    f32x4 t;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = x[G >> 2][4 * (G & 3) + e];
                    xo[G * 64] = t;
                }
            }
            generated = true;
        }
    }
    auto load_x = [&]() T2S_X3_KERNEL {
        const f32x4* xr = reinterpret_cast<const f32x4*>(a.x_in) + (size_t)tile_src * 16 * 64 + lane;
#pragma unroll
        for (int G = 0; G < 16; ++G) {
            const f32x4 t = xr[G * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[G >> 2][4 * (G & 3) + e] = t[e];
        }
    };
    if (!DO_MLP && !generated) load_x();
    int ci = 0;

    if constexpr (DO_MLP) {
        const float* mb = cm;   // [shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp] of a.blk
        // ---------------- x += gate_msa * (proj(ao) + b): ao planes resident ----------------
        {
            SP aop[8];      // k-step ks = features 16 ks .. 16 ks + 15 in the permuted order
            // Order of the prologue's vector-memory operations: chunk 0's DMA, the attention output (top of the kernel), the
            // constants, and LAST the 16 loads of the residual stream -- it is first needed after the four proj chunks, so the
            // first barrier does not wait for it (X3_SYNC_BUT16) and the split of ao runs while it is in flight.  A timing-only
            // build without any prologue load bounded this at +5.3 % of the sampler (profiles/EXPERIMENTS.md 0.11).
            __builtin_amdgcn_sched_barrier(0);
            load_x();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const f32x4 lo = araw[2 * ks], hi = araw[2 * ks + 1];
                const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                aop[ks] = splitp<SP>(v);
            }
            X3_SYNC_BUT16()  // chunk 0 landed, ao consumed; the residual stream may still be on its way
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const bf16x8* wb = wring3 + (ci & 1) * CHUNK_UNITS + lane;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                ktile_x3<false, SP>(wb, [&](int ks) T2S_X3_KERNEL -> const SP& { return aop[ks]; }, acc,
                                [&](int ks) T2S_X3_KERNEL { X3_FILL_MIX(ci + 1, ks) });
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bias = ldc4(c_bp, nt, g, half);
                    const f32x4 gate = ldc4(mb + 2 * D, nt, g, half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[nt][4 * g + e] += gate[e] * (acc[4 * g + e] + bias[e]);
                }
                X3_DMA_LANDED()
                X3_SYNC()
                ++ci;
            }
        }
        // ---------------- x += gate_mlp * (fc2(gelu(fc1(mod(LN(x))))) + b2) ----------------
        f32x4* xw = reinterpret_cast<f32x4*>(a.x) + (size_t)tile * 16 * 64 + lane;
        {
            SP xmp[8];      // LayerNorm + modulate output as resident planes (the fp32 copy dies here)
            X3_PRIO(2)
            {
                f32x16 xm[4];
                ln_modulate(x, xm, mb + 3 * D, mb + 4 * D, half, 1e-6f);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) xmp[ks] = splitp_acc<SP>(xm[ks >> 1], ks & 1);
            }
            // park the post-attention residual in HBM for the MLP loop (t2s_rows.h)
            if (active) {
#pragma unroll
                for (int G = 0; G < 16; ++G) {
                    f32x4 t;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = x[G >> 2][4 * (G & 3) + e];
                    xw[G * 64] = t;
                }
            }
            f32x16 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
            X3_PRIO(0)
#pragma unroll 1
            for (int c = 0; c < 8; ++c) {  // 32 hidden units per chunk; ci = 4 + 2c (even) here
                f32x16 hT;
                {
                    const bf16x8* wb = wring3 + lane;  // ci even -> ring slot 0
#pragma unroll
                    for (int r = 0; r < 16; ++r) hT[r] = 0.f;
                    ktile_x3<false, SP>(wb, [&](int ks) T2S_X3_KERNEL -> const SP& { return xmp[ks]; }, hT,
                                    [&](int ks) T2S_X3_KERNEL { X3_FILL_MIX(ci + 1, ks) });
                    X3_PRIO(2)   // GELU + split: let this wave's VALU win the issue arbitration over the partner's MFMA stream
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 bias = *reinterpret_cast<const f32x4*>(c_b1 + 32 * c + 8 * g + 4 * half);
#pragma unroll
                        for (int e = 0; e < 4; ++e) hT[4 * g + e] = gelu_tanh_f(hT[4 * g + e] + bias[e]);
                    }
                }
                X3_DMA_LANDED()
                X3_SYNC()
                ++ci;
                {   // fc2 partial over the 32 hidden units of this chunk: pieces (nt, s)
                    const bf16x8* wb = wring3 + CHUNK_UNITS + lane;  // ci odd -> ring slot 1
                    const SP h0 = splitp_acc<SP>(hT, 0), h1 = splitp_acc<SP>(hT, 1);
                    X3_PRIO(0)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        acc[nt] = mfma_x3(ldwp<SP>(wb, nt * 2 + 0), h0, acc[nt]);
                        if (ci + 1 < N_CHUNKS) { X3_FILL_MIX(ci + 1, 2 * nt) }
                        acc[nt] = mfma_x3(ldwp<SP>(wb, nt * 2 + 1), h1, acc[nt]);
                        if (ci + 1 < N_CHUNKS) { X3_FILL_MIX(ci + 1, 2 * nt + 1) }
                    }
                }
                X3_DMA_LANDED()
                X3_SYNC()
                ++ci;
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bias = ldc4(c_b2, nt, g, half);
                    const f32x4 gate = ldc4(mb + 5 * D, nt, g, half);
                    const f32x4 xo = xw[(nt * 4 + g) * 64];   // the parked residual
                    f32x4 t;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        t[e] = xo[e] + gate[e] * (acc[nt][4 * g + e] + bias[e]);
                        x[nt][4 * g + e] = t[e];
                    }
                    if (active && (DO_QKV || a.out0 == nullptr || a.keep_x)) xw[(nt * 4 + g) * 64] = t;   // final residual stream of this block
                }
        }
    } else {
        X3_SYNC()  // chunk 0 landed
    }

    // ---- fused final layer of the LAST block (transformer.py:182-191): affine LayerNorm (eps 1e-5),
    // Linear 128 -> 4, unpatchify out[s][(2ww+pw)*W + 2hh+ph] = y[ph*2+pw]; the lane pair of a token holds its
    // 128 features, so everything is lane-local up to one cross-half add per output
    if constexpr (DO_MLP && !DO_QKV) {
        if (a.out0 != nullptr) {
            float s1 = 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    s1 += (x[nt][4 * g] + x[nt][4 * g + 1]) + (x[nt][4 * g + 2] + x[nt][4 * g + 3]);
            s1 += xhalf(s1);
            const float mean = s1 * (1.0f / 128.0f);
            float s2 = 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[nt][4 * g + e] -= mean;
                    s2 += (x[nt][4 * g] * x[nt][4 * g] + x[nt][4 * g + 1] * x[nt][4 * g + 1]) +
                          (x[nt][4 * g + 2] * x[nt][4 * g + 2] + x[nt][4 * g + 3] * x[nt][4 * g + 3]);
                }
            s2 += xhalf(s2);
            const float rstd = rsqrtf(s2 * (1.0f / 128.0f) + 1e-5f);
            // (one plane: a vector, not an array -- `half ? fa[2 + q2] : fa[q2]` below goes through 32 B of scratch with the array.
            // The bf16x3 instance keeps the array it was measured and pinned with, tests/test_isa_pins.py.)
            std::conditional_t<NP == 3, float[4], f32x4> fa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = 32 * nt + 8 * g + 4 * half;
                    const f32x4 gam = *reinterpret_cast<const f32x4*>(a.f_lnw + col);
                    const f32x4 bet = *reinterpret_cast<const f32x4*>(a.f_lnb + col);
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = (x[nt][4 * g + e] * rstd) * gam[e] + bet[e];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(a.f_ow + p * D + col);
                        fa[p] += (y.x * w.x + y.y * w.y) + (y.z * w.z + y.w * w.w);
                    }
                }
#pragma unroll
            for (int p = 0; p < 4; ++p) fa[p] += xhalf(fa[p]);
            if (active) {   // lane half 0 writes patch outputs p = 0,1; half 1 writes p = 2,3
                const int n = (tile - seq * tps) * 32 + (lane & 31);
                const int hh = n >> 5, ww = n & 31;
                const int lat = LATC * latw;
                float* dst = (seq < a.split) ? a.out0 + (size_t)seq * lat : a.out1 + (size_t)(seq - a.split) * lat;
#pragma unroll
                for (int q2 = 0; q2 < 2; ++q2) {
                    const int p = 2 * half + q2;
                    dst[(2 * ww + (p & 1)) * latw + 2 * hh + (p >> 1)] = (half ? fa[2 + q2] : fa[q2]) + a.f_ob[p];
                }
            }
        }
    }
    if constexpr (DO_QKV) {
        SP xmp[8];      // LayerNorm + modulate output as resident planes
        X3_PRIO(2)
        {
            f32x16 xm[4];
            ln_modulate(x, xm, cm + 768, cm + 768 + D, half, 1e-6f);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) xmp[ks] = splitp_acc<SP>(xm[ks >> 1], ks & 1);
        }
        const int tile_in_seq = tile - seq * tps;
        X3_PRIO(0)
#pragma unroll 1
        for (int t = 0; t < 12; ++t) {  // output tile t = which*4 + head
            const bf16x8* wb = wring3 + (ci & 1) * CHUNK_UNITS + lane;
            const int which = t >> 2, head = t & 3;
            const size_t head_tile = ((size_t)seq * NH + head) * tps + tile_in_seq;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (which < 2) {
                // q / k tile, transposed product: lane = token, registers = features d
                ktile_x3<false, SP>(wb, [&](int ks) T2S_X3_KERNEL -> const SP& { return xmp[ks]; }, acc,
                                [&](int ks) T2S_X3_KERNEL { if (ci + 1 < N_CHUNKS) { X3_FILL_MIX(ci + 1, ks) } });
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bias = *reinterpret_cast<const f32x4*>(c_bq + 32 * t + 8 * g + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * g + e] += bias[e];
                }
                if (active) {
                    if (which == 0) {
                        f32x4* dst = reinterpret_cast<f32x4*>(a.q) + head_tile * 4 * 64 + lane;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 o = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                            dst[g * 64] = o;
                        }
                    } else {
                        bf16x8* d3 = reinterpret_cast<bf16x8*>(a.k3) + head_tile * XN_TILE_UNITS<NP> + lane;
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) {
                            const SP sp = splitp_acc<SP>(acc, s2);
                            d3[(0 + s2) * 64] = sp.h;
                            if constexpr (NP == 3) {
                                d3[(2 + s2) * 64] = sp.m;
                                d3[(4 + s2) * 64] = sp.l;
                            }
                        }
                    }
                }
            } else {
                // v tile with the MFMA operands swapped: lane = feature d, registers = keys
                const float bias = c_bq[32 * t + (lane & 31)];
                ktile_x3<true, SP>(wb, [&](int ks) T2S_X3_KERNEL -> const SP& { return xmp[ks]; }, acc,
                               [&](int ks) T2S_X3_KERNEL { if (ci + 1 < N_CHUNKS) { X3_FILL_MIX(ci + 1, ks) } });
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += bias;
                if (active) {
                    bf16x8* d3 = reinterpret_cast<bf16x8*>(a.v3) + head_tile * XN_TILE_UNITS<NP> + lane;
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const SP sp = splitp_acc<SP>(acc, s2);
                        d3[(0 + s2) * 64] = sp.h;
                        if constexpr (NP == 3) {
                            d3[(2 + s2) * 64] = sp.m;
                            d3[(4 + s2) * 64] = sp.l;
                        }
                    }
                }
            }
            // counted wait + raw barrier: the next chunk's 6 DMA pieces (one plane: 2) must have landed; the q (4) or
            // k / v plane (6; one plane: 2) stores issued after them stay in flight.  Tail waves store nothing.
            if (!active)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (which >= 1 && NP == 3)
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else if (which >= 1)
                asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            ++ci;
        }
    }
}

template <bool DO_MLP, bool DO_QKV>
__global__ __launch_bounds__(256, 2) T2S_X3_KERNEL void dit_rows_x3_kernel(const RowArgsX3 a) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 wring3[];  // [2][X3_CHUNK_UNITS]
    dit_rows_xn_body<DO_MLP, DO_QKV, Split3, NTOK / 32>(a, wring3);
}

// T2S_MATH_BF16: the one-plane instantiation (a kernel of its own, no run-time branch in the bf16x3 one)
template <bool DO_MLP, bool DO_QKV>
__global__ __launch_bounds__(256, 2) T2S_P1_KERNEL void dit_rows_bf16p_kernel(const RowArgsX3 a) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 wring1[];  // [2][XN_CHUNK_UNITS<1>]
    dit_rows_xn_body<DO_MLP, DO_QKV, Split1, NTOK / 32>(a, wring1);
}

// the same bodies for the wide latents (800 / 1024 tokens; t2s_dit_set_wide_math): tiles per sequence from RowArgsX3::tps
template <bool DO_MLP, bool DO_QKV>
__global__ __launch_bounds__(256, 2) T2S_X3_KERNEL void dit_rows_x3_wide_kernel(const RowArgsX3 a) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 wring3w[];
    dit_rows_xn_body<DO_MLP, DO_QKV, Split3, 0>(a, wring3w);
}
template <bool DO_MLP, bool DO_QKV>
__global__ __launch_bounds__(256, 2) T2S_P1_KERNEL void dit_rows_bf16p_wide_kernel(const RowArgsX3 a) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 wring1w[];
    dit_rows_xn_body<DO_MLP, DO_QKV, Split1, 0>(a, wring1w);
}

// host side: one set of helpers for both plane counts (np = 3: bf16x3, np = 1: the one-plane kernels, named first: their
// place in the code object, profiles/EXPERIMENTS.md 0.16)
template <bool DO_MLP, bool DO_QKV>
inline auto dit_rows_xn_kernel(int np) { return np == 1 ? dit_rows_bf16p_kernel<DO_MLP, DO_QKV> : dit_rows_x3_kernel<DO_MLP, DO_QKV>; }
template <bool DO_MLP, bool DO_QKV>
inline auto dit_rows_xn_wide_kernel(int np) { return np == 1 ? dit_rows_bf16p_wide_kernel<DO_MLP, DO_QKV> : dit_rows_x3_wide_kernel<DO_MLP, DO_QKV>; }
inline int rows_xn_lds_bytes(int np) { return np == 3 ? ROWS_X3_LDS_BYTES : ROWS_P1_LDS_BYTES; }

inline int dit_rows_xn_init(int np) {   // all three instances of a mode, in both forms
    const void* const kernels[6] = {reinterpret_cast<const void*>(dit_rows_xn_kernel<false, true>(np)),
                                    reinterpret_cast<const void*>(dit_rows_xn_kernel<true, true>(np)),
                                    reinterpret_cast<const void*>(dit_rows_xn_kernel<true, false>(np)),
                                    reinterpret_cast<const void*>(dit_rows_xn_wide_kernel<false, true>(np)),
                                    reinterpret_cast<const void*>(dit_rows_xn_wide_kernel<true, true>(np)),
                                    reinterpret_cast<const void*>(dit_rows_xn_wide_kernel<true, false>(np))};
    for (const void* k : kernels)
        T2S_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, rows_xn_lds_bytes(np)));
    return T2S_OK;
}

template <bool DO_MLP, bool DO_QKV>
inline int launch_dit_rows_xn(int np, const RowArgsX3& a, hipStream_t st) {
    if (a.M <= 0 || a.M % 32 != 0) {
        set_error("dit_rows_xn (%d planes): M=%d must be a positive multiple of 32", np, a.M);
        return T2S_E_INVALID;
    }
    const int tiles = a.M / 32;
    if (a.tps != 0 && ((a.tps != 25 && a.tps != 32) || tiles % a.tps != 0)) {
        set_error("dit_rows_xn (%d planes): tps=%d must be 25 or 32 and divide the %d tiles", np, a.tps, tiles);
        return T2S_E_INVALID;
    }
    if (a.tps != 0)
        dit_rows_xn_wide_kernel<DO_MLP, DO_QKV>(np)<<<(tiles + 3) / 4, 256, rows_xn_lds_bytes(np), st>>>(a);
    else
        dit_rows_xn_kernel<DO_MLP, DO_QKV>(np)<<<(tiles + 3) / 4, 256, rows_xn_lds_bytes(np), st>>>(a);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

}  // namespace t2s
