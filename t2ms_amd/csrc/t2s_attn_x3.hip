// Fused attention of the DiT forward in "bf16x3" arithmetic (t2s_x3.h): fp32-accurate QK^T and PV
// on v_mfma_f32_32x32x16_bf16.  Same algorithm and skeleton as attn_fwd_persistent_kernel
// (t2s_attn.hip; timm 1.0.11 Attention core, reference call site model/denoiser/transformer.py:116):
// transposed tiles (a query's scores live in one lane pair), sticky-reference softmax with the
// reference folded into the MFMA C operand, ONE persistent 8-wave workgroup per CU walking the heads
// with the K / V^T operands streamed through a 4-slot LDS ring by LDS-DMA three blocks ahead.
//
// Operands: q fp32 fragment-major (as the fp32 kernel; scaled and split in registers once per head);
// k, v^T pre-split bf16 planes written by the row-chain kernel (t2s_x3.h: X3_TILE_UNITS); the
// exponentiated tile P^T is split in registers.  Per 32-key block and query tile: 12 + 12 MFMAs of
// 32 cycles (768) instead of 16 + 16 of 64 (2048).
//
// The same body instantiated on one bf16 plane (Split1, t2s_x3.h) is the attention of the single-pass "bf16" arithmetic
// (T2S_MATH_BF16, attn_fwd_bf16p_kernel): q, k, v^T and P^T each rounded once, 2 + 2 MFMAs per key block and query tile (128
// cycles), a ring slot of 4 KiB.  Not fp32-accurate; the softmax reference, exponent and running sum stay fp32.
//
// Both plane counts also exist at 800 / 1024 tokens (attn_fwd_x3_wide_kernel / attn_fwd_bf16p_wide_kernel, the attention of a
// wide handle after t2s_dit_set_wide_math): a body of its own further down, because a head then has 25 / 32 query tiles for the
// workgroup's 16 slots and no light wave to issue the LDS-DMA.
#include "t2s_dit_internal.h"
#include "t2s_x3.h"

namespace t2s {

namespace {
constexpr int NKB = NTOK / 32;                                   // 15 key blocks / query tiles
constexpr float QSCALE = 0.17677669529663687f * 1.4426950408889634f;   // 32^-0.5 * log2(e)
constexpr float SM_BIG = 1.152921504606847e18f;                  // 2^60
constexpr int X3_SLOTS = 4;
constexpr int X3_SLOT_UNITS = 2 * X3_TILE_UNITS;                 // K planes + V^T planes = 12 KiB
constexpr int X3_LDS_BYTES = X3_SLOTS * X3_SLOT_UNITS * 16;      // 48 KiB
constexpr int X3_THREADS = 512;
// the one-plane form ("bf16" arithmetic, t2s_x3.h): same ring, a third of the bytes per slot
constexpr int P1_SLOT_UNITS = 2 * XN_TILE_UNITS<1>;              // K plane + V^T plane = 4 KiB
constexpr int P1_LDS_BYTES = X3_SLOTS * P1_SLOT_UNITS * 16;      // 16 KiB

__device__ __forceinline__ float pair_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pair_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}


struct TileState {
    f32x16 negm;   // -m_ref in all 16 registers (C operand of the first QK MFMA)
    float m_ref;
    float l_lane;
};

__device__ __forceinline__ float exp_sum(f32x16& st) {
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r]);
    return ((st[0] + st[1]) + (st[2] + st[3])) + ((st[4] + st[5]) + (st[6] + st[7])) +
           (((st[8] + st[9]) + (st[10] + st[11])) + ((st[12] + st[13]) + (st[14] + st[15])));
}

__device__ __forceinline__ void glds16u(const bf16x8* gsrc_lane, bf16x8* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc_lane,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// S^T tile (+ c) = K Q^T over the head dimension (two 16-deep steps), fp32-accurate
template <class SP>
__device__ __forceinline__ f32x16 scores(const SP (&kf)[2], const SP (&q)[2], f32x16 c) {
    c = mfma_x3(kf[0], q[0], c);
    return mfma_x3(kf[1], q[1], c);
}

// the same with a C operand that must survive (the sticky reference): the first MFMA writes registers of its own
// instead of hipcc's copy + tied accumulate (see mfma32_from, t2s_common.h); same order of additions as scores()
__device__ __forceinline__ f32x16 scores_from(const Split3 (&kf)[2], const Split3 (&q)[2], const f32x16& c) {
    f32x16 acc;
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(acc) : "v"(kf[0].m), "v"(q[0].m), "v"(c));
    acc = mfma16(kf[0].l, q[0].h, acc);
    acc = mfma16(kf[0].h, q[0].l, acc);
    acc = mfma16(kf[0].m, q[0].h, acc);
    acc = mfma16(kf[0].h, q[0].m, acc);
    acc = mfma16(kf[0].h, q[0].h, acc);
    return mfma_x3(kf[1], q[1], acc);
}
__device__ __forceinline__ f32x16 scores_from(const Split1 (&kf)[2], const Split1 (&q)[2], const f32x16& c) {
    f32x16 acc;
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(acc) : "v"(kf[0].h), "v"(q[0].h), "v"(c));
    return mfma16(kf[1].h, q[1].h, acc);
}

// rare path: raw scores (C = 0) -> new reference, rescale the running sum / output, P^T in st
template <class SP>
__device__ __forceinline__ float rereference(const SP (&kf)[2], const SP (&q)[2], f32x16& st, f32x16& ot,
                                             TileState& t) {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    st = scores(kf, q, z);
    float mloc = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, st[r]);
    mloc = pair_max(mloc);
    const float m_new = fmaxf(t.m_ref, mloc);
    const float alpha = __builtin_amdgcn_exp2f(t.m_ref - m_new);   // 0 on the first block
    t.m_ref = m_new;
    t.l_lane *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        ot[r] *= alpha;
        t.negm[r] = -m_new;
        st[r] -= m_new;
    }
    return exp_sum(st);
}

// scaled + split Q^T operand of one query tile from its four fp32 fragments (k-step s = fragments 2s, 2s+1).
// One-plane form: q is rounded to bf16 HERE, after the fp32 multiplication by 32^-0.5 log2(e) (the contract of t2s.h).
template <class SP>
__device__ __forceinline__ void load_q(const f32x4 (&raw)[4], SP (&q)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f32x4 a = raw[2 * s] * QSCALE, b = raw[2 * s + 1] * QSCALE;
        const f32x8 v = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        q[s] = splitp<SP>(v);
    }
}

// NT = query tiles of this wave (2; 1 for the wave that holds tile 14 alone).
// STAG: the two waves of a SIMD (waves w and w+4) run the same loop with the per-block barrier at
// DIFFERENT points -- after the softmax (STAG = 0) or right after QK^T (STAG = 1) -- so that they
// meet half a period apart: one is in its MFMA phases (PV, QK^T) while the other exponentiates and
// splits P on the VALU.  bf16 MFMAs occupy the vector issue port for 8 of their 32 cycles, so the
// two phases of different waves overlap; with the barrier at the same point both waves would run
// their MFMA phases together and their VALU phases together, leaving the matrix pipe idle half the time.
//
// Ring protocol (4 slots, block gb in slot gb & 3).  Barrier j (the one of key block j) guarantees
//   * block j+1 has landed (every DMA-issuing wave waited until only its youngest block is in flight),
//   * every wave is done with block j-1 (both variants finish PV(j-1) before QK(j)),
// so after it a wave may read K(j+1) and refill slot (j+3) & 3 == (j-1) & 3 with block j+3.
//
// SP = Split3 (bf16x3) or Split1 (one plane): NP planes make 2 NP pieces of K and 2 NP of V^T per key block, and the counted
// waits below are in units of that piece count -- 12 for bf16x3, 4 for the one-plane form.
template <int NT, int STAG, class SP>
__device__ __forceinline__ void attn_x3_body(bf16x8* ring, const f32x4* qall, const bf16x8* kall, const bf16x8* vall,
                                             f32x4* og, int BH, int lane, int wave) {
    const int stride = gridDim.x;
    const int t0 = wave * 2;
    constexpr int NP = planes_of<SP>::n;
    constexpr int PK = 2 * NP;                       // pieces of K (and of V^T) per key block
    constexpr int SLOT_UNITS = 2 * XN_TILE_UNITS<NP>;
    static_assert(NP == 1 || SLOT_UNITS == X3_SLOT_UNITS, "bf16x3 ring geometry");
    // 2 PK pieces of 1 KiB per key block (bf16x3: 6 K planes/steps, 6 V^T)
    auto issue_piece = [&](int bh, int jb, int gslot, int p) {
        const bf16x8* src = (p < PK ? kall : vall) + ((size_t)(bh * NKB + jb) * PK + (p < PK ? p : p - PK)) * 64 + lane;
        glds16u(src, ring + (gslot & (X3_SLOTS - 1)) * SLOT_UNITS + p * 64);
    };
    // The one-tile wave (NT == 1: wave 7, whose SIMD carries 3 tiles where the others carry 4) issues all 12 pieces of a block,
    // the two-tile waves none (round 5, as t2s_attn.hip: attention 350 against 360 us per launch, sampler +0.9 %,
    // profiles/r05_x3_dma_w7_ab.txt).  `jb` may run past 14 into the following heads of this workgroup.
    auto issue_block = [&](int bh, int jb, int gslot) {
        if constexpr (NT == 1) {
            if (jb >= NKB) { jb -= NKB; bh += stride; }
            if (bh >= BH) { bh -= stride; jb = NKB - 1; }   // past the end: harmless re-fetch
#pragma unroll
            for (int p = 0; p < 2 * PK; ++p) issue_piece(bh, jb, gslot, p);
        }
    };
    // counted waits of the issuing wave: everything but the 2 PK-piece DMAs of the youngest one / two blocks has landed
    // (12 / 24 for bf16x3; one plane: 4 pieces per block, so 4 / 8.  Whatever else the wave has in flight behind them -- the
    // Q prefetch, the O stores -- only makes a wait stricter: "all but the N youngest" still covers every older piece)
    auto wait_but = [&](int blocks) {
        if constexpr (NT == 1 && NP == 3) {
            if (blocks == 2) asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        }
        if constexpr (NT == 1 && NP == 1) {
            if (blocks == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
    };
    // operand fragments of the two k-steps from PK pieces at `base` ([plane * 2 + s])
    auto load_op = [&](SP (&f)[2], const bf16x8* base) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f[s].h = base[(0 + s) * 64];
            if constexpr (NP == 3) {
                f[s].m = base[(2 + s) * 64];
                f[s].l = base[(4 + s) * 64];
            }
        }
    };
    auto load_k = [&](SP (&kf)[2], int gslot) { load_op(kf, ring + (gslot & (X3_SLOTS - 1)) * SLOT_UNITS + lane); };
    int bh = blockIdx.x;
    int gb = 0;                                      // global block counter -> ring slot
    issue_block(bh, 0, 0);
    issue_block(bh, 1, 1);
    issue_block(bh, 2, 2);

    SP qa[2], qb[2];
    f32x4 qna[4], qnb[4];
    {
        const f32x4* qg = qall + (size_t)bh * NKB * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            qna[g] = qg[(t0 * 4 + g) * 64 + lane];
            qnb[g] = (NT == 2) ? qg[((t0 + 1) * 4 + g) * 64 + lane] : qna[g];
        }
        load_q(qna, qa);
        load_q(qnb, qb);
    }
    wait_but(2);                                     // block 0 landed
    __builtin_amdgcn_s_barrier();
    SP kf[2];
    load_k(kf, 0);

#pragma unroll 1
    for (; bh < BH; bh += stride) {
        f32x16 oa, ob;
        TileState ta, tb;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            oa[r] = ob[r] = 0.f;
            ta.negm[r] = tb.negm[r] = INFINITY;
        }
        ta.m_ref = tb.m_ref = -INFINITY;
        ta.l_lane = tb.l_lane = 0.f;

#pragma unroll 1
        for (int jb = 0; jb < NKB; ++jb, ++gb) {
            // ---- QK^T (MFMA)
            // block 0 of a head has no reference yet: straight to the reference-setting path (one QK pass, not two)
            const bool first = jb == 0;                           // scalar
            f32x16 sta = ta.negm, stb = tb.negm;
            if (!first) {
                sta = scores_from(kf, qa, ta.negm);
                if (NT == 2) stb = scores_from(kf, qb, tb.negm);
            }
            if (STAG) {
                wait_but(1);
                __builtin_amdgcn_s_barrier();
                issue_block(bh, jb + 3, gb + 3);
            }
            SP vf[2];
            load_op(vf, ring + (gb & (X3_SLOTS - 1)) * SLOT_UNITS + PK * 64 + lane);
            // ---- softmax + split of P^T (VALU)
            float psa = 0.f, psb = 0.f;
            bool redo = first;
            if (!first) {
                psa = exp_sum(sta);
                if (NT == 2) psb = exp_sum(stb);
                const bool stale = !(psa < SM_BIG) || !(psb < SM_BIG);
                redo = __builtin_amdgcn_ballot_w64(stale) != 0;   // wave-uniform, rare
            }
            if (redo) {
                psa = rereference(kf, qa, sta, oa, ta);
                if (NT == 2) psb = rereference(kf, qb, stb, ob, tb);
            }
            ta.l_lane += psa;
            tb.l_lane += psb;
            // (one plane: P is rounded to bf16 here, for PV only -- the running sum above took the unrounded P)
            const SP pa0 = splitp_acc<SP>(sta, 0), pa1 = splitp_acc<SP>(sta, 1);
            SP pb0 = pa0, pb1 = pa1;
            if (NT == 2) { pb0 = splitp_acc<SP>(stb, 0); pb1 = splitp_acc<SP>(stb, 1); }
            if (!STAG) {
                wait_but(1);
                __builtin_amdgcn_s_barrier();
                issue_block(bh, jb + 3, gb + 3);
            }
            // K fragments of the next block (landed: barrier above), read behind the PV MFMAs
            load_k(kf, gb + 1);
            // ---- PV (MFMA): O^T += V^T P^T
            oa = mfma_x3(vf[0], pa0, oa);
            oa = mfma_x3(vf[1], pa1, oa);
            if (NT == 2) {
                ob = mfma_x3(vf[0], pb0, ob);
                ob = mfma_x3(vf[1], pb1, ob);
            }
            // prefetch the next head's Q fragments (a whole block old by the next counted wait)
            if (jb == NKB - 4 && bh + stride < BH) {
                const f32x4* qg = qall + (size_t)(bh + stride) * NKB * 256;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    qna[g] = qg[(t0 * 4 + g) * 64 + lane];
                    if (NT == 2) qnb[g] = qg[((t0 + 1) * 4 + g) * 64 + lane];
                }
            }
        }
        // ---- normalise and store O of this head; swap in the prefetched Q ----
        const int seq = bh / NH, head = bh % NH;
        {
            const float inv = 1.0f / pair_sum(ta.l_lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = {oa[4 * g] * inv, oa[4 * g + 1] * inv, oa[4 * g + 2] * inv, oa[4 * g + 3] * inv};
                og[(((size_t)seq * NKB + t0) * 16 + head * 4 + g) * 64 + lane] = w;
            }
        }
        if (NT == 2) {
            const float inv = 1.0f / pair_sum(tb.l_lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = {ob[4 * g] * inv, ob[4 * g + 1] * inv, ob[4 * g + 2] * inv, ob[4 * g + 3] * inv};
                og[(((size_t)seq * NKB + t0 + 1) * 16 + head * 4 + g) * 64 + lane] = w;
            }
        }
        load_q(qna, qa);
        if (NT == 2) load_q(qnb, qb);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the trailing (unused) DMAs
}

template <class SP>
__device__ __forceinline__ void attn_fwd_xn(bf16x8* ring3, const float* __restrict__ q, const __bf16* __restrict__ k3,
                                            const __bf16* __restrict__ vT3, float* __restrict__ o, int BH) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f32x4* qg = reinterpret_cast<const f32x4*>(q);
    const bf16x8* kg = reinterpret_cast<const bf16x8*>(k3);
    const bf16x8* vg = reinterpret_cast<const bf16x8*>(vT3);
    f32x4* og = reinterpret_cast<f32x4*>(o);
    // (measured: without the stagger 324 us, with 313 us; s_setprio 1 for waves 4-7 on top: 320 us)
    constexpr int SG = 1;
    if (wave < 4)
        attn_x3_body<2, 0, SP>(ring3, qg, kg, vg, og, BH, lane, wave);
    else if (wave < 7)
        attn_x3_body<2, SG, SP>(ring3, qg, kg, vg, og, BH, lane, wave);
    else
        attn_x3_body<1, SG, SP>(ring3, qg, kg, vg, og, BH, lane, wave);   // tile 14 only (15 is void)
}

// k3 / vT3: split planes (BH*15 tiles x 6 KiB each); q, o: fp32 fragment-major as in t2s_attn_fwd_packed
__global__ __launch_bounds__(X3_THREADS, 2) T2S_X3_KERNEL void attn_fwd_x3_kernel(const float* __restrict__ q,
                                                                    const __bf16* __restrict__ k3,
                                                                    const __bf16* __restrict__ vT3,
                                                                    float* __restrict__ o, int BH) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 ring3[];
    attn_fwd_xn<Split3>(ring3, q, k3, vT3, o, BH);
}

// the one-plane form (T2S_MATH_BF16): k1 / vT1 one bf16 plane (BH*15 tiles x 2 KiB each), 2 + 2 MFMAs per key block and
// query tile; a separate instantiation of the same body, not a run-time branch inside it
__global__ __launch_bounds__(X3_THREADS, 2) T2S_P1_KERNEL void attn_fwd_bf16p_kernel(const float* __restrict__ q,
                                                                       const __bf16* __restrict__ k1,
                                                                       const __bf16* __restrict__ vT1,
                                                                       float* __restrict__ o, int BH) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 ring1[];
    attn_fwd_xn<Split1>(ring1, q, k1, vT1, o, BH);
}


// ---------------------------------------------------------------- the wide form: 800 / 1024 tokens (t2s_dit_set_wide_math)
// nkb = 25 or 32 key blocks and as many query tiles per head, against 16 tile slots of the workgroup (8 waves x 2 tiles).
// A persistent WORK ITEM is therefore a (head, part) pair, item = 2 bh + part: part p holds the query tiles 16 p .. 16 p + 15
// and streams ALL nkb key blocks of the head through the same 4-slot ring; a workgroup walks items blockIdx.x,
// blockIdx.x + gridDim.x, ...  The ring protocol, the barrier per key block and the stagger are those of attn_x3_body; what
// differs:
//
// Tiles.  Wave w of part p owns tiles 16 p + 2 w and 16 p + 2 w + 1 -- a fixed function of the tile index, so the two tiles
// that share the wave-uniform re-reference branch are the same two in every launch, batch and grid (a row's bits do not depend
// on them).  1024 tokens: two full parts.  800 tokens: part 0 is full, part 1 holds tiles 16 .. 24 -- waves 0-3 two tiles, wave
// 4 one, waves 5-7 none.  A slot without a tile REPEATS tile nkb - 1 (same Q, same scores, so it never changes the wave's
// branch) and stores nothing: every wave runs the same nkb barriers per item.  7 of the 32 slots of a head idle at 800 tokens.
//
// LDS-DMA.  Every wave owns two tiles, so there is no light wave to carry the issue: wave w issues pieces w and w + 8 of a
// block's 2 PK (12 for bf16x3, 4 for one plane), i.e. NPW pieces per block and wave
//     bf16x3:    waves 0-3 two (w, w + 8), waves 4-7 one (w)          one plane: waves 0-3 one (w), waves 4-7 none.
// Waves 0-3 are the STAG = 0 instantiation and waves 4-7 the STAG = 1 one, so NPW is a compile-time value of the body.
//
// Counted waits, per wave (vmcnt counts a wave's own vector-memory operations, oldest first).  Barrier j must guarantee
// that block j + 1 has landed, i.e. each issuing wave must have seen ITS pieces of block j + 1 land before it arrives.  At
// that point the wave has issued, after those pieces, exactly its NPW pieces of block j + 2 (block j + 3 is issued behind
// the barrier) and possibly loads / stores of its own (the Q prefetch, the O stores of the previous item).  "At most NPW
// operations outstanding" = s_waitcnt vmcnt(NPW) therefore covers every piece of block j + 1: with nothing else in flight
// the NPW youngest are the pieces of block j + 2, and anything else in flight is younger than block j + 1's pieces too, so
// it only makes the wait stricter.  Before the first barrier blocks 1 and 2 are behind block 0: vmcnt(2 NPW).  A wave with
// NPW = 0 has nothing to wait for.  The stream of blocks runs on across items (block nkb + d of an item is block d of the
// workgroup's next item), so the count holds at item borders as well; past the last item the last block is fetched again
// into slots nobody reads and drained by the final vmcnt(0).
template <int STAG, class SP>
__device__ __forceinline__ void attn_xw_body(bf16x8* ring, const f32x4* qall, const bf16x8* kall, const bf16x8* vall,
                                             f32x4* og, int BH, int nkb, int lane, int wave) {
    const int stride = gridDim.x;
    const int n_items = 2 * BH;
    constexpr int NP = planes_of<SP>::n;
    constexpr int PK = 2 * NP;
    constexpr int SLOT_UNITS = 2 * XN_TILE_UNITS<NP>;
    constexpr int NPW = STAG ? (NP == 3 ? 1 : 0) : (NP == 3 ? 2 : 1);
    static_assert(4 * (NP == 3 ? 2 : 1) + 4 * (NP == 3 ? 1 : 0) == 2 * PK, "every piece of a block has one issuing wave");
    auto issue_block = [&](int it, int jb, int gslot) {
        if constexpr (NPW > 0) {
            if (jb >= nkb) { jb -= nkb; it += stride; }
            if (it >= n_items) { it -= stride; jb = nkb - 1; }   // past the end: harmless re-fetch
            const int bh = it >> 1;
#pragma unroll
            for (int i = 0; i < NPW; ++i) {
                const int p = wave + 8 * i;                       // < 2 PK by the table above
                const bf16x8* src = (p < PK ? kall : vall) + ((size_t)(bh * nkb + jb) * PK + (p < PK ? p : p - PK)) * 64 + lane;
                glds16u(src, ring + (gslot & (X3_SLOTS - 1)) * SLOT_UNITS + p * 64);
            }
        }
    };
    auto wait_but = [&](int blocks) {
        if constexpr (NPW == 2) {
            if (blocks == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        }
        if constexpr (NPW == 1) {
            if (blocks == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        }
    };
    auto load_op = [&](SP (&f)[2], const bf16x8* base) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f[s].h = base[(0 + s) * 64];
            if constexpr (NP == 3) {
                f[s].m = base[(2 + s) * 64];
                f[s].l = base[(4 + s) * 64];
            }
        }
    };
    auto load_k = [&](SP (&kf)[2], int gslot) { load_op(kf, ring + (gslot & (X3_SLOTS - 1)) * SLOT_UNITS + lane); };
    // the raw fragments of the wave's two tiles of item `it` (a void slot repeats the head's last tile)
    auto fetch_q = [&](int it, f32x4 (&ra)[4], f32x4 (&rb)[4]) {
        const int t0 = (it & 1) * 16 + wave * 2;
        const int ta = t0 < nkb ? t0 : nkb - 1, tb = t0 + 1 < nkb ? t0 + 1 : nkb - 1;
        const f32x4* qg = qall + (size_t)(it >> 1) * nkb * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            ra[g] = qg[(ta * 4 + g) * 64 + lane];
            rb[g] = qg[(tb * 4 + g) * 64 + lane];
        }
    };
    int it = blockIdx.x;
    int gb = 0;
    issue_block(it, 0, 0);
    issue_block(it, 1, 1);
    issue_block(it, 2, 2);

    SP qa[2], qb[2];
    f32x4 qna[4], qnb[4];
    fetch_q(it, qna, qnb);
    load_q(qna, qa);
    load_q(qnb, qb);
    wait_but(2);                                     // block 0 landed
    __builtin_amdgcn_s_barrier();
    SP kf[2];
    load_k(kf, 0);

#pragma unroll 1
    for (; it < n_items; it += stride) {
        f32x16 oa, ob;
        TileState ta, tb;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            oa[r] = ob[r] = 0.f;
            ta.negm[r] = tb.negm[r] = INFINITY;
        }
        ta.m_ref = tb.m_ref = -INFINITY;
        ta.l_lane = tb.l_lane = 0.f;

#pragma unroll 1
        for (int jb = 0; jb < nkb; ++jb, ++gb) {
            const bool first = jb == 0;                           // scalar
            f32x16 sta = ta.negm, stb = tb.negm;
            if (!first) {
                sta = scores_from(kf, qa, ta.negm);
                stb = scores_from(kf, qb, tb.negm);
            }
            if (STAG) {
                wait_but(1);
                __builtin_amdgcn_s_barrier();
                issue_block(it, jb + 3, gb + 3);
            }
            SP vf[2];
            load_op(vf, ring + (gb & (X3_SLOTS - 1)) * SLOT_UNITS + PK * 64 + lane);
            float psa = 0.f, psb = 0.f;
            bool redo = first;
            if (!first) {
                psa = exp_sum(sta);
                psb = exp_sum(stb);
                const bool stale = !(psa < SM_BIG) || !(psb < SM_BIG);
                redo = __builtin_amdgcn_ballot_w64(stale) != 0;   // wave-uniform, rare
            }
            if (redo) {
                psa = rereference(kf, qa, sta, oa, ta);
                psb = rereference(kf, qb, stb, ob, tb);
            }
            ta.l_lane += psa;
            tb.l_lane += psb;
            const SP pa0 = splitp_acc<SP>(sta, 0), pa1 = splitp_acc<SP>(sta, 1);
            const SP pb0 = splitp_acc<SP>(stb, 0), pb1 = splitp_acc<SP>(stb, 1);
            if (!STAG) {
                wait_but(1);
                __builtin_amdgcn_s_barrier();
                issue_block(it, jb + 3, gb + 3);
            }
            load_k(kf, gb + 1);
            oa = mfma_x3(vf[0], pa0, oa);
            oa = mfma_x3(vf[1], pa1, oa);
            ob = mfma_x3(vf[0], pb0, ob);
            ob = mfma_x3(vf[1], pb1, ob);
            // prefetch the next item's Q fragments (a whole block old by the next counted wait)
            if (jb == nkb - 4 && it + stride < n_items) fetch_q(it + stride, qna, qnb);
        }
        // ---- normalise and store O of this item's tiles (void slots store nothing); swap in the prefetched Q ----
        const int bh = it >> 1, seq = bh / NH, head = bh % NH;
        const int t0 = (it & 1) * 16 + wave * 2;
        if (t0 < nkb) {
            const float inv = 1.0f / pair_sum(ta.l_lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = {oa[4 * g] * inv, oa[4 * g + 1] * inv, oa[4 * g + 2] * inv, oa[4 * g + 3] * inv};
                og[(((size_t)seq * nkb + t0) * 16 + head * 4 + g) * 64 + lane] = w;
            }
        }
        if (t0 + 1 < nkb) {
            const float inv = 1.0f / pair_sum(tb.l_lane);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = {ob[4 * g] * inv, ob[4 * g + 1] * inv, ob[4 * g + 2] * inv, ob[4 * g + 3] * inv};
                og[(((size_t)seq * nkb + t0 + 1) * 16 + head * 4 + g) * 64 + lane] = w;
            }
        }
        load_q(qna, qa);
        load_q(qnb, qb);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the trailing (unused) DMAs
}

template <class SP>
__device__ __forceinline__ void attn_fwd_xw(bf16x8* ring, const float* __restrict__ q, const __bf16* __restrict__ kp,
                                            const __bf16* __restrict__ vTp, float* __restrict__ o, int BH, int nkb) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f32x4* qg = reinterpret_cast<const f32x4*>(q);
    const bf16x8* kg = reinterpret_cast<const bf16x8*>(kp);
    const bf16x8* vg = reinterpret_cast<const bf16x8*>(vTp);
    f32x4* og = reinterpret_cast<f32x4*>(o);
    // the stagger of the 480-token kernel, kept: the SIMD partners w / w + 4 still run one body each
    if (wave < 4)
        attn_xw_body<0, SP>(ring, qg, kg, vg, og, BH, nkb, lane, wave);
    else
        attn_xw_body<1, SP>(ring, qg, kg, vg, og, BH, nkb, lane, wave);
}

// kp / vTp: planes (BH * nkb tiles, 2 NP pieces each); q, o: fp32 fragment-major as in t2s_attn_fwd_packed_n
__global__ __launch_bounds__(X3_THREADS, 2) T2S_X3_KERNEL void attn_fwd_x3_wide_kernel(const float* __restrict__ q,
                                                                         const __bf16* __restrict__ k3,
                                                                         const __bf16* __restrict__ vT3,
                                                                         float* __restrict__ o, int BH, int nkb) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 ring3w[];
    attn_fwd_xw<Split3>(ring3w, q, k3, vT3, o, BH, nkb);
}
__global__ __launch_bounds__(X3_THREADS, 2) T2S_P1_KERNEL void attn_fwd_bf16p_wide_kernel(const float* __restrict__ q,
                                                                            const __bf16* __restrict__ k1,
                                                                            const __bf16* __restrict__ vT1,
                                                                            float* __restrict__ o, int BH, int nkb) {
    extern __shared__ __attribute__((aligned(16))) bf16x8 ring1w[];
    attn_fwd_xw<Split1>(ring1w, q, k1, vT1, o, BH, nkb);
}

// plain (BH, 32 nkb, 32) fp32 k or v -> split planes: k as the A operand with the key on the lane
// (transpose = 0), v as V^T with the feature on the lane (transpose = 1)
template <int NP>
__global__ void pack_xn_kernel(const float* __restrict__ src, bf16x8* __restrict__ dst, int BH, int nkb, int transpose) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // one (bh, tile, s, lane)
    if (idx >= BH * nkb * 2 * 64) return;
    const int ntok = 32 * nkb;
    const int lane = idx & 63, s = (idx >> 6) & 1, tile = (idx >> 7) % nkb, bh = idx / (nkb * 128);
    const int i = lane & 31, h = lane >> 5;
    f32x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kk = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);     // permuted k order of the fragment
        v[j] = transpose ? src[((size_t)bh * ntok + tile * 32 + kk) * DH + i]     // V^T[d = i][key = kk]
                         : src[((size_t)bh * ntok + tile * 32 + i) * DH + kk];    // K[key = i][d = kk]
    }
    const Split3 sp = split3(v);   // (the one-plane form keeps h = rn_bf16(v))
    bf16x8* d = dst + ((size_t)(bh * nkb + tile) * 2 * NP + s) * 64 + lane;
    d[0] = sp.h;
    if constexpr (NP == 3) {
        d[2 * 64] = sp.m;
        d[4 * 64] = sp.l;
    }
}
}  // namespace

// host side: one set of helpers for both plane counts (np = 3: bf16x3, np = 1: the one-plane form)
struct AttnXn {
    void (*kernel)(const float*, const __bf16*, const __bf16*, float*, int);
    void (*wide)(const float*, const __bf16*, const __bf16*, float*, int, int);   // 800 / 1024 tokens
    int lds_bytes;
};
static AttnXn attn_xn(int np) {
    return np == 3 ? AttnXn{attn_fwd_x3_kernel, attn_fwd_x3_wide_kernel, X3_LDS_BYTES}
                   : AttnXn{attn_fwd_bf16p_kernel, attn_fwd_bf16p_wide_kernel, P1_LDS_BYTES};
}

int attn_xn_init(int np) {   // once per kernel, outside any stream capture (16 KiB of LDS needs no opt-in; a ring may grow)
    static bool done[4] = {};
    if (!done[np]) {
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_xn(np).kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, attn_xn(np).lds_bytes));
        T2S_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_xn(np).wide),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, attn_xn(np).lds_bytes));
        done[np] = true;
    }
    return T2S_OK;
}

static int attn_xn_grid(int items) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            n_cu = prop.multiProcessorCount;
        else
            n_cu = 256;
    }
    return items < n_cu ? items : n_cu;   // one persistent workgroup per CU
}

int launch_attn_xn(int np, const float* q, const __bf16* k, const __bf16* vT, float* o, int BH, int n_tok, hipStream_t st) {
    const AttnXn x = attn_xn(np);
    if (n_tok == NTOK) {
        x.kernel<<<attn_xn_grid(BH), X3_THREADS, x.lds_bytes, st>>>(q, k, vT, o, BH);
    } else {
        if ((n_tok != 800 && n_tok != 1024) || BH <= 0 || BH > (1 << 22)) {
            set_error("attention (%d planes): n_tok=%d must be 480, 800 or 1024 (BH=%d)", np, n_tok, BH);
            return T2S_E_INVALID;
        }
        x.wide<<<attn_xn_grid(2 * BH), X3_THREADS, x.lds_bytes, st>>>(q, k, vT, o, BH, n_tok / 32);   // items = (head, part)
    }
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

template <int NP>
static int pack_xn(const float* src, __bf16* dst, int BH, int nkb, int transpose, hipStream_t st) {
    const int n = BH * nkb * 2 * 64;
    pack_xn_kernel<NP><<<(n + 255) / 256, 256, 0, st>>>(src, reinterpret_cast<bf16x8*>(dst), BH, nkb, transpose);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

}  // namespace t2s

// ------------------------------------------------------------------ C ABI: stand-alone entry on plain tensors
namespace {
using namespace t2s;
// q (BH, 32 nkb, 32) -> fp32 fragment-major [(bh*nkb + tile)*4 + g][lane][e] = Q[32 tile + i][8g + 4h + e]
__global__ void q_to_frag_kernel(const float* __restrict__ q, f32x4* __restrict__ qf, int BH, int nkb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= BH * nkb * 4 * 64) return;
    const int lane = idx & 63, g = (idx >> 6) & 3, tile = (idx >> 8) % nkb, bh = idx / (nkb * 256);
    qf[idx] = *reinterpret_cast<const f32x4*>(q + ((size_t)bh * nkb * 32 + tile * 32 + (lane & 31)) * DH + 8 * g + 4 * (lane >> 5));
}
// o fragment-major [((seq*nkb + tile)*16 + head*4 + g)][lane][e] -> (BH, 32 nkb, 32)
__global__ void o_from_frag_kernel(const f32x4* __restrict__ of, float* __restrict__ o, int BH, int nkb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= BH * nkb * 4 * 64) return;
    const int lane = idx & 63, g = (idx >> 6) & 3, tile = (idx >> 8) % nkb, bh = idx / (nkb * 256);
    const int seq = bh / NH, head = bh % NH;
    *reinterpret_cast<f32x4*>(o + ((size_t)bh * nkb * 32 + tile * 32 + (lane & 31)) * DH + 8 * g + 4 * (lane >> 5)) =
        of[(((size_t)seq * nkb + tile) * 16 + head * 4 + g) * 64 + lane];
}
}  // namespace

// NP = 3: bf16x3, NP = 1: the one-plane form
template <int NP>
static int attn_fwd_plain(const char* who, const float* q, const float* k, const float* v, float* o, int BH, int n_tok, void* stream) {
    T2S_REQUIRE(n_tok == 480 || n_tok == 800 || n_tok == 1024, "%s: n_tok=%d must be 480, 800 or 1024", who, n_tok);
    T2S_REQUIRE(q && k && v && o && BH > 0 && BH % NH == 0, "%s: bad argument (BH=%d must be a multiple of 4)", who, BH);
    const int nkb = n_tok / 32;
    T2S_REQUIRE((long long)BH * nkb * 256 <= 0x7fffffffLL, "%s: BH=%d at n_tok=%d exceeds the helpers' 32-bit index", who, BH, n_tok);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = attn_xn_init(NP)) return rc;
    const size_t n = (size_t)BH * n_tok * DH;
    float* f32buf = nullptr;
    __bf16* planes = nullptr;
    T2S_HIP_CHECK(hipMalloc(&f32buf, 2 * n * sizeof(float)));
    if (hipMalloc(&planes, 2 * NP * n * sizeof(__bf16)) != hipSuccess) {
        (void)hipFree(f32buf);
        set_error("%s: hipMalloc failed", who);
        return T2S_E_HIP;
    }
    const int nf = BH * nkb * 4 * 64;
    q_to_frag_kernel<<<(nf + 255) / 256, 256, 0, st>>>(q, reinterpret_cast<f32x4*>(f32buf), BH, nkb);
    int rc = pack_xn<NP>(k, planes, BH, nkb, 0, st);
    if (rc == T2S_OK) rc = pack_xn<NP>(v, planes + NP * n, BH, nkb, 1, st);
    if (rc == T2S_OK) rc = launch_attn_xn(NP, f32buf, planes, planes + NP * n, f32buf + n, BH, n_tok, st);
    if (rc == T2S_OK) {
        o_from_frag_kernel<<<(nf + 255) / 256, 256, 0, st>>>(reinterpret_cast<const f32x4*>(f32buf + n), o, BH, nkb);
        if (hipGetLastError() != hipSuccess) rc = T2S_E_HIP;
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(f32buf);
    (void)hipFree(planes);
    return rc;
}

extern "C" int t2s_attn_fwd_x3(const float* q, const float* k, const float* v, float* o, int BH, void* stream) {
    return attn_fwd_plain<3>("t2s_attn_fwd_x3", q, k, v, o, BH, NTOK, stream);
}

extern "C" int t2s_attn_fwd_bf16p(const float* q, const float* k, const float* v, float* o, int BH, void* stream) {
    return attn_fwd_plain<1>("t2s_attn_fwd_bf16p", q, k, v, o, BH, NTOK, stream);
}

// include/t2s_wide_math.h
extern "C" int t2s_attn_fwd_x3_n(const float* q, const float* k, const float* v, float* o, int BH, int n_tok, void* stream) {
    return attn_fwd_plain<3>("t2s_attn_fwd_x3_n", q, k, v, o, BH, n_tok, stream);
}

extern "C" int t2s_attn_fwd_bf16p_n(const float* q, const float* k, const float* v, float* o, int BH, int n_tok, void* stream) {
    return attn_fwd_plain<1>("t2s_attn_fwd_bf16p_n", q, k, v, o, BH, n_tok, stream);
}
