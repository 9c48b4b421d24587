// What the TSae translation units share (t2s_tsae.hip: inference entries, create / update; t2s_tsae_train.hip: the teacher-forced
// training forward and backward): the handle, the layout of its weight blob, LayerNorm over a wave and the exact-f32 MFMA tile.
#pragma once
#include "t2s_common.h"

#include <math.h>

#include <vector>

namespace t2s {
namespace tsae {

constexpr int TS_D = T2S_TSAE_D_MODEL;        // 64
constexpr int TS_ML = T2S_TSAE_MAX_LAYERS;    // 6
constexpr int TS_MAXT = T2S_TSAE_MAX_T;       // 2000
constexpr int TS_MAXF = T2S_TSAE_MAX_FEATURES;  // 16
constexpr int TS_MAXFF = T2S_TSAE_MAX_D_FF;   // 512
constexpr float TS_EPS = 1e-5f;

// Packed at create: a Linear (N,K) becomes w (K, Npad) -- consecutive outputs are consecutive floats -- and b (Npad), zero padded;
// t is the same weight as torch holds it, (N rounded up to 32, K) with zero rows behind N: the operand of the backward's
// data-gradient products (NULL where no gradient flows to the input: the two embeddings).
struct Lin { const float* w; const float* b; const float* t; };
struct Norm { const float* g; const float* b; };
struct EncLayerP { Lin qkv, out, l1, l2; Norm n1, n2; };
struct DecLayerP { Lin qkv, out, cq, ckv, cout, l1, l2; Norm n1, n2, n3; };
struct GenP {
    DecLayerP L[TS_ML];
    Lin inp, outp;
    const float* pe;
    int n_dec, dff, F;
};

// One tensor pair of t2s_tsae_weights and where it lives in the blob: the create-time packing as data, replayed on the device by
// t2s_tsae_update_weights.  w_field / b_field are byte offsets of the two pointers inside t2s_tsae_weights; rows [r0, r0 + N) of
// the (.., K) weight go to off_w as (K, Npad) and, if off_t, to off_t as (N, K); the bias rows to off_b.  (A LayerNorm is K = 1.)
struct PackItem {
    uint32_t w_field, b_field;
    int r0, N, K, Npad;
    uint32_t off_w, off_b, off_t;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LayerNorm over the 64 channels a wave holds one per lane (biased variance, eps 1e-5)
__device__ __forceinline__ float layer_norm_lane(float v, float g, float b) {
    const float mean = wave_sum(v) * (1.0f / TS_D);
    const float d = v - mean;
    const float var = wave_sum(d * d) * (1.0f / TS_D);
    return d * (1.0f / sqrtf(var + TS_EPS)) * g + b;
}

// One wave: acc(32 x 32) += xs(32 rows x [k0,k1), row stride ldx, LDS) . wt([k0,k1) x ldw, global)[:, n0 .. n0+31]; k1 - k0 a multiple of 16.
__device__ __forceinline__ f32x16 tile_gemm(const float* xs, int ldx, const float* __restrict__ wt, int ldw, int n0, int k0, int k1,
                                            f32x16 acc) {
    const int lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
    const float* xp = xs + j * ldx + k0 + half;
    const float* wp = wt + (size_t)(k0 + half) * ldw + n0 + j;
    for (int k = k0; k < k1; k += 16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = mfma32(xp[2 * e], wp[(size_t)(2 * e) * ldw], acc);
        xp += 16;
        wp += 16 * (size_t)ldw;
    }
    return acc;
}

}  // namespace tsae
}  // namespace t2s

struct t2s_tsae {
    int F = 0, dff = 0, heads = 0, n_enc = 0, n_dec = 0;
    float* blob = nullptr;
    t2s::tsae::Lin emb{};
    t2s::tsae::Norm emb_ln{};
    t2s::tsae::EncLayerP enc[t2s::tsae::TS_ML]{};
    t2s::tsae::GenP dec{};
    std::vector<t2s::tsae::PackItem> items;   // every tensor pair of the blob, in create order
    t2s::tsae::PackItem* items_dev = nullptr;  // the same on the device, inside the blob's allocation
};

#define TS_TRY(expr)                 \
    do {                             \
        const int _rc = (expr);      \
        if (_rc != T2S_OK) return _rc; \
    } while (0)
