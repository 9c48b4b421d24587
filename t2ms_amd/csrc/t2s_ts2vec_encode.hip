// TS2Vec encoder forward at any series length up to T2S_TS2VEC_ENCODE_MAX_T (t2s_ts2vec_encode_long): the function of
// t2s_ts2vec_encode (t2s_eval.hip) with the three activation planes in a caller-owned workspace instead of LDS and every
// dilated convolution as a GEMM on the exact-f32 matrix instruction (mfma32, t2s_common.h).
//
// Workspace: [packed weights of the 2 (depth + 1) convolutions][H][G][Y], every part 256-byte aligned.
//   H, G, Y   (B, CP, T) fp32 planes, CP = max(hidden, output_dims) rounded up to 32.  H = the raw residual stream,
//             G = gelu(H), Y = gelu(conv1 output).  Every launch writes whole 32-row tiles (zero weights and biases give
//             exact zeros in the padding rows), so no row is read before this call wrote it.
//   packed    per convolution (m tile, k step, lane): lane l of k step s of m tile m holds A[32 m + (l & 31)][2 s + (l >> 5)],
//             the A fragment of one mfma32 as one coalesced 256-byte read.  K runs tap-major: k = tap * KC + ci with
//             KC = ci rounded up to 2; the final conv2 appends the 1x1 projector's KP = hidden (rounded up to 2) rows.
// Launches per call: 1 pack + 1 input_fc + 2 (depth + 1) convolutions + 1 finish = 2 depth + 5 (25 at depth 10).
//   A wave owns (series, 32 time steps): its B fragment is 32 consecutive time steps of two channel rows (two coalesced
//   128-byte reads, predicated at the series' ends) and all M tiles of a group of <= 4 run against it.  No LDS, no
//   barrier, no atomics.  An output element is acc = sum over k in the order above, one fmaf chain inside the matrix
//   instruction starting from 0, then + bias (+ projector bias) (+ residual): the order depends on neither the tile nor
//   the series' place in the batch nor B.  A block whose dilation is >= T runs its centre tap only.
//   finish transposes the final (C, T) plane to rep (B, T, C) through a 32 x 32 LDS tile and takes full = max over time
//   in a fixed order (per channel: 32 strided running maxima, then a 5-step butterfly).
#include <stdio.h>

#include "t2s_common.h"

namespace t2s {
namespace {

constexpr int ENC_MAX_IN = 64, ENC_MAX_HIDDEN = 128, ENC_MAX_OUT = 320;
constexpr int ENC_MAX_CONVS = 2 * T2S_TS2VEC_MAX_BLOCKS;

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

inline int up(int v, int m) { return (v + m - 1) / m * m; }
inline uint64_t up256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// The shape of one packed convolution.
struct EncConv {
    int ci, co;        // true widths
    int kc;            // K rows per tap (ci rounded up to 2)
    int kp;            // projector K rows appended after the three taps (0 or hidden rounded up to 2)
    int mt;            // M tiles in the packed image (a multiple of `group`)
    int group;         // M tiles one wave runs against a B fragment: 1..4
    int ks;            // k steps per M tile = (3 kc + kp) / 2
    uint64_t off;      // float offset of the packed image in the workspace
};

struct EncPlan {
    int n_convs, cp, ntiles;
    EncConv conv[ENC_MAX_CONVS];
    uint64_t packed_floats, plane_floats;     // plane_floats: one of H / G / Y
    uint64_t off_h, off_g, off_y, total;      // byte offsets
};

const char* enc_check(const t2s_ts2vec_weights* w, int B, int T, char* msg, size_t n) {
    if (w == nullptr) { snprintf(msg, n, "NULL weights"); return msg; }
    if (T < 1 || T > T2S_TS2VEC_ENCODE_MAX_T) { snprintf(msg, n, "T=%d is outside [1, %d]", T, T2S_TS2VEC_ENCODE_MAX_T); return msg; }
    if (B < 1) { snprintf(msg, n, "B=%d must be at least 1", B); return msg; }
    if (w->depth < 0 || w->depth >= T2S_TS2VEC_MAX_BLOCKS) { snprintf(msg, n, "depth=%d is outside [0, %d]", w->depth, T2S_TS2VEC_MAX_BLOCKS - 1); return msg; }
    if (w->input_dims < 1 || w->input_dims > ENC_MAX_IN) { snprintf(msg, n, "input_dims=%d is outside [1, %d]", w->input_dims, ENC_MAX_IN); return msg; }
    if (w->hidden < 1 || w->hidden > ENC_MAX_HIDDEN) { snprintf(msg, n, "hidden=%d is outside [1, %d]", w->hidden, ENC_MAX_HIDDEN); return msg; }
    if (w->output_dims < 1 || w->output_dims > ENC_MAX_OUT) { snprintf(msg, n, "output_dims=%d is outside [1, %d]", w->output_dims, ENC_MAX_OUT); return msg; }
    // one wave per (series, 32 steps), four waves per workgroup, a one-dimensional grid
    if ((uint64_t)B * (uint64_t)((T + 31) / 32) > (uint64_t)1 << 32) { snprintf(msg, n, "B=%d x T=%d exceeds 2^32 time tiles", B, T); return msg; }
    return nullptr;
}

EncPlan enc_plan(const t2s_ts2vec_weights* w, int B, int T) {
    EncPlan p{};
    p.n_convs = 2 * (w->depth + 1);
    p.cp = up(w->hidden > w->output_dims ? w->hidden : w->output_dims, 32);
    p.ntiles = (T + 31) / 32;
    uint64_t off = 0;
    for (int j = 0; j < p.n_convs; ++j) {
        const int blk = j >> 1;
        const bool last = blk == w->depth, second = (j & 1) != 0;
        EncConv& c = p.conv[j];
        c.co = last ? w->output_dims : w->hidden;
        c.ci = (last && second) ? w->output_dims : w->hidden;
        c.kc = up(c.ci, 2);
        c.kp = (last && second) ? up(w->hidden, 2) : 0;
        const int tiles = (c.co + 31) / 32;
        c.group = tiles < 4 ? tiles : 4;
        c.mt = up(tiles, c.group);
        c.ks = (3 * c.kc + c.kp) / 2;
        c.off = off;
        off += (uint64_t)c.mt * c.ks * 64;
    }
    p.packed_floats = off;
    p.plane_floats = (uint64_t)B * p.cp * T;
    p.off_h = up256(p.packed_floats * sizeof(float));
    p.off_g = p.off_h + up256(p.plane_floats * sizeof(float));
    p.off_y = p.off_g + up256(p.plane_floats * sizeof(float));
    p.total = p.off_y + up256(p.plane_floats * sizeof(float));
    return p;
}

struct EncPackDev {
    const float* w[ENC_MAX_CONVS];     // (co, ci, 3)
    const float* pw;                   // (output_dims, hidden) projector, rows of the last convolution
    int ci[ENC_MAX_CONVS], co[ENC_MAX_CONVS], kc[ENC_MAX_CONVS], kp[ENC_MAX_CONVS], ks[ENC_MAX_CONVS], mt[ENC_MAX_CONVS];
    unsigned long long off[ENC_MAX_CONVS];
    int hidden;
};

// grid (blocks, convolution): every float of every packed image is written, zeros where the row or the channel is padding.
__global__ __launch_bounds__(256) void enc_pack_kernel(const EncPackDev d, float* __restrict__ packed) {
    const int j = blockIdx.y;
    const int ci = d.ci[j], co = d.co[j], kc = d.kc[j], kp = d.kp[j], ks = d.ks[j];
    const size_t n = (size_t)d.mt[j] * ks * 64;
    float* out = packed + d.off[j];
    const float* w = d.w[j];
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
        const int lane = (int)(idx & 63);
        const size_t q = idx >> 6;
        const int s = (int)(q % ks), m = (int)(q / ks);
        const int row = 32 * m + (lane & 31), k = 2 * s + (lane >> 5);
        float v = 0.f;
        if (row < co) {
            if (k < 3 * kc) {
                const int tap = k / kc, c = k - tap * kc;
                if (c < ci) v = w[((size_t)row * ci + c) * 3 + tap];
            } else {
                const int c = k - 3 * kc;
                if (c < d.hidden && kp > 0) v = d.pw[(size_t)row * d.hidden + c];
            }
        }
        out[idx] = v;
    }
}

// input_fc with the NaN rule (a time step holding a NaN is zeroed before AND after the linear): H and G = gelu(H),
// (B, cp, T) with exact zeros in rows >= hidden.  One thread per (series, row < hp, t).
__global__ __launch_bounds__(256) void enc_input_kernel(const float* __restrict__ x, const float* __restrict__ fc_w,
                                                        const float* __restrict__ fc_b, float* __restrict__ H,
                                                        float* __restrict__ G, int cin, int hidden, int hp, int cp, int T) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= hp * T) return;
    const int c = idx / T, t = idx - c * T;
    float v = 0.f;
    if (c < hidden) {
        const float* xs = x + ((size_t)b * T + t) * cin;
        bool ok = true;
        float acc = fc_b[c];
        for (int k = 0; k < cin; ++k) {
            const float xv = xs[k];
            ok = ok && (xv == xv);
            acc += fc_w[c * cin + k] * xv;
        }
        v = ok ? acc : 0.f;
    }
    const size_t o = ((size_t)b * cp + c) * T + t;
    H[o] = v;
    G[o] = gelu_erf(v);
}

struct EncConvDev {
    const float* A;        // packed image of this convolution
    const float* in;       // plane read at t - d, t, t + d
    const float* raw;      // H: the residual (mode 1) / the projector's input (mode 2)
    const float* bias;     // (co)
    const float* bias2;    // (co) projector bias, mode 2
    float* out0;           // mode 0: Y = gelu(.)   mode 1: H   mode 2: the final (C, T) plane
    float* out1;           // mode 1: G = gelu(H)
    int mode, T, ntiles, cp, kc, kp, ks, co, cop, dil, tap_lo, tap_hi;
    unsigned long long waves;   // B * ntiles
};

// `steps` k steps of one tap: acc[m] += A[m tile][:, 2 s + half] * in[2 s + half][t'] for s = 0 .. steps - 1, in that order.
// p points at (row `half`, t') of the operand plane -- always a valid address; `ok` zeroes a tap outside [0, T).
template <int MT>
__device__ __forceinline__ void enc_sweep(f32x16 (&acc)[MT], const float* __restrict__ a, size_t a_tile,
                                          const float* __restrict__ p, int T, bool ok, int steps) {
    const size_t two_rows = (size_t)2 * T;
    int s = 0;
    for (; s + 4 <= steps; s += 4) {
        float av[4][MT], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bv[u] = p[(size_t)(s + u) * two_rows];
#pragma unroll
            for (int m = 0; m < MT; ++m) av[u][m] = a[(size_t)m * a_tile + (size_t)(s + u) * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma32(av[u][m], ok ? bv[u] : 0.f, acc[m]);
    }
    for (; s < steps; ++s) {
        const float bv = p[(size_t)s * two_rows];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mfma32(a[(size_t)m * a_tile + (size_t)s * 64], ok ? bv : 0.f, acc[m]);
    }
}

template <int MT>
__global__ __launch_bounds__(256) void enc_conv_kernel(const EncConvDev d) {
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const unsigned long long wid = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= d.waves) return;                                  // wave-uniform
    const int T = d.T;
    const size_t b = (size_t)(wid / (unsigned)d.ntiles);
    const int t = (int)(wid % (unsigned)d.ntiles) * 32 + (lane & 31);
    const int m0 = blockIdx.y * MT;                              // first M tile of this group
    const size_t plane = b * (size_t)d.cp * T;
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    const float* a_lane = d.A + (size_t)m0 * d.ks * 64 + lane;
    const size_t a_tile = (size_t)d.ks * 64;
    const int steps = d.kc >> 1;
    for (int tap = d.tap_lo; tap <= d.tap_hi; ++tap) {
        const int tt = t + (tap - 1) * d.dil;
        const bool ok = tt >= 0 && tt < T;
        enc_sweep<MT>(acc, a_lane + (size_t)tap * steps * 64, a_tile, d.in + plane + (size_t)half * T + (ok ? tt : 0), T, ok, steps);
    }
    if (d.kp > 0)                                                // the projector's rows: the raw stream at t
        enc_sweep<MT>(acc, a_lane + (size_t)3 * steps * 64, a_tile, d.raw + plane + (size_t)half * T + (t < T ? t : 0), T, t < T,
                      d.kp >> 1);
    if (t >= T) return;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if ((m0 + m) * 32 >= d.cop) continue;                    // a padding tile of the last group (wave-uniform)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (m0 + m) * 32 + acc_row(r, half);
            const size_t o = plane + (size_t)row * T + t;
            float v = acc[m][r];
            if (row < d.co) v += d.bias[row];
            if (d.mode == 0) {
                d.out0[o] = gelu_erf(v);
            } else if (d.mode == 1) {
                v += d.raw[o];
                d.out0[o] = v;
                d.out1[o] = gelu_erf(v);
            } else {
                if (row < d.co) v += d.bias2[row];
                d.out0[o] = v;
            }
        }
    }
}

// grid (series, 32-channel group): walks the final (C, T) plane in 32-step tiles, writes rep time-major through a
// 32 x 32 LDS transpose and keeps the running maximum over time.
__global__ __launch_bounds__(256) void enc_finish_kernel(const float* __restrict__ P, float* __restrict__ rep,
                                                         float* __restrict__ full, int cout, int cp, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.x, c0 = blockIdx.y * 32;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;      // hi in 0..7
    const float* Pb = P + ((size_t)b * cp + c0) * T;
    float mx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mx[j] = -INFINITY;
    for (int t0 = 0; t0 < T; t0 += 32) {
        const int t = t0 + lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = hi + 8 * j;                            // rows c0 + c < cp are always written planes rows
            if (t < T) {
                const float v = Pb[(size_t)c * T + t];
                mx[j] = fmaxf(mx[j], v);
                tile[c][lo] = v;
            }
        }
        if (rep != nullptr) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tr = hi + 8 * j;
                if (t0 + tr < T && c0 + lo < cout) rep[((size_t)b * T + t0 + tr) * cout + c0 + lo] = tile[lo][tr];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float m = mx[j];
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 32));
        const int c = c0 + hi + 8 * j;
        if (lo == 0 && c < cout) full[(size_t)b * cout + c] = m;
    }
}

template <int MT>
void enc_launch(const EncConvDev& d, unsigned blocks, unsigned groups, hipStream_t st) {
    enc_conv_kernel<MT><<<dim3(blocks, groups), 256, 0, st>>>(d);
}

}  // namespace
}  // namespace t2s

extern "C" uint64_t t2s_ts2vec_encode_workspace_bytes(const t2s_ts2vec_weights* w, int B, int T) {
    using namespace t2s;
    char msg[160];
    if (enc_check(w, B, T, msg, sizeof msg) != nullptr) {
        set_error("t2s_ts2vec_encode_workspace_bytes: %s", msg);
        return 0;
    }
    return enc_plan(w, B, T).total;
}

extern "C" int t2s_ts2vec_encode_long(const t2s_ts2vec_weights* w, const float* x, float* rep, float* full, int B, int T,
                                      void* workspace, uint64_t workspace_bytes, void* stream) {
    using namespace t2s;
    char msg[160];
    T2S_REQUIRE(enc_check(w, B, T, msg, sizeof msg) == nullptr, "t2s_ts2vec_encode_long: %s", msg);
    T2S_REQUIRE(x != nullptr, "t2s_ts2vec_encode_long: x must not be NULL");
    T2S_REQUIRE(full != nullptr, "t2s_ts2vec_encode_long: full must not be NULL");
    T2S_REQUIRE(w->fc_w && w->fc_b && w->proj_w && w->proj_b, "t2s_ts2vec_encode_long: NULL weight");
    for (int i = 0; i <= w->depth; ++i)
        T2S_REQUIRE(w->conv1_w[i] && w->conv1_b[i] && w->conv2_w[i] && w->conv2_b[i],
                    "t2s_ts2vec_encode_long: NULL weight of block %d", i);
    const EncPlan p = enc_plan(w, B, T);
    T2S_REQUIRE(workspace != nullptr, "t2s_ts2vec_encode_long: workspace must not be NULL (t2s_ts2vec_encode_workspace_bytes asks for %llu bytes)",
                (unsigned long long)p.total);
    T2S_REQUIRE(workspace_bytes >= p.total, "t2s_ts2vec_encode_long: workspace of %llu bytes, t2s_ts2vec_encode_workspace_bytes asks for %llu",
                (unsigned long long)workspace_bytes, (unsigned long long)p.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* packed = (float*)ws;
    float* H = (float*)(ws + p.off_h);
    float* G = (float*)(ws + p.off_g);
    float* Y = (float*)(ws + p.off_y);

    EncPackDev pk{};
    pk.pw = w->proj_w;
    pk.hidden = w->hidden;
    uint64_t biggest = 0;
    for (int j = 0; j < p.n_convs; ++j) {
        const EncConv& c = p.conv[j];
        pk.w[j] = (j & 1) ? w->conv2_w[j >> 1] : w->conv1_w[j >> 1];
        pk.ci[j] = c.ci; pk.co[j] = c.co; pk.kc[j] = c.kc; pk.kp[j] = c.kp; pk.ks[j] = c.ks; pk.mt[j] = c.mt;
        pk.off[j] = c.off;
        const uint64_t n = (uint64_t)c.mt * c.ks * 64;
        if (n > biggest) biggest = n;
    }
    enc_pack_kernel<<<dim3((unsigned)((biggest + 255) / 256), (unsigned)p.n_convs), 256, 0, st>>>(pk, packed);
    T2S_LAUNCH_CHECK();

    const int hp = up(w->hidden, 32);
    // B sits in the grid's y (< 65536 per launch): walk the batch in slabs
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        const size_t po = (size_t)b0 * p.cp * T;
        enc_input_kernel<<<dim3((unsigned)((hp * T + 255) / 256), (unsigned)nb), 256, 0, st>>>(
            x + (size_t)b0 * T * w->input_dims, w->fc_w, w->fc_b, H + po, G + po, w->input_dims, w->hidden, hp, p.cp, T);
        T2S_LAUNCH_CHECK();
    }

    const unsigned long long waves = (unsigned long long)B * p.ntiles;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    for (int j = 0; j < p.n_convs; ++j) {
        const EncConv& c = p.conv[j];
        const int blk = j >> 1;
        const bool last = blk == w->depth, second = (j & 1) != 0;
        EncConvDev d{};
        d.A = packed + c.off;
        d.in = second ? Y : G;
        d.raw = H;
        d.bias = second ? w->conv2_b[blk] : w->conv1_b[blk];
        d.bias2 = w->proj_b;
        d.mode = !second ? 0 : (last ? 2 : 1);
        d.out0 = d.mode == 0 ? Y : (d.mode == 1 ? H : G);       // the final plane lands in G: G is dead by then
        d.out1 = G;
        d.T = T; d.ntiles = p.ntiles; d.cp = p.cp; d.kc = c.kc; d.kp = c.kp; d.ks = c.ks; d.co = c.co;
        d.cop = up(c.co, 32);
        d.dil = 1 << blk;
        const bool centre_only = d.dil >= T;                    // both outer taps fall outside [0, T) for every t
        d.tap_lo = centre_only ? 1 : 0;
        d.tap_hi = centre_only ? 1 : 2;
        d.waves = waves;
        const unsigned groups = (unsigned)(c.mt / c.group);
        switch (c.group) {
            case 1: enc_launch<1>(d, blocks, groups, st); break;
            case 2: enc_launch<2>(d, blocks, groups, st); break;
            case 3: enc_launch<3>(d, blocks, groups, st); break;
            default: enc_launch<4>(d, blocks, groups, st); break;
        }
        T2S_LAUNCH_CHECK();
    }

    const unsigned cgroups = (unsigned)((w->output_dims + 31) / 32);
    for (int b0 = 0; b0 < B; b0 += 1 << 30) {
        const int nb = B - b0 < (1 << 30) ? B - b0 : (1 << 30);
        enc_finish_kernel<<<dim3((unsigned)nb, cgroups), 256, 0, st>>>(
            G + (size_t)b0 * p.cp * T, rep == nullptr ? nullptr : rep + (size_t)b0 * T * w->output_dims,
            full + (size_t)b0 * w->output_dims, w->output_dims, p.cp, T);
        T2S_LAUNCH_CHECK();
    }
    return T2S_OK;
}
