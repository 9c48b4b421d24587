// Diffusion backbones and the fused sampling loop for MI355X.
//   DDPM.p_sample / q_sample      reference model/backbone/DDPM.py:19-36
//   RectifiedFlow.euler / flow    reference model/backbone/rectified_flow.py:5-12
//   CFG loop                      reference infer.py:75-95
// One sampling step (2B-sequence DiT forward + CFG combine + sampler update) is captured once
// into a hipGraph and replayed `steps` times; everything that changes from step to step
// (time-embedding row, DDPM coefficients, noise stream / injected-noise slice) is looked up on
// the device through a step counter that the last node of the graph advances.  With a guided window short of the loop
// (t2s_sampler_set_guided_steps) the steps outside it run the conditional pass alone: a step of a second kind, StepKind.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <stdlib.h>
#include <vector>

#include "t2s_dit_internal.h"

struct t2s_vae;

namespace t2s {

// ---------------------------------------------------------------- Philox4x32-10 (t2s_common.h) + Box-Muller
// 4 N(0,1) draws for quad `quad` of global row `row` in stream `stream_id`
__device__ __forceinline__ f32x4 normal4(uint64_t seed, uint32_t stream_id, uint32_t row, uint32_t quad) {
    const u32x4 r = philox4x32_10(u32x4{quad, row, stream_id, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float two_pi = 6.283185307179586f;
    const float two_m24 = 1.0f / 16777216.0f;
    // 24-bit uniforms (exact in fp32): u1 in (0,1], u2 in [0,1)
    const float u1a = ((float)(r.x >> 8) + 1.0f) * two_m24;
    const float u1b = ((float)(r.z >> 8) + 1.0f) * two_m24;
    const float u2a = (float)(r.y >> 8) * two_m24;
    const float u2b = (float)(r.w >> 8) * two_m24;
    const float ra = sqrtf(-2.0f * logf(u1a));
    const float rb = sqrtf(-2.0f * logf(u1b));
    f32x4 z;
    z.x = ra * cosf(two_pi * u2a);
    z.y = ra * sinf(two_pi * u2a);
    z.z = rb * cosf(two_pi * u2b);
    z.w = rb * sinf(two_pi * u2b);
    return z;
}

__global__ void philox_normal_kernel(float* __restrict__ out, uint64_t seed, uint32_t stream_id,
                                     uint32_t row0, int n_rows, int quads_per_row) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * quads_per_row) return;
    const int row = idx / quads_per_row, quad = idx - row * quads_per_row;
    reinterpret_cast<f32x4*>(out)[idx] = normal4(seed, stream_id, row0 + (uint32_t)row, (uint32_t)quad);
}

// the same draws with a key and a key row per row: row r of out = row key_rows[r] of stream `stream_id` under seeds[r]
__global__ void philox_normal_rows_kernel(float* __restrict__ out, const uint64_t* __restrict__ seeds,
                                          const uint32_t* __restrict__ key_rows, uint32_t stream_id, int n_rows,
                                          int quads_per_row) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * quads_per_row) return;
    const int row = idx / quads_per_row, quad = idx - row * quads_per_row;
    reinterpret_cast<f32x4*>(out)[idx] = normal4(seeds[row], stream_id, key_rows[row], (uint32_t)quad);
}

// U[0,1) draws of the same counter layout: element e of global row `row` = lane e % 4 of counter (e / 4, row, stream_id);
// 24-bit uniforms (exact in fp32, never 1.0)
__global__ void philox_uniform_kernel(float* __restrict__ out, uint64_t seed, uint32_t stream_id, uint32_t row0, int n_rows,
                                      int row_elems) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * row_elems) return;
    const int row = idx / row_elems, e = idx - row * row_elems;
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)(e >> 2), row0 + (uint32_t)row, stream_id, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t v = (e & 3) == 0 ? r.x : ((e & 3) == 1 ? r.y : ((e & 3) == 2 ? r.z : r.w));
    out[idx] = (float)(v >> 8) * (1.0f / 16777216.0f);
}

// ---------------------------------------------------------------- sampler update kernels
// A lane's loop state on the device.  set_step_kernel writes it at the start of a run, every kernel of a step reads its loop
// index from it (the DiT kernels through a const int* to `index`, which therefore stays the first member) and the last
// workgroup of the update kernel advances it.  All of it is read on the device, so one captured graph serves every step,
// every shard position and runs with or without per-row tables.
struct LoopState {
    int index;      // loop index j
    int row0;       // global row of the lane's first series (Philox key)
    int arrivals;   // arrival counter of the update kernel (advance_step_when_last)
    int rows;       // ROWS_* bits: the per-row tables this run uses (t2s_sampler_set_rows)
};
static_assert(offsetof(LoopState, index) == 0 && sizeof(LoopState) == 16, "the DiT kernels read LoopState::index through an int*");
constexpr int LANE_STATES = 4;   // LoopStates from one lane's to the next: 64 bytes apart
constexpr int ROWS_SEED = 1, ROWS_KEY = 2, ROWS_CFG = 4;

// What every update kernel takes: the sampling loop's (loop != NULL) and the stand-alone C entries' (loop == NULL) alike.
struct UpdateArgs {
    float* x;             // (B,1920) in place
    float* hist;          // (B,1920) in place; LMS only
    const float* pred_u;  // (B,1920)
    const float* pred_c;  // (B,1920) or NULL
    const float* noise;   // injected draws: (steps,noise_rows,1920) indexed by step (this shard's first row), or (B,1920)
                          // if loop NULL; NULL: Philox
    const float* coef;    // DEVICE (T,3) DDPM by timestep, (S,6) LMS by loop index
    const LoopState* loop;   // the lane's loop state, or NULL: then index / stream_id / row0 below are immediate
    int index;            // loop NULL: the coefficient row (DDPM: t_index; LMS: loop index)
    int steps;            // DDPM in the loop: T (t = steps-1-j)
    float cfg;
    float dt;             // RF
    uint64_t seed;
    uint32_t stream_id;
    uint32_t row0;
    int B;
    int qpr;              // quads (float4) per row: 64 W / 4 of the (64, W) latent -- 480 at W = 30
    int noise_rows;       // rows per step of the injected-noise array (>= B: a lane steps a row range of the batch)
    LoopState* advance;   // sampling loop: the last workgroup increments the lane's loop index (advance_step_when_last)
    // per-row tables (t2s_sampler_set_rows), this lane's slice: used where bit ROWS_SEED / ROWS_KEY / ROWS_CFG of loop->rows
    // is set; NULL outside the sampler
    const uint64_t* row_seed;
    const uint32_t* row_key;
    const float* row_cfg;
};

// Last workgroup to finish advances the device loop index: every workgroup has read it before it arrives, so the
// increment cannot overtake a reader, and the stand-alone one-thread set_step launch per step (4 us of a 690 us step at
// 32 series) is gone.
__device__ __forceinline__ void advance_step_when_last(LoopState* loop) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&loop->arrivals, 1) == (int)gridDim.x - 1) {
            loop->arrivals = 0;
            loop->index += 1;
        }
    }
}

// The prologue: where this launch stands.  In the loop everything comes from the lane's state: the draw of loop index j is
// stream j, and the injected noise of step j is slice j.
struct Step {
    int index;            // loop index j (stand-alone: UpdateArgs::index)
    uint32_t stream_id, row0;
    int rows;             // ROWS_* bits
    const float* noise;
};
__device__ __forceinline__ Step resolve_step(const UpdateArgs& a) {
    Step s{a.index, a.stream_id, a.row0, 0, a.noise};
    if (a.loop) {
        s.index = a.loop->index;
        s.row0 = (uint32_t)a.loop->row0;
        s.rows = a.loop->rows;
        s.stream_id = (uint32_t)s.index;
        if (s.noise) s.noise += (size_t)s.index * a.noise_rows * a.qpr * 4;
    }
    return s;
}

// An Update is built once per thread from the arguments and the loop index (it picks its coefficient row), says which
// operands it needs -- reads_h / draws / writes_h, launch-uniform -- and maps one quad: x, u, c (guided: pred_c given, with
// the row's guidance scale), h, z -> the new x (returned) and the new h.  Operands it did not ask for hold placeholders.
// The arithmetic of each is fixed: results repeat bit for bit.

// DDPM.p_sample: x' = c0 * (x - c1 * pred) + c2 * z with the coefficient row of timestep t
struct DdpmUpdate {
    float c0, c1, c2;
    __device__ DdpmUpdate(const UpdateArgs& a, int j) {
        const int t = a.loop ? a.steps - 1 - j : j;
        c0 = a.coef[t * 3 + 0], c1 = a.coef[t * 3 + 1], c2 = a.coef[t * 3 + 2];
    }
    __device__ bool reads_h() const { return false; }
    __device__ bool draws() const { return true; }
    __device__ bool writes_h() const { return false; }
    __device__ f32x4 operator()(f32x4 x, f32x4 u, f32x4 c, bool guided, float scale, f32x4, f32x4 z, f32x4&) const {
        f32x4 pred = u;
        if (guided) pred = u + scale * (c - u);
        const f32x4 mean = c0 * (x - c1 * pred);
        return mean + c2 * z;
    }
};

// RectifiedFlow.euler: x' = x + pred * dt
struct RfUpdate {
    float dt;
    __device__ RfUpdate(const UpdateArgs& a, int) : dt(a.dt) {}
    __device__ bool reads_h() const { return false; }
    __device__ bool draws() const { return false; }
    __device__ bool writes_h() const { return false; }
    __device__ f32x4 operator()(f32x4 x, f32x4 u, f32x4 c, bool guided, float scale, f32x4, f32x4, f32x4&) const {
        f32x4 pred = u;
        if (guided) pred = u + scale * (c - u);
        return x + pred * dt;
    }
};

// Linear multistep update (DDIM, DPM-Solver++(2M), AB2): one table-driven update for every few-step solver, per element
//   x' = c0 * x + c1 * pred + c2 * h + c3 * z        h' = c4 * x + c5 * pred   (from the OLD x)
// coef row j = {c0 .. c5} belongs to LOOP INDEX j (not steps-1-j: the solver's grid is in t_values, the table follows the
// loop).  A coefficient that is exactly 0 means its operand is not touched -- c2 == 0: h is not loaded (NaN / uninitialised
// history on the first step is fine); c3 == 0: no draw, no Philox work, noise may be NULL; c4 == c5 == 0: h is not
// written.  The coefficients are launch-uniform, so are the branches.
// Arithmetic: the fp32 operands are widened, the update is evaluated in fp64 in the order
// pred = fma(cfg, c - u, u); acc = c0 * x; acc = fma(c1, pred, acc); acc = fma(c2, h, acc); acc = fma(c3, z, acc);
// hn = fma(c5, pred, c4 * x), and acc / hn are rounded to fp32 ONCE.  Why fp64: the x0-prediction history of DPM-Solver++ is
// (x - s * eps) / a with 1 / a = 157 at t = 999 of the 1000-step schedule -- two large terms that cancel -- and a four-term
// fp32 sum carries four roundings of partial sums larger than its result; the kernel is bound by its four to seven
// (B,1920) streams, the ~40 fp64 operations per quad do not show (tools/solver_probe.py).
struct LmsUpdate {
    float c0, c1, c2, c3, c4, c5;
    __device__ LmsUpdate(const UpdateArgs& a, int j) {
        const float* cj = a.coef + (size_t)j * 6;
        c0 = cj[0], c1 = cj[1], c2 = cj[2], c3 = cj[3], c4 = cj[4], c5 = cj[5];
    }
    __device__ bool reads_h() const { return c2 != 0.0f; }
    __device__ bool draws() const { return c3 != 0.0f; }
    __device__ bool writes_h() const { return c4 != 0.0f || c5 != 0.0f; }
    __device__ f32x4 operator()(f32x4 x, f32x4 u, f32x4 c, bool guided, float scale, f32x4 h, f32x4 z, f32x4& hn) const {
        const double cfg = (double)scale;
        f32x4 xn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double pred = (double)u[e];
            if (guided) pred = fma(cfg, (double)c[e] - (double)u[e], pred);
            double acc = (double)c0 * (double)x[e];
            acc = fma((double)c1, pred, acc);
            if (reads_h()) acc = fma((double)c2, (double)h[e], acc);
            if (draws()) acc = fma((double)c3, (double)z[e], acc);
            xn[e] = (float)acc;
            hn[e] = (float)fma((double)c5, pred, (double)c4 * (double)x[e]);
        }
        return xn;
    }
};

// The scaffold of every update: prologue, grid-stride loop over the quads (one float4 at a time), the operands of a quad,
// the Update's arithmetic, and the loop's advance.
constexpr int STEP_MAX_WGS = 96;   // see launch_update
template <class Update>
__global__ __launch_bounds__(256) void update_kernel(const UpdateArgs a) {
    const int QPR = a.qpr;
    const Step s = resolve_step(a);
    const Update update(a, s.index);
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < a.B * QPR; idx += gridDim.x * blockDim.x) {
        const int row = idx / QPR;
        const f32x4 x = reinterpret_cast<const f32x4*>(a.x)[idx];
        const f32x4 u = reinterpret_cast<const f32x4*>(a.pred_u)[idx];
        f32x4 c = u, h = x, z = x;                   // (placeholders where the operand is not read)
        float scale = 0.0f;
        if (a.pred_c) {
            c = reinterpret_cast<const f32x4*>(a.pred_c)[idx];
            scale = (s.rows & ROWS_CFG) ? a.row_cfg[row] : a.cfg;
        }
        if (update.reads_h()) h = reinterpret_cast<const f32x4*>(a.hist)[idx];
        if (update.draws()) {
            if (s.noise) {
                z = reinterpret_cast<const f32x4*>(s.noise)[idx];
            } else {
                const int quad = idx - row * QPR;
                const uint64_t seed = (s.rows & ROWS_SEED) ? a.row_seed[row] : a.seed;
                const uint32_t key = (s.rows & ROWS_KEY) ? a.row_key[row] : s.row0 + (uint32_t)row;
                z = normal4(seed, s.stream_id, key, (uint32_t)quad);
            }
        }
        f32x4 hn;
        const f32x4 xn = update(x, u, c, a.pred_c != nullptr, scale, h, z, hn);
        if (update.writes_h()) reinterpret_cast<f32x4*>(a.hist)[idx] = hn;
        reinterpret_cast<f32x4*>(a.x)[idx] = xn;
    }
    if (a.advance) advance_step_when_last(a.advance);
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ eps,
                                                       const int32_t* __restrict__ t, const float* __restrict__ sab,
                                                       const float* __restrict__ s1m, float* __restrict__ out, int B,
                                                       int QPR, int T) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * QPR) return;
    const int tt = t[idx / QPR];
    if (tt < 0 || tt >= T) {      // the reference's gather raises (DDPM.py:7-9): no table read, a loud NaN row
        reinterpret_cast<f32x4*>(out)[idx] = f32x4{NAN, NAN, NAN, NAN};
        return;
    }
    const f32x4 a = reinterpret_cast<const f32x4*>(x0)[idx];
    const f32x4 e = reinterpret_cast<const f32x4*>(eps)[idx];
    reinterpret_cast<f32x4*>(out)[idx] = sab[tt] * a + s1m[tt] * e;
}

__global__ __launch_bounds__(256) void create_flow_kernel(const float* __restrict__ x1, const float* __restrict__ x0,
                                                          const float* __restrict__ t, float* __restrict__ out, int B) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int QPR = LAT / 4;
    if (idx >= B * QPR) return;
    const float tt = t[idx / QPR];
    const f32x4 a = reinterpret_cast<const f32x4*>(x1)[idx];
    const f32x4 b = reinterpret_cast<const f32x4*>(x0)[idx];
    reinterpret_cast<f32x4*>(out)[idx] = tt * a + (1.0f - tt) * b;
}

// DDPM.p_sample with a per-row timestep (the class API allows t to differ per row), out of place
__global__ __launch_bounds__(256) void p_sample_rows_kernel(const float* __restrict__ xt, const float* __restrict__ eh,
                                                            const int32_t* __restrict__ t, const float* __restrict__ noise,
                                                            const float* __restrict__ coef, float* __restrict__ out, int B,
                                                            int QPR, int T) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * QPR) return;
    const int tt = t[idx / QPR];
    if (tt < 0 || tt >= T) {
        reinterpret_cast<f32x4*>(out)[idx] = f32x4{NAN, NAN, NAN, NAN};
        return;
    }
    const float c0 = coef[tt * 3 + 0], c1 = coef[tt * 3 + 1], c2 = coef[tt * 3 + 2];
    const f32x4 x = reinterpret_cast<const f32x4*>(xt)[idx];
    const f32x4 e = reinterpret_cast<const f32x4*>(eh)[idx];
    const f32x4 z = reinterpret_cast<const f32x4*>(noise)[idx];
    reinterpret_cast<f32x4*>(out)[idx] = c0 * (x - c1 * e) + c2 * z;
}

// F.mse_loss (mean over all elements), deterministic and STATELESS: stage 1, every workgroup sums a fixed contiguous
// chunk in a fixed order into part[blockIdx.x] of the CALLER's scratch; stage 2, one workgroup adds the partials in index
// order.  No device globals, no arrival counter, nothing to zero: calls on different streams / from different threads
// cannot meet (until round 5 the partials lived in one __device__ array per device and two overlapping calls raced
// silently).
constexpr int MSE_MAX_WGS = 1024;
static_assert(MSE_MAX_WGS <= T2S_MSE_SCRATCH_FLOATS, "t2s.h: T2S_MSE_SCRATCH_FLOATS too small");
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ part_out, size_t n) {
    __shared__ float part[4];
    const size_t n4 = n >> 2;
    const size_t per = (n4 + gridDim.x - 1) / gridDim.x;          // float4 per workgroup
    const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
    float acc = 0.f;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
        const f32x4 d = reinterpret_cast<const f32x4*>(a)[i] - reinterpret_cast<const f32x4*>(b)[i];
        acc += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
    if (blockIdx.x == gridDim.x - 1)                                // ragged tail (n % 4 elements)
        for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            const float d = a[i] - b[i];
            acc += d * d;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part_out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void mse_final_kernel(const float* __restrict__ part_in, int n_part, float* __restrict__ out,
                                                        size_t n) {
    __shared__ float part[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n_part; i += 256) s += part_in[i];      // fixed assignment, fixed order below
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((part[0] + part[1]) + (part[2] + part[3])) / (float)n;
}

__global__ void set_step_kernel(LoopState* loop, int value, uint32_t row0, int rows) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *loop = LoopState{value, (int)row0, 0, rows};
}

}  // namespace t2s

using namespace t2s;

// The one launch of an update kernel, mode = T2S_MODE_*.  Grid rule: a workgroup per 256 quads, capped at STEP_MAX_WGS
// (the rest by grid stride) exactly when the kernel advances the loop: the arrival counter is ONE address, and same-address
// atomics serialise at ~25 ns each -- 480 of them (one per 256 quads at B = 256) made this 6 us kernel 18 us.  The result
// of a quad does not depend on the grid.
static int launch_update(int mode, const UpdateArgs& a, hipStream_t st) {
    const int wgs = (a.B * a.qpr + 255) / 256;
    const int grid = (a.advance && wgs > STEP_MAX_WGS) ? STEP_MAX_WGS : wgs;
    switch (mode) {
    case T2S_MODE_DDPM: update_kernel<DdpmUpdate><<<grid, 256, 0, st>>>(a); break;
    case T2S_MODE_LMS: update_kernel<LmsUpdate><<<grid, 256, 0, st>>>(a); break;
    case T2S_MODE_RF: update_kernel<RfUpdate><<<grid, 256, 0, st>>>(a); break;
    default: T2S_REQUIRE(false, "launch_update: mode=%d", mode);
    }
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// ---------------------------------------------------------------- C ABI: single-step entry points
extern "C" int t2s_philox_normal(float* out, uint64_t seed, uint32_t stream_id, uint32_t row0, int n_rows,
                                 int row_elems, void* stream) {
    T2S_REQUIRE(out && n_rows > 0 && row_elems > 0 && row_elems % 4 == 0,
                "t2s_philox_normal: bad argument (n_rows=%d,row_elems=%d; row_elems %% 4 must be 0)", n_rows, row_elems);
    const int q = row_elems / 4, total = n_rows * q;
    philox_normal_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(out, seed, stream_id, row0, n_rows, q);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_philox_normal_rows(float* out, const uint64_t* seeds, const uint32_t* key_rows, uint32_t stream_id,
                                      int n_rows, int row_elems, void* stream) {
    T2S_REQUIRE(out && seeds && key_rows && n_rows > 0 && row_elems > 0 && row_elems % 4 == 0 &&
                    (long long)n_rows * row_elems < (1ll << 31),
                "t2s_philox_normal_rows: bad argument (n_rows=%d,row_elems=%d; row_elems %% 4 must be 0)", n_rows, row_elems);
    const int q = row_elems / 4, total = n_rows * q;
    philox_normal_rows_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(out, seeds, key_rows, stream_id, n_rows, q);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_philox_uniform(float* out, uint64_t seed, uint32_t stream_id, uint32_t row0, int n_rows, int row_elems,
                                  void* stream) {
    T2S_REQUIRE(out && n_rows > 0 && row_elems > 0 && (long long)n_rows * row_elems < (1ll << 31),
                "t2s_philox_uniform: bad argument (n_rows=%d,row_elems=%d)", n_rows, row_elems);
    const int total = n_rows * row_elems;
    philox_uniform_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(out, seed, stream_id, row0, n_rows, row_elems);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_ddpm_step(float* x, const float* eps_u, const float* eps_c, const float* noise,
                             const float* coef, int t_index, float cfg, uint64_t seed, uint32_t stream_id,
                             uint32_t row0, int B, void* stream) {
    T2S_REQUIRE(x && eps_u && coef, "t2s_ddpm_step: NULL argument");
    T2S_REQUIRE(B > 0 && t_index >= 0 && (long long)B * LAT < (1ll << 31), "t2s_ddpm_step: B=%d t_index=%d", B, t_index);
    UpdateArgs a{};
    a.x = x; a.pred_u = eps_u; a.pred_c = eps_c; a.noise = noise; a.coef = coef;
    a.index = t_index; a.cfg = cfg; a.seed = seed; a.stream_id = stream_id; a.row0 = row0; a.B = B; a.qpr = LAT / 4;
    return launch_update(T2S_MODE_DDPM, a, (hipStream_t)stream);
}

extern "C" int t2s_lms_step_n(float* x, float* hist, const float* pred_u, const float* pred_c, const float* noise,
                              const float* coef, int index, float cfg, uint64_t seed, uint32_t stream_id, uint32_t row0, int B,
                              int row_elems, void* stream) {
    T2S_REQUIRE(x && hist && pred_u && coef, "t2s_lms_step: NULL argument");
    T2S_REQUIRE(row_elems > 0 && row_elems % 4 == 0, "t2s_lms_step: row_elems=%d must be a positive multiple of 4", row_elems);
    T2S_REQUIRE(B > 0 && index >= 0 && (long long)B * row_elems < (1ll << 31), "t2s_lms_step: B=%d index=%d", B, index);
    UpdateArgs a{};
    a.x = x; a.hist = hist; a.pred_u = pred_u; a.pred_c = pred_c; a.noise = noise; a.coef = coef;
    a.index = index; a.cfg = cfg; a.seed = seed; a.stream_id = stream_id; a.row0 = row0; a.B = B; a.qpr = row_elems / 4;
    return launch_update(T2S_MODE_LMS, a, (hipStream_t)stream);
}

extern "C" int t2s_lms_step(float* x, float* hist, const float* pred_u, const float* pred_c, const float* noise,
                            const float* coef, int index, float cfg, uint64_t seed, uint32_t stream_id, uint32_t row0, int B,
                            void* stream) {
    return t2s_lms_step_n(x, hist, pred_u, pred_c, noise, coef, index, cfg, seed, stream_id, row0, B, LAT, stream);
}

extern "C" int t2s_rf_step(float* x, const float* v_u, const float* v_c, float cfg, float dt, int B, void* stream) {
    T2S_REQUIRE(x && v_u, "t2s_rf_step: NULL argument");
    T2S_REQUIRE(B > 0 && (long long)B * LAT < (1ll << 31), "t2s_rf_step: B=%d", B);
    UpdateArgs a{};
    a.x = x; a.pred_u = v_u; a.pred_c = v_c; a.cfg = cfg; a.dt = dt; a.B = B; a.qpr = LAT / 4;
    return launch_update(T2S_MODE_RF, a, (hipStream_t)stream);
}

extern "C" int t2s_ddpm_q_sample_n(const float* x0, const float* eps, const int32_t* t, const float* sqrt_ab,
                                   const float* sqrt_1mab, float* out, int B, int row_elems, int n_steps, void* stream) {
    T2S_REQUIRE(x0 && eps && t && sqrt_ab && sqrt_1mab && out && B > 0 && n_steps > 0, "t2s_ddpm_q_sample: bad argument");
    T2S_REQUIRE(row_elems > 0 && row_elems % 4 == 0, "t2s_ddpm_q_sample: row_elems=%d must be a positive multiple of 4", row_elems);
    const int total = B * (row_elems / 4);
    q_sample_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(x0, eps, t, sqrt_ab, sqrt_1mab, out, B, row_elems / 4, n_steps);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_ddpm_q_sample(const float* x0, const float* eps, const int32_t* t, const float* sqrt_ab,
                                 const float* sqrt_1mab, float* out, int B, int n_steps, void* stream) {
    return t2s_ddpm_q_sample_n(x0, eps, t, sqrt_ab, sqrt_1mab, out, B, LAT, n_steps, stream);
}

extern "C" int t2s_ddpm_p_sample_n(const float* xt, const float* eps_hat, const int32_t* t, const float* noise,
                                   const float* coef, float* out, int B, int row_elems, int n_steps, void* stream) {
    T2S_REQUIRE(xt && eps_hat && t && noise && coef && out && B > 0 && n_steps > 0, "t2s_ddpm_p_sample: bad argument");
    T2S_REQUIRE(row_elems > 0 && row_elems % 4 == 0, "t2s_ddpm_p_sample: row_elems=%d must be a positive multiple of 4", row_elems);
    const int total = B * (row_elems / 4);
    p_sample_rows_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(xt, eps_hat, t, noise, coef, out, B, row_elems / 4, n_steps);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

extern "C" int t2s_ddpm_p_sample(const float* xt, const float* eps_hat, const int32_t* t, const float* noise,
                                 const float* coef, float* out, int B, int n_steps, void* stream) {
    return t2s_ddpm_p_sample_n(xt, eps_hat, t, noise, coef, out, B, LAT, n_steps, stream);
}

extern "C" int t2s_mse_ws(const float* a, const float* b, float* out, uint64_t n, float* scratch, void* stream) {
    T2S_REQUIRE(a && b && out && scratch && n > 0, "t2s_mse_ws: bad argument");
    const size_t n4 = n / 4;
    const int wgs = (int)(n4 / 1024 < 1 ? 1 : (n4 / 1024 > MSE_MAX_WGS ? MSE_MAX_WGS : n4 / 1024));   // >= 4 float4 per thread
    mse_partial_kernel<<<wgs, 256, 0, (hipStream_t)stream>>>(a, b, scratch, (size_t)n);
    T2S_LAUNCH_CHECK();
    mse_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(scratch, wgs, out, (size_t)n);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// t2s_mse keeps its scratch-free signature: the library lends one scratch per (device, stream), allocated the first time that
// stream calls (so: not capturable THEN; later calls on the stream are).  Calls on one stream are ordered by the stream,
// calls on different streams use different scratch.
extern "C" int t2s_mse(const float* a, const float* b, float* out, uint64_t n, void* stream) {
    T2S_REQUIRE(a && b && out && n > 0, "t2s_mse: bad argument");
    static std::mutex guard;
    static std::vector<std::pair<std::pair<int, void*>, float*>> lent;
    int dev = 0;
    T2S_HIP_CHECK(hipGetDevice(&dev));
    float* scratch = nullptr;
    {
        std::lock_guard<std::mutex> lock(guard);
        for (auto& e : lent)
            if (e.first.first == dev && e.first.second == stream) scratch = e.second;
        if (!scratch) {
            T2S_HIP_CHECK(hipMalloc((void**)&scratch, T2S_MSE_SCRATCH_FLOATS * sizeof(float)));
            lent.push_back({{dev, stream}, scratch});
        }
    }
    return t2s_mse_ws(a, b, out, n, scratch, stream);
}

extern "C" int t2s_rf_create_flow(const float* x1, const float* x0, const float* t, float* out, int B, void* stream) {
    T2S_REQUIRE(x1 && x0 && t && out && B > 0, "t2s_rf_create_flow: bad argument");
    const int total = B * (LAT / 4);
    create_flow_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(x1, x0, t, out, B);
    T2S_LAUNCH_CHECK();
    return T2S_OK;
}

// ---------------------------------------------------------------- fused sampling loop
struct t2s_sampler {
    int lat = LAT;                // elements of a latent row: 64 W, W = t2s_dit_latent_w(dit)
    t2s_dit* dit = nullptr;
    t2s_vae* vae = nullptr;
    t2s_sample_config cfg{};
    float* temb_table = nullptr;  // (steps,128)
    float* coef = nullptr;        // (steps,3)  DDPM; (steps,6) by LOOP INDEX in T2S_MODE_LMS
    float* hist = nullptr;        // (B,1920)   T2S_MODE_LMS: the solver's history (x0_prev / v_prev), sliced by rows per lane
    float* eps_u = nullptr;       // (B,1920)
    float* eps_c = nullptr;
    float* tvals = nullptr;       // (steps)
    float* mod_table = nullptr;   // (steps, batch + 1, 3072): the adaLN modulation of every step, refreshed at the start of a run
    LoopState* step = nullptr;    // device loop states, one per lane (LANE_STATES apart)
    // Lanes: the rows of the batch are independent through the whole loop, so the batch can run as TWO half
    // batches, each a complete chain (own step counter, own hipGraph, own slice of the DiT workspace) on its own
    // stream, joined only before the decode.  One chain alone drains and refills the chip at each of its 9 kernel
    // boundaries per pass and the row-chain kernel quantises to 7.5 tiles per SIMD at 512 sequences; the other
    // lane's kernels fill those holes.  Results are bitwise those of one lane (batch-invariant kernels).
    int lanes_req = 0;            // 0 = automatic, 1 .. MAX_LANES (t2s_sampler_set_lanes)
    int lanes_cap = 0;            // lanes the graphs below were captured for
    int whole_req = -1;           // t2s_sampler_set_loop_graph: 1 = the WHOLE loop is one graph per lane, 0 = one step, -1 = default
    int whole_cap = 0;            // what the graphs below hold
    static constexpr int MAX_LANES = 4;
    // Guided window [guide_first, guide_end) in loop indices (t2s_sampler_set_guided_steps): step j inside it is the CFG step
    // (kind STEP_GUIDED), any other step ONE conditional pass over the lane's rows whose output is pred (STEP_COND).  The
    // default (0, steps) guides every step.
    int guide_first = 0, guide_end = 0;
    // graph[k][l]: whole-loop form, k = 0 holds lane l's loop (each step enqueued with its kind); one-step form, k = the
    // step's kind -- only the kinds the window needs are captured, and the host replays the one that step j needs
    static constexpr int KINDS = 2;
    hipGraph_t graph[KINDS][MAX_LANES] = {};
    hipGraphExec_t exec[KINDS][MAX_LANES] = {};
    hipStream_t side[MAX_LANES] = {};          // lanes 1 .. (index 0 unused: lane 0 runs on the caller's stream); BORROWED
                                               // from the per-device pool below, never destroyed by a sampler
    hipEvent_t ev_fork = nullptr, ev_join[MAX_LANES] = {};
    // Runs with more than one lane -- and graph runs on the default stream (stream == NULL at the C ABI), which cannot be
    // captured -- go through the library's pooled streams (lane 0 on pool stream 0), forked from and joined to the
    // caller's stream by events inside the call
    hipStream_t own = nullptr;    // borrowed from the pool
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // pointers the captured graphs were built for
    float* g_x = nullptr;
    const float* g_text = nullptr;
    const float* g_noise = nullptr;
    // Per-row tables (t2s_sampler_set_rows): `rows` = the ROWS_* bits in use; the host copy `h_rows` (seeds, key rows, cfg
    // of every batch row, in the device layout) is uploaded at the next run when `rows_dirty`, through the pinned staging
    // buffer `h_stage` on the run's stream -- which the next upload reuses only after `ev_rows` says the copy has read it
    int rows = 0;
    bool rows_dirty = false;
    std::vector<unsigned char> h_rows;
    void* h_stage = nullptr;
    void* d_rows = nullptr;       // (batch) u64 seeds | (batch) u32 key rows | (batch) f32 cfg
    hipEvent_t ev_rows = nullptr;
    bool ev_rows_recorded = false;
    // Per-row series lengths (t2s_sampler_set_lengths): the host copy `h_len` = (batch + 1) u64 offsets | (batch) i32 lengths,
    // staged behind the row tables in the same pinned buffer and the same device buffer, uploaded the same way
    bool ragged = false, len_dirty = false;
    std::vector<unsigned char> h_len;
};

namespace {
inline size_t rows_bytes(int batch) { return (size_t)batch * (sizeof(uint64_t) + sizeof(uint32_t) + sizeof(float)); }
inline uint64_t* rows_seed(void* base, int batch) { (void)batch; return (uint64_t*)base; }
inline uint32_t* rows_key(void* base, int batch) { return (uint32_t*)((uint64_t*)base + batch); }
inline float* rows_cfg(void* base, int batch) { return (float*)(rows_key(base, batch) + batch); }
// behind the row tables (rows_bytes is a multiple of 8)
inline size_t len_bytes(int batch) { return (size_t)(batch + 1) * sizeof(uint64_t) + (size_t)batch * sizeof(int32_t); }
inline uint64_t* len_offsets(void* base) { return (uint64_t*)base; }
inline int32_t* len_lengths(void* base, int batch) { return (int32_t*)((uint64_t*)base + batch + 1); }
}  // namespace

namespace {

// The lanes' streams come from ONE pool per device, created together the first time a sampler needs it.  HIP maps
// streams onto a few hardware queues (four by default) in creation order, and two lanes whose streams share a queue run
// one after the other: with a capture stream per Sampler object (the Python wrapper's, then) lane 0 landed on lane 1's
// queue for every fourth sampler a process built -- 52 instead of 61 series/s at 64 series, 58 instead of 62 at 96,
// reproducibly by construction order (tools/strong_probe.py).  Four streams created back to back take four different
// queues, and because lane 0 runs on pool stream 0 too, the caller's stream -- whatever queue it sits on -- only carries
// the fork and the join ...  (GPU_MAX_HW_QUEUES=8 / 16 did not help and cost 3-5 % at 128 / 256.)
// ... in THEORY: measured, pool streams 0 and 2 of four created back to back still shared a queue (96 series as three
// lanes: 57.9 against 62.3 series/s).  So the pool is CALIBRATED once per device: a 400 us spin kernel on each of two
// streams tells whether they overlap (the second started before the first ended); candidates are created until four
// mutually concurrent streams are found (at most 12 candidates, ~10-40 ms once per process).
__global__ void spin_kernel(unsigned long long ticks, unsigned long long* stamp) {
    const unsigned long long t0 = wall_clock64();      // constant 100 MHz
    if (threadIdx.x == 0) stamp[0] = t0;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (threadIdx.x == 0) stamp[1] = wall_clock64();
}

bool streams_overlap(hipStream_t a, hipStream_t b, unsigned long long* stamps_dev) {
    // 400 us spins, and a second look before a pair is declared serial: the test needs the host to issue the second launch
    // while the first kernel still runs, and on a node where eight ranks calibrate at once a host hiccup of 100 us would
    // have rejected a perfectly concurrent pair (the lane then shares a queue: correct, but the lanes no longer overlap)
    for (int attempt = 0; attempt < 2; ++attempt) {
        unsigned long long h[4] = {0, 0, 0, 0};
        spin_kernel<<<1, 64, 0, a>>>(40000ull, stamps_dev);          // 400 us at the 100 MHz wall clock
        spin_kernel<<<1, 64, 0, b>>>(40000ull, stamps_dev + 2);
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
        // (read back on stream a, not with a legacy-stream hipMemcpy: see t2s_sampler_create)
        if (hipMemcpyAsync(h, stamps_dev, sizeof(h), hipMemcpyDeviceToHost, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return false;
        if (h[2] < h[1] && h[0] < h[3]) return true;
    }
    return false;
}

int g_lane_pool_concurrent[16] = {};      // per device: mutually concurrent streams the calibration found

// The pool is shared by every sampler of the process on a device, lane 0 included: two host threads driving two samplers
// would capture, record events and launch graphs on the SAME streams at once (one thread's work pulled into the other's
// capture, or hipErrorStreamCaptureIsolation).  A run that uses pool streams holds this lock from its first event to its
// join: the enqueue of a run is host work of a few ms, the GPU side stays asynchronous.
std::recursive_mutex g_pool_use[16];     // recursive: a failing t2s_sampler_create destroys its half-built sampler under the lock

// one non-blocking stream per device for the library's own set-up work (t2s_sampler_create); see there
hipStream_t setup_stream(int dev) {
    static hipStream_t st[16] = {};
    static std::mutex guard;
    std::lock_guard<std::mutex> lock(guard);
    if (dev < 0 || dev >= 16) return nullptr;
    if (!st[dev] && hipStreamCreateWithFlags(&st[dev], hipStreamNonBlocking) != hipSuccess) {
        st[dev] = nullptr;
        (void)hipGetLastError();
    }
    return st[dev];
}

hipStream_t* lane_streams() {
    constexpr int ML = t2s_sampler::MAX_LANES;
    static hipStream_t pool[16][ML] = {};
    static bool ready[16] = {}, failed[16] = {};
    static std::mutex guard;                    // the pool is process-wide: samplers of different threads may meet here
    std::lock_guard<std::mutex> lock(guard);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (ready[dev]) return pool[dev];
    if (failed[dev]) return nullptr;            // calibrated once per process: a device without streams stays on one lane
    unsigned long long* stamps = nullptr;
    if (hipMalloc((void**)&stamps, 4 * sizeof(unsigned long long)) != hipSuccess) return nullptr;
    int have = 0;
    hipStream_t spare[12] = {};
    int n_spare = 0;
    for (int c = 0; c < 12 && have < ML; ++c) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) break;
        bool ok = true;
        for (int l = 0; l < have && ok; ++l) ok = streams_overlap(pool[dev][l], cand, stamps);
        if (ok) pool[dev][have++] = cand;
        else spare[n_spare++] = cand;
    }
    g_lane_pool_concurrent[dev] = have;
    // fewer than ML concurrent queues on this device / configuration: the remaining lanes share (correct, only slower)
    for (int i = 0; have < ML && i < n_spare; ++i) pool[dev][have++] = spare[i], spare[i] = nullptr;
    for (int i = 0; i < n_spare; ++i)
        if (spare[i]) (void)hipStreamDestroy(spare[i]);
    (void)hipFree(stamps);
    (void)hipGetLastError();
    if (have < ML) {                            // stream creation failed part-way: give back what was made, do not retry
        for (int i = 0; i < have; ++i) (void)hipStreamDestroy(pool[dev][i]), pool[dev][i] = nullptr;
        g_lane_pool_concurrent[dev] = 0;
        failed[dev] = true;
        (void)hipGetLastError();
        return nullptr;
    }
    ready[dev] = true;
    return pool[dev];
}

// The two kinds of step: STEP_GUIDED = the CFG pass over 2n sequences and pred = u + w (c - u); STEP_COND = one pass over
// the n rows with their text, whose output the update takes as pred unchanged (pred_u = out, pred_c = NULL: no w = 1
// arithmetic; a row's guidance scale is not read).  Draws, stream ids, coefficient row, history and the advance of the loop
// index do not depend on the kind.
enum StepKind { STEP_GUIDED = 0, STEP_COND = 1 };
inline StepKind step_kind(const t2s_sampler* s, int j) { return (j >= s->guide_first && j < s->guide_end) ? STEP_GUIDED : STEP_COND; }

// one loop iteration of rows [r0, r0 + n) of the batch on stream st, stepping the lane's counter
int enqueue_step(t2s_sampler* s, float* x, const float* text, const float* noise, hipStream_t st, int lane, int r0,
                 int n, StepKind kind) {
    const t2s_sample_config& c = s->cfg;
    LoopState* loop = s->step + LANE_STATES * lane;
    const size_t lat = (size_t)s->lat;   // the sampler's row length
    float* xl = x + (size_t)r0 * lat;
    float* eu = s->eps_u + (size_t)r0 * lat;
    float* ec = kind == STEP_GUIDED ? s->eps_c + (size_t)r0 * lat : nullptr;
    int rc = kind == STEP_GUIDED
                 ? dit_forward_cfg_step(s->dit, xl, s->temb_table, &loop->index, text + (size_t)r0 * D, eu, ec, n, st, 2 * r0,
                                        s->mod_table, c.batch + 1, r0)
                 : dit_forward_cond_step(s->dit, xl, s->temb_table, &loop->index, text + (size_t)r0 * D, eu, n, st, 2 * r0,
                                         s->mod_table, c.batch + 1, r0);
    if (rc != T2S_OK) return rc;
    UpdateArgs a{};
    a.x = xl; a.pred_u = eu; a.pred_c = ec; a.noise = noise ? noise + (size_t)r0 * lat : nullptr; a.coef = s->coef;
    a.loop = loop; a.cfg = c.cfg_scale; a.seed = c.seed; a.B = n; a.qpr = s->lat / 4; a.noise_rows = c.batch; a.advance = loop;
    a.row_seed = rows_seed(s->d_rows, c.batch) + r0;
    a.row_key = rows_key(s->d_rows, c.batch) + r0;
    a.row_cfg = rows_cfg(s->d_rows, c.batch) + r0;
    switch (c.mode) {   // (the create entries admit these three modes only; launch_update refuses any other)
    case T2S_MODE_DDPM: a.steps = c.steps; break;
    case T2S_MODE_LMS: a.hist = s->hist + (size_t)r0 * lat; break;
    case T2S_MODE_RF: a.dt = 1.0f / (float)c.steps; break;
    }
    return launch_update(c.mode, a, st);   // (the update kernel's last workgroup advances the lane's loop index)
}

// Whole-loop graphs by default?  Same-box A/B (tools/ab_loop_graph.sh, profiles/r04_loop_graph_ab.txt), series/s one-step /
// whole-loop: rectified flow 100 steps at B = 1024 637.4 / 636.3 (-0.2 %, noise), at B = 32 569.3 / 574.7 (+0.9 %: the host's
// 200 graph launches per run are on the critical path of a 56 ms run), DDPM 1000 steps at B = 256 63.70 / 63.75.  So: the
// whole loop as ONE graph per lane for the step counts the authors sample with (10 - 100, scripts/script.sh), where it is
// never slower and a capture is <= 2,560 nodes; the one-step graph beyond (a 1000-step loop would be 10,000 nodes per
// lane for nothing).
inline int loop_graph_default(int steps) { return steps <= 256; }

void drop_graph(t2s_sampler* s) {
    for (int k = 0; k < t2s_sampler::KINDS; ++k)
        for (int l = 0; l < t2s_sampler::MAX_LANES; ++l) {
            if (s->exec[k][l]) (void)hipGraphExecDestroy(s->exec[k][l]);
            if (s->graph[k][l]) (void)hipGraphDestroy(s->graph[k][l]);
            s->exec[k][l] = nullptr;
            s->graph[k][l] = nullptr;
        }
    s->lanes_cap = 0;
}

inline bool has_graphs(const t2s_sampler* s) { return s->exec[STEP_GUIDED][0] || s->exec[STEP_COND][0]; }

// lanes of this run: as asked for, or automatically EQUAL shares of whole 32-row groups: two for a batch that is a
// multiple of 64 (and 16 + 16 for 32 series), three for 96.  Measured with the round-3 kernels (tools/strong_probe.py,
// series/s with one lane / the automatic choice): 256: 60.1 / 64.3, 192: 59.9 / 63.5, 128: 58.7 / 62.8, 96: 58.3 / 62.3,
// 64: 57.4 / 61.5, 32: 52.1 / 58.4 -- at the small sizes a launch is mostly fixed cost, which the other lanes' kernels
// cover.  Unequal lanes go either way (224 = 128 + 96: 60.1 / 62.6; 160 = 96 + 64: 59.4 / 57.7; 96 = 64 + 32: 55.6 when the
// two lanes run DIFFERENT attention kernels -- a persistent workgroup fills a CU's registers and the other lane's packed
// workgroups wait for it) and splits without whole groups lose (48: 47.3 / 39.8, 16: 44.1 / 37.7), so those stay on one
// lane; three lanes 61.6 and four 60.4 at 256, three 61.2 at 192.
int pick_lanes(const t2s_sampler* s, bool trace) {
    if (trace || s->cfg.batch < 2) return 1;
    const int B = s->cfg.batch;
    int lanes = (B % 64 == 0 || B == 32) ? 2 : (B == 96 ? 3 : 1);
    if (const char* e = getenv("T2S_SAMPLER_LANES")) lanes = atoi(e);
    if (s->lanes_req) lanes = s->lanes_req;
    lanes = lanes < 1 ? 1 : (lanes > t2s_sampler::MAX_LANES ? t2s_sampler::MAX_LANES : lanes);
    return lanes < s->cfg.batch ? lanes : s->cfg.batch;
}

}  // namespace

// for the other translation units' set-up work (t2s_dit_set_math): the same stream, the same lock
namespace t2s {
hipStream_t lib_setup_stream(int dev) { return setup_stream(dev); }
std::recursive_mutex* lib_pool_lock(int dev) { return dev >= 0 && dev < 16 ? &g_pool_use[dev] : nullptr; }
}  // namespace t2s

// t2s_sampler_create (lms_coef NULL; modes DDPM / RF) and t2s_sampler_create_lms (mode LMS, HOST (steps,6) table)
static int sampler_create(t2s_dit* dit, t2s_vae* vae, const t2s_sample_config* cfg, const float* lms_coef, t2s_sampler** out) {
    T2S_REQUIRE(cfg->steps > 0 && cfg->steps <= 100000, "t2s_sampler_create: steps=%d", cfg->steps);
    T2S_REQUIRE(cfg->batch > 0 && 2 * cfg->batch <= t2s_dit_max_seqs(dit),
                "t2s_sampler_create: batch=%d needs 2*batch <= dit max_seqs=%d", cfg->batch, t2s_dit_max_seqs(dit));
    T2S_REQUIRE(cfg->t_values, "t2s_sampler_create: t_values is NULL");
    const int latw = t2s_dit_latent_w(dit);
    T2S_REQUIRE(!vae || latw <= 32 || t2s_vae_channels(vae) != 0,
                "t2s_sampler_create: a DiT of latent width %d needs a multichannel decoder (t2s_vae_create_mc) or NULL", latw);
    T2S_REQUIRE((long long)cfg->batch * LATC * latw < (1ll << 31), "t2s_sampler_create: batch=%d at latent width %d", cfg->batch, latw);
    T2S_REQUIRE(cfg->mode != T2S_MODE_DDPM || cfg->ddpm_coef, "t2s_sampler_create: DDPM needs ddpm_coef");
    // a multichannel decoder (t2s_vae_create_mc) resamples to any length >= 8; the single-channel one builds multiples of 4
    T2S_REQUIRE(!vae || (t2s_vae_channels(vae) ? cfg->length >= 8 : cfg->length >= 4 && cfg->length % 4 == 0) && cfg->length <= (1 << 20),
                "t2s_sampler_create: length=%d unsupported", cfg->length);
    // allocations, synchronous copies and a stream synchronisation follow: not while another thread's run has a capture open
    // on the pool streams (same lock as t2s_sampler_run; see include/t2s.h "Threads")
    int cur_dev = 0;
    T2S_HIP_CHECK(hipGetDevice(&cur_dev));
    T2S_REQUIRE(cur_dev >= 0 && cur_dev < 16, "t2s_sampler_create: device %d", cur_dev);
    std::lock_guard<std::recursive_mutex> pool_lock(g_pool_use[cur_dev]);
    t2s_sampler* s = new t2s_sampler();
    s->dit = dit; s->vae = vae; s->cfg = *cfg; s->lat = LATC * latw;
    s->guide_first = 0; s->guide_end = cfg->steps;     // every step guided
    const size_t lat = (size_t)s->lat;
    s->cfg.ddpm_coef = nullptr; s->cfg.t_values = nullptr;  // host pointers are not retained
    const size_t B = (size_t)cfg->batch, T = (size_t)cfg->steps;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    alloc((void**)&s->temb_table, T * D * sizeof(float));
    alloc((void**)&s->coef, T * (lms_coef ? 6 : 3) * sizeof(float));
    if (lms_coef) alloc((void**)&s->hist, B * lat * sizeof(float));
    alloc((void**)&s->eps_u, B * lat * sizeof(float));
    alloc((void**)&s->eps_c, B * lat * sizeof(float));
    alloc((void**)&s->tvals, T * sizeof(float));
    alloc((void**)&s->step, t2s_sampler::MAX_LANES * LANE_STATES * sizeof(LoopState));   // one per lane, 64 B apart
    alloc(&s->d_rows, rows_bytes(cfg->batch) + len_bytes(cfg->batch));    // per-row tables (t2s_sampler_set_rows, _set_lengths)
    if (e == hipSuccess) e = hipHostMalloc(&s->h_stage, rows_bytes(cfg->batch) + len_bytes(cfg->batch), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_rows, hipEventDisableTiming);
    s->h_rows.assign(rows_bytes(cfg->batch), 0);
    s->h_len.assign(len_bytes(cfg->batch), 0);
    // whole-run adaLN table (dit_adaln_table; 3.2 GB at 256 series x 1000 steps for ~2 % of a step): only while it is a
    // small part of what the device has FREE right now -- at most 1/8 of it and 16 GB -- so that a process holding several
    // samplers, or sharing the GPU with torch's allocator or a training job, does not run dry later for an optimisation;
    // beyond that the per-step kernel stays in the loop (same bits).  T2S_ADALN_TABLE=0 switches the table off.
    const size_t table_bytes = T * (B + 1) * (size_t)MODROW * sizeof(float);
    const char* table_env = getenv("T2S_ADALN_TABLE");   // =0: keep the per-step adaLN kernel (A/B, and the test of that path)
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) mem_free = 0, (void)hipGetLastError();
    if (e == hipSuccess && !(table_env && atoi(table_env) == 0) && table_bytes <= ((size_t)16 << 30) && table_bytes <= mem_free / 8 &&
        hipMalloc((void**)&s->mod_table, table_bytes) != hipSuccess) {
        s->mod_table = nullptr;       // an optimisation only: a device too full for it keeps the per-step kernel
        (void)hipGetLastError();
    }
    // Uploads and the table kernel run on a NON-BLOCKING stream of the library's own, never on the legacy default stream: an
    // operation on the legacy stream implicitly joins every blocking stream of the device, and HIP refuses it
    // (hipErrorStreamCaptureImplicit, "operation would make the legacy stream depend on a capturing blocking stream") while
    // ANY thread has a capture open -- invalidating that capture.  That was the round-4 two-thread failure (reproduced in
    // round 5 by a diagnosis build with the serialisation taken away, last carried by commit f0cbfbc).
    hipStream_t setup = setup_stream(cur_dev);
    if (e == hipSuccess && !setup) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipMemcpyAsync(s->tvals, cfg->t_values, T * sizeof(float), hipMemcpyHostToDevice, setup);
    if (e == hipSuccess && cfg->mode == T2S_MODE_DDPM)
        e = hipMemcpyAsync(s->coef, cfg->ddpm_coef, T * 3 * sizeof(float), hipMemcpyHostToDevice, setup);
    if (e == hipSuccess && lms_coef) e = hipMemcpyAsync(s->coef, lms_coef, T * 6 * sizeof(float), hipMemcpyHostToDevice, setup);
    // a caller's table may read the history at its first step (the solvers of t2ms_amd.sampler.solver_tables never do)
    if (e == hipSuccess && lms_coef) e = hipMemsetAsync(s->hist, 0, B * lat * sizeof(float), setup);
    if (e == hipSuccess) e = hipStreamSynchronize(setup);      // the host tables may go away when the call returns
    if (e != hipSuccess) {
        set_error("t2s_sampler_create: allocation/upload failed: %s", hipGetErrorString(e));
        t2s_sampler_destroy(s);
        return T2S_E_HIP;
    }
    // time-embedding table for every loop index (transformer.py:30-40 applied to t_values)
    int rc = t2s_time_embedding(dit, s->tvals, s->temb_table, cfg->steps, setup);
    if (rc == T2S_OK && hipStreamSynchronize(setup) != hipSuccess) {
        set_error("t2s_sampler_create: time-embedding table failed");
        rc = T2S_E_HIP;
    }
    if (rc != T2S_OK) {
        t2s_sampler_destroy(s);
        return rc;
    }
    // calibrate the lane-stream pool HERE (create synchronises anyway): t2s_sampler_run then never allocates, copies or
    // synchronises for it -- legal while the calling thread has a capture open, and its timing test runs on an idle stream
    (void)lane_streams();
    *out = s;
    return T2S_OK;
}

extern "C" int t2s_sampler_create(t2s_dit* dit, t2s_vae* vae, const t2s_sample_config* cfg, t2s_sampler** out) {
    T2S_REQUIRE(dit && cfg && out, "t2s_sampler_create: NULL argument");
    T2S_REQUIRE(cfg->mode == T2S_MODE_DDPM || cfg->mode == T2S_MODE_RF, "t2s_sampler_create: mode=%d", cfg->mode);
    return sampler_create(dit, vae, cfg, nullptr, out);
}

extern "C" int t2s_sampler_create_lms(t2s_dit* dit, t2s_vae* vae, const t2s_sample_config* cfg, const float* lms_coef,
                                      t2s_sampler** out) {
    // every refusal before any allocation
    T2S_REQUIRE(dit && cfg && out, "t2s_sampler_create_lms: NULL argument");
    T2S_REQUIRE(cfg->mode == T2S_MODE_LMS, "t2s_sampler_create_lms: mode=%d (T2S_MODE_LMS = %d)", cfg->mode, T2S_MODE_LMS);
    T2S_REQUIRE(cfg->steps >= 1, "t2s_sampler_create_lms: steps=%d", cfg->steps);
    T2S_REQUIRE(lms_coef, "t2s_sampler_create_lms: the coefficient table is NULL");
    T2S_REQUIRE(cfg->steps <= 100000, "t2s_sampler_create_lms: steps=%d", cfg->steps);
    for (int i = 0; i < cfg->steps * 6; ++i)
        T2S_REQUIRE(std::isfinite(lms_coef[i]), "t2s_sampler_create_lms: coefficient %d of step %d is not finite", i % 6, i / 6);
    return sampler_create(dit, vae, cfg, lms_coef, out);
}

extern "C" int t2s_sampler_set_lanes(t2s_sampler* s, int lanes) {
    T2S_REQUIRE(s && lanes >= 0 && lanes <= t2s_sampler::MAX_LANES, "t2s_sampler_set_lanes: lanes=%d (0 = automatic, 1 .. %d)", lanes,
                t2s_sampler::MAX_LANES);
    s->lanes_req = lanes;
    return T2S_OK;
}

extern "C" int t2s_sampler_set_loop_graph(t2s_sampler* s, int whole_loop) {
    T2S_REQUIRE(s && (whole_loop == 0 || whole_loop == 1 || whole_loop == -1), "t2s_sampler_set_loop_graph: %d (1 whole loop, 0 one step, -1 default)", whole_loop);
    s->whole_req = whole_loop;
    return T2S_OK;
}

extern "C" int t2s_sampler_set_guided_steps(t2s_sampler* s, int first, int end) {
    T2S_REQUIRE(s, "t2s_sampler_set_guided_steps: NULL sampler");
    T2S_REQUIRE(0 <= first && first <= end && end <= s->cfg.steps,
                "t2s_sampler_set_guided_steps: first=%d end=%d must satisfy 0 <= first <= end <= steps=%d", first, end, s->cfg.steps);
    if (first == s->guide_first && end == s->guide_end) return T2S_OK;    // unchanged: the captured graphs stay
    // the graphs hold the kinds of the old window (destroying them waits for no stream: same lock as a run's capture)
    int cur_dev = 0;
    std::unique_lock<std::recursive_mutex> pool_lock;
    if (hipGetDevice(&cur_dev) == hipSuccess && cur_dev >= 0 && cur_dev < 16) pool_lock = std::unique_lock<std::recursive_mutex>(g_pool_use[cur_dev]);
    drop_graph(s);
    s->guide_first = first;
    s->guide_end = end;
    return T2S_OK;
}

extern "C" int t2s_sampler_guided_steps(const t2s_sampler* s, int* first, int* end) {
    T2S_REQUIRE(s && first && end, "t2s_sampler_guided_steps: NULL argument");
    *first = s->guide_first;
    *end = s->guide_end;
    return T2S_OK;
}

extern "C" int t2s_sampler_set_row0(t2s_sampler* s, uint32_t row0) {
    T2S_REQUIRE(s, "t2s_sampler_set_row0: NULL sampler");
    s->cfg.row0 = row0;   // uploaded next to the step counters at the start of every run: no re-capture
    return T2S_OK;
}

extern "C" int t2s_sampler_set_rows(t2s_sampler* s, const uint64_t* seeds, const uint32_t* key_rows, const float* cfg, int n) {
    T2S_REQUIRE(s, "t2s_sampler_set_rows: NULL sampler");
    const int B = s->cfg.batch;
    T2S_REQUIRE(n == B, "t2s_sampler_set_rows: n=%d, the sampler's batch is %d", n, B);
    if (cfg)
        for (int r = 0; r < n; ++r) T2S_REQUIRE(std::isfinite(cfg[r]), "t2s_sampler_set_rows: cfg[%d] is not finite", r);
    // host work only: the tables reach the device at the next run (no copy here, so no thread-contract question)
    void* h = s->h_rows.data();
    int rows = 0;
    if (seeds) memcpy(rows_seed(h, B), seeds, (size_t)n * sizeof(uint64_t)), rows |= ROWS_SEED;
    if (key_rows) memcpy(rows_key(h, B), key_rows, (size_t)n * sizeof(uint32_t)), rows |= ROWS_KEY;
    if (cfg) memcpy(rows_cfg(h, B), cfg, (size_t)n * sizeof(float)), rows |= ROWS_CFG;
    s->rows = rows;
    s->rows_dirty = rows != 0;
    return T2S_OK;
}

extern "C" int t2s_sampler_set_lengths(t2s_sampler* s, const int32_t* lengths, int n) {
    T2S_REQUIRE(s, "t2s_sampler_set_lengths: NULL sampler");
    if (!lengths) {          // uniform again
        s->ragged = false;
        s->len_dirty = false;
        return T2S_OK;
    }
    T2S_REQUIRE(s->vae && t2s_vae_channels(s->vae) != 0,
                "t2s_sampler_set_lengths: per-row lengths need a multichannel decoder (t2s_vae_create_mc)");
    const int B = s->cfg.batch;
    T2S_REQUIRE(n == B, "t2s_sampler_set_lengths: n=%d, the sampler's batch is %d", n, B);
    for (int r = 0; r < n; ++r)
        T2S_REQUIRE(lengths[r] == 0 || (lengths[r] >= 8 && lengths[r] <= s->cfg.length),
                    "t2s_sampler_set_lengths: lengths[%d]=%d (0, or 8 .. the sampler's length %d)", r, lengths[r], s->cfg.length);
    // host work only, as t2s_sampler_set_rows: the arrays reach the device at the next run
    void* h = s->h_len.data();
    uint64_t off = 0;
    for (int r = 0; r < n; ++r) {
        len_offsets(h)[r] = off;
        len_lengths(h, B)[r] = lengths[r];
        off += (uint64_t)lengths[r];
    }
    len_offsets(h)[n] = off;
    s->ragged = true;
    s->len_dirty = true;
    return T2S_OK;
}

extern "C" int t2s_sampler_lane_pool(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    return g_lane_pool_concurrent[dev];
}

extern "C" int t2s_sampler_graph_lanes(const t2s_sampler* s) { return (s && has_graphs(s)) ? s->lanes_cap : 0; }

extern "C" void t2s_sampler_destroy(t2s_sampler* s) {
    if (!s) return;
    int cur_dev = 0;
    std::unique_lock<std::recursive_mutex> pool_lock;  // hipFree synchronises the device: not inside another thread's capture
    if (hipGetDevice(&cur_dev) == hipSuccess && cur_dev >= 0 && cur_dev < 16) pool_lock = std::unique_lock<std::recursive_mutex>(g_pool_use[cur_dev]);
    drop_graph(s);
    for (int l = 0; l < t2s_sampler::MAX_LANES; ++l)
        if (s->ev_join[l]) (void)hipEventDestroy(s->ev_join[l]);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_in) (void)hipEventDestroy(s->ev_in);
    if (s->ev_out) (void)hipEventDestroy(s->ev_out);
    if (s->ev_rows && s->ev_rows_recorded) (void)hipEventSynchronize(s->ev_rows);   // the last upload has read h_stage
    if (s->ev_rows) (void)hipEventDestroy(s->ev_rows);
    if (s->h_stage) (void)hipHostFree(s->h_stage);
    void* bufs[] = {s->temb_table, s->coef, s->hist, s->eps_u, s->eps_c, s->tvals, s->step, s->mod_table, s->d_rows};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete s;
}

// the sampler's decode of n latents: a multichannel decoder handle writes (n,C,L) at the DiT's latent width, a single-channel
// one (n,L) (width 30 only: sampler_create refuses it on a wider DiT)
static int sampler_decode(t2s_vae* vae, const float* x, float* out, int n, int L, int latw, hipStream_t st) {
    if (t2s_vae_channels(vae) != 0) return t2s_vae_decode_mc(vae, x, out, nullptr, n, L, latw, st);
    return t2s_vae_decode(vae, x, out, nullptr, n, L, st);
}

extern "C" int t2s_sampler_run(t2s_sampler* s, float* x, const float* text, const float* noise, float* series,
                               float* trace0, void* stream) {
    T2S_REQUIRE(s && x && text, "t2s_sampler_run: NULL argument");
    T2S_REQUIRE(!series || s->vae, "t2s_sampler_run: series requested but the sampler has no VAE");
    T2S_REQUIRE(!trace0 || s->vae, "t2s_sampler_run: trace requested but the sampler has no VAE");
    hipStream_t st = (hipStream_t)stream;
    const t2s_sample_config& c = s->cfg;
    const int len0 = s->ragged ? len_lengths(s->h_len.data(), c.batch)[0] : c.length;
    T2S_REQUIRE(!trace0 || len0 != 0, "t2s_sampler_run: trace requested but row 0 has length 0 (t2s_sampler_set_lengths)");
    int rc;
    int lanes = pick_lanes(s, trace0 != nullptr);
    const bool graph_ok = c.use_graph && !trace0;
    // Held to the end of the call by EVERY run that opens a stream capture or touches the pool streams -- a single-lane run
    // capturing on the caller's own stream included: another thread's t2s_sampler_create / _destroy (allocations, synchronous
    // copies, synchronisation) and the pool's calibration are then never concurrent with an open capture of this library.
    std::unique_lock<std::recursive_mutex> pool_lock;
    if (graph_ok || lanes > 1) {
        int dev = 0;
        T2S_HIP_CHECK(hipGetDevice(&dev));
        T2S_REQUIRE(dev >= 0 && dev < 16, "t2s_sampler_run: device %d", dev);
        pool_lock = std::unique_lock<std::recursive_mutex>(g_pool_use[dev]);
    }
    if (lanes > 1 && !lane_streams()) lanes = 1;      // no stream pool on this device: one chain, same results
    // the default stream cannot be captured (never a silent eager run), and several lanes run on streams created TOGETHER
    // (distinct hardware queues): the caller's stream then only carries the fork and the join
    hipStream_t const caller = st;
    const bool via_own = (graph_ok && st == nullptr) || lanes > 1;
    if (via_own) {
        if (!s->own) {
            hipStream_t* pool = lane_streams();
            T2S_REQUIRE(pool, "t2s_sampler_run: cannot create the lane streams");
            s->own = pool[0];
            T2S_HIP_CHECK(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
            T2S_HIP_CHECK(hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming));
        }
        T2S_HIP_CHECK(hipEventRecord(s->ev_in, caller));
        T2S_HIP_CHECK(hipStreamWaitEvent(s->own, s->ev_in, 0));
        st = s->own;
    }
    if (lanes > 1 && !s->ev_fork) T2S_HIP_CHECK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
    for (int l = 1; l < lanes; ++l)
        if (!s->side[l]) {
            hipStream_t* pool = lane_streams();
            T2S_REQUIRE(pool, "t2s_sampler_run: cannot create the lane streams");
            s->side[l] = pool[l];
            T2S_HIP_CHECK(hipEventCreateWithFlags(&s->ev_join[l], hipEventDisableTiming));
        }
    // lane l steps rows [r0[l], r0[l] + nr[l]) on lst[l]
    // split point: half the batch, rounded to a multiple of 32 rows when both lanes keep >= 32 -- the persistent
    // attention kernel walks 8 * rows / n_cu (sequence, head) items per CU, a whole number only in steps of 32 rows
    // (a 144 + 112 split of 256 measured 12 % SLOWER than one lane, 128 + 128 or 160 + 96 4 % faster)
    // (more lanes: equal shares, in whole 32-row groups when every lane keeps at least one)
    constexpr int ML = t2s_sampler::MAX_LANES;
    int r0[ML + 1] = {}, nr[ML] = {};
    {
        const int share = (c.batch + lanes - 1) / lanes, share32 = (share + 31) / 32 * 32;
        const int step = (c.batch - (lanes - 1) * share32 >= 32) ? share32 : share;
        for (int l = 0; l <= lanes; ++l) r0[l] = l * step < c.batch ? l * step : c.batch;
        r0[lanes] = c.batch;
        for (int l = 0; l < lanes; ++l) nr[l] = r0[l + 1] - r0[l];
        while (lanes > 1 && nr[lanes - 1] == 0) --lanes;      // a batch too small for its last lane
    }
    hipStream_t lst[ML] = {st, s->side[1], s->side[2], s->side[3]};
    // One graph per lane holds either ONE step (replayed `steps` times from the host) or the WHOLE loop (steps x 10 kernel
    // nodes, launched once): every node reads its loop index from the lane's device counter, so the two are the same
    // kernels in the same order.  Default: see loop_graph_default().
    int whole = s->whole_req;
    if (whole < 0) {
        const char* e = getenv("T2S_SAMPLER_LOOP_GRAPH");
        whole = e ? (atoi(e) != 0) : loop_graph_default(c.steps);
    }
    // (a changed guided window has dropped the graphs: t2s_sampler_set_guided_steps)
    if (graph_ok && (!has_graphs(s) || s->lanes_cap != lanes || s->whole_cap != whole || s->g_x != x || s->g_text != text ||
                     s->g_noise != noise)) {
        drop_graph(s);
        // whole loop: one graph per lane (slot 0), step j enqueued with the kind of j; one step: a graph per kind that the
        // window needs -- with the default window the guided one alone, as before there were kinds
        const bool need[t2s_sampler::KINDS] = {s->guide_first < s->guide_end, s->guide_first > 0 || s->guide_end < c.steps};
        for (int l = 0; l < lanes; ++l)
            for (int k = 0; k < (whole ? 1 : t2s_sampler::KINDS); ++k) {
                if (!whole && !need[k]) continue;
                T2S_HIP_CHECK(hipStreamBeginCapture(lst[l], hipStreamCaptureModeThreadLocal));
                rc = T2S_OK;
                for (int j = 0; j < (whole ? c.steps : 1) && rc == T2S_OK; ++j)
                    rc = enqueue_step(s, x, text, noise, lst[l], l, r0[l], nr[l], whole ? step_kind(s, j) : (StepKind)k);
                hipError_t e = hipStreamEndCapture(lst[l], &s->graph[k][l]);
                if (rc != T2S_OK) {
                    drop_graph(s);
                    return rc;
                }
                if (e != hipSuccess) {
                    set_error("t2s_sampler_run: hipStreamEndCapture failed: %s", hipGetErrorString(e));
                    drop_graph(s);
                    return T2S_E_HIP;
                }
                T2S_HIP_CHECK(hipGraphInstantiate(&s->exec[k][l], s->graph[k][l], nullptr, nullptr, 0));
            }
        s->lanes_cap = lanes;
        s->whole_cap = whole;
        s->g_x = x; s->g_text = text; s->g_noise = noise;
    }
    // the adaLN modulation of every step for this run's text (state-independent: off the loop's critical path)
    if (s->mod_table && (rc = dit_adaln_table(s->dit, s->temb_table, c.steps, text, c.batch, s->mod_table, st)) != T2S_OK) return rc;
    // per-row tables set since the last run: stream-ordered upload from the sampler's own pinned staging buffer (the
    // previous upload has read it once ev_rows completes), before the fork so that every lane sees them
    // (the lengths of t2s_sampler_set_lengths ride behind them, for the decode at the end)
    const bool up_rows = s->rows && s->rows_dirty, up_len = s->ragged && s->len_dirty;
    if (up_rows || up_len) {
        if (s->ev_rows_recorded) T2S_HIP_CHECK(hipEventSynchronize(s->ev_rows));
        if (up_rows) {
            memcpy(s->h_stage, s->h_rows.data(), s->h_rows.size());
            T2S_HIP_CHECK(hipMemcpyAsync(s->d_rows, s->h_stage, s->h_rows.size(), hipMemcpyHostToDevice, st));
            s->rows_dirty = false;
        }
        if (up_len) {
            const size_t at = rows_bytes(c.batch);
            memcpy((unsigned char*)s->h_stage + at, s->h_len.data(), s->h_len.size());
            T2S_HIP_CHECK(hipMemcpyAsync((unsigned char*)s->d_rows + at, (unsigned char*)s->h_stage + at, s->h_len.size(),
                                         hipMemcpyHostToDevice, st));
            s->len_dirty = false;
        }
        T2S_HIP_CHECK(hipEventRecord(s->ev_rows, st));
        s->ev_rows_recorded = true;
    }
    if (lanes > 1) {    // fork: the other lanes start after everything already queued on the caller's stream
        T2S_HIP_CHECK(hipEventRecord(s->ev_fork, st));
        for (int l = 1; l < lanes; ++l) T2S_HIP_CHECK(hipStreamWaitEvent(s->side[l], s->ev_fork, 0));
    }
    for (int l = 0; l < lanes; ++l) {
        set_step_kernel<<<1, 64, 0, lst[l]>>>(s->step + LANE_STATES * l, 0, c.row0 + (uint32_t)r0[l], s->rows);
        T2S_LAUNCH_CHECK();
    }
    if (graph_ok && whole)
        for (int l = 0; l < lanes; ++l) T2S_HIP_CHECK(hipGraphLaunch(s->exec[0][l], lst[l]));
    for (int j = 0; j < c.steps && !(graph_ok && whole); ++j) {
        const StepKind kind = step_kind(s, j);     // (the host's j is the lanes' device loop index: every step advances it by one)
        for (int l = 0; l < lanes; ++l) {
            if (graph_ok) {
                T2S_HIP_CHECK(hipGraphLaunch(s->exec[kind][l], lst[l]));
            } else if ((rc = enqueue_step(s, x, text, noise, lst[l], l, r0[l], nr[l], kind)) != T2S_OK) {
                return rc;
            }
        }
        if (trace0) {
            // infer.py:90-93: decode row 0 of the first batch after every step
            // (with per-row lengths: at row 0's own length)
            const int ch = t2s_vae_channels(s->vae);
            if ((rc = sampler_decode(s->vae, x, trace0 + (size_t)j * (ch ? ch : 1) * len0, 1, len0, s->lat / LATC, st)) != T2S_OK) return rc;
        }
    }
    for (int l = 1; l < lanes; ++l) {   // join before the decode (and before anything the caller queues next)
        T2S_HIP_CHECK(hipEventRecord(s->ev_join[l], s->side[l]));
        T2S_HIP_CHECK(hipStreamWaitEvent(st, s->ev_join[l], 0));
    }
    if (series && s->ragged) {
        void* d_len = (unsigned char*)s->d_rows + rows_bytes(c.batch);
        if ((rc = t2s_vae_decode_mc_ragged(s->vae, x, len_lengths(d_len, c.batch), len_offsets(d_len), series, c.batch, c.length,
                                           s->lat / LATC, st)) != T2S_OK) return rc;
    } else if (series) {
        if ((rc = sampler_decode(s->vae, x, series, c.batch, c.length, s->lat / LATC, st)) != T2S_OK) return rc;
    }
    if (via_own) {      // whatever the caller queues on its stream next sees the results
        T2S_HIP_CHECK(hipEventRecord(s->ev_out, st));
        T2S_HIP_CHECK(hipStreamWaitEvent(caller, s->ev_out, 0));
    }
    return T2S_OK;
}
