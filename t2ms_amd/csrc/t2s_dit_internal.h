// Internal definition of the t2s_dit handle, shared by t2s_dit.hip (inference) and t2s_train.hip, and the functions the
// translation units of the DiT call across their borders.
#pragma once
#include <mutex>
#include <vector>

#include "t2s_arena.h"
#include "t2s_common.h"

struct t2s_train_ws;   // training workspace (t2s_train.hip), created on first use

struct t2s_dit {
    int max_seqs = 0;
    int latw = t2s::LATW;        // latent width W: the latent is (64, W), a sequence 16 W tokens (30 / 50 / 64: 480 / 800 / 1024)
    int ntok() const { return 16 * latw; }
    int lat() const { return t2s::LATC * latw; }
    // parameters (device)
    float* arena = nullptr;  // all parameters, laid out by carve_params (t2s_dit.hip)
    float *conv_w, *conv_b, *patch_w, *patch_b, *pos, *ln_w, *ln_b, *out_w, *out_b, *freqs, *ada_b;
    t2s::f32x4* ada_p;
    t2s::BlockMats<float*> bias[t2s::NBLK];
    t2s::BlockMats<t2s::f32x4*> p32[t2s::NBLK];   // the row-chain weights in fragment order, fc2 in chunk order (t2s_rows.h)
    t2s::BlockMats<t2s::f32x4*> p16[t2s::NBLK];   // the same in the 16-token kernel's fragment order (t2s_rows16.h; small launches)
    // workspace (device), activations fragment-major; one allocation each, listed by workspace_bufs (t2s_dit.hip)
    float *h = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *ao = nullptr;
    float* h0 = nullptr;         // patchified tokens of the B distinct sequences of a CFG pass (both branches share them)
    float* mod = nullptr;        // (S, MODROW) adaLN modulation of all blocks (adaln_kernel)
    int math = 0;
    // T2S_MATH_BF16X3 / T2S_MATH_BF16: k and V^T of the running block as np split bf16 planes (t2s_x3.h; bf16 keeps the h plane
    // of the split alone) and the row chain's weights as np planes in chunk order (t2s_rows_x3.h).  Allocated on the mode's
    // first use (w != NULL: ready); a workspace per mode, so that switching between the arithmetics never reads another
    // mode's planes
    struct BfPlanes {
        int np;
        __bf16 *k = nullptr, *v = nullptr, *w = nullptr;
        t2s::BlockMats<__bf16*> m[t2s::NBLK];   // pieces of w (fc2 in chunk order)
    };
    BfPlanes bf[2] = {{3}, {1}};   // [math - T2S_MATH_BF16X3]
    hipEvent_t w_ev = nullptr;   // recorded behind the last t2s_dit_update_weights (what a first-use pack must wait for)
    t2s_train_ws* train = nullptr;
    int train_dtype = 0;         // T2S_TRAIN_F32 / T2S_TRAIN_BF16 (t2s_dit_set_train_dtype)
    bool trainable = false;      // a wide handle trains only after t2s_dit_set_trainable (width 30 always does)
    bool wide_math = false;      // ... and takes T2S_MATH_BF16X3 / _BF16 only after t2s_dit_set_wide_math (t2s_wide_math.h)
    bool wide_train_bf16 = false;   // ... and T2S_TRAIN_BF16 only after t2s_dit_set_wide_train_bf16 on top of `trainable` (t2s_wide_train_bf16.h)
    // optional in-situ kernel timing (HIP events on the launching stream; never under capture)
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_class;   // class of interval i = [ev_pool[2i], ev_pool[2i+1]]
};


namespace t2s {
// launch classes of the in-situ timing (t2s_dit_timing_begin / _end[_ex]): inference forward 0-2, training step 3-8
// 9 / 10: the first (<qkv only>, with patchify) and the last (<proj + MLP> + final layer) row-chain launch of a forward; they
// are ALSO counted in class 1, which stays "every row-chain launch"
enum { TC_ATTN = 0, TC_ROWS = 1, TC_OTHER = 2, TC_TR_GEMM = 3, TC_TR_ATTN_FWD = 4, TC_TR_ATTN_BWD = 5, TC_TR_WGRAD = 6,
       TC_TR_ELEM = 7, TC_TR_TAIL = 8, TC_ROWS_FIRST = 9, TC_ROWS_LAST = 10, TC_COUNT = 11 };
struct TimeScope {   // records an event pair around the launches issued in its scope when timing is on
    t2s_dit* h; hipStream_t st; bool on;
    TimeScope(t2s_dit* h_, int cls, hipStream_t st_) : h(h_), st(st_), on(h_->timing) {
        if (!on) return;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
        h->ev_pool.push_back(a); h->ev_pool.push_back(b); h->ev_class.push_back(cls);
        (void)hipEventRecord(a, st);
    }
    ~TimeScope() { if (on) (void)hipEventRecord(h->ev_pool.back(), st); }
};
// One launch as one timed interval of class `cls`, in a function that returns a t2s code: T2S_TIMED takes a call that returns
// such a code, T2S_TIMED_LAUNCH a kernel<<<...>>>(...) statement.  A failure returns from the enclosing function.
#define T2S_TIMED(h, cls, st, ...)                                                             \
    do {                                                                                       \
        ::t2s::TimeScope _ts(h, cls, st);                                                      \
        if (const int _rc = (__VA_ARGS__)) return _rc;                                         \
    } while (0)
#define T2S_TIMED_LAUNCH(h, cls, st, ...)                                                      \
    do {                                                                                       \
        ::t2s::TimeScope _ts(h, cls, st);                                                      \
        __VA_ARGS__;                                                                           \
        T2S_LAUNCH_CHECK();                                                                    \
    } while (0)

// t2s_attn.hip
int attn_init();
int launch_attn_packed(const float* q, const float* k, const float* vT, float* o, int BH, hipStream_t st);
int launch_attn_packed_n(const float* q, const float* k, const float* vT, float* o, int BH, int n_tok, hipStream_t st);
// t2s_attn_x3.hip; np = 3: bf16x3, np = 1: bf16 (k / vT: np planes)
int attn_xn_init(int np);
int launch_attn_xn(int np, const float* q, const __bf16* k, const __bf16* vT, float* o, int BH, int n_tok, hipStream_t st);
// t2s_dit.hip
int dit_forward_cfg_step(t2s_dit* h, const float* x, const float* temb_table, const int* step_ptr,
                         const float* text, float* out_u, float* out_c, int B, hipStream_t st, int ws_seq0,
                         const float* mod_table, int mod_rows, int mod_row0);
int dit_forward_cond_step(t2s_dit* h, const float* x, const float* temb_table, const int* step_ptr, const float* text,
                          float* out, int B, hipStream_t st, int ws_seq0, const float* mod_table, int mod_rows, int mod_row0);
int dit_adaln_table(t2s_dit* h, const float* temb_table, int steps, const float* text, int B, float* table, hipStream_t st);
// t2s_sampler.hip: the library's non-blocking set-up stream and per-device run lock (t2s_sampler_create)
hipStream_t lib_setup_stream(int dev);
std::recursive_mutex* lib_pool_lock(int dev);
// t2s_train.hip
void train_free(t2s_dit* h);
}  // namespace t2s
