/* libt2s_hip.so -- the row kernels of the DiT training step, one launch form at a time: for tests / benchmarking of those
 * kernels.  t2s_train_rows runs ONE launch form of t2s_dit_train_forward / _backward (the fused row GEMMs of both arithmetics
 * with their prologues and epilogues, the fp32 step's elementwise / per-sequence kernels, the final-layer backward) alone, on
 * caller buffers, through the host helpers the training recipes themselves launch with -- no kernel of its own.  Nothing of
 * the product path calls it.  An extension of t2s.h in the way of t2s_wide_train_bf16.h: that header's entry list stays as it
 * is; t2ms_amd/_lib.py lists this one under SYMBOLS_TRAIN_ROWS. */
#ifndef T2S_TRAIN_ROWS_H
#define T2S_TRAIN_ROWS_H

#include "t2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launch forms.  M = n_seq * n_tok rows; "rows" are row-major (M, width); W is a Linear's weight (N, K) row-major and the
 * product is pro(a) W^T + bias (a data-gradient form takes the TRANSPOSED Linear weight as its W); bias may be NULL.
 * T2S_TRAIN_BF16 forms (t2s_bf16.h bgemm_kernel<K, N, PRO, EPI>; 800 / 1024 tokens: the run-time TOK = 0 forms): */
enum {
    T2S_ROWS_QKV0 = 0,        /* <128,384,LN,QKV>      a = x (M,128) fp32, mod -> q (pre-scaled), k, v heads; save_a = a1 */
    T2S_ROWS_QKV1 = 1,        /* <128,384,LN_RES,QKV>  x = a + mod[gate_off] * res first: also x_out */
    T2S_ROWS_FC1 = 2,         /* <128,256,LN_RES,BF16> -> out = u (M,256), save_a = a2, x_out */
    T2S_ROWS_FC2 = 3,         /* <256,128,GELU,BF16>   a = u (M,256) -> out (M,128) */
    T2S_ROWS_LIN128 = 4,      /* <128,128,BF16,BF16>   a (M,128) -> out (M,128): proj forward, the `do` data gradient */
    T2S_ROWS_GELUBWD = 5,     /* <128,256,BF16,GELUBWD> a (M,128), aux = u (M,256) -> out = (a W^T) gelu'(u) */
    T2S_ROWS_LNBWD256 = 6,    /* bgemm_lnbwd<256>: a = dY (M,256), ln_x, mod[scale_off]; dx (M,128) is READ and written; */
    T2S_ROWS_LNBWD384 = 7,    /* bgemm_lnbwd<384>:   dmod[shift_off | scale_off]; with res (f_next) also out = t_next, dmod[gate_off] */
    T2S_ROWS_FINAL_FUSED = 8, /* final_bwd_kernel<true,..> + tail_reduce + final_gate_reduce: a = x_mid, res = f, dout, ln_w, ln_b,
                                 w = linear_emb_to_patch.weight (4,128) -> dx, out = t, dmod[gate_off], g_ln_w, g_ln_b, g_out_w, g_out_b */
    /* T2S_TRAIN_F32 forms (t2s_gemm.h gemm_rows_kernel<K, NT, PRO, EPI> and the kernels of t2s_train.hip): */
    T2S_ROWS_F_QKV = 16,      /* <128,3,LNMOD,QKV>     a = x, mod -> q, k, v heads; save_a */
    T2S_ROWS_F_FC1 = 17,      /* <128,2,LNMOD,BIAS>    -> out (M,256); save_a */
    T2S_ROWS_F_FC2 = 18,      /* <256,1,GELU,BIAS>     a (M,256) -> out (M,128) */
    T2S_ROWS_F_LIN128 = 19,   /* <128,1,PLAIN,BIAS>    a (M,128) -> out (M,128) */
    T2S_ROWS_F_LIN256 = 20,   /* <256,1,PLAIN,BIAS>    a (M,256) -> out (M,128) */
    T2S_ROWS_F_LIN384 = 21,   /* <384,1,PLAIN,BIAS>    a (M,384) -> out (M,128) */
    T2S_ROWS_F_GELUBWD = 22,  /* <128,2,PLAIN,GELUBWD> a (M,128), aux = u (M,256) -> out (M,256) */
    T2S_ROWS_F_GATE_RES = 23, /* gate_res_kernel:      x_out = a + mod[gate_off] * res */
    T2S_ROWS_F_GATE_BWD = 24, /* gate_bwd_kernel:      out = mod[gate_off] * dx, dmod[gate_off] = sum_tok dx * res (dx is read only) */
    T2S_ROWS_F_LN_MOD_BWD = 25, /* ln_mod_bwd_kernel with f_next == NULL, as the recipe calls it: a = da, ln_x, mod[scale_off];
                                   dx is READ and written; dmod[shift_off | scale_off] */
    T2S_ROWS_F_GELU = 26,     /* gelu_kernel:          a (M,256) -> out (M,256) */
    T2S_ROWS_F_FINAL = 27     /* final_bwd_kernel<false,..> + tail_reduce: as FINAL_FUSED without res / mod / out / dmod; a = the layer input */
};

/* Device pointers, all fp32.  A form reads and writes only what its line above names; the rest may be NULL.  The adaLN
 * offsets are columns of a (n_seq, 3072) mod / dmod row: multiples of 4 in [0, 3072 - 128]. */
typedef struct t2s_train_rows_args {
    const float* a;
    const float* w;
    const float* bias;
    const float* mod;
    const float* res;
    const float* aux;
    const float* ln_x;
    const float* dout;      /* FINAL_*: (n_seq, 64, n_tok / 16) */
    const float* ln_w;      /* FINAL_*: (128) */
    const float* ln_b;
    float* out;
    float* save_a;
    float* x_out;
    float* q;               /* heads (n_seq * 4, n_tok, 32) */
    float* k;
    float* v;
    float* dx;
    float* dmod;
    float* g_ln_w;          /* FINAL_*: (128) (128) (4,128) (4) */
    float* g_ln_b;
    float* g_out_w;
    float* g_out_b;
    int shift_off;
    int scale_off;
    int gate_off;
} t2s_train_rows_args;

/* Runs launch form `op` in arithmetic `dtype` (T2S_TRAIN_F32 / T2S_TRAIN_BF16; each form exists in one of them) on n_seq
 * sequences of n_tok tokens: 480, 800 or 1024, anything else is T2S_E_INVALID with n_tok=<n> in the message.  In
 * T2S_TRAIN_BF16 the operands the step keeps in bf16 (a unless it is the fp32 residual stream, res, aux) are rounded to bf16
 * on the way in, the weight is packed as bf16, and bf16 results (out, save_a, q, k, v) are widened on the way out; x, mod,
 * bias, dx, dmod and the final layer's tensors are fp32 in both arithmetics.  flags bit 1 (value 2): the persistent GEMMs walk
 * their tiles descending, as every second launch of a training step does (as t2s_wgrad's bit 1); no other bit is defined.
 * Allocates its own temporaries and synchronises the stream before it returns.  A bad argument is T2S_E_INVALID with the
 * argument's name in t2s_last_error(), before anything is launched. */
int t2s_train_rows(int op, int dtype, int n_tok, int n_seq, int flags, const t2s_train_rows_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* T2S_TRAIN_ROWS_H */
