/* libt2s_hip.so -- bf16 mixed-precision training at the WIDE latent widths (the T2MS motion denoisers, reference mytrain.py):
 * the two entries that opt a trainable t2s_dit_create_w handle into the T2S_TRAIN_BF16 step of t2s.h and test its attention
 * alone.  An extension of t2s.h and t2s_wide_train.h: those headers' entry lists stay as they are; t2ms_amd/_lib.py lists
 * these under SYMBOLS_WIDE_TRAIN_BF16. */
#ifndef T2S_WIDE_TRAIN_BF16_H
#define T2S_WIDE_TRAIN_BF16_H

#include "t2s_wide_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opt a WIDE handle into the bf16 training step: with on != 0 AND t2s_dit_set_trainable on, t2s_dit_set_train_dtype accepts
 * T2S_TRAIN_BF16, and t2s_dit_train_forward / _backward / _input_grad then run the mixed-precision step of train.py --bf16 at
 * 16*latent_w tokens (bf16 MFMA operands and saved activations; fp32 accumulate, master weights, residual stream, statistics
 * and gradients; results repeat bit for bit from run to run).  The two switches may be set in either order.  With on == 0
 * every return code and message is what it is without this header, and a handle that was on T2S_TRAIN_BF16 goes back to
 * T2S_TRAIN_F32 (its next forward rebuilds the workspace).  A NULL handle is T2S_E_INVALID.  A width-30 handle has always had
 * both arithmetics: T2S_OK, nothing changes. */
int t2s_dit_set_wide_train_bf16(t2s_dit* h, int on);

/* t2s_attn_train_n (t2s_wide_train.h) in T2S_TRAIN_BF16 at every built token count (the launchers of a wide handle's bf16
 * training step): same arguments without the dtype; n_tok 480, 800 or 1024, anything else is T2S_E_INVALID with n_tok=<n> in
 * the message.  The fp32 arguments are rounded to bf16 (q pre-scaled by log2(e)/sqrt(32)) as t2s_attn_train does.  At 480 it
 * gives the bits of t2s_attn_train(..., T2S_TRAIN_BF16).  t2s_attn_train_n keeps refusing T2S_TRAIN_BF16 at 800 / 1024. */
int t2s_attn_train_bf16_n(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows,
                          float* lse, float* dqkv_rows, int n_seq, int n_tok, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* T2S_WIDE_TRAIN_BF16_H */
