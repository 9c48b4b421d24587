/* libt2s_hip.so -- the bf16x3 and bf16 arithmetics at the WIDE latent widths (the T2MS motion denoisers at 800 / 1024
 * tokens): the entry that opts a t2s_dit_create_w handle into them and the stand-alone entries of their attention at a
 * run-time token count.  An extension of t2s.h: that header's entry list stays as it is; t2ms_amd/_lib.py lists these under
 * SYMBOLS_WIDE_MATH. */
#ifndef T2S_WIDE_MATH_H
#define T2S_WIDE_MATH_H

#include "t2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opt a WIDE handle into the bf16 arithmetics of the inference forward: with on != 0, t2s_dit_set_math accepts
 * T2S_MATH_BF16X3 and T2S_MATH_BF16 on it (the plane workspaces are allocated on a mode's first use, sized by the handle's
 * token count) and the forwards, CFG passes and samplers over the handle run the wide row-chain and attention kernels of that
 * arithmetic.  on == 0 restores the refusal of t2s_dit_set_math and puts the handle back on T2S_MATH_F32.  Training is not
 * affected: T2S_TRAIN_BF16 stays T2S_E_INVALID at a wide width.  A width-30 handle: T2S_OK, nothing changes. */
int t2s_dit_set_wide_math(t2s_dit* h, int on);

/* t2s_attn_fwd_x3 / t2s_attn_fwd_bf16p (t2s.h) on plain (BH, n_tok, 32) tensors with n_tok tokens per sequence in place of
 * 480: n_tok 480, 800 or 1024, anything else is T2S_E_INVALID with a message.  At 480 they give the bits of those entries;
 * at 800 / 1024 they run the attention kernel of a wide handle's forward. */
int t2s_attn_fwd_x3_n(const float* q, const float* k, const float* v, float* o, int BH, int n_tok, void* stream);
int t2s_attn_fwd_bf16p_n(const float* q, const float* k, const float* v, float* o, int BH, int n_tok, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* T2S_WIDE_MATH_H */
