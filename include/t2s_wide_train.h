/* libt2s_hip.so -- training at the WIDE latent widths (the T2MS motion denoisers, reference mytrain.py): the two entries
 * that opt a t2s_dit_create_w handle into the fp32 training step of t2s.h and test its attention alone.  An extension of
 * t2s.h: that header's entry list stays as it is; t2ms_amd/_lib.py lists these under SYMBOLS_WIDE_TRAIN. */
#ifndef T2S_WIDE_TRAIN_H
#define T2S_WIDE_TRAIN_H

#include "t2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opt a WIDE handle into training (the reference's mytrain.py): with on != 0, t2s_dit_set_train_dtype(T2S_TRAIN_F32),
 * t2s_dit_train_forward / _backward / _input_grad and the training classes of t2s_dit_timing_* accept it and run the fp32
 * step at 16*latent_w tokens (chunked attention kernels, run-time geometry; results repeat bit for bit from run to run).
 * T2S_TRAIN_BF16 stays T2S_E_INVALID with a message at a wide width (t2s_wide_train_bf16.h holds the opt-in that lifts this), and
 * there is no ragged backward.  on == 0 restores the
 * refusals.  A width-30 handle always trains: T2S_OK, nothing changes. */
int t2s_dit_set_trainable(t2s_dit* h, int on);

/* t2s_attn_train (t2s.h) with n_tok tokens per sequence in place of 480 (the launchers of a wide handle's training step): n_tok 480,
 * 800 or 1024, anything else is T2S_E_INVALID with a message; dtype must be T2S_TRAIN_F32 unless n_tok == 480.  At 480
 * it gives the bits of t2s_attn_train. */
int t2s_attn_train_n(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows,
                     float* lse, float* dqkv_rows, int n_seq, int n_tok, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* T2S_WIDE_TRAIN_H */
