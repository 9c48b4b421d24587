/*
 * t2s.h -- C ABI of libt2s_hip.so: the MI355X (gfx950) implementation of the
 * T2S diffusion hot path of Bill9125/T2MS.
 *
 * The reference has no FFI layer: its boundary is a set of Python classes
 * (SURVEY.md section 8b).  The host-side mirrors of those classes live in
 * t2ms_amd/model/... and call the entry points below through ctypes; each
 * entry point cites the reference interface it replaces (paths relative to
 * the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *     tensors are dense, row-major fp32 in exactly the reference's layout;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     no entry point synchronises the device or allocates in the launch path
 *     (so callers may capture them into a hipGraph); only *_create/_destroy
 *     allocate / free;
 *   - return value: 0 on success, negative T2S_E_* on failure, with a
 *     human-readable message available from t2s_last_error();
 *   - the caller owns every buffer it passes in; the library owns only its
 *     packed weight copies, workspaces and hipGraph handles;
 *   - threads: a handle (t2s_dit, t2s_vae, t2s_sampler) is driven by ONE thread at a
 *     time -- a t2s_sampler together with the t2s_dit it was created on (it runs in
 *     that handle's workspace).  Different handles may be driven by different threads
 *     of one process on one device (what the library serialises for them: "Threads"
 *     at t2s_sampler_run).  The handle-free entry points (t2s_ddpm_*, t2s_rf_*,
 *     t2s_philox_*, t2s_mse_ws, t2s_mse_backward, t2s_adamw_*, t2s_attn_fwd*,
 *     t2s_time_embedding_freqs, t2s_eval_*, t2s_ts2vec_encode, t2s_mlp_*) keep no state between
 *     calls and may be called from any thread on any stream; t2s_mse lends a scratch
 *     per (device, stream), see there.  The deployment model is one process per GPU.
 */
#ifndef T2S_H
#define T2S_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2S_OK 0
#define T2S_E_INVALID (-1)  /* bad argument (shape, NULL, range)          */
#define T2S_E_HIP (-2)      /* a HIP runtime call failed                  */
#define T2S_E_STATE (-3)    /* handle not in a state that allows the call */

#define T2S_D_MODEL 128
#define T2S_N_TOK 480  /* (30/2) * (64/2) patches, transformer.py:132-136 */
#define T2S_N_HEADS 4
#define T2S_HEAD_DIM 32
#define T2S_N_BLOCKS 4
#define T2S_LAT_C 64
#define T2S_LAT_W 30
#define T2S_LAT_ELEMS (T2S_LAT_C * T2S_LAT_W)

const char* t2s_last_error(void);
/* library build id + the gfx arch it was compiled for, e.g. "t2s 0.1 gfx950" (host string) */
const char* t2s_version(void);

/* ------------------------------------------------------------------------ *
 * DiT denoiser: model/denoiser/transformer.py:128-193 (Transformer),
 * :94-124 (Transformerlayer), timm 1.0.11 Attention/Mlp call sites :104-105.
 * ------------------------------------------------------------------------ */
typedef struct t2s_dit t2s_dit;

/* Device pointers to the reference state-dict tensors. */
typedef struct t2s_dit_block_weights {
    const float* qkv_w;  /* layers.i.attn.qkv.weight            (384,128) */
    const float* qkv_b;  /* layers.i.attn.qkv.bias              (384)     */
    const float* proj_w; /* layers.i.attn.proj.weight           (128,128) */
    const float* proj_b; /* layers.i.attn.proj.bias             (128)     */
    const float* fc1_w;  /* layers.i.mlp.fc1.weight             (256,128) */
    const float* fc1_b;  /* layers.i.mlp.fc1.bias               (256)     */
    const float* fc2_w;  /* layers.i.mlp.fc2.weight             (128,256) */
    const float* fc2_b;  /* layers.i.mlp.fc2.bias               (128)     */
    const float* ada_w;  /* layers.i.adaLN_modulation.1.weight  (768,128) */
    const float* ada_b;  /* layers.i.adaLN_modulation.1.bias    (768)     */
} t2s_dit_block_weights;

typedef struct t2s_dit_weights {
    const float* conv_w;    /* conv.weight                (4,1,2,2) */
    const float* conv_b;    /* conv.bias                  (4)       */
    const float* patch_w;   /* patch_emb.weight           (128,4)   */
    const float* patch_b;   /* patch_emb.bias             (128)     */
    const float* pos_embed; /* pos_embed                  (1,480,128) */
    const float* ln_w;      /* ln.weight                  (128)     */
    const float* ln_b;      /* ln.bias                    (128)     */
    const float* out_w;     /* linear_emb_to_patch.weight (4,128)   */
    const float* out_b;     /* linear_emb_to_patch.bias   (4)       */
    const float* time_freqs; /* 10000^linspace(0,1,64), transformer.py:34 (64) */
    t2s_dit_block_weights blk[T2S_N_BLOCKS];
} t2s_dit_weights;

/* Create a denoiser able to run up to `max_seqs` sequences per call (a CFG
 * sampling step over a batch of B series uses 2*B sequences).  Packs the
 * weights into the kernels' MFMA-fragment layout (synchronous). */
int t2s_dit_create(const t2s_dit_weights* w, int max_seqs, t2s_dit** out);
/* The same denoiser over a WIDE latent (the T2MS motion models, model/denoiser/mytransformer.py Transformer(dim)): the latent
 * is (64, latent_w), patchified 2x2 into 16*latent_w tokens -- latent_w 30 (480 tokens; this IS t2s_dit_create), 50 (800,
 * the deadlift model) or 64 (1024, the bench-press model); anything else is T2S_E_INVALID with a message.  The weights are
 * those of t2s_dit_weights except pos_embed, which holds 16*latent_w*128 floats (an undersized one is T2S_E_INVALID naming
 * "pos_embed").  On such a handle every entry below takes and gives (S,64,latent_w) latents and (S,16*latent_w,128) token
 * streams.  A handle with latent_w != 30 runs T2S_MATH_F32, and inference only until t2s_dit_set_trainable (t2s_wide_train.h)
 * switches training on: t2s_dit_set_math(T2S_MATH_BF16X3 / _BF16) returns T2S_E_INVALID with a message unless
 * t2s_dit_set_wide_math (t2s_wide_math.h) opted the handle in, and so do t2s_dit_set_train_dtype and
 * every t2s_dit_train_* entry on a handle without the switch, before any launch. */
int t2s_dit_create_w(const t2s_dit_weights* w, int latent_w, int max_seqs, t2s_dit** out);
/* latent width of a handle (30 for t2s_dit_create); 0 for NULL */
int t2s_dit_latent_w(const t2s_dit* h);
/* t2s_dit_weights is T2S_DIT_N_TENSORS device pointers: 10 top-level fields in declaration order, then the 10 fields of each
 * of the 4 blocks.  The ABI carries no sizes, so: n_floats[i] (HOST array, n_entries == T2S_DIT_N_TENSORS, or NULL) = the
 * number of floats the caller holds behind pointer i; the call returns T2S_E_INVALID -- naming the tensor by its state-dict
 * key -- when one is NULL, holds fewer floats than the kernels read (the shapes in the struct comments above), or lies in a
 * device allocation that ends before those floats do (hipMemGetAddressRange; pointers HIP cannot place are passed through).
 * t2s_dit_create and t2s_dit_update_weights run the allocation-extent part themselves: an undersized buffer is an error
 * code, never a memory fault.  The host mirror calls this with the numel() of every parameter before it hands a new struct over. */
#define T2S_DIT_N_TENSORS (10 + 10 * T2S_N_BLOCKS)
int t2s_dit_weights_check(const t2s_dit_weights* w, const uint64_t* n_floats, int n_entries);
/* The same check for a handle of t2s_dit_create_w: pos_embed must hold 16*latent_w*128 floats (latent_w 30, 50 or 64). */
int t2s_dit_weights_check_w(const t2s_dit_weights* w, int latent_w, const uint64_t* n_floats, int n_entries);
/* Re-pack after the caller changed the weights (load_state_dict, optimizer step). */
int t2s_dit_update_weights(t2s_dit* h, const t2s_dit_weights* w, void* stream);
void t2s_dit_destroy(t2s_dit* h);
int t2s_dit_max_seqs(const t2s_dit* h);
/* Matrix arithmetic of t2s_dit_forward[_cfg] / the sampler (attention and the row chain; the adaLN
 * linear and the small layers always run in f32).
 *   T2S_MATH_F32 (a new handle's mode)  v_mfma_f32_32x32x2_f32: exact fp32 multiply-add chains.
 *   T2S_MATH_BF16X3         every fp32 operand split into three bf16 terms, each product evaluated as
 *                           the six bf16 MFMAs of weight >= 2^-16 with fp32 accumulation: the same
 *                           accuracy as an fp32 product (dropped terms <= 3 * 2^-24 relative; measured
 *                           against fp64 the attention kernel is as close as the f32 one) at 2.67x
 *                           fewer matrix cycles.  Allocates 2 x max_seqs x 368,640 B + 3.1 MB of split
 *                           weights on first use and packs them on the library's own set-up stream, under the per-device
 *                           lock of t2s_sampler_run ("Threads") and behind the last t2s_dit_update_weights, whatever
 *                           stream that ran on; a first use that fails leaves the handle as it was.  Weights follow
 *                           t2s_dit_update_weights.
 *                           Since round 5 the host-side Sampler and infer.py SELECT this mode unless told otherwise
 *                           (its error against fp64 is not larger than the reference's own CPU fp32 arithmetic at any of
 *                           17 table entries, profiles/r05_accuracy.md); the class API and the bench headline stay on F32.
 *   T2S_MATH_BF16           single-pass bf16 mixed precision (opt-in; NOT fp32-accurate).  The operands of every matrix
 *                           product of the DiT forward (qkv, QK^T, PV, proj, fc1, fc2) are rounded ONCE to bf16, round to
 *                           nearest even, and multiplied by one v_mfma_f32_32x32x16_bf16 per k-step with fp32 accumulation.
 *                           Where the operands are rounded: weights when they are packed; LayerNorm / adaLN-modulated
 *                           activations, the attention output and GELU(fc1) in registers in front of their product; k and v
 *                           after their bias, as they leave the qkv epilogue; q AFTER its fp32 multiplication by
 *                           32^-0.5 * log2(e) (q itself travels in fp32); the exponentiated scores P = exp2(s - ref) in front
 *                           of PV -- the running row sum adds the unrounded P.
 *                           Everything else is fp32 exactly as in the other modes: the residual stream (also in memory),
 *                           LayerNorm and adaLN modulation, the softmax reference / exponent / running sum, GELU, biases,
 *                           the final layer, patchify, the time embedding, the adaLN table, the CFG combine, the DDPM / RF
 *                           update, the Philox noise and the LA-VAE.  This is the contract of the training step's
 *                           T2S_TRAIN_BF16.  Allocates 2 x max_seqs x 122,880 B + 1.0 MB of bf16 weights on first use, by
 *                           the same path as T2S_MATH_BF16X3; weights follow t2s_dit_update_weights.  Errors against fp64:
 *                           rms ~1e-3 on outputs of magnitude ~4.5 per forward, a quarter of what PyTorch's bf16 autocast
 *                           makes of the same forward (tests/test_math_bf16.py).
 * Not capturable; a hipGraph captured under one mode keeps replaying that mode's kernels.  Each mode has a workspace of
 * its own, so a handle may be switched back and forth. */
#define T2S_MATH_F32 0
#define T2S_MATH_BF16X3 1
#define T2S_MATH_BF16 2
int t2s_dit_set_math(t2s_dit* h, int math);

/* TimeEmbedding.forward, transformer.py:30-40.  t: (B) fp32 (int64 timesteps are
 * converted to fp32 by the host mirror exactly as `t * 100.0` promotes them);
 * out: (B,128) = [sin(100 t / f) | cos(100 t / f)]. */
int t2s_time_embedding(const t2s_dit* h, const float* t, float* out, int B, void* stream);
/* The same without a handle (the module TimeEmbedding is parameter-free, transformer.py:25-40): freqs (64) =
 * 10000^linspace(0,1,64) as the caller evaluated it (the host mirror uses the reference's own fp32 torch ops, :34). */
int t2s_time_embedding_freqs(const float* freqs, const float* t, float* out, int B, void* stream);

/* Transformer.forward, transformer.py:158-193.
 *   x    (B,64,30)   latent
 *   temb (temb_rows,128), temb_rows in {1,B}: output of t2s_time_embedding
 *   text (B,128) or NULL (text_input=None -> unconditional)
 *   out  (B,64,30)
 * B <= max_seqs. */
int t2s_dit_forward(t2s_dit* h, const float* x, const float* temb, int temb_rows,
                    const float* text, float* out, int B, void* stream);

/* Both classifier-free-guidance branches of one sampling step in ONE pass
 * (infer.py:79-80 / 85-86): sequences [0,B) are the unconditional branch
 * (c = temb), [B,2B) the conditional one (c = temb + text); both read x[b].
 *   temb (1,128); out_uncond, out_cond (B,64,30).  2*B <= max_seqs. */
int t2s_dit_forward_cfg(t2s_dit* h, const float* x, const float* temb, const float* text,
                        float* out_uncond, float* out_cond, int B, void* stream);
/* The same pass with one time-embedding row PER series (temb_rows == B; 1 = shared): what the pair of calls
 * `model(x_t, t, None)`, `model(x_t, t, emb)` at infer.py:79-80 / 85-86 computes for a per-row t.  The class-API mirror
 * runs such a pair as ONE pass once it has seen the pattern (t2ms_amd/model/denoiser/transformer.py) -- speculation on
 * torch tensor identity, which cannot see a raw-pointer write: a caller that updates x_t IN PLACE through this ABI
 * (t2s_ddpm_step, t2s_rf_step) between the two calls of a mirror Transformer switches the pairing off
 * (Transformer.set_pairing(False), or T2S_NO_PAIRING=1 in the environment). */
int t2s_dit_forward_cfg_rows(t2s_dit* h, const float* x, const float* temb, int temb_rows, const float* text,
                             float* out_uncond, float* out_cond, int B, void* stream);

/* In-situ kernel timing with HIP events recorded on the launching stream around every launch of
 * the forward (not usable while the stream is being captured).  _begin arms it; after running
 * forwards, _end synchronises and returns {attention ms, attention launches, row-chain ms,
 * row-chain launches, other ms, other launches} in out6 and disarms it. */
int t2s_dit_timing_begin(t2s_dit* h);
int t2s_dit_timing_end(t2s_dit* h, double* out6);
/* The same with the launches of the training step (t2s_dit_train_forward / _backward) in classes 3..8: out holds
 * n_classes pairs {ms, launches}: 0 attention, 1 row chain, 2 other (inference forward); 3 streaming GEMMs / fused row
 * kernels, 4 attention forward, 5 attention backward, 6 weight gradients, 7 gate / LayerNorm elementwise kernels,
 * 8 everything else of the step (packs, patchify, final layer, adaLN linear); 9 / 10 the first (block 0's qkv with the
 * patchify prologue) and the last (block 3's proj + MLP with the final layer) row-chain launch of an inference forward,
 * which class 1 contains as well.  n_classes <= 11. */
int t2s_dit_timing_end_ex(t2s_dit* h, double* out, int n_classes);

/* Test tap: copy out the residual stream (S,480,128) the last forward left in the
 * workspace (post block 3, before the final LayerNorm).  Used by tests to bisect. */
int t2s_dit_read_stream(const t2s_dit* h, float* out, int S, void* stream);

/* Fused softmax(q k^T / sqrt(32)) v for N=480, head_dim=32 (timm Attention.forward
 * core; call site transformer.py:116).  q,k,v: (BH,480,32); o: (BH,480,32). */
int t2s_attn_fwd(const float* q, const float* k, const float* v, float* o, int BH, void* stream);
/* The same attention on the library's internal "fragment-major" tensors -- the kernel the DiT
 * forward actually launches (exposed for benchmarking / tests).  With tile = row/32, i = row%32,
 * a (480,32) per-head matrix X is stored as float4 fragments
 *     P[((tile*4 + g)*64 + 32*h + i)*4 + e] = X[32*tile + i][8*g + 4*h + e]
 * q, k: P of the head's Q and K;  vT: P of V TRANSPOSED, i.e.
 *     vT[((tile*4 + g)*64 + 32*h + d)*4 + e] = V[32*tile + 8*g + 4*h + e][d];
 * heads ordered (seq*4 + head).  o: (n_seq*480, 128) with
 *     o[(((row/32)*16 + G)*64 + 32*h + row%32)*4 + e] = O[row][8*G + 4*h + e]  (G = col/8). */
int t2s_attn_fwd_packed(const float* q, const float* k, const float* vT, float* o, int n_seq,
                        void* stream);
/* The same fragment-major contract for a sequence of n_tok tokens, n_tok = 480, 800 or 1024 (n_tok/32 tiles per head; q, k,
 * vT: (n_seq*4, n_tok, 32) per head, o: (n_seq*n_tok, 128)).  At 480 it launches what t2s_attn_fwd_packed launches; at 800 /
 * 1024 the packed kernel's body over 25 / 32 key blocks, four workgroups per head (the wide DiT's attention). */
int t2s_attn_fwd_packed_n(const float* q, const float* k, const float* vT, float* o, int n_seq, int n_tok, void* stream);

/* The "bf16x3" attention kernel (T2S_MATH_BF16X3, see t2s_dit_set_math) on plain tensors: same
 * contract as t2s_attn_fwd (q, k, v, o: (BH, 480, 32) fp32, BH a multiple of 4), fp32-accurate
 * products evaluated as six bf16 MFMAs each.  Packs / unpacks its operands internally and
 * synchronises the stream (tests, benchmarking). */
int t2s_attn_fwd_x3(const float* q, const float* k, const float* v, float* o, int BH, void* stream);

/* The one-plane bf16 attention kernel (T2S_MATH_BF16) on plain tensors, same calling contract as t2s_attn_fwd_x3.
 * (Not t2s_attn_fwd_bf16: that is the training kernel, with bf16 operands in memory.)  It computes
 *     O = sum_j rb(P_j) rb(v_j) / sum_j P_j,   P_j = exp2(rb(q * c) . rb(k_j) - ref),   c = 32^-0.5 * log2(e),
 * rb = round to nearest even bf16, q * c one fp32 multiplication, products exact in fp32 accumulators. */
int t2s_attn_fwd_bf16p(const float* q, const float* k, const float* v, float* o, int BH, void* stream);

/* ------------------------------------------------------------------------ *
 * Training step of the DiT: train.py:101-127 (pred = model(x_t, t, emb); loss.backward();
 * optimizer.step()).  The host mirror wraps these in a torch.autograd.Function.
 * ------------------------------------------------------------------------ */
typedef struct t2s_dit_block_grads { /* same shapes as t2s_dit_block_weights */
    float *qkv_w, *qkv_b, *proj_w, *proj_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ada_w, *ada_b;
} t2s_dit_block_grads;
typedef struct t2s_dit_grads { /* every tensor that receives a gradient (925,592 values) */
    float *conv_w, *conv_b, *patch_w, *patch_b, *ln_w, *ln_b, *out_w, *out_b;
    t2s_dit_block_grads blk[T2S_N_BLOCKS];
} t2s_dit_grads;

/* Arithmetic of the training path.  T2S_TRAIN_F32 (default): fp32 end to end, gradients equal
 * autograd through the fp32 reference to ~1e-6 relative.  T2S_TRAIN_BF16 (BASELINE config 4,
 * "train.py bf16"): every contraction on bf16 MFMA with fp32 accumulation, saved activations in
 * bf16; master weights, residual stream, LayerNorm / softmax statistics, gradients and the
 * optimizer stay fp32.  Takes effect at the next t2s_dit_train_forward. */
#define T2S_TRAIN_F32 0
#define T2S_TRAIN_BF16 1
int t2s_dit_set_train_dtype(t2s_dit* h, int dtype);
/* Transformer.forward that keeps the activations for a following backward (plain layouts).
 * `w` are the caller's CURRENT weights (call t2s_dit_update_weights first if they changed since
 * the handle was created/updated); arguments otherwise as t2s_dit_forward.  Allocates its
 * workspace on first use (not capturable). */
int t2s_dit_train_forward(t2s_dit* h, const t2s_dit_weights* w, const float* x, const float* temb,
                          int temb_rows, const float* text, float* out, int B, void* stream);
/* The attention forward of the T2S_TRAIN_BF16 path on fp32 buffers (converted to bf16 on the way
 * in, back on the way out; synchronises the stream): q, k, v (n_seq*4, 480, 32) heads ->
 * o_rows (n_seq*480, 128) token rows, lse (n_seq*4, 480) = log2-domain log-sum-exp of the scaled
 * scores.  For tests / benchmarking of that kernel (incl. its stale-reference branch). */
int t2s_attn_fwd_bf16(const float* q, const float* k, const float* v, float* o_rows, float* lse,
                      int n_seq, void* stream);
/* The attention of the training path alone, forward then backward, on fp32 buffers: exactly the kernels
 * t2s_dit_train_forward / t2s_dit_train_backward launch for one block, through the same host launchers.
 * q, k, v (n_seq*4, 480, 32) heads, UNSCALED; do_rows, o_rows (n_seq*480, 128) token rows, head h at columns
 * 32h..32h+31; lse (n_seq*4, 480) log2-domain log-sum-exp of the scaled scores; dqkv_rows (n_seq*480, 384) =
 * [dq | dk | dv], the gradient with respect to the unscaled q, k, v.  dtype T2S_TRAIN_F32 or T2S_TRAIN_BF16; bf16
 * converts on the way in (q times 32^-0.5 log2(e) before the rounding, as the qkv GEMM's epilogue stores it; k, v, dO
 * rounded) and back on the way out.  Allocates its temporaries and synchronises the stream.  For tests /
 * benchmarking of those kernels. */
int t2s_attn_train(const float* q, const float* k, const float* v, const float* do_rows, float* o_rows,
                   float* lse, float* dqkv_rows, int n_seq, int dtype, void* stream);
/* The weight-gradient kernels of the training path (and of the LA-VAE backwards) alone, on fp32 buffers:
 * dW (N,K) = dY^T X over the M rows of dY (M,N) and X (M,K), db (N) = column sums of dY (db may be NULL).
 * N % 128 == 0, K % 128 == 0, M > 0.  dtype T2S_TRAIN_F32 (the exact-fp32 kernel) or T2S_TRAIN_BF16 (operands
 * rounded to bf16 on the way in, fp32 accumulation).  flags bit 0: the X operand is gelu(X), applied after the rounding
 * and rounded again (the fc2 weight gradient; bf16 only).  flags bit 1: walk the row slabs in reverse (bf16; the fp32
 * kernel has no direction).  Allocates its temporaries and synchronises the stream.  For tests / benchmarking of
 * those kernels. */
int t2s_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, int dtype,
              int flags, void* stream);
/* Backward of the last t2s_dit_train_forward: dout (B,64,30) = dLoss/dout; writes (overwrites)
 * every gradient tensor of `g`.  Every gradient is reduced in a fixed order (bit-reproducible from run to run): the block
 * weights / biases per row slab in slab order, the small final-layer and patchify gradients (ln, linear_emb_to_patch,
 * patch_emb, conv) per workgroup in workgroup order. */
int t2s_dit_train_backward(t2s_dit* h, const float* dout, const t2s_dit_grads* g, int B, void* stream);
/* The gradient with respect to the denoiser's INPUT latent, dinput (B,64,30) (patchify backwards, transformer.py:166-172), after
 * t2s_dit_train_backward of the same batch.  train.py needs it only when something upstream of the latent trains: the LA-VAE
 * encoder un-frozen (train.py:31-33, `usepretrainedvae` false). */
int t2s_dit_train_input_grad(t2s_dit* h, float* dinput, int B, void* stream);
/* One fused AdamW update (torch.optim.AdamW semantics; train.py:37 uses lr 1e-4, weight_decay 0):
 * p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).  step >= 1. */
int t2s_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   void* stream);
/* The same update for up to 64 tensors in ONE launch (the DiT has 48 trainable tensors).  table_dev: device array
 * of n_tensors entries; total_chunks = sum over entries of ceil(n / 1024).  All entries share lr / betas / eps /
 * weight_decay / step. */
typedef struct t2s_adamw_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t n;
} t2s_adamw_tensor;
int t2s_adamw_step_multi(const t2s_adamw_tensor* table_dev, int n_tensors, uint64_t total_chunks, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* Backward of t2s_mse: da = 2 (a-b) g / n, db = -da (either may be NULL); grad_out: device scalar. */
int t2s_mse_backward(const float* a, const float* b, const float* grad_out, float* da, float* db,
                     uint64_t n, void* stream);

/* ------------------------------------------------------------------------ *
 * Diffusion backbones: model/backbone/DDPM.py, model/backbone/rectified_flow.py
 * ------------------------------------------------------------------------ */
/* DDPM.p_sample (DDPM.py:28-36) fused with the CFG combine (infer.py:87):
 *   pred = u + cfg*(c-u);  x <- coef[t][0]*(x - coef[t][1]*pred) + coef[t][2]*z
 * coef: (T,3) = {1/sqrt(alpha), (1-alpha)/sqrt(1-alpha_bar), sqrt(beta)} (host-built
 * with the reference's own fp32 ops); t_index in [0,T).
 * z = noise[n] if noise != NULL, else the library's Philox N(0,1) stream
 * (seed, stream_id, row0 + row) -- see t2s_philox_normal.
 * eps_c may be NULL (then pred = eps_u and cfg is ignored).  In-place on x. */
int t2s_ddpm_step(float* x, const float* eps_u, const float* eps_c, const float* noise,
                  const float* coef, int t_index, float cfg, uint64_t seed, uint32_t stream_id,
                  uint32_t row0, int B, void* stream);
/* DDPM.p_sample as the class exposes it (DDPM.py:28-36): per-row timestep t (B) int32,
 * injected draws `noise` (B,64,30) (the host mirror supplies torch.randn like DDPM.py:35),
 * out of place.  n_steps = T, the length of the coefficient tables: a row whose t is outside [0,T) (the reference's
 * `gather` raises for it, DDPM.py:7-9) reads no table entry and comes out as NaN -- memory-safe and loud, without a
 * host sync in the sampling loop. */
int t2s_ddpm_p_sample(const float* xt, const float* eps_hat, const int32_t* t, const float* noise,
                      const float* coef, float* out, int B, int n_steps, void* stream);
/* The same two class methods on latents of another size, rows of `row_elems` floats (a multiple of 4): the MLP denoiser
 * of BASELINE configs[0] runs on the (B,64,L/4) pre-interpolation latent, not on (B,64,30). */
int t2s_ddpm_p_sample_n(const float* xt, const float* eps_hat, const int32_t* t, const float* noise,
                        const float* coef, float* out, int B, int row_elems, int n_steps, void* stream);
int t2s_ddpm_q_sample_n(const float* x0, const float* eps, const int32_t* t, const float* sqrt_ab,
                        const float* sqrt_1mab, float* out, int B, int row_elems, int n_steps, void* stream);
/* DDPM.loss / RectifiedFlow.loss = F.mse_loss(a, b) (DDPM.py:37-38, rectified_flow.py:13-16):
 * mean over n elements into out[0]; fixed summation order (deterministic, two launches: per-workgroup partials, then
 * their sum in index order).  scratch: T2S_MSE_SCRATCH_FLOATS floats of the CALLER's device memory, contents irrelevant
 * before and after; no state is kept anywhere else, so concurrent calls (other streams, other threads) only need
 * different scratch. */
#define T2S_MSE_SCRATCH_FLOATS 1024
int t2s_mse_ws(const float* a, const float* b, float* out, uint64_t n, float* scratch, void* stream);
/* The same with a scratch the library lends per (device, stream): allocated (hipMalloc, kept for the life of the
 * process) the first time a stream calls -- that first call is not capturable, later ones are.  Calls on one stream
 * are ordered by the stream; calls on different streams use different scratch. */
int t2s_mse(const float* a, const float* b, float* out, uint64_t n, void* stream);
/* RectifiedFlow.euler (rectified_flow.py:5-7) fused with the CFG combine (infer.py:81-82):
 *   x <- x + (u + cfg*(c-u)) * dt */
int t2s_rf_step(float* x, const float* v_u, const float* v_c, float cfg, float dt, int B,
                void* stream);
/* One table-driven linear multistep update for the few-step solvers (DDIM, DPM-Solver++(2M), Adams-Bashforth 2 -- built on
 * the host by t2ms_amd.sampler.solver_tables; no counterpart in the reference), fused with the CFG combine.  Per element,
 *   pred = u + cfg*(c-u)   (pred = u when pred_c is NULL)
 *   x' = c0*x + c1*pred + c2*h + c3*z        h' = c4*x + c5*pred   (from the OLD x)
 * coef: DEVICE (S,6), row `index` = {c0..c5}: the row of LOOP INDEX `index` (not S-1-index).  hist: (B,1920) history of the
 * solver (the previous x0 prediction / velocity), in place like x.  z = noise[n] (B,1920) if noise != NULL, else the Philox
 * N(0,1) stream (seed, stream_id, row0 + row) exactly as t2s_ddpm_step draws it.
 * A coefficient that is exactly 0 means its operand is not touched: c2 == 0 -> hist is not read (it may hold NaN or be
 * uninitialised on the first step); c3 == 0 -> no draw is made (noise may be NULL, no Philox work); c4 == c5 == 0 -> hist
 * is not written.  Arithmetic, fixed: evaluated in fp64 from the fp32 operands in the order pred, c0*x, + c1*pred, + c2*h,
 * + c3*z (fused multiply-adds) and rounded to fp32 once -- the x0-prediction history cancels two terms 157 times its size
 * at t = 999 of a 1000-step schedule; results repeat bit for bit. */
int t2s_lms_step(float* x, float* hist, const float* pred_u, const float* pred_c /* may be NULL */,
                 const float* noise /* (B,1920) or NULL */, const float* coef /* DEVICE (S,6) */, int index,
                 float cfg, uint64_t seed, uint32_t stream_id, uint32_t row0, int B, void* stream);
/* The same update on rows of row_elems values (a multiple of 4; 64*W for a wide latent): x, hist, pred_*, noise are
 * (B,row_elems), and the Philox draw of a row covers row_elems values.  t2s_lms_step is row_elems = 1920. */
int t2s_lms_step_n(float* x, float* hist, const float* pred_u, const float* pred_c /* may be NULL */,
                   const float* noise /* (B,row_elems) or NULL */, const float* coef /* DEVICE (S,6) */, int index,
                   float cfg, uint64_t seed, uint32_t stream_id, uint32_t row0, int B, int row_elems, void* stream);
/* DDPM.q_sample (DDPM.py:19-27): out = sqrt_ab[t[b]]*x0 + sqrt_1mab[t[b]]*eps.
 * sqrt_ab, sqrt_1mab: (T) host-built tables, T = n_steps; t: (B) int32 (out of range -> NaN row, see p_sample). */
int t2s_ddpm_q_sample(const float* x0, const float* eps, const int32_t* t, const float* sqrt_ab,
                      const float* sqrt_1mab, float* out, int B, int n_steps, void* stream);
/* RectifiedFlow.create_flow (rectified_flow.py:8-12): out = t*x1 + (1-t)*x0, t: (B) fp32. */
int t2s_rf_create_flow(const float* x1, const float* x0, const float* t, float* out, int B,
                       void* stream);
/* N(0,1) draws, Philox4x32-10 + Box-Muller: element e of GLOBAL row r uses counter
 * (e/4, r, stream_id, 0), key = seed; identical for any sharding of rows over GPUs.
 * out: (n_rows,row_elems), row_elems % 4 == 0.  (replaces torch.randn at
 * DDPM.py:35 / infer.py:75 in perf mode; parity mode injects noise instead.) */
int t2s_philox_normal(float* out, uint64_t seed, uint32_t stream_id, uint32_t row0, int n_rows,
                      int row_elems, void* stream);
/* The same draws with a key and a key row PER ROW: row r of out = row key_rows[r] of stream `stream_id` under key seeds[r],
 * bit for bit what t2s_philox_normal(out + r * row_elems, seeds[r], stream_id, key_rows[r], 1, row_elems) writes.
 * seeds (n_rows) u64 and key_rows (n_rows) u32 are DEVICE arrays.  With stream_id 0xFFFFFFFF it is the x_T draw of a
 * sampler whose rows come from different runs (t2s_sampler_set_rows). */
int t2s_philox_normal_rows(float* out, const uint64_t* seeds, const uint32_t* key_rows, uint32_t stream_id,
                           int n_rows, int row_elems, void* stream);
/* U[0,1) draws of the same stream: element e of GLOBAL row r = lane e % 4 of counter (e/4, r, stream_id, 0), key = seed,
 * as the 24-bit uniform (x >> 8) * 2^-24 (exact in fp32, never 1.0).  out: (n_rows,row_elems), any row_elems >= 1.
 * (replaces torch.rand at train.py:109,113: the per-row diffusion time of a training step, drawn on the device as a
 * function of (seed, step, global row) -- the same for any number of GPUs, and no host -> device copy per step.) */
int t2s_philox_uniform(float* out, uint64_t seed, uint32_t stream_id, uint32_t row0, int n_rows,
                       int row_elems, void* stream);

/* ------------------------------------------------------------------------ *
 * LA-VAE codec: model/pretrained/vqvae.py:36-105 (Encoder, Decoder)
 * ------------------------------------------------------------------------ */
typedef struct t2s_vae t2s_vae;

typedef struct t2s_vae_stack_weights { /* ResidualStack, vqvae.py:7-33 */
    const float* conv3_w[4]; /* _layers.i._block.1.weight (res_hidden,hidden,3), no bias */
    const float* conv1_w[4]; /* _layers.i._block.3.weight (hidden,res_hidden,1), no bias */
} t2s_vae_stack_weights;

typedef struct t2s_vae_weights {
    int hidden;       /* block_hidden_size (128)   */
    int res_hidden;   /* res_hidden_size (256)     */
    int n_res_layers; /* num_residual_layers (2), <= 4 */
    int emb;          /* embedding_dim (64)        */
    /* decoder.* (may all be NULL for an encode-only handle) */
    const float* dec_conv1_w; /* (hidden,emb,3) */
    const float* dec_conv1_b;
    t2s_vae_stack_weights dec_stack;
    const float* dec_ct1_w; /* ConvTranspose1d (hidden,hidden/2,4) */
    const float* dec_ct1_b;
    const float* dec_ct2_w; /* ConvTranspose1d (hidden/2,1,4) */
    const float* dec_ct2_b;
    /* encoder.* (may all be NULL for a decode-only handle) */
    const float* enc_conv1_w; /* (hidden/2,1,4) */
    const float* enc_conv1_b;
    const float* enc_conv2_w; /* (hidden,hidden/2,4) */
    const float* enc_conv2_b;
    const float* enc_conv3_w; /* (hidden,hidden,3) */
    const float* enc_conv3_b;
    t2s_vae_stack_weights enc_stack;
    const float* enc_prevq_w; /* (emb,hidden,1) */
    const float* enc_prevq_b;
} t2s_vae_weights;

int t2s_vae_create(const t2s_vae_weights* w, t2s_vae** out);
void t2s_vae_destroy(t2s_vae* h);
/* Decoder.forward, vqvae.py:97-105: z (B,64,30) -> recon (B,L), after (B,64,L/4) (may be NULL).
 * Any L % 4 == 0: up to 128 a series is one LDS-resident tile, longer ones (the reference's SUSHI set is 2048 long) run
 * as time tiles with recomputed halos -- the same values bit for bit.  (The host mirror applies torch.squeeze's rule.) */
int t2s_vae_decode(t2s_vae* h, const float* z, float* recon, float* after, int B, int L,
                   void* stream);
/* Decoder.forward on a latent of another width: z (B,64,latent_w), latent_w <= 32 (F.interpolate at vqvae.py:98 accepts any;
 * BASELINE configs[0] decodes the (B,64,L/4) latent of the MLP denoiser, for which the interpolation is the identity). */
int t2s_vae_decode_w(t2s_vae* h, const float* z, float* recon, float* after, int B, int L, int latent_w,
                     void* stream);
/* Encoder.forward, vqvae.py:57-71: x (B,L) -> z (B,64,30), before (B,64,L/4) (may be NULL for L <= 128; for longer
 * series the time tiles write `before` and a second launch interpolates it to the latent, so the buffer is required). */
int t2s_vae_encode(t2s_vae* h, const float* x, float* z, float* before, int B, int L,
                   void* stream);

/* Re-copy the weights into an existing handle (same hyper-parameters, same encoder / decoder presence): what a training
 * step does after the optimizer changed encoder.* (train.py:31-33 with usepretrainedvae false) -- no allocation, stream-ordered. */
int t2s_vae_update_weights(t2s_vae* h, const t2s_vae_weights* w, void* stream);

/* Multichannel LA-VAE codec: model/pretrained/myvqvae.py:32-86 (Encoder, Decoder) of the T2MS motion models -- C-channel
 * series (7 deadlift, 10 bench press), latent width flow_dim.  t2s_vae_weights is the same struct; three tensors carry the
 * channel count: enc_conv1_w (hidden/2,channels,4), dec_ct2_w (hidden/2,channels,4), dec_ct2_b (channels).
 *   channels 1..16, hidden <= 128 even, res_hidden <= 256, 0..4 residual layers, emb 64, latent_w 1..64, B > 0,
 *   8 <= L <= 2^20 -- a multiple of 4 OR NOT: the encoder's stride-2 convolutions give L/2 and L/4 positions (floor), the
 *   decoder builds 4 * (L/4) samples and resamples them to L (F.interpolate linear, align_corners; skipped when L % 4 == 0).
 * One launch per direction, one workgroup per (series, time tile), exact fp32, no atomics, bit-reproducible; neither entry
 * allocates device memory, so both can run inside a captured graph.  A handle is EITHER kind: a single-channel entry
 * (t2s_vae_encode, _decode, _decode_w, _encode_backward, _decode_backward) handed a multichannel handle returns
 * T2S_E_INVALID naming the _mc entry, and the _mc entries refuse a t2s_vae_create handle likewise; a handle made here with
 * channels = 1 is a multichannel handle.  t2s_vae_update_weights and t2s_vae_destroy serve both kinds.  The backward of the
 * two _mc entries is t2s_vae_encode_backward_mc / t2s_vae_decode_backward_mc below. */
int t2s_vae_create_mc(const t2s_vae_weights* w, int channels, t2s_vae** out);
int t2s_vae_channels(const t2s_vae* h);            /* 0 for a handle made by t2s_vae_create */
/* x (B,channels,L) -> z (B,emb,latent_w), before (B,emb,L/4) (may be NULL while L/4 <= 32; longer series run in time
 * tiles that write `before`, and a second launch interpolates it to the latent, so the buffer is required) */
int t2s_vae_encode_mc(t2s_vae* h, const float* x, float* z, float* before, int B, int L, int latent_w, void* stream);
/* z (B,emb,latent_w) -> recon (B,channels,L) (never squeezed), after (B,emb,L/4) (may be NULL) */
int t2s_vae_decode_mc(t2s_vae* h, const float* z, float* recon, float* after, int B, int L, int latent_w, void* stream);
/* 0.7 additions: ragged rows -- every series of a launch has its own length, so the clips of a motion test split (each a
 * (channels, T_i) recording) share one launch.  lengths (B) int32 and offsets (B + 1) uint64 = the prefix sums of lengths are
 * DEVICE arrays; series b is (channels, L_b), contiguous at base + channels * offsets[b]; z is (B,emb,latent_w) as in the
 * uniform entries.  offsets4 (B + 1) = the prefix sums of L_b / 4, `before` the packed (emb, L_b / 4) rows at
 * emb * offsets4[b] -- required unless max_L / 4 <= 32, as the uniform entry's `before`.  max_L (host, 8 .. 2^20) sizes the
 * grid's tile dimension for the longest row.  A row is skipped -- nothing of it read or written, its z row untouched by the
 * encode -- when L_b == 0, when L_b is outside [8, max_L], or when its offsets do not span L_b (offsets4: L_b / 4): a kernel
 * never leaves the span a row's own offsets give it.  Each row comes out bit for bit as from the uniform entry run on that
 * row alone at L_b (the kernels share one per-series body).  One launch per direction (the tiled encode adds one ragged
 * interpolation launch), no device allocation, no synchronisation: usable inside a captured graph.  T2S_E_INVALID before any
 * launch for a NULL pointer, a handle that is not multichannel, B <= 0, max_L or latent_w out of range. */
int t2s_vae_decode_mc_ragged(t2s_vae* h, const float* z, const int32_t* lengths, const uint64_t* offsets, float* recon, int B,
                             int max_L, int latent_w, void* stream);
int t2s_vae_encode_mc_ragged(t2s_vae* h, const float* x, const int32_t* lengths, const uint64_t* offsets,
                             const uint64_t* offsets4, float* z, float* before, int B, int max_L, int latent_w, void* stream);

/* Backward of Encoder.forward (vqvae.py:57-71) for the one reference configuration that TRAINS the LA-VAE encoder (train.py:31-33,
 * `usepretrainedvae` false: the encoder is grafted into the denoiser and its parameters join the optimizer).
 *   x (B,L) the forward's input; dz (B,64,30) = dLoss/dz; dbefore (B,64,L/4) = dLoss/dbefore or NULL (train.py uses z only);
 *   g: one gradient tensor per encoder.* parameter, same shapes as t2s_vae_weights' enc_* fields; every one is OVERWRITTEN.
 * The forward is recomputed from x (nothing is saved by t2s_vae_encode); data gradients run per series in LDS, weight gradients
 * as exact-fp32 MFMA GEMMs over all (series, position) rows with a fixed two-stage reduction: bit-reproducible.
 * Default LA-VAE shape only (hidden 128, res_hidden 128 / 256, emb 64) and L <= 128; allocates its row blocks on first use /
 * when B * L grows (not capturable then). */
typedef struct t2s_vae_enc_grads {
    float *conv1_w, *conv1_b;   /* encoder._conv_1 (hidden/2,1,4), (hidden/2) */
    float *conv2_w, *conv2_b;   /* encoder._conv_2 (hidden,hidden/2,4), (hidden) */
    float *conv3_w, *conv3_b;   /* encoder._conv_3 (hidden,hidden,3), (hidden) */
    float* stack_conv3_w[4];    /* encoder._residual_stack._layers.i._block.1.weight (res_hidden,hidden,3) */
    float* stack_conv1_w[4];    /* encoder._residual_stack._layers.i._block.3.weight (hidden,res_hidden,1) */
    float *prevq_w, *prevq_b;   /* encoder._pre_vq_conv (emb,hidden,1), (emb) */
} t2s_vae_enc_grads;
int t2s_vae_encode_backward(t2s_vae* h, const float* x, const float* dz, const float* dbefore, const t2s_vae_enc_grads* g, int B,
                            int L, void* stream);

/* Backward of Decoder.forward (vqvae.py:97-105): with the encoder backward above, the MSE pair and t2s_adamw_step_multi this is
 * one optimisation step of LA-VAE pre-training (pretrained_lavae_unified.py:142-174, vqvae.shared_eval mode 'train').
 *   z (B,64,latent_w) the forward's input; drecon (B,L) = dLoss/drecon; dafter (B,64,L/4) = dLoss/dafter or NULL;
 *   g: one gradient tensor per decoder.* parameter, same shapes as t2s_vae_weights' dec_* fields; every one is OVERWRITTEN;
 *   dz (B,64,latent_w) receives dLoss/dz (decoder part + the transposed interpolation of dafter); NULL: not computed.
 * The forward is recomputed from z (nothing is saved by t2s_vae_decode[_w]); data gradients run per series in LDS, weight
 * gradients as exact-fp32 MFMA GEMMs over all (series, position) rows with a fixed two-stage reduction, the 4-tap
 * _conv_trans_2 and the two small biases as per-series partial rows added in series order: bit-reproducible.
 * Default LA-VAE shape only (hidden 128, res_hidden 128 / 256, emb 64), 8 <= L <= 128, 1 <= latent_w <= 32; anything else
 * is T2S_E_INVALID ("unsupported").  Like t2s_vae_encode_backward it allocates its row blocks on first use / when B * L grows
 * (not capturable then, and a device-wide call: the host mirror takes its per-device lock around a call that grows them). */
typedef struct t2s_vae_dec_grads {
    float *conv1_w, *conv1_b;   /* decoder._conv_1 (hidden,emb,3), (hidden) */
    float* stack_conv3_w[4];    /* decoder._residual_stack._layers.i._block.1.weight (res_hidden,hidden,3) */
    float* stack_conv1_w[4];    /* decoder._residual_stack._layers.i._block.3.weight (hidden,res_hidden,1) */
    float *ct1_w, *ct1_b;       /* decoder._conv_trans_1 (hidden,hidden/2,4), (hidden/2) */
    float *ct2_w, *ct2_b;       /* decoder._conv_trans_2 (hidden/2,1,4), (1) */
} t2s_vae_dec_grads;
int t2s_vae_decode_backward(t2s_vae* h, const float* z, const float* drecon, const float* dafter, const t2s_vae_dec_grads* g,
                            float* dz, int B, int L, int latent_w, void* stream);

/* The two backwards for the multichannel codec (a t2s_vae_create_mc handle): one optimisation step of the motion codec's
 * pre-training (myvqvae.py:116-136) with t2s_vae_encode_mc / t2s_vae_decode_mc, and the encoder's part of a DiT step
 * (mytrain.py:37-40).  The same kernels and host path as the single-channel entries above, which are their C = 1 case (a
 * channels = 1 handle gives the single-channel entries' bits); the same gradient structs, with
 *   conv1_w (hidden/2,channels,4), ct2_w (hidden/2,channels,4), ct2_b (channels);
 *   x (B,channels,L), dz (B,64,latent_w), drecon (B,channels,L); dbefore, dafter and the decoder's dz may be NULL as above.
 * When L % 4 != 0 the decoder's way back starts with the transpose of the final resampling 4 (L/4) -> L.
 *   channels 1..16, hidden 128, res_hidden 128 / 256, 1..4 residual layers, emb 64, latent_w 1..64, B > 0, 8 <= L <= 192 (the
 *   whole series is one LDS tile: L/4 <= 32 in today's geometry, L/4 <= 48 in about 150 KiB of LDS);
 * anything else, a t2s_vae_create handle or a NULL gradient pointer is T2S_E_INVALID before any launch or allocation.
 * T2S_E_HIP if the runtime refuses the kernels' dynamic-LDS cap.  Row blocks grow like the single-channel entries'. */
int t2s_vae_encode_backward_mc(t2s_vae* h, const float* x, const float* dz, const float* dbefore, const t2s_vae_enc_grads* g, int B,
                               int L, int latent_w, void* stream);
int t2s_vae_decode_backward_mc(t2s_vae* h, const float* z, const float* drecon, const float* dafter, const t2s_vae_dec_grads* g,
                               float* dz, int B, int L, int latent_w, void* stream);

/* ------------------------------------------------------------------------ *
 * Fused sampling loop: infer.py:75-95 (x_T -> steps x [2 DiT forwards + CFG +
 * sampler update] -> LA-VAE decode), one hipGraph per step replayed `steps`
 * times with a device-side step counter.
 * ------------------------------------------------------------------------ */
typedef struct t2s_sampler t2s_sampler;

#define T2S_MODE_DDPM 0
#define T2S_MODE_RF 1
#define T2S_MODE_LMS 2   /* table-driven linear multistep update (t2s_lms_step): t2s_sampler_create_lms only */

typedef struct t2s_sample_config {
    int mode;            /* T2S_MODE_DDPM | T2S_MODE_RF (| T2S_MODE_LMS: _create_lms)    */
    int steps;           /* infer.py --total_step                                         */
    float cfg_scale;     /* infer.py --cfg_scale                                          */
    int batch;           /* series per call on this GPU (2*batch <= dit max_seqs)         */
    int length;          /* decoded series length L (24/48/96)                            */
    int use_graph;       /* 1: capture one step into a hipGraph and replay it             */
    uint64_t seed;       /* Philox key (perf mode)                                        */
    uint32_t row0;       /* global index of this shard's first series (multi-GPU)         */
    const float* ddpm_coef; /* HOST (steps,3), see t2s_ddpm_step; NULL for RF             */
    const float* t_values;  /* HOST (steps): the t passed to the denoiser at loop index j:
                               DDPM steps-1-j (infer.py:84), RF round(j/steps*steps)/steps (:78) */
} t2s_sample_config;

/* On a DiT handle of t2s_dit_create_w the sampler's rows are 64*W values: x is (B,64,W), noise (steps,B,64,W), the Philox draw
 * of a row covers 64*W values, the history / eps buffers follow.  With W > 32 `vae` must be a multichannel decoder handle
 * (t2s_vae_create_mc; it decodes at latent width W) or NULL: a single-channel t2s_vae_create handle is T2S_E_INVALID here and
 * in t2s_sampler_create_lms, before any allocation. */
int t2s_sampler_create(t2s_dit* dit, t2s_vae* vae /* may be NULL: no decode */,
                       const t2s_sample_config* cfg, t2s_sampler** out);
/* The same sampler with the few-step update of t2s_lms_step in place of the ancestral DDPM / Euler update: cfg->mode =
 * T2S_MODE_LMS, cfg->steps = S (the number of denoiser evaluations), cfg->t_values (S) the t handed to the denoiser at loop
 * index j (a DDPM solver's grid of TRAINED integer times, or the flow model's j/S), cfg->ddpm_coef NULL; lms_coef HOST
 * (S,6), row j = the coefficients of loop index j, copied at the call.  The sampler owns the (batch,1920) history buffer
 * (zeroed here; lanes slice it by rows).  Everything else is t2s_sampler_run's as it is: graphs (one step / whole loop),
 * lanes, trace0, set_row0 / set_rows, the adaLN table, every matrix arithmetic.  `noise` stays (steps,B,64,30) and is read
 * only at steps whose c3 != 0.  T2S_E_INVALID -- before any allocation, with a t2s_last_error text -- for a NULL table, a
 * coefficient that is not finite, steps < 1 or another mode; t2s_sampler_create in turn refuses T2S_MODE_LMS. */
int t2s_sampler_create_lms(t2s_dit* dit, t2s_vae* vae /* may be NULL: no decode */, const t2s_sample_config* cfg,
                           const float* lms_coef, t2s_sampler** out);
void t2s_sampler_destroy(t2s_sampler* s);
/* Run the whole loop.
 *   x      (B,64,30) in: x_T (perf mode: fill it with t2s_philox_normal, stream_id 0xFFFFFFFF);
 *          out: final latent
 *   text   (B,128)
 *   noise  (steps,B,64,30) injected per-step draws (parity mode) or NULL (Philox, perf mode)
 *   series (B,L) decoded output, or NULL
 *   trace0 (steps,L) or NULL: decode of row 0 after every step (infer.py:90-93)
 *          With a multichannel decoder handle (t2s_vae_create_mc, C channels) given at create, the decodes run
 *          t2s_vae_decode_mc at latent width 30: series is (B,C,L), trace0 (steps,C,L), and cfg->length may be any value
 *          >= 8.  A single-channel handle takes the path above unchanged (length a multiple of 4).
 *   stream NULL = the default stream.  With use_graph = 1 the graphs are then captured and replayed on a stream
 *          the sampler owns (the default stream cannot be captured), ordered after everything queued on the default
 *          stream before the call and joined back to it before the call returns -- same semantics, never an eager
 *          fallback.  trace0 runs are eager by design (a decode between the steps).  Runs with more than one lane
 *          (t2s_sampler_set_lanes) execute on the library's own pool of streams in the same way for ANY `stream`: the
 *          run is ordered after everything queued on `stream` before the call and joined back to it before the call
 *          returns.
 * Threads: (the header's convention: one thread per handle at a time.)  Two threads may drive two samplers on two t2s_dit
 *          handles of one device concurrently.  Every run that opens a stream capture (use_graph) or uses the library's
 *          stream pool (several lanes, or stream NULL with use_graph) holds a per-device lock for the length of its
 *          ENQUEUE (host work of a few ms; the GPU work stays asynchronous), and t2s_sampler_create / _destroy take the
 *          same lock.  Why (measured): while ANY thread has a stream capture open on the device, HIP
 *          answers a synchronous hipMemcpy and a hipDeviceSynchronize from any other thread with an error
 *          (hipErrorStreamCaptureImplicit / hipErrorStreamCaptureUnsupported) and INVALIDATES the open capture, thread-
 *          local capture mode notwithstanding.  The library itself issues neither outside that lock (t2s_sampler_create
 *          uploads on a non-blocking stream of its own; no entry point copies synchronously), and the Python mirrors
 *          build / grow / destroy their handles under the same per-device lock (t2ms_amd._lib.device_lock).  What no lock
 *          of the library can cover is the CALLER's own device-wide calls on other threads while a run is being enqueued
 *          -- hipDeviceSynchronize (torch.cuda.synchronize()), synchronous hipMemcpy -- and a `stream` handed to a
 *          single-lane run, which -- like any HIP stream under capture -- must not be used by another thread meanwhile.
 *          (Stream-ordered work of other threads, including torch's default-stream kernels, asynchronous copies and
 *          stream synchronisations, is fine: tools/stress_threads.py runs it against open captures by the thousand.)
 *          The pool is created and calibrated by the first t2s_sampler_create on a device (not by a run), so a run
 *          never allocates or synchronises for it.
 * Memory:  t2s_sampler_create also allocates a whole-run adaLN table (steps x (batch + 1) x 3072 floats: 3.2 GB at
 *          256 series x 1000 steps, ~2 % of a step) when that is at most 1/8 of the device memory currently free and
 *          16 GB; otherwise -- or with T2S_ADALN_TABLE=0 in the environment -- the per-step adaLN kernel runs instead
 *          (bitwise the same results).
 */
int t2s_sampler_run(t2s_sampler* s, float* x, const float* text, const float* noise,
                    float* series, float* trace0, void* stream);
/* Lanes of t2s_sampler_run: the rows of a batch never interact (infer.py:76-88), so the loop may run as two (up to four)
 * part batches, each a complete chain with its own hipGraph on its own stream (lanes 1.. on streams the sampler owns,
 * forked from / joined to `stream` inside the call), so that one chain's kernels fill the chip while the other's
 * drain.  Bitwise the same result.  lanes: 0 = automatic (equal shares: two when the batch is a multiple of 64 or 32 series, three for 96; env
 * T2S_SAMPLER_LANES=<n> overrides), or 1 .. 4 chains of equal shares.  trace0 runs always use one lane. */
int t2s_sampler_set_lanes(t2s_sampler* s, int lanes);
/* What a lane's hipGraph holds (use_graph = 1): whole_loop = 1 -> the WHOLE loop, steps x (forward + update) kernel nodes,
 * launched once per run ("whole loop in one hipGraph"); 0 -> ONE step, replayed `steps` times from the
 * host; -1 -> the library's default (env T2S_SAMPLER_LOOP_GRAPH=0|1 overrides it).  Every node reads its loop index from
 * the lane's device counter, so both forms run the same kernels in the same order: bitwise the same result.  Takes effect
 * at the next t2s_sampler_run (the graphs are re-captured when the form changes). */
int t2s_sampler_set_loop_graph(t2s_sampler* s, int whole_loop);
/* Guidance interval: classifier-free guidance on the window [first, end) of LOOP indices only (j = 0 is the noisiest step of
 * both backbones; `steps` is the sampler's loop length, i.e. sample_steps with a few-step solver).  A step inside the window
 * is the step described above: the CFG pass over 2 * batch sequences and pred = u + w (c - u).  Any other step runs ONE DiT
 * pass over the batch rows with their text and the update takes its output as pred, unchanged (no w = 1 arithmetic): half the
 * sequences of a guided step.  Noise draws, Philox stream ids, the coefficient row, the few-step solvers' history and the
 * loop index are those of step j either way; a row's guidance scale (t2s_sampler_set_rows) is not read on an unguided step,
 * its seed and key row are.  The default window is (0, steps): every step guided, the kernels, launch order and graphs of a
 * sampler that was never given a window.  Applies to the next runs.  A window that differs from the current one drops the
 * captured hipGraphs (the whole-loop graph holds each step's kind; the one-step form keeps one graph per kind in use); the
 * same window again keeps them.  T2S_E_INVALID, with first / end / steps in t2s_last_error and before anything is touched,
 * unless 0 <= first <= end <= steps.  Not in the reference (Kynkaanniemi et al., NeurIPS 2024). */
int t2s_sampler_set_guided_steps(t2s_sampler* s, int first, int end);
/* The current window of t2s_sampler_set_guided_steps. */
int t2s_sampler_guided_steps(const t2s_sampler* s, int* first, int* end);
/* Move the sampler to another shard position: global index of its first series (the Philox key of row r is
 * row0 + r).  Takes effect at the next t2s_sampler_run; the captured hipGraphs are kept (the kernels read the
 * value from device memory next to the step counter).  infer.py:66 loops over batches with one sampler. */
int t2s_sampler_set_row0(t2s_sampler* s, uint32_t row0);
/* Per-row noise keys and guidance scale: row r of the batch draws its per-step noise as row key_rows[r] of the Philox
 * stream keyed by seeds[r] and combines pred = u + cfg[r] * (c - u), so one run may hold the rows of several runs
 * (seeds), positions (key rows) and guidance scales -- rows never interact, so each row comes out bit for bit as in a
 * uniform sampler of its own seed / row0 / cfg_scale.  HOST arrays of n == batch entries, copied at the call; any of them
 * NULL = uniform (config seed, row0 + r, cfg_scale respectively); all three NULL restores the uniform sampler.  Takes
 * effect at the next t2s_sampler_run, the captured hipGraphs are kept (the kernels read the tables and which of them are
 * in use from device memory).  The run uploads the tables stream-ordered from a pinned buffer the sampler owns; no
 * synchronous copy.  x_T is the caller's: draw it with t2s_philox_normal_rows (stream_id 0xFFFFFFFF).
 * T2S_E_INVALID when n != batch or a cfg value is not finite. */
int t2s_sampler_set_rows(t2s_sampler* s, const uint64_t* seeds, const uint32_t* key_rows, const float* cfg, int n);
/* 0.7 additions: per-row series lengths for a sampler with a multichannel decoder.  lengths is a HOST array of n == batch
 * entries, each 0 (the row decodes nothing) or in [8, cfg.length] -- cfg.length is the maximum; NULL restores the uniform
 * sampler.  With lengths set, the final decode of t2s_sampler_run is t2s_vae_decode_mc_ragged: `series` is the packed
 * layout above (row b is (channels, L_b) at channels * sum of the lengths before it) and trace0 is (steps, channels,
 * lengths[0]).  The loop, its graphs, lanes, solvers and guidance window are untouched: the latent of a run does not depend
 * on the lengths.  Copied at the call; lengths and offsets reach the device at the next run, stream-ordered from the
 * sampler's pinned buffer like the tables of t2s_sampler_set_rows.  T2S_E_INVALID, before anything is touched, without a
 * multichannel decoder, when n != batch or a length is out of range. */
int t2s_sampler_set_lengths(t2s_sampler* s, const int32_t* lengths, int n);
/* Number of lanes the sampler currently holds an instantiated hipGraph for (0: the last run was eager / nothing run
 * yet).  Lets a caller (and tests/test_hip_parity.py) check that use_graph = 1 really replays a graph. */
int t2s_sampler_graph_lanes(const t2s_sampler* s);
/* How many MUTUALLY CONCURRENT streams the calibration of the current device's lane-stream pool found (0: the pool has
 * not been built yet -- it is built by the first multi-lane or NULL-stream graph run; 4: every lane has a hardware queue
 * of its own).  Diagnostic: HIP streams that share a hardware queue execute one after the other. */
int t2s_sampler_lane_pool(void);

/* ------------------------------------------------------------------------ *
 * Evaluation metrics: evaluation.py:166-206 (calculate_mse, calculate_wape), :21-45 (calculate_mrr)
 * ------------------------------------------------------------------------ */
/* ori, gen: (n, len) device arrays, len = L * n_series of the (N, L, n_series) arrays infer.py writes;
 * per_sample: (n, 2) output = [mse_i, wape_i (NaN when sum |ori_i| == 0)]; out: [MSE, WAPE] =
 * [mean_i mse_i, nanmean_i wape_i].  Deterministic summation order.
 * Non-finite input is not filtered, IEEE arithmetic decides, as in the reference's numpy: a NaN in ori_i or gen_i makes mse_i
 * and wape_i NaN; an Inf makes mse_i +Inf (NaN where Inf meets Inf of the same sign) and wape_i +Inf when it is in gen_i, NaN
 * (Inf / Inf) when it is in ori_i.  MSE takes every mse_i, so it is NaN / Inf with them; WAPE skips every NaN wape_i, whatever
 * made it NaN, and is NaN when none is left. */
int t2s_eval_mse_wape(const float* ori, const float* gen, float* per_sample, float* out, int n, int len,
                      void* stream);

/* MRR over repeated generations: evaluation.py:21-45 (calculate_mrr) with cosine_similarity of
 * Dataset_Construction_Pipeline/Evaluate_Datasets.py:6-15, as evaluation.py:298-314 feeds it (x_1.npy against the
 * x_t.npy of run_0..run_{runs-1}).
 * ori (n, len); gen (runs, n, len), run-major (the reference stacks the runs on a trailing axis; the host mirror
 * passes them in the order it loads them); sims (n, runs) output: the cosine similarities (0 where not finite);
 * score (n) output: 1 / (g + 1) for the best run g when its similarity exceeds `threshold` (the reference uses
 * 0.5, evaluation.py:300), else 0 -- g is the run INDEX, as the reference computes it; ties go to the largest
 * index; out[0] = mean score.
 * A similarity that is not finite -- a NaN or an Inf anywhere in ori_i or in that run -- is stored as 0 and takes part in the
 * search for the best run as 0 (the reference's nan_to_num); score and out[0] are always finite. */
int t2s_eval_mrr(const float* ori, const float* gen, float* sims, float* score, float* out, int n, int len,
                 int runs, float threshold, void* stream);

/* ED: evaluation.py:137-150 (calculate_ed).  ori, gen: (n, L, n_series); per_sample (n): mean over series of the
 * Euclidean distance over time; out[0] = mean over samples.  A NaN in ori_i or gen_i makes per_sample[i] and out[0] NaN, an Inf
 * makes them +Inf (NaN where Inf meets Inf of the same sign); other samples are not touched. */
int t2s_eval_ed(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                void* stream);
/* CRPS: evaluation.py:51-83 (calculate_crps) over the repeated generations evaluation.py:298-314 stacks.
 * ori (n, L, n_series); gen (runs, n, L, n_series) run-major; per_sample (n); out[0] = mean.  Per series and run the mean
 * and the population std over time are taken in fp64 and rounded once to fp32 (a std of exactly 0 becomes 1e-8f), the step
 * is `obs < mean ? 0 : 1` on fp32 values, Phi runs in fp64.  A NaN or an Inf in gen_i (its mean or std is NaN then) or a NaN
 * in ori_i makes per_sample[i] and out[0] NaN; an Inf in ori_i contributes 0 at that step (Phi = the step), the rest stays
 * finite. */
int t2s_eval_crps(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                  int runs, void* stream);
/* DTW: evaluation.py:152-163 (calculate_dtw = dtaidistance 2.3 dtw_ndim.distance, no window, no penalty): sqrt of the
 * minimal warping-path cost with squared-Euclidean point costs between the (L, n_series) sequences of each sample.
 * per_sample (n); out[0] = mean.  L <= 4096 (T2S_E_INVALID beyond, before any launch).  A NaN anywhere in ori_i or gen_i
 * makes per_sample[i] and out[0] NaN (every warping path crosses its row or column); an Inf makes them +Inf, NaN where Inf
 * meets Inf of the same sign. */
int t2s_eval_dtw(const float* ori, const float* gen, float* per_sample, float* out, int n, int L, int n_series,
                 void* stream);

/* Feature-based measures of evaluate/feature_based_measures.py: calculate_mdd (:30-94), calculate_acd (:98-161),
 * calculate_sd (:165-191), calculate_kd (:195-223).  They compare the SET ori ("real") with the SET gen ("fake"), both
 * (n, L, n_series) fp32 contiguous on the device; no row of one is paired with a row of the other, so a common
 * permutation of the rows changes nothing.  n >= 2, 1 <= L <= 4096, n_series >= 1 (L * n_series <= 2^24); anything else,
 * a NULL array or a workspace smaller than t2s_eval_features_workspace_bytes is T2S_E_INVALID before any launch.  The
 * entries never allocate, copy or synchronise and keep no state: the caller owns the workspace (its contents are
 * scratch; the two entries use disjoint parts of it).  The same input gives the same bits on every call, whatever the
 * device: sums run in fp64 over chunks of samples that depend on n alone, MDD's counts are integers. */
#define T2S_EVAL_MAX_LAG 64  /* ACFLoss(max_lag=64): K = min(64, L) lags */
#define T2S_EVAL_MDD_BINS 50 /* calculate_mdd: n_bins=50 */
/* Bytes of workspace t2s_eval_moments / t2s_eval_mdd need at this shape (0 and an error message if unsupported). */
uint64_t t2s_eval_features_workspace_bytes(int n, int L, int n_series);
/* ACD, SD, KD from one statistics pass.  Per channel, over its n*L values centred by the channel mean: acf_k = mean of
 * x[i,t] x[i,t-k] over (i, t >= k) / population variance for k < K (acf_torch, :98-109); skewness = mean x^3 / unbiased
 * std^3 (skew_torch, :165-172); excess kurtosis = mean x^4 / population variance^2 - 3 (kurtosis_torch, :195-204).
 * out[3] = [ACD, SD, KD] = the means over channels of [sqrt(sum_k (acf_k(gen) - acf_k(ori))^2), |skew(gen) - skew(ori)|,
 * |kurt(gen) - kurt(ori)|].  stats (may be NULL): (2, n_series, 4 + K), set 0 = ori, 1 = gen, each row
 * [mean, population variance, skewness, excess kurtosis, acf_0 .. acf_{K-1}]. */
int t2s_eval_moments(const float* ori, const float* gen, float* stats, float* out, int n, int L, int n_series,
                     void* workspace, uint64_t workspace_bytes, void* stream);
/* MDD (HistoLoss + histogram_torch, :30-94).  Per column (t, c): 50 equal bins between the min and the max of the n real
 * values (max = min + 1e-5 for a constant column), real and fake values counted per bin (torch.histc's binning, the max
 * in the last bin; a fake value outside [min, max] counts nowhere), loss = mean over bins of |fake density - real
 * density|, density = count / (n * bin width).  per_column (may be NULL): (L, n_series) column losses -- the reference
 * lists them channel-major; out[0] = their mean. */
int t2s_eval_mdd(const float* ori, const float* gen, float* per_column, float* out, int n, int L, int n_series,
                 void* workspace, uint64_t workspace_bytes, void* stream);

/* Motion measures of evaluate/metrics.py, the ones its __main__ (:290-370) compares recordings of unequal length with:
 * the correlational score (:112-137), the sequence correlation (:219-266) and DTW of two sequences of unequal length
 * (calculate_dtw(seq1, seq2), :139-170).  Like the feature entries they use the caller's stream, never allocate, copy
 * or synchronise and keep no state; every refusal is T2S_E_INVALID with the entry's name and the offending value in
 * t2s_last_error, before any launch; the same input gives the same bits on every call, whatever the grid (fixed fp64
 * summation orders, no floating-point atomics). */
#define T2S_EVAL_CORR_MAX_SERIES 64    /* t2s_eval_corr: channels */
#define T2S_EVAL_MOTION_MAX_LEN 4096   /* t2s_eval_shift / t2s_eval_dtw_ragged: padded length of either side */
/* Bytes of workspace t2s_eval_corr needs at this shape (0 and an error message if unsupported): about 16 P n_series^2 with
 * P = min(max(rows_ori, rows_gen), 1024), i.e. 1.6 MB at 10 channels and 64 MiB at 64. */
uint64_t t2s_eval_corr_workspace_bytes(int rows_ori, int rows_gen, int n_series);
/* Correlational score: calculate_correlation_matrix / calculate_correlational_score (:112-137).  ori (rows_ori, n_series),
 * gen (rows_gen, n_series) fp32 contiguous -- the reference's reshape(N * T, D), so the two sets may differ in N and T;
 * rows >= 2 each, 1 <= n_series <= T2S_EVAL_CORR_MAX_SERIES.  As np.corrcoef(rowvar=False), all in fp64: the channel
 * means, the centred co-moments c_ij = sum_r (x_ri - mean_i)(x_rj - mean_j), C_ij = (c_ij / sqrt(c_ii)) / sqrt(c_jj)
 * (two divisions, as numpy does them) clipped to [-1, 1]; out[0] = 1 - sum |C_ori - C_gen| / sum |C_ori|, NaN when that
 * denominator is exactly 0.  corr (may be NULL): (2, n_series, n_series), set 0 = ori, 1 = gen; every stored value is
 * rounded once from fp64, and the score is taken from the fp64 matrices.  Sums run over P = min(rows, 1024) chunks of
 * rows (a function of rows alone), partials are folded in index order.
 * Non-finite values are not filtered, IEEE arithmetic decides as in numpy: a constant channel (c_ii == 0) gives NaN in
 * its row and column of that set's matrix (0 / 0) and a NaN score; a NaN or an Inf in the data makes the mean and with
 * it every co-moment of that channel NaN, hence its row and column and the score NaN. */
int t2s_eval_corr(const float* ori, const float* gen, float* corr, float* out, int rows_ori, int rows_gen, int n_series,
                  void* workspace, uint64_t workspace_bytes, void* stream);
/* Sequence correlation: sequence_correlation (:219-266) for n pairs in padded storage a (n, La, n_series), b (n, Lb,
 * n_series); len_a, len_b: device int32 (n), the lengths m_i, n_i of the pairs, either NULL = the full La / Lb.  A length
 * is clamped into [1, La] resp. [1, Lb] by the kernels, so no value in those arrays takes a read outside a or b (the
 * Python mirror refuses such a length on the host); the padding is never read.  1 <= La, Lb <= 4096, n_series >= 1.
 * Per pair, M = min(m, n) - 1 and for every shift s in -M .. M:
 *   s >= 0: ov = min(m, n - s), a[0:ov] against b[s:s+ov];    s < 0: ov = min(m + s, n), a[-s:-s+ov] against b[0:ov];
 *   dist_s = mean over the overlap of the Euclidean norm over the channels (norm and sum in fp64, rounded once).
 * table (n, W), W = 2 min(La, Lb) - 1: dist_s in column min(La, Lb) - 1 + s, NaN where a pair has no such shift.
 * Search rule: the reference's left-to-right scan min(keys, key=...) on the values AS STORED in fp32, starting at s = -M:
 * a later shift wins only if its value is strictly smaller, so among equal values the most negative shift wins, and a
 * NaN is never chosen unless it is the first shift's value, which then stays, as in the reference.  best_shift (n, int32);
 * min_dist (n): bit for bit table[i, best]; out[0] = mean of min_dist.
 * A NaN in an overlap makes that shift's distance NaN, an Inf makes it +Inf (NaN where Inf meets Inf of the same sign);
 * shifts whose overlap avoids the value are not touched.
 * The reference's wrapper calculate_sequence_correlation (:197-217) returns only the LAST pair's result; this entry returns
 * every pair's. */
int t2s_eval_shift(const float* a, const float* b, const int* len_a, const int* len_b, float* table, int* best_shift,
                   float* min_dist, float* out, int n, int La, int Lb, int n_series, void* stream);
/* DTW of sequences of unequal length: calculate_dtw(seq1, seq2) (:139-170) with its default squared-Euclidean cost, no
 * window, no penalty, then a sqrt -- the recurrence of t2s_eval_dtw on an m x n table.  Storage, length arrays and
 * clamping as for t2s_eval_shift; per_sample (n); out[0] = mean; La, Lb <= 4096 (T2S_E_INVALID beyond, before any
 * launch).  With La == Lb and no length arrays the result equals t2s_eval_dtw's bit for bit.  As there, a NaN anywhere in
 * a_i or b_i (inside the lengths) makes per_sample[i] and out[0] NaN, an Inf makes them +Inf, NaN where Inf meets Inf of
 * the same sign. */
int t2s_eval_dtw_ragged(const float* a, const float* b, const int* len_a, const int* len_b, float* per_sample, float* out,
                        int n, int La, int Lb, int n_series, void* stream);

/* TS2Vec encoder of the C-FID metric: evaluate/ts2vec.py:352-399 (TSEncoder.forward, eval mode, mask 'all_true') followed
 * by the 'full_series' pooling of TS2Vec.encode (:236-245).  Device pointers to the state-dict tensors:
 * input_fc.{weight (hidden,input_dims),bias}; block i in [0,depth]: feature_extractor.net.i.conv{1,2}.conv.{weight
 * (co,ci,3),bias} with dilation 2^i (blocks 0..depth-1: hidden -> hidden, block depth: hidden -> output_dims with the 1x1
 * projector feature_extractor.net.depth.projector.{weight (output_dims,hidden,1),bias}). */
#define T2S_TS2VEC_MAX_BLOCKS 16
typedef struct t2s_ts2vec_weights {
    int input_dims, hidden, output_dims, depth;
    const float *fc_w, *fc_b;
    const float* conv1_w[T2S_TS2VEC_MAX_BLOCKS];
    const float* conv1_b[T2S_TS2VEC_MAX_BLOCKS];
    const float* conv2_w[T2S_TS2VEC_MAX_BLOCKS];
    const float* conv2_b[T2S_TS2VEC_MAX_BLOCKS];
    const float *proj_w, *proj_b;
} t2s_ts2vec_weights;
/* x (B, T, input_dims) -> rep (B, T, output_dims) per-step representations (may be NULL) and full (B, output_dims) =
 * their maximum over time.  Time steps of x holding a NaN are zeroed as the reference does.  3 * max(hidden,
 * output_dims) * T * 4 bytes must fit in 160 KB of LDS (T <= 128 at the evaluation's 64 / 100 channels). */
int t2s_ts2vec_encode(const t2s_ts2vec_weights* w, const float* x, float* rep, float* full, int B, int T, void* stream);
/* The same function at any length 1 <= T <= T2S_TS2VEC_ENCODE_MAX_T (csrc/t2s_ts2vec_encode.hip): the three activation
 * planes live in the caller's workspace as (B, C rounded up to 32, T) fp32 and every dilated convolution is a GEMM with
 * K = 3 ci on the exact-f32 matrix instruction, one launch per convolution.  Supported: B >= 1, equal hidden widths,
 * depth < T2S_TS2VEC_MAX_BLOCKS, 1 <= input_dims <= 64, hidden <= 128, output_dims <= 320 (no multiple of the 32-row
 * tile is needed: the kernels pad); anything else, a NULL x / full / workspace or a workspace smaller than
 * t2s_ts2vec_encode_workspace_bytes is T2S_E_INVALID before any launch.  fp32 throughout; an output element's sum over
 * (tap, input channel[, projector channel]) runs in that one order whatever tile computes it, wherever the series sits
 * in the batch and whatever B is; no floating-point atomics: the same input gives the same bits on every call, and row
 * i of a batch equals that row encoded alone.  The summation order differs from t2s_ts2vec_encode's, so the two agree
 * to rounding, not bit for bit.  The entry never allocates, copies synchronously or synchronises and keeps no state:
 * the weights are re-packed into the workspace (whose contents are scratch) at every call; 2 depth + 5 launches, all on
 * `stream`.  A block whose dilation is >= T runs its centre tap only. */
#define T2S_TS2VEC_ENCODE_MAX_T 4096
/* Bytes of workspace t2s_ts2vec_encode_long needs: the packed weights + 3 planes of B * roundup32(max(hidden,
 * output_dims)) * T floats, each part rounded up to 256 bytes (0 and an error message if unsupported). */
uint64_t t2s_ts2vec_encode_workspace_bytes(const t2s_ts2vec_weights* w, int B, int T);
int t2s_ts2vec_encode_long(const t2s_ts2vec_weights* w, const float* x, float* rep /* may be NULL */, float* full,
                           int B, int T, void* workspace, uint64_t workspace_bytes, void* stream);

/* One training step of TS2Vec.fit (evaluate/ts2vec.py:113-140): the TRAINING forward of both cropped views (binomial
 * time mask after input_fc, dropout on the representations), hierarchical_contrastive_loss (:451-497) of their overlap,
 * and the backward down to every parameter.  fp32 throughout, exact erf GELU and its exact derivative.  The entries below
 * never allocate, copy synchronously or synchronise: the caller owns the workspace, the calls are capturable and need no
 * per-device lock.  Bit-reproducible: every weight gradient is summed over (view, series, time) in that order by one
 * thread, the loss terms in (level, kind, task) order; no floating-point atomics. */
#define T2S_TS2VEC_TRAIN_MAX_T 128
#define T2S_TS2VEC_TRAIN_MAX_B 16
/* The gradient of every tensor of t2s_ts2vec_weights, in its own layout; every entry is OVERWRITTEN. */
typedef struct t2s_ts2vec_grads {
    float *fc_w, *fc_b;
    float* conv1_w[T2S_TS2VEC_MAX_BLOCKS];
    float* conv1_b[T2S_TS2VEC_MAX_BLOCKS];
    float* conv2_w[T2S_TS2VEC_MAX_BLOCKS];
    float* conv2_b[T2S_TS2VEC_MAX_BLOCKS];
    float *proj_w, *proj_b;
} t2s_ts2vec_grads;
/* View row b is x[b, start[b] : start[b]+length] (start is clamped into [0, T-length] on the device). */
typedef struct t2s_ts2vec_view {
    const int32_t* start;   /* (B) device */
    const uint8_t* mask;    /* (B, length) device; 0 = the time step is hidden after input_fc */
    const uint8_t* keep;    /* (B, output_dims, length) device; the dropout draw: 0 = dropped, else multiplied by keep_scale */
    int length;             /* crop_l <= length <= T */
    int pad_;
} t2s_ts2vec_view;
typedef struct t2s_ts2vec_step {
    const float* x;         /* (B, T, input_dims) device */
    int B, T, crop_l;       /* the loss compares view 0's last crop_l steps with view 1's first crop_l */
    int temporal_unit;
    float alpha;            /* weight of the instance loss (the reference: 0.5) */
    float keep_scale;       /* 1 / (1 - p_dropout) as the caller's dropout evaluates it in fp32 */
    int x_nan_count;        /* NaNs the caller counted in x on the host; anything but 0 is refused (x is never read here) */
    int pad_;
    t2s_ts2vec_view view[2];
} t2s_ts2vec_step;
/* Bytes of workspace a step of up to max_B series x max_T time steps needs (0 and an error message if unsupported). */
uint64_t t2s_ts2vec_train_workspace_bytes(const t2s_ts2vec_weights* w, int max_B, int max_T);
/* Supported: what t2s_ts2vec_encode supports (equal hidden widths, depth < T2S_TS2VEC_MAX_BLOCKS, its LDS bound),
 * T <= 128, 1 <= B <= 16, NaN-free x; anything else is T2S_E_INVALID before any launch.  loss_out: device scalar.
 * A block whose dilation is >= a view's length contributes through its centre tap only: its outer-tap gradients are
 * exact zeros (no work is done for them).  A max-pool tie sends the gradient to the lower index (torch's rule). */
int t2s_ts2vec_train_step(const t2s_ts2vec_weights* w, const t2s_ts2vec_grads* grads, const t2s_ts2vec_step* step,
                          float* loss_out, void* workspace, uint64_t ws_bytes, void* stream);
/* torch.optim.swa_utils.AveragedModel.update_parameters for a whole parameter list in one launch:
 * avg += (p - avg) / (n_averaged + 1).  table_dev as for t2s_adamw_step_multi with `param` = the average and `grad` = the
 * current weights (exp_avg / exp_avg_sq unused); n_averaged >= 1 (the first update is a copy the host does). */
int t2s_swa_update_multi(const t2s_adamw_tensor* table_dev, int n_tensors, uint64_t total_chunks, int64_t n_averaged,
                         void* stream);

/* ------------------------------------------------------------------------ *
 * MLP denoiser of BASELINE configs[0]: model/denoiser/mlp.py:49-94 (MLPlayer x 8 on a
 * (64, 6) latent; forward, and the backward for train.py --denoiser MLP).
 * ------------------------------------------------------------------------ */
#define T2S_MLP_LAYERS 8
#define T2S_MLP_WIDTH 64      /* channels, mlp.py:52-56 */
#define T2S_MLP_POSITIONS 6   /* latent width the layer is built for, mlp.py:55,67 */
#define T2S_MLP_TEXT_DIM 128
#define T2S_MLP_HIDDEN 256
#define T2S_MLP_PACKED_FLOATS 397888 /* 8 x 49,736: what t2s_mlp_pack writes */
/* Device pointers to the state-dict tensors of layers.<i> that the forward reads (torch layouts).  cross_attn.query /
 * cross_attn.key are not among them: the six keys are the same row (mlp.py:77 repeats the text over the positions), every
 * softmax row is uniform and the attended value is value(text) whatever they hold.  norm1, norm3, pos_emb, self_attn,
 * self_attn2 are constructed and never called (mlp.py:53-60). */
typedef struct t2s_mlp_layer_weights {
    const float *value_w, *value_b; /* cross_attn.value (64,128), (64) */
    const float *proj_w, *proj_b;   /* cross_attn.proj  (64,64), (64)  */
    const float *norm2_w, *norm2_b; /* (64) */
    const float *mlp0_w, *mlp0_b;   /* mlp.0  (256,64), (256) */
    const float *mlp2_w, *mlp2_b;   /* mlp.2  (64,256), (64)  */
    const float *pos0_w, *pos0_b;   /* mlp2.0 (256,6), (256)  */
    const float *pos2_w, *pos2_b;   /* mlp2.2 (6,256), (6)    */
} t2s_mlp_layer_weights;
typedef struct t2s_mlp_weights {
    t2s_mlp_layer_weights layer[T2S_MLP_LAYERS];
} t2s_mlp_weights;
/* Transposes the weights into `packed` (T2S_MLP_PACKED_FLOATS floats, caller-owned device buffer).  Every pointer's
 * allocation extent is checked against the shape above.  Stateless: pack again after the weights change. */
int t2s_mlp_pack(const t2s_mlp_weights* w, float* packed, void* stream);
/* MLP.forward (mlp.py:90-94): x (B,64,6); t (B) fp32 (int64 timesteps converted by the host mirror exactly as
 * `t * 100.0` promotes them) and freqs (32) = 10000^linspace(0,1,32) as the caller evaluated it (mlp.py:12) for
 * TimeEmbedding(64), mlp.py:5-18; text (B,128) or NULL (mlp.py:75 skips the cross attention) -> out (B,64,6); out may
 * alias x.  One launch, one workgroup per series. */
int t2s_mlp_forward(const float* packed, const float* x, const float* t, const float* freqs, const float* text, float* out,
                    int B, void* stream);
/* Gradients of the same forward (train.py:123-125 with --denoiser MLP): every tensor of t2s_mlp_layer_weights, in its own layout. */
typedef struct t2s_mlp_layer_grads {
    float *value_w, *value_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *mlp0_w, *mlp0_b, *mlp2_w, *mlp2_b, *pos0_w, *pos0_b, *pos2_w,
        *pos2_b;
} t2s_mlp_layer_grads;
typedef struct t2s_mlp_grads {
    t2s_mlp_layer_grads layer[T2S_MLP_LAYERS];
} t2s_mlp_grads;
#define T2S_MLP_GRAD_PART_FLOATS 391744 /* 8 x 48,968: one series' contributions, what `scratch` holds per series */
/* Backward of t2s_mlp_forward for dout (B,64,6): the forward is recomputed from x (nothing else is saved); every series writes
 * its contribution to `scratch` (B x T2S_MLP_GRAD_PART_FLOATS floats, caller-owned) and the contributions are added in series
 * order -- bit-reproducible.  grads receives d loss / d parameter (overwritten, not accumulated); dx (B,64,6) the gradient of
 * x, or NULL.  `w` are the tensors `packed` was made from.  cross_attn.query / key get no gradient here: exact zeros are theirs. */
int t2s_mlp_backward(const t2s_mlp_weights* w, const float* packed, const float* x, const float* t, const float* freqs,
                     const float* text, const float* dout, float* dx, const t2s_mlp_grads* grads, float* scratch,
                     uint64_t scratch_floats, int B, void* stream);

/* ------------------------------------------------------------------------ *
 * TSae: the attention seq2seq codec of the motion models, model/pretrained/TSae.py
 * (AttentionSeq2SeqAutoencoder): pre-norm transformer encoder, teacher-forced
 * decoder, and the autoregressive generation with a key/value cache.  fp32.
 * ------------------------------------------------------------------------ */
#define T2S_TSAE_D_MODEL 64
#define T2S_TSAE_MAX_LAYERS 6
#define T2S_TSAE_MAX_T 2000      /* the reference's positional table */
#define T2S_TSAE_MAX_FEATURES 16
#define T2S_TSAE_MAX_D_FF 512
typedef struct t2s_tsae t2s_tsae;
/* Device pointers to the state-dict tensors, torch layouts (nn.MultiheadAttention, nn.Linear, nn.LayerNorm). */
typedef struct t2s_tsae_attn_weights {
    const float *in_proj_w, *in_proj_b;   /* (192,64), (192): q, k, v rows */
    const float *out_proj_w, *out_proj_b; /* (64,64), (64) */
} t2s_tsae_attn_weights;
typedef struct t2s_tsae_enc_layer { /* encoder.transformer_encoder.layers.<i> */
    t2s_tsae_attn_weights self_attn;
    const float *linear1_w, *linear1_b; /* (d_ff,64), (d_ff) */
    const float *linear2_w, *linear2_b; /* (64,d_ff), (64) */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} t2s_tsae_enc_layer;
typedef struct t2s_tsae_dec_layer { /* decoder.transformer_decoder.layers.<i> */
    t2s_tsae_attn_weights self_attn, multihead_attn;
    const float *linear1_w, *linear1_b, *linear2_w, *linear2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
} t2s_tsae_dec_layer;
typedef struct t2s_tsae_weights {
    int n_features, d_model, d_ff, heads, n_enc, n_dec;
    const float *value_embedding_w, *value_embedding_b; /* encoder.value_embedding (64,F), (64) */
    const float *embedding_ln_w, *embedding_ln_b;       /* encoder.embedding_ln (64) */
    t2s_tsae_enc_layer enc[T2S_TSAE_MAX_LAYERS];
    t2s_tsae_dec_layer dec[T2S_TSAE_MAX_LAYERS];
    const float *input_projection_w, *input_projection_b;   /* decoder.input_projection (64,F), (64) */
    const float *output_projection_w, *output_projection_b; /* decoder.output_projection (F,64), (F) */
} t2s_tsae_weights;
/* Reads every tensor once (extents checked), packs the transposes and the sinusoidal table (a function of position and channel,
 * computed here) into one device buffer the handle owns; later calls copy nothing.  Covered: d_model 64, heads 4 or 8, d_ff a
 * multiple of 64 up to 512, 1..6 layers on each side, 1..16 features; anything else is T2S_E_INVALID naming the value.  n_enc 0 or
 * n_dec 0 (not both) makes a one-sided handle: that side's tensors are not read, and its entries are T2S_E_INVALID.  After the
 * weights change, create again or call t2s_tsae_update_weights.  Synchronous (not for use inside a stream capture). */
int t2s_tsae_create(const t2s_tsae_weights* w, t2s_tsae** out);
void t2s_tsae_destroy(t2s_tsae* h);
/* Rows [first, first + count) of the handle's positional table -> pe (count,64), device. */
int t2s_tsae_positional(const t2s_tsae* h, float* pe, int first, int count, void* stream);
/* Bytes of workspace the three entries below need for (B, T) -- one size serves all three; 0 (and a message) out of range.
 * The entries allocate nothing and never synchronise; each refuses, before any launch and with its outputs untouched, T outside
 * 1..T2S_TSAE_MAX_T, B outside 1..65535, a NULL pointer and a workspace smaller than this.  A series' result is a function of that
 * series alone: bitwise the same at any B and any place in the batch, and from call to call. */
uint64_t t2s_tsae_workspace_bytes(const t2s_tsae* h, int B, int T);
/* x (B,T,F) -> memory (B,T,64): value embedding, LayerNorm, + position, n_enc pre-norm layers (unmasked attention, ReLU FFN),
 * no final norm.  1 + 4 n_enc launches. */
int t2s_tsae_encode(const t2s_tsae* h, const float* x, float* memory, int B, int T, void* workspace, uint64_t workspace_bytes,
                    void* stream);
/* Teacher-forced decoder: memory (B,T,64), target (B,T,F) -> prediction (B,T,F).  Input row 0 is the zero BOS row, row i > 0
 * input_projection(target[i-1]); + position; n_dec pre-norm layers (causal self-attention, cross-attention over the T memory rows,
 * ReLU FFN); output_projection.  3 + 7 n_dec launches. */
int t2s_tsae_decode(const t2s_tsae* h, const float* memory, const float* target, float* prediction, int B, int T, void* workspace,
                    uint64_t workspace_bytes, void* stream);
/* decoder.generate: memory (B,S,64) -> series (B,S,F), autoregressively.  One launch projects the memory to every layer's
 * cross-attention K / V, one launch (a workgroup per series) runs all S steps with the self-attention K / V cached in the workspace. */
int t2s_tsae_generate(const t2s_tsae* h, const float* memory, float* series, int B, int S, void* workspace, uint64_t workspace_bytes,
                      void* stream);

/* ---- TSae training: the teacher-forced step  prediction = decoder(memory = encoder(x), target_seq = x)  in training mode ---- */
#define T2S_TSAE_TRAIN_MAX_T 192 /* trained lengths: a whole head's K and V rows stay in LDS */
/* Re-reads every tensor of `w` into the handle's blob on the caller's stream (one launch): no allocation, no synchronisation, the
 * positional table is not recomputed.  The shape fields of `w` must equal the handle's; a one-sided handle reads its side only.
 * Afterwards every entry computes what a fresh handle on the same tensors computes, bit for bit. */
int t2s_tsae_update_weights(t2s_tsae* h, const t2s_tsae_weights* w, void* stream);
/* Dropout of the training entries.  Nothing is stored: element e of series b at site s is KEPT iff u >= p, u the value
 * t2s_philox_uniform defines for (seed, stream_id = s, row = b, element e), p the fp32 dropout probability; kept values are
 * multiplied by the fp32 1 / (1 - p).  At p == 0 no Philox work is done.  The element index:
 *   a row site of width W (64; d_ff for the FFN hidden rows):  e = t * W + c        (row t, column c)
 *   an attention site (the softmax probabilities, not renormalised):  e = (h * T + i) * T + j   (head, query, key)
 * The sites:
 *   0  encoder embedding_dropout          1  encoder positional_encoding.dropout          2  decoder positional_encoding.dropout
 *   16 + 4 i + k  encoder layer i:  k = 0 attention probabilities, 1 dropout1 (after attention), 2 dropout (FFN hidden), 3 dropout2
 *   64 + 6 i + k  decoder layer i:  k = 0 self-attention probabilities, 1 dropout1, 2 cross-attention probabilities, 3 dropout2,
 *                                   4 dropout (FFN hidden), 5 dropout3
 * The training entries below need a two-sided handle, 1 <= T <= T2S_TSAE_TRAIN_MAX_T, 1 <= B <= 65535 and 0 <= p_drop < 1; they
 * run on the caller's stream, never allocate or synchronise, keep no state outside the workspace, and refuse with T2S_E_INVALID,
 * before any launch, anything else, a NULL pointer and a workspace smaller than t2s_tsae_train_workspace_bytes (0 and a message on
 * a bad argument). */
uint64_t t2s_tsae_train_workspace_bytes(const t2s_tsae* h, int B, int T);
/* x (B,T,F) -> prediction (B,T,F), every activation the backward needs left in the workspace.  2 + 5 n_enc + 9 n_dec + 1 launches. */
int t2s_tsae_train_forward(const t2s_tsae* h, const float* x, float* prediction, int B, int T, float p_drop, uint64_t seed,
                           void* workspace, uint64_t workspace_bytes, void* stream);
/* The gradients: the fields of t2s_tsae_weights, written through (the library casts the const away); the shape fields are not read. */
typedef t2s_tsae_weights t2s_tsae_grads;
/* d_prediction (B,T,F) -> d loss / d (every tensor that takes part), torch layouts, written (not accumulated); the sums over
 * (series, row) run in an order that depends on (B, T, shape) only, so a step repeats bit for bit.  x, B, T, p_drop, seed and the
 * workspace are those of the matching t2s_tsae_train_forward, the workspace untouched in between.  No gradient for x. */
int t2s_tsae_train_backward(const t2s_tsae* h, const float* x, const float* d_prediction, const t2s_tsae_grads* g, int B, int T,
                            float p_drop, uint64_t seed, void* workspace, uint64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T2S_H */
