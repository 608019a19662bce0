/*
 * w2v2.h -- C ABI of the MI355X-native Wav2Vec2 forward / CTC path.
 *
 * The reference (thevasudevgupta/gsoc-wav2vec2) has NO plugin / operator / FFI
 * interface: its hot path sits behind a plain Python package surface
 * (src/wav2vec2/__init__.py:1-4) and every arithmetic op is a TensorFlow call.
 * This header is therefore the boundary a maintainer of that package would
 * bind *instead of* TensorFlow: each entry point names the reference call it
 * replaces.  The Python host side (gsoc-wav2vec2_amd/wav2vec2) binds it with
 * ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns 0 on success, a negative W2V2_E* code on failure;
 *     w2v2_last_error() returns a thread-local message.  No exceptions cross
 *     the ABI.
 *   - `*_dev` pointers are HIP device pointers (fp32 unless stated), owned by
 *     the caller; `*_host` pointers are host memory.  The model owns its
 *     weights and its activation workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     work is enqueued on it; nothing synchronises unless stated.
 *   - one model per stream at a time; the library is not thread-safe per model.
 *   - activations are channels-last (batch, time, channels), as in the
 *     reference; kernels are (K, C_in, C_out) / (in, out) -- the reference's
 *     TF checkpoint layout (src/convert_torch_to_tf.py:110-117).
 */
#ifndef W2V2_H_
#define W2V2_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2V2_MAX_CONV_LAYERS 16

enum {
    W2V2_OK = 0,
    W2V2_EINVAL = -1,     /* bad argument / shape / config           */
    W2V2_ENOTFOUND = -2,  /* unknown parameter or activation name    */
    W2V2_EHIP = -3,       /* a HIP runtime call failed               */
    W2V2_ESTATE = -4      /* call order (e.g. forward before all params are set) */
};

/* Mirrors Wav2Vec2Config (reference src/wav2vec2/config.py:6-60); only the
 * fields the forward / CTC arithmetic reads.  dropout, survival_prob and the
 * spec-augment fields are train-time host concerns. */
typedef struct w2v2_config {
    int32_t vocab_size;
    int32_t hidden_size;
    int32_t num_heads;
    int32_t num_layers;
    int32_t intermediate_size;
    int32_t num_conv_pos_embeddings;
    int32_t num_conv_pos_embedding_groups;
    int32_t num_conv_layers;
    int32_t filter_sizes[W2V2_MAX_CONV_LAYERS];
    int32_t kernal_sizes[W2V2_MAX_CONV_LAYERS];   /* sic: the reference's spelling is API */
    int32_t strides[W2V2_MAX_CONV_LAYERS];
    int32_t conv_bias;                    /* 0 / 1 */
    int32_t feature_extractor_norm_type;  /* 0 = "group", 1 = "layer"        */
    int32_t attention_norm_type;          /* 0 = "postnorm", 1 = "prenorm"   */
    int32_t is_gelu_approx;               /* 0 = exact erf GELU              */
    int32_t with_lm_head;                 /* 1 = Wav2Vec2ForCTC, 0 = Wav2Vec2Model */
    int32_t pad_id;                       /* CTC blank index                 */
    float   layer_norm_eps;
} w2v2_config;

typedef struct w2v2_model w2v2_model;

const char* w2v2_last_error(void);
const char* w2v2_version(void);
/* Free the library-owned per-(device, stream) scratch buffers (split-K slabs, CTC alpha / beta, the aligners' workspaces) and the
 * per-device pinned buffers their host tables are staged in, of the calling thread's current device; they are otherwise kept,
 * grow-only, for the life of the process.  The device must be idle. */
int w2v2_release_scratch(void);

/* ---- model lifetime ------------------------------------------------------
 * Replaces Wav2Vec2Model.__init__ / Wav2Vec2ForCTC.__init__
 * (reference modeling.py:105-167, 217-233): allocates every variable on the
 * current HIP device (zero-filled). */
int  w2v2_create(const w2v2_config* cfg, w2v2_model** out);
void w2v2_destroy(w2v2_model* m);

/* Variable inventory, named as the reference's TF variables without the model
 * prefix and ":0" (convert_torch_to_tf.py:12-44), e.g.
 * "encoder/layers/3/attention/q_proj/kernel", "lm_head/bias". */
int w2v2_num_params(const w2v2_model* m);
int w2v2_param_info(const w2v2_model* m, int index, const char** name,
                    int64_t shape[4], int* rank);

/* Replaces model.load_weights / keras batch_set_value
 * (modeling.py:82, convert_torch_to_tf.py:121): copy one variable host->device.
 * `shape`/`rank` must match the inventory. */
int w2v2_set_param(w2v2_model* m, const char* name, const float* host_src,
                   const int64_t* shape, int rank);
/* Replaces model.variables[i].numpy() (convert_torch_to_tf.py:81). */
int w2v2_get_param(w2v2_model* m, const char* name, float* host_dst, int64_t numel);

/* Derives the tensors the kernels consume from the variables: the
 * weight-normalised positional kernel  l2_normalize(weight_v,[1,2])*weight_g
 * (tensorflow_addons.py:16-21) regrouped per conv group, and the packed
 * q|k|v projection.  Must be called after the last w2v2_set_param and before
 * w2v2_forward; enqueued on `stream`. */
int w2v2_finalize(w2v2_model* m, void* stream);

/* Frames out of the conv stack for `num_samples` input samples:
 * 1 + (len - k) // s per layer (modeling.py:202-204, losses.py:47-56). */
int64_t w2v2_num_frames(const w2v2_model* m, int64_t num_samples);

/* Arithmetic of the dense contractions (Conv1D layers 1..6 and every Dense, forward and backward):
 *   W2V2_PRECISION_FP32  v_mfma_f32_32x32x2_f32 on fp32 operands -- the reference's arithmetic (default);
 *   W2V2_PRECISION_BF16  operands rounded to bf16 (nearest-even) on the way into LDS, fp32 accumulation,
 *                        fp32 bias / GELU / residual / storage: what BASELINE configs "bf16 CTC fine-tune"
 *                        ask for (mixed precision; variables, optimizer state and activations stay fp32).
 *                        Attention (head size 64) takes bf16 q, k, v and probabilities on the same pipe with
 *                        fp32 scores / softmax / accumulation; the grouped positional conv runs as one batched
 *                        GEMM with bf16-rounded input and kernel.  In the TRAINING step of this mode four tensors that sit
 *                        between two roundings are also stored as bf16 (as a mixed_bfloat16 Dense would hand them on): the
 *                        FFN pre-activation (GELU and GELU' see bf16(u)), the gradient of the FFN hidden activation, the
 *                        attention output and its gradient (D = rowsum(dO o O) is taken from the bf16 values).  The
 *                        residual stream, LayerNorm inputs / outputs and every gradient of them stay fp32.
 *   W2V2_PRECISION_BF16X3  fp32 results from the bf16 matrix cores (forward, and the data-gradient GEMMs of the
 *                        training step): every fp32 operand is written
 *                        exactly as a sum of three bf16 terms and each fp32 product is evaluated as the six bf16 x bf16
 *                        products of order <= 2, accumulated in fp32 (the dropped terms are < 2^-23 of the product, below
 *                        the rounding of an fp32 running sum).  Same fp32 inputs, outputs and error level as
 *                        W2V2_PRECISION_FP32 -- logits within the same 1e-3 of the reference -- at the bf16 pipe's rate.
 *                        Attention (head size 64) takes the same route; shapes the split kernels do not take, the
 *                        positional conv, the weight-gradient GEMMs and the training attention stay on the fp32 MFMA.
 *                        In the inference forward the producers of the GEMM operands (conv0, LayerNorm, the GEMM and attention
 *                        epilogues) write the three planes themselves and the GEMMs stream them (gemm_split_sw.hip).
 *   W2V2_PRECISION_F16X2   fp32-grade results from the fp16 matrix cores at HALF the MFMA work of BF16X3 (inference forward):
 *                        an operand is the sum of TWO fp16 terms of x 2^e (22 significant bits; e = 4 for activations, chosen
 *                        from max |w| for a weight), a product keeps a0 b0 + a0 b1 + a1 b0.  The error per product (~2^-22) is
 *                        below what an fp32 running sum over K >= 64 products commits: measured GEMM error at or below the
 *                        fp32 MFMA kernel's, logits within the same bar.  Domain: |activation| < 4094 (a larger value
 *                        saturates and sets a sticky flag, w2v2_range_overflow).  GEMM shapes its kernel does not take, the
 *                        attention core and the training step run as in BF16X3.
 * Everything else (conv0 + GroupNorm, LayerNorm, softmax, CTC) is fp32 in all modes. */
#define W2V2_PRECISION_FP32 0
#define W2V2_PRECISION_BF16 1
#define W2V2_PRECISION_BF16X3 2
#define W2V2_PRECISION_F16X2 3
int w2v2_set_precision(w2v2_model* m, int32_t mode);
int w2v2_get_precision(const w2v2_model* m);

/* Per-model switches of the bf16 precision mode (no environment variable is read anywhere in the library):
 *   W2V2_OPT_BF16_SHADOWS (default 1)      0 = no bf16 operand shadows: every GEMM rounds its fp32 operands itself.  Same
 *                                          results bit for bit, slower; the parity tests flip it to prove exactly that.
 *   W2V2_OPT_KEEP_ACTIVATIONS (default 0)  1 = also write the fp32 copies of stage outputs whose only reader streams the bf16
 *                                          shadow, so w2v2_copy_activation can tap them (otherwise such a tap is an error).
 *   W2V2_OPT_SPLIT_PLANES (default 1)      precision modes BF16X3 / F16X2: 0 = no operand planes written by the producers; the
 *                                          forward GEMMs then load fp32 rows and split them in registers (gemm_split.hip, six
 *                                          bf16 products in both modes) -- the round-4 path, kept for A/B measurements.
 *   W2V2_OPT_WGRAD_STREAM (default 0)      bf16 training backward: 1 = the encoder layers' weight-gradient GEMMs run on a second,
 *                                          lower-priority HIP stream owned by the model, ordered against the caller's stream by
 *                                          events only (w2v2_train_backward returns with the caller's stream waiting for all of it;
 *                                          bucket events then come from that stream).  Same results bit for bit; measured neutral
 *                                          on one GPU (profiles/history.md 7.1), hence off.
 *   W2V2_OPT_DEFER_FOLDS (default 1)       training backward: the small reductions that finish an encoder layer's gradients (split-K
 *                                          slab sums of the four weight gradients, the q|k|v unpack, the LayerNorm / dropout /
 *                                          attention column-sum folds: nine launches per layer) run as ONE launch in front of the
 *                                          layer's bucket event.  Same summation order, same bits; 0 = one launch behind each
 *                                          producer (the round-4 behaviour, kept for the bit-identity test and A/B timing).
 *   W2V2_OPT_BF16_PACKED (default 0)       1 = w2v2_forward_packed, w2v2_forward_windows and everything built on them accept
 *                                          W2V2_PRECISION_BF16: attention and the positional conv take segment forms of the bf16
 *                                          kernels, each utterance as w2v2_forward computes it alone in that mode.  bf16-grade
 *                                          logits (what torch.autocast(bfloat16) costs the model): for decoding, not for exact
 *                                          scores.  0 = the mode is refused there, as before the option existed.  No effect on
 *                                          the other precision modes.
 * w2v2_get_option returns the value, or W2V2_EINVAL for an unknown option. */
#define W2V2_OPT_BF16_SHADOWS 0
#define W2V2_OPT_KEEP_ACTIVATIONS 1
#define W2V2_OPT_SPLIT_PLANES 2
#define W2V2_OPT_WGRAD_STREAM 3
#define W2V2_OPT_DEFER_FOLDS 4
#define W2V2_OPT_BF16_PACKED 5
int w2v2_set_option(w2v2_model* m, int32_t option, int32_t value);
int w2v2_get_option(const w2v2_model* m, int32_t option);
/* W2V2_PRECISION_F16X2: *flag = 1 if a forward since the last call met an activation outside fp16's range after scaling
 * (|x| >= 4094: its planes were saturated, the logits of that forward are NOT fp32-grade -- rerun in BF16X3 or FP32); clears the
 * flag.  Synchronises `stream`.  Always 0 in the other modes. */
int w2v2_range_overflow(w2v2_model* m, int32_t* flag, void* stream);

/* ---- the hot path --------------------------------------------------------
 * Replaces Wav2Vec2ForCTC.call / Wav2Vec2Model.call at training=False
 * (modeling.py:169-209, 239-255).
 *   wave_dev   (B, L) fp32 waveform, already normalised + padded by the caller
 *   mask_dev   (B, L) int32 0/1 attention mask, or NULL (base checkpoints)
 *   out_dev    (B, T, vocab) logits if with_lm_head else (B, T, hidden);
 *              T = w2v2_num_frames(L)
 * The first call for a new (B, L) allocates the activation workspace
 * (hipMalloc; not capturable); later calls with B*L no larger reuse it. */
int w2v2_forward(w2v2_model* m, const float* wave_dev, int32_t B, int64_t L,
                 const int32_t* mask_dev, float* out_dev, void* stream);

/* Packed variable-length inference forward (training=False): n utterances in one call, each computed as
 * w2v2_forward computes it alone (B = 1, no mask).
 *   wave_dev         (sum len_i) fp32, the utterances back to back, each already normalised
 *   cu_samples_host  (n + 1) int64 prefix offsets, cu_samples_host[0] = 0
 *   out_dev          (sum T_i, vocab | hidden), T_i = w2v2_num_frames(len_i); utterance i at row sum_{j<i} T_j
 * Precision modes W2V2_PRECISION_FP32, _BF16X3 and _F16X2, and W2V2_PRECISION_BF16 once W2V2_OPT_BF16_PACKED is set (without the
 * option it gives W2V2_EINVAL naming the mode; with it, each utterance carries w2v2_forward's bf16-grade logits).  In
 * f16x2 the same range contract as w2v2_forward holds: poll w2v2_range_overflow.  Every len_i must give T_i >= 1.
 * The utterances run as one stream with each start aligned to the conv stack's total stride; only conv0's GroupNorm
 * statistics, the positional conv and attention see utterance boundaries.  The 1-2 stream rows behind each utterance
 * are zeroed where only those stages would write them, so nothing of an earlier call is read.  The workspace is sized from the aligned
 * stream length, rounded up; a later packed call whose stream fits reuses it.  Synchronises with the previous packed
 * call's table upload (host-side), otherwise enqueued on `stream`. */
int w2v2_forward_packed(w2v2_model* m, const float* wave_dev, int32_t n, const int64_t* cu_samples_host,
                        float* out_dev, void* stream);

/* Windowed inference forward for long recordings: n windows of ONE device buffer in one call, each computed as
 * w2v2_forward computes it alone (B = 1, no mask), and a range of each window's frames kept.  w2v2_forward_packed is the special
 * case sample0 = cu_samples, every frame kept, normalize = 0, and shares the body: layout, workspace, precision modes, the range
 * contract of f16x2 and the synchronisation are as described there.  One difference: conv0's GroupNorm statistics are taken per
 * window in the form w2v2_forward takes them, so that in fp32 a window's rows carry the bits w2v2_forward gives that window alone;
 * w2v2_forward_packed keeps its own summation (and its bits), which agrees with w2v2_forward to the fp32 bar.
 *   wave_dev       (wave_samples) fp32
 *   window i       wave_dev[sample0_host[i] .. sample0_host[i] + samples_host[i]); windows may overlap and need not be ordered
 *   keep0_host, keepn_host   rows [keep0_i, keep0_i + keepn_i) of window i's w2v2_num_frames(samples_i) output rows are kept
 *   normalize      1: every window is normalised over its own samples as Wav2Vec2Processor._normalize does it,
 *                  (x - mean) / sqrt(var + 1e-5) with the population variance; mean and variance accumulate in fp64 (two passes, a
 *                  fixed reduction order, no atomics: deterministic) and the quotient is formed in fp64 and rounded once to fp32.
 *                  0: the samples are used as they are
 *   out_dev        (sum keepn_i, vocab | hidden); window i's kept rows at row sum_{j<i} keepn_j
 * W2V2_EINVAL with a message naming the window: a window outside [0, wave_samples), shorter than the receptive field, keepn_i == 0,
 * a kept range outside the window's frames; also precision W2V2_PRECISION_BF16 without W2V2_OPT_BF16_PACKED (naming the mode) and
 * normalize outside {0, 1}.  In W2V2_PRECISION_BF16 with the option a window's rows carry the bits w2v2_forward gives it alone in that mode. */
int w2v2_forward_windows(w2v2_model* m, const float* wave_dev, int64_t wave_samples, int32_t n, const int64_t* sample0_host,
                         const int64_t* samples_host, const int32_t* keep0_host, const int32_t* keepn_host, int32_t normalize,
                         float* out_dev, void* stream);

/* Replaces CTCLoss.call (losses.py:14-45) = tf.nn.ctc_loss(
 * logits_time_major=False, blank_index=pad_id) with the reference's length
 * convention supplied by the caller:
 *   logits_dev       (B, T, V) fp32
 *   labels_dev       (B, U) int32, label_length_dev (B) int32  (count of labels != pad)
 *   logit_length_dev (B) int32 (the reference passes the full T for every row)
 *   nll_dev          (B) fp32 per-sample negative log-likelihood (not divided,
 *                    not reduced: division_factor and the SUM are the caller's)
 *   grad_logits_dev  (B, T, V) fp32 d(sum_b nll_b)/d logits, or NULL to skip */
int w2v2_ctc_loss(const float* logits_dev, int32_t B, int32_t T, int32_t V,
                  const int32_t* labels_dev, int32_t U,
                  const int32_t* label_length_dev, const int32_t* logit_length_dev,
                  int32_t blank, float* nll_dev, float* grad_logits_dev, void* stream);
/* The same with CTCLoss.call's conventions evaluated on the device, so that the caller issues no tensor arithmetic around the call
 * (the training step: no framework kernels between the forward and the backward; capturable):
 *   label_length = count of labels != blank per row (losses.py:32-33); logit_length = logit_length_all for every row (losses.py:29-30:
 *   the full frame count); grad_logits_dev = d(sum_b nll_b) / d logits / division_factor (losses.py:45: a DIVISION, as the reference
 *   computes it -- multiplying by a rounded reciprocal differs by an ulp for factors that are not powers of two);
 *   loss_sum_dev (optional device scalar) = sum_b (nll_b / division_factor), added in row order (Keras Reduction.SUM, losses.py:6). */
int w2v2_ctc_loss_fused(const float* logits_dev, int32_t B, int32_t T, int32_t V, const int32_t* labels_dev, int32_t U,
                        int32_t logit_length_all, int32_t blank, float division_factor, float* nll_dev, float* grad_logits_dev,
                        float* loss_sum_dev, void* stream);

/* CTC forced alignment (Viterbi; DESIGN.md §11, exact definition in csrc/align.hip): the single best frame-level path that spells
 * each utterance's labels.  Model-free, like w2v2_ctc_loss; asynchronous on `stream`.
 *   utterance i: logits_dev rows [row0_host[i], row0_host[i] + frames_host[i]) (rows of V fp32: the packed output of
 *                w2v2_forward_packed back to back, or a padded (B, T, V) batch with row0 = b T), labels
 *                labels_dev[label0_host[i] .. label0_host[i] + nlabels_host[i]) (int32, on the device)
 *   token_dev, label_index_dev, frame_logp_dev  (sum_i frames_i), utterance after utterance: the path's token (blank or label),
 *                the label's index k (-1 on a blank), log_softmax(logits[t])[token] (fp32)
 *   score_dev    (n) fp64 log-probability of the path
 * frames_i >= 1, 0 <= nlabels_i <= W2V2_ALIGN_MAX_LABELS, blank in [0, V): otherwise W2V2_EINVAL.  Per utterance, with its neighbours
 * unaffected: frames_i < nlabels_i + (count of labels equal to the one before) gives score -inf; a label outside [0, V) or equal to
 * the blank gives score NaN; both with token = label_index = -1 and frame_logp NaN.  Synchronises with the previous call's table
 * upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_ALIGN_MAX_LABELS 8191
int w2v2_ctc_align(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                   const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host, int32_t blank,
                   int32_t* token_dev, int32_t* label_index_dev, float* frame_logp_dev, double* score_dev, void* stream);

/* CTC forced alignment of whole recordings (csrc/align_long.hip): w2v2_ctc_align without the label limit.  The same
 * definition, addressing and outputs, and the same bits: every output, the score included, is identical to w2v2_ctc_align's wherever
 * that one accepts the input, and to the fp64 reference on every input (ties, -inf and NaN logits included).  nlabels_i is any
 * non-negative int32.  The plane of frames x states runs as tiles: a strip of `strip_pairs` state pairs (blank 2k, label 2k + 1) by a
 * panel of `panel_frames` steps, one kernel launch per anti-diagonal of tiles over all recordings of the call; stream order is the
 * only synchronisation between tiles (no block waits for another, no atomics), so results do not depend on the other recordings of
 * the call, their order, the geometry, or repetition.
 *   strip_pairs   0 (the measured default) or a multiple of 64 in [64, 8192]; a strip is never wider than the longest recording needs
 *   panel_frames  0 (the measured default) or a multiple of 8 that is >= 8
 *   max_workspace_bytes  cap of the library-owned scratch of the call; 0 = 32 GiB.  The scratch holds the tile table, lse, one carry
 *                 row (8 S_i bytes) and the strips' boundary columns (8 T_i strips_i bytes) per recording, and 2 bits of backpointer
 *                 per frame and state, about T_i (U_i + 1) / 2 bytes: 5 GB for one hour of speech (180 000 frames, 54 000
 *                 labels), growing with the product.  A call that needs more returns W2V2_EINVAL, its message naming the bytes,
 *                 BEFORE anything is allocated.
 * Anything else outside the ranges above is W2V2_EINVAL, with w2v2_ctc_align's other argument checks (frames_i >= 1, non-negative
 * offsets, blank in [0, V), no null pointer, n >= 1).  Infeasible recordings and bad device labels as w2v2_ctc_align, neighbours
 * unaffected.  The scratch is grow-only per (device, stream) like the library's other scratch: w2v2_release_scratch gives it back.
 * Synchronises with the previous call's table upload (host-side), otherwise enqueued on `stream`.
 *
 * w2v2_ctc_align_long_workspace: host only; the bytes of scratch a call of these shapes and this geometry needs (INT64_MAX when the
 * figure does not fit), or a negative W2V2_E* for arguments the call itself would refuse. */
int w2v2_ctc_align_long(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                        const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host, int32_t blank,
                        int32_t* token_dev, int32_t* label_index_dev, float* frame_logp_dev, double* score_dev,
                        int32_t strip_pairs, int32_t panel_frames, int64_t max_workspace_bytes, void* stream);
int64_t w2v2_ctc_align_long_workspace(int32_t n, const int32_t* frames_host, const int32_t* nlabels_host, int32_t strip_pairs,
                                      int32_t panel_frames);

/* Forced alignment with a wildcard label, the "star", for transcripts that do not spell everything that is spoken (DESIGN.md §21,
 * exact definition in csrc/align.hip).  The three calls are w2v2_ctc_align, w2v2_ctc_align_long and
 * w2v2_ctc_align_long_workspace with one more label id: V, the star, as if the logits had one more column whose raw-logit value at
 * frame t is max_v logits[t][v] + star_score (the fp32 maximum over all V columns, the blank included, widened to fp64 before the
 * sum).  A star may stand anywhere in a label string and absorbs whatever is spoken there; it occupies at least one frame, and the
 * recursion, its ties, the end state and the feasibility rule frames_i >= nlabels_i + repeats (V counts like any id) are unchanged.
 *   star_score   fp32, <= 0, nats per frame: a star frame costs what the greedy path pays for the frame, plus star_score.  NaN or
 *                > 0 is W2V2_EINVAL.
 *   outputs      on a star frame token = V, label_index = k, frame_logp = (float)(max + star_score - lse).  score is the score of
 *                the path: with a star in the labels it is no longer the log-probability of a label string.
 * A label < 0, > V or equal to the blank gives the NaN utterance.  Labels without a star give w2v2_ctc_align's bits.  The workspace
 * of the _long call holds one more fp64 per frame than w2v2_ctc_align_long's. */
int w2v2_ctc_align_star(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                        const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host, int32_t blank,
                        float star_score, int32_t* token_dev, int32_t* label_index_dev, float* frame_logp_dev, double* score_dev,
                        void* stream);
int w2v2_ctc_align_long_star(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                             const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host, int32_t blank,
                             float star_score, int32_t* token_dev, int32_t* label_index_dev, float* frame_logp_dev,
                             double* score_dev, int32_t strip_pairs, int32_t panel_frames, int64_t max_workspace_bytes, void* stream);
int64_t w2v2_ctc_align_long_star_workspace(int32_t n, const int32_t* frames_host, const int32_t* nlabels_host, int32_t strip_pairs,
                                           int32_t panel_frames);

/* Exact CTC scoring (exact definition in csrc/score.hip): the log-probability of a label string given an utterance's
 * logits, summed over every frame path that spells it (-ctc_loss in fp64), for m (utterance, label string) pairs in one call.
 * Model-free, like w2v2_ctc_align, and with its addressing of the utterances; asynchronous on `stream`.
 *   utterance i: logits_dev rows [row0_host[i], row0_host[i] + frames_host[i]) of V fp32 (read in place; pairs share rows)
 *   pair j:      scores utterance utt_of_host[j] against labels_dev[label0_host[j] .. label0_host[j] + nlabels_host[j]) (int32, device)
 *   logp_dev     (m) fp64, in the caller's order
 * n >= 1, m >= 1, V >= 2, frames_i >= 1, utt_of_j in [0, n), 0 <= nlabels_j <= W2V2_SCORE_MAX_LABELS, non-negative offsets, blank in
 * [0, V), no null pointer: otherwise W2V2_EINVAL, before anything is launched.  Per pair, the others unaffected: frames < nlabels +
 * (count of labels equal to the one before) gives -inf (a result, not an error); a label outside [0, V) or equal to the blank gives
 * NaN; an utterance with a NaN or +inf logit gives NaN for each of its pairs; -inf logits are legal.  fp64 log space: nothing
 * underflows.  No atomics; a pair's bits do not depend on the other pairs, their order or repetition.  Synchronises with the previous
 * call's table upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_SCORE_MAX_LABELS 8191
int w2v2_ctc_score(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host, int32_t m,
                   const int32_t* utt_of_host, const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host,
                   int32_t blank, double* logp_dev, void* stream);

/* The gradient of a weighted sum of exact CTC log-probabilities (exact definition in csrc/score.hip): per
 * utterance, grad = sum_j coef_j d logp_j / d logits over its pairs, with w2v2_ctc_score's addressing, argument checks and per-pair
 * conventions; asynchronous on `stream`.  coef = -1 on one pair per utterance is the CTC loss in fp64 log space; coef_j = P_j (W_j - L)
 * is an expected risk over an n-best list.
 *   coef_dev     (m) fp64, in the caller's order
 *   logp_dev     (m) fp64, out: the bits w2v2_ctc_score gives for the same pairs
 *   grad_dev     fp32, rows addressed like logits_dev: every row of every utterance is written (zeros where no pair contributes);
 *                rows outside the utterances are not touched
 * A pair whose logp is -inf or NaN contributes nothing.  No float atomics: two runs give the same bits, and an utterance's rows do
 * not depend on the other utterances, their pairs or their position.  The workspace holds frames_i (2 nlabels_j + 2) fp64 per pair;
 * w2v2_ctc_score_grad_workspace returns the bytes of one pass over the call (host only; a negative W2V2_E* for bad shapes).  A call
 * that needs more than max_workspace_bytes (0: 8 GiB) runs the utterances in consecutive groups that fit, stream-ordered, with
 * identical results; if one utterance's pairs alone do not fit, W2V2_EINVAL before anything is allocated, the message naming the
 * utterance and the bytes.  Nothing is launched or written on W2V2_EINVAL. */
int w2v2_ctc_score_grad(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                        int32_t m, const int32_t* utt_of_host, const int32_t* labels_dev, const int64_t* label0_host,
                        const int32_t* nlabels_host, int32_t blank, const double* coef_dev, double* logp_dev, float* grad_dev,
                        int64_t max_workspace_bytes, void* stream);
int64_t w2v2_ctc_score_grad_workspace(int32_t n, const int32_t* frames_host, int32_t m, const int32_t* utt_of_host,
                                      const int32_t* nlabels_host, int32_t V);

/* Exact CTC scoring and its gradient with the star, the wildcard label of w2v2_ctc_align_star (exact definition in
 * csrc/score.hip): the arguments, checks and per-pair conventions of w2v2_ctc_score / w2v2_ctc_score_grad plus
 *   labels_dev   may hold V, the star: a state like any other that takes at least one frame and counts as a label in the frame check
 *   star_score   fp32, <= 0, nats per frame: a star frame emits (frame maximum + star_score) - lse.  NaN or > 0 is W2V2_EINVAL,
 *                before anything is launched.
 * With a star in the labels logp is the score of a set of paths, not a log-probability (it may exceed 0); it is never below the
 * score w2v2_ctc_align_star gives for the same input.  In the gradient a star state emits the frame's top token: its occupancy is
 * added to the lowest column that holds the frame's maximum.  A label < 0, > V or equal to the blank gives NaN.  Pairs without a
 * star give the bits of w2v2_ctc_score / w2v2_ctc_score_grad, alone or mixed with star pairs.  The gradient's workspace holds two
 * more arrays per frame (fp64 and int32) than w2v2_ctc_score_grad's; grouping under max_workspace_bytes changes no bit. */
int w2v2_ctc_score_star(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host, int32_t m,
                        const int32_t* utt_of_host, const int32_t* labels_dev, const int64_t* label0_host,
                        const int32_t* nlabels_host, int32_t blank, float star_score, double* logp_dev, void* stream);
int w2v2_ctc_score_grad_star(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                             int32_t m, const int32_t* utt_of_host, const int32_t* labels_dev, const int64_t* label0_host,
                             const int32_t* nlabels_host, int32_t blank, float star_score, const double* coef_dev,
                             double* logp_dev, float* grad_dev, int64_t max_workspace_bytes, void* stream);
int64_t w2v2_ctc_score_grad_star_workspace(int32_t n, const int32_t* frames_host, int32_t m, const int32_t* utt_of_host,
                                           const int32_t* nlabels_host, int32_t V);

/* CTC phrase search (csrc/spot.hip): where in a recording a label string is spoken, for m (recording, phrase) pairs
 * in one call.  Model-free, with w2v2_ctc_score's addressing of recordings and pairs; asynchronous on `stream`.
 *   recording i: logits_dev rows [row0_host[i], row0_host[i] + frames_host[i]) of V fp32 (read in place; pairs share rows)
 *   pair j:      searches recording utt_of_host[j] for labels_dev[label0_host[j] .. + nlabels_host[j]) (int32, device), l_0 .. l_{U-1}
 * Definition.  S = 2U - 1 states, ext[2k] = l_k, ext[2k + 1] = blank: no leading or trailing blank state, a hit begins on a frame of
 * its first label and ends on a frame of its last.  m_t = max_v x_t(v) (fp32); e_t(v) = (double)x_t(v) - (double)m_t, <= 0 and 0 for
 * the argmax: a path's score is ln P(path) - ln P(greedy path) over the same frames.  A state carries a score d (fp64) and the begin
 * frame b (int32) of the path that produced it; before frame 0 d = -inf, b = -1.  At frame t the candidates of state s are taken
 * in this order, each compared with a strict > against the best so far: (1) stay, (d_{t-1}(s), b_{t-1}(s)); (2) s >= 1: from s - 1;
 * (3) s >= 2, s even and ext[s] != ext[s-2]: from s - 2; (4) s == 0: the fresh start (0.0, t).  d_t(s) = chosen + e_t(ext[s]), b_t(s)
 * the chosen begin, so ties keep the earlier begin.  The phrase ends at t with z_t = d_t(S-1), c_t = b_t(S-1).
 * Recording edges, delim >= 0 and U >= 3 only (delim = -1: off): l_0 == delim: state 2 also gets the fresh start (0.0, 0) at t = 0,
 * compared last; l_{U-1} == delim: at t = T - 1, d_t(S-2) and then d_t(S-3) also compete for (z, c), each with strict >.
 * Hits, one pass over t with thr = min_score_host[j]: frame t is a candidate (z_t, c_t, t) when z_t >= thr and z_t > -inf.  One
 * current hit is kept; a candidate with c_t <= cur.end overlaps it and replaces it only if z_t > cur.score; a candidate that does
 * not overlap flushes the current hit to the output and becomes the current hit; the last one is flushed behind the last frame.
 *   hit_score_dev (m, max_hits) fp64, hit_begin_dev / hit_end_dev (m, max_hits) int32: the hits in time order, end inclusive; NaN and
 *                 -1 behind the stored ones.  count_dev (m): the TRUE number of hits, which may exceed max_hits.
 *   trace_score_dev fp64 / trace_begin_dev int32: both NULL, or both given with trace0_host (m): z_t and c_t of every frame of pair j
 *                 at entries [trace0_host[j], + frames), -1: no trace for this pair.
 * Per pair, the others unaffected: a recording with a NaN logit, a +inf logit or a frame whose max is -inf, or a label outside
 * [0, V) or equal to the blank, gives count -1, empty slots and an empty trace (NaN, -1).  -inf logits are otherwise legal; fewer
 * frames than labels simply yields no hit.  Every step is one fp64 compare-select or add in a fixed order and there is no multiply:
 * the results do not depend on the other pairs, their order or repetition.  No atomics.
 * W2V2_EINVAL before anything is launched: a null pointer, n, m or max_hits < 1, V < 2, frames_i < 1, a negative offset, utt_of_j
 * outside [0, n), nlabels_j outside [1, W2V2_SPOT_MAX_LABELS], blank outside [0, V), delim neither -1 nor a label other than the
 * blank, a NaN min_score, only one trace pointer (or trace pointers without trace0_host).  Scratch is the library's grow-only
 * scratch; synchronises with the previous call's table upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_SPOT_MAX_LABELS 256
int w2v2_ctc_spot(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host, int32_t m,
                  const int32_t* utt_of_host, const int32_t* labels_dev, const int64_t* label0_host, const int32_t* nlabels_host,
                  int32_t blank, int32_t delim, const double* min_score_host, int32_t max_hits, double* hit_score_dev,
                  int32_t* hit_begin_dev, int32_t* hit_end_dev, int32_t* count_dev, double* trace_score_dev, int32_t* trace_begin_dev,
                  const int64_t* trace0_host, void* stream);

/* CTC prefix beam search (exact definition in csrc/beam.hip): the nbest most probable transcripts of each utterance,
 * optionally fused with a character n-gram language model.  Model-free, like w2v2_ctc_align, and with the same addressing:
 *   utterance i: logits_dev rows [row0_host[i], row0_host[i] + frames_host[i]) of V fp32
 *   lm_table_dev  NULL (every table value 0), or (V^(lm_order - 1), V) fp32 log-probabilities: row = the last lm_order - 1 labels of
 *                 the prefix as digits base V, oldest first, missing history filled with the blank; a new label c adds
 *                 lm_alpha * table[row][c] + lm_beta to the hypothesis' LM score.  The table must be finite (not checked here).
 *   labels_out_dev (n, nbest, max_len) int32, -1 behind each hypothesis; length_dev (n, nbest), -1 where the utterance has fewer
 *                 hypotheses; score_dev (n, nbest) fp64: the CTC log-probability of the transcript summed over the frame paths whose
 *                 prefixes stayed in the beam at every step -- a LOWER bound of the exact value, equal to it when nothing was
 *                 pruned; total_dev = score + LM score, the ranking key; hypotheses in descending total.
 * 1 <= beam_width <= W2V2_BEAM_MAX_WIDTH, 1 <= nbest <= beam_width, 1 <= V <= W2V2_BEAM_MAX_VOCAB, blank in [0, V), lm_order 1..4,
 * finite lm_alpha / lm_beta, frames_i >= 1, max_len >= max_i frames_i: otherwise W2V2_EINVAL.  An utterance with a NaN or +inf logit
 * (or a frame of -inf only) has no hypothesis (every length -1, score = total = NaN); -inf logits are legal; neighbours are
 * unaffected.  Results do not depend on the other utterances of the call, their order, or repetition.  Synchronises with the
 * previous call's table upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_BEAM_MAX_WIDTH 64
#define W2V2_BEAM_MAX_VOCAB 64
int w2v2_ctc_beam_search(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                         int32_t blank, int32_t beam_width, int32_t nbest, const float* lm_table_dev, int32_t lm_order,
                         float lm_alpha, float lm_beta, int32_t max_len, int32_t* labels_out_dev, int32_t* length_dev,
                         double* score_dev, double* total_dev, void* stream);

/* The same search with a WORD n-gram language model and a lexicon in place of the character table (exact definition
 * in csrc/beam.hip).  Label `delim` is the word delimiter: a prefix is split into words at it.  The lexicon is a trie over labels
 * (node 0 the root); the model is a backoff n-gram compiled into states (one per context, state 0 the empty context) with sorted
 * arcs.  Everything is built on the host (wav2vec2.decoding.WordNgramLM compiles an ARPA model) and lives on the device:
 *   child_dev     (n_nodes, V) int32: the child of a node by a label, -1 none;  word_at_dev (n_nodes): the word a node spells, -1 none
 *   arc0_dev      (n_states + 1): the arcs of state s are arc0[s] .. arc0[s + 1], sorted by word; state 0 holds the n_words words
 *                 0 .. n_words - 1 in order;  arc_word_dev / arc_logp_dev / arc_next_dev (n_arcs): word, ln P(word | context) fp32,
 *                 the state after it (the longest suffix of context + word that is a state)
 *   bo_dev        (n_states) fp32 ln backoff weight;  bstate_dev (n_states): the context without its oldest word
 *   start_state   the context <s> (or 0);  unk: the word scored for a string outside the lexicon;  eos: </s> or -1
 * A word w that ends in state s adds lm_alpha * lookup(s, w) + lm_beta to the hypothesis' LM score, lookup walking the backoff
 * chain (miss: add bo[s], go to bstate[s]).  unk_penalty <= 0 is added to ln P(unk | .) for a string that is no word; -INFINITY
 * is the CONSTRAINED mode: a hypothesis may not leave the lexicon (such candidates are dropped).  After the last frame the open
 * word is ended, lm_alpha * ln P(eos | .) is added where score_eos != 0 and eos >= 0, and the entries of the final beam are
 * re-ordered by that total; an entry whose open word is dropped is removed, so an utterance can have no hypothesis at all.
 * Outputs, addressing, limits and the treatment of bad logits are w2v2_ctc_beam_search's.  W2V2_EINVAL with a message: a null
 * pointer, delim outside [0, V) or equal to the blank, a size <= 0, order outside 1..W2V2_WORDLM_MAX_ORDER, n_nodes * V >= 2^31,
 * non-finite lm_alpha / lm_beta, unk_penalty NaN or > 0, start_state / unk / eos out of range.  The CONTENTS of the arrays are
 * trusted (the Python class validates them). */
#define W2V2_WORDLM_MAX_ORDER 5
typedef struct w2v2_word_lm {
    const int32_t* child_dev;
    const int32_t* word_at_dev;
    const int32_t* arc0_dev;
    const int32_t* arc_word_dev;
    const float* arc_logp_dev;
    const int32_t* arc_next_dev;
    const float* bo_dev;
    const int32_t* bstate_dev;
    int32_t n_nodes, n_states, n_arcs, n_words;
    int32_t order, start_state, unk, eos;
} w2v2_word_lm;
int w2v2_ctc_beam_search_words(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                               int32_t blank, int32_t beam_width, int32_t nbest, const w2v2_word_lm* lm, int32_t delim,
                               float lm_alpha, float lm_beta, float unk_penalty, int32_t score_eos, int32_t max_len,
                               int32_t* labels_out_dev, int32_t* length_dev, double* score_dev, double* total_dev, void* stream);

/* Either search with a PHRASE BIAS (contextual biasing, "hotwords"; DESIGN.md §20, exact definition in csrc/beam.hip): hypotheses that
 * spell given phrases are preferred while the search runs.  The bias is an Aho-Corasick automaton over labels with its failure links
 * resolved, compiled on the host (wav2vec2.decoding.ContextBias) into dense device tables:
 *   next_dev      (n_states, V) int32: the state after a label (the longest suffix of the prefix that begins a phrase); state 0 the root
 *   delta_dev     (n_states, V) fp32: what that label adds to the hypothesis' LM score: the boosts of the phrases it completes plus the
 *                 change of the partial credit of the phrase under way
 *   final_dev     (n_states) fp32: added after the last frame (partial credit of an unfinished phrase is given back)
 *   start_state   the state of the empty prefix
 * The blank's column is never read.  Every entry of the beam carries its state; a new label c from state s adds (double)delta[s][c]
 * after the language model's own term and moves to next[s][c]; after the last frame (and, in the word form, after the open word and
 * eos) (double)final[s] is added and the final beam is re-ordered by descending total, equal totals by beam rank.
 * The language model is the character table (lm_table_dev, lm_order; NULL: none) when word_lm == NULL, else the word model (delim,
 * unk_penalty, score_eos as in w2v2_ctc_beam_search_words; delim is ignored without a word model).  `bias` is required: the calls
 * without one are the two entries above.  W2V2_EINVAL with a message, before anything is launched: a null bias or a null array in
 * it, n_states outside [1, W2V2_BIAS_MAX_STATES], start_state outside [0, n_states), n_states * V >= 2^31, word_lm and lm_table_dev
 * both given, and every check of the entry of the chosen form.  The CONTENTS of the tables are trusted (the Python class validates
 * them).  Outputs, addressing, limits, scratch and the treatment of bad logits are w2v2_ctc_beam_search's. */
#define W2V2_BIAS_MAX_STATES (1 << 20)
typedef struct w2v2_ctc_bias {
    const int32_t* next_dev;
    const float* delta_dev;
    const float* final_dev;
    int32_t n_states, start_state;
} w2v2_ctc_bias;
int w2v2_ctc_beam_search_biased(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                                int32_t blank, int32_t beam_width, int32_t nbest, const float* lm_table_dev, int32_t lm_order,
                                const w2v2_word_lm* word_lm, int32_t delim, float lm_alpha, float lm_beta, float unk_penalty,
                                int32_t score_eos, const w2v2_ctc_bias* bias, int32_t max_len, int32_t* labels_out_dev,
                                int32_t* length_dev, double* score_dev, double* total_dev, void* stream);

/* The same search, RESUMABLE (streaming; DESIGN.md §25, exact definition in csrc/beam.hip): any of the four forms above -- no model or
 * a character table (lm_table_dev, lm_order), or a word model (word_lm; lm_table_dev then NULL), each with or without a phrase bias
 * (`bias` may be NULL) -- over frames that arrive in pieces.  Stream i has searched frames_done_host[i] frames in earlier calls; this
 * call searches the frames_host[i] >= 0 rows from row0_host[i] on as the frames behind them and leaves the stream ready for the next
 * call.  Cutting T frames into calls in any way -- calls of zero frames included -- gives the bits of one call of T frames, and one call
 * from frames_done = 0 gives the bits of the entry of that form above.
 *   state_dev     n slabs of w2v2_ctc_beam_stream_state_bytes() bytes, slab i stream i's: the beam between two calls, written by every
 *                 call, read when frames_done_i > 0 (a call with frames_done_i == 0 starts the stream and needs no initialised slab)
 *   nodes_dev     the prefix tries: stream i owns entries [node0_host[i], node0_host[i] + node_cap_host[i]) and needs
 *                 (frames_done_i + frames_i) * beam_width + 1 of them after this call; the entries written by earlier calls must still be
 *                 there (a caller that moves a stream to a larger buffer copies them)
 *   labels_out_dev (n, nbest, max_len) or NULL.  Given: the hypotheses of everything searched so far, as the entries above would return
 *                 them had the utterance ended here (open word ended, eos, end-of-utterance bias term), with length_dev, score_dev and
 *                 total_dev; returning them does not disturb the state.  NULL: the call only advances the state (length_dev, score_dev
 *                 and total_dev are not written and may be NULL).
 *   stable_len_dev (n) int32, always written: the number of leading labels that all entries of stream i's beam share after this call.
 *                 Every hypothesis any later call returns for the stream begins with those labels, and the number never decreases.
 * A stream that meets a frame with a non-finite log-sum-exp (a NaN or +inf logit, a frame of -inf only) is DEAD from that call on:
 * the call and every later one advance nothing and report no hypothesis (length -1, score = total = NaN), stable_len keeps its value;
 * the other streams of the call are unaffected.  Starting again with frames_done_i == 0 revives it.
 * W2V2_EINVAL with a message, before anything is launched: every check of the entry of the chosen form (frames_i == 0 is legal here),
 * frames_i < 0, frames_done_i < 0, node0_i < 0, (frames_done_i + frames_i) * beam_width + 1 > node_cap_i,
 * (frames_done_i + frames_i) * beam_width >= 2^31 - 1, and, with labels_out_dev, max_len < frames_done_i + frames_i.  The CONTENTS of
 * the slabs, and that V, blank, beam_width, the model and the bias are the same in all calls of a stream, are trusted
 * (wav2vec2.decoding.BeamStream guards them).  Enqueued on `stream` like the entries above; calls of one stream must be ordered. */
int64_t w2v2_ctc_beam_stream_state_bytes(void);   /* per stream, one size for all four forms, a multiple of 256 */
int w2v2_ctc_beam_search_stream(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                                const int64_t* frames_done_host, int32_t blank, int32_t beam_width, int32_t nbest,
                                const float* lm_table_dev, int32_t lm_order, const w2v2_word_lm* word_lm, int32_t delim,
                                float lm_alpha, float lm_beta, float unk_penalty, int32_t score_eos, const w2v2_ctc_bias* bias /* may be NULL */,
                                void* state_dev /* n slabs */, uint64_t* nodes_dev, const int64_t* node0_host, const int64_t* node_cap_host,
                                int32_t max_len, int32_t* labels_out_dev /* may be NULL */, int32_t* length_dev, double* score_dev,
                                double* total_dev, int32_t* stable_len_dev, void* stream);

/* Pause cuts (exact definition in csrc/segment.hip and, in numpy, tests/longform_reference.py): where the logits
 * of a long recording can be cut into utterance-sized pieces for w2v2_ctc_beam_search and w2v2_ctc_align.  Model-free, with their
 * addressing:  utterance i: logits_dev rows [row0_host[i], row0_host[i] + frames_host[i]) of V fp32.
 * With a_t the argmax of row t (lowest index on ties; -1 for a row that holds a NaN), frame t is QUIET when a_t == blank and
 * x_t[blank] - max_{v != blank} x_t[v] >= margin (one fp32 subtraction; V == 1: quiet).  A pause is a maximal run [a, b) of quiet
 * frames with b - a >= min_pause, a > 0 and b < frames_i; with delim >= 0 it counts only if the last frame before a whose a_t is not
 * the blank exists and has a_t == delim (the cut then falls between words of the greedy path); delim = -1 drops that condition.
 * The cut of a pause is a + (b - a) / 2.
 *   cut_dev, pause_dev  (n, max_cuts) int32: the cuts in ascending order and their pauses' lengths b - a; -1 behind the last
 *   count_dev           (n) int32: the TRUE count, which may exceed max_cuts; only the first max_cuts are stored
 * n >= 1, V >= 1, blank in [0, V), delim -1 or a label in [0, V) other than the blank, margin not NaN, min_pause >= 1,
 * max_cuts >= 1, 1 <= frames_i <= W2V2_CUTS_MAX_FRAMES, row0_i >= 0: otherwise W2V2_EINVAL.  One utterance is spread over blocks of
 * W2V2_CUTS_CHUNK frames; what crosses a block's edge (the running count of quiet frames, the last label that is not the blank) is
 * carried by a scan, and the cuts are compacted in order by a prefix sum: no atomics, the same bits on every call, and results do
 * not depend on the other utterances of the call.  Launches are attributed to the `ctc` profiling family.  Synchronises with the
 * previous call's table upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_CUTS_CHUNK 1024
#define W2V2_CUTS_MAX_FRAMES (1 << 24)
int w2v2_ctc_pause_cuts(const float* logits_dev, int32_t V, int32_t n, const int64_t* row0_host, const int32_t* frames_host,
                        int32_t blank, int32_t delim, float margin, int32_t min_pause, int32_t max_cuts, int32_t* cut_dev,
                        int32_t* pause_dev, int32_t* count_dev, void* stream);

/* Edit distance with its breakdown (exact definition in csrc/edit.hip and, in plain Python,
 * tests/edit_reference.py): what a word or character error rate is made of.  Model-free: many pairs per call, addressed by host
 * tables into ONE token buffer, each pair computed as if it were alone.
 *   pair p: the hypothesis tokens_dev[hyp0_host[p] .. + hyp_len_host[p]) (length m) against the reference
 *           tokens_dev[ref0_host[p] .. + ref_len_host[p]) (length n), int32 tokens compared for equality only.  Ranges may
 *           overlap and may be shared by any number of pairs.
 *   out_dev (n_pairs, 4) int32: distance, substitutions, deletions, insertions.
 * distance is the least number of substitutions, deletions (a reference token without a counterpart) and insertions (a
 * hypothesis token without one) that turn the reference into the hypothesis.  The counts are those of the alignment of that
 * distance with the FEWEST substitutions -- which is also the one with the most hits (hits = n - substitutions - deletions) --
 * and are unique: with (C, S) the lexicographic minimum of (cost, substitutions) over all alignments, deletions =
 * (C - S - (m - n)) / 2 and insertions = deletions + m - n.  No tie-break rule enters the result, so the split can differ from a
 * tool that backtraces with a fixed priority (`ab` against `ba`: one deletion, one insertion and a hit here, two substitutions
 * there); the distance, and with it any error rate, cannot.  Lengths of 0 are legal: an empty hypothesis gives n deletions, an
 * empty reference m insertions.
 * W2V2_EINVAL with a message: a null pointer, n_pairs < 1, a negative offset or length, a range past n_tokens, a length above
 * W2V2_EDIT_MAX_LEN (a cell packs cost and substitutions into 16 bits each).  Device memory is O(n) per pair in flight, never
 * O(m n); no atomics, the same bits on every call, and a pair's result does not depend on the other pairs of the call, their
 * order, or repetition.  At most two launches per call, attributed to the `ctc` profiling family.  Synchronises with the previous
 * call's table upload (host-side), otherwise enqueued on `stream`. */
#define W2V2_EDIT_MAX_LEN 65535
int w2v2_edit_distance(const int32_t* tokens_dev, int64_t n_tokens, int32_t n_pairs, const int64_t* hyp0_host,
                       const int32_t* hyp_len_host, const int64_t* ref0_host, const int32_t* ref_len_host, int32_t* out_dev,
                       void* stream);

/* Resampling (the same definition in fp64 numpy: tests/resample_reference.py): a polyphase Kaiser-windowed-sinc
 * filter with a rational ratio.  Model-free: many segments per call, addressed by host tables, each computed as if it were alone.
 *
 * Design (host only, no device needed).  g = gcd(rate_in, rate_out), M = rate_in / g, L = rate_out / g; fc = min(L, M) rolloff / M,
 * width = ceil(zeros / fc), K = 2 width, lead = width - 1.  For phase r in [0, L) and tap t in [0, K): u = (t - lead) - r / L,
 * s = u fc, table[r][t] = fc sinc(s) I0(beta sqrt(1 - (s / zeros)^2)) / I0(beta) where |s| < zeros and 0 elsewhere, formed in fp64
 * and rounded once to fp32.  L == M: K = 1, lead = 0, table = [[1.0]].  The sizes are always written; the (L, K) row-major table
 * when table != NULL, and then table_capacity (in floats) below L K is W2V2_EINVAL.  W2V2_EINVAL also for a rate or zeros < 1,
 * rolloff outside (0, 1], beta negative or not finite, or a K beyond 2^31.
 *
 * Application.  Segment i is in_dev[in0_host[i] .. + in_len_host[i]), zero outside, with filter f = filter_of_host[i] (NULL: filter
 * 0 for all); it writes out_dev[out0_host[i] .. + w2v2_resample_length(in_len_host[i], L_f, M_f)).  For output n, with 64-bit
 * integers q = floor(n M / L), r = (n M) mod L:
 *     out[n] = sum_{t < K} table[r][t] x[q - lead + t]
 * as ONE fp32 chain in ascending t over all K taps, zero pads included: the product of tap 0, then one fmaf per tap.  The bits of
 * out[n] therefore depend on the segment's own samples, the table and n alone -- not on the other segments, on where the segment
 * lies in the buffers, or on the tiling -- and the copy filter returns the input's bits.  table_dev is (L, K) fp32, row-major, and
 * is not interpreted.  A block computes W2V2_RESAMPLE_TILE consecutive outputs of one segment (fewer where their input span would
 * not fit the LDS).
 * W2V2_EINVAL with a message: a null pointer, n < 1, n_filters < 1, in_len outside [1, 2^31), a negative in0 / out0, filter_of out of
 * range, a filter with L < 1, M < 1, K < 1, lead outside [0, K), L > W2V2_RESAMPLE_MAX_L or L K > W2V2_RESAMPLE_MAX_TABLE, more
 * than 2^31 - 1 tiles in all.  Output ranges that overlap each other or the input are the caller's error and are not detected.
 * Launches are attributed to the `misc` profiling family.  Synchronises with the previous call's table upload (host-side),
 * otherwise enqueued on `stream`. */
#define W2V2_RESAMPLE_TILE 2048
#define W2V2_RESAMPLE_MAX_L 4096
#define W2V2_RESAMPLE_MAX_TABLE (1 << 22)
int w2v2_resample_design(int32_t rate_in, int32_t rate_out, int32_t zeros, double rolloff, double beta, int32_t* L, int32_t* M,
                         int32_t* K, int32_t* lead, float* table, int64_t table_capacity);
int64_t w2v2_resample_length(int64_t len, int32_t L, int32_t M);      /* ceil(len L / M); -1 for len < 0, L < 1 or M < 1 */
typedef struct w2v2_resample_filter {
    const float* table_dev;
    int32_t L, M, K, lead;
} w2v2_resample_filter;
int w2v2_resample(const float* in_dev, int32_t n, const int64_t* in0_host, const int64_t* in_len_host, const int32_t* filter_of_host,
                  const w2v2_resample_filter* filters, int32_t n_filters, float* out_dev, const int64_t* out0_host, void* stream);

/* Waveform augmentation for fine-tuning (the same definitions in numpy: tests/augment_reference.py): reverberation
 * and additive noise.  Model-free like w2v2_resample: many segments per call, addressed by host tables, each computed as if it were
 * alone; enqueued on `stream` (the host tables are uploaded as there); launches are attributed to the `misc` profiling family;
 * ranges that overlap each other or an input are the caller's error and are not detected.  Inputs are assumed finite: what a NaN or
 * Inf does within its own segment is unspecified, and it never reaches another segment.
 *
 * w2v2_fir.  Segment i is x = in_dev[in0_host[i] .. + len_host[i]), zero outside, its filter h = taps_dev[taps0_host[i] .. +
 * ntaps_host[i]), K = ntaps_host[i], d = delay_host[i] in [0, K); it writes out_dev[out0_host[i] .. + len_host[i]):
 *     y[n] = sum_{k < K} h[k] x[n + d - k]        for n in [0, len)
 * as ONE fp32 chain in ascending k from +0.0f, one fmaf per tap, zero pads included.  The bits of y[n] depend on the segment's
 * samples, its taps, d and n alone -- not on the other segments, on where the segment lies in the buffers, or on the tiling: a block
 * computes W2V2_FIR_TILE consecutive outputs counted from the segment's first sample and walks k in chunks of W2V2_FIR_CHUNK
 * (csrc/augment.hip).  With match_power != 0, Px = sum x^2 and Py = sum y^2 over the segment in fp64 (chunks of 4096 samples from the
 * segment's start; within a chunk 256 strided sums folded by a tree; the chunks folded the same way), g = (float)sqrt(Px / Py), g = 1
 * when either sum is 0, and out = g * y, one fp32 multiply per sample.  Otherwise out = y and g = 1.  gain_dev (n floats, or NULL)
 * receives g.
 *
 * w2v2_mix.  Segment i as above; v[n] = noise_dev[noise0_host[i] + (offset_host[i] + n) mod noise_len_host[i]].  Px = sum x^2 and
 * Pv = sum v^2 over the len samples read, as above; g = (float)(sqrt(Px / Pv) * scale_host[i]), g = 0 when either sum is 0;
 * out[n] = fmaf(g, v[n], x[n]), and x[n]'s own bits where g == 0.  scale = 10^(-snr_db / 20) gives that signal-to-noise ratio.
 *
 * W2V2_EINVAL with a message: a null pointer (gain_dev excepted), n < 1, a length (or noise length) outside [1, 2^31), ntaps outside
 * [1, W2V2_FIR_MAX_TAPS], a delay outside [0, ntaps), an offset outside [0, noise_len), a scale that is negative or not finite, a
 * negative in0 / taps0 / noise0 / out0. */
#define W2V2_FIR_MAX_TAPS 65536
#define W2V2_FIR_TILE 8192
#define W2V2_FIR_CHUNK 2048
int w2v2_fir(const float* in_dev, int32_t n, const int64_t* in0_host, const int64_t* len_host, const float* taps_dev,
             const int64_t* taps0_host, const int32_t* ntaps_host, const int32_t* delay_host, float* out_dev, const int64_t* out0_host,
             int32_t match_power, float* gain_dev, void* stream);
int w2v2_mix(const float* in_dev, int32_t n, const int64_t* in0_host, const int64_t* len_host, const float* noise_dev,
             const int64_t* noise0_host, const int64_t* noise_len_host, const int64_t* offset_host, const double* scale_host,
             float* out_dev, const int64_t* out0_host, float* gain_dev, void* stream);

/* ---- the training step (reference src/main.py:136-259) --------
 * Replaces what Keras' train_step does around the forward: training-mode forward, backward of every
 * trainable variable, Adam.  Postnorm (base) and prenorm (robust / xlsr) transformers; the conv feature
 * extractor has no backward (the reference freezes it, main.py:234-237) -- mark it non-trainable first.
 *
 * w2v2_train_forward: Wav2Vec2ForCTC.call(training=True): Dropout(p) at every Dropout layer
 *   (feature_extractor.py:95; encoder.py:42-44,118,128,270; modeling.py:253) with masks from a
 *   counter-based hash of (seed, site, element) -- regenerated in the backward (the bf16 attention keeps its
 *   decisions as one bit per score for its own backward); the probability is realised to 2^-16;
 *   spec_mask_host (B*T bytes, or NULL): frames replaced by masked_spec_embed (spec_augment.py:119-127;
 *   the span sampling itself is host-side numpy in the reference and stays on the host here);
 *   sd_keep_host (num_layers floats of 0/1, or NULL): StochasticDepth's one Bernoulli draw per layer
 *   call (tensorflow_addons.py:381).  Saves what the backward needs.
 * w2v2_train_backward: given d loss / d logits (B, T, V) fills the flat gradient buffer (zero for
 *   frozen variables).  w2v2_grad_buffer exposes that buffer for the data-parallel all-reduce (SUM).
 *   The precision mode and W2V2_OPT_BF16_SHADOWS must be what the forward ran with: W2V2_ESTATE otherwise.
 * w2v2_adam_step: Keras Adam, p -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps), then re-derives the
 *   tensors w2v2_finalize builds. */
int w2v2_set_trainable(w2v2_model* m, const char* name_prefix, int trainable);
/* The whole flag vector in one call: flags[i] != 0 marks variable i of the inventory (w2v2_param_info order) trainable;
 * n must equal w2v2_num_params.  This is what `model.trainable = ...` / `layer.trainable = ...` push after walking the
 * Keras-style layer tree (reference src/main.py:210,234-237 flips whole layers). */
int w2v2_set_trainable_flags(w2v2_model* m, const uint8_t* flags, int32_t n);
int w2v2_train_forward(w2v2_model* m, const float* wave_dev, int32_t B, int64_t L, const int32_t* mask_dev,
                       const uint8_t* spec_mask_host, const float* sd_keep_host, float dropout_p,
                       uint64_t seed, float* logits_dev, void* stream);
int w2v2_train_backward(w2v2_model* m, const float* grad_logits_dev, void* stream);
int w2v2_grad_buffer(w2v2_model* m, float** dev_ptr, int64_t* numel);
/* Gradient buckets for overlapping the data-parallel all-reduce with the backward (the reference leaves this to
 * tf.distribute; main.py:156,192).  Bucket k is a contiguous slice [offset, offset + numel) of the flat gradient buffer;
 * buckets are numbered in the order w2v2_train_backward completes them: 0 = lm_head, 1 .. N = encoder layers N-1 .. 0,
 * N+1 = everything in front of layer 0 (positional conv, feature projection, ...).  They tile the buffer exactly.
 * w2v2_train_bucket_wait makes `stream` wait until bucket k of the LAST enqueued backward is final -- and for nothing
 * else, so a collective enqueued behind it runs under the rest of the backward. */
int w2v2_train_num_buckets(const w2v2_model* m);
int w2v2_train_bucket(w2v2_model* m, int32_t k, int64_t* offset, int64_t* numel);
int w2v2_train_bucket_wait(w2v2_model* m, int32_t k, void* stream);
/* Slot [offset, offset + numel) of one variable in the flat gradient / Adam buffers (inventory order, 16-byte aligned slots):
 * lets the caller send only the trainable runs of a bucket (the reference's payload excludes the frozen conv stack). */
int w2v2_grad_slot(w2v2_model* m, const char* name, int64_t* offset, int64_t* numel);

/* ---- native data-parallel collective (RCCL over xGMI; gsoc-wav2vec2_amd/csrc/comm.hip) ------------------------------------------
 * The gradient SUM of the reference's MirroredStrategy step (src/main.py:148-156,192: one replica per device; :198-200: the loss is
 * divided by the GLOBAL batch, so the cross-replica SUM of the gradients is the global-mean gradient) issued by the library itself:
 * one process per GPU, one communicator per model.  RCCL is bound at run time (dlopen librccl.so.1; a copy the process already holds
 * is reused), so hosts without it only lose these entry points (W2V2_ESTATE with the reason in w2v2_last_error).
 *   w2v2_comm_unique_id    rank 0 draws the rendezvous id (W2V2_COMM_ID_BYTES bytes) and hands it to the other ranks by any channel
 *                          the host has (a file, MPI, a TCP store: bytes, not a torch type);
 *   w2v2_comm_init         every rank: ncclCommInitRank on the CURRENT device + the library's own high-priority communication stream;
 *   w2v2_allreduce_bucket  in-place SUM of gradient bucket k's TRAINABLE runs (frozen slots are zero on every rank and stay home:
 *                          90,195,104 + 768 elements = 360.8 MB for wav2vec2-base in stage 2) on the communication stream,
 *                          which first waits for that bucket's completion event of the last enqueued backward -- and for nothing
 *                          else: call it for k = 0 .. w2v2_train_num_buckets - 1 right after w2v2_train_backward and the upper layers'
 *                          collectives run under the lower layers' backward.  algo 0 = ncclAllReduce; 1 = ncclReduceScatter +
 *                          ncclAllGather over the run's world-divisible body (+ an all-reduce of the < world-element tail);
 *   w2v2_allreduce_finish  `stream` (the optimizer's) waits for everything enqueued on the communication stream; *payload_bytes
 *                          (may be NULL) = bytes reduced since the previous finish;
 *   w2v2_allreduce_num_runs / _run   the (offset, numel) runs a bucket sends (tests; equal to wav2vec2/dist.py::trainable_ranges).
 * Not thread-safe; every rank must make the same calls in the same order (RCCL's rule). */
#define W2V2_COMM_ID_BYTES 128
int w2v2_comm_unique_id(uint8_t* id_out, int32_t nbytes);
int w2v2_comm_init(w2v2_model* m, const uint8_t* unique_id, int32_t nbytes, int32_t rank, int32_t world);
int w2v2_comm_info(const w2v2_model* m, int32_t* rank, int32_t* world, int32_t* rccl_version);
int w2v2_comm_destroy(w2v2_model* m);
int w2v2_allreduce_num_runs(w2v2_model* m, int32_t k, int32_t* count);
int w2v2_allreduce_run(w2v2_model* m, int32_t k, int32_t i, int64_t* offset, int64_t* numel);
int w2v2_allreduce_bucket(w2v2_model* m, int32_t k, int32_t algo);
int w2v2_allreduce_finish(w2v2_model* m, void* stream, int64_t* payload_bytes);
/* Adam's moment buffers (device, flat, same layout as the gradient buffer): what a training checkpoint must carry besides
 * the variables and the step count (the reference's ModelCheckpoint writes a TF checkpoint, training_utils.py:38-45). */
int w2v2_adam_buffers(w2v2_model* m, float** m_dev, float** v_dev, int64_t* numel);
/* A fresh optimizer: zero both moment buffers.  The reference creates a new tf.keras.optimizers.Adam for each of its two
 * stages (src/main.py:213,240); the moments live in the model's training state here, so whoever starts a new optimizer
 * (a new Trainer, or a checkpoint without moments) calls this. */
int w2v2_adam_reset(w2v2_model* m, void* stream);
int w2v2_get_grad(w2v2_model* m, const char* name, float* host_dst, int64_t numel, void* stream);
/* Which per-layer activations the LAST training forward kept only as bf16 (precision mode BF16 on the shadow paths; their fp32 buffers
 * are then not allocated at all), and the bytes of shape-dependent training workspace currently allocated.  Introspection for the tests:
 * a step that silently fell back to the fp32 activations (twice the element-wise traffic) must not pass unnoticed.
 *   *mask: bit 0 = q|k|v, bit 1 = attention output, bit 2 = FFN hidden activation, bit 3 = FFN pre-activation u (bf16 in half a buffer),
 *          bit 4 = (prenorm) the in-layer LayerNorm outputs */
#define W2V2_TRAIN_BF16_QKV 1
#define W2V2_TRAIN_BF16_CTX 2
#define W2V2_TRAIN_BF16_FFN 4
#define W2V2_TRAIN_BF16_U 8
#define W2V2_TRAIN_BF16_LN 16   /* prenorm only: the outputs of the two LayerNorms inside a layer (they feed GEMMs only) */
int w2v2_train_storage(const w2v2_model* m, int32_t* mask, int64_t* workspace_bytes);
int w2v2_adam_step(w2v2_model* m, float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* ---- gradient accumulation, clipping by the global norm, AdamW, non-finite step skip --------------------
 * What the usual wav2vec2 CTC fine-tuning recipes put between the backward and the update, none of it in the reference's model.fit.
 * Every decision stays in device memory: the norm, the clip factor and the skip flag are written into a small record by one call and
 * read by the optimizer kernel of the next, so the step stays free of device-to-host synchronisation, capturable and bitwise
 * reproducible (fixed summation orders, no float atomics).  All calls run over the trainable variables only, in 4096-element chunks;
 * none of the buffers below exists until the first call that needs it, and w2v2_adam_step is untouched by all of this.
 *   w2v2_grad_accumulate  micro-steps: mode W2V2_ACCUM_STORE copies the gradient buffer into a second flat buffer (allocated by the first
 *                         such call), W2V2_ACCUM_ADD adds it, W2V2_ACCUM_FINISH adds the buffer INTO the gradient buffer -- a plain sum:
 *                         the loss is divided by the global batch already, so micro-steps add exactly as data-parallel ranks do.
 *                         With the native per-bucket collective (w2v2_allreduce_bucket) FINISH would race with the collectives, which
 *                         wait for the backward's bucket events only: reduce after FINISH on the same stream instead.
 *   w2v2_set_decay_flags  flags[i] != 0: variable i of the inventory takes the decoupled weight decay of w2v2_adamw_step; n must equal
 *                         w2v2_num_params (the shape of w2v2_set_trainable_flags).  Default: none.
 *   w2v2_grad_norm        the record of the current gradient (after any all-reduce, so every rank decides alike): sumsq in fp64 -- each
 *                         thread adds its squares in index order, per-chunk and final sums fold in fixed trees --, norm = sqrt(sumsq),
 *                         scale = min(1, max_norm / (norm + 1e-6)) evaluated in fp64 and rounded once (torch's clip_grad_norm_;
 *                         max_norm <= 0: no clipping, scale = 1), nonfinite = an inf / NaN element was seen (exponent-field test),
 *                         skip = skip_nonfinite && (nonfinite || norm not finite), skipped_total += skip.  With clipping on and
 *                         skip_nonfinite off a non-finite gradient gives NaN parameters, as in torch.
 *   w2v2_adamw_step       g' = g scale;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p = p (1 - lr wd) - lr_t m / (sqrt(v) + eps) with
 *                         lr_t as in w2v2_adam_step (Keras' placement of eps) and wd = weight_decay for flagged variables, 0 otherwise;
 *                         reads the record of the last w2v2_grad_norm (W2V2_ESTATE if none has run since the last backward); when skip is
 *                         set, parameters and both moments keep their bits.  `step` is the caller's count of calls, skipped ones
 *                         included: the host does not know the skip without a synchronisation, so a skipped step still advances the
 *                         bias correction.  scale == 1, wd == 0, skip == 0: bit-identical to w2v2_adam_step.  Ends with w2v2_finalize.
 *   w2v2_optimizer_stats  the one call that synchronises `stream`: norm, scale and skip of the last w2v2_grad_norm and the running count of
 *                         skipped steps since the last w2v2_adam_reset (0, 1, 0, 0 before the first w2v2_grad_norm). */
#define W2V2_ACCUM_STORE 0
#define W2V2_ACCUM_ADD 1
#define W2V2_ACCUM_FINISH 2
typedef struct w2v2_opt_stats {
    double sumsq;
    float norm;
    float scale;
    int32_t nonfinite;
    int32_t skip;
    int64_t skipped_total;
} w2v2_opt_stats;
int w2v2_grad_accumulate(w2v2_model* m, int32_t mode, void* stream);
int w2v2_set_decay_flags(w2v2_model* m, const uint8_t* flags, int32_t n);
int w2v2_grad_norm(w2v2_model* m, float max_norm, int32_t skip_nonfinite, void* stream);
int w2v2_adamw_step(w2v2_model* m, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int w2v2_optimizer_stats(w2v2_model* m, float* norm, float* scale, int32_t* skipped_last, int64_t* skipped_total, void* stream);

/* ---- introspection (parity tests, profiling) -----------------------------
 * Stage activations of the LAST forward, by name: "conv0".."conv6",
 * "projection", "encoder_in", "layer0".."layerN-1", "encoder_out".  Copies
 * device -> host after synchronising `stream`. */
int w2v2_activation_info(const w2v2_model* m, const char* name, int64_t shape[3]);
int w2v2_copy_activation(w2v2_model* m, const char* name, float* host_dst,
                         int64_t numel, void* stream);

/* Per-kernel-family timing with HIP events on the launch stream.
 * enable=1 starts recording (every launch is bracketed by an event pair);
 * w2v2_profile_read synchronises and returns, for family `index`, its name,
 * launch count, total milliseconds, algorithmic FLOPs and algorithmic bytes
 * summed over the recorded launches; w2v2_profile_reset clears the record. */
int w2v2_profile_enable(w2v2_model* m, int enable);
/* Restrict the event pairs to some families (bit i = family index i of w2v2_profile_read; 0 = all):
 * an event pair costs ~7 us of stream time, so timing ONLY the dominant family keeps the timed region
 * of a benchmark within 1 % of the un-instrumented run. */
int w2v2_profile_families(w2v2_model* m, uint32_t family_mask);
/* Sampling: only every stride-th launch of a family gets the event pair (default 1 = every launch).  With a stride coprime to
 * the number of launches per layer the samples rotate through all shapes; averages stay unbiased, the tax drops by the stride.
 * w2v2_profile_seen: how many launches of the family were issued since the last reset, sampled or not. */
int w2v2_profile_sampling(w2v2_model* m, int32_t stride);
int w2v2_profile_seen(w2v2_model* m, int index, int64_t* launches);
/* KERNEL launches enqueued for the family since the last w2v2_profile_reset, by any model of the process: an op-level call
 * counted by w2v2_profile_seen may enqueue several kernels (main + tail-tile kernels of one GEMM, partial + final reductions);
 * this is the count a rocprofv3 --kernel-trace of the same steps shows.  Counted whether or not profiling is enabled. */
int w2v2_profile_kernel_launches(w2v2_model* m, int index, int64_t* launches);
int w2v2_profile_num_families(void);
int w2v2_profile_read(w2v2_model* m, int index, const char** name, int64_t* launches,
                      double* total_ms, double* flops, double* bytes);
int w2v2_profile_reset(w2v2_model* m);

/* Shader-clock probe (measurement aid; no reference counterpart).  Enqueues on `stream` a one-wave kernel that samples the
 * shader-cycle counter and the constant-rate wall clock, spins `spin_us` microseconds of wall time (0 < spin_us <= 200000) and
 * samples both again into dev_out4 = {cycles0, wall0, cycles1, wall1} (device memory, 4 x uint64).  *wall_clock_khz receives the
 * wall counter's rate.  Shader MHz while it ran = (cycles1 - cycles0) / (wall1 - wall0) * wall_clock_khz / 1000.  Launched on
 * a side stream while a workload runs on another, it reports the clock the chip holds UNDER that workload (MI355X clocks to its
 * power budget), which bench.py prints beside the nominal-peak roofline fraction. */
int w2v2_clock_probe(void* stream, int32_t spin_us, uint64_t* dev_out4, int32_t* wall_clock_khz);

/* ---- individual operators (each is one hot-path kernel family) -----------
 * Exposed so every kernel is parity-tested on its own against the oracle. */

/* C[z] = act(A[z] @ Bm + bias) + residual[z]      (tf.keras.layers.Dense /
 * Conv1D-as-implicit-GEMM; feature_extractor.py:31-37, encoder.py:15-18,99-104)
 *   A  (M, K) row-major with leading dimension lda (elements) -- an overlapping
 *      lda < K window view is how strided Conv1D is expressed;
 *   Bm (K, N) row-major, ldb;  C (M, N), ldc;  bias (N) or NULL;
 *   residual (M, N) with ldc or NULL (added AFTER the activation);
 *   act: 0 none, 1 exact GELU, 2 tanh GELU;
 *   batch z in [0, nbatch): A += z*strideA, C/residual += z*strideC. */
int w2v2_op_gemm(const float* A_dev, int64_t lda, int64_t strideA,
                 const float* B_dev, int64_t ldb,
                 float* C_dev, int64_t ldc, int64_t strideC,
                 const float* bias_dev, const float* residual_dev,
                 int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, void* stream);
/* w2v2_op_gemm with the fp32 kernel family pinned, for bit-for-bit comparisons: variant -1 by shape (= w2v2_op_gemm),
 * 0 the double-buffered LDS-DMA kernels only, 1 the LDS-ring kernels where the shape routes to them, 2 the same with a
 * persistent grid (csrc/gemm_f32_sw.hip).  The ring kernels have an instance per epilogue form the models use (plain, bias,
 * bias + exact GELU, exact GELU, bias + residual, residual): with any other form, tanh GELU or GELU + residual among them,
 * variants 1 and 2 run the double-buffered kernels as variant 0 does (the same bits). */
int w2v2_op_gemm_variant(const float* A_dev, int64_t lda, int64_t strideA,
                         const float* B_dev, int64_t ldb,
                         float* C_dev, int64_t ldc, int64_t strideC,
                         const float* bias_dev, const float* residual_dev,
                         int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, int32_t variant, void* stream);

/* Precision of the w2v2_op_* calls issued by the calling thread from now on (per-kernel tests of the bf16
 * mode); model-level calls take the model's own setting (w2v2_set_precision) and restore this one. */
int w2v2_op_set_precision(int32_t mode);

/* Same contract, operands rounded to bf16 / fp32 accumulate (W2V2_PRECISION_BF16's GEMM). */
int w2v2_op_gemm_bf16(const float* A_dev, int64_t lda, int64_t strideA,
                      const float* B_dev, int64_t ldb,
                      float* C_dev, int64_t ldc, int64_t strideC,
                      const float* bias_dev, const float* residual_dev,
                      int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, void* stream);

/* The same contraction fed from bf16 SHADOWS, the form the model's forward and data-gradient GEMMs run in precision mode bf16:
 *   A16 (M, K) bf16 rows lda elements apart (overlapping rows = strided Conv1D, batch stride strideA), B16 = the (N, K) bf16
 *   shadow of the (K, N) kernel; C fp32 and / or C16 bf16 (either may be NULL).  Both operands stream HBM / L2 -> LDS by DMA.
 * variant: 0 = the kernel the library would pick for the shape, 1 = the 128 x 128-tile kernel (gemm_bf16.hip), 2 = the 128 x 256
 * software-pipelined kernel with two 4-wave blocks per CU (gemm_bf16_sw.hip; needs N % 256 == 0, K % 64 == 0, K >= 192).  All
 * variants produce identical bits (tests/test_ops_gpu.py). */
int w2v2_op_gemm_bf16_shadows(const uint16_t* A16_dev, int64_t lda, int64_t strideA, const uint16_t* B16_nk_dev, float* C_dev,
                              uint16_t* C16_dev, int64_t ldc, int64_t strideC, const float* bias_dev, const float* residual_dev,
                              int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, int32_t variant, void* stream);

/* C_z = act(A_z B + bias) + residual_z with fp32 operands split exactly into three bf16 terms each and six bf16 MFMA
 * products per fp32 product (W2V2_PRECISION_BF16X3's GEMM; B dense (K, N), split into planes inside the call).
 * N % 256 == 0, K % 32 == 0, lda % 4 == 0, 16-byte aligned A. */
int w2v2_op_gemm_split(const float* A_dev, int64_t lda, int64_t strideA, const float* B_dev,
                       float* C_dev, int64_t ldc, int64_t strideC,
                       const float* bias_dev, const float* residual_dev,
                       int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, void* stream);

/* The same contraction with BOTH operands pre-split into 16-bit planes, the form the model's forward GEMMs run in precision modes
 * bf16x3 and f16x2 (gemm_split_sw.hip: software-pipelined 128 x 256 tiles, operands HBM / L2 -> LDS by DMA).  fmt:
 *   W2V2_PLANES_BF16X3  three bf16 planes, x = p0 + p1 + p2 exactly; six MFMA products per fp32 product;
 *   W2V2_PLANES_F16X2   two fp16 planes of x * 2^e (activations: e = 4; a weight: e chosen from max |w|); three products.
 *   w2v2_op_split_planes   x (n fp32) -> planes, plane p at planes + p * plane_stride (what the producing kernels of the model write
 *                          next to / instead of their fp32 output);
 *   w2v2_op_split_weight   Bm (K, N) fp32 -> the kernel's weight images, plane_count * K * N 16-bit elements (done once per variable
 *                          update).  f16x2: scale_ws_dev = two device words, [0] work space, [1] receives the fp32 scale
 *                          1 / (2^e_w * 2^4) that the GEMM must be given as out_scale_dev; bf16x3: NULL;
 *   w2v2_op_gemm_split_planes   A as planes (rows lda elements apart, overlapping rows = strided Conv1D, batch stride strideA, planes
 *                          planeA elements apart), B as images; the result as fp32 C (+ residual) or -- C NULL -- as the planes of
 *                          act(A B + bias) at C16 + p * planeC for the next GEMM.  range_flag_dev (int, may be NULL): set to 1 when an
 *                          f16x2 plane output saturates fp16 (|x| >= 4094).  N % 256 == 0, K % 64 == 0, lda % 8 == 0, 16-byte aligned planes. */
#define W2V2_PLANES_BF16X3 0
#define W2V2_PLANES_F16X2 1
int w2v2_op_split_planes(const float* x_dev, uint16_t* planes_dev, int64_t plane_stride, int64_t n, int32_t fmt, int32_t* range_flag_dev,
                         void* stream);
int w2v2_op_split_weight(const float* B_dev, uint16_t* images_dev, float* scale_ws_dev, int32_t K, int32_t N, int32_t fmt, void* stream);
int w2v2_op_gemm_split_planes(int32_t fmt, const uint16_t* A16_dev, int64_t planeA, int64_t lda, int64_t strideA,
                              const uint16_t* B_images_dev, const float* out_scale_dev,
                              float* C_dev, uint16_t* C16_dev, int64_t planeC, int64_t ldc, int64_t strideC,
                              const float* bias_dev, const float* residual_dev,
                              int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act, int32_t* range_flag_dev, void* stream);

/* Self-check of the branch-free GELU forms the bf16x3 GEMM epilogues use (csrc/common.h: erf_select, tanh_select): evaluates them
 * and the device library's erff / tanhf on all 2^32 float bit patterns; mismatches_dev[0] / [1] receive the number of patterns whose
 * results differ in any bit (NaNs compare equal).  Both must be 0: the forms are drop-in for the fp32 path's GELU. */
int w2v2_op_check_select_forms(uint64_t* mismatches_dev, void* stream);

/* The same sweep for the exact GELU of the fp32 GEMM epilogue (csrc/common.h: gelu_erf_epi) and for gelu_erf_select, each against
 * 0.5 x (1 + erff(x / sqrt 2)) with the library erff: mismatches_dev[0] / [1], both must be 0 (NaNs compare equal). */
int w2v2_op_check_gelu_epilogue(uint64_t* mismatches_dev, void* stream);
/* y[i] = 0.5 x[i] (1 + erff(x[i] / sqrt 2)) through the library erff, n elements: the element-wise reference of the epilogue tests. */
int w2v2_op_gelu_reference(const float* x_dev, float* y_dev, int64_t n, void* stream);
/* Launches of the LDS-ring fp32 GEMM instances by this process so far (host memory): counts[0] 256 x 128, [1] 128 x 128, [2] 64 x 64,
 * [3] 64 x 64 quarters of a split launch.  Diagnostic only (one relaxed atomic add per launch): tests read it before and after a call
 * to see which instances the call reached. */
int w2v2_op_gemm_ring_launches(int64_t* counts);
/* Which kernels w2v2_op_gemm (variant -1) / w2v2_op_gemm_variant would launch for this problem (csrc/gemm_f32_route.h).  Host only:
 * touches no device and launches nothing.  ab_aligned: A and B are 16-byte aligned; c_aligned: C, bias and residual are.
 *   out[0] kind: 0 one launch, 1 split-K (out[3] slabs on out[1], then the fold), 2 split of the 128 x 128 tile order at out[4] tiles
 *          (out[1], then out[2] as quarters), 3 split at row out[5] (out[1], then out[2]);
 *   out[1], out[2] kernels (out[2] = 0: none): 1 ring 256 x 128, 2 ring 128 x 128, 3 ring 64 x 64, 4 ring 64 x 64 quarters (the four
 *          counters of w2v2_op_gemm_ring_launches, in order), 5 double buffer 256 x 128 x 16, 6 double buffer 128 x 128 x 32,
 *          7 double buffer 64 x 64 x 32, 8 register-staged 128 x 128 (shapes without 16-byte accesses);
 *   out[6] the ring kernels run a persistent grid; out[7] kernel launches in all. */
int w2v2_op_gemm_f32_route(int32_t M, int32_t N, int32_t K, int32_t nbatch, int64_t lda, int64_t ldb, int64_t ldc, int64_t strideA,
                           int64_t strideB, int32_t act, int32_t has_bias, int32_t has_residual, int32_t ab_aligned, int32_t c_aligned,
                           int32_t variant, int32_t* out);
/* Which kernel a bf16 GEMM call (w2v2_op_gemm_bf16, _shadows, _at, w2v2_op_weight_grad_bf16, and every bf16 GEMM of the models) would
 * launch (csrc/gemm_bf16_route.h).  Host only: touches no device and launches nothing.  problem[24], in order: M, N, K, nbatch, lda,
 * ldb, strideA, strideB, ldb16 (0 = K); the operands fp32 A, fp32 B, A16, B16, B16p (0 absent, 1 present, 2 present and 16-byte
 * aligned); C, C16 asked for (0 / 1); then of GemmShadows transA, zmod, colsum given, overlapA, validK, kextra, b_zero_row,
 * force_kernel.
 *   out[0] kernel (0 when refused): 1 fp32 guarded loads, 2 fp32 16-byte loads, 3 A from its shadow, 4 B from its shadow, 5 LDS-DMA
 *          128 x 128, 6 LDS-DMA 128 x 64, 7 transposed fp32 128 x 128, 8 transposed fp32 128 x 64, 9 transposing-read 128 x 128,
 *          10 software-pipelined 128 x 256, 11 its weight-gradient form;
 *   out[1] rows in the ragged last K tile of kernel 11 (0 = whole); out[2] != 0: the call is refused (the reason, by
 *          GemmBf16Refusal); out[3], out[4] bytes per element read of A and B. */
int w2v2_op_gemm_bf16_route(const int64_t* problem, int32_t* out);
/* Launches by this process so far per kernel of that list (host memory): counts[12], counts[k] for kernel k, counts[0] unused.
 * Diagnostic only (one relaxed atomic add per launch), the twin of w2v2_op_gemm_ring_launches. */
int w2v2_op_gemm_bf16_launches(int64_t* counts);
/* Which kernel an attention call (w2v2_op_attention, _packed, _packed_bf16, _train, _bwd, and the attention of every model forward
 * and training step) would launch (csrc/attention_route.h).  Host only: touches no device and launches nothing.  problem[12], in
 * order: pass (0 inference forward, 1 training forward, 2 backward), precision (W2V2_PRECISION_*), B, T, H, heads, packed,
 * split_allowed (1 outside the tools-only build), io_aligned (q | k | v and ctx on 16-byte boundaries), then the output forms wanted:
 * fp32, bf16 shadow, planes.
 *   out[0] kernel (0 when refused): 1-3 fp32 head size 32 with 4 / 8 / 12 waves, 4-6 head size 64, 7-8 head size 128 with 4 / 8,
 *          9-11 fp32 packed head size 32 / 64 / 128, 12 fp32 training head size 32, 13-14 head size 64 with 4 / 12 waves, 15-16 fp32
 *          backward head size 32 / 64, 17-18 split bf16x3 / f16x2, 19-20 their packed forms, 21 bf16, 22 bf16 packed, 23 bf16
 *          training, 24 bf16 backward;
 *   out[1] != 0: the call is refused (1 head size, 2 a bf16 shadow wanted outside the bf16 family, 3 planes wanted outside the split
 *          family); out[2] family (1 fp32, 2 split, 3 bf16); out[3] plane format of the split family (0 bf16x3, 1 f16x2, else -1);
 *   out[4] head size; out[5] waves per block; out[6] queries per block (the height of a packed tile); out[7] the training forward
 *          saves the base-2 lse; out[8], out[9] the family can write a bf16 shadow / planes. */
int w2v2_op_attention_route(const int32_t* problem, int32_t* out);
/* Launches by this process so far per kernel of that list (host memory): counts[25], counts[k] for kernel k, counts[0] unused.  One
 * count per call of a pass (the backward's three kernels count once).  Diagnostic only, as w2v2_op_gemm_bf16_launches. */
int w2v2_op_attention_launches(int64_t* counts);
/* How the training step would compute a weight gradient dW (Kin, Nout) = A^T dY over M rows and the bias gradient db (csrc/
 * weight_grad_plan.h).  Host only: touches no device and launches nothing.  problem[17], in order: M, Kin, Nout, precision
 * (W2V2_PRECISION_*), the operands present (0 / 1) fp32 A, fp32 dY, A16, dY16, row M of dY16 is all-zero, dW wanted, db wanted, the fold
 * unpacks q|k|v, floats of the shared slab scratch, of the site's own (0 = none), of the column-sum scratch, then W2V2_DW_BLOCKS and
 * W2V2_DW_UNEVEN (512 and 1 outside the tools-only build).
 *   out[0] != 0: refused (1 the fp32 operands are needed, 2 slab scratch too small, 3 the bias gradient needs the fp32 dY);
 *   out[1] form: 0 bias only, 1 uneven slabs on the 128 x 256 transposed kernel, 2 ragged rows on the 128 x 128 transposing-read kernel,
 *          3 divisor rule from both shadows, 4 divisor rule from fp32 operands transposed in registers, 5 divisor rule through a
 *          transposed copy on the fp32 GEMM;
 *   out[2] kernel of the slab GEMM, as w2v2_op_gemm_bf16_route numbers them (0: the fp32 GEMM, or no slab GEMM);
 *   out[3] K granularity; out[4] most slabs allowed; out[5] S slabs of out[6] rows; out[7] kextra, out[8] validK, out[9] b_zero_row
 *          (GemmShadows); out[10] rows on the slab kernel, out[11] leftover rows; out[12] their kernel (0 none, 1 the shadow tail,
 *          2 transposed copy); out[13] slabs in all; out[14] the GEMMs write 1 dW, 2 slabs; out[15] a fold runs;
 *   out[16] db: 0 none, 1 column sums fused into the GEMM, 2 a column-sum pass; out[17] slabs a site's scratch is sized for. */
int w2v2_op_weight_grad_plan(const int64_t* problem, int64_t* out);
/* Plans and runs that weight gradient on the caller's operands and scratch: dW (Kin, Nout) and db (Nout), either may be NULL.  The
 * problem's operand flags must agree with the pointers, its precision with w2v2_op_set_precision, and it must not ask for the
 * unpacking fold.  slabs: the scratch the problem sized (the site's when that is non-zero); at: at_floats >= Kin M floats where the
 * plan takes a transposed copy; cs_ws: the problem's column-sum scratch; red_ws: red_ws_floats >= ceil(M / 128) Nout + 8 floats cover
 * every column-sum pass.  With dy16_zero_row set, dy16 has M + 1 rows and row M holds zeros. */
int w2v2_op_weight_grad(const int64_t* problem, const float* A_dev, const float* dY_dev, const uint16_t* A16_dev, const uint16_t* dY16_dev,
                        float* dW_dev, float* db_dev, float* slabs_dev, float* at_dev, int64_t at_floats, float* cs_ws_dev, float* red_ws_dev,
                        int64_t red_ws_floats, void* stream);

/* The weight-gradient form of the same GEMM: C_z (M, N) = A_z^T B_z with A given TRANSPOSED, (K, M) fp32 row-major with
 * row stride lda (>= M), and per-batch strides on A, B and C (split-K: batch z covers rows [z K, (z+1) K) of both
 * operands and writes slab z).  bf16-rounded operands, fp32 accumulation.  K % 64 == 0, M % 4 == 0, N % 4 == 0. */
int w2v2_op_gemm_bf16_at(const float* At_dev, int64_t lda, int64_t strideA,
                         const float* B_dev, int64_t ldb, int64_t strideB,
                         float* C_dev, int64_t ldc, int64_t strideC,
                         int32_t M, int32_t N, int32_t K, int32_t nbatch, void* stream);

/* The same weight gradient from bf16 copies of both operands in their natural layouts: slab z (Kin, Nout) = X_z^T dY_z over rows
 * [z rows_per_slab, (z + 1) rows_per_slab) of x16 (rows, Kin) and dy16 (rows, Nout), uint16 bf16 bit patterns, row-major.  `rows`
 * need not fill the last slab (nor be a multiple of the 64-row K tile): rows past it count as zero, every slab must own at least
 * one row.  Kin % 128 == 0, Nout % 128 == 0, rows_per_slab % 64 == 0, 16-byte aligned operands.  (The fine-tune step's dW GEMMs
 * in W2V2_PRECISION_BF16: tf.GradientTape's kernel gradient of Dense, src/main.py:198.)
 * variant: 0 = the kernel the library would pick, 1 = the 128 x 128-tile transposing-read kernel, 2 = the 128 x 256 software-pipelined
 * kernel in its transposed form (whole 64-row K tiles, Nout % 256 == 0, >= 192 rows per slab); identical bits.  Variant 2 also takes
 * UNEVEN slabs, the form the training step uses to cut B T rows into any number of slabs: rows = rows_per_slab nslabs + 64 e with
 * 0 < e < nslabs gives each of the first e slabs 64 rows more, slab z then starting at row z rows_per_slab + 64 min(z, e).
 * Variant 3 = variant 2 plus the caller's promise that dy16 has one more row, index `rows`, holding zeros: `rows` may then end
 * inside the last K tile (its missing rows are read from that zero row and from x16's last row) -- what the training step does
 * with its own dY shadows at B T = 23984 (480000-sample utterances). */
int w2v2_op_weight_grad_bf16(const uint16_t* x16_dev, const uint16_t* dy16_dev, float* slabs_dev,
                             int64_t rows, int32_t Kin, int32_t Nout, int32_t rows_per_slab, int32_t nslabs, int32_t variant,
                             void* stream);

/* CRC-32C (Castagnoli; TFRecord and TensorFlow-checkpoint checksums, tensorflow/core/lib/hash/crc32c.h: crc32c::Extend) of `n` host
 * bytes continuing from `crc` (0 to start).  Host-only helper for the package's checkpoint / record I/O: no device work. */
uint32_t w2v2_crc32c_extend(uint32_t crc, const void* data_host, uint64_t n);

/* y = LN(x) * gamma + beta over the last axis, optional GELU after
 * (tf.keras.layers.LayerNormalization(axis=-1); act as above). rows x C. */
int w2v2_op_layer_norm(const float* x_dev, float* y_dev, const float* gamma_dev,
                       const float* beta_dev, int64_t rows, int32_t C, float eps,
                       int32_t act, void* stream);

/* Layer 0 of the feature extractor in "group" mode: Conv1D(C_in=1, K, stride,
 * valid) -> GroupNormalization(groups=C) = per-(sample, channel) statistics
 * over time -> GELU, without materialising the un-normalised conv output
 * (feature_extractor.py:31-47,54-59; tensorflow_addons.py:207-231).
 *   wave (B, L); kernel (K, 1, C); bias (C) or NULL; out (B, T0, C);
 *   stats_ws: caller scratch of w2v2_conv0_ws_floats(B, L, K, stride, C) floats.
 * norm_mode: 0 = group-norm + activation, 1 = conv(+bias) only, 2 = conv -> LayerNormalization over the C channels of each frame
 * -> activation in one pass (the "layer" configs, feature_extractor.py:40-50): a frame's channel mean and variance follow from
 * its 10 input samples and a 10 x 10 moment matrix of the kernel, so the un-normalised conv output is never written.  Mode 2
 * needs gamma, beta and stats_ws; geometries other than K = 10, stride 5, C % 4 == 0 run mode 1 + w2v2_op_layer_norm inside.
 * act as in w2v2_op_layer_norm (modes 0 and 2). */
int64_t w2v2_conv0_ws_floats(int32_t B, int64_t L, int32_t K, int32_t stride, int32_t C);
int w2v2_op_conv0(const float* wave_dev, const float* kernel_dev, const float* bias_dev,
                  const float* gamma_dev, const float* beta_dev, float* out_dev,
                  float* stats_ws_dev, int32_t B, int64_t L, int32_t K, int32_t stride,
                  int32_t C, float eps, int32_t norm_mode, int32_t act, void* stream);

/* Effective positional kernel: l2_normalize(weight_v, axes [1,2]) * weight_g,
 * regrouped to (groups, K, C_in/groups, C_out/groups)
 * (tensorflow_addons.py:16-21; encoder.py:168-175). */
int w2v2_op_weight_norm_regroup(const float* weight_v_dev, const float* weight_g_dev,
                                float* wg_dev, int32_t K, int32_t cg, int32_t H,
                                int32_t groups, void* stream);

/* y = xz + GELU(grouped_conv_same(xz) + bias), xz = x with frames >=
 * frame_len[b] zeroed (encoder.py:253,265; PositionalConvEmbedding
 * encoder.py:177-181: pad K/2 both sides, drop the last frame for even K).
 *   x, y (B, T, H); wg from w2v2_op_weight_norm_regroup; frame_len (B) or NULL. */
int w2v2_op_pos_conv(const float* x_dev, const float* wg_dev, const float* bias_dev,
                     const int32_t* frame_len_dev, float* y_dev, int32_t B, int32_t T,
                     int32_t H, int32_t K, int32_t groups, int32_t act, void* stream);

/* Multi-head self-attention context (TransformerAttention.get_context,
 * encoder.py:34-47, with the q pre-scale of :28): per (batch, head)
 * softmax((q*scale) k^T + mask) v, mask = -10000 on keys >= frame_len[b].
 *   qkv (B, T, 3H) packed q|k|v rows;  ctx (B, T, H). Scores are never
 *   materialised. */
int w2v2_op_attention(const float* qkv_dev, const int32_t* frame_len_dev, float* ctx_dev,
                      int32_t B, int32_t T, int32_t H, int32_t num_heads, void* stream);

/* Attention of n packed utterances (the packed forward's segment kernels): utterance i owns rows
 * [cu_frames_host[i], cu_frames_host[i + 1]) of qkv (rows, 3H) and ctx (rows, H), back to back, and attends only
 * within them, unmasked -- each as w2v2_op_attention computes it alone (B = 1, T = its frames, no frame_len).
 * Dispatches on w2v2_op_set_precision: fp32 kernel in mode 0; the split kernel in modes 2 / 3 (head size 64, else the
 * fp32 kernel and a split of its output); mode 1 (bf16) gives W2V2_EINVAL (w2v2_op_attention_packed_bf16 is that mode's
 * entry).  planes_dev (optional, modes 2 / 3):
 * the planes of ctx, plane_stride elements apart (W2V2_PLANES_* of the mode); ctx_dev may then be null on the split
 * kernel.  range_flag_dev (optional): f16x2 sticky saturation flag.  Stages its tile table synchronously. */
int w2v2_op_attention_packed(const float* qkv_dev, int32_t n, const int32_t* cu_frames_host, float* ctx_dev,
                             uint16_t* planes_dev, int64_t plane_stride, int32_t* range_flag_dev,
                             int32_t H, int32_t heads, void* stream);

/* The same packed layout on the bf16 matrix pipe (head size 64): the segment form of precision mode 1's attention kernel, whatever
 * w2v2_op_set_precision says.  Each utterance's ctx (fp32) and ctx16 (its nearest-even bf16 shadow) are the bits w2v2_op_attention
 * gives it alone in mode 1.  qkv16_dev: the bf16 shadow of qkv, or NULL (qkv_dev is then rounded into scratch first); qkv_dev may be
 * NULL when the shadow is given.  ctx_dev or ctx16_dev may be NULL, not both.  Stages its tile table synchronously. */
int w2v2_op_attention_packed_bf16(const float* qkv_dev, const uint16_t* qkv16_dev, int32_t n, const int32_t* cu_frames_host,
                                  float* ctx_dev, uint16_t* ctx16_dev, int32_t H, int32_t heads, void* stream);

/* frame_len[b] = conv-stack length arithmetic applied to sum(mask[b, :])
 * (modeling.py:201-204). */
int w2v2_op_frame_lengths(const int32_t* mask_dev, int32_t* frame_len_dev, int32_t B,
                          int64_t L, const int32_t* kernal_sizes, const int32_t* strides,
                          int32_t num_layers, void* stream);

/* The normalisation of w2v2_forward_windows on its own: window i = wave_dev[sample0_host[i] .. + samples_host[i]) (samples_i >= 1),
 * normalised over its own samples, written to out_dev (sum samples_i) back to back. */
int w2v2_op_normalize_windows(const float* wave_dev, int32_t n, const int64_t* sample0_host, const int64_t* samples_host,
                              float* out_dev, void* stream);

/* ---- training operators (parity-tested on their own) ----------------------------------------- */

/* LayerNormalization backward: dx, dgamma, dbeta from x (pre-norm input), gamma and dy.
 * ws: scratch of w2v2_ln_bwd_ws_floats(rows, C) floats. */
int64_t w2v2_ln_bwd_ws_floats(int64_t rows, int32_t C);
int w2v2_op_layer_norm_bwd(const float* x_dev, const float* gamma_dev, const float* dy_dev, float* dx_dev,
                           float* dgamma_dev, float* dbeta_dev, int64_t rows, int32_t C, float eps,
                           float* ws_dev, void* stream);

/* Attention with dropout on the probabilities (encoder.py:42-44) + the saved row statistic (B, heads, T),
 * and its backward: dqkv (B, T, 3H) from dctx (B, T, H).  dvec_ws: (B, heads, T) scratch.
 * lse_dev is what the forward leaves for the backward of the SAME precision mode: the natural log-sum-exp of the (masked, scaled)
 * scores under W2V2_PRECISION_FP32; minus the log2-sum-exp2 (= -lse * log2 e, the kernels' own exponent units: P = exp2(S c + lse2)
 * is then one fused multiply-add and one v_exp_f32 per score in the backward) under W2V2_PRECISION_BF16. */
int w2v2_op_attention_train(const float* qkv_dev, const int32_t* frame_len_dev, float* ctx_dev, float* lse_dev,
                            int32_t B, int32_t T, int32_t H, int32_t num_heads, float dropout_p,
                            uint64_t seed, uint32_t stream_id, void* stream);
int w2v2_op_attention_bwd(const float* qkv_dev, const int32_t* frame_len_dev, const float* ctx_dev,
                          const float* lse_dev, const float* dctx_dev, float* dqkv_dev, float* dvec_ws_dev,
                          int32_t B, int32_t T, int32_t H, int32_t num_heads, float dropout_p,
                          uint64_t seed, uint32_t stream_id, void* stream);

/* y = dropout(act(x)) [+ residual]: keep iff (hash16(seed, stream_id, index) ^ 0x8000) >= floor(p 2^16) -- the 16-bit value read as
 * a signed number --, kept values / (1 - p)  (csrc/train.h, wav2vec2/variables.py::dropout_keep: the same integer function). */
int w2v2_op_dropout(const float* x_dev, const float* residual_dev, float* y_dev, int64_t n, int32_t act,
                    float p, uint64_t seed, uint32_t stream_id, void* stream);

/* t1 = dropout(x) + residual  and  y = LayerNorm(t1) over the last axis (C % 4 == 0), one pass over the rows: the training forward's
 * "x + drop(attn(x))" followed by the layer's next LayerNorm (encoder.py:116-124).  Bit-identical to w2v2_op_dropout (act 0) followed by
 * w2v2_op_layer_norm (act 0) on the same operands; y16_dev (optional) receives the nearest-even bf16 copy of y. */
int w2v2_op_layer_norm_dropout(const float* x_dev, const float* residual_dev, float* t1_dev, float* y_dev, uint16_t* y16_dev,
                               const float* gamma_dev, const float* beta_dev, int64_t rows, int32_t C, float eps, float p, uint64_t seed,
                               uint32_t stream_id, void* stream);

/* ---- the positional convolution's training launch paths, one entry each (PositionalConvEmbedding, encoder.py:153-181) ----
 * Layouts: x, y, pre_act, xz, dc (B, T, H); wg, wg_t, dwg (groups, K, cg, cg) with cg = H / groups, as w2v2_op_weight_norm_regroup
 * writes it; frame_len (B) or NULL.  cg is 16, 32, 48 or 64 on the fp32 entries; the bf16 entries need (K cg) % 64 == 0. */

/* y = [xz +] act(conv(xz, wg, pad_left) + bias), xz = x with frames >= frame_len[b] zeroed; output frame t reads input frames
 * t - pad_left .. t - pad_left + K - 1.  bias_dev may be NULL; pre_act_dev (optional) receives conv + bias.  pad_left = K / 2 is the
 * forward; the data gradient is the same conv of dc with the flipped kernel at pad_left = K - 1 - K / 2, no bias, no residual. */
int w2v2_op_pos_conv_ex(const float* x_dev, const float* wg_dev, const float* bias_dev, const int32_t* frame_len_dev, float* y_dev,
                        float* pre_act_dev, int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int32_t act, int32_t pad_left,
                        int32_t add_residual, void* stream);

/* The same contract on the bf16 matrix pipe (precision mode 1: x and the kernel rounded to bf16, fp32 accumulation), as one batched
 * GEMM over overlapping rows.  w16: (groups, cg, K cg) bf16 from w2v2_op_pos_conv_weight_shadow; pack16_dev: scratch of
 * w2v2_op_pos_conv_bf16_pack_elems(B, T, H, K) bf16 elements; xz_ws_dev: (B, T, H) floats, needed when frame_len and add_residual. */
int64_t w2v2_op_pos_conv_bf16_pack_elems(int32_t B, int32_t T, int32_t H, int32_t K);
int w2v2_op_pos_conv_weight_shadow(const float* wg_dev, uint16_t* w16_dev, int32_t K, int32_t cg, int32_t groups, void* stream);
int w2v2_op_pos_conv_bf16(const float* x_dev, const uint16_t* w16_dev, const float* bias_dev, const int32_t* frame_len_dev, float* y_dev,
                          float* pre_act_dev, uint16_t* pack16_dev, float* xz_ws_dev, int32_t B, int32_t T, int32_t H, int32_t K,
                          int32_t groups, int32_t act, int32_t pad_left, int32_t add_residual, void* stream);

/* The forward positional conv (pad_left = K / 2, residual on) of n packed utterances on the bf16 matrix pipe: utterance i owns rows
 * [cu_frames_host[i], cu_frames_host[i + 1]) of x and y (rows, H), back to back, and is zero-padded at its own edges -- each as
 * w2v2_op_pos_conv_bf16 computes it alone (B = 1, T = its frames, no frame_len), bit for bit.  Scratch is the library's own.
 * Stages its utterance table synchronously. */
int w2v2_op_pos_conv_packed_bf16(const float* x_dev, const uint16_t* w16_dev, const float* bias_dev, int32_t n,
                                 const int32_t* cu_frames_host, float* y_dev, int32_t H, int32_t K, int32_t groups, int32_t act,
                                 void* stream);

/* wg_t[g][K-1-k][co][ci] = wg[g][k][ci][co]: the kernel of the data-gradient pass. */
int w2v2_op_pos_conv_flip_regroup(const float* wg_dev, float* wg_t_dev, int32_t K, int32_t cg, int32_t groups, void* stream);

/* Kernel gradient dwg[g][k][ci][co] = sum over b, t of xz[b][t + k - K/2][g cg + ci] dc[b][t][g cg + co] (xz already masked), fp32. */
int w2v2_op_pos_conv_dw(const float* xz_dev, const float* dc_dev, float* dwg_dev, int32_t B, int32_t T, int32_t H, int32_t K,
                        int32_t groups, void* stream);

/* The same gradient on the bf16 pipe (xz and dc rounded to bf16): samples concatenated along the contraction in S = 1, 2 or 4
 * slabs that are summed afterwards, B <= 64.  The query fills sizes4 with the floats of pack32, slabs, red_ws and dc_pad (0: T is a
 * multiple of 64 and dc_pad may be NULL) and *slabs_S with the S the launcher will pick. */
int w2v2_pos_conv_dw_bf16_ws_floats(int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int64_t* sizes4, int32_t* slabs_S);
int w2v2_op_pos_conv_dw_bf16(const float* xz_dev, const float* dc_dev, float* dwg_dev, float* pack32_dev, float* slabs_dev,
                             float* red_ws_dev, float* dc_pad_dev, int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups,
                             void* stream);

/* Weight-norm backward, W_eff[k] = g[k] v[k] / n[k], n^2 = max(sum v[k]^2, 1e-12): dweight_g = <dW, v> / n,
 * dweight_v = (g / n)(dW - <dW, v> v / n^2).  weight_v, dweight_v (K, cg, H); weight_g, dweight_g (K); dwg as above. */
int w2v2_op_weight_norm_bwd(const float* weight_v_dev, const float* weight_g_dev, const float* dwg_dev, float* dweight_v_dev,
                            float* dweight_g_dev, int32_t K, int32_t cg, int32_t H, int32_t groups, void* stream);

/* The two kernels of w2v2_grad_norm over a raw buffer g (n floats) cut into 4096-element chunks, the last one short: *stats_out_dev
 * (device memory, zeroed first: skipped_total = skip) receives the record.  The per-chunk scratch is allocated and freed inside the
 * call, so it synchronises the device: a test entry. */
int w2v2_op_grad_norm(const float* g_dev, int64_t n, float max_norm, int32_t skip_nonfinite, w2v2_opt_stats* stats_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* W2V2_H_ */
