/* cst.h — C ABI of libcst_hip.so: the MI355X (gfx950) hot path of Chimera-ST.
 *
 * The reference (Glaciohound/Chimera-ST, a fairseq fork) has NO C ABI on this path: its seam is
 * nn.Module.forward / torch.autograd.Function calling PyTorch ATen.  Each entry
 * point below therefore replaces an ATen call site of the reference; the file:line it replaces
 * is cited per function (paths relative to the reference root).
 *
 * Conventions (SURVEY.md §8b "Native (C-ABI) layer"):
 *   - plain C: raw DEVICE pointers + explicit int64 sizes/strides (in ELEMENTS) + dtype enum +
 *     a hipStream_t passed as void*; no torch types.
 *   - ownership: every buffer (inputs, outputs, workspaces, saved-for-backward) is allocated and
 *     owned by the caller; the library never frees or retains a pointer past return.
 *   - errors: int return, 0 = ok, negative = cst_status; text via cst_last_error() (thread-local).
 *     Nothing throws across the boundary.
 *   - threading: re-entrant; no global mutable state except the optional profiling table and, per
 *     device, one 64 KiB device allocation made on the first large cst_gemm launch: the ring of
 *     work-item counters of the persistent GEMM (csrc/gemm8p.hip; each launch uses one 64-byte
 *     slot and leaves it zeroed).  It is the only memory the library owns.
 *   - all kernels are asynchronous on the given stream.
 *   - accumulation is always fp32; `dtype` is the storage type of activations/weights.
 */
#ifndef CST_H
#define CST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumps on any change of a signature or a descriptor layout (3: cst_gemm_desc.m_len, cst_attn_desc.seq_offsets, workspaces of the
 * fixed-order reductions; 4: cst_attn_desc.kpm_bits / bwd_ws, the separable attention-dropout mask; 5: cst_gemm_desc.colsum;
 * 6: cst_dec_ln_q_cross_attn; 7: cst_fbank_desc, cst_fbank, cst_fbank_workspace_bytes; 8: cst_conv0_ln_gelu_fwd / _bwd,
 * cst_ln_gelu_fwd / _bwd and their workspaces; 9: cst_beam_desc.members / logits_n / lprobs_out — checkpoint ensembles;
 * 10: cst_beam_desc.no_repeat_ngram / prefix_tokens / prefix_len — n-gram blocking and forced prefixes;
 * 11: cst_beam_desc.sampling / sample_topk / sample_topp / sample_key — sampling decode;
 * 12: cst_beam_desc.diverse_groups / diverse_strength / diverse_siblings / sibling_rate — diverse beam groups and diverse siblings;
 * 13: cst_score_tokens — scores of given target tokens, --score-reference).  cst_beam_step_lm and cst_lm_fusion_desc were ADDED at 13
 * without a bump: no existing signature or layout changed, and a library without the symbol fails at symbol lookup.  The same holds for
 * cst_lex_desc, cst_lex_workspace, cst_lex_init and cst_beam_step_lex (lexical constraints), added later at 13, and for cst_ctc_fwd,
 * cst_ctc_bwd, cst_ctc_greedy and cst_edit_distance (CTC fine-tuning), for cst_ctc_topn, cst_ctc_beam_workspace_bytes and cst_ctc_beam
 * (CTC prefix beam search), and for cst_w2v_negatives, cst_infonce_fwd, cst_infonce_bwd_x and
 * cst_infonce_bwd_y, cst_gumbel_vq_workspace, cst_gumbel_vq_fwd and cst_gumbel_vq_bwd (the head of wav2vec2 pre-training), and for the
 * host-only query cst_gemm_route.
 * cst_version() returns the value the library was built with; chimera-st_amd/lib.py refuses a mismatch. */
#define CST_ABI_VERSION 13

typedef enum { CST_F32 = 0, CST_BF16 = 1 } cst_dtype;

typedef enum {
  CST_OK = 0,
  CST_ERR_BAD_ARG = -1,     /* shape / stride / alignment / dtype not supported */
  CST_ERR_LAUNCH = -2,      /* hipLaunch / hipGetLastError failure */
  CST_ERR_WORKSPACE = -3,   /* caller workspace too small */
  CST_ERR_UNSUPPORTED = -4
} cst_status;

typedef void* cst_stream; /* hipStream_t */

const char* cst_last_error(void);
int cst_version(void);            /* ABI version, bumps on any signature change */
int cst_device_arch_ok(void);     /* 1 if the current device is gfx950, 0 otherwise */

/* ------------------------------------------------------------------------------------------
 * Profiling table (bench.py roofline leg): when enabled every launch below is bracketed with
 * hipEvents on its own stream and its algorithmic flops/bytes are recorded per kernel class.
 * ------------------------------------------------------------------------------------------ */
typedef enum {
  CST_K_GEMM = 0, CST_K_ATTN_FWD, CST_K_ATTN_BWD, CST_K_LAYERNORM, CST_K_CONV0, CST_K_ELEMENTWISE,
  CST_K_LOSS, CST_K_OPTIM, CST_K_NUM
} cst_kernel_class;
void cst_prof_enable(int on);     /* clears the table when switching on */
/* synchronises the recorded events; returns launches; outputs total ms / flops / bytes */
int64_t cst_prof_query(int kernel_class, double* total_ms, double* flops, double* bytes);
/* per-launch records of a class as text, one line per launch in launch order: "<ms> <flops> <bytes> <tag>" (tag = the launcher's
 * description: kernel family and shape).  Returns the bytes needed including the terminating 0 (call with cap = 0 to size buf). */
int64_t cst_prof_dump(int kernel_class, char* buf, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (eps, affine) — replaces torch.nn.LayerNorm at fairseq/modules/layer_norm.py:30-35
 * (apex FusedLayerNorm seam, :11-28) and Fp32LayerNorm (:38-50).
 *   s = x (+ res);  y = (s - mean) * rstd * gamma + beta
 * x,res,y,sum_out: [rows, cols] row-major contiguous; gamma/beta [cols]; mean/rstd fp32 [rows].
 * res and sum_out may be NULL.  cols % 8 == 0, cols <= 2048.
 * ------------------------------------------------------------------------------------------ */
int cst_layernorm_fwd(const void* x, const void* res, const void* gamma, const void* beta,
                      void* y, void* sum_out, float* mean, float* rstd,
                      int64_t rows, int64_t cols, float eps, int dtype, cst_stream stream);
/* dx = LN backward w.r.t. s (s = x + res is what `s` points to); dgamma/dbeta fp32 [cols]
 * (overwritten) in `grad_dtype` (CST_F32 or `dtype`: accumulated in fp32, rounded once).  dres (optional extra upstream gradient on s, e.g. the residual branch) is
 * added into dx when non-NULL.  workspace: cst_layernorm_bwd_workspace() bytes.  dgamma = dbeta = NULL (ABI 5): the second stage is
 * left to cst_reduce_multi — the row-block partials stay in `workspace` as fp32 [blocks][2][cols] (dgamma row, dbeta row per block),
 * blocks = cst_layernorm_bwd_workspace(rows, cols) / (8 * cols). */
int64_t cst_layernorm_bwd_workspace(int64_t rows, int64_t cols);
int cst_layernorm_bwd(const void* dy, const void* s, const void* gamma, const float* mean,
                      const float* rstd, const void* dres, void* dx, void* dgamma, void* dbeta,
                      void* workspace, int64_t rows, int64_t cols, int dtype, int grad_dtype, cst_stream stream);
/* the same, and additionally stamps tile_live[row / 64] = epoch for every row whose dx is not exactly zero (tile_live: uint32
 * [ceil(rows / 64)], NOT initialised by the caller: a tile is live iff its stamp equals this call's unique, non-zero epoch) —
 * the k_live / k_epoch operand of the weight-gradient GEMMs that consume dx (or a row-wise function of it) */
int cst_layernorm_bwd_tiles(const void* dy, const void* s, const void* gamma, const float* mean,
                            const float* rstd, const void* dres, void* dx, void* dgamma, void* dbeta,
                            void* workspace, int64_t rows, int64_t cols, int dtype, int grad_dtype,
                            uint32_t* tile_live, uint32_t epoch, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * GEMM on MFMA tiles — replaces F.linear / nn.Conv1d call sites:
 *   q/k/v/out projections  modules/multihead_attention.py:205-224,370
 *   fc1/fc2                modules/transformer_layer.py:144-148,404-408; models/wav2vec/wav2vec2.py:949-953
 *   conv layers 1..6       models/wav2vec/wav2vec2.py:707 (implicit GEMM on channels-last rows)
 *   pos_conv               models/wav2vec/wav2vec2.py:773-779 (grouped; segmented-K implicit GEMM)
 *   subsampler convs       models/speech_to_text/s2t_transformer.py:53-74
 *   post_extract_proj      models/wav2vec/wav2vec2.py:550-551
 *   vocab projection       models/transformer.py:830-836
 * and their autograd backward GEMMs.
 *
 *   C[M,N] = epilogue( alpha * sum_k Aop[m,k] * Bop[k,n] )
 * Operand storage ("k-major" = the reduction index is the contiguous one):
 *   a_kmajor=1: Aop[m,k] at A[m*lda + segaddr_a(k)]      a_kmajor=0: Aop[m,k] at A[k*lda + segaddr_a(m)]
 *   b_kmajor=1: Bop[k,n] at B[n*ldb + segaddr_b(k)]      b_kmajor=0: Bop[k,n] at B[k*ldb + segaddr_b(n)]
 *   segaddr(c) = (c / seg) * seg_stride + c % seg   (seg = 0 means plain c).  seg % 8 == 0.
 * lda/ldb may be SMALLER than the contiguous extent (overlapping rows = implicit-GEMM conv1d).
 * Epilogue, in order:  v = alpha*acc;  v += bias;  [aux_out = v];  v = act(v);
 *                      [v *= act'(aux_in)];  v += resid;  C = v
 * One rounding, at the store — except on the bf16 image path of the persistent kernels (gemm8p.hip's fast epilogue, gemm4w.hip: bf16
 * C, unsplit, 16-byte aligned operands, column bias only with alpha == 1), where the pre-activation v = alpha*acc + bias is rounded to
 * bf16 once (the reference's bf16 F.linear output; aux_out is that value) before act / dropout / act' / resid act on it.
 * tests/gemm_ref.py states both forms; tests/test_gemm_parity_gpu.py pins them bit for bit.
 * Batching: two batch levels (e.g. utterance x group); offsets in elements.
 * split_k > 1: partial sums go through `workspace` (cst_gemm_workspace bytes) and are reduced
 * into C by a second kernel (bias/act/resid are applied there).
 * ------------------------------------------------------------------------------------------ */
typedef enum { CST_ACT_NONE = 0, CST_ACT_RELU = 1, CST_ACT_GELU = 2 } cst_act;
typedef enum { CST_BIAS_NONE = 0, CST_BIAS_COL = 1, CST_BIAS_ROW = 2 } cst_bias_mode;

typedef struct {
  int dtype;              /* storage dtype of A, B, bias, resid, aux (cst_dtype) */
  int c_dtype;            /* storage dtype of C (cst_dtype; fp32 allowed with bf16 inputs) */
  int a_kmajor, b_kmajor;
  int64_t M, N, K;
  const void* A; int64_t lda, a_seg, a_seg_stride;
  const void* B; int64_t ldb, b_seg, b_seg_stride;
  void* C; int64_t ldc;
  const void* bias; int bias_mode;   /* dtype `dtype`; [N] or [M] */
  int64_t sbias0, sbias1;            /* batch strides of bias (0 = shared; grouped conv: per group) */
  int act;                           /* cst_act applied after bias */
  void* aux_out; int64_t ld_aux_out; /* optional pre-activation copy, dtype `dtype` */
  int dact;                          /* cst_act whose derivative (at aux_in) multiplies v */
  const void* aux_in; int64_t ld_aux_in;
  const void* resid; int64_t ld_resid;
  float alpha;
  float drop_p; uint32_t drop_key;   /* drop_p > 0: v *= keep(drop_key, row*N + col) / (1 - drop_p) after `act`, before dact /
                                        resid (FairseqDropout fused: residual + dropout(linear(x)), dropout(act(fc1 x)) and the
                                        matching mask in the dX-through-activation GEMM); needs batch0*batch1 == 1 */
  int64_t batch0, batch1;            /* >= 1 */
  int64_t sa0, sa1, sb0, sb1, sc0, sc1; /* batch strides (elements) for A, B, C(+aux/resid) */
  int split_k;                       /* 0/1 = none; >1 explicit; -1 = let the library choose */
  void* workspace; int64_t workspace_bytes;
  const uint32_t* k_live; uint32_t k_epoch; /* optional (NULL = off): one stamp per 64 consecutive k indices; a k block whose stamp
                                        != k_epoch is declared ALL-ZERO in A (every row/column of A at those k) and may be skipped —
                                        exact, 0 * b adds nothing.  Used for the weight-gradient GEMMs (k = token), whose dY rows
                                        at padded frames are exactly zero; stamps come from cst_layernorm_bwd_tiles.  Kernels
                                        that do not implement skipping ignore it. */
  const uint32_t* m_live; uint32_t m_epoch; /* optional: the same stamps on the M side — one per 64 consecutive rows of A (= rows
                                        of C); an output tile whose rows of A are all dead skips its K loop (its accumulators
                                        are exactly 0; the epilogue still runs: act', residual, stores).  Used for the dX GEMMs. */
  const int32_t* k_len;              /* optional, [batch0]: rows k >= k_len[b0] of batch b0's A are all zero (a trailing run — the
                                        frames past an utterance's end in the conv weight-gradient GEMMs); the K loop of that batch
                                        stops there and split-K divides the live range.  Exact. */
  const int32_t* m_len;              /* optional, [batch0]: rows m >= m_len[b0] of batch b0's A are all zero AND nobody reads those rows
                                        of C for their value (the frames past an utterance's end in the conv feature extractor: the
                                        reference zeroes them behind the CNN, wav2vec2.py:820-821, and their gradient is exactly zero).
                                        Output tiles that lie entirely behind m_len[b0] skip their K loop and run the epilogue on
                                        zero accumulators (C = epilogue(0): 0 for the bias-free GELU / GELU' epilogues of that stack). */
  void* colsum;                      /* optional (ABI 5), mn-major A only: colsum[batch][m] = sum_k A[k][m] in `dtype`, a by-product of staging
                                        A (the tiles of output column 0 add up the A vectors they load anyway; with split-K the slices'
                                        partial sums ride behind the slabs in the workspace and the reduce kernel adds them in split
                                        order).  With A = dY of a Linear this is the bias gradient (torch's `grad_output.sum(0)` behind
                                        F.linear, modules/multihead_attention.py / transformer_layer.py call sites): the weight-gradient
                                        GEMM dW = dY^T X reads every dY element exactly once per output tile column, so no separate
                                        column-sum pass over dY is needed.  Fixed summation order (bit-reproducible). */
  int defer_reduce;                  /* split-K launches only (ABI 5): 1 = do not launch the reduce; the fp32 slabs [split][M][N] (and the
                                        colsum slices [split][M] behind them) stay in `workspace`, which the caller keeps alive and
                                        hands to cst_reduce_multi later.  Needs a plain epilogue (alpha 1, no bias / activation /
                                        operand) and a caller-owned workspace; batched launches (slabs [batch][split][M][N], no colsum)
                                        let the caller sum over the batch in the same pass.  Ignored when the launch does
                                        not split K (cst_gemm_splits tells). */
} cst_gemm_desc;

int64_t cst_gemm_workspace(const cst_gemm_desc* d);
/* 1 if cst_gemm would produce d->colsum (non-NULL) as a by-product of this launch's own kernel, 0 if it would run the separate
 * two-launch column sum behind it (the 16-wave / DMA configurations): a caller that can get the sums cheaper elsewhere — e.g. from
 * the dropout pass that has to read dY anyway, cst_dropout_colsum — asks first. */
int cst_gemm_colsum_is_fused(const cst_gemm_desc* d);
/* The number of K slices cst_gemm will use for this descriptor (1 = no split, no workspace slabs). */
int cst_gemm_splits(const cst_gemm_desc* d);
/* Which kernel cst_gemm would launch for this descriptor, as text (host only: no HIP call, no operand is read).  Runs cst_gemm's
 * validation: a descriptor cst_gemm rejects gets the same code and cst_last_error text.  out receives one of
 *   "reg <bf16|f32> <a><b>[ seg] <BM>x<BN> nt<threads>[ colsum] split<s>"   register-staged kernel
 *   "glds <bf16|f32> <a><b> <BM>x<BN> nt<threads> ns<stages> split<s>"      DMA-ring kernel
 *   "8p <a><b>"                                                             persistent 8-wave kernel
 *   "4w"                                                                    four-wave 256 x 192 kernel
 * <a>/<b>: k or m, a k-major or mn-major operand; " seg": the segmented-K instantiation; " colsum": the column sums are the launch's own
 * by-product; <s>: K slices.  The three queries above are views of the same decision. */
int cst_gemm_route(const cst_gemm_desc* d, char* out, int64_t out_bytes);
/* Persistent GEMM launches use (CUs - n) workgroups from now on (n < 0: query only); returns the previous value.  The data-parallel
 * reducer sets it while bucket all-reduces are in flight under the backward pass, so that the RCCL kernels on the side stream find free
 * CUs instead of waiting for a launch boundary (legacy_distributed_data_parallel.py has no overlap to protect).  Initial value:
 * environment variable CST_GEMM_RESERVE_CUS (default 0). */
int cst_gemm_reserve_cus(int n);
int cst_gemm(const cst_gemm_desc* d, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * wav2vec2 positional convolution, sliding-window kernels (posconv.hip): bf16, C = 48 * groups, k <= 128 taps, pad k / 2,
 * SamePad.  x / dz / dy / y / z / dx are channels-last [B, T, C]; the results have the bits of the cst_gemm route
 * (functional._PosConvGemmFn).  m_len (int32 [B], device, or NULL): frame blocks from m_len[b] on keep zero accumulators.
 *   fwd: z = conv(x) + bias, y = x + GELU(z);              w     = [g][co][j][ci]
 *   dx : dx = dy + sum_j' dz[m - (k - 1 - k / 2) + j'] w;   wflip = [g][ci][j'][co]  (taps reversed)
 *   dw : dw [C][48][k] (the parameter's layout) and db [C] (or NULL) over all frames of the batch; k_live / k_epoch: the
 *        stamps of cst_gemm_desc.k_live for the zero-padded frame axis [B][T + k - 1 (+ 1 for even k)], or NULL.
 * ------------------------------------------------------------------------------------------ */
int cst_posconv_fwd(const void* x, const void* w, const void* bias, void* y, void* z, const int32_t* m_len, int64_t B, int64_t T,
                    int64_t C, int64_t groups, int64_t k, cst_stream stream);
int cst_posconv_dx(const void* dz, const void* wflip, const void* dy, void* dx, const int32_t* m_len, int64_t B, int64_t T,
                   int64_t C, int64_t groups, int64_t k, cst_stream stream);
int cst_posconv_dw(const void* dz, const void* x, void* dw, void* db, const uint32_t* k_live, uint32_t k_epoch, int64_t B,
                   int64_t T, int64_t C, int64_t groups, int64_t k, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention (flash-style, scores never reach HBM) — replaces
 * F.multi_head_attention_forward (modules/multihead_attention.py:155-187) and the in-tree
 * bmm/softmax/bmm branch (:326-361):  O = softmax(scale * Q K^T + masks) V, softmax in fp32.
 * Modes covered by the descriptor: padded self-attention (key_padding_mask), memory attention
 * (Tq = M slots, Tk = encoder frames: the column mask of w2v2_transformer_interlingua.py:284-288
 * is "keys = first Tk columns"), causal decoder self-attention, cross-attention, and
 * single-query incremental decode (Tq = 1, Tk = cache length).
 * Q,K,V,O element (b,h,t,d) at ptr[b*sb + h*sh + t*st + d]; D in {32, 64}; d contiguous.
 * key_padding_mask: uint8 [B, Tk] (1 = pad -> -inf), row stride kpm_stride; may be NULL.
 * lse: fp32 [B,H,Tq] log-sum-exp of the scaled masked scores (saved for backward).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;
  int64_t B, H, Tq, Tk, D;
  const void* Q; int64_t q_sb, q_sh, q_st;
  const void* K; int64_t k_sb, k_sh, k_st;
  const void* V; int64_t v_sb, v_sh, v_st;
  void* O; int64_t o_sb, o_sh, o_st;
  float* lse;
  const uint8_t* key_padding_mask; int64_t kpm_stride;
  int causal;
  float scale;
  float drop_p; uint32_t drop_key;   /* attention dropout (multihead_attention.py:359): P * keep(drop_key, row (b*H+h)*Tq + q, key k) / (1-p),
                                        keep = the separable mask of csrc/cst_common.h (cst_adrop_*; numpy twin rng.keep_mask_attn_numpy);
                                        the backward call must carry the same two values */
  /* backward only */
  const void* dO; int64_t do_sb, do_sh, do_st;
  void* dQ; int64_t dq_sb, dq_sh, dq_st;
  void* dK; int64_t dk_sb, dk_sh, dk_st;
  void* dV; int64_t dv_sb, dv_sh, dv_st;
  float* delta;  /* fp32 [B,H,Tq] workspace: rowsum(dO * O) */
  /* optional int32 [B] (NULL = none): the caller's promise that every key >= kv_len[b] is padding in key_padding_mask
   * (trailing padding of a length-sorted batch).  Those key tiles are skipped in all three kernels — they contribute
   * exact zeros, so results are bit-identical to the unskipped run; key_padding_mask still governs keys < kv_len[b]. */
  const int32_t* kv_len;
  /* optional uint8 [B, H, ceil(Tq/64)] workspace of cst_attn_bwd (NULL = off): the delta pre-pass records which 64-query tiles
   * have a non-zero dO row and the dQ / dK-dV kernels stop at the last such tile — the tiles beyond it contribute exact zeros
   * (dP = dO V^T = 0 and delta = 0 give dS = 0), so the gradients are bit-identical to the full walk. */
  uint8_t* q_flags;
  /* optional int32 [B+1] (NULL = dense [B, T] batches): PACKED self-attention over the row sets of cst_rows_pack.  Q / K / V / O and
   * all gradients are [rows, H*D] (the *_sb batch strides are ignored; Q, K and V share one row stride); sequence b owns rows
   * [seq_offsets[b], seq_offsets[b+1]) as QUERIES and its first kv_len[b] rows as KEYS (kv_len NULL: all of them; the remaining
   * rows are the padding frames kept for their outputs: they attend, nobody attends to them, their dK / dV are zero).  Tq = Tk =
   * the longest sequence: it sizes the grid and strides lse / delta / q_flags [B, H, Tq] and the dropout index space, so that a
   * packed call draws exactly the dropout masks of the dense call it replaces.  key_padding_mask must be NULL. */
  const int32_t* seq_offsets;
  /* optional uint64 [B, ceil(Tk/64)] (NULL = none): key_padding_mask packed one word per 64-key tile (bit k of word j: key 64 j + k is
   * masked; bits of keys >= Tk set).  With it (or without any key_padding_mask) bf16 / D = 64 / non-causal problems run the DMA-staged
   * kernels (csrc/attention_fast.inc), which read tile masks from scalar registers; without it a masked problem runs the generic
   * kernels.  Must describe exactly key_padding_mask. */
  const uint64_t* kpm_bits;
  /* optional workspace of cst_attn_bwd, cst_attn_bwd_workspace() bytes (NULL = generic backward kernels): the dQ kernel writes
   * -lse * log2(e) and -delta / dropout-scale per query, padded to whole 64-query tiles, and (round 5) every query row's 32-byte
   * dropout signature behind them, for the DMA-staged dK/dV kernel. */
  void* bwd_ws;
} cst_attn_desc;

int64_t cst_attn_bwd_workspace(const cst_attn_desc* d);
int cst_attn_fwd(const cst_attn_desc* d, cst_stream stream);
int cst_attn_bwd(const cst_attn_desc* d, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * wav2vec2 conv layer 0 (Cin = 1) fused with GroupNorm(C groups) and GELU — replaces
 * Conv1d + Fp32GroupNorm + GELU at models/wav2vec/wav2vec2.py:697-753 (layer 0) and
 * modules/fp32_group_norm.py:13-25.  The pre-norm conv output is never written to HBM
 * (two-phase: statistics, then normalise+GELU+store), backward recomputes it from the wave.
 *   wav [B,S] fp32 (the raw samples as the collater hands them over; never down-cast);
 *   w [C,k], gamma, beta [C] in `dtype`;  y [B,L,C] channels-last in `dtype`;
 *   mean,rstd fp32 [B,C];  gram fp32 [B, k*k + k] (per-utterance lag moments, saved for backward);
 *   L = (S-k)/stride + 1;  k <= 16;  C % 8 == 0, C <= 2048.
 *   A (k, stride, C) whose kernels would need more dynamic LDS than the 160 KiB of a CU is refused (CST_ERR_BAD_ARG) before anything
 *   is launched or written: forward 4 (k C + C + 64 stride + k) bytes, backward 4 (k C + 4 C + 2048 stride + k); at k = 10 with C / 4
 *   a divisor of 256 the register kernels need 4 (128 stride + 10) and 4 (2048 stride + 10) instead.
 * ------------------------------------------------------------------------------------------ */
/* Live-frame limits of the conv feature extractor (wav2vec2.py:685-763) for one batch, all layers in ONE launch: which frames of every
 * layer's output anything reads, from the count of real frames behind the LAST layer (frames past an utterance's end are zeroed
 * behind the stack, wav2vec2.py:820-821, and carry exactly zero gradient).  They feed cst_gemm_desc.m_len / k_len of the conv GEMMs.
 *   nz_last int32 [B]: real frames per utterance behind layer L-1;  k, stride: int32 [L] kernel widths / strides;  S: samples.
 *   out int32 [L][1 + smax][B], smax = max stride of layers 1..L-1:
 *     out[i][0][b]     = nz_i[b]: layer i's frames t >= nz_i[b] are unread; nz_{i-1} = (nz_i - 1) stride_i + k_i (0 if nz_i = 0),
 *                        each clamped to the layer's frame count
 *     out[i][1 + r][b] = max(0, ceil((nz_{i-1}[b] - r) / stride_i)) for i >= 1, r < stride_i: the live rows of residue class r of
 *                        layer i's INPUT gradient (the windowed dX GEMMs of functional.conv1d_cl)
 *     out[0][1][b]     = frames of layer 0 that layer 1's live 256-row output tiles read: min(len_0, ceil(nz_1 / 256) 256 stride_1 +
 *                        k_1) — what cst_conv0_gn_gelu_fwd has to write (L >= 2)
 * L <= 8, strides <= 8. */
int cst_conv_row_limits(const int32_t* nz_last, const int32_t* k, const int32_t* stride, int L, int64_t S, int32_t* out, int64_t B,
                        int smax, cst_stream stream);
/* workspace: cst_conv0_fwd_workspace() bytes — per-block partial moments, added up in a fixed order (no atomics: the statistics,
 * and with them the whole forward pass, are bit-reproducible run to run). */
int64_t cst_conv0_fwd_workspace(int64_t B, int64_t S, int k, int stride);
/* frame_limit (optional, int32 [B]): forward — frames t >= frame_limit[b] of utterance b are read by nobody (cst_conv_row_limits
 * out[0][1]: behind the rows the next layer's live 256-row tiles reach) and are neither computed nor written (y keeps whatever the
 * buffer held there; the GroupNorm statistics still cover all L frames, as the reference's do over the zero-padded audio);
 * backward — dy is exactly zero from frame frame_limit[b] on (cst_conv_row_limits out[0][0]) and those frames are not read.
 * NULL = every frame. */
int cst_conv0_gn_gelu_fwd(const float* wav, const void* w, const void* gamma, const void* beta,
                          void* y, float* mean, float* rstd, float* gram, float* workspace, const int32_t* frame_limit, int64_t B,
                          int64_t S, int64_t C, int k, int stride, float eps, int dtype, cst_stream stream);
/* dw [C,k], dgamma [C], dbeta [C] are fp32 and overwritten.
 * workspace: cst_conv0_bwd_workspace() bytes — per-block partial sums [B][blocks][k+2][C] + their fixed-order reduction
 * (no atomics: bit-reproducible gradients). */
int64_t cst_conv0_bwd_workspace(int64_t B, int64_t S, int64_t C, int k, int stride);
int cst_conv0_gn_gelu_bwd(const void* dy, const float* wav, const void* w, const void* gamma,
                          const void* beta, const float* mean, const float* rstd, const float* gram,
                          float* dw, float* dgamma, float* dbeta, float* workspace, const int32_t* frame_limit,
                          int64_t B, int64_t S, int64_t C, int k, int stride, int dtype,
                          cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * The feature extractor in extractor_mode="layer_norm" (ABI 8; wav2vec2.py:714-724, the published large models): every conv layer
 * is followed by a LayerNorm over the C channels of a FRAME (fp32 statistics, Fp32LayerNorm) and GELU.  No statistic crosses
 * frames, so every frame limit below is exact without caveat.  All sums over frames go through per-block partials in the caller's
 * workspace, added in a fixed order (no atomics: bit-reproducible forward and backward).
 *
 * Layer 0: y = GELU(LayerNorm_C(conv1d(wav, w, stride) + bias)), one pass (the pre-norm conv output is never written; the backward
 * recomputes it from the samples).
 *   wav [B,S] fp32 (never down-cast);  w [C,k], bias, gamma, beta [C] in `dtype`;  y [B,L,C] channels-last in `dtype`;
 *   mean, rstd fp32 [B,L] (per frame);  L = (S-k)/stride + 1;  k <= 16;  stride <= 7;  C % 8 == 0, C <= 512 (one wave64 holds a frame).
 *   frame_limit (optional, int32 [B]): forward — frames t >= frame_limit[b] are neither computed nor written (y, mean, rstd keep
 *   whatever the buffers held); backward — dy is exactly zero from there on and is not read.  NULL = every frame.
 *   dw [C,k], dbias, dgamma, dbeta [C] are fp32 and overwritten (there is no input gradient: the input is audio). */
int cst_conv0_ln_gelu_fwd(const float* wav, const void* w, const void* bias, const void* gamma, const void* beta, void* y,
                          float* mean, float* rstd, const int32_t* frame_limit, int64_t B, int64_t S, int64_t C, int k,
                          int stride, float eps, int dtype, cst_stream stream);
int64_t cst_conv0_ln_bwd_workspace(int64_t B, int64_t S, int64_t C, int k, int stride);
int cst_conv0_ln_gelu_bwd(const void* dy, const float* wav, const void* w, const void* bias, const void* gamma, const void* beta,
                          const float* mean, const float* rstd, float* dw, float* dbias, float* dgamma, float* dbeta,
                          float* workspace, const int32_t* frame_limit, int64_t B, int64_t S, int64_t C, int k, int stride,
                          int dtype, cst_stream stream);
/* Layers 1..: y = GELU(LayerNorm_C(u)) over channels-last rows u [B,L,C] (the conv GEMM's output with bias), C % 8 == 0, C <= 2048.
 *   mean, rstd fp32 [B,L].  row_limit (optional, int32 [B]; cst_conv_row_limits out[i][0], the limits the conv GEMMs take): rows
 *   t >= row_limit[b] are read by nobody — they are not read or computed, and y (forward) / du (backward, where dy is exactly zero)
 *   are written as zeros there, so that tiles of the neighbouring GEMMs that straddle a limit meet numbers.
 *   Backward: du in `dtype` with `du_batch_stride` elements between utterances (>= L*C: the windowed dX GEMMs of the conv in front
 *   want a spare row before and after every utterance); dgamma, dbeta fp32 [C]; dcolsum (optional) fp32 [C] = column sums of du,
 *   i.e. the gradient of the conv bias in front.  workspace: cst_ln_gelu_bwd_workspace(B*L, C) bytes. */
int cst_ln_gelu_fwd(const void* u, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                    const int32_t* row_limit, int64_t B, int64_t L, int64_t C, float eps, int dtype, cst_stream stream);
int64_t cst_ln_gelu_bwd_workspace(int64_t rows, int64_t C);
int cst_ln_gelu_bwd(const void* dy, const void* u, const void* gamma, const void* beta, const float* mean, const float* rstd,
                    void* du, int64_t du_batch_stride, float* dgamma, float* dbeta, float* dcolsum, float* workspace,
                    const int32_t* row_limit, int64_t B, int64_t L, int64_t C, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise / reduction helpers (HBM-bound)
 * ------------------------------------------------------------------------------------------ */
/* GLU over the channel pairs (c, c+C) of z [rows, 2C] -> y [rows, C]  (F.glu, s2t_transformer.py:74) */
int cst_glu_fwd(const void* z, void* y, int64_t rows, int64_t C, int dtype, cst_stream stream);
int cst_glu_bwd(const void* dy, const void* z, void* dz, int64_t rows, int64_t C, int dtype, cst_stream stream);
/* dx = dy * act'(z)  (GELU: modules/gelu.py:25; ReLU) */
int cst_act_bwd(const void* dy, const void* z, void* dx, int64_t n, int act, int dtype, cst_stream stream);
/* y = act(x) */
int cst_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, cst_stream stream);
/* out[c] = sum_r x[r, c]  (bias gradients); out fp32 [cols], overwritten */
int cst_colsum(const void* x, int64_t ldx, float* out, int64_t rows, int64_t cols, int dtype, cst_stream stream);
/* Gradient of `residual + dropout(linear(x))` on its way into the Linear's backward, in ONE pass: xd = x * keep(key, index) / (1 - p)
 * (FairseqDropout backward, modules/fairseq_dropout.py:20-37: the mask of the forward call, element index = r * cols + c) stored in
 * `dtype`, and out[c] = sum_r xd[r][c] (the bias gradient) over the STORED values — the same bits as cst_dropout followed by
 * cst_colsum_typed.  x, xd contiguous [rows, cols]; workspace: cst_colsum_workspace(rows, cols) bytes; row_live / epoch as in
 * cst_colsum_typed_live (optional): all-zero 64-row tiles are written as zeros without being read. */
int cst_dropout_colsum(const void* x, void* xd, void* out, void* workspace, int64_t rows, int64_t cols, int dtype, int out_dtype,
                       float p, uint32_t key, const uint32_t* row_live, uint32_t epoch, cst_stream stream);
/* the same sums without atomics: row-chunk partials in `workspace` (cst_colsum_workspace bytes), reduced in a fixed order and
 * written in `out_dtype` (the bias parameter's dtype) — deterministic, no zero-fill and no conversion launch around it.
 * out == NULL (here, in cst_colsum_typed_live and in cst_dropout_colsum): the second stage is left to the caller — the partials stay in
 * `workspace` as fp32 [cst_colsum_workspace / (4 cols)][cols], to be finished by cst_reduce_multi with order 1 (same summation order,
 * same bits), together with the other deferred reductions of a backward pass. */
int64_t cst_colsum_workspace(int64_t rows, int64_t cols);
int cst_colsum_typed(const void* x, int64_t ldx, void* out, void* workspace, int64_t rows, int64_t cols, int dtype, int out_dtype,
                     cst_stream stream);
/* the same with live-tile stamps of x's rows (cst_layernorm_bwd_tiles): 64-row tiles whose stamp != epoch are all zero and skipped */
int cst_colsum_typed_live(const void* x, int64_t ldx, void* out, void* workspace, int64_t rows, int64_t cols, int dtype,
                          int out_dtype, const uint32_t* row_live, uint32_t epoch, cst_stream stream);
/* gradient of a strided conv1d input from the column-gradient rows of the implicit GEMM:
 * dx[b, l, c] = sum_{t,j : t*stride + j = l} dcol[b, t, j*C + c];  optionally multiplied by
 * act'(z[b,l,c]) (GELU of the previous conv layer).  dcol [B, Lout, k*C]; dx/z [B, Lin, C]. */
int cst_col2im1d(const void* dcol, const void* z, void* dx, int64_t B, int64_t Lin, int64_t Lout,
                 int64_t C, int k, int stride, int pad, int dact, int dtype, cst_stream stream);
/* Weight normalisation along the LAST dimension — nn.utils.weight_norm(conv, dim=2) of the wav2vec2 positional convolution
 * (models/wav2vec/wav2vec2.py:773-779): v, w, dw, dv [R, C] contiguous (R = C_out * C_in / groups, C = kernel width), g, dg [C],
 * norm fp32 [C] (saved by the forward call).  w = v * g / ||v[:, c]||;  dv = (g/n) (dw - v dot / n^2), dg = dot / n, dot = sum_r dw v.
 * Fixed summation order.  C % 8 == 0, C <= 256, (C / 8) divides 256.  workspace: cst_weight_norm_workspace(R, C) bytes. */
int64_t cst_weight_norm_workspace(int64_t R, int64_t C);
int cst_weight_norm_fwd(const void* v, const void* g, void* w, float* norm, void* workspace, int64_t R, int64_t C, int dtype, cst_stream stream);
int cst_weight_norm_bwd(const void* v, const void* g, const void* dw, const float* norm, void* dv, void* dg, void* workspace, int64_t R,
                        int64_t C, int dtype, cst_stream stream);
/* dst [C, R] = src [R, C] transposed (contiguous both; R, C multiples of the 16-byte vector).  The Linear dX GEMMs take the weight this
 * way (dY W with W^T k-major: both operands read as the forward GEMM reads them). */
int cst_transpose2d(const void* src, void* dst, int64_t R, int64_t C, int dtype, cst_stream stream);
/* The same for a whole table of matrices in one launch (every Linear weight of a model once per update, after the optimizer step):
 * items_dev = DEVICE array of n entries ordered by tile0 = the number of 64 x 64 tiles of the entries before it (entry 0: 0);
 * total_tiles = their sum over the table.  One dtype per call. */
typedef struct cst_transpose_item {
  const void* src; void* dst;
  int64_t R, C;      /* src [R, C] -> dst [C, R] */
  int64_t tile0;
} cst_transpose_item;
int cst_transpose2d_multi(const cst_transpose_item* items_dev, int n, int64_t total_tiles, int dtype, cst_stream stream);
/* The second stage of many fixed-order reductions in ONE launch (ABI 5).  The reference has no counterpart: its weight / bias /
 * LayerNorm gradients come out of single ATen calls (F.linear / F.layer_norm backward at modules/transformer_layer.py:105-155,
 * multihead_attention.py:326-361); here the weight-gradient GEMMs of the small layers split K, the LayerNorm backward reduces over
 * row blocks, and each used to finish with a launch of its own.  cst_gemm (desc.defer_reduce) and cst_layernorm_bwd (dgamma = dbeta
 * = NULL) leave their fp32 partials in the caller's workspace; this call finishes up to CST_REDUCE_MAX_ITEMS of them:
 *   dst[i] = sum_{p < P} src[p * stride + i],  i < L      (L % 8 == 0, src / dst 16-byte aligned, stride % 4 == 0)
 * in the summation order of the launch-each kernel the item stands in for — order 0: p = 0, 1, 2, ... (cst_gemm's split-K reduce
 * and its colsum slices), order 1: 64 interleaved chains p = g, g + 64, ... added 0..63 (cst_layernorm_bwd's second stage) — so a
 * gradient has the same bits whichever route finished it; dst in dst_dtype (fp32 or bf16).  `items` is a HOST array (it travels in
 * the kernel arguments: no host-to-device copy, no synchronisation); block0 is filled in by the library. */
#define CST_REDUCE_MAX_ITEMS 64
typedef struct cst_reduce_item {
  const float* src; void* dst;
  int64_t stride, L;
  int32_t P, dst_dtype, block0, order;
} cst_reduce_item;
int cst_reduce_multi(const cst_reduce_item* items, int n, cst_stream stream);
/* y[r,:] = mask[r] ? 0 : x[r,:]   (x[padding_mask] = 0, wav2vec2.py:820-821) */
int cst_mask_rows(const void* x, const uint8_t* mask, void* y, int64_t rows, int64_t cols, int dtype, cst_stream stream);

/* Packed (padding-free) row sets.  A length-sorted, right-padded batch [B, T, C] of a row-wise network (LayerNorm, Linear, FFN,
 * self-attention with a key-padding mask: wav2vec2.py:818-845, 937-957) carries, per utterance, `len` real frames followed by
 * padding frames whose values the reference also computes.  Past the reach of the positional convolution (len + conv_pos/2) all
 * padding frames of an utterance enter the layer stack with the SAME vector and keep identical values through every row-wise
 * layer, so the stack may run on  n_b = min(T, len_b + conv_pos/2 + 1)  rows per utterance — the last one standing for all the
 * identical rows behind it — and reproduce the padded result bit for bit (dropout off; with dropout on the padding rows share a
 * mask).  seq_off int32 [B+1]: sequence b owns packed rows [seq_off[b], seq_off[b+1]).
 *   cst_rows_pack   : dst[seq_off[b] + t] = src[b, t]; with tail_sum the last packed row of a sequence receives the SUM of
 *                     src[b, n_b - 1 .. T - 1] in index order (the gradient of cst_rows_unpack with tail_broadcast; deterministic).
 *   cst_rows_unpack : dst[b, t] = src[seq_off[b] + min(t, n_b - 1)] with tail_broadcast, zeros beyond n_b otherwise (the
 *                     gradient of cst_rows_pack without tail_sum).
 * C % 8 == 0. */
int cst_rows_pack(const void* src, const int32_t* seq_off, void* dst, int64_t B, int64_t T, int64_t C, int tail_sum, int dtype,
                  cst_stream stream);
int cst_rows_unpack(const void* src, const int32_t* seq_off, void* dst, int64_t B, int64_t T, int64_t C, int tail_broadcast, int dtype,
                    cst_stream stream);

/* y = x * keep / (1 - p): FairseqDropout (modules/fairseq_dropout.py:20-37) forward; the same call on dy is its backward.
 * The mask is counter-based — keep(key, element index), csrc/cst_common.h — so nothing is stored between the two calls and
 * fused epilogues (cst_gemm / cst_attn_*) regenerate the identical mask from the same key.  n elements, contiguous. */
int cst_dropout(const void* x, void* y, int64_t n, float p, uint32_t key, int dtype, cst_stream stream);
/* y = alpha * x * keep / (1 - p)   (n % 8 == 0): the gradient of `dropout(alpha * x + const)` — the dense-feature branch of
 * cst_embed_pos_fwd below. */
int cst_dropout_scale(const void* x, void* y, int64_t n, float alpha, float p, uint32_t key, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Token embedding + sinusoidal positions of the TRAINING path — replaces, in one kernel,
 *   embed_scale * nn.Embedding(tokens)            models/transformer.py:744-760 (decoder), w2v2_transformer_interlingua.py:216, :231
 *   + SinusoidalPositionalEmbedding.forward       modules/sinusoidal_positional_embedding.py:60-105: weights.index_select(make_positions(input))
 *     with utils.make_positions                   utils.py:235-245: pad_idx + cumsum(non-pad) for non-pad symbols, pad_idx for pads
 *   + FairseqDropout                              modules/fairseq_dropout.py:20-37 (counter-based mask, see cst_dropout)
 *   out[b,t,:] = dropout(scale * src[b,t,:] + pos_table[position(b,t),:])
 * src: exactly one of `embed` [V, C] (row tokens[b,t]; ids outside [0, V) read the pad row) or `x` [B, T, C] (dense features: the
 *   audio branch of S2T_W2V2_TransformerEncoder, w2v2_transformer.py:352-358).
 * position source: `pad_mask` uint8 [B, T] when given (the encoders pass their padding mask: non-pad <=> mask != pad_idx, as
 *   `tensor.ne(padding_idx)` reads a 0/1 mask), else `tokens` (non-pad <=> tokens != pad_idx).
 * pos_table: fp32 [pos_rows, C], the reference's sin || cos table with row pad_idx zero; pos_rows >= pad_idx + 1 + T; NULL = no
 *   positional term.  C % 8 == 0.  tokens int64 [B, T]. */
int cst_embed_pos_fwd(const int64_t* tokens, const uint8_t* pad_mask, const void* embed, const void* x, const float* pos_table,
                      float scale, int64_t pad_idx, void* out, int64_t B, int64_t T, int64_t C, int64_t V, int64_t pos_rows,
                      float drop_p, uint32_t drop_key, int dtype, cst_stream stream);
/* Gradient of the embedding table of cst_embed_pos_fwd — replaces ATen's embedding_dense_backward (sort by key + segmented
 * reduce, 5 kernels; F.embedding with padding_idx: the pad row receives no gradient):
 *   dE[v,:] = scale * sum over occurrences (b,t) of v != pad_idx, in (b,t) order, of keep(b,t,:) * dy[b,t,:];  all other rows 0.
 * Deterministic (fixed summation order, no atomics).  dy [n, C] (n = B*T), tokens int64 [n], dE [V, C] in grad_dtype (fp32 or
 * dtype; fully overwritten).  C % 8 == 0, C <= 8192. */
int cst_embed_bwd(const void* dy, const int64_t* tokens, void* dE, float scale, int64_t pad_idx, int64_t n, int64_t C, int64_t V,
                  float drop_p, uint32_t drop_key, int dtype, int grad_dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Label-smoothed cross entropy over vocabulary logits — replaces fp32 log_softmax
 * (models/fairseq_decoder.py:75-79 -> utils.py:469-473) + label_smoothed_nll_loss
 * (criterions/label_smoothed_cross_entropy.py:13-30), reduce=True, ignore_index=pad.
 *   logits [rows, V] (dtype), target int64 [rows];  out2 fp32[2] = {loss_sum, nll_sum} (overwritten);
 *   lse fp32 [rows] saved for backward;  row_ws fp32 [2 * rows]: the per-row terms, added up in a fixed order by a second
 *   one-workgroup kernel (no atomics: the loss is bit-reproducible run to run).
 * bwd: dlogits = gscale * d loss / d logits  (gscale = upstream grad of the summed loss).
 * ------------------------------------------------------------------------------------------ */
int cst_ls_ce_fwd(const void* logits, const int64_t* target, float* out2, float* lse, float* row_ws,
                  int64_t rows, int64_t V, float eps, int64_t pad_idx, int dtype, cst_stream stream);
int cst_ls_ce_bwd(const void* logits, const int64_t* target, const float* lse, const float* gscale,
                  void* dlogits, int64_t rows, int64_t V, float eps, int64_t pad_idx, int dtype,
                  cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Scores of GIVEN target tokens (ABI 13; fairseq-generate --score-reference) — replaces, in fairseq/sequence_scorer.py, the fp32
 * (log-)softmax of every ensemble member's [B, T, V] decoder output (:77-79 -> models/fairseq_decoder.py:58-79 -> utils.py:469-473),
 * the gather of the target column (:54-59, :81), the average over the members (:96-111) and the per-sentence mean (:118-127).  The
 * float32 [B, T, V] probability tensor the reference builds per member is never materialised.
 *   logits / logits_n: N = `members` matrices (1 <= N <= 8), member 0 in `logits`, members 1 .. N-1 in the HOST array logits_n[0 ..
 *     N-2] (it travels in the kernel arguments, as cst_beam_desc.logits_n does; NULL when N = 1).  Each is [rows = B*T, V] in `dtype`
 *     with the common row stride ld >= V (elements); any V, any ld, any element-aligned base: 16-byte loads are used on the part of a
 *     row between its first and last 16-byte boundary, scalar loads in front and behind.
 *   target int64 [B, T] with 0 <= id < V or id == pad (the kernel cannot validate device data: the caller checks — kernels.score_tokens
 *     does so on the host; an id outside the vocabulary yields NaN and reads nothing).
 *   pos fp32 [B, T], score fp32 [B], len int32 [B]: all overwritten.
 * All in fp32.  Per non-pad position and member m, with mx_m the row's maximum (taken out before the exponentials):
 *     lse_m = mx_m + log(sum_v exp(x_v - mx_m)),   l_m = x_target - lse_m;
 *     N = 1: pos = l_1;      N > 1: pos = logsumexp_m(l_m) - log N  (the members' maximum taken out likewise);
 *   pos = 0 at pad positions, whose logits are NOT read;  len[b] = the non-pad targets of sentence b;
 *   score[b] = (sum of the non-pad pos[b, :]) / len[b], added in a fixed order without atomics (bit-reproducible); a sentence without
 *   targets gives the reference's 0 / 0 = NaN.
 * DIFFERENCE to the reference: for N > 1 it averages the members' PROBABILITIES in fp32 and takes the log (:96-111); the log-domain
 * form here is the same number wherever the reference's is finite, and stays finite where every member's probability underflows fp32
 * (the reference then returns log 0 = -inf).
 * Bad scalar arguments (null operand, dtype, B / T / V < 1, ld < V, members outside 1 .. 8, a missing member): CST_ERR_BAD_ARG, nothing
 * is launched.
 * ------------------------------------------------------------------------------------------ */
int cst_score_tokens(const void* logits, const void* const* logits_n, int64_t members, int64_t ld, const int64_t* target, int64_t pad,
                     float* pos, float* score, int32_t* len, int64_t B, int64_t T, int64_t V, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Connectionist temporal classification on RAW logits (criterion `ctc`; added at ABI 13 without a bump, as cst_beam_step_lm was: no
 * existing signature changed).  The fp32 [T, B, V] log-probability tensor of the reference is never materialised, on either pass.
 *
 * Common operands.  logits: `dtype` (fp32 or bf16), element (t, b, v) at logits[t * stride_t + b * stride_b + v] — unit class stride,
 *   strides in elements, both >= V, any element-aligned base: a contiguous [T, B, V] tensor (stride_t = B V, stride_b = V) and the
 *   time-major view of batch-major memory (stride_t = V, stride_b = T V) are read by the same kernel without a copy, and give EQUAL
 *   BITS: every sum's order depends on class indices only, never on a row's alignment (16-byte loads where a row's base is 16-byte
 *   aligned, scalar loads of the same elements in the same order where it is not).
 *   targets int64 [B, Lmax], padded; target_len int64 [B], input_len int64 [B], both on the device (clamped to [0, Lmax] / [0, T]).
 *   Labels must lie in [0, V) and differ from `blank` (the kernel cannot validate device data: kernels.ctc_fwd checks on request; a
 *   label outside the vocabulary reads nothing and yields NaN).  0 <= blank < V.
 *   Lmax <= 2047 (the recursion keeps the 2 L + 1 states of one time step twice in LDS: 2 x 4099 floats + 4095 flags = 36 KiB of the
 *   64 KiB a workgroup may hold statically); beyond: CST_ERR_UNSUPPORTED, nothing launched.  Null operands, a bad dtype, T / B / V < 1,
 *   B > 65535, blank outside [0, V), a stride below V: CST_ERR_BAD_ARG, nothing launched, no output touched.
 *
 * cst_ctc_fwd replaces log_softmax(logits.float()) + F.ctc_loss(reduction = "sum") (fairseq/criterions/ctc.py:97-113; likewise
 *   criterions/ctc_chi.py).  The standard recursion over the extended sequence l' = (blank, l1, blank, ..., blank) of S = 2 L + 1
 *   states, in log space, in fp32; the skip s - 2 -> s is allowed only when l'_s != blank and l'_s != l'_{s-2}.
 *   Outputs (fp32, overwritten): nll [B] (+inf for an infeasible utterance, also under zero_infinity); loss [1] = the sum of nll in a
 *   fixed order (zero_infinity: +inf terms count 0); lse [B, T] = each live frame's log-sum-exp (0 at frames >= input_len[b], whose
 *   logits are NOT read).  Workspaces kept for backward, [B, T, 2 Lmax + 1] fp32 each, written only at live frames and states:
 *   emit (the extended labels' log-probabilities), alpha, beta (the forward / backward variables, both INCLUDING the emission at t);
 *   beta may be NULL when no gradient is wanted — then only alpha runs.  alpha and beta run as two workgroups per utterance in ONE
 *   launch.  An empty target is legal (all-blank paths).  No atomics: bit-reproducible, and independent of the rest of the batch.
 * cst_ctc_bwd: dlogits (`dtype`, own strides, every element of the T x B x V box overwritten) = gscale[0] * d loss / d logits, fused
 *   with the log-softmax backward; at a live frame  softmax(x)[v] - exp(logsumexp_{s: l'_s = v}(alpha_t(s) + beta_t(s)) + nll_b -
 *   logp_t(v)).  Exactly 0 at frames >= input_len[b] and, under zero_infinity, at every frame of an infeasible utterance; without
 *   zero_infinity such an utterance's gradient is non-finite (as torch's) and the others are unaffected.  A class's occupancy sum over
 *   its states has a fixed order (one owner thread per class).  gscale: fp32 device scalar (the upstream gradient; no host read).
 * cst_ctc_greedy replaces the host copy of the fp32 [B, T, V] log-probabilities and the per-utterance argmax().unique_consecutive()
 *   loop of criterions/ctc.py:116-160: per utterance the argmax over classes (a tie: the lowest index) of the frames before
 *   input_len[b], runs of equal ids collapsed, then `blank` dropped.  ids int32 [B, T]: the counts[b] ids of utterance b, then -1;
 *   counts int32 [B]; argmax_ws int32 [B, T] scratch.
 * ------------------------------------------------------------------------------------------ */
int cst_ctc_fwd(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* targets, int64_t Lmax, const int64_t* target_len,
                const int64_t* input_len, int64_t blank, int zero_infinity, float* nll, float* loss, float* lse, float* emit, float* alpha,
                float* beta, int64_t T, int64_t B, int64_t V, int dtype, cst_stream stream);
int cst_ctc_bwd(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* targets, int64_t Lmax, const int64_t* target_len,
                const int64_t* input_len, int64_t blank, int zero_infinity, const float* nll, const float* lse, const float* alpha,
                const float* beta, const float* gscale, void* dlogits, int64_t dstride_t, int64_t dstride_b, int64_t T, int64_t B,
                int64_t V, int dtype, cst_stream stream);
int cst_ctc_greedy(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank, int32_t* argmax_ws,
                   int32_t* ids, int32_t* counts, int64_t T, int64_t B, int64_t V, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * CTC prefix beam search on RAW logits (fairseq_infer.py --w2l-decoder beam; added at ABI 13 without a bump, as the CTC entries above
 * were: no existing signature changed).  It stands where examples/speech_recognition/w2l_decoder.py puts the flashlight decoders
 * (W2lKenLMDecoder, W2lFairseqLMDecoder) behind examples/speech_recognition/infer.py; it is NOT a port of them: flashlight's
 * lexicon-free decoder keeps the best alignment per state, this one sums all alignments of a prefix (Graves 2006 §7.5.3; Hannun et
 * al. 2014, Alg. 1).  W2lViterbiDecoder with the ctc criterion is cst_ctc_greedy.  Operands, strides, dtypes, the clamping of input_len
 * and the CST_ERR_BAD_ARG refusals (nothing launched, no output touched) are those of the CTC block above.
 *
 * cst_ctc_topn, one workgroup per live frame (64 threads for V <= 512, else 256), writes (all [B, T] or [B, T, N], overwritten):
 *   lse fp32: the frame's log-sum-exp, summed in the order of cst_ctc_fwd (equal bits, independent of the layout);
 *   blank_lp fp32 = x[blank] - lse;  tok_id int32 / tok_lp fp32: the N most probable classes other than `blank` and their
 *   log-probabilities x - lse, ordered by (log-probability descending, class id ascending); -1 / -inf past the V - 1 classes there are.
 *   Frames at or past input_len[b] are not read: lse 0, blank_lp -inf, tok_id -1, tok_lp -inf.  1 <= N <= 128, beyond:
 *   CST_ERR_UNSUPPORTED.
 * cst_ctc_beam, one workgroup per utterance, loops over that utterance's frames.  The beam holds at most K prefixes with (p_b, p_nb),
 *   the fp32 log-probabilities of the prefix's alignments so far that end in blank / in non-blank; it starts as the empty prefix with
 *   (0, -inf).  (+) is logaddexp(a, b) = max + logf(1 + expf(min - max)).  Per frame and beam prefix l, tot = p_b (+) p_nb:
 *     stay    p_b'(l) = tot + blank_lp;  p_nb'(l) = p_nb(l) + (x[last(l)] - lse) for a non-empty l — the last token's EXACT
 *             log-probability, read from the logits, whether or not the frame's list holds it;
 *     extend  by each listed token c:  p_nb'(l + c) = (c == last(l) ? p_b(l) : tot) + tok_lp(c).
 *   Identity is exact: a prefix is a node (parent node, token) of an append-only per-utterance trie, and l + c IS beam entry l' exactly
 *   when parent(l') == node(l) and token(l') == c; that term is added to p_nb'(l') (after the stay term; a prefix has one parent, so
 *   one term at most) and is no candidate of its own.  Candidates score p_b' (+) p_nb'; those of score -inf or below (the best
 *   score - beam_threshold) are dropped, the best K survive, ties broken by source beam rank, then stay before extension, then token
 *   id.  A selected extension first looks (parent node, token) up among its parent's children — a prefix that left the beam and comes
 *   back gets the node it had, so a prefix has ONE node and the identity above is exact — and creates a node only where there is none:
 *   a frame adds at most K, and the 1 + T K nodes of the table suffice (the kernel checks all the same).  Nothing depends on the rest of the batch or on the order of execution: bit-reproducible.
 *   Outputs: hyp_tokens int32 [B, nbest, T] (-1 padded), hyp_len int32 [B, nbest], hyp_score fp32 [B, nbest] (-inf past n_hyp[b]),
 *   n_hyp int32 [B] = min(nbest, the final beam), best first.  input_len[b] = 0: one empty hypothesis of score 0.  1 <= nbest <= K.
 *   workspace: cst_ctc_beam_workspace_bytes(T, B, K, N) bytes, the node table — per utterance four int32 arrays of 1 + T K entries:
 *   parent, token, youngest child, next older sibling (0: none); node 0 is the empty prefix (-1, -1).  Readable after the call.
 *   trace_node int32 / trace_pb / trace_pnb fp32 [B, T, K]: the beam after each live frame, in rank order, -1 / -inf past its size;
 *   all three NULL: off.  Frames at or past input_len[b] are not written.
 *   Envelope: K <= 128, N <= 128 and K N <= 8192 (so K = 64 with N = 128, K = 128 with N <= 64).  The extension scores of one frame
 *   stay in LDS, 4 K N <= 32 KiB, beside 2 x 5 x 128 words of beam, 4 x 128 of stay terms, 2 x 128 of the frame's list and 2 x 128 of
 *   child-list heads and sources (9 KiB): 41 KiB of the 64 KiB a workgroup may hold statically, three workgroups in a CU's 160 KiB.  Beyond: CST_ERR_UNSUPPORTED, nothing
 *   launched (ctc_decoder.CtcBeamDecoder then takes its host route).
 * ------------------------------------------------------------------------------------------ */
int cst_ctc_topn(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank, int64_t N, float* lse,
                 float* blank_lp, int32_t* tok_id, float* tok_lp, int64_t T, int64_t B, int64_t V, int dtype, cst_stream stream);
int64_t cst_ctc_beam_workspace_bytes(int64_t T, int64_t B, int64_t K, int64_t N);
int cst_ctc_beam(const void* logits, int64_t stride_t, int64_t stride_b, const int64_t* input_len, int64_t blank, const float* lse,
                 const float* blank_lp, const int32_t* tok_id, const float* tok_lp, int64_t N, int64_t K, float beam_threshold,
                 int64_t nbest, void* workspace, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyp,
                 int32_t* trace_node, float* trace_pb, float* trace_pnb, int64_t T, int64_t B, int64_t V, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Contrastive head of wav2vec2 pre-training (added at ABI 13 without a bump: no existing signature changed).  Replaces sample_negatives
 * and compute_preds (fairseq/models/wav2vec/wav2vec2.py:454-525) and the cross entropy of criterions/wav2vec_criterion.py:64-103.  The
 * reference's [K' + 1, B, M, D] tensor of gathered targets and its [K' + 1, B M] logits are never built: one wave owns one masked
 * position and reads its K' + 1 target rows by index.  fp32 arithmetic on fp32 / bf16 storage; no float atomics and no host
 * synchronisation anywhere: every output is bit-reproducible.
 *
 * cst_w2v_negatives: out int32 [B, M, K + Kx] = the flat row indices (into [B M]) of each position's negatives.  Element e of `out`
 *   takes the 32-bit word bits = hash(key, e) of the dropout counter hash (csrc/cst_common.h: cst_drop_bits with e as the pair index).
 *   j < K (own utterance):  r = mulhi(bits, M - 1);  r += (r >= m);  out = b M + r  — never the position itself.
 *   j >= K (any utterance): r = mulhi(bits, B M - 1);  r += (r >= m);  out = r      — shifted past the position's TIME index m, which is
 *   what the reference does (its `tszs`, :481-493), so at b > 0 a cross-sample negative may be the position itself (it is then masked
 *   by cst_infonce_fwd like any negative equal to its positive).  The reference's cat(dim = 1) + view, which at Kx > 0 hands position m
 *   draws shifted against OTHER positions, is not reproduced.  Integers only; rng.negatives_numpy restates it bit for bit.
 *   Refused (CST_ERR_BAD_ARG, nothing launched): null out, B / M < 1, K + Kx < 1, K > 0 with M < 2, Kx > 0 with B M < 2, 2^31 elements.
 *
 * Common operands of the three cst_infonce entries: x [N, D] (the final_proj output at the masked positions, N = B M), y [N, D] (the
 *   project_q output), both `dtype`, contiguous, 16-byte aligned; idx int32 [N, KP] on the device, KP = K + Kx, values in [0, N) (the
 *   kernels cannot refuse device data: a value outside is clamped into the range); inv_temp = 1 / logit_temp.
 *   Target j of position p: j = 0 the positive y[p], j >= 1 the negative y[idx[p][j - 1]].
 *   cos = x.t / (max(|x|, 1e-8) max(|t|, 1e-8)) — the installed torch.cosine_similarity, each norm clamped on its own; logit = cos *
 *   inv_temp in fp32 (the reference rounds the logits to the storage type first: DESIGN.md); a negative whose row equals the positive's
 *   row element for element has logit -inf (compute_preds :514-523).
 *   Refused (CST_ERR_BAD_ARG, nothing launched, nothing touched): null operands, a bad dtype, N / KP / D < 1, D not a multiple of 8 or
 *   above 1024, KP > 1023, N (KP + 1) >= 2^31, a base that is not 16-byte aligned.
 * cst_infonce_fwd: nll fp32 [N] = logsumexp_j logit - logit_0 (exactly 0 where every negative is masked); loss fp32 [1] = their sum in
 *   a fixed tree, in double; counters int32 [2] = (correct, count): count = N, correct = the positions where argmax_j == 0 and not
 *   argmin_j == 0, ties to the lowest index (wav2vec_criterion.py:97-103).  Kept for backward: lse fp32 [N], nx fp32 [N] = |x_p|,
 *   ny fp32 [N] = |y_r| (each y row's norm is computed once, in a pre-pass).  flags int32 [N]: scratch.  logits_dbg: NULL on the training
 *   path; fp32 [N, KP + 1] receives the logits (tests).
 * cst_infonce_bwd_x: dx (`dtype`, [N, D]) = gscale[0] * d loss / d x; pairs fp32 [N, KP + 1, 2] = per (position, j) the pair
 *   (gscale[0] * d loss / d cos, cos), which cst_infonce_bwd_y consumes.  gscale: fp32 device scalar (no host read).  The logits are
 *   recomputed with the forward's operation sequence (equal bits), so only lse / nx / ny are kept between the passes.
 * cst_infonce_bwd_y: dy (`dtype`, [N, D]) through the inverted index (perm, offs) of the targets: perm int64 [N (KP + 1)] = the STABLE
 *   argsort of the keys cat(0 .. N-1, idx.flatten()) (value v < N: the positive of position v; else (p, j) = ((v - N) / KP, (v - N) %
 *   KP + 1)), offs int32 [N + 1] = the first sorted place of each row (offs[N] = N (KP + 1)): row r's list is perm[offs[r] ..
 *   offs[r + 1]), its own positive first, then the negatives that drew it in ascending (p, j).  The index holds integers only and is
 *   built on the device (kernels.infonce_bwd: torch's stable sort + searchsorted).  One wave sums a row's list in list order.
 * ------------------------------------------------------------------------------------------ */
int cst_w2v_negatives(uint32_t key, int64_t B, int64_t M, int64_t K, int64_t Kx, int32_t* out, cst_stream stream);
int cst_infonce_fwd(const void* x, const void* y, const int32_t* idx, float inv_temp, float* nll, float* loss, int32_t* counters,
                    float* lse, float* nx, float* ny, int32_t* flags, float* logits_dbg, int64_t N, int64_t KP, int64_t D, int dtype,
                    cst_stream stream);
int cst_infonce_bwd_x(const void* x, const void* y, const int32_t* idx, float inv_temp, const float* lse, const float* nx,
                      const float* ny, const float* gscale, void* dx, float* pairs, int64_t N, int64_t KP, int64_t D, int dtype,
                      cst_stream stream);
int cst_infonce_bwd_y(const void* x, const void* y, const int64_t* perm, const int32_t* offs, const float* pairs, const float* nx,
                      const float* ny, void* dy, int64_t N, int64_t KP, int64_t D, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Gumbel vector quantizer of wav2vec2 pre-training (added at ABI 13 without a bump).  Replaces GumbelVectorQuantizer.forward after its
 * weight_proj (fairseq/modules/gumbel_vector_quantizer.py:148-199): the argmax / scatter one-hot, F.gumbel_softmax(hard = True), the
 * two perplexities and the [N, G V, 1] * vars product, and their autograd.  One wave owns one (row, group); V <= 1024 codes per group.
 *   logits `dtype` [N, G V] contiguous (the weight_proj output); vars `dtype` [G V, d] (the codebook, groups not combined), d % 8 == 0.
 *   Noise of element e = (n G + g) V + v: g_e = -log(-log u), u = ((bits >> 9) + 0.5) 2^-23, bits = the counter hash of (key, e)
 *   (cst_drop_bits) — 23 bits: u is exact in fp32 and never 1; rng.gumbel_uniform_numpy restates u exactly.  noise != NULL (fp32
 *   [N, G, V]) is read instead.
 * cst_gumbel_vq_fwd: k = argmax_v (l_v + g_v) when training, argmax_v l_v otherwise, ties to the lowest index.  Writes q `dtype` [N, G d]
 *   = vars[g V + k] (a copy: exact), idx int32 [N, G], onehot `dtype` [N, G V] (the hard choice; the weight-gradient GEMM's operand),
 *   avg_probs fp32 [G, V] = the mean over rows of softmax(l) (no noise, no tau: :161-163), stats fp32 [2] = (prob_perplexity,
 *   code_perplexity) = sum_g exp(-sum_v a log(a + 1e-7)) over avg_probs and over the frequencies of the RAW logits' argmax (:150-166),
 *   exph fp32 [G] = exp(H_g) of avg_probs.  The sums over rows run as per-workgroup partials (32 rows each) and a second, one-workgroup
 *   launch that adds them in block order: no atomics.  workspace: cst_gumbel_vq_workspace(N, G, V) bytes.  Nothing is kept for backward.
 * cst_gumbel_vq_bwd (training): dl `dtype` [N, G V] = (1 / tau) s~ (gy - sum_v s~ gy) + (1 / N) s (h - sum_v s h), with s~ =
 *   softmax((l + g) / tau) recomputed from the logits and the same noise source, gy `dtype` [N, G, V] = dq . vars^T per group (the
 *   caller's GEMM), s = softmax(l), h_v = -dppl[0] exph[g] (log(a_v + 1e-7) + a_v / (a_v + 1e-7)); dppl: fp32 device scalar, d loss /
 *   d prob_perplexity.  d vars = onehot^T dq per group is the caller's weight-gradient GEMM (dense and exact in the one-hot operand; not
 *   a scatter: code usage is skewed).
 * Refused (CST_ERR_BAD_ARG, nothing launched, nothing touched): null operands, a bad dtype, N / G / V < 1, V > 1024, d not a multiple
 *   of 8, 1 / tau <= 0, vars / q not 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t cst_gumbel_vq_workspace(int64_t N, int64_t G, int64_t V);
int cst_gumbel_vq_fwd(const void* logits, const void* vars, const float* noise, uint32_t key, int training, void* q, int32_t* idx,
                      void* onehot, float* avg_probs, float* stats, float* exph, void* workspace, int64_t N, int64_t G, int64_t V, int64_t d,
                      int dtype, cst_stream stream);
int cst_gumbel_vq_bwd(const void* logits, const float* noise, uint32_t key, float inv_tau, const void* gy, const float* avg_probs,
                      const float* exph, const float* dppl, void* dl, int64_t N, int64_t G, int64_t V, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Contrastive term of TripletSTMTContrastiveCriterion.compute_contrastive
 * (criterions/triplet_st_mt_contrastive.py:154-169): a = audio memory, t = text memory, both [B, M, C] batch-major
 * (M <= 64 slots); c[b,i,j] = cosine(a[b,i], t[b,j]) (fp32, eps 1e-8), logits = c / temp with the AUDIO slot as class
 * dim and target(j) = j;  loss[0] = sum_b sum_j ( logsumexp_i - logits[j][j] )  (overwritten; loss_rows fp32 [B] holds the
 * per-utterance terms, added up in a fixed order).
 * sim fp32 [B,M,M], na/nt fp32 [B,M] (norms) are saved for backward;  bwd: da, dt = gscale[0] * d loss / d a, t.
 * ------------------------------------------------------------------------------------------ */
int cst_contrastive_fwd(const void* a, const void* t, float* loss, float* loss_rows, float* sim, float* na, float* nt,
                        int64_t B, int64_t M, int64_t C, float temp, int dtype, cst_stream stream);
int cst_contrastive_bwd(const void* a, const void* t, const float* sim, const float* na, const float* nt,
                        const float* gscale, void* da, void* dt, int64_t B, int64_t M, int64_t C, float temp,
                        int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer path — replaces FP16Optimizer's flat-copy / unscale / clip / Adam / copy-back chain
 * (optim/fp16_optimizer.py:16-300; utils.py:323-364; optim/adam.py:146-226).
 * ------------------------------------------------------------------------------------------ */
/* out[0] += sum(x^2).  Deterministic (fixed-order two-stage reduction, no atomics): data-parallel replicas must get
 * bit-identical gradient norms.  workspace: cst_sumsq_workspace() bytes. */
int64_t cst_sumsq_workspace(void);
int cst_sumsq(const void* x, int64_t n, float* out, float* workspace, int dtype, cst_stream stream);
/* One fused pass over flat buffers: g = grad * (*grad_scale); Adam (fairseq semantics: bias
 * correction folded into the step size, decoupled weight decay); master fp32 -> model dtype.
 * grad_scale is a DEVICE fp32 scalar (e.g. clip coefficient / sample_size) so no host sync. */
int cst_adam_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, void* model_param,
                  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, const float* grad_scale, int grad_dtype, int param_dtype,
                  cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident incremental decoding — replaces the per-step host loop of
 * fairseq/sequence_generator.py:_generate (:286-541), search.py BeamSearch.step (:109-144), finalize_hypos
 * (:575-696), the incremental self-attention branch of modules/multihead_attention.py:189-293 and
 * reorder_incremental_state (:419-437).  Every kernel reads the step counter from DEVICE memory, so one decode step is
 * a fixed launch sequence (capturable in a hipGraph); the host polls *num_remaining instead of synchronising per step.
 *
 * State (all caller-owned device buffers; bbsz = bsz*beam, L1 = max_len+1, LT = max_len+2):
 *   step int32[1]; tokens int64[2][bbsz][LT], scores f32[2][bbsz][L1], anc int32[2][bbsz][L1]: ping-pong halves, step s
 *   reads half (s & 1) and writes half ((s+1) & 1).  anc[h][j] = cache row holding position j of hypothesis h (the K/V
 *   caches are append-only: row h writes slot [h][s]; a beam reorder moves ancestry entries, not cache contents).
 *   cands_to_ignore u8[bsz][beam], finished u8[bsz], nfinal int32[bsz], num_remaining int32[1];
 *   finalized hypotheses in emission order: fin_tokens int64[bsz][beam][L1], fin_pos f32[bsz][beam][L1] (positional
 *   scores), fin_score f32[bsz][beam] (length-normalised when normalize_scores), fin_len int32[bsz][beam].
 * cst_beam_step: fp32 log-softmax of logits [bbsz, vocab] (/temperature), NaN/pad/unk/min-len/max-len masks, + cumulative
 *   score, top-(2*beam) per sentence, eos finalisation, next active hypotheses, then *step += 1.  beam <= 20.
 *   logits: 16-byte aligned, ld_logits a multiple of 16 bytes and >= vocab rounded up to it (rows are read as vectors).
 *   members = N >= 2 (at most 8, else CST_ERR_BAD_ARG): the step searches the AVERAGE of N models' next-token distributions
 *   (sequence_generator.py EnsembleModel.forward_decoder :806-868): per member lse_n = logsumexp_v(l_n[v] / temperature), then
 *   lp[v] = log(sum_n exp(l_n[v] / temperature - lse_n)) - log N, in fp32 inside the same first kernel (no extra launch; the
 *   per-element maximum over the members is taken out before the exp; -inf in every member stays -inf; a member whose row
 *   has NaN logits or no finite entry makes the row NaN -> -inf, as the reference's stack + logsumexp does).  The
 *   temperature divides every member's logits BEFORE its softmax.  Masks, scores, top-2*beam and bookkeeping are unchanged.
 *   Constraints (ABI 10; both are off in a zero-filled descriptor tail, and a step with both off launches the kernels without them):
 *   no_repeat_ngram = n >= 2 (--no-repeat-ngram-size, sequence_generator.py:_no_repeat_ngram :734-767): with tk[0 .. s] the row's tokens
 *   (tk[0] = eos) and last = tk[s+2-n .. s], every i in [0, s+1-n] with tk[i .. i+n-2] == last makes token tk[i+n-1] -inf.  It is applied
 *   after the NaN / pad / unk / max-len / prefix / min-len masks and before the cumulative score is added, inside the row kernel (an LDS
 *   bitmap built by the workgroup; no extra launch).  n == 1 or n < 0: CST_ERR_BAD_ARG (1 would ban the initial eos for good).
 *   prefix_tokens int64[bsz][prefix_len], padded with `pad` (--prefix-size, :336-347 and _prefix_tokens :543-575): at steps
 *   s < prefix_len, s < max_len, with t = prefix_tokens[sentence][s]: t != pad -> every candidate of the sentence's rows except t becomes
 *   -inf (t keeps its log-probability after the unk penalty); t == pad -> unconstrained; at those steps the min-len mask is applied to NO
 *   row of the batch (the reference's `elif`); t == eos -> the sentence's rows all read the logits, cumulative score and tokens of its
 *   FIRST row and that row is the parent of every candidate (the reference copies the first beam over the others): `beam` identical
 *   hypotheses are finalised.  The buffer is read at every step, so a captured step sees the contents of the moment it runs.
 *   prefix_len > 0 with a null pointer, prefix_len < 0 or > max_len: CST_ERR_BAD_ARG.
 *   Sampling (ABI 11; off in a zero-filled tail, and a step with it off launches exactly the kernels above; search.py Sampling.step
 *   :676-742): sampling != 0 replaces the top-2*beam selection by one DRAW per row, still two launches.  After the masks above, with
 *   q_v = exp(masked log-probability) (not renormalised): sample_topp > 0 keeps, in the order (value descending, token ascending), every
 *   element with less than p of mass in front of it (_sample_topp :630-673; whole mass < p: everything); else sample_topk = k > 0 keeps
 *   the first k of that order; else everything.  Step 0 uses the sentence's first row and draws `beam` tokens with replacement (slots
 *   0 .. beam-1); later steps draw one token per row, and row i continues hypothesis i (no competition between beams; where the
 *   prefix holds eos, every row draws from the first row, which is then the parent).  The draw of (sentence, slot) at step s:
 *     u = (cst_drop_bits32(key, cst_drop_key2(key), (sentence * beam + slot) * (max_len + 1) + s) >> 8) * 2^-24,   key = *sample_key,
 *   token = the smallest kept v with sum of q_w over kept w <= v exceeding u * Z, Z = the kept mass (inverse CDF in vocabulary order).
 *   Its score is its masked log-probability + the row's cumulative score (NOT the renormalised probability); a row without mass yields
 *   (-inf, pad).  The sentence has `beam` candidates: an eos candidate whose slot is not ignored is finalised, the next rows are the
 *   non-eos candidates in slot order followed by the others, which are ignored for good — every slot yields exactly one sample.
 *   sample_key is read from device memory at every step: a captured step draws with the key of the call that replays it.  All sums that
 *   decide the cut or the draw have a fixed order (no floating-point atomics; longest addition chain 64), so a call is reproducible.
 *   sample_topk < 0 or > vocab, sampling with a null sample_key: CST_ERR_BAD_ARG.  Vocabularies beyond the register-resident row
 *   kernels (more than 5 * 512 16-byte vectors per row): CST_ERR_UNSUPPORTED — nothing is launched in either case.
 *   Diverse decoding (ABI 12; both strategies are off in a zero-filled tail, and a step with both off launches exactly the kernels above).
 *   Both act on the rows' sorted top-2*beam lists inside the per-sentence merge kernel: still two launches, every row kernel (wide
 *   vocabularies, ensembles, constraints) unchanged, and everything after the selection — eos handling, finalisation, cands_to_ignore,
 *   the next rows — runs over the resulting 2*beam candidates as before.  The PENALISED value is the cumulative score that is written.
 *   Beam groups (search.py DiverseBeamSearch.step :568-618, Hamming diversity): diverse_groups = G >= 1, mb = beam / G.  Group g owns the
 *   sentence's rows r with r % G == g (lprobs[:, g::G]); the groups are processed in the order g = 0 .. G-1.  A candidate (row r, token
 *   t) of group g has the value
 *     fl(fl(lp + cumulative score of r) + fl(-diverse_strength * count_g(t))),
 *   count_g(t) = the number of candidates selected at this step by the groups 0 .. g-1 of the sentence whose token is t — all 2*mb of
 *   each group, duplicates, eos and -inf candidates included (scatter_add_ :610).  ORDER OF THE ADDITIONS: the reference forms
 *   fl(fl(lp + alpha * count) + score); here the penalty is added to the row kernel's candidate value, which differs by the rounding of
 *   one fp32 addition (at most one ulp of the cumulative score).  The group keeps its top 2*mb of its mb * vocab candidates, ties to the
 *   smaller local_row * vocab + token; its j-th selection is the sentence's candidate j * G + g (the interleave of torch.stack(...,
 *   dim=2) :615-617) with parent row local_row * G + g.  At step 0 every group searches the sentence's first row, which is the recorded
 *   parent (in a decode the rows are equal there).  G == 1 equals plain beam search bit for bit.  The rows' top 2*beam suffice because
 *   diverse_strength >= 0 only lowers values (argument at beam_merge_kernel).  diverse_groups < 0 or > beam, beam % G != 0 (the
 *   reference's ValueError), diverse_strength < 0: CST_ERR_BAD_ARG.
 *   Diverse siblings (search.py DiverseSiblingsSearch.step :765-814): on iff diverse_siblings != 0 — a switch of its own, so that a
 *   zero-filled tail is off although 0 is a legal rate; sibling_rate = R is read only then.  Step 0 is plain beam search; at later steps
 *   the candidate at position p (from 0) of a row's sorted list has the value fl(v - fl((p + 1) * R)), v = fl(lp + cumulative score),
 *   and the sentence's top 2*beam is taken over the beam * 2*beam penalised candidates, ties to the smaller row * 2*beam + p; parent =
 *   the row.  R == 0 equals plain beam search bit for bit.  R < 0 (or NaN): CST_ERR_BAD_ARG.
 *   sampling, diverse_groups > 0 and diverse_siblings != 0 are mutually exclusive (fairseq_task.py:338-350): two of them together are
 *   CST_ERR_BAD_ARG.  Either diverse strategy composes with members, no_repeat_ngram and prefix_tokens (where the step's prefix token is
 *   eos, the parent is the sentence's first row as above).  Nothing is launched on an error.
 *   Ancestry of a finalised hypothesis (a tail field added WITHOUT raising CST_ABI_VERSION: off in a zero-filled tail, and the binding
 *   resolves cst_attn_avg_probs — declared with it — when it loads the library, so a library built before the field fails to load instead
 *   of ignoring it; no other launch, kernel or store): fin_anc != NULL makes the
 *   finalisation that writes fin_tokens / fin_pos also write fin_anc[slot][j] = anc[parent row][j] for j <= s — the cache row that
 *   computed position j of the hypothesis, which is also the row of any other per-step, append-only history (the attention history
 *   cst_attn_avg_probs writes).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;                         /* storage type of logits */
  int64_t bsz, beam, vocab, max_len;
  int64_t pad, unk, eos, min_len;
  float unk_penalty, len_penalty, temperature;
  int normalize_scores;
  const void* logits; int64_t ld_logits;
  int32_t* step;
  int64_t* tokens; float* scores; int32_t* anc;
  uint8_t* cands_to_ignore; uint8_t* finished; int32_t* nfinal; int32_t* num_remaining;
  int64_t* fin_tokens; float* fin_pos; float* fin_score; int32_t* fin_len;
  void* workspace;                   /* cst_beam_workspace(bsz, beam) bytes, 16-byte aligned: per-row candidates + step ticket */
  int64_t members;                   /* checkpoint ensemble (ABI 9): 0 or 1 = the single matrix `logits`; N >= 2 = `logits` and logits_n[0 .. N-2] */
  const void* logits_n[7];           /* members 1 .. N-1: same rows, vocab, ld_logits, dtype and alignment as `logits` */
  float* lprobs_out;                 /* optional, members >= 2: fp32 [bbsz][ld_logits], the combined log-probabilities before the masks */
  int64_t no_repeat_ngram;           /* ABI 10: 0 = off, else n >= 2 */
  const int64_t* prefix_tokens;      /* ABI 10: device [bsz][prefix_len], padded with `pad`; read when prefix_len > 0 */
  int64_t prefix_len;                /* ABI 10: 0 = off, at most max_len */
  int64_t sampling;                  /* ABI 11: 0 = off (beam search), else every row DRAWS its next token */
  int64_t sample_topk;               /* ABI 11: 0 = off, else draw among the k most probable tokens (at most vocab) */
  float sample_topp;                 /* ABI 11: <= 0 = off, else draw from the nucleus of mass p (wins over sample_topk) */
  const uint32_t* sample_key;        /* ABI 11: device [1], the 32-bit key of the draws; read at every step (required when sampling) */
  int64_t diverse_groups;            /* ABI 12: 0 = off, else G >= 1 beam groups (beam % G == 0) */
  float diverse_strength;            /* ABI 12: S >= 0, the Hamming diversity penalty per earlier selection of the token */
  int64_t diverse_siblings;          /* ABI 12: 0 = off, else the sibling penalty below is applied */
  float sibling_rate;                /* ABI 12: R >= 0, read when diverse_siblings != 0 (a negative rate is an error, not "off") */
  int32_t* fin_anc;                  /* optional, device [bsz][beam][L1]: the ancestry row of every finalised hypothesis (NULL = off; see above) */
} cst_beam_desc;
int64_t cst_beam_workspace(int64_t bsz, int64_t beam);
int cst_beam_init(const cst_beam_desc* d, cst_stream stream);
int cst_beam_step(const cst_beam_desc* d, cst_stream stream);
/* Shallow fusion with a target-side language model (sequence_generator.py:318-324; added at ABI 13): cst_beam_step with one more
 * logits matrix, fused inside the same row kernel — still two launches.  lm_logits: the LM's next-token logits of the hypothesis rows,
 * same rows, vocab, ld_logits, dtype and alignment as d->logits.  With lp[v] the model's log-probability (single, or the ensemble's
 * combination; after the temperature):
 *     lm_lp[v] = lm_logits[v] - logsumexp_v(lm_logits)        (NO temperature: the reference normalises the raw LM output)
 *     lp'[v]   = fl(lp[v] + fl(lm_weight * lm_lp[v]))          (the reference's `probs * w`, then `lprobs += probs`)
 * in fp32, and everything cst_beam_step does from the NaN mask on — pad / unk / max-len / prefix / min-len / n-gram masks, cumulative
 * score, top-2*beam or the draw, the merge kernel, the diverse strategies — runs on lp'.  An LM row with a NaN or without a finite entry
 * makes the row NaN -> -inf, as in the reference; where the prefix holds eos the row reads the sentence's first row of lm_logits too.
 * cst_beam_step(d, s) is cst_beam_step_lm(d, NULL, s); f == NULL or f->lm_logits == NULL: off — the kernels and arguments of
 * cst_beam_step.  lprobs_out (optional, 16-byte aligned): fp32 [bbsz][ld_logits], receives lp' before the masks for any number of
 * members (columns >= vocab are undefined); cst_beam_desc.lprobs_out keeps its meaning (the ensemble's lp, without the LM) and its
 * restriction.  lm_logits or lprobs_out not 16-byte aligned, lm_weight not finite: CST_ERR_BAD_ARG.  Nothing is launched on an error. */
typedef struct { const void* lm_logits; float lm_weight; float* lprobs_out; } cst_lm_fusion_desc;
int cst_beam_step_lm(const cst_beam_desc* d, const cst_lm_fusion_desc* f, cst_stream stream);
/* Lexically constrained beam search (search.py LexicallyConstrainedBeamSearch :210-523 with token_generation_constraints.py; added at
 * ABI 13): "these phrases must appear".  Every hypothesis row carries a constraint state, every sentence a table; both live in the
 * workspace of cst_lex_desc.  Still two launches per step: the row kernel rides on the instantiations of no_repeat_ngram / prefix_tokens
 * behind a pointer, the selection is a third rule of the per-sentence merge kernel beside the two diverse ones.
 *   constraints: device int64 [bsz][width], the reference's packed layout (pack_constraints :41-91): per sentence
 *     [count, tokens of constraint 0, 0, tokens of constraint 1, 0, ...], zero-padded.  Read by cst_lex_init only; the caller refills it
 *     before each call.
 *   representation 1 (ordered, OrderedConstraintState :387-506): the state is an index into the concatenated constraints, -1 = root.
 *     advance(t): finished -> stay; t is the next token -> on; the state ends a constraint -> stay, and the ROOT reads endpoints[-1]
 *     (Python's last entry, always true), so a token that does not start the constraints keeps the root; t is the first token of all ->
 *     state 0; else the root.  bank = state + 1.  next tokens: the first token of all if state > 0, and the advancing token if not
 *     finished.  No constraints: finished, bank 0, no next tokens.
 *   representation 2 (unordered, UnorderedConstraintState :202-358 over the trie ConstraintNode :111-199): the state is a trie node plus,
 *     per node, `generated` and `completed` counts.  advance(t): the node's child by t if generated[child] < child.num_constraints; else
 *     back to the root (onto the root's child by t under the same test) and rewind: from the old node upwards, the first node with
 *     terminal > completed gets completed + 1 and the walk ends, every node before it generated - 1.  bank = sum of generated;
 *     finished = every constraint completed, counting the node itself when it is an unfinished terminal; next tokens = the root's
 *     children united with the node's.
 *   cst_lex_init (after cst_beam_init, on every call, outside a captured step): one workgroup per sentence builds the table — the
 *     concatenated sequence + endpoints, or the trie's parent / token / terminal / num_constraints, and nd, the number of DISTINCT
 *     constraint tokens (the reference's len(state.tokens)) — and sets every row's state to the root in both halves of the state pair.
 *   cst_beam_step_lex(d, f, x): x == NULL is cst_beam_step_lm(d, f): the same kernels and arguments.  Else, at step s, per sentence:
 *     1. eos ban (:308-321): at s > 0 a row whose state is not finished gets lp[eos] = -inf, after every mask of cst_beam_step (NaN, pad,
 *        unk, max-len, min-len, n-gram) and before the cumulative score is added; not at step 0.
 *     2. the list L (:332-357, :398-414): the sentence's plain top 2*beam (value descending, ties to the smaller flat index); at s > 0 each
 *        row's own best candidate in row order; then per row in row order (only the first row at s = 0) one candidate per next token of
 *        the row's state in ascending token order, value fl(lp_masked[t] + cumulative score) — formed by the same operations as a list
 *        entry, so a duplicate is bit-equal to its twin.
 *     3. (:425-449) bank = the bank of advance(parent's state, token); key = fl(float((nd - bank) * -100) + value) in fp32; L is ordered
 *        by that fp32 key, descending, stably.  (Not a lexicographic (bank, value) order: scores below -100 and sub-ulp gaps differ.)
 *     4. (:451-478) a candidate whose predecessor in that order has the same (parent, token) is dropped — cyclically: the first is
 *        compared with the last; adjacent duplicates only.
 *     5. (:480-521) the j-th survivor (from 0) of a run of equal banks gets the stripe nd - bank + j * (survivors + 1); a stable ascending
 *        sort by stripe, the first 2*beam are the sentence's candidates (score = value, token, parent).
 *     6. the eos / finalize / next-row bookkeeping of cst_beam_step over those; next row i takes the advanced state of its candidate
 *        (update_constraints :254-260), written into the other half of the state pair.
 *     A sentence without constraints goes through the same rule and comes out as plain beam search.  A sentence whose constraints cannot
 *     be met within max_len never finalises anything (all its last-step candidates are -inf): nfinal stays 0, `finished` 0.
 *   Limits: at most 32 constraint tokens per sentence, i.e. width <= 65 — beyond: CST_ERR_UNSUPPORTED; at most 16 next tokens per state
 *     (the caller checks both on the host: tokens past the limits are not read).  representation outside {1, 2}, a null or unaligned
 *     workspace, width < 1, sampling / diverse_groups / diverse_siblings set in d, prefix_len > 0: CST_ERR_BAD_ARG.  Nothing is launched
 *     on an error.  Composes with members, no_repeat_ngram and f. */
typedef struct {
  int64_t representation;            /* 1 ordered, 2 unordered */
  const int64_t* constraints;        /* device [bsz][width], the packed layout; read by cst_lex_init only */
  int64_t width;
  void* workspace;                   /* cst_lex_workspace(bsz, beam, width) bytes, 16-byte aligned: tables, state pair, next-token candidates */
} cst_lex_desc;
int64_t cst_lex_workspace(int64_t bsz, int64_t beam, int64_t width);
int cst_lex_init(const cst_beam_desc* d, const cst_lex_desc* x, cst_stream stream);
int cst_beam_step_lex(const cst_beam_desc* d, const cst_lm_fusion_desc* f, const cst_lex_desc* x, cst_stream stream);
/* out[h] = scale * embed[tokens[s&1][h][s]] + pos_table[pad_idx + 1 + s], s = *step (models/transformer.py:744-760,
 * sinusoidal_positional_embedding.py:88-95).  embed/out in `dtype`, pos_table fp32 [pos_rows, C]. */
int cst_dec_embed(const int64_t* tokens, const int32_t* step, const void* embed, const float* pos_table, float scale,
                  int64_t pad_idx, void* out, int64_t rows, int64_t C, int64_t max_len, int64_t pos_rows, int dtype,
                  cst_stream stream);
/* Linear layer of one decode step over the hypothesis rows: y[M, N] = act(x[M, K] W[N, K]^T + bias[N]) (+ resid[M, N]) — replaces the
 * F.linear calls of the incremental decoder layer (modules/transformer_layer.py:293-420 at one target position) with a kernel shaped
 * for M = bsz * beam rows: every weight byte is requested within one memory round trip (N/16..N/64 x ceil(M/80) small workgroups,
 * operands global -> MFMA fragments, K split over the four waves and added in wave order: deterministic).  bf16 only;
 * K % 512 == 0; ldx % 8 == 0; x, W 16-byte aligned.  bias / resid may be NULL.  step (optional, device): the launch does nothing
 * once *step > max_len (a captured step replayed past the end of the search). */
int cst_dec_linear(const void* x, const void* W, const void* bias, const void* resid, void* y, int64_t M, int64_t N, int64_t K,
                   int64_t ldx, int64_t ld_resid, int64_t ldy, int act, const int32_t* step, int64_t max_len, int dtype,
                   cst_stream stream);
/* LayerNorm + Linear of one decode step in ONE launch: y = act(LN(x; gamma, beta, eps) W^T + b) (+ resid), the pre-norm sub-blocks of
 * the decoder layer (modules/transformer_layer.py:346-349, :369-372, :403-406).  The caller folds the affine part into the weights
 * once (they are constants while decoding): Wg[n,k] = bf16(W[n,k] gamma[k]);  sg[n] = sum_k Wg[n,k];  sb[n] = sum_k W[n,k] beta[k] +
 * b[n] (fp32 vectors).  The kernel multiplies the raw rows by Wg, gathers every row's sum(x) and sum(x^2) from the operand fragments
 * it loads anyway, and applies  rstd_m (acc - mean_m sg[n]) + sb[n]  in the epilogue.  Same limits as cst_dec_linear. */
int cst_dec_ln_linear(const void* x, const void* Wg, const float* sg, const float* sb, float eps, const void* resid, void* y, int64_t M,
                      int64_t N, int64_t K, int64_t ldx, int64_t ld_resid, int64_t ldy, int act, const int32_t* step, int64_t max_len,
                      int dtype, cst_stream stream);
/* Single-query self-attention at position s = *step: qkv [rows, 3*H*D] (q | k | v of the newest token), caches
 * [rows, L1, H*D]; appends k/v at slot s, attends over positions 0..s through anc (half s & 1), out [rows, H*D].
 * `scale` multiplies QK^T in fp32.  D in {32, 64}. */
int cst_dec_self_attn(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const int32_t* step, void* out,
                      int64_t rows, int64_t H, int64_t D, int64_t max_len, float scale, int dtype, cst_stream stream);
/* Cross attention of one decode step (modules/multihead_attention.py:189-293 with static_kv): q, out [bsz*beam, H*D];
 * kx, vx HEAD-MAJOR [bsz, H, S, D] — the encoder keys / values of a SENTENCE, shared by its beam hypotheses (not replicated);
 * key_padding_mask uint8 [bsz, S] or NULL.  No-op when *step > max_len.  One pass, online softmax; any S.
 * bf16 / D = 64 / beam <= 32 (operands 16-byte aligned): the matrix-core kernel of csrc/attention_fast.inc — the beam rows are one
 * 32-row MFMA block, the four waves of a (sentence, head) workgroup split the keys (32-key tiles, own LDS-DMA rings, no barrier in the
 * loop) and add their (max, sum, output) states in wave order; every other case: a VALU kernel with the same structure. */
int cst_dec_cross_attn(const void* q, const void* kx, const void* vx, const uint8_t* key_padding_mask, void* out,
                       const int32_t* step, int64_t max_len, int64_t bsz, int64_t beam, int64_t H, int64_t D, int64_t S, float scale,
                       int dtype, cst_stream stream);
/* The query projection of that attention and the attention itself as ONE launch (modules/transformer_layer.py:369-372 with
 * normalize_before + multihead_attention.py:189-207): x [bsz*beam, H*D] (row stride ldx) is the decoder's residual stream in front of
 * encoder_attn_layer_norm; Wg / sg / sb / eps are cst_dec_ln_linear's folded operands of q_proj (fp32 [H*D] vectors; Wg = bf16(W gamma),
 * [H*D, K = H*D]) with Wg stored FRAGMENT-MAJOR — element (n, k) at  ((((n / 64) * 2 + n % 64 / 32) * (K / 16) + k / 16) * 64 +
 * 32 * (k / 8 % 2) + n % 32) * 8 + k % 8  — so that a wave's load of one MFMA operand is one contiguous KiB (the weights are constants
 * while decoding: packed once; Python: Wg.view(H, 2, 32, K/16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous()).  The
 * workgroup of (sentence, head) forms its own 64 query columns for the sentence's beam rows while its first K / V tiles stream in, rounds
 * them to bf16 as the stored q of the two-launch path is, and attends as cst_dec_cross_attn does.  bf16, D = 64, beam <= 32, (H*D) % 256 == 0. */
int cst_dec_ln_q_cross_attn(const void* x, int64_t ldx, const void* Wg, const float* sg, const float* sb, float eps, const void* kx, const void* vx,
                            const uint8_t* key_padding_mask, void* out, const int32_t* step, int64_t max_len, int64_t bsz, int64_t beam, int64_t H,
                            int64_t D, int64_t S, float scale, int dtype, cst_stream stream);

/* Head-averaged attention probabilities — the `attn` the reference's decoder returns for alignment: the weights of
 * modules/multihead_attention.py:334-362 averaged over the heads (models/transformer.py:808-812 with alignment_heads = None), which
 * the fused attention kernels never materialise:
 *   out(b, t)[j] (+)= out_scale * (1/H) * sum_{h = 0 .. H-1} softmax_j(scale * <q[b,t,h,:], k[b,h,j,:]>),   j in [0, S).
 * q: [B*Tq, H*D] in `dtype`, row stride ldq (elements).  k in `dtype`, element (b, h, j, 0) at k + b*k_sb + h*k_sh + j*k_st with D
 * contiguous elements behind it: row-major [B, S, H*D] is (S*H*D, D, H*D), head-major [B, H, S, D] is (H*S*D, S*D, D).
 * key_padding_mask: uint8 [B, S] or NULL; a masked key has probability exactly 0.  out: fp32; the row of (b, t) starts at
 * out + (b*Tq + t) * out_row_stride, + *step * S when `step` (device int32, optional) is given, and then the launch does nothing once
 * *step > max_len, like every launch of a captured decode step (max_len is not read without step).  accumulate != 0 adds to what is
 * there (the members of an ensemble, one after the other on one stream, with out_scale = 1/N); else the S entries are overwritten.
 * Scores, maxima, exponentials, sums and the head sum are fp32; the heads are added in the order h = 0 .. H-1 by one thread per
 * (row, key) — no floating-point atomics, so a call is bit-reproducible.  One launch, two passes over the keys: the (maximum, sum) of
 * every (row, head), then the probabilities (the scores are recomputed, never stored: any S).  VALU arithmetic for every shape.
 * DIFFERENCE to the reference: in a bf16 model it rounds every head's probabilities to bf16 before averaging
 * (attn_weights_float.type_as); here the fp32 probabilities are averaged.  A row whose keys are ALL masked writes zeros where the
 * reference yields NaN; real input always has a valid key.
 * D in {32, 64}; any S >= 1, Tq >= 1; H*D <= 16384.  A null q / k / out, q, k or out not 16-byte aligned, ldq or a k stride not a
 * multiple of 16 bytes, out_row_stride < S, a bad D or dtype: CST_ERR_BAD_ARG, nothing is launched. */
int cst_attn_avg_probs(const void* q, int64_t ldq, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_st, const uint8_t* key_padding_mask,
                       float* out, int64_t out_row_stride, const int32_t* step, int64_t max_len, int64_t B, int64_t Tq, int64_t H, int64_t D,
                       int64_t S, float scale, float out_scale, int accumulate, int dtype, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Filter banks of collated 16 kHz audio — replaces the per-utterance host feature extraction of the fbank-input route:
 *   get_features_or_waveform -> get_features_from_npy_or_audio -> get_fbank
 *                                             fairseq/data/audio/speech_to_text_dataset.py:143-147
 *   torchaudio.compliance.kaldi.fbank(wave, num_mel_bins=80, sample_frequency=16000)
 *                                             fairseq/data/audio/audio_utils.py:80-93 (input x 2^15, no dither)
 * and the transforms __getitem__ applies to its result (speech_to_text_dataset.py:310-312, CompositeAudioFeatureTransform):
 *   utterance_cmvn  feature_transforms/utterance_cmvn.py:26-37   global_cmvn  feature_transforms/global_cmvn.py:20-23
 *   specaugment     feature_transforms/specaugment.py:79-133 (masks only: the intervals are drawn on the host; no time warp)
 * wave: fp32 [B, S] (row stride S), samples in [-1, 1); n_samples: int64 [B] on the device (clamped to S).  T_i = 1 + (n_i - 400)
 * / 160 frames (0 below 400 samples).  out: fp32 [B, T, 80], 16-byte aligned; rows t >= T_i are 0 (T should be max T_i; frames
 * beyond T are not computed).  n_frames: int64 [B] (optional) receives T_i.
 * Transforms, applied in this order: CMVN — utterance_cmvn (norm_means / norm_vars) and global_cmvn (global_mean / global_std fp32
 * [80], NULL = absent), global first when global_first — then SpecAugment when `specaugment`: cells of the frequency intervals
 * fmask int32 [B][n_fmask][2] = (f0, width) and the time intervals tmask int32 [B][n_tmask][2] = (t0, width) (width 0 = no mask,
 * at most 8 of each) take mask_value, or the mean of the spectrogram entering SpecAugment when mask_mean.  Utterance statistics
 * are per-tile partial sums (fp64) reduced by a second launch in a fixed order: bit-reproducible.  workspace (8-byte aligned,
 * cst_fbank_workspace_bytes(B, T) bytes) is needed when any transform is configured; without one, one launch writes `out`.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int64_t B, S, T;
  const float* wave;
  const int64_t* n_samples;
  float* out;
  int64_t* n_frames;
  int utterance_cmvn, norm_means, norm_vars;
  const float* global_mean;
  const float* global_std;
  int global_first;
  int specaugment;
  int n_fmask, n_tmask;
  const int32_t* fmask;
  const int32_t* tmask;
  int mask_mean;
  float mask_value;
  void* workspace;
  int64_t workspace_bytes;
} cst_fbank_desc;
int64_t cst_fbank_workspace_bytes(int64_t B, int64_t T);
int cst_fbank(const cst_fbank_desc* d, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Host-side (CPU) natives of the input pipeline — no device work, no stream.
 * cst_batch_by_size replaces the Cython batch_by_size_fast (fairseq/data/data_utils_fast.pyx:17-67): num_tokens[i] is
 *   the size of the i-th sample IN BATCHING ORDER; batches are consecutive runs of that order; batch_sizes (capacity n)
 *   receives their lengths; returns the number of batches, or a negative cst_status (a sample above max_tokens).
 *   max_tokens / max_sentences <= 0 mean "no limit"; bsz_mult = required_batch_size_multiple.
 * cst_wav_info / cst_wav_read_f32 replace soundfile.read(path, dtype="float32", start=, frames=) for 16-bit PCM WAV
 *   (fairseq/data/audio/audio_utils.py:7-55): samples / 32768 as float32, interleaved if multi-channel; nframes < 0 =
 *   to the end; returns frames read or a negative cst_status.  cst_wav_info returns CST_ERR_UNSUPPORTED for non-PCM16.
 * cst_edit_distance replaces editdistance.eval in the CTC criterion's validation (fairseq/criterions/ctc.py:150-170): the Levenshtein
 *   distance (insert / delete / substitute, cost 1 each) of two int64 sequences — letters or words mapped to ids by the caller; a or b
 *   may be NULL when its length is 0; returns the distance or a negative cst_status (a negative length).  O(na nb) time, O(min) space.
 * ------------------------------------------------------------------------------------------ */
int64_t cst_batch_by_size(const int64_t* num_tokens, int64_t n, int64_t max_tokens, int64_t max_sentences, int32_t bsz_mult,
                          int64_t* batch_sizes);
int cst_wav_info(const char* path, int32_t* sample_rate, int32_t* channels, int64_t* frames, int32_t* bits);
int64_t cst_wav_read_f32(const char* path, int64_t start_frame, int64_t nframes, float* out, int64_t capacity_samples);
int64_t cst_edit_distance(const int64_t* a, int64_t na, const int64_t* b, int64_t nb);

/* ------------------------------------------------------------------------------------------
 * Device batch assembly for the `translation` task (added at ABI 13 without a bump, as cst_score_tokens' successors were: a pure
 * addition).  Replaces LanguagePairDataset.collater on a device-resident binarised corpus: collate() of
 * fairseq/data/language_pair_dataset.py:16-126 over data_utils.py collate_tokens :34-64.
 *   src_stream / tgt_stream: the token streams of the split's two .bin files as stored, both of type tok_dtype.
 *   src_offsets / tgt_offsets: int64 [n_sentences + 1] ELEMENT offsets; sentence i is stream[off[i] .. off[i + 1]).  The caller
 *     guarantees they are non-decreasing and end at the stream's length (the binding checks this once, at upload).
 *   idx: int64 [B] sentence indices in the batch's row order (the collater's descending-source-length order is the caller's).
 *   out: int64 [B*S + 2*B*T + B], 16-byte aligned = src_tokens [B, S] | prev_output_tokens [B, T] | target [B, T] | src_lengths [B].
 *     Every word is written, padding included: pad outside a sentence, on the left of it when the side's left_pad flag is set;
 *     prev_output_tokens is the target with eos moved to the front (eos, t[0], .., t[n - 2]).  S / T are the caller's widths (at
 *     least the batch's longest sentence — rounded up for --required-seq-len-multiple; a longer sentence is truncated to the width).
 *   An idx outside [0, n_sentences) gives an all-pad row and length 0 and reads no token.
 * One launch, no atomics, every word a pure function of its index: bit-reproducible.  Token loads are one element wide (sentences
 * start at any element offset); stores are 16 bytes.
 * A null operand, a bad tok_dtype, B / S / T / n_sentences < 1, B * (S + 2T + 1) > 2^31, a misaligned out or stream: CST_ERR_BAD_ARG,
 * nothing is launched.
 * ------------------------------------------------------------------------------------------ */
typedef enum { CST_TOK_U8 = 0, CST_TOK_U16 = 1, CST_TOK_I32 = 2, CST_TOK_I64 = 3 } cst_tok_dtype;
int cst_collate_pairs(const void* src_stream, const void* tgt_stream, int tok_dtype, const int64_t* src_offsets,
                      const int64_t* tgt_offsets, int64_t n_sentences, const int64_t* idx, int64_t B, int64_t S, int64_t T, int64_t pad,
                      int64_t eos, int left_pad_source, int left_pad_target, int64_t* out, cst_stream stream);

/* ------------------------------------------------------------------------------------------
 * Token blocks of the `language_modeling` task (added at ABI 13 without a bump: pure additions).
 *
 * Host natives (no device work, no stream) — they replace the reference's Cython token_block_utils_fast
 * (_get_slice_indices_fast and _get_block_to_dataset_index_fast, called by TokenBlockDataset.__init__,
 * fairseq/data/token_block_dataset.py:78-100):
 * cst_token_block_slices cuts a corpus of n sentences of sizes[i] tokens into blocks; slices_out (capacity `capacity` blocks,
 *   int64 [.., 2]) receives per block (first stream element, one past the last); returns the block count or a negative cst_status.
 *   slices_out = NULL returns the count only.  break_mode:
 *     CST_BREAK_NONE          ceil(total / block_size) equal blocks of block_size tokens, the last one short;
 *     CST_BREAK_COMPLETE      whole sentences, greedily, up to block_size; a sentence longer than block_size is a block of its own;
 *     CST_BREAK_COMPLETE_DOC  as COMPLETE, and a sentence of exactly document_sep_len tokens ends the document: the block before it
 *                             is closed, its own tokens belong to no block; blocks of <= 1 token are dropped;
 *     CST_BREAK_EOS           one block per sentence (block_size is not read).
 *   sizes NULL, n < 1, a negative size, block_size < 1 in a mode that reads it, an unknown mode: CST_ERR_BAD_ARG; more blocks than
 *   `capacity`: CST_ERR_WORKSPACE.
 * cst_token_block_index writes, per block, out[3 i ..] = (index of the sentence holding the block's first token, the offset of that
 *   token inside the sentence, index of the sentence holding the block's last token); an empty block ends in its first sentence.
 *   Slices must lie inside the corpus and sentences must not be empty (the reference asserts the same): CST_ERR_BAD_ARG otherwise.
 *
 * cst_collate_blocks replaces MonolingualDataset.collater over TokenBlockDataset.__getitem__ on a device-resident binarised corpus
 * (fairseq/data/monolingual_dataset.py:12-53 collate, data_utils.py collate_tokens :34-64, token_block_dataset.py:121-149: the
 * "future" target and its right-shifted source):
 *   stream: the split's ONE token stream as stored, of type tok_dtype.
 *   blocks: int64 [n_blocks, 3] = (first stream element, length, prev).  prev is the stream element whose token precedes the block in
 *     its source row — start - 1 when the block begins inside a sentence — or negative when the block begins at a sentence's first
 *     token: the source row then starts with `eos`, the DICTIONARY's, whatever token ends the sentence before
 *     (token_block_dataset.py:137-138).  The caller guarantees that start, start + length and prev lie inside the stream.
 *   idx: int64 [B] block indices in row order.
 *   out: int64 [2*B*T + B], 16-byte aligned = src_tokens [B, T] | target [B, T] | src_lengths [B].  With n = min(length, T):
 *     target[b, j] = stream[start + j] for j < n;  src_tokens[b, 0] = eos or stream[prev];  src_tokens[b, j] = stream[start + j - 1]
 *     for 1 <= j < n;  pad beyond n (right padding only);  src_lengths[b] = n.  Every word is written.
 *   An idx outside [0, n_blocks) gives an all-pad row and length 0 and reads no token.
 * One launch, no atomics, every word a pure function of its index: bit-reproducible.  Token loads are one element wide; stores are
 * 16 bytes, the lone last word of an odd total is stored alone.
 * A null operand, a bad tok_dtype, B / T / n_blocks < 1, B * (2T + 1) > 2^31, a misaligned out or stream: CST_ERR_BAD_ARG, nothing
 * is launched.
 * ------------------------------------------------------------------------------------------ */
typedef enum { CST_BREAK_NONE = 0, CST_BREAK_COMPLETE = 1, CST_BREAK_COMPLETE_DOC = 2, CST_BREAK_EOS = 3 } cst_break_mode;
int64_t cst_token_block_slices(const int64_t* sizes, int64_t n, int break_mode, int64_t block_size, int64_t document_sep_len,
                               int64_t* slices_out, int64_t capacity);
int cst_token_block_index(const int64_t* sizes, int64_t n, const int64_t* slices, int64_t n_blocks, int64_t* out);
int cst_collate_blocks(const void* stream_tokens, int tok_dtype, const int64_t* blocks, int64_t n_blocks, const int64_t* idx, int64_t B,
                       int64_t T, int64_t pad, int64_t eos, int64_t* out, cst_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CST_H */
