/*
 * ergm_hip.h — C-ABI of libergm_hip.so, the MI355X (gfx950) implementation of ERGM's fused GPT-2
 * training step (LovesickPatience/ERGM src/model.py + the src/main.py train step).
 *
 * Every entry point is `extern "C"`, takes plain pointers + sizes + an explicit hipStream_t
 * (passed as void*), never allocates on the hot path (the caller passes workspace), never frees or
 * retains caller memory, and returns 0 (ERGM_OK) or a negative ergm_status.  A thread-local
 * message is kept for the last error (ergm_last_error).  All calls are asynchronous on `stream`,
 * re-entrant and callable from any host thread (PyTorch's autograd worker thread included).
 *
 * Which reference interface each entry replaces (paths relative to /root/reference):
 *   ergm_gemm             transformers Conv1D.forward (addmm, W stored [in,out]) used at
 *                         src/model.py:95-99,257-258 and its autograd backward (dX = dY·Wᵀ,
 *                         dW = Xᵀ·dY); nn.Linear lm_head (src/model.py:605,698)
 *   ergm_attn_fwd         GPT2Attention._attn src/model.py:119-148 (+ _split_heads/_merge_heads
 *                         :190-198 folded into addressing)
 *   ergm_attn_bwd         autograd backward of the same
 *   ergm_layernorm_fwd    nn.LayerNorm (src/model.py:276,278,282,392; applied :298,318,332,578)
 *   ergm_layernorm_bwd    its autograd backward
 *   ergm_embed_fwd        wte/wpe lookups + visual/audio injection + token-type add
 *                         (src/model.py:459-463,495-504)
 *   ergm_embed_bwd        Embedding backward into the tied wte / wpe
 *   ergm_xent_fwd_bwd     CrossEntropyLoss(ignore_index=-100) on shifted logits (src/model.py:704-708)
 *   ergm_emotion_head     emotion_head + its CrossEntropyLoss (src/model.py:700-701,710-711)
 *   ergm_adamw_step       torch.optim.AdamW.step (src/main.py:68,155)
 *   ergm_attn_decode, ergm_embed_rows, ergm_topp_sample,
 *   ergm_attn_fwd_ragged, ergm_embed_packed, ergm_rows_to_slots, ergm_topp_sample_rows
 *   ergm_attn_fwd_extend, ergm_rows_to_slots_at, ergm_decode_extend (later additions, same version)
 *   ergm_sample_rows, ergm_sample_mark, ergm_decode_run_slots_sampled (per-request sampling controls, same version)
 *                         the per-token work of nucleus_sampling (src/main.py:253-282), for a batch
 *   ergm_beam_select, ergm_beam_gather, ergm_decode_run_beams (same version)
 *                         beam search over the same caches: the cache reordering of _reorder_cache
 *                         (src/model.py:739-746) and the ranking in front of it, on the device
 *   ergm_logit_rules_apply, ergm_hist_write, ergm_hist_append, ergm_hist_follow, ergm_decode_set_rules (same version)
 *                         no_repeat_ngram_size and bad_words_ids of generation, over a token history on the device
 *   ergm_session_bytes, ergm_session_header, ergm_slots_save, ergm_slots_load (same version)
 *                         no counterpart: a conversation's cache and sampler state leave and re-enter a slot
 *   ergm_linear_rows      Conv1D / lm_head for the few rows of a decode step, with the nn.LayerNorm in front
 *                         of it (src/model.py:298,318,332) computed in the same launch
 *   ergm_decode_*         the token loop of nucleus_sampling (src/main.py:253-282) for a batch, after the
 *                         prompt: one native launch sequence per step and per chunk of samples
 *   ergm_model_*          the whole GPT2LMHeadModel.forward (src/model.py:654-737) and its
 *                         backward (src/main.py:154) as one native launch sequence
 */
#ifndef ERGM_HIP_H
#define ERGM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ERGM_ABI_VERSION 14  /* 14: ergm_gemm_plan, ergm_gemm_cfg_count (the planning query) */

typedef enum {
    ERGM_OK = 0,
    ERGM_EINVAL = -1,        /* bad shape / stride / dtype / alignment / null pointer */
    ERGM_EUNSUPPORTED = -2,  /* valid request this build does not implement */
    ERGM_EHIP = -3,          /* HIP launch / runtime failure (hipError_t in the message) */
} ergm_status;

/* Dropout (nn.Dropout of the reference model in training mode: attention probabilities
 * src/model.py:142, attention / cross-attention resid_dropout :245, MLP dropout :266, embedding
 * dropout :506; p = GPT2Config attn_pdrop / resid_pdrop / embd_pdrop, 0.1 for the "gpt2" checkpoint
 * src/main.py:62).  The keep decision of element (row, col) of a dropout site is a pure function of
 * (seed, offset, site, row0 + row, col): Philox4x32-10 with key = seed and counter =
 * {g mod 2^32, g >> 32, site, offset}, g = (row0 + row)·ceil(cols/4) + col/4; the element takes word
 * (col mod 4) and is dropped iff that word < round(p·2^32); kept elements are scaled by 1/(1-p).
 * Backward passes recompute the elementwise sites' bits; the attention forward stores its keep bits
 * (1 bit per probability, ergm_attn_fwd) for the backward.  For the elementwise sites rows are
 * tokens (b·S + s) and cols = n_embd; for attention probabilities rows are (b·H + h)·Sq + q and
 * cols = Sk.  p = 0 or a NULL descriptor: no dropout.                                               */
typedef struct {
    uint64_t seed;
    uint32_t offset;   /* forward number: every training forward draws fresh masks */
    uint32_t site;     /* which nn.Dropout: ergm_drop_site */
    float p;           /* drop probability, [0, 1) */
    int64_t row0;      /* global row of the caller's row 0 (data-parallel ranks, batch slices) */
} ergm_dropout;

/* Site numbering of the executor (L blocks): 0 = embedding dropout; 3l+1 / 3l+2 / 3l+3 = the
 * attention / cross-attention / MLP residual-branch dropout of block l (the residual-stream tensor
 * they produce); 3L+1+2l / 3L+2+2l = attention / cross-attention probabilities of block l. */
#define ERGM_DROP_SITE_EMBD 0u
#define ERGM_DROP_SITE_RESID(l, k) (3u * (uint32_t)(l) + 1u + (uint32_t)(k)) /* k: 0 attn, 1 cross, 2 mlp */
#define ERGM_DROP_SITE_ATTN(L, l, cross) (3u * (uint32_t)(L) + 1u + 2u * (uint32_t)(l) + ((cross) ? 1u : 0u))

/* The keep mask itself: bits[r][w], ceil(cols/32) words per row, bit j of word w = element
 * (r, 32w + j) kept (pad bits 0).  Tests replay these masks through the CPU oracle.               */
int ergm_dropout_mask(const ergm_dropout* d, int rows, int cols, uint32_t* bits, void* stream);
/* x[r][c] = keep ? x·1/(1-p) : 0, in place (f32, row stride ld; cols, ld multiples of 4). */
int ergm_dropout_apply(const ergm_dropout* d, float* x, int rows, int cols, int ld, void* stream);

typedef enum { ERGM_F32 = 0, ERGM_BF16 = 1 } ergm_dtype;

/* Operand storage layouts (row-major storage, leading dimension in elements).
 *   A: ERGM_MK = A[m][k] (k contiguous)   ERGM_KM = A[k][m] (m contiguous)
 *   B: ERGM_NK = B[n][k] (nn.Linear weight, k contiguous)
 *      ERGM_KN = B[k][n] (Conv1D weight [in,out], n contiguous)                    */
typedef enum { ERGM_MK = 0, ERGM_KM = 1 } ergm_a_layout;
typedef enum { ERGM_NK = 0, ERGM_KN = 1 } ergm_b_layout;

/* Epilogues applied to v = alpha * (A·B)[m][n] (all math fp32):
 *   NONE        C = v
 *   BIAS        C = v + bias[n]
 *   BIAS_GELU   C = gelu_new(v + bias[n]); aux_out[m][n] = bf16(gelu_new'(v + bias[n])) (the
 *               derivative the backward multiplies by)
 *   BIAS_RESID  C(f32) = aux[m][n](f32) + drop(v + bias[n])      (residual add; aux may == C;
 *               drop = the optional `dropout` site over [M][N], identity when NULL)
 *   GELU_BWD    C = v * aux[m][n] with aux = the bf16 gelu_new' that BIAS_GELU stored
 *   ACCUM       C(f32) = C + v                                   (beta = 1 accumulation)          */
typedef enum {
    ERGM_EPI_NONE = 0,
    ERGM_EPI_BIAS = 1,
    ERGM_EPI_BIAS_GELU = 2,
    ERGM_EPI_BIAS_RESID = 3,
    ERGM_EPI_GELU_BWD = 4,
    ERGM_EPI_ACCUM = 5,
} ergm_epilogue;

typedef struct {
    int M, N, K;
    int lda, ldb, ldc;
    int a_layout;   /* ergm_a_layout */
    int b_layout;   /* ergm_b_layout */
    int c_dtype;    /* ergm_dtype of C (A and B are bf16) */
    int epilogue;   /* ergm_epilogue */
    float alpha;
    const float* bias;   /* [N] f32 or NULL */
    const void* aux;     /* epilogue input: f32 residual [M][ld_aux] or bf16 gelu' */
    int ld_aux;
    void* aux_out;       /* epilogue second output (bf16 gelu' of the pre-activation) [M][ld_aux_out] */
    int ld_aux_out;
    int split_k;         /* 0 = choose automatically, 1 = none, >1 = forced split count */
    const float* alpha_dev;  /* optional device scalar multiplied into alpha (autograd grad_output) */
    const ergm_dropout* dropout;  /* BIAS_RESID only: residual-branch dropout (rows m, cols n); NULL = none */
    float* bias_grad;    /* a_layout KM + b_layout KN (a weight gradient Xᵀ·dY), epilogue NONE, f32 C only:
                          * also write alpha·Σ_k B[k][n] (the Conv1D bias gradient, column sums of dY over
                          * the K tokens) to bias_grad[n], f32 [N]; NULL = none.  Computed from the B
                          * fragments the GEMM already stages (no second pass over dY), deterministic. */
    /* Extents in device memory (ABI 12; all NULL by default; b_layout KN, epilogue NONE, f32 C, no bias_grad).  M
     * and K are then capacities: the grid and the split-K workspace are sized for them on the host, and the
     * kernels read the extents when they run (nothing waits inside a kernel).
     *   m_count_dev  int*: only rows m < min(M, *m_count_dev) are computed and stored; a tile whose first row lies
     *                past the count returns at once.  Rows of A at or past the count are never used.
     *   k_count_dev  int*: the contraction runs over k < *k_count_dev, a multiple of 64 no larger than K rounded
     *                up to 64 (A and B must hold that many k rows/columns); 0 writes C = 0.  Never split.
     *   row_map      int[M]: computed row m is stored to row row_map[m] of C (rows of C no row maps to are not
     *                written).  Entries at or past the row count are not read.                                */
    const int* m_count_dev;
    const int* k_count_dev;
    const int* row_map;
} ergm_gemm_desc;

/* Tuning hook (calling thread only): force pipelined-kernel configuration `cfg` (tile / wave grid /
 * LDS stages, see kCfgs in ergm_amd/csrc/gemm.hip) and split-K count for later ergm_gemm calls;
 * cfg = -1 restores the automatic choice.  Used by tools/gemm_tune.py.                          */
int ergm_gemm_tune(int cfg, int split);
/* Per-shape override of the automatic choice: GEMMs of exactly (M, N, K, a_layout, b_layout) with
 * split_k == 0 use configuration `cfg` and `split`; cfg = -1 removes the entry.  Process-wide, set
 * before the plans that use it are created (their workspace is sized then).  ergm_gemm_trace(on,
 * shapes, max) records the distinct shapes of later ergm_gemm calls (on = 1 starts a new record) and
 * returns how many were recorded so far, copying up to `max` of them as 5 ints (M, N, K, layouts).
 * Both serve tools/step_tune.py, which measures configurations inside the running training step. */
int ergm_gemm_set_override(int M, int N, int K, int a_layout, int b_layout, int cfg, int split);
int ergm_gemm_trace(int on, int* shapes, int max_shapes);
/* Workspace bytes ergm_gemm needs for `desc` (split-K partial slabs); 0 if none. */
size_t ergm_gemm_workspace_size(const ergm_gemm_desc* desc);
int ergm_gemm(const ergm_gemm_desc* desc, const void* A, const void* B, void* C, void* workspace,
              size_t ws_bytes, void* stream);
/* Planning query (ABI 14, host only: works without a GPU, launches nothing, leaves the shape trace as it is).
 * Reports what ergm_gemm would run for `desc` right now, the calling thread's ergm_gemm_tune setting and the
 * override tables included: *cfg = the index into kCfgs, or -1 for the register-staged kernel; *split = the
 * effective split-K count after rounding the slices to whole 64-deep K steps; *flags bit 0 = the bias gradient
 * is summed inside the GEMM kernel (else by the column-sum pass behind it), bit 1 = one K slice per XCD, bit 2 =
 * the path with device-side extents.  The descriptor's shape, layout and epilogue fields are checked as ergm_gemm
 * checks them (ERGM_EINVAL); no operand pointer is needed, and the device pointers inside `desc` are only tested for NULL.
 * ergm_gemm_cfg_count returns the number of entries of kCfgs (the bound of ergm_gemm_tune's cfg).             */
int ergm_gemm_plan(const ergm_gemm_desc* desc, int* cfg, int* split, int* flags);
int ergm_gemm_cfg_count(void);

/* fp8 GEMM (config 5's forward Conv1D GEMMs; build-side, the reference is fp32):
 *   C = epilogue(alpha · a_scale[m] · b_scale[n] · Σ_k A[m][k]·B[n][k])
 * A [M][lda], B [N][ldb]: OCP e4m3fn bytes, k contiguous (desc->a_layout = ERGM_MK, b_layout =
 * ERGM_NK); K % 128 == 0; lda, ldb multiples of 16.  Runs v_mfma_scale_f32_16x16x128_f8f6f4 (unit
 * block scales; 2x the bf16 MFMA rate).  Epilogues: NONE (f32/bf16 C), BIAS / BIAS_GELU (bf16 C),
 * BIAS_RESID (f32 C).  ergm_gemm_f8_tune forces a tile configuration (-1 = automatic).           */
int ergm_gemm_f8(const ergm_gemm_desc* desc, const void* A, const float* a_scale, const void* B,
                 const float* b_scale, void* C, void* stream);
int ergm_gemm_f8_tune(int cfg);
/* Per-shape tile configuration of the fp8 / MX GEMMs (ergm_gemm_f8, ergm_gemm_mx) keyed on (M, N, K): the in-step
 * tuner's hook (tools/step_tune.py --f8), as ergm_gemm_set_override is for the bf16 GEMMs; cfg -1 removes the entry.
 * ergm_gemm_trace lists these GEMMs with a_layout 16.  ABI 10. */
int ergm_gemm_f8_set_override(int M, int N, int K, int cfg);
/* Row-wise e4m3 quantisation (activations): scale[r] = max_c |X[r][c]| / 448 (1 for a zero row),
 * Q[r][c] = e4m3(clamp(X[r][c] / scale[r], ±448)).  X bf16 or f32 (x_dtype), cols % 8 == 0.       */
int ergm_quant_rows_fp8(const void* X, int x_dtype, int ldx, int rows, int cols, void* Q, int ldq,
                        float* scale, void* stream);
/* Column-wise e4m3 quantisation of a Conv1D weight W [K][ldw] (in, out; f32 or bf16 per w_dtype)
 * into its transpose Wt [N][ldt] (k contiguous, the B operand of ergm_gemm_f8): scale[n] =
 * max_k |W[k][n]| / 448.  amax_ws: N x 4 bytes of workspace.  K, N multiples of 64.             */
int ergm_quant_weight_fp8(const void* W, int w_dtype, int ldw, int K, int N, void* Wt, int ldt,
                          float* scale, void* amax_ws, void* stream);

/* MX-fp8 (OCP microscaling) GEMM, config 5's forward: A [M][lda]
 * and B [N][ldb] e4m3fn bytes (k contiguous),
 * each with an e8m0 scale byte per 32-element K block (a_scale [M][ld_sa], b_scale [N][ld_sb]: 2^(byte-127)),
 *   C = epilogue(alpha · Σ_blocks 2^(ea+eb-254) · Σ_{k in block} A[m][k]·B[n][k])
 * on v_mfma_scale_f32_16x16x128_f8f6f4 with the block scales consumed by the MFMA (no dequantisation pass).
 * Scale layout (every MX scale array of this library): the 4 bytes of one row's 128-deep K step form a word and
 * the words of one K step are contiguous over the rows — byte (row r, block b) at ((b/4)·pitch + r)·4 + b%4, with
 * pitch >= the row count (ld_sa >= M, ld_sb >= N, ld_qs >= M), so a GEMM stage loads its scales as whole lines.
 * K % 128 == 0.  Epilogues as ergm_gemm_f8, plus GELU_BWD (bf16 C,
 * aux = gelu_new').  q_out / q_scale (BIAS_GELU or GELU_BWD, N % 32 == 0): the epilogue also writes the MX copy
 * of its bf16 output, [M][ld_q] e4m3 and
 * [M][ld_qs] e8m0 (the next MX GEMM's A operand).  Tile configurations as ergm_gemm_f8 (ergm_gemm_f8_tune). */
int ergm_gemm_mx(const ergm_gemm_desc* desc, const void* A, const void* a_scale, int ld_sa, const void* B,
                 const void* b_scale, int ld_sb, void* C, void* q_out, void* q_scale, int ld_q, int ld_qs, void* stream);
/* MX-fp8 quantisation of rows (activations): block b of row r = columns 32b..32b+31; e = the smallest integer
 * with max|block| <= 448·2^e (0 for a zero block), scale byte (r, b) = e + 127 in the layout above (pitch lds >=
 * rows), Q[r][c] = e4m3(X[r][c]·2^-e) (exact scaling, round to nearest even, never saturating).  X bf16 or f32
 * (x_dtype), cols % 32 == 0.                                                                                  */
int ergm_quant_rows_mx(const void* X, int x_dtype, int ldx, int rows, int cols, void* Q, int ldq, void* S, int lds,
                       void* stream);
/* MX-fp8 quantisation of a Conv1D weight W [K][ldw] (bf16) into its transpose Wt [N][ldt] (k contiguous) with a
 * scale per (column n, 32-row block): S, pitch lds >= N; same rule as ergm_quant_rows_mx; one pass, no amax pass.
 * Optionally (Wr != NULL) in the same pass the row form — Wr [K][ldr] e4m3 with a scale per (row k, 32-column
 * block), Sr pitch ldsr >= K: the B operand of the data-gradient GEMM dX = dY·Wᵀ.  K, N multiples of 64.       */
int ergm_quant_weight_mx(const void* W, int ldw, int K, int N, void* Wt, int ldt, void* S, int lds, void* Wr, int ldr,
                         void* Sr, int ldsr, void* stream);

/* Fused attention over head_dim = 64, token-major tensors with head h at columns [64h, 64h+64):
 *   Q[b][s][h*64+d] = q + (b*Sq + s)*ldq + h*64 + d     (likewise K/V with Sk rows, O with ldo)
 * out: O (bf16) and lse[b][h][s] = ln Σ_k exp(score) (f32; backward recomputes P from it).
 * `causal`: key j visible to query i iff j <= i (Sq == Sk required). scale = 1/sqrt(64).
 * dropout (optional, p > 0): O = (P∘keep/(1-p))·V with the keep bits of ergm_dropout_mask over rows
 * (b·H + h)·Sq + q and cols Sk (the LSE stays that of the undropped softmax); the forward stores them
 * in keep_bits: u64 [B·H·Sq][ceil(Sk/64)], bit key mod 64 of word key/64 (Sq, Sk <= 1024); the
 * backward reads the same buffer.  NULL / p == 0: no dropout, keep_bits unused.                  */
int ergm_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H,
                  int Sq, int Sk, int ldq, int ldk, int ldv, int ldo, int causal,
                  const ergm_dropout* dropout, void* keep_bits, void* stream);
/* Inference attention over a packed batch of sequences of different lengths, one launch (no dropout; lse optional).
 * Sequence b < n_seq owns query rows q_start[b] .. q_start[b] + q_len[b] - 1 of q [total_q][ldq] and o [total_q][ldo],
 * and key rows k_start[b] .. k_start[b] + k_len[b] - 1 of k / v [total_k][ld]; nothing is padded.  Self-attention of
 * a packed qkv buffer passes the same starts and lengths for both with causal = 1 (k_len[b] == q_len[b]); cross-
 * attention the caption rows' own arrays with causal = 0.  The four arrays are device ints; max_q / max_k are the
 * host's bounds on q_len / k_len (max_q sizes the grid: (ceil(max_q / 64), H, n_seq) workgroups, those past a
 * sequence's last query tile exit at once).  Every value read from the arrays is clamped to [0, max] and to the
 * packed extents before an address is formed, and no row outside a sequence's own query rows is written.  Query
 * tiles are counted from each sequence's first row and run ergm_attn_fwd's tile loop, so the rows of sequence b are
 * bitwise ergm_attn_fwd(B = 1, Sq = q_len[b], Sk = k_len[b]) on that sequence alone.  lse (may be NULL): f32, the
 * [H][q_len[b]] block of sequence b at lse + H·q_start[b].                                                      */
int ergm_attn_fwd_ragged(const void* q, const void* k, const void* v, void* o, float* lse, const int* q_start,
                         const int* q_len, const int* k_start, const int* k_len, int n_seq, int H, int total_q,
                         int total_k, int max_q, int max_k, int ldq, int ldk, int ldv, int ldo, int causal,
                         void* stream);
/* Causal inference attention of packed NEW query rows over caches that already hold a past, one launch (found by
 * symbol; the ABI version is unchanged).  ergm_attn_fwd_ragged's arguments without lse and causal; the mask is aligned
 * to the bottom-right corner: sequence b owns query rows q_start[b] .. q_start[b] + q_len[b] - 1 of q / o and key rows
 * k_start[b] .. k_start[b] + k_len[b] - 1 of k / v with k_len[b] >= q_len[b]; past_b = k_len[b] - q_len[b]; query row s
 * is position past_b + s and sees keys 0 .. past_b + s.  The new rows' own K / V must already be among the key rows
 * (ergm_rows_to_slots_at).  With a layer's slot cache as k / v: k_start[b] = slot_b · max_len, total_k = max_batch ·
 * max_len, ldk = ldv = 2 · n_embd.  Query tiles are counted in absolute positions (tile t = positions 64t .. 64t + 63,
 * a sequence runs tiles past_b / 64 .. ceil(k_len[b] / 64) - 1; grid (ceil(max_q / 64) + 1, H, n_seq)), so that output
 * row s is bitwise row past_b + s of ergm_attn_fwd(B = 1, Sq = Sk = k_len[b], causal = 1) over the sequence alone.
 * Every value read from the arrays is clamped to [0, max] and the packed extents before an address is formed, q_len to
 * k_len, and no row outside a sequence's own query rows is read from q or written to o.                            */
int ergm_attn_fwd_extend(const void* q, const void* k, const void* v, void* o, const int* q_start, const int* q_len,
                         const int* k_start, const int* k_len, int n_seq, int H, int total_q, int total_k, int max_q,
                         int max_k, int ldq, int ldk, int ldv, int ldo, void* stream);
/* delta workspace: B*H*Sq floats.  dq/dk/dv are bf16 with their own leading dims.              */
int ergm_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                  const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int H, int Sq,
                  int Sk, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv,
                  int causal, const ergm_dropout* dropout, const void* keep_bits, void* stream);
/* Path selection hook (tests / tuning): bit 0 of force_generic makes ergm_attn_bwd use the tiled
 * kernels even where the one-workgroup-per-(b,h) kernel applies (Sq, Sk <= 128; the forward is tiled at
 * every length); bits 4-7 select the
 * tiled kernels' LDS ring depth (0 = per-kernel defaults; 2, 3 or 4).  Process-wide; not for concurrent use with
 * running attention calls. */
int ergm_attn_tune(int force_generic);
/* Decode attention (ABI 13; generation, src/main.py:253-282): one query per sequence over a ragged K/V cache.  For
 * b < B, h < H (head_dim 64, scale 1/8, bf16 in, f32 math, bf16 out):
 *   n_b = clamp(lens[b], 0, max_len - append)         (lens: device int [B], read when the kernel runs, never written)
 *   q = qkv[b][64h .. 64h+64)                          (qkv [B][ld_qkv] bf16)
 *   cache row t of sequence b at kcache / vcache + b*ld_seq + t*ld_row, head h at columns [64h, 64h+64); K and V
 *   may interleave in one [max_len][2E] buffer (vcache = kcache + E, ld_row = 2E).
 * append = 0 (cross-attention): out[b] = softmax(q·Kᵀ/8)·V over rows t < n_b of a read-only cache; n_b = 0 writes zeros.
 * append = 1 (self-attention): the new key qkv[b][E + 64h ..) and value qkv[b][2E + 64h ..) are stored, bitwise, to
 * row n_b, and the query attends rows 0 .. n_b, the new row taken from qkv (no workgroup reads another's store).
 * No cache row at or past max_len and no sequence at or past B is read or written, whatever lens holds.
 * splits: the rows t < n_b are cut into `splits` chunks of ceil(n_b / splits) rounded up to 32 rows, one workgroup
 * per (chunk, head, sequence); with splits > 1 the partials (m, l, o[64]: 66 floats per chunk) go through
 * `workspace` (B*H*splits*66 floats) and are merged in chunk order.  0 = automatic (1 when B*H fills the chip),
 * at most 32; ergm_attn_decode_workspace_size covers the automatic choice.  No float atomics: the same inputs give
 * the same bits in every run.  Every stride is a multiple of 8 elements, every pointer 16-byte aligned.        */
size_t ergm_attn_decode_workspace_size(int B, int H, int max_len);
int ergm_attn_decode(const void* qkv, int ld_qkv, void* kcache, void* vcache, int64_t ld_seq, int ld_row,
                     const int* lens, int B, int H, int max_len, int append, int splits, void* out, int ldo,
                     void* workspace, size_t ws_bytes, void* stream);

/* Linear layer for a handful of rows (a decode step: M = the batch, designed for M <= 32; any M >= 1 runs, the
 * weights being streamed once per group of 32 rows), with an optional LayerNorm in front:
 *   C[m][n] = epi( Σ_k A'[m][k]·W[k|n] + bias[n] ),   K % 64 == 0, N % 8 == 0
 *   A' = A, bf16 [M][lda]                                     when ln_gamma == ln_beta == NULL
 *   A' = bf16((x − μ_m)·rstd_m·γ + β), x = A as f32 [M][lda]   when both are given (biased variance and ln_eps as
 *        ergm_layernorm_fwd; mean and variance in fp32 in two passes; the operand is rounded to bf16 once)
 *   W bf16: ERGM_KN [K][ldw] (Conv1D) or ERGM_NK [N][ldw] (nn.Linear, the tied LM head)
 *   epi: NONE (f32 C) | BIAS (bf16 C) | BIAS_GELU (bf16 C = gelu_new, no derivative output) |
 *        BIAS_RESID (f32 C = aux[m][n] + v + bias[n], aux f32 [M][ld_aux], aux may be C); either weight layout.
 * One launch, no workspace (there is no _workspace_size query), no atomics: K is split over the waves of one
 * workgroup per 16-column strip and the partials are summed in a fixed order, so the same inputs give the same bits
 * in every run.  A row's result depends on no other row: row r of a call on M rows equals, bitwise, a call on that
 * row alone.  Rows at or past M are neither read nor written.  lda: a multiple of 8 elements (4 with the LayerNorm),
 * ldw of 8; A, W, ln_gamma, ln_beta 16-byte aligned.  Unsupported arguments: ERGM_EINVAL before any launch.       */
typedef struct {
    int M, N, K;
    int lda, ldw, ldc;
    int w_layout;            /* ergm_b_layout */
    int epilogue;            /* ergm_epilogue: NONE, BIAS, BIAS_GELU or BIAS_RESID */
    const float* bias;       /* [N] f32; NULL only with NONE */
    const float* aux;        /* BIAS_RESID: f32 residual [M][ld_aux] */
    int ld_aux;
    const float* ln_gamma;   /* [K] f32, or NULL: no LayerNorm */
    const float* ln_beta;    /* [K] f32 */
    float ln_eps;
} ergm_linear_rows_desc;
int ergm_linear_rows(const ergm_linear_rows_desc* desc, const void* A, const void* W, void* C, void* stream);

/* LayerNorm over rows of E (biased variance, eps): y(bf16) = (x-μ)·rstd·γ + β; x f32.        */
int ergm_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, float* mean,
                       float* rstd, int rows, int E, float eps, void* stream);
/* dres(f32, in/out) += LN_bwd(dy); dres_bf16 (optional) = bf16(dres), or bf16(dres·keep/(1-p))
 * with `dropout` (rows x E): the gradient of the residual branch whose dropped output was added into
 * this residual-stream tensor; dγ/dβ (f32 [E], written).
 * workspace: ergm_layernorm_bwd_workspace_size(rows, E) bytes.                                  */
size_t ergm_layernorm_bwd_workspace_size(int rows, int E);
int ergm_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                       const float* gamma, float* dres, void* dres_bf16, float* dgamma, float* dbeta,
                       void* workspace, size_t ws_bytes, int rows, int E, const ergm_dropout* dropout,
                       void* stream);

/* The forms of the two calls above that the training step runs.  ergm_layernorm_fwd_ld: y has rows of ldy >= E bf16
 * (ldy % 4 == 0; the columns past E are not written).  ergm_layernorm_bwd_ex: dy is f32 (ERGM_F32) or bf16 (ERGM_BF16,
 * the block LayerNorms' form); dres_bf16 may be NULL; drop_res = 1 (dres_bf16 NULL: the step uses it for the
 * embedding slot only, which has no bf16 consumer) takes the updated dres itself through `dropout`:
 * dres = (dres + LN_bwd(dy))·keep/(1-p).  With ERGM_F32, drop_res = 0 and dres_bf16 given it is ergm_layernorm_bwd
 * bit for bit.                                                                                   */
int ergm_layernorm_fwd_ld(const float* x, const float* gamma, const float* beta, void* y, int ldy, float* mean,
                          float* rstd, int rows, int E, float eps, void* stream);
int ergm_layernorm_bwd_ex(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd,
                          const float* gamma, float* dres, void* dres_bf16, float* dgamma, float* dbeta,
                          void* workspace, size_t ws_bytes, int rows, int E, const ergm_dropout* dropout,
                          int drop_res, void* stream);

/* Column sums of a row-major matrix (bias gradients, wpe gradient): out[c] (=|+=) Σ_r X[r][c]. */
size_t ergm_colsum_workspace_size(int rows, int cols);
int ergm_colsum(const void* X, int x_dtype, int rows, int cols, int ldx, float* out, int accumulate,
                void* workspace, size_t ws_bytes, void* stream);

/* Embedding + fusion (src/model.py:459-463,495-506):
 *   h0[b,s] = drop(((wte[ids] + [s==0]·vis[b] + [s==1]·aud[b]) + wpe[s]) + wte[tt])      (f32)
 *   cap[b,s] = bf16(wte[cap_ids])                       (caption embeddings are not dropped)
 * vis: [B][ld_vis] row b's first E values (imgs[i][0]); vis/aud may be NULL (text-only);
 * tt may be NULL; dropout (rows b·S + s, cols E) may be NULL.                                  */
int ergm_embed_fwd(const int64_t* ids, const int64_t* tt, const int64_t* cap_ids, const float* wte,
                   const float* wpe, const float* vis, int ld_vis, const float* aud, float* h0,
                   void* cap, int B, int S, int E, int V, const ergm_dropout* dropout, void* stream);
/* One token per sequence at its own position (ABI 13; a decode step of B ragged sequences):
 *   h[b] = (wte[ids[b]] + wpe[clamp(pos[b], 0, n_positions-1)]) + wte[tt[b]]            (f32 [B][E])
 * in ergm_embed_fwd's summation order: a row equals that kernel's row for the same token at the same position
 * (positions >= 2, or no features).  pos: device int [B] (the cache lengths).  ids outside [0, V) are clamped, a
 * tt outside it adds nothing (as ergm_embed_fwd), tt may be NULL: no index is ever followed out of a table. */
int ergm_embed_rows(const int64_t* ids, const int64_t* tt, const int* pos, const float* wte, const float* wpe,
                    float* h, int B, int E, int V, int n_positions, void* stream);
/* Nucleus sampling of B logit rows (ABI 13; src/main.py:259-270 without the sort and without a host round trip).
 * logits f32 [B][ldl], the first V columns count (V <= 53,248).  p = softmax(row); rank the tokens by descending p,
 * ties by ascending token id; the token of rank r is kept iff r == 0 or the summed p of the ranks < r is <= top_p
 * (the reference's `cumsum > top_p` shifted right by one).  The draw: u = (w + 0.5) / 2^32 with w = word 0 of
 * Philox4x32-10(counter {b, 0, 0xE5A3, step}, key seed); the token is the first kept token, in ascending token id,
 * whose running sum of kept p reaches u · (the kept mass): the reference's renormalised multinomial in distribution.
 * Arithmetic: e = expf(x - max) in f32, then every sum over the integers floor(e · 2^30), so no result depends on a
 * summation order.  finished (uint8 [B], in/out, may be NULL): a row with a nonzero flag emits eos_id and draws
 * nothing; a row that draws eos_id sets its flag.  tokens int64 [B]; kept (int [B]) and kept_mass (f32 [B], the
 * kept share of the row's probability) are optional outputs, 0 for a finished row.                          */
int ergm_topp_sample(const float* logits, int ldl, int B, int V, float top_p, uint64_t seed, uint32_t step,
                     void* finished, int64_t eos_id, int64_t* tokens, int* kept, float* kept_mass, void* stream);
/* ergm_topp_sample with a Philox counter per row: {row_ids[b], 0, 0xE5A3, row_steps[b]} (device uint32 [B] each), so
 * a row's draws follow the request it serves and the tokens that request has drawn, not the row it happens to occupy.
 * With row_ids = 0 .. B-1 and every row_steps[b] = step every output is bitwise ergm_topp_sample's.               */
int ergm_topp_sample_rows(const float* logits, int ldl, int B, int V, float top_p, uint64_t seed,
                          const uint32_t* row_ids, const uint32_t* row_steps, void* finished, int64_t eos_id,
                          int64_t* tokens, int* kept, float* kept_mass, void* stream);
/* The per-row sampling controls of ergm_sample_rows: device arrays of one value per row [B], any of them NULL for the
 * default of every row, and the bitmap of the tokens each row has seen (uint32 [B][ld_seen], token j = bit j & 31 of
 * word j >> 5, ld_seen >= (V + 31) / 32 words; NULL: no token is penalised and none is recorded).                */
typedef struct {
    const float* top_p;        /* default: the scalar argument */
    const float* temperature;  /* default 1 */
    const float* rep_penalty;  /* default 1 */
    const int* top_k;          /* default 0: off */
    const uint32_t* min_step;  /* default 0: eos may be drawn at once */
    uint32_t* seen;
    int ld_seen;
} ergm_sample_ctl;
/* ergm_topp_sample_rows with sampling controls per row (found by symbol, ABI unchanged).  For row b, x_j =
 * logits[b][j], j < V, in this order (the usual order of logits processors):
 *   1. repetition penalty r = rep_penalty[b]: for every j whose bit is set in seen[b], x_j <- x_j · r if x_j < 0,
 *      else x_j / r;
 *   2. minimum length: while row_steps[b] < min_step[b] the token eos_id holds no mass, is not counted in `kept` and
 *      cannot be drawn;
 *   3. temperature: x_j <- x_j / temperature[b], an f32 IEEE division (temperature = 1 and r = 1 change no bit);
 *   4. masses: e_j = expf(x_j - max_j x_j), q_j = floor(e_j · 2^30), S = sum q_j: ergm_topp_sample's integers;
 *   5. rank: descending value, ties by ascending token id;
 *   6. top-k, k = top_k[b]: with k >= 1 only the ranks < k remain and S_k is their mass; otherwise S_k = S;
 *   7. top-p: rank r is kept iff it remains under top-k and (r == 0 or the mass of the ranks < r is <= T), T from
 *      top_p[b] by ergm_topp_sample's expression with S_k in the place of S: top-p over the renormalised top-k set;
 *   8. the draw: ergm_topp_sample_rows', counter {row_ids[b], 0, 0xE5A3, row_steps[b]}: the first kept token in
 *      ascending id whose running kept mass reaches ceil(u · K), K the kept mass.
 * top_k = 1 is greedy decoding: the arg-max, the lowest id on ties, whatever the seed.  A temperature or penalty that
 * is NaN, infinite or <= 0 acts as 1; top_k <= 0 or >= the number of tokens with mass (q_j > 0) is off; no value
 * makes the kernel follow an index out of a table.  ctl may be NULL: every output is then ergm_topp_sample_rows'.
 * logprob (f32 [B], optional): (x_tok - max) - ln(S · 2^-30), the log-probability of the drawn token under the
 * processed distribution before truncation, 0 for a finished row.  kept and kept_mass (K / S) keep their meaning.
 * With ctl->seen a live row sets the bit of the token it drew (eos included) in the same launch; a finished row sets
 * nothing.                                                                                                        */
int ergm_sample_rows(const float* logits, int ldl, int B, int V, float top_p, const ergm_sample_ctl* ctl, uint64_t seed,
                     const uint32_t* row_ids, const uint32_t* row_steps, void* finished, int64_t eos_id,
                     int64_t* tokens, int* kept, float* kept_mass, float* logprob, void* stream);
/* The bitmap and the minimum length of the slots an admission or an extension filled, one launch: sequence b < n_seq
 * (device int [n_seq] each: slot, start, len over the packed device int64 ids [total]; reset and min_new may be NULL)
 * clears row slot[b] of seen when reset[b] != 0, then sets the bit of each of its ids, and writes min_step[slot[b]] =
 * row_steps[slot[b]] + max(min_new[b], 0), so that a minimum length counts from the start of the turn (min_step and
 * row_steps uint32 [n_slots], both NULL to leave the minimum alone).  Clamped like ergm_rows_to_slots: len to [0,
 * total], start to the packed extent, an id outside [0, V) sets nothing, a slot outside [0, n_slots) writes nothing.
 * Found by symbol (ABI unchanged).                                                                                 */
int ergm_sample_mark(const int64_t* ids, int total, const int* slot, const int* start, const int* len, const int* reset,
                     const int* min_new, int n_seq, int V, int n_slots, uint32_t* seen, int ld_seen,
                     const uint32_t* row_steps, uint32_t* min_step, void* stream);
/* Packed rows into per-slot buffers: row t < len[b] of sequence b (row start[b] + t of src, ld_src bytes apart) is
 * copied to dst + slot[b]·ld_slot + t·ld_row (bytes), row_bytes bytes in 16-byte pieces.  start / len / slot: device
 * int [n_seq]; total_rows = the rows of src, max_rows = the host's bound on len (it sizes the grid).  len is clamped
 * to [0, min(max_rows, slot_rows)], start to the rows of src, and a sequence whose slot lies outside [0, n_slots)
 * writes nothing.  Moves K | V rows into the caches, caption K | V rows, and f32 logits rows (slot_rows = 1).      */
int ergm_rows_to_slots(const void* src, int64_t ld_src, const int* start, const int* len, const int* slot, int n_seq,
                       int total_rows, int max_rows, void* dst, int64_t ld_slot, int64_t ld_row, int row_bytes,
                       int n_slots, int slot_rows, void* stream);
/* ergm_rows_to_slots with a first destination row per sequence: row t goes to slot row dst_row0[b] + t (device int
 * [n_seq]).  dst_row0 is clamped to [0, slot_rows] and len to the rows left after it, so nothing lands at or past
 * slot_rows.  With every dst_row0[b] = 0 the result is ergm_rows_to_slots'.  Found by symbol (ABI unchanged).      */
int ergm_rows_to_slots_at(const void* src, int64_t ld_src, const int* start, const int* len, const int* slot,
                          const int* dst_row0, int n_seq, int total_rows, int max_rows, void* dst, int64_t ld_slot,
                          int64_t ld_row, int row_bytes, int n_slots, int slot_rows, void* stream);
/* ergm_embed_fwd for packed rows of n_seq sequences of different lengths: token row s < q_len[b] of sequence b (packed
 * row q_start[b] + s of ids / tt / h0) is ((wte[id] + [s==0]·vis[b] + [s==1]·aud[b]) + wpe[s]) + wte[tt], in that
 * kernel's summation order: bitwise the row ergm_embed_fwd(B = 1, S = q_len[b]) writes.  Caption row s < c_len[b]
 * (packed row c_start[b] + s of cap_ids / cap) is bf16(wte[cap_id]).  vis / aud: f32 [n_seq][E] (already projected)
 * or both NULL; has_feat (uint8 [n_seq], may be NULL = all) marks the sequences they apply to.  The starts and
 * lengths are device ints, clamped to max_rows / max_cap (host bounds, sizing the grid), n_positions and the packed
 * extents; ids outside [0, V) contribute zeros and tt may be NULL, as in ergm_embed_fwd.                          */
int ergm_embed_packed(const int64_t* ids, const int64_t* tt, const int64_t* cap_ids, const float* wte,
                      const float* wpe, const float* vis, const float* aud, const uint8_t* has_feat,
                      const int* q_start, const int* q_len, const int* c_start, const int* c_len, int n_seq,
                      int total_rows, int total_cap, int max_rows, int max_cap, float* h0, void* cap, int ld_cap,
                      int E, int V, int n_positions, void* stream);
/* Feature pooling (data_process/feature_extraction.py:63,69: torch.mean(last_hidden_state, dim=1) of the
 * wav2vec2 / BLIP-vision encoder outputs): out[b][d] = mean_{t < len_b} x[b][t][d], x f32 or bf16 with
 * strides ld_t (frames) and ld_b (samples) in elements, lengths optional (NULL = all T frames; padded
 * audio otherwise), out f32 [B][ld_out].  Fixed summation order (deterministic).                   */
int ergm_feat_pool(const void* x, int x_dtype, int B, int T, int D, long ld_t, long ld_b,
                   const int* lengths, float* out, int ld_out, void* stream);
/* Deterministic (sorted segment-sum) embedding backward:
 *   dwte[v] += Σ_{t: ids[t]=v} dh0[t] + Σ_{t: tt[t]=v} dh0[t] + Σ_{t: cap[t]=v} dcap[t]
 *   dwpe[s]  = Σ_b dh0[b,s]
 * workspace: ergm_embed_bwd_workspace_size(B*S) bytes.                                          */
size_t ergm_embed_bwd_workspace_size(int T);
int ergm_embed_bwd(const int64_t* ids, const int64_t* tt, const int64_t* cap_ids, const float* dh0,
                   const float* dcap, float* dwte, float* dwpe, void* workspace, size_t ws_bytes,
                   int B, int S, int E, int V, void* stream);

/* Shifted LM cross-entropy, fused forward+backward over bf16 logits [B*S][ldl] (columns >= V
 * ignored, zeroed in dlogits).  Row t=(b,s) is valid iff s < S-1 and labels[b][s+1] != -100.
 * n_valid_global: device int (count of valid rows over all DP ranks).
 * row_loss[t] = lse - logit[target] (0 for invalid); dlogits = grad_scale·(softmax - onehot)/n_valid
 * (bf16, may be NULL for forward only).  ergm_count_valid writes the local counts: counts[0] = LM
 * labels at s >= 1 with 0 <= y < V, counts[1] = emotion labels with 0 <= y < C (either label tensor
 * may be NULL: count 0).  Labels outside the range (-100 = torch's ignore_index) are ignored.       */
int ergm_count_valid(const int64_t* labels, const int64_t* emotion_labels, int B, int S, int V, int C,
                     int* counts, void* stream);
int ergm_xent_fwd_bwd(const void* logits, int ldl, const int64_t* labels, const int* n_valid_global,
                      float* row_loss, void* dlogits, int B, int S, int V, float grad_scale,
                      void* stream);
/* The rows the LM loss scores, for an LM-head backward over those rows only (ABI 12).  ergm_lm_rows writes, from
 * the labels alone (NULL: no row), rows[j] = the j-th row t = b*S+s with s < S-1 and 0 <= labels[b][s+1] < V in
 * ascending order (rows[j] = -1 for n <= j < B*S), pos[t] = j or -1, counts[0] = n (the local count) and
 * counts[1] = n rounded up to 64: a prefix sum in one workgroup, the same list in every run.
 * ergm_xent_compact is ergm_xent_fwd_bwd (grad_scale 1) writing the gradient row of scored row t to row pos[t] of
 * dlogits_c (bitwise the dense row), nothing for an ignored row (row_loss[t] = 0 as before), and zeros to rows
 * counts[0] .. counts[1]-1; dlogits_c holds B*S rounded up to 64 rows of ldl bf16.                       */
int ergm_lm_rows(const int64_t* labels, int B, int S, int V, int* rows, int* pos, int* counts, void* stream);
int ergm_xent_compact(const void* logits, int ldl, const int64_t* labels, const int* n_valid_global,
                      float* row_loss, void* dlogits_c, const int* pos, const int* counts, int B, int S, int V,
                      void* stream);
/* Emotion head on the last token: logits[b][c] = Σ_e h[b,S-1,e]·W[c][e] (h bf16, W f32 [C][E]);
 * with labels: loss_sum = Σ_b CE_b over valid labels (0 <= y < C; others, e.g. -100, are ignored),
 * scratch = B*(C+1) floats, n_valid_global = device count of valid labels (all DP ranks); with dW/dh:
 * dW[C][E] written and dh[b,S-1,:] += dlogits·W (f32 dh [B*S][E]), dlogits =
 * (softmax - onehot)·grad_scale/n_valid (0 for ignored labels).                                  */
int ergm_emotion_head(const void* h, const float* W, const int64_t* labels, float* logits,
                      float* loss_sum, float* dW, float* dh, float* scratch, int B, int S, int E, int C,
                      const int* n_valid_global, const float* grad_scale_dev, void* stream);
/* out[0] = Σ row_loss / n_valid_global (0 if n_valid_global is NULL), out[1] = emo_loss_sum /
 * n_valid_emo (0 if emo_loss_sum is NULL), out[2] = out[0]+out[1]; a zero count gives 0/0 = NaN,
 * as torch's mean CrossEntropyLoss does.                                                         */
int ergm_loss_finalize(const float* row_loss, int T, const int* n_valid_global,
                       const float* emo_loss_sum, const int* n_valid_emo, float* out, void* stream);

/* torch.optim.AdamW step over flat fp32 arrays; also refreshes the bf16 shadow copy.
 * Arithmetic in torch's order: p*=(1-lr·wd); m=lerp(m,g,1-β1); v=β2·v+(1-β2)g²;
 * p -= step_size · m / (sqrt(v)/bc2_sqrt + eps), step_size = lr/(1-β1^t), bc2_sqrt = sqrt(1-β2^t).
 * lr, β1, β2 and weight_decay are doubles (ABI 5): torch forms 1-lr·wd, 1-β1 and 1-β2 from the Python
 * doubles and rounds each once to fp32 (from a float β2 = 0.999f, 1-β2 is off by 1.3e-5 relative).
 * max_blocks > 0 caps the grid (grid-stride loop): an update running concurrently with the backward
 * on another stream then occupies only that many CUs instead of flooding the chip; 0 = full grid. */
int ergm_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n, double lr,
                    double beta1, double beta2, float eps, double weight_decay, float step_size,
                    float bc2_sqrt, int max_blocks, void* stream);
/* The same update restricted to the rows of a [rows][row_len] block whose flag byte matches:
 * row r is updated iff (row_flag[r] != 0) == (select != 0).  With ergm_model_set_row_flags this
 * splits the tied-embedding update into the rows only the LM head touched (final early in the
 * backward) and the rows the lookups touched (final after the embedding backward). */
int ergm_adamw_rows(float* p, const float* g, float* m, float* v, void* p_bf16, int rows, int row_len,
                    const void* row_flag, int select, double lr, double beta1, double beta2, float eps,
                    double weight_decay, float step_size, float bc2_sqrt, int max_blocks, void* stream);
/* bf16 shadow copy of fp32 values: dst[i] = bf16(src[i]). */
int ergm_cast_bf16(const float* src, void* dst, size_t n, void* stream);
/* y[i] += x[i] (f32), used to accumulate gradients across backward calls. */
int ergm_axpy(const float* x, float* y, size_t n, float alpha, void* stream);
/* Data-parallel gradient exchange in bf16 with fp32 accumulation (ergm_amd/dist.py): after an
 * all-to-all of bf16 gradient chunks, out[i] = bf16(Σ_{j < nchunks} in[j·chunk + i]) summed in fp32
 * in rank order j; after the all-gather, dst[i] = f32(src[i]).  chunk, n multiples of 4.           */
int ergm_chunk_sum_bf16(const void* in, int nchunks, size_t chunk, void* out, void* stream);
/* ZeRO-1 reduce-scatter tail: the same rank-order fp32 sum of the nchunks copies, rounded once to bf16 and
 * written widened to fp32 (out[i], i < n <= chunk, n % 4 == 0): this rank's reduced gradient chunk. */
int ergm_chunk_sum_bf16_f32(const void* in, int nchunks, size_t chunk, size_t n, float* out, void* stream);
/* Data-parallel bucket helpers (ergm_amd/dist.py, ZeRO-1 bf16 exchange), one launch each where the Python path
 * issued two or three: ergm_dp_pack_bf16 casts a bucket's n fp32 gradients into the all-to-all send buffer and zeroes
 * its padding up to `total`; ergm_dp_sum_adamw sums the received chunks in rank order, rounds once to bf16 (the
 * ergm_chunk_sum_bf16_f32 value, bitwise), writes the widened sum into grad[0..n) and applies ergm_adamw_step's
 * update to p / m / v [0..n) with it, the updated bf16 parameters going to `shadow` (this rank's all-gather slot);
 * max_blocks > 0 caps its grid like ergm_adamw_step's (an update overlapped with the backward's GEMMs). */
int ergm_dp_pack_bf16(const float* src, size_t n, void* dst, size_t total, void* stream);
int ergm_dp_sum_adamw(const void* in, int nchunks, size_t chunk, size_t n, float* grad, float* p, float* m, float* v,
                      void* shadow, double lr, double beta1, double beta2, float eps, double weight_decay,
                      float step_size, float bc2_sqrt, int max_blocks, void* stream);
int ergm_cast_f32(const void* src, float* dst, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-model executor.  The caller owns every buffer; ergm_model_plan only records pointers and
 * dimensions (see ergm_amd/model.py for the layout it builds).  Forward = src/model.py:654-737;
 * backward = loss.backward() (src/main.py:154), with per-layer entry points so a data-parallel
 * caller can start gradient all-reduce buckets as layers finish.
 * ------------------------------------------------------------------------------------------- */
typedef struct ergm_model_plan ergm_model_plan;

typedef struct {
    int vocab, vocab_pad, n_embd, n_layer, n_head, n_inner, n_positions;
    int batch, seq;           /* local (per-rank) batch and sequence length */
    float eps;
    int has_features;         /* visual/audio injection present */
    int ld_vis;               /* row stride of the visual feature (Tv*Fd when [B,Tv,Fd]) */
    int feat_dim;             /* Fd: width of the pooled features; 0 or n_embd = added directly
                               * (src/model.py:497-498); otherwise a Conv1D projection per modality
                               * (build-side, config 5: 768-d features into a 1024-d backbone) */
    int fp8;                  /* 1: the forward Conv1D GEMMs of every block (and the caption K/V
                               * GEMM) run on fp8: ergm_gemm_mx on MX-fp8 operands (default; the
                               * LayerNorms, the GELU epilogue and the attention forward write the MX
                               * copies of their outputs) or, with ERGM_FP8_MX=0, ergm_gemm_f8 with
                               * per-row activation / per-column weight scales; weights are
                               * re-quantised from the bf16 shadow at every forward; LM head,
                               * backward and optimizer stay bf16/f32 */
} ergm_model_dims;

/* Pointer table: names follow the reference state_dict; see ergm_amd/model.py. */
typedef struct {
    /* fp32 master params and their bf16 shadows (same element offsets) */
    const float* wte;  const void* wte_b;   /* [vocab_pad][E] */
    const float* wpe;                        /* [n_positions][E] */
    const float* ln_f_w; const float* ln_f_b;
    const float* emo_w;                      /* [7][E] */
    const void* capkv_w_b; const float* capkv_b;  /* stacked cross c_attn: [E][L*2E], [L*2E] */
    /* per layer i, base pointers into the flat buffers; offsets of each tensor within a layer
     * block are given by layer_off[] (elements) in the order of ergm_layer_tensor. */
    const float* layer_f32; const void* layer_b16;
    int64_t layer_stride;     /* elements between layer i and i+1 blocks (negative: reversed order) */
    int64_t layer_off[18];
    /* gradients (f32, same layout as params) */
    float* g_wte; float* g_wpe; float* g_ln_f_w; float* g_ln_f_b; float* g_emo_w;
    float* g_capkv_w; float* g_capkv_b; float* g_layer;
    /* feature projections (feat_dim != n_embd only): visual / audio Conv1D weights [Fd][E] (bf16
     * shadow), biases [E] f32, gradients f32; each bias stored right after its weight */
    const void* vproj_w_b; const float* vproj_b; const void* aproj_w_b; const float* aproj_b;
    float* g_vproj_w; float* g_vproj_b; float* g_aproj_w; float* g_aproj_b;
    /* fp32 master of the stacked caption K/V weight [E][L*2E]; optional, not read by the executor (the
     * fp8 weight quantiser reads the bf16 shadow capkv_w_b) */
    const float* capkv_w;
} ergm_model_params;

typedef enum {
    ERGM_T_LN1_W = 0, ERGM_T_LN1_B, ERGM_T_ATTN_W, ERGM_T_ATTN_B, ERGM_T_APROJ_W, ERGM_T_APROJ_B,
    ERGM_T_LNX_W, ERGM_T_LNX_B, ERGM_T_XQ_W, ERGM_T_XQ_B, ERGM_T_XPROJ_W, ERGM_T_XPROJ_B,
    ERGM_T_LN2_W, ERGM_T_LN2_B, ERGM_T_FC_W, ERGM_T_FC_B, ERGM_T_MPROJ_W, ERGM_T_MPROJ_B,
} ergm_layer_tensor;

/* Bytes of device workspace the executor needs (activations saved for backward + scratch).
 * Shape rules: 2 <= seq <= n_positions, any batch (token counts B*S that are not multiples of 64 run
 * the weight-gradient GEMMs on the register-staged kernel), n_head * 64 == n_embd <= 1024, n_inner and
 * feat_dim multiples of 64; ERGM_EINVAL otherwise. */
size_t ergm_model_workspace_size(const ergm_model_dims* dims);
int ergm_model_create(const ergm_model_dims* dims, const ergm_model_params* params, void* workspace,
                      size_t ws_bytes, ergm_model_plan** out_plan);
int ergm_model_destroy(ergm_model_plan* plan);
/* Inputs for the next forward (device pointers, int64 [B][S]; features f32 or NULL; labels may be
 * NULL for inference).  counts_global: device int[2] the caller filled (ergm_count_valid + optional
 * all-reduce over DP ranks): the LM and the emotion loss means divide by these global counts.     */
/* Optional: a caller-owned byte per padded vocabulary row (n >= vocab_pad).  When set, every training
 * forward writes 1 for the rows its token / token-type / caption lookups touch and 0 elsewhere
 * (stream-ordered, final once the forward returns on its stream).  The lookup gradients of the
 * embedding backward land only in flagged rows of g_wte; all other rows of g_wte are final once
 * the LM-head weight gradient is (after ergm_model_backward_layer(L-2)), which lets an optimizer
 * update them while the rest of the backward runs.  NULL disables. */
int ergm_model_set_row_flags(ergm_model_plan* plan, void* row_flag, int n);
/* Optional (data parallelism): route the lookup gradient sums of the embedding backward to
 * compact[row_pos[row]] (rows of E floats, added onto caller-zeroed rows) instead of adding them to
 * g_wte[row].  row_pos = ergm_rows_scan of the rank-union of the row flags.  NULLs disable. */
int ergm_model_set_lookup_compact(ergm_model_plan* plan, const int* row_pos, float* compact);
/* pos[r] = number of nonzero flags before r (exclusive prefix sum), count[0] = the total. */
int ergm_rows_scan(const void* row_flag, int n, int* pos, int* count, void* stream);
/* For every flagged row r of n: mode 0 zeroes compact[pos[r]]; mode 1 adds it into dst[r]
 * (rows of row_len floats). */
int ergm_rows_compact(const void* row_flag, const int* pos, int n, int row_len, float* compact, float* dst,
                      int mode, void* stream);
int ergm_model_set_inputs(ergm_model_plan* plan, const int64_t* ids, const int64_t* tt,
                          const int64_t* cap_ids, const float* vis, const float* aud,
                          const int64_t* labels, const int64_t* emotion_labels,
                          const int* counts_global);
/* Forward. Outputs (device): logits bf16 [B*S][vocab_pad], emotion logits f32 [B][7],
 * loss parts f32 (ergm_loss_finalize layout: [lm, emotion, total], local contributions over the
 * global normalisers); with `train`, dlogits are prepared for the backward.                      */
int ergm_model_forward(ergm_model_plan* plan, void* logits, float* emo_logits, float* out_loss,
                       int train, void* stream);
/* Backward in stages so a DP caller can overlap communication:
 *   ergm_model_backward_head  — LM head + emotion head + ln_f (grads of wte(part), emo, ln_f)
 *   ergm_model_backward_layer — block `layer` (call for L-1 … 0)
 *   ergm_model_backward_embed — stacked caption K/V projection + embeddings (wte rest, wpe)
 * Weight-gradient GEMMs run on the plan's internal side stream.  Ordering guarantee on `stream`:
 * after backward_layer(l) the gradients of the head stage and of blocks > l are final (block l's
 * own weight gradients are joined by the NEXT stage); after backward_embed every gradient is. */
int ergm_model_backward_head(ergm_model_plan* plan, const float* grad_scale_dev, void* stream);
int ergm_model_backward_layer(ergm_model_plan* plan, int layer, void* stream);
int ergm_model_backward_embed(ergm_model_plan* plan, void* stream);
/* Dropout of the next training forwards (ergm_model_forward with train = 1) and their backward:
 * attn_p = attention probabilities (src/model.py:142), resid_p = the attention / cross-attention /
 * MLP residual branches (:245, :266), embd_p = the embeddings (:506); all 0 = the deterministic path
 * (default).  Masks are ergm_dropout_mask's with this seed and offset (the caller advances offset
 * every training forward), site numbers ERGM_DROP_SITE_*, rows counted from global sample
 * batch_base (data parallelism: rank·batch, so DP ranks draw exactly the masks one process would
 * draw for the concatenated batch).  Inference forwards (train = 0) never drop.                  */
int ergm_model_set_dropout(ergm_model_plan* plan, float attn_p, float resid_p, float embd_p, uint64_t seed,
                           uint32_t offset, int batch_base);
/* Executor-scheduled AdamW (single process).  With a descriptor set, the backward stages also launch the
 * torch.optim.AdamW update (ergm_adamw_step / ergm_adamw_rows arithmetic) of each parameter range as soon as
 * its gradient is final, on an optimizer stream of the plan that waits for the stage's data-gradient work and
 * its weight-gradient mark; ergm_model_backward_embed joins that stream into the caller's, so every update is
 * done, in stream order, when it returns.  Schedule: range k of `ranges` after stage k (0: head + block L-1,
 * …, L-1: block 0, the last after the embedding stage), range L (caption K/V + wpe) after the embedding
 * stage; the tied wte ([vocab_pad][n_embd] at wte_begin): the rows no lookup touched (ergm_model_set_row_flags)
 * after the LM-head weight gradient (stage L-2), the touched rows after the embedding stage (all rows there
 * when no row flags are set).  The descriptor (and its ranges) is copied; set it again every step (lr, step
 * size); NULL disables.  Replaces ergm_amd's per-bucket Python hooks: one Python call per backward stage. */
typedef struct {
    float* param;             /* flat fp32 master */
    const float* grad;        /* flat fp32 gradient */
    float* exp_avg;
    float* exp_avg_sq;
    void* param_bf16;         /* flat bf16 shadow (refreshed by the update), or NULL */
    const int64_t* ranges;    /* [n_ranges][2] element ranges [a, b) */
    int n_ranges;             /* n_layer + 1 */
    int64_t wte_begin;        /* element offset of the tied wte */
    double lr, beta1, beta2, weight_decay;  /* doubles as torch holds them (ABI 5) */
    float eps;
    float step_size;          /* lr / (1 - beta1^t) */
    float bc2_sqrt;           /* sqrt(1 - beta2^t) */
    int max_blocks;           /* grid cap of each update, 0 = none */
    int defer;                /* 1: the updates of blocks 1 … L-1 (and the head) are launched after the embedding
                               * stage instead, in forward order, and NOT joined: the next forward of the plan
                               * waits for each block's update before that block (so they overlap the
                               * latency-bound forward instead of the throughput-bound backward); anything else
                               * that reads the parameters first calls ergm_model_optimizer_join */
} ergm_adamw_desc;
int ergm_model_set_optimizer(ergm_model_plan* plan, const ergm_adamw_desc* opt);
/* Make `stream` wait for every deferred update still pending (no-op when none). */
int ergm_model_optimizer_join(ergm_model_plan* plan, void* stream);
/* Side-stream joins.  per_stage = 1 (default): the ordering guarantee above.  per_stage = 0: the
 * caller's stream does not wait for block l+1's weight gradients at the end of stage l (so the
 * data-gradient chain never idles behind the weight-gradient GEMMs); only backward_embed joins, after
 * which every gradient is final on `stream` as before.  A consumer of block l's gradients (a DP
 * all-reduce, an overlapped optimizer) then makes its stream wait with ergm_model_stage_wait(plan, l,
 * its_stream) after the stage that finalises it was enqueued; stage L+1 = the LM-head (tied wte)
 * weight gradient, L+2 = the caption K/V / projection weight gradients.                             */
int ergm_model_set_side_joins(ergm_model_plan* plan, int per_stage);
/* Trainer metrics on the device (src/main.py:158-169: the running sum of loss.item() and the emotion
 * argmax accuracy): when set, every training forward adds its total loss to loss_acc[0], its LM loss to
 * loss_acc[1] and its number of samples with argmax(emotion_logits) == emotion_labels (first maximum, as
 * torch.argmax) to *correct, in the loss finalisation (no extra launch).  nullptr pointers: off.      */
int ergm_model_set_metrics(ergm_model_plan* plan, float* loss_acc, int64_t* correct);
/* A caller's gradient on the logits of the last training forward (bf16 [B*S][vocab_pad], pad columns 0;
 * src/model.py:698 returns differentiable logits): the next ergm_model_backward_head adds it to the
 * cross-entropy's dlogits (dlogits = bf16(grad_scale · dlogits + grad_logits)) before the LM-head backward
 * GEMMs, then forgets it.  NULL: none (default).  The buffer must stay valid until that call. */
int ergm_model_set_logits_grad(ergm_model_plan* plan, const void* grad_logits);
int ergm_model_stage_wait(ergm_model_plan* plan, int stage, void* stream);

/* Kernel probe for in-loop timing: while set, the executor records `ev_begin` / `ev_end`
 * (hipEvent_t, passed as void*) on the stream immediately around the probed launch:
 *   1 = tied LM-head forward GEMM      2 = LM-head dX GEMM      3 = LM-head dW GEMM
 *   4 = stacked caption-K/V forward GEMM (all blocks)        0 = off                         */
int ergm_model_set_probe(ergm_model_plan* plan, int probe, void* ev_begin, void* ev_end);
/* List probe (bench roofline of a launch class): event pair k is recorded around the k-th launch of the class
 * in the following steps, up to n, and flops[k] (host array, may be NULL) receives its algorithmic FLOPs;
 * ergm_model_probe_count returns how many were recorded.  probe 5 = the weight-gradient GEMMs (every block's
 * Conv1D dW + bias, the stacked caption K/V dW, the LM-head dW), 6 = the block forward Conv1D GEMMs.
 * n = 0 disables.  The LM-head dW runs over the scored rows only: in steps with list probe 5 active its entry is
 * the FLOPs issued, 2·vocab_pad·n_embd·(scored rows rounded up to 64), from a host copy of the row count that
 * only those steps make. */
int ergm_model_set_probe_list(ergm_model_plan* plan, int probe, void** ev_begin, void** ev_end, double* flops, int n);
int ergm_model_probe_count(const ergm_model_plan* plan);
/* Copies the head stage's data gradient dy [batch*seq][n_embd] f32 (the LM-head dX plus the emotion head's rows
 * seq-1) to dst on `stream`: valid between ergm_model_backward_head and the next training forward (ABI 12). */
int ergm_model_copy_head_dy(ergm_model_plan* plan, float* dst, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Decode executor: one generation step of B ragged sequences (ergm_amd/generate.py BatchedGenerator.step) and
 * the sampling loop around it as native launch sequences.  Like ergm_model_plan the plan records pointers and
 * dimensions only; creating and destroying one touches no GPU.  Everything runs on the caller's one stream: no
 * events, no second stream, no graph capture, nothing synchronises and no device memory is read on the host.
 * The prompt is encoded by the caller (the training kernels; generate.py's prefill), which then binds its caches.
 * ------------------------------------------------------------------------------------------- */
typedef struct ergm_decode_plan ergm_decode_plan;
typedef struct {
    int vocab, vocab_pad, n_embd, n_layer, n_head, n_inner, n_positions;
    int max_batch;            /* sequences at most */
    int max_len;              /* rows of every sequence's self-attention cache, <= n_positions */
    int cap_max;              /* caption rows at most (Sc of ergm_decode_bind) */
    float eps;
} ergm_decode_dims;
/* Bytes of device workspace of a plan (the step's activations and the kernels' scratch); host only.  0 for
 * dimensions ergm_decode_create rejects: n_head·64 == n_embd <= 1024, n_inner % 64 == 0, vocab_pad % 64 == 0,
 * 1 <= max_len <= n_positions, max_batch, cap_max, n_layer >= 1.                                              */
size_t ergm_decode_workspace_size(const ergm_decode_dims* dims);
/* params: only the forward pointers are read (wte, wte_b, wpe, ln_f_w, ln_f_b, layer_f32, layer_b16, layer_stride,
 * layer_off; capkv_w_b and capkv_b by ergm_decode_admit only, which refuses a plan created without them).  workspace: 256-byte aligned, ws_bytes >= ergm_decode_workspace_size(dims).                       */
int ergm_decode_create(const ergm_decode_dims* dims, const ergm_model_params* params, void* workspace,
                       size_t ws_bytes, ergm_decode_plan** out_plan);
int ergm_decode_destroy(ergm_decode_plan* plan);
/* The state of B <= max_batch sequences after the prefill (device pointers the caller owns and keeps valid):
 *   kv[l]    layer l's self-attention cache, bf16 [max_batch][max_len][2·n_embd], K | V of a position in one row
 *   xkv[l]   layer l's caption K | V, bf16 [B][Sc][2·n_embd], 1 <= Sc <= cap_max
 *   lens     int [B] cache lengths (in/out: a step adds 1 for every sequence not yet finished); n_max = the host's
 *            bound on max(lens), which the plan advances by one per step
 *   cap_lens int [B] caption lengths; finished uint8 [B] (ergm_topp_sample's flags); logits f32 [B][vocab_pad], written
 *            by every step.  The pointer arrays kv / xkv (n_layer host entries each) are copied.                */
int ergm_decode_bind(ergm_decode_plan* plan, int B, int n_max, void* const* kv, void* const* xkv, int Sc, int* lens,
                     const int* cap_lens, uint8_t* finished, float* logits);
/* engine 0 (default): the kernels generate.py's Python step calls, launch for launch with the same arguments
 * (ergm_layernorm_fwd, ergm_gemm with split_k = 0, ergm_attn_decode with splits = 0): every buffer is bitwise what
 * that path writes.  engine 1: every LayerNorm + GEMM pair and every plain GEMM of the blocks is one
 * ergm_linear_rows launch (8 launches per block instead of 11); the head stays ergm_layernorm_fwd + ergm_gemm, which
 * measured faster at vocabulary width.                                                            */
int ergm_decode_set_engine(ergm_decode_plan* plan, int engine);
/* One step: ergm_embed_rows of `tokens` / `token_types` (device int64 [B]; token_types may be NULL) at lens, the
 * n_layer blocks (self-attention appends the new K | V row to kv), ln_f and the tied head into logits, then
 * lens[b] += !finished[b].  ERGM_EINVAL, before any launch, without a bind or with the cache full (n_max >= max_len). */
int ergm_decode_step(ergm_decode_plan* plan, const int64_t* tokens, const int64_t* token_types, void* stream);
/* Samples i = first .. first+n-1 of nucleus sampling (generate.py's loop): for i > 0 a step on tokens_out[i-1] typed
 * sp2_id, then ergm_topp_sample(logits, vocab, top_p, seed, step = i, finished, eos_id) into tokens_out[i]
 * (device int64 [>= first+n][B]).  A row that has just drawn eos is stepped once more without advancing its length.
 * Enqueues and returns.  ERGM_EINVAL before any launch when n < 1, first < 0 or the steps would overrun the cache.
 * `first` is the caller's count of samples already drawn since the bind: the plan does not check it.  After any other
 * failure (a launch error part-way) bind again before going on.                                                     */
int ergm_decode_run(ergm_decode_plan* plan, int first, int n, float top_p, uint64_t seed, int64_t eos_id,
                    int64_t sp2_id, int64_t* tokens_out, void* stream);
/* Kernel launches one ergm_decode_step enqueues with `engine`, for the bound batch (max_batch before a bind) and the
 * GEMM / attention plans as they stand now: counted by walking the step's own launch sequence dry.  Host only;
 * negative ergm_status on a bad argument.                                                                          */
int ergm_decode_launches(const ergm_decode_plan* plan, int engine);
/* Slot mode (continuous batching): the plan's max_batch cache slots stay bound for its life, every step runs over all
 * of them, and sequences enter free slots between steps (ergm_decode_admit) while the others keep decoding.
 *   kv[l] bf16 [max_batch][max_len][2·n_embd], xkv[l] bf16 [max_batch][cap_max][2·n_embd], logits f32
 *   [max_batch][vocab_pad]; lens, cap_lens, stop_lens int [max_batch]; finished uint8 [max_batch]; row_ids, row_steps
 *   uint32 [max_batch] (ergm_topp_sample_rows' counters: the request a slot serves and the tokens it has drawn).
 * An idle slot holds finished = 1, lens = 0, cap_lens = 0 (the caller initialises all slots so): its cross-attention
 * writes zeros and its self-attention append lands in row 0 of a cache nobody reads.  After this bind
 * ergm_decode_step / _run refuse (they serve ergm_decode_bind), and the other way round.                          */
int ergm_decode_bind_slots(ergm_decode_plan* plan, void* const* kv, void* const* xkv, float* logits, int* lens,
                           int* cap_lens, uint8_t* finished, int* stop_lens, uint32_t* row_ids, uint32_t* row_steps);
#define ERGM_ADMIT_META_ROWS 10
/* Bytes of device workspace of one ergm_decode_admit of at most max_rows packed token rows and max_cap_rows packed
 * caption rows; host only, 0 for dimensions or row counts it rejects.                                              */
size_t ergm_decode_admit_workspace_size(const ergm_decode_dims* dims, int max_rows, int max_cap_rows);
/* The prefill of n_seq new sequences into the named slots, enqueued on `stream` between decode steps:
 * ergm_embed_packed; per layer ergm_layernorm_fwd / ergm_gemm (split_k = 0) over the packed rows, ragged causal
 * attention, K | V rows to the slots, the caption K | V GEMM over the packed caption rows and its rows to the slots,
 * ragged cross-attention, the MLP; then the last row of every sequence through ln_f and the head into logits[slot];
 * then one kernel sets lens = n_b, cap_lens = c_b, stop_lens = n_b + max_new, row_ids = the request id, row_steps = 0,
 * finished = 0 of every slot filled.  The same kernels with the same arguments on both engines.
 *   slots, lens, cap_lens, max_new: HOST int [n_seq], checked here; ERGM_EINVAL before any launch for a slot outside
 *     [0, max_batch) or named twice, n_b < 1, c_b < 1, c_b > cap_max, max_new < 1, n_b + max_new > max_len, or more
 *     packed rows than the workspace holds.
 *   meta: DEVICE int [ERGM_ADMIT_META_ROWS][n_seq], what the kernels read (each value clamped before use): rows
 *     0 slot, 1 first packed token row, 2 n_b, 3 first packed caption row, 4 c_b, 5 max_new, 6 request id (uint32),
 *     7 last packed token row (row 1 + row 2 - 1), 8 all ones, 9 0 .. n_seq-1.
 *   ids, token_types (may be NULL): device int64 [Σ n_b]; cap_ids: device int64 [Σ c_b]; vis / aud: device f32
 *     [n_seq][n_embd] already projected, or both NULL; has_feat: device uint8 [n_seq] or NULL (ergm_embed_packed).  */
int ergm_decode_admit(ergm_decode_plan* plan, int n_seq, const int* slots, const int* lens, const int* cap_lens,
                      const int* max_new, const int* meta, const int64_t* ids, const int64_t* token_types,
                      const int64_t* cap_ids, const float* vis, const float* aud, const uint8_t* has_feat,
                      void* workspace, size_t ws_bytes, void* stream);
/* Kernel launches of one ergm_decode_admit of n_seq sequences with `rows` packed token rows and `cap_rows` packed
 * caption rows, counted by walking the admission's own launch sequence dry.  Host only.                          */
int ergm_decode_admit_launches(const ergm_decode_plan* plan, int n_seq, int rows, int cap_rows);
#define ERGM_EXTEND_META_ROWS 12
/* Extends n_seq OCCUPIED slots by n_b >= 1 new tokens each (a later turn of a conversation; found by symbol, the ABI
 * version is unchanged), on the admission's workspace (ergm_decode_admit_workspace_size; max_cap_rows is not used):
 * ergm_embed_rows over the R = Σ n_b packed rows at their own positions; per layer LayerNorm, the qkv GEMM over the
 * packed rows, ergm_rows_to_slots_at of the K | V columns to rows past_b .. of the slot, ergm_attn_fwd_extend over the
 * slot's cache, the projection, LayerNorm, the q GEMM, ergm_attn_fwd_ragged(causal = 0) over the caption rows the
 * admission left in the slot (xkv[l] as packed rows; no caption GEMM runs), the projection, the MLP; then the last new
 * row of every sequence through ln_f and the head into logits[slot]; then one kernel sets lens = past_b + n_b,
 * stop_lens = past_b + n_b + max_new and finished = 0 of every slot extended, and leaves cap_lens, row_ids and
 * row_steps alone: the request goes on drawing from fresh Philox counters.  12 launches per block + 6 when no GEMM
 * splits, whatever n_seq is.
 *   slots, past, lens (= n_b), cap_lens, max_new: HOST int [n_seq], checked here; ERGM_EINVAL before any launch for a
 *     slot outside [0, max_batch) or named twice, n_b < 1, past_b < 2 (positions 0 and 1 may carry the admission's
 *     visual / audio vectors), c_b outside [1, cap_max], max_new < 1, past_b + n_b + max_new > max_len, or more packed
 *     rows than the workspace holds.  past_b and c_b are the caller's record of the slot's lens and cap_lens.
 *   meta: DEVICE int [ERGM_EXTEND_META_ROWS][n_seq], what the kernels read (each value clamped before use): rows
 *     0 slot, 1 first packed row, 2 n_b, 3 past_b, 4 slot · max_len (first key row), 5 past_b + n_b (key rows),
 *     6 slot · cap_max (first caption row), 7 c_b, 8 max_new, 9 last packed row (row 1 + row 2 - 1), 10 all ones,
 *     11 0 .. n_seq-1.
 *   ids, token_types (may be NULL): device int64 [R]; pos: device int [R], past_b + s for row s of sequence b.      */
int ergm_decode_extend(ergm_decode_plan* plan, int n_seq, const int* slots, const int* past, const int* lens,
                       const int* cap_lens, const int* max_new, const int* meta, const int64_t* ids,
                       const int64_t* token_types, const int* pos, void* workspace, size_t ws_bytes, void* stream);
/* Kernel launches of one ergm_decode_extend of n_seq sequences with `rows` packed rows, counted by walking the
 * extension's own launch sequence dry.  Host only.                                                               */
int ergm_decode_extend_launches(const ergm_decode_plan* plan, int n_seq, int rows);
/* One step over all max_batch slots (ergm_decode_step's kernels at B = max_batch, caption bound cap_max), then the
 * slot length update: a row not finished gets ++lens, ++row_steps, and finished = 1 when lens reaches stop_lens, so
 * no row can pass the bound recorded at its admission (n_b + max_new <= max_len) whatever the host does.          */
int ergm_decode_step_slots(ergm_decode_plan* plan, const int64_t* tokens, const int64_t* token_types, void* stream);
/* For i < n: ergm_topp_sample_rows(logits, row_ids, row_steps, finished) into tokens_out[i] (device int64
 * [n][max_batch]), then one step on those tokens typed sp2_id, over every slot.  One stream, no events, nothing read
 * back: the host looks at tokens_out and finished when it chooses.                                                */
int ergm_decode_run_slots(ergm_decode_plan* plan, int n, float top_p, uint64_t seed, int64_t eos_id, int64_t sp2_id,
                          int64_t* tokens_out, void* stream);
/* ergm_decode_run_slots with ergm_sample_rows(ctl, may be NULL) in the place of ergm_topp_sample_rows: the same loop,
 * the same stream discipline and the same launch counts.  logprobs_out: device f32 [n][max_batch] or NULL.  Found by
 * symbol (ABI unchanged).                                                                                          */
int ergm_decode_run_slots_sampled(ergm_decode_plan* plan, int n, float top_p, const ergm_sample_ctl* ctl, uint64_t seed,
                                  int64_t eos_id, int64_t sp2_id, int64_t* tokens_out, float* logprobs_out, void* stream);

/* ---- Beam search (found by symbol, ABI unchanged) ----------------------------------------------------------------
 * A batch of G prompts with W beams each (1 <= W <= 8, W <= V) occupies R = G·W rows; group g owns rows g·W ..
 * g·W + W - 1.  A row's state is its score (f32, the sum of the log-probabilities of the tokens the beam has taken),
 * its finished flag (uint8), its length, its caches and its logits.  One round is select, gather, step.
 *
 * Select, per group.  A live beam w (not finished, score above -inf; a NaN score counts as -inf) offers a candidate
 * (w, j) for every j < V whose logit x_j is finite, with the value
 *     c = score[w] + ((x_j - max) - ln(S · 2^-30)),
 * max the row's largest finite logit and S = Σ floor(expf(x - max) · 2^30) its integer mass over the finite logits
 * (ergm_sample_rows' logprob: the same max, the same exact S; the logarithm is taken in double and rounded to f32 once
 * per row, the two subtractions and the sum are f32, in that order), so c depends on no summation order.  A finished
 * beam offers the one candidate (w, eos_id) with c = score[w]; a beam at -inf offers nothing and its logits are not
 * read.  The W candidates with the largest c are taken, ties to the lower beam, then the lower token.  Slot
 * assignment depends on the selected set only, not on rank: with the selected candidates ordered by (beam, token)
 * ascending, the first child of beam w stays in row w of the group, and the remaining children, in that order, fill
 * the rows of the group's childless beams in ascending row order.  For every row r: parent_out[r] (int32, the global
 * row index), token_out[r] (int64), scores[r] = c, finished[r] = the parent's flag or token == eos_id.  With fewer than
 * W candidates the rows left over get score -inf, finished 1, token eos_id, parent r.  scores and finished are updated
 * in place; the result is the same bits in every run (no float atomics).  workspace: 8-byte aligned, at least
 * ergm_beam_select_workspace_size(R, W) bytes (0 for a bad R or W).  V <= 53,248; 0 <= eos_id < V.
 *
 * Gather.  For every row with parent[r] != r, rows [0, lens[parent[r]]) of every layer's cache go from slot parent[r]
 * to slot r (slot s of layer l at caches[l] + s·ld_seq, its row i at + i·ld_row, row_bytes each; bytes, multiples of
 * 16, copied in 16-byte pieces) and lens[r] = lens[parent[r]].  Select's sources keep their own row and its
 * destinations are childless rows, so no slot is both read and written and the copy is safe in place.  Rows with
 * parent[r] == r are not touched, nothing at or past the length is written, and a round in which every beam keeps its
 * row moves no byte.  A parent outside the row's own group, or one that does not keep its own row, counts as self, and
 * a length is clamped to [0, max_len]: no value makes the kernel follow an index out of a table.  caches: a host array
 * of n_layer device pointers; one launch covers up to 48 layers.
 *
 * ergm_decode_run_beams: n rounds over the state ergm_decode_bind bound with B = R (refused in slot mode): select on
 * the bound logits into tokens_out[i] / parents_out[i] (device int64 / int32 [n][R]) with scores (device f32 [R]) and
 * the bound finished flags, gather over the bound self-attention caches and lens, then ergm_decode_step's kernels on
 * the tokens typed sp2_id (a finished row is stepped on eos without advancing).  Round 0 needs no fan-out: after the
 * prefill only row g·W of each group holds the prompt (cache rows, length, logits), the scores are [0, -inf, ...], so
 * all W children come from beam 0 and the gather copies the prompt into the other rows; the caption K | V and cap_lens
 * are the same in all W rows of a group from the start.  One stream, no events, nothing read back.  workspace: that of
 * ergm_beam_select for (R, W).  ERGM_EINVAL before any launch for W outside [1, 8], R % W != 0, a plan bound in slot
 * mode or not bound, and n rounds that would overrun the cache (n_max + n > max_len).                               */
size_t ergm_beam_select_workspace_size(int R, int W);
int ergm_beam_select(const float* logits, int ldl, int R, int W, int V, float* scores, uint8_t* finished, int64_t eos_id,
                     int* parent_out, int64_t* token_out, void* workspace, size_t ws_bytes, void* stream);
int ergm_beam_gather(void* const* caches, int n_layer, int64_t ld_seq, int64_t ld_row, int row_bytes, const int* parent,
                     int* lens, int R, int W, int max_len, void* stream);
int ergm_decode_run_beams(ergm_decode_plan* plan, int n, int W, int64_t eos_id, int64_t sp2_id, float* scores,
                          int64_t* tokens_out, int* parents_out, void* workspace, size_t ws_bytes, void* stream);

/* ---- Beam search in slot mode (found by symbol, ABI unchanged) -----------------------------------------------------
 * The max_batch slots of ergm_decode_bind_slots are G = max_batch / W groups of W slots, group g rows g·W .. g·W + W - 1:
 * the layout select and gather assume.  A prompt enters a group through ergm_decode_admit with slots[b] = g_b·W, which
 * fills row g·W alone; ergm_beam_seed, on the same stream behind it, leaves the group in the state round 0 starts from:
 *   - rows [0, c) of every layer's caption K | V go from slot g·W to slots g·W + 1 .. g·W + W - 1, with
 *     c = clamp(cap_lens[g·W], 0, cap_max) read on the device and clamped before an address is formed (slot s of layer
 *     l at xkv[l] + s·ld_seq, its row i at + i·ld_row, row_bytes each; bytes, multiples of 16; the gather's layout: a
 *     workgroup per (destination row, layer, 64-row chunk), a wave per row, up to 48 layers per launch);
 *   - rows g·W + w, w >= 1: cap_lens = c, stop_lens = stop_lens[g·W], lens = 0, finished = 0, scores = -inf;
 *   - row g·W: scores = 0, and nothing else of it is written.
 * The kernels read the group ids from groups_dev (device int32 [n_grp]); an id outside [0, G) writes nothing.  Every
 * destination row has one writer and what is read (cap_lens / stop_lens of row g·W, its caption rows) is written by
 * nobody, so the launches need no ordering among themselves: plain stores, no atomics.  groups is the same list on the
 * host.  ERGM_EINVAL before any launch for an id outside [0, G) or named twice, n_grp outside [1, G], W outside [1, 8],
 * max_batch % W != 0, strides or row_bytes that are no multiples of 16, and a null pointer.  W = 1 launches the state
 * kernel only.
 *
 * ergm_decode_run_slot_beams: n rounds over all max_batch slots of a plan bound in slot mode.  A round is
 * ergm_logit_rules_apply while ergm_decode_set_rules holds rules, ergm_beam_select with R = max_batch on the bound
 * logits and finished flags into tokens_out[i] / parents_out[i] (device int64 / int32 [n][max_batch]) and scores
 * (device f32 [max_batch]), ergm_beam_gather over the bound self-attention caches and lens, ergm_hist_follow +
 * ergm_hist_append under rules, then ergm_decode_step_slots' kernels on the round's tokens typed sp2_id: a live row
 * advances and is finished by the device when its length reaches stop_lens, so a group ends at eos on every beam or at
 * its bound.  An idle or finished group offers eos at unchanged scores and moves nothing.  rows_bound is the caller's
 * host bound on the live lengths at entry: the gather's grid covers min(rows_bound + i, max_len) cache rows in round i;
 * the kernel's own clamp keeps a wrong bound from reading or writing outside a cache, but rows past it are not copied,
 * so the caller passes a correct one.  One stream, no events, nothing read back.  workspace: that of ergm_beam_select
 * for (max_batch, W).  ERGM_EINVAL before any launch for a plan not bound in slot mode, n < 1, W outside [1, 8] or above
 * the vocabulary, max_batch % W != 0, eos_id outside the vocabulary, rows_bound outside [0, max_len], a null or
 * misaligned argument, and a workspace below ergm_beam_select_workspace_size(max_batch, W).                            */
int ergm_beam_seed(void* const* xkv, int n_layer, int64_t ld_seq, int64_t ld_row, int row_bytes, const int* groups_dev,
                   const int* groups, int n_grp, int W, int max_batch, int cap_max, int* lens, int* cap_lens, int* stop_lens,
                   uint8_t* finished, float* scores, void* stream);
int ergm_decode_run_slot_beams(ergm_decode_plan* plan, int n, int W, int rows_bound, int64_t eos_id, int64_t sp2_id,
                               float* scores, int64_t* tokens_out, int* parents_out, void* workspace, size_t ws_bytes,
                               void* stream);

/* ---- Logit rules: no repeated n-gram, bad words (found by symbol, ABI unchanged) ------------------------------------
 * Both rules need the ordered tokens of a row, which no other kernel keeps: hist is int32 [R][ld_hist], row r holding
 * the prompt and the generated tokens of the sequence in row r at their sequence positions.  For a row r:
 *     L  = clamp(lens[r], 0, max_len)           h[0 .. L) = hist[r][0 .. L)
 *     s0 = clamp(start[r], 0, L)                n = ngram[r]
 * No-repeat n-gram.  Off for n < 1 or n > ERGM_NGRAM_MAX; nothing is banned while L - s0 < n - 1.  Otherwise, with the
 * tail t = h[L-n+1 .. L-1] (empty for n = 1): for every i with s0 <= i and i + n - 1 <= L - 1 such that
 * h[i .. i+n-2] == t, the token h[i+n-1] is banned.  Only n-grams that lie wholly inside [s0, L) count; for n = 1
 * every token of h[s0 .. L) is banned.  This is Hugging Face's NoRepeatNGramLogitsProcessor over [s0, L).
 * Bad words.  bad is int32 [R][ld_bad]; a row is a run of sequences, each a length m followed by its m tokens
 * w_0 .. w_{m-1}, 1 <= m <= ERGM_NGRAM_MAX.  The run ends at a length outside [1, ERGM_NGRAM_MAX] (0 is the usual
 * terminator), at a sequence the pool cuts off (its last token would lie at or past ld_bad), or at ld_bad.  The token
 * w_{m-1} is banned when m - 1 <= L and h[L-m+1 .. L-1] == w[0 .. m-2]: the match runs over the whole history, not
 * from s0, and a one-token sequence is always banned.
 * Both.  A banned token j with 0 <= j < V and j != eos_id gets logits[r][j] = -inf.  eos_id is never banned, so a
 * sequence can always end.  History entries and list tokens outside [0, V) ban nothing and match nothing but
 * themselves (the compares are on the int32 values).  Logits are never read; columns >= V, rows with both rules off
 * and rows whose finished flag is set are not touched, bit for bit.  start, ngram and bad may each be NULL: off (s0 =
 * 0).  lens, start, ngram and the list contents are device data and may hold anything: every value is clamped or
 * compared as above before it forms an address.  One workgroup per row, the history staged in LDS; a ban is a plain
 * 4-byte store of one value, so there are no atomics and every run gives the same bits, and applying twice equals
 * applying once.
 * Consumers.  ergm_sample_rows and ergm_beam_select treat -inf as "no mass / no candidate", so the ban precedes every
 * other step of the sampler (the penalty, the minimum length, ...) and the returned logprob is under the distribution
 * renormalised over the tokens still allowed.  A beam candidate's value is likewise normalised over the tokens its
 * beam may still take: this deviates from Hugging Face, which masks after the log-softmax and so keeps the banned
 * tokens' mass in the denominator.  A row in which every token with mass is banned (n = 1 with a history that covers
 * the vocabulary but for eos, whose own mass floors to 0) is the caller's problem: the sampler then falls back as it
 * does for any row without mass (it returns a token inside [0, V), ergm_sample_rows), a beam offers no candidate and
 * ergm_beam_select ends the rows it cannot fill (score -inf, finished, eos_id).  No index leaves a table.
 * ERGM_EINVAL before any launch: a NULL logits / rules / lens / hist, R outside [1, 65,535], V outside [1, 53,248]
 * (the sampler's bound), ldl < V, max_len outside [1, 1,024], ld_hist < max_len, eos_id outside [0, V), bad with
 * ld_bad < 1.  With ngram and bad both NULL nothing is launched.
 *
 * History upkeep.  ergm_hist_write: the packed ids of an admission or an extension (ergm_sample_mark's slot / start /
 * len over device int64 ids [total], clamped the same way) go to hist[slot[b]][pos0[b] ..), pos0 (device int [n_seq],
 * NULL: 0) clamped to [0, max_len] and the length to what is left before max_len; a slot outside [0, n_slots) writes
 * nothing; an id that is no int32 is stored as -1.  ergm_hist_append: a row that is not finished (finished may be
 * NULL) records tokens[r] at hist[r][lens[r]] when 0 <= lens[r] < max_len: called behind the sampler or the select and
 * before the step advances the length.  ergm_hist_follow: for every row that ergm_beam_gather moves (parent[r] != r,
 * parent[r] in the row's own group and keeping its own row), positions [0, clamp(lens[parent[r]], 0, max_len)) of row
 * parent[r] go to row r; sources keep their row, so the copy is safe in place, and lens is not written (it may run
 * before or behind the gather).
 *
 * ergm_decode_set_rules(plan, rules): the struct is copied, NULL turns the rules off (works on an unbound plan;
 * ERGM_EINVAL for a NULL hist, ld_hist < the plan's max_len or a max_len above 1,024).  While set,
 * ergm_decode_run_slots_sampled runs ergm_logit_rules_apply over all slots before each ergm_sample_rows and
 * ergm_hist_append behind it (2 launches more per round), and ergm_decode_run_beams runs ergm_logit_rules_apply before
 * each select and ergm_hist_follow, ergm_hist_append behind the gather (3 more).  When not set both enqueue what they
 * always did; the caller, who knows whether any occupied row has a rule, sets and clears it.                        */
#define ERGM_NGRAM_MAX 8
typedef struct {
    int32_t* hist;       /* [R][ld_hist] */
    int ld_hist;
    const int* start;    /* [R] s0, NULL: 0 */
    const int* ngram;    /* [R] n, NULL: the n-gram rule is off */
    const int32_t* bad;  /* [R][ld_bad] length-prefixed sequences, NULL: no bad words */
    int ld_bad;
} ergm_logit_rules;
int ergm_logit_rules_apply(float* logits, int ldl, int R, int V, const ergm_logit_rules* rules, const int* lens,
                           const uint8_t* finished, int64_t eos_id, int max_len, void* stream);
int ergm_hist_write(const int64_t* ids, int total, const int* slot, const int* start, const int* len, const int* pos0,
                    int n_seq, int n_slots, int32_t* hist, int ld_hist, int max_len, void* stream);
int ergm_hist_append(const int64_t* tokens, const int* lens, const uint8_t* finished, int R, int32_t* hist, int ld_hist,
                     int max_len, void* stream);
int ergm_hist_follow(int32_t* hist, int ld_hist, const int* parent, const int* lens, int R, int W, int max_len,
                     void* stream);
int ergm_decode_set_rules(ergm_decode_plan* plan, const ergm_logit_rules* rules);

/* ---- Scoring given tokens (found by symbol, ABI unchanged) ---------------------------------------------------------
 * ergm_lm_score: the tied LM head and the log-softmax of R rows in one pass; no logits are written.  For row r and the
 * columns j < V, x_j = Σ_k X[r][k]·W[j][k] (bf16 operands, f32 accumulation, never rounded to bf16), and
 *     lse[r]        = m + logf(Σ_j expf(x_j - m)), m the row's largest logit,
 *     top1[r]       = the column of the largest x_j, ties to the lowest column; top1_logit[r] = its value,
 *     logprob[r]    = x_target - lse, or exactly 0.0f when targets[r] lies outside [0, V) (the row is not scored; its
 *                     lse and top1 are still written).
 * X: bf16 [R][ldx], the ln_f rows; W: bf16 [>= V rows][ldw] (ERGM_NK), the tied head.  Rows of W at or past V (the pad
 * of vocab_pad) never contribute whatever they hold, NaN included, and rows of X at or past R are never read.  Any of
 * the four outputs may be NULL.  The vocabulary is cut into partitions of 512 columns, a function of V alone; a
 * workgroup runs an online softmax over one partition for 64 rows and leaves one (max, Σexp, argmax) per row, and a
 * second launch folds the partitions in ascending order.  No atomics: the same bits in every run, and a row's outputs
 * are bitwise the same whatever other rows the call holds and wherever the row sits.
 * workspace: 16-byte aligned, at least ergm_lm_score_workspace_size(R, V, K) = (3·ceil(V / 512) + 1)·R·4 bytes (0 for
 * dimensions the call rejects).  ERGM_EINVAL before any launch unless R >= 1, 1 <= V <= 65,536, K a positive multiple
 * of 64, ldx and ldw >= K and multiples of 8, X and W 16-byte aligned, and for a NULL X / W / targets or a short
 * workspace.                                                                                                        */
size_t ergm_lm_score_workspace_size(int R, int V, int K);
int ergm_lm_score(const void* X, int ldx, const void* W, int ldw, const int64_t* targets, int R, int V, int K,
                  float* logprob, float* lse, float* top1_logit, int* top1, void* workspace, size_t ws_bytes,
                  void* stream);

/* ergm_decode_score: teacher-forced scoring of n_seq given sequences, the admission's walk with the slots left out:
 * ergm_embed_packed; per layer ergm_layernorm_fwd / ergm_gemm (split_k = 0) over the R = Σ n_b packed rows, ragged causal
 * attention (ergm_attn_fwd_ragged alone: no K | V row goes to a slot), the caption K | V GEMM over the Rc = Σ c_b packed
 * caption rows, read in place by the ragged cross-attention, the MLP; then ln_f over all R rows and ergm_lm_score against
 * `targets` with V = vocab.  Engine 0's kernels whatever engine the plan is set to.  It reads and writes no cache, no
 * lens, no finished flag and no logits: the plan needs no bind, and with slots bound it may be called between steps
 * while requests are live or parked.  12 launches per block + 4 when no GEMM splits, whatever n_seq is.
 *   lens (= n_b), cap_lens: HOST int [n_seq], checked here; ERGM_EINVAL before any launch for n_seq outside
 *     [1, max_batch], n_b < 2 (no position to score), n_b > n_positions, c_b outside [1, cap_max], a vocabulary above
 *     65,536, a NULL lens / cap_lens / meta / ids / cap_ids / targets / workspace, or more packed rows than the workspace
 *     holds.
 *   meta: DEVICE int [ERGM_ADMIT_META_ROWS][n_seq] in ergm_decode_admit's layout; rows 0, 5 and 6 are ignored.
 *   ids, token_types (may be NULL), cap_ids, vis / aud, has_feat: as ergm_decode_admit takes them.
 *   targets: device int64 [R], the token each packed row is scored against, or a value outside [0, vocab) for a row that
 *     is not scored (the caller shifts: row s of a sequence holds its token s + 1, the last row none).
 *   logprob: device f32 [R], log p(target | the row's prefix), exactly 0 for a row not scored; top1: device int32 [R], the
 *     model's most probable token at every row.  Either may be NULL.
 *   workspace: 256-byte aligned, at least ergm_decode_score_workspace_size(dims, max_rows, max_cap_rows) bytes for any call
 *     of at most that many rows (0 for dimensions or row counts it rejects: max_rows <= max_batch · n_positions,
 *     max_cap_rows <= max_batch · cap_max); linear in the rows, nothing of size R x vocab.
 * ergm_decode_score_launches: the kernel launches of one such call, counted by walking its launch sequence dry; host only. */
size_t ergm_decode_score_workspace_size(const ergm_decode_dims* dims, int max_rows, int max_cap_rows);
int ergm_decode_score(ergm_decode_plan* plan, int n_seq, const int* lens, const int* cap_lens, const int* meta,
                      const int64_t* ids, const int64_t* token_types, const int64_t* cap_ids, const float* vis,
                      const float* aud, const uint8_t* has_feat, const int64_t* targets, float* logprob, int* top1,
                      void* workspace, size_t ws_bytes, void* stream);
int ergm_decode_score_launches(const ergm_decode_plan* plan, int n_seq, int rows, int cap_rows);

/* ---- Session store: a slot's state as one blob in HBM (found by symbol, ABI unchanged) -------------------------------
 * A parked conversation leaves its cache slot as one compact blob and returns into any free slot.  What travels is the
 * state of one slot: rows [0, n) of every layer's self-attention K | V, rows [0, c) of every layer's caption K | V, the
 * draw counters, with ERGM_SESSION_CTL the slot's sampling controls and its whole `seen` row, with ERGM_SESSION_RULES the
 * slot's rule values, its bad-word pool row and hist[slot][0 .. n).  n and c are the host's record of the rows the slot
 * holds; the kernels clamp them to [0, max_len] / [0, cap_max] before an address is formed.  The logits do not travel.
 *
 * Blob layout (little endian; every section starts on a 16-byte boundary, padding bytes are written as 0):
 *     0    header, 64 bytes = 16 words: magic "ERGS" 0x53475245 | version 1 | flags | n_layer | row_bytes | n | c |
 *          row_ids[slot] | row_steps[slot] | ld_seen (0 without CTL) | bad_cap (0 without RULES) | 0 |
 *          blob bytes, low word | high word | 0 | 0
 *     64   self-attention K | V: layer l's row i at 64 + (l·n + i)·row_bytes
 *          caption K | V behind it: layer l's row i at 64 + n_layer·n·row_bytes + (l·c + i)·row_bytes
 *     CTL  8 words: top_p | temperature | rep_penalty (f32 bits) | top_k | min_step | 0 | 0 | 0;
 *          then the seen row: ld_seen words, padded to 16 bytes
 *     RULES 4 words: start | ngram | 0 | 0; then the pool row: bad_cap words padded to 16 bytes; then hist[slot][0 .. n):
 *          n words padded to 16 bytes
 * ergm_session_bytes: the blob's size, a multiple of 16; 0 for arguments it rejects (n_layer, rows, cap_rows < 1,
 * row_bytes no positive multiple of 16, flags outside ERGM_SESSION_CTL | ERGM_SESSION_RULES, CTL with ld_seen < 1, RULES
 * with bad_cap < 1; ld_seen / bad_cap are ignored without their flag).  Host only, as is ergm_session_header, which
 * fills the caller's host copy of a header (row_ids / row_steps, which only the device knows, are left 0).
 *
 * ergm_session_state: the bound buffers.  kv / xkv: HOST arrays of n_layer device pointers, slot s of layer l at
 * kv[l] + s·kv_ld_seq, its row i at + i·kv_ld_row (bytes, multiples of 16; ergm_beam_gather's layout), row_bytes each;
 * the slot-state arrays of ergm_decode_bind_slots; ctl / rules: NULL, or the generator's per-slot arrays, every pointer of
 * them set (they are written by a load; ld_seen words of a seen row and ld_bad words of a pool row travel).
 *
 * ergm_slots_save packs n_seq slots into n_seq blobs, session b of slot slots[b] with rows[b] / cap_rows[b] rows and the
 * sections flags[b] names, and leaves each slot idle: finished = 1, lens = 0, cap_lens = 0; a slot saved with RULES also
 * gets start = ngram = 0 and a zero pool row, so the next tenant inherits no rule.  ergm_slots_load unpacks blobs into
 * slots: lens = n, cap_lens = c, stop_lens = n, finished = 1 (the parked state), row_steps, the controls and the rule
 * values from the blob, row_ids from the blob or, when row_ids is given (device uint32 [n_seq]), from that array (a fork
 * draws under its own id).  A blob without RULES loaded under a state with rules leaves start = ngram = 0 and a zero pool
 * row.  A load writes nothing at or past row n / c of a cache, nothing of hist at or past n, nothing in another slot.
 * hdrs: the caller's HOST copies of the blobs' headers, checked against `state` here; the device header supplies only
 * the draw counters, which form no address.
 *   meta_dev: DEVICE int64 [ERGM_SESSION_META_ROWS][n_seq]: slot | rows | cap_rows | blob address | flags | blob bytes,
 *     the host arguments again for the kernels.  rows / cap_rows are clamped and flags masked by what `state` has; a
 *     slot outside [0, max_batch), a zero address, or clamped sizes that give a blob above the stated bytes make the
 *     kernels skip the session: no value makes a kernel follow an index out of a table or past the end of a blob.  The
 *     blob address itself is followed as any pointer argument is.
 * Kernels: a workgroup per (session, layer, 64-row chunk), a wave per cache row, 16 bytes per lane, the layer pointers in
 * the kernel arguments (48 per launch), and one state kernel of a workgroup per session: 3 launches for up to 48 layers
 * whatever n_seq is (ergm_session_launches).  Plain loads and stores, no atomics; one stream, nothing read back.
 * ERGM_EINVAL before any launch: n_seq outside [1, max_batch]; a slot outside [0, max_batch) or named twice; rows outside
 * [1, max_len]; cap_rows outside [1, cap_max]; flags naming a section `state` lacks (CTL also when `state` has controls
 * and the flag is missing); a blob below ergm_session_bytes, NULL, not 16-byte aligned or (save) named twice; on load a
 * header whose magic, version, n_layer, row_bytes, flags, ld_seen, bad_cap or size disagree with `state`; strides or
 * row_bytes that are no multiples of 16 or shorter than the rows they span; a NULL or misaligned pointer.             */
#define ERGM_SESSION_CTL 1
#define ERGM_SESSION_RULES 2
#define ERGM_SESSION_META_ROWS 6
#define ERGM_SESSION_MAGIC 0x53475245u
typedef struct {
    uint32_t magic, version, flags;
    int32_t n_layer, row_bytes, rows, cap_rows;
    uint32_t row_id, row_steps;
    int32_t ld_seen, bad_cap, reserved0;
    uint64_t bytes;
    uint32_t reserved1[2];
} ergm_session_hdr; /* 64 bytes */
typedef struct {
    void* const* kv;
    void* const* xkv;
    int n_layer;
    int row_bytes;
    int64_t kv_ld_seq, kv_ld_row, xkv_ld_seq, xkv_ld_row;
    int max_batch, max_len, cap_max;
    int* lens;
    int* cap_lens;
    int* stop_lens;
    uint8_t* finished;
    uint32_t* row_ids;
    uint32_t* row_steps;
    const ergm_sample_ctl* ctl;     /* NULL: no control section */
    const ergm_logit_rules* rules;  /* NULL: no rule section */
} ergm_session_state;
size_t ergm_session_bytes(int n_layer, int row_bytes, int rows, int cap_rows, int ld_seen, int bad_cap, int flags);
int ergm_session_header(int n_layer, int row_bytes, int rows, int cap_rows, int ld_seen, int bad_cap, int flags,
                        ergm_session_hdr* out);
int ergm_session_launches(int n_layer);
int ergm_slots_save(const ergm_session_state* state, int n_seq, const int* slots, const int* rows, const int* cap_rows,
                    const int* flags, void* const* blobs, const size_t* blob_bytes, const int64_t* meta_dev, void* stream);
int ergm_slots_load(const ergm_session_state* state, int n_seq, const int* slots, const ergm_session_hdr* hdrs,
                    void* const* blobs, const size_t* blob_bytes, const uint32_t* row_ids, const int64_t* meta_dev,
                    void* stream);

/* Library information and errors. */
int ergm_version(void);
int ergm_last_error(char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* ERGM_HIP_H */
