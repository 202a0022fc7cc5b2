// Native decode executor (ergm_hip.h, ergm_decode_*): BatchedGenerator.step and the sampling loop of
// BatchedGenerator.generate (ergm_amd/generate.py) as launch sequences on the caller's one stream.
//
// Every kernel goes through Walk::on, which counts the launch and, in a dry walk, returns before calling anything, so
// the *_launches queries report what the live calls enqueue.  The transformer block is written once (block): its
// LayerNorms and GEMMs run on a set of row buffers (Bufs), and the mode supplies the stages that differ, the
// self-attention with its cache write, the caption K | V and the cross-attention.  Engine 0 calls the C-ABI entry
// points the Python path calls, with its arguments; engine 1 puts ergm_linear_rows in the place of each LayerNorm +
// GEMM pair and each plain GEMM of the blocks.
//
// Three modes run the block: the step (walk: one row per sequence over the bound caches), and in slot mode
// (ergm_decode_bind_slots, serving ContinuousGenerator, where the step runs over all max_batch slots and ends with
// the slot length update) the admission of new sequences into free slots (walk_admit: the prefill over packed ragged
// rows) and the extension of occupied slots by more than one token (walk_extend: packed new rows over the slots' own
// caches).  Those two share the blocks on engine 0 (walk_blocks) and the head tail (walk_packed).  A fourth walk binds
// nothing: ergm_decode_score (walk_score) runs the admission's packed rows through walk_blocks with the slot copies
// left out and ends in ln_f over every row and ergm_lm_score.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"

namespace ergm {
int decode_lens_advance(int* lens, const uint8_t* finished, int B, hipStream_t s);
int decode_fill_i64(int64_t* p, int64_t v, int n, hipStream_t s);
int attn_decode_launches(int B, int H, int max_len);
int decode_slots_admit(const int* slot, const int* n_tok, const int* n_cap, const int* max_new, const uint32_t* req, int n_seq,
                       int n_slots, int max_len, int cap_max, int* lens, int* cap_lens, int* stop_lens, uint32_t* row_ids,
                       uint32_t* row_steps, uint8_t* finished, hipStream_t s);
int decode_slots_advance(int* lens, uint32_t* row_steps, uint8_t* finished, const int* stop_lens, int B, hipStream_t s);
int decode_slots_extend(const int* slot, const int* past, const int* n_new, const int* max_new, int n_seq, int n_slots,
                        int max_len, int* lens, int* stop_lens, uint8_t* finished, hipStream_t s);
int beam_select_launches();
int beam_gather_launches(int n_layer);
int lm_score_launches();

// The row buffers a block runs on, for some number of rows R.
struct Bufs {
    float* h;        // [R][E] the residual stream
    __bf16* x;       // [R][E] LayerNorm output (engine 0, and the head)
    __bf16* qkv;     // [R][3E]
    __bf16* att;     // [R][E] attention output
    __bf16* q;       // [R][E] cross-attention query
    __bf16* pre;     // [R][F] gelu' (engine 0: the Python path's aux_out)
    __bf16* act;     // [R][F]
    float *mean, *rstd;  // [R]
    void* gemm_ws;
    size_t gemm_ws_bytes;
};
}  // namespace ergm

using namespace ergm;

struct ergm_decode_plan {
    ergm_decode_dims d;
    ergm_model_params p;
    // workspace
    Bufs b;          // max_batch rows: the step's
    int64_t* tt;     // [max_batch] ergm_decode_run's token types
    void* attn_ws;
    size_t attn_ws_bytes;
    // bound state
    bool bound;
    int B, n_max, Sc, engine;
    int head_lr;     // measurement switch ERGM_DECODE_HEAD (engine 1 only): 0 = ergm_gemm, 1 = lr, 2 = ln
    std::vector<void*> kv, xkv;
    int* lens;
    const int* cap_lens;
    uint8_t* finished;
    float* logits;
    // slot mode (ergm_decode_bind_slots): every step runs over all max_batch slots
    bool slots;
    int* cap_lens_rw;
    int* stop_lens;
    uint32_t* row_ids;
    uint32_t* row_steps;
    // logit rules (ergm_decode_set_rules): applied by the sampled slot loop and the beam loop while set
    bool ruled;
    ergm_logit_rules rules;
};

namespace {

constexpr int kEngines = 2;

size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

bool dims_ok(const ergm_decode_dims& d) {
    return d.n_embd > 0 && d.n_head > 0 && d.n_embd == 64 * d.n_head && d.n_embd <= 1024 && d.n_inner > 0 &&
           d.n_inner % 64 == 0 && d.vocab > 0 && d.vocab_pad >= d.vocab && d.vocab_pad % 64 == 0 && d.n_layer > 0 &&
           d.max_batch > 0 && d.max_len > 0 && d.max_len <= d.n_positions && d.cap_max > 0;
}

// C [M][N] packed (ldc = N), as every GEMM of the executor writes it
ergm_gemm_desc gemm_desc(int M, int N, int K, int b_layout, int c_dtype, int epi, const float* bias, const void* aux,
                         void* aux_out) {
    ergm_gemm_desc g{};
    g.M = M, g.N = N, g.K = K;
    g.lda = K, g.ldb = b_layout == ERGM_KN ? N : K, g.ldc = N;
    g.a_layout = ERGM_MK, g.b_layout = b_layout, g.c_dtype = c_dtype, g.epilogue = epi;
    g.alpha = 1.0f;
    g.bias = bias;
    g.aux = aux, g.ld_aux = aux ? N : 0;
    g.aux_out = aux_out, g.ld_aux_out = aux_out ? N : 0;
    return g;
}

// The largest split-K workspace of a walk's GEMMs: over every row count up to (R block rows, Rc caption rows,
// max_batch head rows), so that a workspace sized for R rows serves every smaller call; or (n_seq > 0) of the one call
// of exactly R rows, Rc caption rows and n_seq sequences, which the first covers.  The step's is (max_batch, 0, 0).
size_t gemm_ws_need(const ergm_decode_dims& d, int R, int Rc, int n_seq) {
    const int E = d.n_embd, F = d.n_inner;
    size_t need = 0;
    auto upto = [&](int rows, int N, int K, int b_layout) {
        for (int M = n_seq > 0 ? rows : 1; M <= rows; ++M) {
            const ergm_gemm_desc g = gemm_desc(M, N, K, b_layout, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr, nullptr);
            need = std::max(need, ergm_gemm_workspace_size(&g));
        }
    };
    upto(R, 3 * E, E, ERGM_KN), upto(R, E, E, ERGM_KN), upto(R, F, E, ERGM_KN), upto(R, E, F, ERGM_KN);
    upto(Rc, 2 * E, E, ERGM_KN);
    upto(n_seq > 0 ? n_seq : d.max_batch, d.vocab_pad, E, ERGM_NK);
    return need;
}

// Hands out 256-byte aligned pieces of a workspace; base == nullptr only sizes it.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t n) {
        char* p = base ? base + off : nullptr;
        off += al256(n * sizeof(T));
        return reinterpret_cast<T*>(p);
    }
};

// The block's buffers for R rows; x, mean and rstd for x_rows >= R (the admission's head runs max_batch rows at most).
void carve_rows(Carver& c, Bufs& b, size_t R, size_t x_rows, size_t E, size_t F) {
    b.h = c.take<float>(R * E);
    b.x = c.take<__bf16>(x_rows * E);
    b.qkv = c.take<__bf16>(R * 3 * E);
    b.att = c.take<__bf16>(R * E);
    b.q = c.take<__bf16>(R * E);
    b.pre = c.take<__bf16>(R * F);
    b.act = c.take<__bf16>(R * F);
    b.mean = c.take<float>(x_rows);
    b.rstd = c.take<float>(x_rows);
}

void carve_gemm_ws(Carver& c, Bufs& b, size_t need) {
    b.gemm_ws_bytes = std::max<size_t>(16, need);
    b.gemm_ws = c.take<char>(b.gemm_ws_bytes);
}

// Carves the plan's workspace; base == nullptr only sizes it.
size_t carve(ergm_decode_plan* P, char* base) {
    const ergm_decode_dims& d = P->d;
    Carver c{base};
    carve_rows(c, P->b, d.max_batch, d.max_batch, d.n_embd, d.n_inner);
    P->tt = c.take<int64_t>(d.max_batch);
    P->attn_ws_bytes = std::max<size_t>(16, ergm_attn_decode_workspace_size(d.max_batch, d.n_head, std::max(d.max_len, d.cap_max)));
    P->attn_ws = c.take<char>(P->attn_ws_bytes);
    carve_gemm_ws(c, P->b, gemm_ws_need(d, d.max_batch, 0, 0));
    return c.off;
}

// ---- slot mode: the workspace of an admission or an extension ------------------------------------------------
// The buffers of one call of at most R packed token rows and Rc packed caption rows, carved from the caller's
// workspace like the plan's own.
struct AdmitWs {
    Bufs b;         // R rows
    __bf16* cap;    // [Rc][E] caption embeddings
    __bf16* ckv;    // [Rc][2E] caption K | V of one layer
    float* hl;      // [max_batch][E] the last row of every sequence
    float* lg;      // [max_batch][vocab_pad] their logits, before they go to the slots
};

size_t admit_carve(const ergm_decode_dims& d, int R, int Rc, int n_seq, AdmitWs* A, char* base) {
    const size_t mb = d.max_batch, E = d.n_embd;
    Carver c{base};
    carve_rows(c, A->b, R, std::max<size_t>(R, mb), E, d.n_inner);
    A->cap = c.take<__bf16>(Rc * E);
    A->ckv = c.take<__bf16>(Rc * 2 * E);
    A->hl = c.take<float>(mb * E);
    A->lg = c.take<float>(mb * (size_t)d.vocab_pad);
    carve_gemm_ws(c, A->b, gemm_ws_need(d, R, Rc, n_seq));
    return c.off;
}

// The buffers of one ergm_decode_score of R packed token rows and Rc packed caption rows: the block's rows, the caption
// rows, ergm_lm_score's partials.  No head rows and no logits.
size_t score_carve(const ergm_decode_dims& d, int R, int Rc, AdmitWs* A, void** lm_ws, size_t* lm_bytes, char* base) {
    const size_t E = d.n_embd;
    Carver c{base};
    carve_rows(c, A->b, R, R, E, d.n_inner);
    A->cap = c.take<__bf16>(Rc * E);
    A->ckv = c.take<__bf16>(Rc * 2 * E);
    A->hl = nullptr, A->lg = nullptr;
    *lm_bytes = ergm_lm_score_workspace_size(R, d.vocab, d.n_embd);
    *lm_ws = c.take<char>(*lm_bytes);
    // the block GEMMs at exactly R and Rc rows; the head term of gemm_ws_need is one row's, which they cover
    carve_gemm_ws(c, A->b, gemm_ws_need(d, R, Rc, 1));
    return c.off;
}

struct Walk {
    bool dry;
    const char* what;  // the entry point, for a refusal's text
    hipStream_t s = nullptr;
    int count = 0;
    // counts `launches` kernels; true when the caller should enqueue them
    bool on(int launches = 1) {
        count += launches;
        return !dry;
    }
};

const float* lf(const ergm_decode_plan* P, int l, int t) {
    return P->p.layer_f32 + (int64_t)l * P->p.layer_stride + P->p.layer_off[t];
}
const __bf16* lb(const ergm_decode_plan* P, int l, int t) {
    return reinterpret_cast<const __bf16*>(P->p.layer_b16) + (int64_t)l * P->p.layer_stride + P->p.layer_off[t];
}

int ln(const ergm_decode_plan* P, Walk& w, const Bufs& b, const float* in, int rows, const float* g, const float* beta) {
    if (!w.on()) return ERGM_OK;
    return ergm_layernorm_fwd(in, g, beta, b.x, b.mean, b.rstd, rows, P->d.n_embd, P->d.eps, w.s);
}

// ergm_gemm as ops.gemm calls it (split_k = 0, the workspace of its own query); ldb: 0 = the packed weight
int gemm(Walk& w, const Bufs& b, int M, int N, int K, const void* A, const void* W, int b_layout, void* C, int c_dtype, int epi,
         const float* bias, const void* aux, void* aux_out, int ldb = 0) {
    ergm_gemm_desc g = gemm_desc(M, N, K, b_layout, c_dtype, epi, bias, aux, aux_out);
    if (ldb) g.ldb = ldb;
    int cfg = 0, split = 1, flags = 0;
    ERGM_TRY(ergm_gemm_plan(&g, &cfg, &split, &flags));
    if (!w.on(split > 1 ? 2 : 1)) return ERGM_OK;
    const size_t need = ergm_gemm_workspace_size(&g);
    ERGM_CHECK_ARG(need <= b.gemm_ws_bytes, "%s: GEMM workspace %zu > %zu bytes (a GEMM override set after the workspace was sized)",
                   w.what, need, b.gemm_ws_bytes);
    return ergm_gemm(&g, A, W, C, b.gemm_ws, need, w.s);
}

int linear(const ergm_decode_plan* P, Walk& w, int M, int N, int K, const void* A, const float* gamma, const float* beta,
           const void* W, int w_layout, void* C, int epi, const float* bias, const float* aux) {
    if (!w.on()) return ERGM_OK;
    ergm_linear_rows_desc g{};
    g.M = M, g.N = N, g.K = K;
    g.lda = K, g.ldw = w_layout == ERGM_KN ? N : K, g.ldc = N;
    g.w_layout = w_layout, g.epilogue = epi;
    g.bias = bias;
    g.aux = aux, g.ld_aux = aux ? N : 0;
    g.ln_gamma = gamma, g.ln_beta = beta, g.ln_eps = P->d.eps;
    return ergm_linear_rows(&g, A, W, C, w.s);
}

// LayerNorm(h; ln tensors t_ln, t_ln+1) -> Conv1D (weight t_w, bias t_w+1) of block l, N columns, into bf16 C
int ln_linear(const ergm_decode_plan* P, Walk& w, const Bufs& b, int engine, int rows, int l, int t_ln, int t_w, int N, void* C,
              int epi) {
    const int E = P->d.n_embd;
    if (engine == 0) {
        ERGM_TRY(ln(P, w, b, b.h, rows, lf(P, l, t_ln), lf(P, l, t_ln + 1)));
        void* aux_out = epi == ERGM_EPI_BIAS_GELU ? b.pre : nullptr;
        return gemm(w, b, rows, N, E, b.x, lb(P, l, t_w), ERGM_KN, C, ERGM_BF16, epi, lf(P, l, t_w + 1), nullptr, aux_out);
    }
    return linear(P, w, rows, N, E, b.h, lf(P, l, t_ln), lf(P, l, t_ln + 1), lb(P, l, t_w), ERGM_KN, C, epi, lf(P, l, t_w + 1),
                  nullptr);
}

// h += A·W + bias (weight t_w of block l, K rows)
int proj_resid(const ergm_decode_plan* P, Walk& w, const Bufs& b, int engine, int rows, int l, int t_w, int K, const void* A) {
    const int E = P->d.n_embd;
    if (engine == 0)
        return gemm(w, b, rows, E, K, A, lb(P, l, t_w), ERGM_KN, b.h, ERGM_F32, ERGM_EPI_BIAS_RESID, lf(P, l, t_w + 1), b.h,
                    nullptr);
    return linear(P, w, rows, E, K, A, nullptr, nullptr, lb(P, l, t_w), ERGM_KN, b.h, ERGM_EPI_BIAS_RESID, lf(P, l, t_w + 1),
                  b.h);
}

// Block l over `rows` rows of b.h, the twelve stages of every mode in their one order.  The mode's stages are called
// with l: self_attn reads b.qkv, writes b.att and puts the new K | V rows into the cache; before_cross runs between the
// attention projection and ln_cross_attn (the admission's caption K | V); cross_attn reads b.q and writes b.att.  A
// stage reads P->kv / P->xkv only after w.on() returned true: a dry walk runs on plans that were never bound.
template <class Self, class Before, class Cross>
int block(const ergm_decode_plan* P, Walk& w, const Bufs& b, int engine, int rows, int l, Self&& self_attn,
          Before&& before_cross, Cross&& cross_attn) {
    const int E = P->d.n_embd, F = P->d.n_inner;
    ERGM_TRY(ln_linear(P, w, b, engine, rows, l, ERGM_T_LN1_W, ERGM_T_ATTN_W, 3 * E, b.qkv, ERGM_EPI_BIAS));
    ERGM_TRY(self_attn(l));
    ERGM_TRY(proj_resid(P, w, b, engine, rows, l, ERGM_T_APROJ_W, E, b.att));
    ERGM_TRY(before_cross(l));
    ERGM_TRY(ln_linear(P, w, b, engine, rows, l, ERGM_T_LNX_W, ERGM_T_XQ_W, E, b.q, ERGM_EPI_BIAS));
    ERGM_TRY(cross_attn(l));
    ERGM_TRY(proj_resid(P, w, b, engine, rows, l, ERGM_T_XPROJ_W, E, b.att));
    ERGM_TRY(ln_linear(P, w, b, engine, rows, l, ERGM_T_LN2_W, ERGM_T_FC_W, F, b.act, ERGM_EPI_BIAS_GELU));
    return proj_resid(P, w, b, engine, rows, l, ERGM_T_MPROJ_W, F, b.act);
}

int no_stage(int) { return ERGM_OK; }

// ---- the step ------------------------------------------------------------------------------------------------
// ergm_attn_decode of B queries over layer l of `caches`
int attn(const ergm_decode_plan* P, Walk& w, int B, const __bf16* qkv, int ld_qkv, const std::vector<void*>& caches, int l,
         int rows, const int* lens, int append) {
    const ergm_decode_dims& d = P->d;
    if (!w.on(attn_decode_launches(B, d.n_head, rows))) return ERGM_OK;
    __bf16* k = reinterpret_cast<__bf16*>(caches[l]);
    return ergm_attn_decode(qkv, ld_qkv, k, k + d.n_embd, (int64_t)rows * 2 * d.n_embd, 2 * d.n_embd, lens, B, d.n_head, rows,
                            append, 0, P->b.att, d.n_embd, P->attn_ws, P->attn_ws_bytes, w.s);
}

// One decode step for B sequences; a dry walk (w.dry) only counts.
int walk(const ergm_decode_plan* P, Walk& w, int engine, int B, const int64_t* tokens, const int64_t* tt) {
    const ergm_decode_dims& d = P->d;
    const Bufs& b = P->b;
    const int E = d.n_embd;
    if (w.on())
        ERGM_TRY(ergm_embed_rows(tokens, tt, P->lens, P->p.wte, P->p.wpe, b.h, B, E, d.vocab_pad, d.n_positions, w.s));
    auto self_attn = [&](int l) -> int { return attn(P, w, B, b.qkv, 3 * E, P->kv, l, d.max_len, P->lens, 1); };
    auto cross_attn = [&](int l) -> int { return attn(P, w, B, b.q, E, P->xkv, l, P->bound ? P->Sc : d.cap_max, P->cap_lens, 0); };
    for (int l = 0; l < d.n_layer; ++l) ERGM_TRY(block(P, w, b, engine, B, l, self_attn, no_stage, cross_attn));
    // The head stays ln_f + ergm_gemm on both engines: at N = vocab_pad ergm_gemm has hundreds of workgroups already and
    // measured 19 us against ergm_linear_rows' 41 us at B = 32 (139 us with the LayerNorm in the prologue, every strip
    // re-reading the rows).  ERGM_DECODE_HEAD=lr / ln, read when the plan is created, puts engine 1's head
    // on ergm_linear_rows behind ergm_layernorm_fwd / with the prologue, to repeat that measurement.
    const int head = engine == 1 ? P->head_lr : 0;
    if (head == 2) {
        ERGM_TRY(linear(P, w, B, d.vocab_pad, E, b.h, P->p.ln_f_w, P->p.ln_f_b, P->p.wte_b, ERGM_NK, P->logits, ERGM_EPI_NONE,
                        nullptr, nullptr));
    } else {
        ERGM_TRY(ln(P, w, b, b.h, B, P->p.ln_f_w, P->p.ln_f_b));
        if (head == 0)
            ERGM_TRY(gemm(w, b, B, d.vocab_pad, E, b.x, P->p.wte_b, ERGM_NK, P->logits, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr,
                          nullptr));
        else
            ERGM_TRY(linear(P, w, B, d.vocab_pad, E, b.x, nullptr, nullptr, P->p.wte_b, ERGM_NK, P->logits, ERGM_EPI_NONE,
                            nullptr, nullptr));
    }
    if (w.on())
        ERGM_TRY(P->slots ? decode_slots_advance(P->lens, P->row_steps, P->finished, P->stop_lens, B, w.s)
                          : decode_lens_advance(P->lens, P->finished, B, w.s));
    return ERGM_OK;
}

int step_ready(const ergm_decode_plan* P, int steps, const char* what) {
    ERGM_CHECK_ARG(P, "%s: null plan", what);
    ERGM_CHECK_ARG(P->bound, "%s: no state bound (ergm_decode_bind after the prefill)", what);
    ERGM_CHECK_ARG(P->n_max + steps <= P->d.max_len, "%s: KV cache full (%d rows used, %d step(s), max_len %d)", what,
                   P->n_max, steps, P->d.max_len);
    return ERGM_OK;
}

// ---- slot mode: the admission (ergm_decode_admit) and the extension (ergm_decode_extend) -------------------------
// What one admission or extension was called with; the launch sequence below reads nothing else.  An extension has
// no captions of its own (one caption row carved, none used) and no features.
struct Packed {
    int n_seq, R, Rc;            // sequences, packed token / caption rows
    int max_n, max_c, max_k;     // the longest chunk, caption and (extension) past + chunk
    const int* meta;             // device [ERGM_ADMIT_META_ROWS or ERGM_EXTEND_META_ROWS][n_seq]
    const int64_t *ids, *tt, *cap_ids;
    const float *vis, *aud;
    const uint8_t* has_feat;
    const int* pos;              // extension: device [R], the position of every packed row
    AdmitWs ws;
    const int* row(int i) const { return meta ? meta + (size_t)i * n_seq : nullptr; }
};

// The rows of the meta array a packed walk reads, by mode (ergm_hip.h lists them).
struct MetaRows {
    const int *slot, *q0, *qn, *c0, *cn, *max_new, *last, *ones, *iota;
};

// The blocks over the R packed rows the embedding left in ws.b.h, on engine 0 (LayerNorm + ergm_gemm, as the Python
// path): the loop the admission, the extension and the scoring walk share.  A dry walk (w.dry) only counts.
template <class Self, class Before, class Cross>
int walk_blocks(const ergm_decode_plan* P, Walk& w, const Packed& a, Self&& self_attn, Before&& before_cross, Cross&& cross_attn) {
    for (int l = 0; l < P->d.n_layer; ++l) ERGM_TRY(block(P, w, a.ws.b, 0, a.R, l, self_attn, before_cross, cross_attn));
    return ERGM_OK;
}

// The blocks and the head of an admission or an extension: the last row of every sequence -> ln_f -> the head ->
// logits[slot].
template <class Self, class Before, class Cross>
int walk_packed(const ergm_decode_plan* P, Walk& w, const Packed& a, const MetaRows& m, Self&& self_attn, Before&& before_cross,
                Cross&& cross_attn) {
    const ergm_decode_dims& d = P->d;
    const AdmitWs& W = a.ws;
    const int E = d.n_embd, n = a.n_seq;
    const int64_t h_row = (int64_t)E * 4, lg_row = (int64_t)d.vocab_pad * 4;  // bytes
    ERGM_TRY(walk_blocks(P, w, a, self_attn, before_cross, cross_attn));
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.b.h, h_row, m.last, m.ones, m.iota, n, a.R, 1, W.hl, h_row, h_row, (int)h_row, n, 1, w.s));
    ERGM_TRY(ln(P, w, W.b, W.hl, n, P->p.ln_f_w, P->p.ln_f_b));
    ERGM_TRY(gemm(w, W.b, n, d.vocab_pad, E, W.b.x, P->p.wte_b, ERGM_NK, W.lg, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr, nullptr));
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.lg, lg_row, m.iota, m.ones, m.slot, n, n, 1, P->logits, lg_row, lg_row, (int)lg_row,
                                    d.max_batch, 1, w.s));
    return ERGM_OK;
}

int walk_admit(const ergm_decode_plan* P, Walk& w, const Packed& a) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, H = d.n_head, R = a.R, Rc = a.Rc, n = a.n_seq;
    const AdmitWs& W = a.ws;
    const MetaRows m{a.row(0), a.row(1), a.row(2), a.row(3), a.row(4), a.row(5), a.row(7), a.row(8), a.row(9)};
    const int64_t kv_row = (int64_t)2 * E * 2;  // bytes of a K | V row
    if (w.on())
        ERGM_TRY(ergm_embed_packed(a.ids, a.tt, a.cap_ids, P->p.wte, P->p.wpe, a.vis, a.aud, a.has_feat, m.q0, m.qn, m.c0, m.cn, n,
                                   R, Rc, a.max_n, a.max_c, W.b.h, W.cap, E, E, d.vocab_pad, d.n_positions, w.s));
    auto self_attn = [&](int l) -> int {
        if (w.on())
            ERGM_TRY(ergm_attn_fwd_ragged(W.b.qkv, W.b.qkv + E, W.b.qkv + 2 * E, W.b.att, nullptr, m.q0, m.qn, m.q0, m.qn, n, H, R, R,
                                          a.max_n, a.max_n, 3 * E, 3 * E, 3 * E, E, 1, w.s));
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots(W.b.qkv + E, (int64_t)3 * E * 2, m.q0, m.qn, m.slot, n, R, a.max_n, P->kv[l],
                                        (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, d.max_batch, d.max_len, w.s));
        return ERGM_OK;
    };
    // layer l's columns of the stacked caption K | V weight [E][L·2E] (the view the Python path passes), to the slot
    auto caption_kv = [&](int l) -> int {
        ERGM_TRY(gemm(w, W.b, Rc, 2 * E, E, W.cap, reinterpret_cast<const __bf16*>(P->p.capkv_w_b) + (size_t)l * 2 * E, ERGM_KN,
                      W.ckv, ERGM_BF16, ERGM_EPI_BIAS, P->p.capkv_b + (size_t)l * 2 * E, nullptr, nullptr, d.n_layer * 2 * E));
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots(W.ckv, kv_row, m.c0, m.cn, m.slot, n, Rc, a.max_c, P->xkv[l], (int64_t)d.cap_max * kv_row,
                                        kv_row, (int)kv_row, d.max_batch, d.cap_max, w.s));
        return ERGM_OK;
    };
    auto cross_attn = [&](int) -> int {
        if (!w.on()) return ERGM_OK;
        return ergm_attn_fwd_ragged(W.b.q, W.ckv, W.ckv + E, W.b.att, nullptr, m.q0, m.qn, m.c0, m.cn, n, H, R, Rc, a.max_n, a.max_c,
                                    E, 2 * E, 2 * E, E, 0, w.s);
    };
    ERGM_TRY(walk_packed(P, w, a, m, self_attn, caption_kv, cross_attn));
    if (w.on())
        ERGM_TRY(decode_slots_admit(m.slot, m.qn, m.cn, m.max_new, reinterpret_cast<const uint32_t*>(a.row(6)), n, d.max_batch,
                                    d.max_len, d.cap_max, P->lens, P->cap_lens_rw, P->stop_lens, P->row_ids, P->row_steps,
                                    P->finished, w.s));
    return ERGM_OK;
}

int walk_extend(const ergm_decode_plan* P, Walk& w, const Packed& x) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, H = d.n_head, R = x.R, n = x.n_seq;
    const AdmitWs& W = x.ws;
    const MetaRows m{x.row(0), x.row(1), x.row(2), x.row(6), x.row(7), x.row(8), x.row(9), x.row(10), x.row(11)};
    const int *past = x.row(3), *k0 = x.row(4), *kn = x.row(5);
    const int64_t kv_row = (int64_t)2 * E * 2;  // bytes of a K | V row
    if (w.on())
        ERGM_TRY(ergm_embed_rows(x.ids, x.tt, x.pos, P->p.wte, P->p.wpe, W.b.h, R, E, d.vocab_pad, d.n_positions, w.s));
    // the new rows' K | V into rows past_b .. of their slots, then the queries over the whole slot
    auto self_attn = [&](int l) -> int {
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots_at(W.b.qkv + E, (int64_t)3 * E * 2, m.q0, m.qn, m.slot, past, n, R, x.max_n, P->kv[l],
                                           (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, d.max_batch, d.max_len, w.s));
        if (w.on()) {
            const __bf16* kv = reinterpret_cast<const __bf16*>(P->kv[l]);
            ERGM_TRY(ergm_attn_fwd_extend(W.b.qkv, kv, kv + E, W.b.att, m.q0, m.qn, k0, kn, n, H, R, d.max_batch * d.max_len,
                                          x.max_n, x.max_k, 3 * E, 2 * E, 2 * E, E, w.s));
        }
        return ERGM_OK;
    };
    // the caption rows the admission left in the slot: xkv[l] as packed rows, sequence b's at slot_b · cap_max
    auto cross_attn = [&](int l) -> int {
        if (!w.on()) return ERGM_OK;
        const __bf16* xkv = reinterpret_cast<const __bf16*>(P->xkv[l]);
        return ergm_attn_fwd_ragged(W.b.q, xkv, xkv + E, W.b.att, nullptr, m.q0, m.qn, m.c0, m.cn, n, H, R, d.max_batch * d.cap_max,
                                    x.max_n, x.max_c, E, 2 * E, 2 * E, E, 0, w.s);
    };
    ERGM_TRY(walk_packed(P, w, x, m, self_attn, no_stage, cross_attn));
    if (w.on())
        ERGM_TRY(decode_slots_extend(m.slot, past, m.qn, m.max_new, n, d.max_batch, d.max_len, P->lens, P->stop_lens, P->finished,
                                     w.s));
    return ERGM_OK;
}

// What ergm_decode_score adds to the packed call: the targets, the outputs and ergm_lm_score's workspace.
struct ScoreOut {
    const int64_t* targets;
    float* logprob;
    int* top1;
    void* lm_ws;
    size_t lm_bytes;
};

// The admission's walk with the slots left out: nothing bound is read or written.  The caption K | V of a layer stays
// in ws.ckv, where the cross-attention reads it; the tail is ln_f over all R rows and ergm_lm_score.
int walk_score(const ergm_decode_plan* P, Walk& w, const Packed& a, const ScoreOut& o) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, H = d.n_head, R = a.R, Rc = a.Rc, n = a.n_seq;
    const AdmitWs& W = a.ws;
    const int *q0 = a.row(1), *qn = a.row(2), *c0 = a.row(3), *cn = a.row(4);
    if (w.on())
        ERGM_TRY(ergm_embed_packed(a.ids, a.tt, a.cap_ids, P->p.wte, P->p.wpe, a.vis, a.aud, a.has_feat, q0, qn, c0, cn, n, R, Rc,
                                   a.max_n, a.max_c, W.b.h, W.cap, E, E, d.vocab_pad, d.n_positions, w.s));
    auto self_attn = [&](int) -> int {
        if (!w.on()) return ERGM_OK;
        return ergm_attn_fwd_ragged(W.b.qkv, W.b.qkv + E, W.b.qkv + 2 * E, W.b.att, nullptr, q0, qn, q0, qn, n, H, R, R, a.max_n,
                                    a.max_n, 3 * E, 3 * E, 3 * E, E, 1, w.s);
    };
    auto caption_kv = [&](int l) -> int {
        return gemm(w, W.b, Rc, 2 * E, E, W.cap, reinterpret_cast<const __bf16*>(P->p.capkv_w_b) + (size_t)l * 2 * E, ERGM_KN,
                    W.ckv, ERGM_BF16, ERGM_EPI_BIAS, P->p.capkv_b + (size_t)l * 2 * E, nullptr, nullptr, d.n_layer * 2 * E);
    };
    auto cross_attn = [&](int) -> int {
        if (!w.on()) return ERGM_OK;
        return ergm_attn_fwd_ragged(W.b.q, W.ckv, W.ckv + E, W.b.att, nullptr, q0, qn, c0, cn, n, H, R, Rc, a.max_n, a.max_c, E,
                                    2 * E, 2 * E, E, 0, w.s);
    };
    ERGM_TRY(walk_blocks(P, w, a, self_attn, caption_kv, cross_attn));
    ERGM_TRY(ln(P, w, W.b, W.b.h, R, P->p.ln_f_w, P->p.ln_f_b));
    if (w.on(lm_score_launches()))
        ERGM_TRY(ergm_lm_score(W.b.x, E, P->p.wte_b, E, o.targets, R, d.vocab, E, o.logprob, nullptr, nullptr, o.top1, o.lm_ws,
                               o.lm_bytes, w.s));
    return ERGM_OK;
}

bool score_rows_ok(const ergm_decode_dims& d, int max_rows, int max_cap_rows) {
    return max_rows >= 1 && max_cap_rows >= 1 && (int64_t)max_rows <= (int64_t)d.max_batch * d.n_positions &&
           (int64_t)max_cap_rows <= (int64_t)d.max_batch * d.cap_max && d.vocab <= 65536;
}

int slots_ready(const ergm_decode_plan* P, const char* what) {
    ERGM_CHECK_ARG(P, "%s: null plan", what);
    ERGM_CHECK_ARG(P->slots, "%s: no slots bound (ergm_decode_bind_slots)", what);
    return ERGM_OK;
}

// n_seq slots, each in range and none named twice
int slots_ok(const ergm_decode_dims& d, int n_seq, const int* slots, const char* what) {
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= d.max_batch, "%s: n_seq %d outside [1, max_batch %d]", what, n_seq, d.max_batch);
    std::vector<char> seen(d.max_batch, 0);
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(slots[b] >= 0 && slots[b] < d.max_batch, "%s: slot %d of sequence %d outside [0, max_batch %d)", what,
                       slots[b], b, d.max_batch);
        ERGM_CHECK_ARG(!seen[slots[b]], "%s: slot %d named twice", what, slots[b]);
        seen[slots[b]] = 1;
    }
    return ERGM_OK;
}

// every layer's caches and the logits, as both binds take them
int caches_ok(const ergm_decode_plan* P, void* const* kv, void* const* xkv, const float* logits, const char* what) {
    for (int l = 0; l < P->d.n_layer; ++l)
        ERGM_CHECK_ARG(kv[l] && xkv[l] && aligned16(kv[l]) && aligned16(xkv[l]),
                       "%s: layer %d cache pointer null or not 16-byte aligned", what, l);
    ERGM_CHECK_ARG(aligned16(logits), "%s: logits must be 16-byte aligned", what);
    return ERGM_OK;
}

bool admit_rows_ok(const ergm_decode_dims& d, int max_rows, int max_cap_rows) {
    return max_rows >= 1 && max_cap_rows >= 1 && (int64_t)max_rows <= (int64_t)d.max_batch * d.max_len &&
           (int64_t)max_cap_rows <= (int64_t)d.max_batch * d.cap_max;
}

// Carves this call's buffers (a.R, a.Rc, a.n_seq set) from the caller's workspace, refusing one that is too small.
int packed_carve(const ergm_decode_dims& d, Packed& a, void* workspace, size_t ws_bytes, const char* what) {
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", what);
    ERGM_CHECK_ARG(admit_rows_ok(d, a.R, a.Rc), "%s: bad row counts", what);
    const size_t need = admit_carve(d, a.R, a.Rc, a.n_seq, &a.ws, nullptr);  // this call alone
    ERGM_CHECK_ARG(ws_bytes >= need, "%s: %d packed rows and %d caption rows need a workspace of %zu bytes, %zu given", what, a.R,
                   a.Rc, need, ws_bytes);
    admit_carve(d, a.R, a.Rc, a.n_seq, &a.ws, reinterpret_cast<char*>(workspace));
    return ERGM_OK;
}
}  // namespace

extern "C" size_t ergm_decode_workspace_size(const ergm_decode_dims* dims) {
    if (!dims || !dims_ok(*dims)) return 0;
    ergm_decode_plan P{};
    P.d = *dims;
    return carve(&P, nullptr);
}

extern "C" int ergm_decode_create(const ergm_decode_dims* dims, const ergm_model_params* params, void* ws, size_t ws_bytes,
                                  ergm_decode_plan** out) {
    ERGM_CHECK_ARG(dims && params && ws && out, "decode_create: null argument");
    const ergm_decode_dims& d = *dims;
    ERGM_CHECK_ARG(d.n_embd > 0 && d.n_head > 0 && d.n_embd == 64 * d.n_head,
                   "decode_create: head_dim must be 64 (n_embd=%d n_head=%d)", d.n_embd, d.n_head);
    ERGM_CHECK_ARG(dims_ok(d), "decode_create: unsupported dimensions (n_embd <= 1024, n_inner %% 64, vocab_pad %% 64, "
                               "1 <= max_len <= n_positions, max_batch, cap_max, n_layer >= 1)");
    ERGM_CHECK_ARG(params->wte && params->wte_b && params->wpe && params->ln_f_w && params->ln_f_b && params->layer_f32 &&
                       params->layer_b16,
                   "decode_create: null forward parameter");
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "decode_create: workspace must be 256-byte aligned");
    const size_t need = ergm_decode_workspace_size(dims);
    ERGM_CHECK_ARG(ws_bytes >= need, "decode_create: workspace %zu < %zu bytes", ws_bytes, need);
    auto* P = new (std::nothrow) ergm_decode_plan();
    if (!P) return fail(ERGM_EINVAL, "decode_create: out of host memory");
    P->d = d;
    P->p = *params;
    carve(P, reinterpret_cast<char*>(ws));
    P->bound = false;
    P->B = P->n_max = P->Sc = P->engine = 0;
    P->head_lr = 0;
    if (const char* e = getenv("ERGM_DECODE_HEAD")) P->head_lr = !strcmp(e, "lr") ? 1 : (!strcmp(e, "ln") ? 2 : 0);
    P->lens = nullptr;
    P->cap_lens = nullptr;
    P->finished = nullptr;
    P->logits = nullptr;
    P->slots = false;
    P->cap_lens_rw = P->stop_lens = nullptr;
    P->row_ids = P->row_steps = nullptr;
    *out = P;
    return ERGM_OK;
}

extern "C" int ergm_decode_destroy(ergm_decode_plan* P) {
    delete P;
    return ERGM_OK;
}

extern "C" int ergm_decode_bind(ergm_decode_plan* P, int B, int n_max, void* const* kv, void* const* xkv, int Sc, int* lens,
                                const int* cap_lens, uint8_t* finished, float* logits) {
    ERGM_CHECK_ARG(P && kv && xkv && lens && cap_lens && finished && logits, "decode_bind: null argument");
    ERGM_CHECK_ARG(B >= 1 && B <= P->d.max_batch, "decode_bind: B %d outside [1, max_batch %d]", B, P->d.max_batch);
    ERGM_CHECK_ARG(n_max >= 1 && n_max <= P->d.max_len, "decode_bind: n_max %d outside [1, max_len %d]", n_max, P->d.max_len);
    ERGM_CHECK_ARG(Sc >= 1 && Sc <= P->d.cap_max, "decode_bind: Sc %d outside [1, cap_max %d]", Sc, P->d.cap_max);
    ERGM_TRY(caches_ok(P, kv, xkv, logits, "decode_bind"));
    P->kv.assign(kv, kv + P->d.n_layer);
    P->xkv.assign(xkv, xkv + P->d.n_layer);
    P->B = B, P->n_max = n_max, P->Sc = Sc;
    P->lens = lens, P->cap_lens = cap_lens, P->finished = finished, P->logits = logits;
    P->bound = true;
    P->slots = false;
    return ERGM_OK;
}

extern "C" int ergm_decode_set_engine(ergm_decode_plan* P, int engine) {
    ERGM_CHECK_ARG(P && engine >= 0 && engine < kEngines, "decode_set_engine: engine %d outside [0, %d)", engine, kEngines);
    P->engine = engine;
    return ERGM_OK;
}

extern "C" int ergm_decode_set_rules(ergm_decode_plan* P, const ergm_logit_rules* rules) {
    ERGM_CHECK_ARG(P, "decode_set_rules: null plan");
    if (!rules) {
        P->ruled = false;
        P->rules = ergm_logit_rules{};
        return ERGM_OK;
    }
    ERGM_CHECK_ARG(rules->hist && rules->ld_hist >= P->d.max_len && P->d.max_len <= 1024,
                   "decode_set_rules: null hist, ld_hist %d < max_len %d, or max_len above 1024", rules->ld_hist, P->d.max_len);
    ERGM_CHECK_ARG(!rules->bad || rules->ld_bad >= 1, "decode_set_rules: ld_bad %d < 1", rules->ld_bad);
    P->rules = *rules;
    P->ruled = rules->ngram || rules->bad;
    return ERGM_OK;
}

extern "C" int ergm_decode_step(ergm_decode_plan* P, const int64_t* tokens, const int64_t* token_types, void* stream) {
    ERGM_TRY(step_ready(P, 1, "decode_step"));
    ERGM_CHECK_ARG(tokens, "decode_step: null tokens");
    Walk w{false, "decode_step", as_stream(stream)};
    ERGM_TRY(walk(P, w, P->engine, P->B, tokens, token_types));
    P->n_max += 1;
    return ERGM_OK;
}

extern "C" int ergm_decode_run(ergm_decode_plan* P, int first, int n, float top_p, uint64_t seed, int64_t eos_id,
                               int64_t sp2_id, int64_t* tokens_out, void* stream) {
    ERGM_CHECK_ARG(P, "decode_run: null plan");
    ERGM_CHECK_ARG(n >= 1 && first >= 0 && first <= INT32_MAX - n, "decode_run: bad range first %d n %d", first, n);
    ERGM_TRY(step_ready(P, n - (first == 0 ? 1 : 0), "decode_run"));
    ERGM_CHECK_ARG(tokens_out, "decode_run: null tokens_out");
    ERGM_CHECK_ARG(top_p == top_p, "decode_run: top_p is NaN");
    hipStream_t s = as_stream(stream);
    const int B = P->B;
    ERGM_TRY(decode_fill_i64(P->tt, sp2_id, B, s));
    for (int i = first; i < first + n; ++i) {
        if (i > 0) {
            Walk w{false, "decode_step", s};
            ERGM_TRY(walk(P, w, P->engine, B, tokens_out + (size_t)(i - 1) * B, P->tt));
            P->n_max += 1;  // per step: after a launch failure part-way n_max counts the steps that were enqueued; the
                            // caller then rebinds (ergm_decode_bind sets n_max again) before it goes on
        }
        ERGM_TRY(ergm_topp_sample(P->logits, P->d.vocab_pad, B, P->d.vocab, top_p, seed, (uint32_t)i, P->finished, eos_id,
                                  tokens_out + (size_t)i * B, nullptr, nullptr, s));
    }
    return ERGM_OK;
}

// n rounds of beam search over the bound rows: select, gather, step (ergm_hip.h has the rule).
extern "C" int ergm_decode_run_beams(ergm_decode_plan* P, int n, int W, int64_t eos_id, int64_t sp2_id, float* scores,
                                     int64_t* tokens_out, int* parents_out, void* workspace, size_t ws_bytes, void* stream) {
    ERGM_CHECK_ARG(P, "decode_run_beams: null plan");
    ERGM_CHECK_ARG(!P->slots, "decode_run_beams: the plan is bound in slot mode (ergm_decode_bind_slots)");
    ERGM_CHECK_ARG(n >= 1, "decode_run_beams: n %d < 1", n);
    ERGM_CHECK_ARG(W >= 1 && W <= 8, "decode_run_beams: W %d outside [1, 8]", W);
    ERGM_TRY(step_ready(P, n, "decode_run_beams"));
    ERGM_CHECK_ARG(P->B % W == 0, "decode_run_beams: the %d bound rows are no multiple of W %d", P->B, W);
    ERGM_CHECK_ARG(W <= P->d.vocab && eos_id >= 0 && eos_id < P->d.vocab, "decode_run_beams: W %d or eos_id %lld outside the vocabulary",
                   W, (long long)eos_id);
    ERGM_CHECK_ARG(scores && tokens_out && parents_out && workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                   "decode_run_beams: null argument or workspace not 8-byte aligned");
    ERGM_CHECK_ARG(ws_bytes >= ergm_beam_select_workspace_size(P->B, W), "decode_run_beams: workspace %zu < %zu bytes", ws_bytes,
                   ergm_beam_select_workspace_size(P->B, W));
    hipStream_t s = as_stream(stream);
    const ergm_decode_dims& d = P->d;
    const int B = P->B;
    const int64_t kv_row = (int64_t)2 * d.n_embd * 2;  // bytes of a K | V row
    ERGM_TRY(decode_fill_i64(P->tt, sp2_id, B, s));
    for (int i = 0; i < n; ++i) {
        int64_t* tok = tokens_out + (size_t)i * B;
        int* par = parents_out + (size_t)i * B;
        Walk w{false, "decode_run_beams", s};
        if (P->ruled)
            ERGM_TRY(ergm_logit_rules_apply(P->logits, d.vocab_pad, B, d.vocab, &P->rules, P->lens, P->finished, eos_id, d.max_len, s));
        if (w.on(beam_select_launches()))
            ERGM_TRY(ergm_beam_select(P->logits, d.vocab_pad, B, W, d.vocab, scores, P->finished, eos_id, par, tok, workspace,
                                      ws_bytes, s));
        // n_max bounds every length: the gather's grid covers the rows in use, not the whole cache
        if (w.on(beam_gather_launches(d.n_layer)))
            ERGM_TRY(ergm_beam_gather(P->kv.data(), d.n_layer, (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, par, P->lens, B, W,
                                      P->n_max, s));
        if (P->ruled) {  // the histories follow the caches, then take the round's tokens
            ERGM_TRY(ergm_hist_follow(P->rules.hist, P->rules.ld_hist, par, P->lens, B, W, d.max_len, s));
            ERGM_TRY(ergm_hist_append(tok, P->lens, P->finished, B, P->rules.hist, P->rules.ld_hist, d.max_len, s));
        }
        ERGM_TRY(walk(P, w, P->engine, B, tok, P->tt));
        P->n_max += 1;
    }
    return ERGM_OK;
}

extern "C" int ergm_decode_bind_slots(ergm_decode_plan* P, void* const* kv, void* const* xkv, float* logits, int* lens,
                                      int* cap_lens, uint8_t* finished, int* stop_lens, uint32_t* row_ids,
                                      uint32_t* row_steps) {
    ERGM_CHECK_ARG(P && kv && xkv && logits && lens && cap_lens && finished && stop_lens && row_ids && row_steps,
                   "decode_bind_slots: null argument");
    ERGM_TRY(caches_ok(P, kv, xkv, logits, "decode_bind_slots"));
    P->kv.assign(kv, kv + P->d.n_layer);
    P->xkv.assign(xkv, xkv + P->d.n_layer);
    P->B = P->d.max_batch, P->n_max = 0, P->Sc = P->d.cap_max;
    P->lens = lens, P->cap_lens = P->cap_lens_rw = cap_lens, P->finished = finished, P->logits = logits;
    P->stop_lens = stop_lens, P->row_ids = row_ids, P->row_steps = row_steps;
    P->bound = false;  // ergm_decode_step / _run serve ergm_decode_bind
    P->slots = true;
    return ERGM_OK;
}

extern "C" size_t ergm_decode_admit_workspace_size(const ergm_decode_dims* dims, int max_rows, int max_cap_rows) {
    if (!dims || !dims_ok(*dims) || !admit_rows_ok(*dims, max_rows, max_cap_rows)) return 0;
    AdmitWs A{};
    return admit_carve(*dims, max_rows, max_cap_rows, 0, &A, nullptr);
}

extern "C" int ergm_decode_admit(ergm_decode_plan* P, int n_seq, const int* slots, const int* lens, const int* cap_lens,
                                 const int* max_new, const int* meta, const int64_t* ids, const int64_t* token_types,
                                 const int64_t* cap_ids, const float* vis, const float* aud, const uint8_t* has_feat,
                                 void* workspace, size_t ws_bytes, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_admit"));
    const ergm_decode_dims& d = P->d;
    ERGM_CHECK_ARG(slots && lens && cap_lens && max_new && meta && ids && cap_ids && workspace, "decode_admit: null argument");
    ERGM_TRY(slots_ok(d, n_seq, slots, "decode_admit"));
    ERGM_CHECK_ARG((vis == nullptr) == (aud == nullptr), "decode_admit: visual and audio features go together");
    ERGM_CHECK_ARG(P->p.capkv_w_b && P->p.capkv_b, "decode_admit: the plan was created without the caption K/V weights "
                   "(capkv_w_b, capkv_b)");
    Packed a{};
    int64_t R = 0, Rc = 0;
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(lens[b] >= 1, "decode_admit: sequence %d has an empty prompt (n_b %d < 1)", b, lens[b]);
        ERGM_CHECK_ARG(cap_lens[b] >= 1, "decode_admit: sequence %d has an empty caption (c_b %d < 1)", b, cap_lens[b]);
        ERGM_CHECK_ARG(cap_lens[b] <= d.cap_max, "decode_admit: caption of sequence %d has %d rows > cap_max %d", b, cap_lens[b],
                       d.cap_max);
        ERGM_CHECK_ARG(max_new[b] >= 1, "decode_admit: max_new %d of sequence %d < 1", max_new[b], b);
        ERGM_CHECK_ARG(lens[b] <= d.max_len && max_new[b] <= d.max_len - lens[b],
                       "decode_admit: sequence %d: n_b %d + max_new %d > max_len %d", b, lens[b], max_new[b], d.max_len);
        R += lens[b], Rc += cap_lens[b];
        a.max_n = std::max(a.max_n, lens[b]), a.max_c = std::max(a.max_c, cap_lens[b]);
    }
    a.n_seq = n_seq, a.R = (int)R, a.Rc = (int)Rc;
    ERGM_TRY(packed_carve(d, a, workspace, ws_bytes, "decode_admit"));
    a.meta = meta, a.ids = ids, a.tt = token_types, a.cap_ids = cap_ids;
    a.vis = vis, a.aud = aud, a.has_feat = has_feat;
    Walk w{false, "decode_admit", as_stream(stream)};
    return walk_admit(P, w, a);
}

extern "C" int ergm_decode_admit_launches(const ergm_decode_plan* P, int n_seq, int rows, int cap_rows) {
    ERGM_CHECK_ARG(P && n_seq >= 1 && n_seq <= P->d.max_batch && rows >= n_seq && cap_rows >= n_seq &&
                       admit_rows_ok(P->d, rows, cap_rows),
                   "decode_admit_launches: bad plan or counts (n_seq %d rows %d cap_rows %d)", n_seq, rows, cap_rows);
    Packed a{};
    a.n_seq = n_seq, a.R = rows, a.Rc = cap_rows, a.max_n = rows, a.max_c = cap_rows;
    // buffer addresses for the GEMM descriptors the walk plans (the plan's own workspace; nothing is launched)
    admit_carve(P->d, rows, cap_rows, n_seq, &a.ws, reinterpret_cast<char*>(P->b.h));
    Walk w{true, "decode_admit_launches"};
    ERGM_TRY(walk_admit(P, w, a));
    return w.count;
}

extern "C" int ergm_decode_extend(ergm_decode_plan* P, int n_seq, const int* slots, const int* past, const int* lens,
                                  const int* cap_lens, const int* max_new, const int* meta, const int64_t* ids,
                                  const int64_t* token_types, const int* pos, void* workspace, size_t ws_bytes, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_extend"));
    const ergm_decode_dims& d = P->d;
    ERGM_CHECK_ARG(slots && past && lens && cap_lens && max_new && meta && ids && pos && workspace, "decode_extend: null argument");
    ERGM_TRY(slots_ok(d, n_seq, slots, "decode_extend"));
    Packed x{};
    int64_t R = 0;
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(lens[b] >= 1, "decode_extend: sequence %d gets no new token (n_b %d < 1)", b, lens[b]);
        ERGM_CHECK_ARG(past[b] >= 2, "decode_extend: sequence %d has a past of %d rows < 2 (positions 0 and 1 belong to the "
                       "admission)", b, past[b]);
        ERGM_CHECK_ARG(cap_lens[b] >= 1 && cap_lens[b] <= d.cap_max, "decode_extend: caption of sequence %d has %d rows outside "
                       "[1, cap_max %d]", b, cap_lens[b], d.cap_max);
        ERGM_CHECK_ARG(max_new[b] >= 1, "decode_extend: max_new %d of sequence %d < 1", max_new[b], b);
        ERGM_CHECK_ARG(past[b] <= d.max_len && lens[b] <= d.max_len - past[b] && max_new[b] <= d.max_len - past[b] - lens[b],
                       "decode_extend: sequence %d: past %d + n_b %d + max_new %d > max_len %d", b, past[b], lens[b], max_new[b],
                       d.max_len);
        R += lens[b];
        x.max_n = std::max(x.max_n, lens[b]), x.max_k = std::max(x.max_k, past[b] + lens[b]);
        x.max_c = std::max(x.max_c, cap_lens[b]);
    }
    x.n_seq = n_seq, x.R = (int)R, x.Rc = 1;
    ERGM_TRY(packed_carve(d, x, workspace, ws_bytes, "decode_extend"));
    x.meta = meta, x.ids = ids, x.tt = token_types, x.pos = pos;
    Walk w{false, "decode_extend", as_stream(stream)};
    return walk_extend(P, w, x);
}

extern "C" int ergm_decode_extend_launches(const ergm_decode_plan* P, int n_seq, int rows) {
    ERGM_CHECK_ARG(P && n_seq >= 1 && n_seq <= P->d.max_batch && rows >= n_seq && admit_rows_ok(P->d, rows, 1),
                   "decode_extend_launches: bad plan or counts (n_seq %d rows %d)", n_seq, rows);
    Packed x{};
    x.n_seq = n_seq, x.R = rows, x.Rc = 1, x.max_n = rows, x.max_k = P->d.max_len, x.max_c = P->d.cap_max;
    // buffer addresses for the GEMM descriptors the walk plans (the plan's own workspace; nothing is launched)
    admit_carve(P->d, rows, 1, n_seq, &x.ws, reinterpret_cast<char*>(P->b.h));
    Walk w{true, "decode_extend_launches"};
    ERGM_TRY(walk_extend(P, w, x));
    return w.count;
}

extern "C" size_t ergm_decode_score_workspace_size(const ergm_decode_dims* dims, int max_rows, int max_cap_rows) {
    if (!dims || !dims_ok(*dims) || !score_rows_ok(*dims, max_rows, max_cap_rows)) return 0;
    AdmitWs A{};
    void* lm = nullptr;
    size_t lmb = 0;
    // the block GEMMs' split-K workspace over every row count up to max_rows, as the admission sizes its own
    const size_t rows = score_carve(*dims, max_rows, max_cap_rows, &A, &lm, &lmb, nullptr) - al256(A.b.gemm_ws_bytes);
    return rows + al256(std::max<size_t>(16, gemm_ws_need(*dims, max_rows, max_cap_rows, 0)));
}

extern "C" int ergm_decode_score(ergm_decode_plan* P, int n_seq, const int* lens, const int* cap_lens, const int* meta,
                                 const int64_t* ids, const int64_t* token_types, const int64_t* cap_ids, const float* vis,
                                 const float* aud, const uint8_t* has_feat, const int64_t* targets, float* logprob, int* top1,
                                 void* workspace, size_t ws_bytes, void* stream) {
    ERGM_CHECK_ARG(P, "decode_score: null plan");
    const ergm_decode_dims& d = P->d;
    ERGM_CHECK_ARG(lens && cap_lens && meta && ids && cap_ids && targets && workspace, "decode_score: null argument");
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= d.max_batch, "decode_score: n_seq %d outside [1, max_batch %d]", n_seq, d.max_batch);
    ERGM_CHECK_ARG((vis == nullptr) == (aud == nullptr), "decode_score: visual and audio features go together");
    ERGM_CHECK_ARG(P->p.capkv_w_b && P->p.capkv_b, "decode_score: the plan was created without the caption K/V weights "
                   "(capkv_w_b, capkv_b)");
    ERGM_CHECK_ARG(d.vocab <= 65536, "decode_score: vocabulary %d > 65536 (ergm_lm_score)", d.vocab);
    Packed a{};
    int64_t R = 0, Rc = 0;
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(lens[b] >= 2, "decode_score: sequence %d has %d tokens < 2 (nothing to score)", b, lens[b]);
        ERGM_CHECK_ARG(lens[b] <= d.n_positions, "decode_score: sequence %d has %d tokens > n_positions %d", b, lens[b],
                       d.n_positions);
        ERGM_CHECK_ARG(cap_lens[b] >= 1 && cap_lens[b] <= d.cap_max, "decode_score: caption of sequence %d has %d rows outside "
                       "[1, cap_max %d]", b, cap_lens[b], d.cap_max);
        R += lens[b], Rc += cap_lens[b];
        a.max_n = std::max(a.max_n, lens[b]), a.max_c = std::max(a.max_c, cap_lens[b]);
    }
    a.n_seq = n_seq, a.R = (int)R, a.Rc = (int)Rc;
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "decode_score: workspace must be 256-byte aligned");
    ERGM_CHECK_ARG(score_rows_ok(d, a.R, a.Rc), "decode_score: bad row counts");
    ScoreOut o{targets, logprob, top1, nullptr, 0};
    const size_t need = score_carve(d, a.R, a.Rc, &a.ws, &o.lm_ws, &o.lm_bytes, nullptr);  // this call alone
    ERGM_CHECK_ARG(ws_bytes >= need, "decode_score: %d packed rows and %d caption rows need a workspace of %zu bytes, %zu given",
                   a.R, a.Rc, need, ws_bytes);
    score_carve(d, a.R, a.Rc, &a.ws, &o.lm_ws, &o.lm_bytes, reinterpret_cast<char*>(workspace));
    a.meta = meta, a.ids = ids, a.tt = token_types, a.cap_ids = cap_ids;
    a.vis = vis, a.aud = aud, a.has_feat = has_feat;
    Walk w{false, "decode_score", as_stream(stream)};
    return walk_score(P, w, a, o);
}

extern "C" int ergm_decode_score_launches(const ergm_decode_plan* P, int n_seq, int rows, int cap_rows) {
    ERGM_CHECK_ARG(P && n_seq >= 1 && n_seq <= P->d.max_batch && rows >= 2 * (int64_t)n_seq && cap_rows >= n_seq &&
                       score_rows_ok(P->d, rows, cap_rows),
                   "decode_score_launches: bad plan or counts (n_seq %d rows %d cap_rows %d)", n_seq, rows, cap_rows);
    Packed a{};
    a.n_seq = n_seq, a.R = rows, a.Rc = cap_rows, a.max_n = rows, a.max_c = cap_rows;
    ScoreOut o{};
    // buffer addresses for the GEMM descriptors the walk plans (the plan's own workspace; nothing is launched)
    score_carve(P->d, rows, cap_rows, &a.ws, &o.lm_ws, &o.lm_bytes, reinterpret_cast<char*>(P->b.h));
    Walk w{true, "decode_score_launches"};
    ERGM_TRY(walk_score(P, w, a, o));
    return w.count;
}

extern "C" int ergm_decode_step_slots(ergm_decode_plan* P, const int64_t* tokens, const int64_t* token_types, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_step_slots"));
    ERGM_CHECK_ARG(tokens, "decode_step_slots: null tokens");
    Walk w{false, "decode_step", as_stream(stream)};
    return walk(P, w, P->engine, P->d.max_batch, tokens, token_types);
}

// n steps over the slots: a token per slot from the logits of the step before, then the step.  ctl null: nucleus
// sampling alone; else ergm_sample_rows, with the tokens' log-probabilities where asked for.
static int run_slots(ergm_decode_plan* P, const char* what, int n, float top_p, const ergm_sample_ctl* ctl, uint64_t seed,
                     int64_t eos_id, int64_t sp2_id, int64_t* tokens_out, float* logprobs_out, void* stream) {
    ERGM_TRY(slots_ready(P, what));
    ERGM_CHECK_ARG(n >= 1, "%s: n %d < 1", what, n);
    ERGM_CHECK_ARG(tokens_out, "%s: null tokens_out", what);
    ERGM_CHECK_ARG(top_p == top_p, "%s: top_p is NaN", what);
    hipStream_t s = as_stream(stream);
    const ergm_decode_dims& d = P->d;
    const int B = d.max_batch;
    ERGM_TRY(decode_fill_i64(P->tt, sp2_id, B, s));
    for (int i = 0; i < n; ++i) {
        int64_t* tok = tokens_out + (size_t)i * B;
        const bool ruled = ctl && P->ruled;
        if (ruled)
            ERGM_TRY(ergm_logit_rules_apply(P->logits, d.vocab_pad, B, d.vocab, &P->rules, P->lens, P->finished, eos_id, d.max_len, s));
        if (ctl)
            ERGM_TRY(ergm_sample_rows(P->logits, d.vocab_pad, B, d.vocab, top_p, ctl, seed, P->row_ids, P->row_steps, P->finished,
                                      eos_id, tok, nullptr, nullptr, logprobs_out ? logprobs_out + (size_t)i * B : nullptr, s));
        else
            ERGM_TRY(ergm_topp_sample_rows(P->logits, d.vocab_pad, B, d.vocab, top_p, seed, P->row_ids, P->row_steps, P->finished,
                                           eos_id, tok, nullptr, nullptr, s));
        if (ruled) ERGM_TRY(ergm_hist_append(tok, P->lens, P->finished, B, P->rules.hist, P->rules.ld_hist, d.max_len, s));
        Walk w{false, "decode_step", s};
        ERGM_TRY(walk(P, w, P->engine, B, tok, P->tt));
    }
    return ERGM_OK;
}

extern "C" int ergm_decode_run_slots(ergm_decode_plan* P, int n, float top_p, uint64_t seed, int64_t eos_id, int64_t sp2_id,
                                     int64_t* tokens_out, void* stream) {
    return run_slots(P, "decode_run_slots", n, top_p, nullptr, seed, eos_id, sp2_id, tokens_out, nullptr, stream);
}

extern "C" int ergm_decode_run_slots_sampled(ergm_decode_plan* P, int n, float top_p, const ergm_sample_ctl* ctl, uint64_t seed,
                                             int64_t eos_id, int64_t sp2_id, int64_t* tokens_out, float* logprobs_out,
                                             void* stream) {
    const ergm_sample_ctl none{};  // no control asked for: still ergm_sample_rows, at its defaults
    return run_slots(P, "decode_run_slots_sampled", n, top_p, ctl ? ctl : &none, seed, eos_id, sp2_id, tokens_out, logprobs_out, stream);
}

// n rounds of beam search over all max_batch slots, W slots per group: ergm_decode_run_beams' round with the slot step
// behind it, so a live row is finished by the device at the bound of its admission (ergm_hip.h has the rule).
extern "C" int ergm_decode_run_slot_beams(ergm_decode_plan* P, int n, int W, int rows_bound, int64_t eos_id, int64_t sp2_id,
                                          float* scores, int64_t* tokens_out, int* parents_out, void* workspace, size_t ws_bytes,
                                          void* stream) {
    ERGM_TRY(slots_ready(P, "decode_run_slot_beams"));
    const ergm_decode_dims& d = P->d;
    const int B = d.max_batch;
    ERGM_CHECK_ARG(n >= 1, "decode_run_slot_beams: n %d < 1", n);
    ERGM_CHECK_ARG(W >= 1 && W <= 8 && W <= d.vocab, "decode_run_slot_beams: W %d outside [1, 8] or above the vocabulary %d", W,
                   d.vocab);
    ERGM_CHECK_ARG(B % W == 0, "decode_run_slot_beams: max_batch %d is no multiple of W %d", B, W);
    ERGM_CHECK_ARG(eos_id >= 0 && eos_id < d.vocab, "decode_run_slot_beams: eos_id %lld outside the vocabulary", (long long)eos_id);
    ERGM_CHECK_ARG(rows_bound >= 0 && rows_bound <= d.max_len, "decode_run_slot_beams: rows_bound %d outside [0, max_len %d]",
                   rows_bound, d.max_len);
    ERGM_CHECK_ARG(scores && tokens_out && parents_out && workspace, "decode_run_slot_beams: null argument");
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(scores) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(tokens_out) & 7) == 0 && (reinterpret_cast<uintptr_t>(parents_out) & 3) == 0,
                   "decode_run_slot_beams: misaligned argument (workspace and tokens_out 8 bytes, scores and parents_out 4)");
    ERGM_CHECK_ARG(ws_bytes >= ergm_beam_select_workspace_size(B, W), "decode_run_slot_beams: workspace %zu < %zu bytes", ws_bytes,
                   ergm_beam_select_workspace_size(B, W));
    hipStream_t s = as_stream(stream);
    const int64_t kv_row = (int64_t)2 * d.n_embd * 2;  // bytes of a K | V row
    ERGM_TRY(decode_fill_i64(P->tt, sp2_id, B, s));
    for (int i = 0; i < n; ++i) {
        int64_t* tok = tokens_out + (size_t)i * B;
        int* par = parents_out + (size_t)i * B;
        Walk w{false, "decode_run_slot_beams", s};
        if (P->ruled)
            ERGM_TRY(ergm_logit_rules_apply(P->logits, d.vocab_pad, B, d.vocab, &P->rules, P->lens, P->finished, eos_id, d.max_len, s));
        if (w.on(beam_select_launches()))
            ERGM_TRY(ergm_beam_select(P->logits, d.vocab_pad, B, W, d.vocab, scores, P->finished, eos_id, par, tok, workspace,
                                      ws_bytes, s));
        // the caller's bound on the live lengths, one more per round: the gather's grid covers the rows in use
        const int rows = std::max(1, (int)std::min<int64_t>((int64_t)rows_bound + i, d.max_len));
        if (w.on(beam_gather_launches(d.n_layer)))
            ERGM_TRY(ergm_beam_gather(P->kv.data(), d.n_layer, (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, par, P->lens, B, W, rows,
                                      s));
        if (P->ruled) {  // the histories follow the caches, then take the round's tokens
            ERGM_TRY(ergm_hist_follow(P->rules.hist, P->rules.ld_hist, par, P->lens, B, W, d.max_len, s));
            ERGM_TRY(ergm_hist_append(tok, P->lens, P->finished, B, P->rules.hist, P->rules.ld_hist, d.max_len, s));
        }
        ERGM_TRY(walk(P, w, P->engine, B, tok, P->tt));
    }
    return ERGM_OK;
}

extern "C" int ergm_decode_launches(const ergm_decode_plan* P, int engine) {
    ERGM_CHECK_ARG(P && engine >= 0 && engine < kEngines, "decode_launches: bad plan or engine %d", engine);
    Walk w{true, "decode_launches"};
    ERGM_TRY(walk(P, w, engine, P->bound ? P->B : P->d.max_batch, nullptr, nullptr));
    return w.count;
}
