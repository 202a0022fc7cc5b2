// Native decode executor (ergm_hip.h, ergm_decode_*): BatchedGenerator.step and the sampling loop of
// BatchedGenerator.generate (ergm_amd/generate.py) as launch sequences on the caller's one stream.
//
// The step is written once (walk): every kernel goes through Walk::on, which counts the launch and, in a dry walk,
// returns before calling anything, so ergm_decode_launches reports what ergm_decode_step enqueues.  Engine 0 calls
// the C-ABI entry points the Python path calls, with its arguments; engine 1 puts ergm_linear_rows in the
// place of each LayerNorm + GEMM pair and each plain GEMM of the blocks.
//
// Slot mode (ergm_decode_bind_slots) serves ContinuousGenerator: the same step over all max_batch cache slots with the
// slot length update at its end, the admission of new sequences into free slots (walk_admit: the prefill over
// packed ragged rows, written once like the step so that ergm_decode_admit_launches counts what runs), and the
// extension of occupied slots by more than one token (walk_extend: packed new rows over the slots' own caches).
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
}  // namespace ergm

using namespace ergm;

struct ergm_decode_plan {
    ergm_decode_dims d;
    ergm_model_params p;
    // workspace
    float* h;        // [max_batch][E] the residual stream of the step
    __bf16* x;       // [max_batch][E] LayerNorm output (engine 0, and the head of engine 1)
    __bf16* qkv;     // [max_batch][3E]
    __bf16* att;     // [max_batch][E] attention output
    __bf16* q;       // [max_batch][E] cross-attention query
    __bf16* pre;     // [max_batch][F] gelu' (engine 0: the Python path's aux_out)
    __bf16* act;     // [max_batch][F]
    float* mean;     // [max_batch]
    float* rstd;
    int64_t* tt;     // [max_batch] ergm_decode_run's token types
    void* attn_ws;
    size_t attn_ws_bytes;
    void* gemm_ws;
    size_t gemm_ws_bytes;
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
};

namespace {

constexpr int kEngines = 2;

size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

bool dims_ok(const ergm_decode_dims& d) {
    return d.n_embd > 0 && d.n_head > 0 && d.n_embd == 64 * d.n_head && d.n_embd <= 1024 && d.n_inner > 0 &&
           d.n_inner % 64 == 0 && d.vocab > 0 && d.vocab_pad >= d.vocab && d.vocab_pad % 64 == 0 && d.n_layer > 0 &&
           d.max_batch > 0 && d.max_len > 0 && d.max_len <= d.n_positions && d.cap_max > 0;
}

ergm_gemm_desc gemm_desc(int M, int N, int K, int b_layout, int c_dtype, int epi, const float* bias, const void* aux,
                         void* aux_out, int ldc) {
    ergm_gemm_desc g{};
    g.M = M, g.N = N, g.K = K;
    g.lda = K, g.ldb = b_layout == ERGM_KN ? N : K, g.ldc = ldc;
    g.a_layout = ERGM_MK, g.b_layout = b_layout, g.c_dtype = c_dtype, g.epilogue = epi;
    g.alpha = 1.0f;
    g.bias = bias;
    g.aux = aux, g.ld_aux = aux ? ldc : 0;
    g.aux_out = aux_out, g.ld_aux_out = aux_out ? N : 0;
    return g;
}

// ---- slot mode: the admission (ergm_decode_admit) ----------------------------------------------------------
// The buffers of one admission of at most R packed token rows and Rc packed caption rows, carved from the caller's
// workspace like the plan's own.
struct AdmitWs {
    float* h;       // [R][E] residual stream
    __bf16* x;      // [R][E] LayerNorm output
    __bf16* qkv;    // [R][3E]
    __bf16* att;    // [R][E]
    __bf16* q;      // [R][E]
    __bf16* pre;    // [R][F]
    __bf16* act;    // [R][F]
    float *mean, *rstd;  // [R]
    __bf16* cap;    // [Rc][E] caption embeddings
    __bf16* ckv;    // [Rc][2E] caption K | V of one layer
    float* hl;      // [max_batch][E] the last row of every sequence
    float* lg;      // [max_batch][vocab_pad] their logits, before they go to the slots
    void* gemm_ws;
    size_t gemm_ws_bytes;
};

// The largest split-K workspace of the step's GEMMs over every batch size the plan can be bound to.
size_t gemm_ws_need(const ergm_decode_dims& d) {
    const int E = d.n_embd, F = d.n_inner;
    const int shapes[5][3] = {{3 * E, E, ERGM_KN}, {E, E, ERGM_KN}, {F, E, ERGM_KN}, {E, F, ERGM_KN}, {d.vocab_pad, E, ERGM_NK}};
    size_t need = 0;
    for (int M = 1; M <= d.max_batch; ++M)
        for (const auto& s : shapes) {
            const ergm_gemm_desc g = gemm_desc(M, s[0], s[1], s[2], ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr, nullptr, s[0]);
            need = std::max(need, ergm_gemm_workspace_size(&g));
        }
    return need;
}

// Carves the workspace; base == nullptr only sizes it.
size_t carve(ergm_decode_plan* P, char* base) {
    const ergm_decode_dims& d = P->d;
    const size_t mb = d.max_batch, E = d.n_embd, F = d.n_inner;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += al256(bytes);
        return p;
    };
    P->h = reinterpret_cast<float*>(take(mb * E * 4));
    P->x = reinterpret_cast<__bf16*>(take(mb * E * 2));
    P->qkv = reinterpret_cast<__bf16*>(take(mb * 3 * E * 2));
    P->att = reinterpret_cast<__bf16*>(take(mb * E * 2));
    P->q = reinterpret_cast<__bf16*>(take(mb * E * 2));
    P->pre = reinterpret_cast<__bf16*>(take(mb * F * 2));
    P->act = reinterpret_cast<__bf16*>(take(mb * F * 2));
    P->mean = reinterpret_cast<float*>(take(mb * 4));
    P->rstd = reinterpret_cast<float*>(take(mb * 4));
    P->tt = reinterpret_cast<int64_t*>(take(mb * 8));
    P->attn_ws_bytes = std::max<size_t>(16, ergm_attn_decode_workspace_size(d.max_batch, d.n_head, std::max(d.max_len, d.cap_max)));
    P->attn_ws = take(P->attn_ws_bytes);
    P->gemm_ws_bytes = std::max<size_t>(16, gemm_ws_need(d));
    P->gemm_ws = take(P->gemm_ws_bytes);
    return off;
}

struct Walk {
    bool dry;
    int count = 0;
    hipStream_t s = nullptr;
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

int ln(const ergm_decode_plan* P, Walk& w, int B, const float* g, const float* b) {
    if (!w.on()) return ERGM_OK;
    return ergm_layernorm_fwd(P->h, g, b, P->x, P->mean, P->rstd, B, P->d.n_embd, P->d.eps, w.s);
}

// ergm_gemm as ops.gemm calls it (split_k = 0, the workspace of its own query)
int gemm(const ergm_decode_plan* P, Walk& w, int B, int N, int K, const void* A, const void* W, int b_layout, void* C,
         int c_dtype, int epi, const float* bias, const void* aux, void* aux_out, int ldc) {
    const ergm_gemm_desc g = gemm_desc(B, N, K, b_layout, c_dtype, epi, bias, aux, aux_out, ldc);
    int cfg = 0, split = 1, flags = 0;
    ERGM_TRY(ergm_gemm_plan(&g, &cfg, &split, &flags));
    if (!w.on(split > 1 ? 2 : 1)) return ERGM_OK;
    const size_t need = ergm_gemm_workspace_size(&g);
    ERGM_CHECK_ARG(need <= P->gemm_ws_bytes, "decode_step: GEMM workspace %zu > %zu bytes (a GEMM override set after the plan)",
                   need, P->gemm_ws_bytes);
    return ergm_gemm(&g, A, W, C, P->gemm_ws, need, w.s);
}

int linear(const ergm_decode_plan* P, Walk& w, int B, int N, int K, const void* A, const float* gamma, const float* beta,
           const void* W, int w_layout, void* C, int epi, const float* bias, const float* aux, int ldc) {
    if (!w.on()) return ERGM_OK;
    ergm_linear_rows_desc g{};
    g.M = B, g.N = N, g.K = K;
    g.lda = K, g.ldw = w_layout == ERGM_KN ? N : K, g.ldc = ldc;
    g.w_layout = w_layout, g.epilogue = epi;
    g.bias = bias;
    g.aux = aux, g.ld_aux = aux ? ldc : 0;
    g.ln_gamma = gamma, g.ln_beta = beta, g.ln_eps = P->d.eps;
    return ergm_linear_rows(&g, A, W, C, w.s);
}

// LayerNorm(h; ln tensors t_ln, t_ln+1) -> Conv1D (weight t_w, bias t_w+1) of block l, N columns, into bf16 C
int ln_linear(const ergm_decode_plan* P, Walk& w, int B, int l, int t_ln, int t_w, int N, void* C, int epi) {
    const int E = P->d.n_embd;
    if (P->engine == 0) {
        ERGM_TRY(ln(P, w, B, lf(P, l, t_ln), lf(P, l, t_ln + 1)));
        void* aux_out = epi == ERGM_EPI_BIAS_GELU ? P->pre : nullptr;
        return gemm(P, w, B, N, E, P->x, lb(P, l, t_w), ERGM_KN, C, ERGM_BF16, epi, lf(P, l, t_w + 1), nullptr, aux_out, N);
    }
    return linear(P, w, B, N, E, P->h, lf(P, l, t_ln), lf(P, l, t_ln + 1), lb(P, l, t_w), ERGM_KN, C, epi, lf(P, l, t_w + 1),
                  nullptr, N);
}

// h += A·W + bias (weight t_w of block l, K rows)
int proj_resid(const ergm_decode_plan* P, Walk& w, int B, int l, int t_w, int K, const void* A) {
    const int E = P->d.n_embd;
    if (P->engine == 0)
        return gemm(P, w, B, E, K, A, lb(P, l, t_w), ERGM_KN, P->h, ERGM_F32, ERGM_EPI_BIAS_RESID, lf(P, l, t_w + 1), P->h,
                    nullptr, E);
    return linear(P, w, B, E, K, A, nullptr, nullptr, lb(P, l, t_w), ERGM_KN, P->h, ERGM_EPI_BIAS_RESID, lf(P, l, t_w + 1),
                  P->h, E);
}

int attn(const ergm_decode_plan* P, Walk& w, int B, const __bf16* qkv, int ld_qkv, void* cache, int rows, const int* lens,
         int append) {
    const ergm_decode_dims& d = P->d;
    if (!w.on(attn_decode_launches(B, d.n_head, rows))) return ERGM_OK;
    __bf16* k = reinterpret_cast<__bf16*>(cache);
    return ergm_attn_decode(qkv, ld_qkv, k, k + d.n_embd, (int64_t)rows * 2 * d.n_embd, 2 * d.n_embd, lens, B, d.n_head, rows,
                            append, 0, P->att, d.n_embd, P->attn_ws, P->attn_ws_bytes, w.s);
}

// One decode step for B sequences; a dry walk (w.dry) only counts.
int walk(const ergm_decode_plan* P, Walk& w, int B, const int64_t* tokens, const int64_t* tt) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, F = d.n_inner;
    if (w.on())
        ERGM_TRY(ergm_embed_rows(tokens, tt, P->lens, P->p.wte, P->p.wpe, P->h, B, E, d.vocab_pad, d.n_positions, w.s));
    for (int l = 0; l < d.n_layer; ++l) {
        ERGM_TRY(ln_linear(P, w, B, l, ERGM_T_LN1_W, ERGM_T_ATTN_W, 3 * E, P->qkv, ERGM_EPI_BIAS));
        ERGM_TRY(attn(P, w, B, P->qkv, 3 * E, w.dry ? nullptr : P->kv[l], d.max_len, P->lens, 1));
        ERGM_TRY(proj_resid(P, w, B, l, ERGM_T_APROJ_W, E, P->att));
        ERGM_TRY(ln_linear(P, w, B, l, ERGM_T_LNX_W, ERGM_T_XQ_W, E, P->q, ERGM_EPI_BIAS));
        ERGM_TRY(attn(P, w, B, P->q, E, w.dry ? nullptr : P->xkv[l], P->bound ? P->Sc : d.cap_max, P->cap_lens, 0));
        ERGM_TRY(proj_resid(P, w, B, l, ERGM_T_XPROJ_W, E, P->att));
        ERGM_TRY(ln_linear(P, w, B, l, ERGM_T_LN2_W, ERGM_T_FC_W, F, P->act, ERGM_EPI_BIAS_GELU));
        ERGM_TRY(proj_resid(P, w, B, l, ERGM_T_MPROJ_W, F, P->act));
    }
    // The head stays ln_f + ergm_gemm on both engines: at N = vocab_pad ergm_gemm has hundreds of workgroups already and
    // measured 19 us against ergm_linear_rows' 41 us at B = 32 (139 us with the LayerNorm in the prologue, every strip
    // re-reading the rows).  ERGM_DECODE_HEAD=lr / ln, read when the plan is created, puts engine 1's head
    // on ergm_linear_rows behind ergm_layernorm_fwd / with the prologue, to repeat that measurement.
    const int head = P->engine == 1 ? P->head_lr : 0;
    if (head == 2) {
        ERGM_TRY(linear(P, w, B, d.vocab_pad, E, P->h, P->p.ln_f_w, P->p.ln_f_b, P->p.wte_b, ERGM_NK, P->logits, ERGM_EPI_NONE,
                        nullptr, nullptr, d.vocab_pad));
    } else {
        ERGM_TRY(ln(P, w, B, P->p.ln_f_w, P->p.ln_f_b));
        if (head == 0)
            ERGM_TRY(gemm(P, w, B, d.vocab_pad, E, P->x, P->p.wte_b, ERGM_NK, P->logits, ERGM_F32, ERGM_EPI_NONE, nullptr,
                          nullptr, nullptr, d.vocab_pad));
        else
            ERGM_TRY(linear(P, w, B, d.vocab_pad, E, P->x, nullptr, nullptr, P->p.wte_b, ERGM_NK, P->logits, ERGM_EPI_NONE,
                            nullptr, nullptr, d.vocab_pad));
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


// The largest split-K workspace of an admission's GEMMs: over every row count up to (R, Rc, max_batch sequences), so
// that a workspace sized for R rows serves every smaller admission; or (n_seq > 0) of the one admission of exactly
// R rows, Rc caption rows and n_seq sequences, which the first covers.
size_t admit_gemm_ws_need(const ergm_decode_dims& d, int R, int Rc, int n_seq) {
    const int E = d.n_embd, F = d.n_inner;
    size_t need = 0;
    auto upto = [&](int rows, int N, int K, int b_layout) {
        for (int M = n_seq > 0 ? rows : 1; M <= rows; ++M) {
            const ergm_gemm_desc g = gemm_desc(M, N, K, b_layout, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr, nullptr, N);
            need = std::max(need, ergm_gemm_workspace_size(&g));
        }
    };
    upto(R, 3 * E, E, ERGM_KN), upto(R, E, E, ERGM_KN), upto(R, F, E, ERGM_KN), upto(R, E, F, ERGM_KN);
    upto(Rc, 2 * E, E, ERGM_KN);
    upto(n_seq > 0 ? n_seq : d.max_batch, d.vocab_pad, E, ERGM_NK);
    return need;
}

size_t admit_carve(const ergm_decode_dims& d, int R_, int Rc_, int n_seq, AdmitWs* A, char* base) {
    const size_t R = R_, Rc = Rc_, mb = d.max_batch, E = d.n_embd, F = d.n_inner;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += al256(bytes);
        return p;
    };
    A->h = reinterpret_cast<float*>(take(R * E * 4));
    A->x = reinterpret_cast<__bf16*>(take(std::max(R, mb) * E * 2));
    A->qkv = reinterpret_cast<__bf16*>(take(R * 3 * E * 2));
    A->att = reinterpret_cast<__bf16*>(take(R * E * 2));
    A->q = reinterpret_cast<__bf16*>(take(R * E * 2));
    A->pre = reinterpret_cast<__bf16*>(take(R * F * 2));
    A->act = reinterpret_cast<__bf16*>(take(R * F * 2));
    A->mean = reinterpret_cast<float*>(take(std::max(R, mb) * 4));
    A->rstd = reinterpret_cast<float*>(take(std::max(R, mb) * 4));
    A->cap = reinterpret_cast<__bf16*>(take(Rc * E * 2));
    A->ckv = reinterpret_cast<__bf16*>(take(Rc * 2 * E * 2));
    A->hl = reinterpret_cast<float*>(take(mb * E * 4));
    A->lg = reinterpret_cast<float*>(take(mb * (size_t)d.vocab_pad * 4));
    A->gemm_ws_bytes = std::max<size_t>(16, admit_gemm_ws_need(d, R_, Rc_, n_seq));
    A->gemm_ws = take(A->gemm_ws_bytes);
    return off;
}

// What one admission was called with; the launch sequence below reads nothing else.
struct Admit {
    int n_seq, R, Rc, max_n, max_c;  // sequences, packed token / caption rows, the longest of each
    const int* meta;                 // device [ERGM_ADMIT_META_ROWS][n_seq]
    const int64_t *ids, *tt, *cap_ids;
    const float *vis, *aud;
    const uint8_t* has_feat;
    AdmitWs ws;
    const int* row(int i) const { return meta ? meta + (size_t)i * n_seq : nullptr; }
};

int admit_ln(const ergm_decode_plan* P, Walk& w, const Admit& a, const float* in, int rows, const float* g, const float* b) {
    if (!w.on()) return ERGM_OK;
    return ergm_layernorm_fwd(in, g, b, a.ws.x, a.ws.mean, a.ws.rstd, rows, P->d.n_embd, P->d.eps, w.s);
}

// ergm_gemm as ops.gemm calls it, on the admission's workspace
int admit_gemm(Walk& w, const Admit& a, int M, int N, int K, const void* A, const void* W, int b_layout, void* C, int c_dtype,
               int epi, const float* bias, const void* aux, void* aux_out, int ldb = 0) {
    ergm_gemm_desc g = gemm_desc(M, N, K, b_layout, c_dtype, epi, bias, aux, aux_out, N);
    if (ldb) g.ldb = ldb;
    int cfg = 0, split = 1, flags = 0;
    ERGM_TRY(ergm_gemm_plan(&g, &cfg, &split, &flags));
    if (!w.on(split > 1 ? 2 : 1)) return ERGM_OK;
    const size_t need = ergm_gemm_workspace_size(&g);
    ERGM_CHECK_ARG(need <= a.ws.gemm_ws_bytes, "decode_admit: GEMM workspace %zu > %zu bytes (a GEMM override set after the query)",
                   need, a.ws.gemm_ws_bytes);
    return ergm_gemm(&g, A, W, C, a.ws.gemm_ws, need, w.s);
}

// The admission's launch sequence, written once: a dry walk (w.dry) only counts.
int walk_admit(const ergm_decode_plan* P, Walk& w, const Admit& a) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, F = d.n_inner, H = d.n_head, R = a.R, Rc = a.Rc, n = a.n_seq;
    const AdmitWs& W = a.ws;
    const int *slot = a.row(0), *q0 = a.row(1), *qn = a.row(2), *c0 = a.row(3), *cn = a.row(4), *last = a.row(7),
              *ones = a.row(8), *iota = a.row(9);
    const int64_t kv_row = (int64_t)2 * E * 2;  // bytes of a K | V row
    if (w.on())
        ERGM_TRY(ergm_embed_packed(a.ids, a.tt, a.cap_ids, P->p.wte, P->p.wpe, a.vis, a.aud, a.has_feat, q0, qn, c0, cn, n, R, Rc,
                                   a.max_n, a.max_c, W.h, W.cap, E, E, d.vocab_pad, d.n_positions, w.s));
    for (int l = 0; l < d.n_layer; ++l) {
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LN1_W), lf(P, l, ERGM_T_LN1_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, 3 * E, E, W.x, lb(P, l, ERGM_T_ATTN_W), ERGM_KN, W.qkv, ERGM_BF16, ERGM_EPI_BIAS,
                            lf(P, l, ERGM_T_ATTN_W + 1), nullptr, nullptr));
        if (w.on())
            ERGM_TRY(ergm_attn_fwd_ragged(W.qkv, W.qkv + E, W.qkv + 2 * E, W.att, nullptr, q0, qn, q0, qn, n, H, R, R, a.max_n,
                                          a.max_n, 3 * E, 3 * E, 3 * E, E, 1, w.s));
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots(W.qkv + E, (int64_t)3 * E * 2, q0, qn, slot, n, R, a.max_n, P->kv[l],
                                        (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, d.max_batch, d.max_len, w.s));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.att, lb(P, l, ERGM_T_APROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_APROJ_W + 1), W.h, nullptr));
        // layer l's columns of the stacked caption K | V weight [E][L·2E] (the view the Python path passes)
        ERGM_TRY(admit_gemm(w, a, Rc, 2 * E, E, W.cap, reinterpret_cast<const __bf16*>(P->p.capkv_w_b) + (size_t)l * 2 * E,
                            ERGM_KN, W.ckv, ERGM_BF16, ERGM_EPI_BIAS, P->p.capkv_b + (size_t)l * 2 * E, nullptr, nullptr,
                            d.n_layer * 2 * E));
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots(W.ckv, kv_row, c0, cn, slot, n, Rc, a.max_c, P->xkv[l], (int64_t)d.cap_max * kv_row,
                                        kv_row, (int)kv_row, d.max_batch, d.cap_max, w.s));
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LNX_W), lf(P, l, ERGM_T_LNX_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.x, lb(P, l, ERGM_T_XQ_W), ERGM_KN, W.q, ERGM_BF16, ERGM_EPI_BIAS,
                            lf(P, l, ERGM_T_XQ_W + 1), nullptr, nullptr));
        if (w.on())
            ERGM_TRY(ergm_attn_fwd_ragged(W.q, W.ckv, W.ckv + E, W.att, nullptr, q0, qn, c0, cn, n, H, R, Rc, a.max_n, a.max_c, E,
                                          2 * E, 2 * E, E, 0, w.s));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.att, lb(P, l, ERGM_T_XPROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_XPROJ_W + 1), W.h, nullptr));
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LN2_W), lf(P, l, ERGM_T_LN2_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, F, E, W.x, lb(P, l, ERGM_T_FC_W), ERGM_KN, W.act, ERGM_BF16, ERGM_EPI_BIAS_GELU,
                            lf(P, l, ERGM_T_FC_W + 1), nullptr, W.pre));
        ERGM_TRY(admit_gemm(w, a, R, E, F, W.act, lb(P, l, ERGM_T_MPROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_MPROJ_W + 1), W.h, nullptr));
    }
    // the last row of every sequence -> ln_f -> the head -> logits[slot]
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.h, (int64_t)E * 4, last, ones, iota, n, R, 1, W.hl, (int64_t)E * 4, (int64_t)E * 4, E * 4, n,
                                    1, w.s));
    ERGM_TRY(admit_ln(P, w, a, W.hl, n, P->p.ln_f_w, P->p.ln_f_b));
    ERGM_TRY(admit_gemm(w, a, n, d.vocab_pad, E, W.x, P->p.wte_b, ERGM_NK, W.lg, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr,
                        nullptr));
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.lg, (int64_t)d.vocab_pad * 4, iota, ones, slot, n, n, 1, P->logits, (int64_t)d.vocab_pad * 4,
                                    (int64_t)d.vocab_pad * 4, d.vocab_pad * 4, d.max_batch, 1, w.s));
    if (w.on())
        ERGM_TRY(decode_slots_admit(slot, qn, cn, a.row(5), reinterpret_cast<const uint32_t*>(a.row(6)), n, d.max_batch, d.max_len,
                                    d.cap_max, P->lens, P->cap_lens_rw, P->stop_lens, P->row_ids, P->row_steps, P->finished,
                                    w.s));
    return ERGM_OK;
}

// ---- slot mode: the extension (ergm_decode_extend) -----------------------------------------------------------
// What one extension was called with; it runs on the admission's workspace (one caption row carved, none used).
struct Extend {
    int n_seq, R, max_n, max_k, max_c;  // sequences, packed new rows, the longest chunk, past + chunk and caption
    const int* meta;                    // device [ERGM_EXTEND_META_ROWS][n_seq]
    const int64_t *ids, *tt;
    const int* pos;                     // device [R]: the position of every packed row
    Admit a;                            // the workspace, for admit_ln / admit_gemm
    const int* row(int i) const { return meta ? meta + (size_t)i * n_seq : nullptr; }
};

// The extension's launch sequence, written once: a dry walk (w.dry) only counts.
int walk_extend(const ergm_decode_plan* P, Walk& w, const Extend& x) {
    const ergm_decode_dims& d = P->d;
    const int E = d.n_embd, F = d.n_inner, H = d.n_head, R = x.R, n = x.n_seq;
    const Admit& a = x.a;
    const AdmitWs& W = a.ws;
    const int *slot = x.row(0), *q0 = x.row(1), *qn = x.row(2), *past = x.row(3), *k0 = x.row(4), *kn = x.row(5), *c0 = x.row(6),
              *cn = x.row(7), *last = x.row(9), *ones = x.row(10), *iota = x.row(11);
    const int64_t kv_row = (int64_t)2 * E * 2;  // bytes of a K | V row
    if (w.on())
        ERGM_TRY(ergm_embed_rows(x.ids, x.tt, x.pos, P->p.wte, P->p.wpe, W.h, R, E, d.vocab_pad, d.n_positions, w.s));
    for (int l = 0; l < d.n_layer; ++l) {
        const __bf16* kv = w.dry ? nullptr : reinterpret_cast<const __bf16*>(P->kv[l]);
        const __bf16* xkv = w.dry ? nullptr : reinterpret_cast<const __bf16*>(P->xkv[l]);
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LN1_W), lf(P, l, ERGM_T_LN1_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, 3 * E, E, W.x, lb(P, l, ERGM_T_ATTN_W), ERGM_KN, W.qkv, ERGM_BF16, ERGM_EPI_BIAS,
                            lf(P, l, ERGM_T_ATTN_W + 1), nullptr, nullptr));
        // the new rows' K | V into rows past_b .. of their slots, then the queries over the whole slot
        if (w.on())
            ERGM_TRY(ergm_rows_to_slots_at(W.qkv + E, (int64_t)3 * E * 2, q0, qn, slot, past, n, R, x.max_n, P->kv[l],
                                           (int64_t)d.max_len * kv_row, kv_row, (int)kv_row, d.max_batch, d.max_len, w.s));
        if (w.on())
            ERGM_TRY(ergm_attn_fwd_extend(W.qkv, kv, kv + E, W.att, q0, qn, k0, kn, n, H, R, d.max_batch * d.max_len, x.max_n,
                                          x.max_k, 3 * E, 2 * E, 2 * E, E, w.s));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.att, lb(P, l, ERGM_T_APROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_APROJ_W + 1), W.h, nullptr));
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LNX_W), lf(P, l, ERGM_T_LNX_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.x, lb(P, l, ERGM_T_XQ_W), ERGM_KN, W.q, ERGM_BF16, ERGM_EPI_BIAS,
                            lf(P, l, ERGM_T_XQ_W + 1), nullptr, nullptr));
        // the caption rows the admission left in the slot: xkv[l] as packed rows, sequence b's at slot_b · cap_max
        if (w.on())
            ERGM_TRY(ergm_attn_fwd_ragged(W.q, xkv, xkv + E, W.att, nullptr, q0, qn, c0, cn, n, H, R, d.max_batch * d.cap_max,
                                          x.max_n, x.max_c, E, 2 * E, 2 * E, E, 0, w.s));
        ERGM_TRY(admit_gemm(w, a, R, E, E, W.att, lb(P, l, ERGM_T_XPROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_XPROJ_W + 1), W.h, nullptr));
        ERGM_TRY(admit_ln(P, w, a, W.h, R, lf(P, l, ERGM_T_LN2_W), lf(P, l, ERGM_T_LN2_W + 1)));
        ERGM_TRY(admit_gemm(w, a, R, F, E, W.x, lb(P, l, ERGM_T_FC_W), ERGM_KN, W.act, ERGM_BF16, ERGM_EPI_BIAS_GELU,
                            lf(P, l, ERGM_T_FC_W + 1), nullptr, W.pre));
        ERGM_TRY(admit_gemm(w, a, R, E, F, W.act, lb(P, l, ERGM_T_MPROJ_W), ERGM_KN, W.h, ERGM_F32, ERGM_EPI_BIAS_RESID,
                            lf(P, l, ERGM_T_MPROJ_W + 1), W.h, nullptr));
    }
    // the last new row of every sequence -> ln_f -> the head -> logits[slot]
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.h, (int64_t)E * 4, last, ones, iota, n, R, 1, W.hl, (int64_t)E * 4, (int64_t)E * 4, E * 4, n,
                                    1, w.s));
    ERGM_TRY(admit_ln(P, w, a, W.hl, n, P->p.ln_f_w, P->p.ln_f_b));
    ERGM_TRY(admit_gemm(w, a, n, d.vocab_pad, E, W.x, P->p.wte_b, ERGM_NK, W.lg, ERGM_F32, ERGM_EPI_NONE, nullptr, nullptr,
                        nullptr));
    if (w.on())
        ERGM_TRY(ergm_rows_to_slots(W.lg, (int64_t)d.vocab_pad * 4, iota, ones, slot, n, n, 1, P->logits, (int64_t)d.vocab_pad * 4,
                                    (int64_t)d.vocab_pad * 4, d.vocab_pad * 4, d.max_batch, 1, w.s));
    if (w.on())
        ERGM_TRY(decode_slots_extend(slot, past, qn, x.row(8), n, d.max_batch, d.max_len, P->lens, P->stop_lens, P->finished, w.s));
    return ERGM_OK;
}

int slots_ready(const ergm_decode_plan* P, const char* what) {
    ERGM_CHECK_ARG(P, "%s: null plan", what);
    ERGM_CHECK_ARG(P->slots, "%s: no slots bound (ergm_decode_bind_slots)", what);
    return ERGM_OK;
}

bool admit_rows_ok(const ergm_decode_dims& d, int max_rows, int max_cap_rows) {
    return max_rows >= 1 && max_cap_rows >= 1 && (int64_t)max_rows <= (int64_t)d.max_batch * d.max_len &&
           (int64_t)max_cap_rows <= (int64_t)d.max_batch * d.cap_max;
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
    for (int l = 0; l < P->d.n_layer; ++l)
        ERGM_CHECK_ARG(kv[l] && xkv[l] && aligned16(kv[l]) && aligned16(xkv[l]),
                       "decode_bind: layer %d cache pointer null or not 16-byte aligned", l);
    ERGM_CHECK_ARG(aligned16(logits), "decode_bind: logits must be 16-byte aligned");
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

extern "C" int ergm_decode_step(ergm_decode_plan* P, const int64_t* tokens, const int64_t* token_types, void* stream) {
    ERGM_TRY(step_ready(P, 1, "decode_step"));
    ERGM_CHECK_ARG(tokens, "decode_step: null tokens");
    Walk w{false};
    w.s = as_stream(stream);
    ERGM_TRY(walk(P, w, P->B, tokens, token_types));
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
            Walk w{false};
            w.s = s;
            ERGM_TRY(walk(P, w, B, tokens_out + (size_t)(i - 1) * B, P->tt));
            P->n_max += 1;  // per step: after a launch failure part-way n_max counts the steps that were enqueued; the
                            // caller then rebinds (ergm_decode_bind sets n_max again) before it goes on
        }
        ERGM_TRY(ergm_topp_sample(P->logits, P->d.vocab_pad, B, P->d.vocab, top_p, seed, (uint32_t)i, P->finished, eos_id,
                                  tokens_out + (size_t)i * B, nullptr, nullptr, s));
    }
    return ERGM_OK;
}

extern "C" int ergm_decode_bind_slots(ergm_decode_plan* P, void* const* kv, void* const* xkv, float* logits, int* lens,
                                      int* cap_lens, uint8_t* finished, int* stop_lens, uint32_t* row_ids,
                                      uint32_t* row_steps) {
    ERGM_CHECK_ARG(P && kv && xkv && logits && lens && cap_lens && finished && stop_lens && row_ids && row_steps,
                   "decode_bind_slots: null argument");
    for (int l = 0; l < P->d.n_layer; ++l)
        ERGM_CHECK_ARG(kv[l] && xkv[l] && aligned16(kv[l]) && aligned16(xkv[l]),
                       "decode_bind_slots: layer %d cache pointer null or not 16-byte aligned", l);
    ERGM_CHECK_ARG(aligned16(logits), "decode_bind_slots: logits must be 16-byte aligned");
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
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= d.max_batch, "decode_admit: n_seq %d outside [1, max_batch %d]", n_seq, d.max_batch);
    ERGM_CHECK_ARG((vis == nullptr) == (aud == nullptr), "decode_admit: visual and audio features go together");
    ERGM_CHECK_ARG(P->p.capkv_w_b && P->p.capkv_b, "decode_admit: the plan was created without the caption K/V weights "
                   "(capkv_w_b, capkv_b)");
    Admit a{};
    std::vector<char> seen(d.max_batch, 0);
    int64_t R = 0, Rc = 0;
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(slots[b] >= 0 && slots[b] < d.max_batch, "decode_admit: slot %d of sequence %d outside [0, max_batch %d)",
                       slots[b], b, d.max_batch);
        ERGM_CHECK_ARG(!seen[slots[b]], "decode_admit: slot %d named twice", slots[b]);
        seen[slots[b]] = 1;
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
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "decode_admit: workspace must be 256-byte aligned");
    ERGM_CHECK_ARG(admit_rows_ok(d, (int)R, (int)Rc), "decode_admit: bad row counts");
    const size_t need = admit_carve(d, (int)R, (int)Rc, n_seq, &a.ws, nullptr);  // this admission alone
    ERGM_CHECK_ARG(ws_bytes >= need, "decode_admit: %lld packed rows and %lld caption rows need a workspace of %zu bytes, "
                   "%zu given", (long long)R, (long long)Rc, need, ws_bytes);
    a.n_seq = n_seq, a.R = (int)R, a.Rc = (int)Rc;
    a.meta = meta, a.ids = ids, a.tt = token_types, a.cap_ids = cap_ids;
    a.vis = vis, a.aud = aud, a.has_feat = has_feat;
    admit_carve(d, a.R, a.Rc, n_seq, &a.ws, reinterpret_cast<char*>(workspace));
    Walk w{false};
    w.s = as_stream(stream);
    return walk_admit(P, w, a);
}

extern "C" int ergm_decode_admit_launches(const ergm_decode_plan* P, int n_seq, int rows, int cap_rows) {
    ERGM_CHECK_ARG(P && n_seq >= 1 && n_seq <= P->d.max_batch && rows >= n_seq && cap_rows >= n_seq &&
                       admit_rows_ok(P->d, rows, cap_rows),
                   "decode_admit_launches: bad plan or counts (n_seq %d rows %d cap_rows %d)", n_seq, rows, cap_rows);
    Admit a{};
    a.n_seq = n_seq, a.R = rows, a.Rc = cap_rows, a.max_n = rows, a.max_c = cap_rows;
    // buffer addresses for the GEMM descriptors the walk plans (the plan's own workspace; nothing is launched)
    admit_carve(P->d, rows, cap_rows, n_seq, &a.ws, reinterpret_cast<char*>(P->h));
    Walk w{true};
    ERGM_TRY(walk_admit(P, w, a));
    return w.count;
}

extern "C" int ergm_decode_extend(ergm_decode_plan* P, int n_seq, const int* slots, const int* past, const int* lens,
                                  const int* cap_lens, const int* max_new, const int* meta, const int64_t* ids,
                                  const int64_t* token_types, const int* pos, void* workspace, size_t ws_bytes, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_extend"));
    const ergm_decode_dims& d = P->d;
    ERGM_CHECK_ARG(slots && past && lens && cap_lens && max_new && meta && ids && pos && workspace, "decode_extend: null argument");
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= d.max_batch, "decode_extend: n_seq %d outside [1, max_batch %d]", n_seq, d.max_batch);
    Extend x{};
    std::vector<char> seen(d.max_batch, 0);
    int64_t R = 0;
    for (int b = 0; b < n_seq; ++b) {
        ERGM_CHECK_ARG(slots[b] >= 0 && slots[b] < d.max_batch, "decode_extend: slot %d of sequence %d outside [0, max_batch %d)",
                       slots[b], b, d.max_batch);
        ERGM_CHECK_ARG(!seen[slots[b]], "decode_extend: slot %d named twice", slots[b]);
        seen[slots[b]] = 1;
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
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "decode_extend: workspace must be 256-byte aligned");
    ERGM_CHECK_ARG(admit_rows_ok(d, (int)R, 1), "decode_extend: bad row count");
    const size_t need = admit_carve(d, (int)R, 1, n_seq, &x.a.ws, nullptr);  // this extension alone
    ERGM_CHECK_ARG(ws_bytes >= need, "decode_extend: %lld packed rows need a workspace of %zu bytes, %zu given", (long long)R, need,
                   ws_bytes);
    x.n_seq = n_seq, x.R = (int)R;
    x.meta = meta, x.ids = ids, x.tt = token_types, x.pos = pos;
    admit_carve(d, x.R, 1, n_seq, &x.a.ws, reinterpret_cast<char*>(workspace));
    Walk w{false};
    w.s = as_stream(stream);
    return walk_extend(P, w, x);
}

extern "C" int ergm_decode_extend_launches(const ergm_decode_plan* P, int n_seq, int rows) {
    ERGM_CHECK_ARG(P && n_seq >= 1 && n_seq <= P->d.max_batch && rows >= n_seq && admit_rows_ok(P->d, rows, 1),
                   "decode_extend_launches: bad plan or counts (n_seq %d rows %d)", n_seq, rows);
    Extend x{};
    x.n_seq = n_seq, x.R = rows, x.max_n = rows, x.max_k = P->d.max_len, x.max_c = P->d.cap_max;
    // buffer addresses for the GEMM descriptors the walk plans (the plan's own workspace; nothing is launched)
    admit_carve(P->d, rows, 1, n_seq, &x.a.ws, reinterpret_cast<char*>(P->h));
    Walk w{true};
    ERGM_TRY(walk_extend(P, w, x));
    return w.count;
}

extern "C" int ergm_decode_step_slots(ergm_decode_plan* P, const int64_t* tokens, const int64_t* token_types, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_step_slots"));
    ERGM_CHECK_ARG(tokens, "decode_step_slots: null tokens");
    Walk w{false};
    w.s = as_stream(stream);
    return walk(P, w, P->d.max_batch, tokens, token_types);
}

extern "C" int ergm_decode_run_slots(ergm_decode_plan* P, int n, float top_p, uint64_t seed, int64_t eos_id, int64_t sp2_id,
                                     int64_t* tokens_out, void* stream) {
    ERGM_TRY(slots_ready(P, "decode_run_slots"));
    ERGM_CHECK_ARG(n >= 1, "decode_run_slots: n %d < 1", n);
    ERGM_CHECK_ARG(tokens_out, "decode_run_slots: null tokens_out");
    ERGM_CHECK_ARG(top_p == top_p, "decode_run_slots: top_p is NaN");
    hipStream_t s = as_stream(stream);
    const int B = P->d.max_batch;
    ERGM_TRY(decode_fill_i64(P->tt, sp2_id, B, s));
    for (int i = 0; i < n; ++i) {
        int64_t* tok = tokens_out + (size_t)i * B;
        ERGM_TRY(ergm_topp_sample_rows(P->logits, P->d.vocab_pad, B, P->d.vocab, top_p, seed, P->row_ids, P->row_steps,
                                       P->finished, eos_id, tok, nullptr, nullptr, s));
        Walk w{false};
        w.s = s;
        ERGM_TRY(walk(P, w, B, tok, P->tt));
    }
    return ERGM_OK;
}

extern "C" int ergm_decode_launches(const ergm_decode_plan* P, int engine) {
    ERGM_CHECK_ARG(P && engine >= 0 && engine < kEngines, "decode_launches: bad plan or engine %d", engine);
    ergm_decode_plan Q = *P;
    Q.engine = engine;
    Walk w{true};
    ERGM_TRY(walk(&Q, w, P->bound ? P->B : P->d.max_batch, nullptr, nullptr));
    return w.count;
}
