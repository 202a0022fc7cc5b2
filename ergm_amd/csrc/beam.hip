// Beam search on the device (ergm_hip.h, ergm_beam_*): the ranking of W·V scored continuations per prompt and the
// KV-cache rows following the surviving beams.  The rule is stated in ergm_hip.h; DESIGN.md §12.6 has the measurements.
//
// Select has two stages.  The row stage is the sampler's layout (decode.hip): one workgroup of 1,024 threads per row,
// the row in registers, the row's maximum and its exact integer mass S, then W rounds of a workgroup arg-max that leave
// the row's own top W candidates (c, token), best first.  The group stage is one wave: it ranks the at most W·W
// candidates of a group (a finished beam offers one, a dead beam none), takes the best W and assigns the rows.  The two
// stages run as two launches (a workgroup per row, then a wave per group, the candidates in the caller's workspace) or
// as one (a workgroup per group that walks its W rows, the candidates in LDS): ERGM_BEAM_SELECT=one / two chooses, for
// the measurement; both give the same bits, every comparison is on f32 values and integers and nothing is accumulated
// in floating point across threads.
//
// In slot mode (ContinuousGenerator(num_beams=W)) a prompt is admitted into row g·W of a group alone,
// and ergm_beam_seed gives the group's other rows the caption K | V and the state round 0 starts from.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"

namespace ergm {

constexpr int BM_THREADS = 1024;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_MAXW = 8;

struct BmCand {
    float c;
    int tok;  // < 0: no candidate
};

struct BmShared {
    unsigned long long wred[2][BM_WAVES];
    unsigned long long sred[BM_WAVES];
    float red[BM_WAVES];
    BmCand cand[BM_MAXW * BM_MAXW];  // the one-launch form's candidates
};

// f32 -> u32 whose unsigned order is the float order (-inf lowest); a candidate's key is that word above the
// complement of its token, so the largest key is the largest c and, among equals, the lowest token.  0 = no candidate
__device__ __forceinline__ uint32_t bm_ord(float c) {
    const uint32_t u = __float_as_uint(c);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bm_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

__device__ __forceinline__ unsigned long long bm_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long bm_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The top W candidates of one live row, best first, into out[0 .. W): all 1,024 threads of the workgroup call it.
// Thread t holds the `per` consecutive tokens from t·per.  A logit that is not finite is no candidate and has no part
// in the maximum or the mass.
template <int NPT>
__device__ __forceinline__ void bm_row_top(const float* __restrict__ row, int V, float score, int W, BmShared& sm, BmCand* out) {
    const int t = threadIdx.x;
    const int per = (V + BM_THREADS - 1) / BM_THREADS;
    const int i0 = t * per;
    const int nv = max(0, min(per, V - i0));
    float c[NPT];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const float x = j < nv ? row[i0 + j] : __builtin_nanf("");
        c[j] = fabsf(x) < INFINITY ? x : __builtin_nanf("");
        mx = fmaxf(mx, c[j]);  // fmaxf drops a NaN
    }
    mx = wave_max(mx);
    __syncthreads();  // the caller's earlier use of sm
    if ((t & 63) == 0) sm.red[t >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < BM_WAVES; ++w) mx = fmaxf(mx, sm.red[w]);
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const float e = expf(c[j] - mx);
        mine += e >= 0.f ? (unsigned long long)(e * 1073741824.f) : 0ull;
    }
    mine = bm_wave_sum(mine);
    if ((t & 63) == 0) sm.sred[t >> 6] = mine;
    __syncthreads();
    unsigned long long S = 0;
#pragma unroll
    for (int w = 0; w < BM_WAVES; ++w) S += sm.sred[w];
    // ln of the mass, once per row; a row with no finite logit has S = 0 and every c[j] a NaN already
    const float lz = (float)log((double)S * (1.0 / 1073741824.0));
#pragma unroll
    for (int j = 0; j < NPT; ++j) c[j] = score + ((c[j] - mx) - lz);
    for (int k = 0; k < W; ++k) {
        float bc = 0.f;
        int bj = -1;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const float cj = c[j];
            if (cj == cj && (bj < 0 || cj > bc)) bc = cj, bj = j;  // the first of equals: the lowest token
        }
        unsigned long long key = bj < 0 ? 0ull : ((unsigned long long)bm_ord(bc) << 32) | (0xFFFFFFFFu - (uint32_t)(i0 + bj));
        key = bm_wave_max(key);
        if ((t & 63) == 0) sm.wred[k & 1][t >> 6] = key;
        __syncthreads();  // one barrier per round: round k + 1 writes the other half
#pragma unroll
        for (int w = 0; w < BM_WAVES; ++w) key = max(key, sm.wred[k & 1][w]);
        const int tok = key ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1;
        if (t == 0) out[k] = BmCand{key ? bm_unord((uint32_t)(key >> 32)) : 0.f, tok};
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (i0 + j == tok) c[j] = __builtin_nanf("");
    }
}

// The group stage: the first wave of the workgroup ranks the candidates of group g (cand[w·W + k]: beam w's k-th best,
// read for live beams only), takes the best W and writes the W rows.  Every input is read before anything is written.
__device__ __forceinline__ void bm_merge(const BmCand* cand, int g, int W, float* __restrict__ scores,
                                         uint8_t* __restrict__ finished, int64_t eos_id, int* __restrict__ parent_out,
                                         int64_t* __restrict__ token_out) {
    const int lane = threadIdx.x;  // < 64
    const int r0 = g * W;
    const int w = lane / W, k = lane - w * W;
    // lane (w, k): beam w's candidate k
    bool valid = false;
    float c = 0.f;
    int tok = -1;
    bool fin = false;
    if (w < W) {
        const float sc = scores[r0 + w];
        fin = finished[r0 + w] != 0;
        if (sc > -INFINITY) {  // a NaN score is a dead beam as -inf is
            if (fin) {
                valid = k == 0, c = sc, tok = (int)eos_id;
            } else {
                const BmCand q = cand[w * W + k];
                valid = q.tok >= 0, c = q.c, tok = q.tok;
            }
        }
    }
    // how many candidates beat this one: larger c, then the lower beam, then the lower token
    int rank = 0;
    for (int o = 0; o < W * W; ++o) {
        const bool ov = __shfl(valid ? 1 : 0, o, 64) != 0;
        const float oc = __shfl(c, o, 64);
        const int ot = __shfl(tok, o, 64);
        const int ow = o / W;
        if (ov && (oc > c || (oc == c && (ow < w || (ow == w && ot < tok))))) ++rank;
    }
    const bool sel = valid && rank < W;
    const unsigned long long selmask = __ballot(sel);
    const unsigned wmask = (1u << W) - 1u;
    // beams with a child; the children of the beams below this one that do not stay in their parent's row
    unsigned has_child = 0;
    int extra_below = 0, n_sel = 0;
    for (int b = 0; b < W; ++b) {
        const int n = __popc((unsigned)(selmask >> (b * W)) & wmask);
        if (n) has_child |= 1u << b;
        if (b < w) extra_below += max(n - 1, 0);
        n_sel += n;
    }
    if (sel) {
        // this child's place among its beam's children by token
        int pos = 0;
        for (int o = 0; o < W; ++o) {
            const int src = w * W + o;
            const int ot = __shfl(tok, src, 64);
            if (((selmask >> src) & 1ull) && ot < tok) ++pos;
        }
        int dest = w;
        if (pos > 0) {  // the e-th child without a row of its own takes the e-th childless row
            int e = extra_below + pos - 1;
            dest = -1;
            for (int r = 0; r < W; ++r)
                if (!((has_child >> r) & 1u) && e-- == 0) dest = r;
        }
        if (dest >= 0) {
            parent_out[r0 + dest] = r0 + w;
            token_out[r0 + dest] = tok;
            scores[r0 + dest] = c;
            finished[r0 + dest] = (fin || tok == eos_id) ? 1 : 0;
        }
    }
    // fewer than W candidates: the childless rows no child fills die
    if (lane < W && !((has_child >> lane) & 1u)) {
        const int idx = __popc(~has_child & ((1u << lane) - 1u));  // this row's place among the childless
        if (idx >= n_sel - __popc(has_child)) {
            parent_out[r0 + lane] = r0 + lane;
            token_out[r0 + lane] = eos_id;
            scores[r0 + lane] = -INFINITY;
            finished[r0 + lane] = 1;
        }
    }
}

// a row takes part in the row stage when it is live: not finished and its score above -inf
__device__ __forceinline__ bool bm_live(const float* scores, const uint8_t* finished, int r) {
    return scores[r] > -INFINITY && finished[r] == 0;
}

template <int NPT>
__global__ __launch_bounds__(BM_THREADS) void beam_rows_kernel(const float* __restrict__ logits, int ldl, int V, int W,
                                                               const float* __restrict__ scores,
                                                               const uint8_t* __restrict__ finished, BmCand* __restrict__ ws) {
    __shared__ BmShared sm;
    const int r = blockIdx.x;
    if (!bm_live(scores, finished, r)) return;  // uniform: the row's logits are not read
    bm_row_top<NPT>(logits + (size_t)r * ldl, V, scores[r], W, sm, ws + (size_t)r * W);
}

__global__ __launch_bounds__(64) void beam_merge_kernel(const BmCand* __restrict__ ws, int W, float* scores, uint8_t* finished,
                                                        int64_t eos_id, int* parent_out, int64_t* token_out) {
    bm_merge(ws + (size_t)blockIdx.x * W * W, blockIdx.x, W, scores, finished, eos_id, parent_out, token_out);
}

template <int NPT>
__global__ __launch_bounds__(BM_THREADS) void beam_group_kernel(const float* __restrict__ logits, int ldl, int V, int W,
                                                                float* scores, uint8_t* finished, int64_t eos_id,
                                                                int* parent_out, int64_t* token_out) {
    __shared__ BmShared sm;
    const int g = blockIdx.x;
    for (int w = 0; w < W; ++w) {
        const int r = g * W + w;
        if (!bm_live(scores, finished, r)) continue;  // uniform
        bm_row_top<NPT>(logits + (size_t)r * ldl, V, scores[r], W, sm, sm.cand + w * W);
    }
    __syncthreads();
    if (threadIdx.x < 64) bm_merge(sm.cand, g, W, scores, finished, eos_id, parent_out, token_out);
}

// ---- the caches follow the beams ------------------------------------------------------------------------------
constexpr int BG_MAX_LAYERS = 48;  // cache pointers of one launch, in the kernel arguments
constexpr int BG_ROWS = 64;        // cache rows of one workgroup
struct BgLayers {
    char* p[BG_MAX_LAYERS];
};

// Workgroup (r, layer, chunk): cache rows [chunk·64, chunk·64 + 64) below lens[parent[r]] of the layer from slot
// parent[r] to slot r, 16 bytes per lane, a wave per cache row.  A row is moved only when its parent lies in its own
// group and keeps its own row (select's slot assignment gives nothing else), so no slot is read and written; the
// length is clamped to [0, max_len] before an address is formed.
__global__ __launch_bounds__(256) void beam_gather_kernel(BgLayers layers, int64_t ld_seq, int64_t ld_row, int row_bytes,
                                                          const int* __restrict__ parent, int* __restrict__ lens, int W,
                                                          int max_len, int write_lens) {
    const int r = blockIdx.x, g0 = r - r % W;
    const int p = parent[r];
    if (p == r || p < g0 || p >= g0 + W) return;  // uniform over the workgroup
    if (parent[p] != p) return;
    const int n = max(0, min(lens[p], max_len));
    if (write_lens && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) lens[r] = n;
    const int lane = threadIdx.x & 63;
    const int i1 = min(n, (int)(blockIdx.z + 1) * BG_ROWS);
    char* base = layers.p[blockIdx.y];
    for (int i = blockIdx.z * BG_ROWS + (threadIdx.x >> 6); i < i1; i += 4) {
        const char* s = base + (int64_t)p * ld_seq + (int64_t)i * ld_row;
        char* d = base + (int64_t)r * ld_seq + (int64_t)i * ld_row;
        for (int c = lane * 16; c < row_bytes; c += 64 * 16)
            *reinterpret_cast<uint4*>(d + c) = *reinterpret_cast<const uint4*>(s + c);
    }
}

// ---- seeding a group of slots (slot mode) ---------------------------------------------------------------------------
// The per-row state of the groups an admission filled: thread (b, w) for row w of group groups[b].  Row g·W is the
// admission's and only its score is written; the rows behind it read that row's caption length and bound, which
// nothing here writes, so every row has one writer and one launch needs no ordering inside it.
__global__ void beam_seed_state_kernel(const int* __restrict__ groups, int n_grp, int W, int G, int cap_max, int* lens,
                                       int* cap_lens, int* stop_lens, uint8_t* __restrict__ finished,
                                       float* __restrict__ scores) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_grp * W) return;
    const int b = t / W, w = t - b * W;
    const int g = groups[b];
    if (g < 0 || g >= G) return;
    const int r0 = g * W, r = r0 + w;
    if (w == 0) {
        scores[r0] = 0.f;
        return;
    }
    cap_lens[r] = max(0, min(cap_lens[r0], cap_max));
    stop_lens[r] = stop_lens[r0];
    lens[r] = 0;
    finished[r] = 0;
    scores[r] = -INFINITY;
}

// Workgroup ((b, w), layer, chunk): caption rows [chunk·64, chunk·64 + 64) below cap_lens[g·W] of the layer from slot
// g·W to slot g·W + w, w >= 1: the gather's layout, 16 bytes per lane, a wave per cache row.  The group id is checked
// and the length clamped to [0, cap_max] before an address is formed.
__global__ __launch_bounds__(256) void beam_seed_copy_kernel(BgLayers layers, int64_t ld_seq, int64_t ld_row, int row_bytes,
                                                             const int* __restrict__ groups, const int* __restrict__ cap_lens,
                                                             int W, int G, int cap_max) {
    const int b = blockIdx.x / (W - 1), w = 1 + blockIdx.x % (W - 1);
    const int g = groups[b];
    if (g < 0 || g >= G) return;  // uniform over the workgroup
    const int r0 = g * W;
    const int n = max(0, min(cap_lens[r0], cap_max));
    const int lane = threadIdx.x & 63;
    const int i1 = min(n, (int)(blockIdx.z + 1) * BG_ROWS);
    char* base = layers.p[blockIdx.y];
    for (int i = blockIdx.z * BG_ROWS + (threadIdx.x >> 6); i < i1; i += 4) {
        const char* s = base + (int64_t)r0 * ld_seq + (int64_t)i * ld_row;
        char* d = base + (int64_t)(r0 + w) * ld_seq + (int64_t)i * ld_row;
        for (int c = lane * 16; c < row_bytes; c += 64 * 16)
            *reinterpret_cast<uint4*>(d + c) = *reinterpret_cast<const uint4*>(s + c);
    }
}

// ERGM_BEAM_SELECT=one: the one-launch form; anything else, or unset: two launches
static bool beam_select_one() {
    static const bool one = [] {
        const char* e = getenv("ERGM_BEAM_SELECT");
        return e && !strcmp(e, "one");
    }();
    return one;
}
int beam_select_launches() { return beam_select_one() ? 1 : 2; }
int beam_gather_launches(int n_layer) { return cdiv(n_layer, BG_MAX_LAYERS); }

}  // namespace ergm

using namespace ergm;

extern "C" size_t ergm_beam_select_workspace_size(int R, int W) {
    if (R <= 0 || W < 1 || W > BM_MAXW) return 0;
    return (size_t)R * W * sizeof(BmCand);
}

extern "C" int ergm_beam_select(const float* logits, int ldl, int R, int W, int V, float* scores, uint8_t* finished,
                                int64_t eos_id, int* parent_out, int64_t* token_out, void* workspace, size_t ws_bytes,
                                void* stream) {
    ERGM_CHECK_ARG(logits && scores && finished && parent_out && token_out, "beam_select: null argument");
    ERGM_CHECK_ARG(W >= 1 && W <= BM_MAXW, "beam_select: W %d outside [1, %d]", W, BM_MAXW);
    ERGM_CHECK_ARG(R > 0 && R % W == 0, "beam_select: R %d is not a positive multiple of W %d", R, W);
    ERGM_CHECK_ARG(V >= W && ldl >= V && V <= 52 * BM_THREADS, "beam_select: bad shape V %d (W %d <= V <= %d) ldl %d", V, W,
                   52 * BM_THREADS, ldl);
    ERGM_CHECK_ARG(eos_id >= 0 && eos_id < V, "beam_select: eos_id %lld outside [0, V %d)", (long long)eos_id, V);
    ERGM_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                       ws_bytes >= ergm_beam_select_workspace_size(R, W),
                   "beam_select: workspace null, not 8-byte aligned or below %zu bytes", ergm_beam_select_workspace_size(R, W));
    hipStream_t s = as_stream(stream);
    auto* ws = reinterpret_cast<BmCand*>(workspace);
    const int per = cdiv(V, BM_THREADS), G = R / W;
    if (beam_select_one()) {
#define ERGM_BEAM(NPT) \
    ERGM_LAUNCH((beam_group_kernel<NPT>), dim3(G), dim3(BM_THREADS), 0, s, logits, ldl, V, W, scores, finished, eos_id, parent_out, token_out)
        if (per <= 4) ERGM_BEAM(4);
        else if (per <= 16) ERGM_BEAM(16);
        else ERGM_BEAM(52);
#undef ERGM_BEAM
        return check_launch("beam_select");
    }
#define ERGM_BEAM(NPT) \
    ERGM_LAUNCH((beam_rows_kernel<NPT>), dim3(R), dim3(BM_THREADS), 0, s, logits, ldl, V, W, scores, finished, ws)
    if (per <= 4) ERGM_BEAM(4);
    else if (per <= 16) ERGM_BEAM(16);
    else ERGM_BEAM(52);
#undef ERGM_BEAM
    ERGM_LAUNCH(beam_merge_kernel, dim3(G), dim3(64), 0, s, ws, W, scores, finished, eos_id, parent_out, token_out);
    return check_launch("beam_select");
}

extern "C" int ergm_beam_gather(void* const* caches, int n_layer, int64_t ld_seq, int64_t ld_row, int row_bytes,
                                const int* parent, int* lens, int R, int W, int max_len, void* stream) {
    ERGM_CHECK_ARG(caches && parent && lens, "beam_gather: null argument");
    ERGM_CHECK_ARG(W >= 1 && W <= BM_MAXW, "beam_gather: W %d outside [1, %d]", W, BM_MAXW);
    ERGM_CHECK_ARG(R > 0 && R % W == 0 && R <= 65535 * W, "beam_gather: R %d is not a positive multiple of W %d", R, W);
    ERGM_CHECK_ARG(n_layer >= 1 && max_len >= 1, "beam_gather: bad shape n_layer %d max_len %d", n_layer, max_len);
    ERGM_CHECK_ARG(row_bytes > 0 && row_bytes % 16 == 0 && ld_seq % 16 == 0 && ld_row % 16 == 0,
                   "beam_gather: row_bytes and the strides (bytes) must be multiples of 16");
    ERGM_CHECK_ARG(ld_row >= row_bytes && ld_seq >= (int64_t)(max_len - 1) * ld_row + row_bytes,
                   "beam_gather: stride shorter than the rows it spans");
    for (int l = 0; l < n_layer; ++l)
        ERGM_CHECK_ARG(caches[l] && aligned16(caches[l]), "beam_gather: layer %d cache pointer null or not 16-byte aligned", l);
    const int chunks = cdiv(max_len, BG_ROWS);
    ERGM_CHECK_ARG(chunks <= 65535, "beam_gather: max_len %d too large", max_len);
    hipStream_t s = as_stream(stream);
    for (int l0 = 0; l0 < n_layer; l0 += BG_MAX_LAYERS) {
        const int nl = std::min(BG_MAX_LAYERS, n_layer - l0);
        BgLayers L{};
        for (int l = 0; l < nl; ++l) L.p[l] = reinterpret_cast<char*>(caches[l0 + l]);
        ERGM_LAUNCH(beam_gather_kernel, dim3(R, nl, chunks), dim3(256), 0, s, L, ld_seq, ld_row, row_bytes, parent, lens, W, max_len,
                    l0 == 0 ? 1 : 0);
    }
    return check_launch("beam_gather");
}

extern "C" int ergm_beam_seed(void* const* xkv, int n_layer, int64_t ld_seq, int64_t ld_row, int row_bytes,
                              const int* groups_dev, const int* groups, int n_grp, int W, int max_batch, int cap_max, int* lens,
                              int* cap_lens, int* stop_lens, uint8_t* finished, float* scores, void* stream) {
    ERGM_CHECK_ARG(xkv && groups_dev && groups && lens && cap_lens && stop_lens && finished && scores, "beam_seed: null argument");
    ERGM_CHECK_ARG(W >= 1 && W <= BM_MAXW, "beam_seed: W %d outside [1, %d]", W, BM_MAXW);
    ERGM_CHECK_ARG(max_batch > 0 && max_batch % W == 0, "beam_seed: max_batch %d is not a positive multiple of W %d", max_batch, W);
    const int G = max_batch / W;
    ERGM_CHECK_ARG(n_grp >= 1 && n_grp <= G, "beam_seed: n_grp %d outside [1, %d groups]", n_grp, G);
    unsigned char seen[(1 << 16) / 8] = {};
    ERGM_CHECK_ARG(G <= (1 << 16), "beam_seed: more than 65536 groups");
    for (int b = 0; b < n_grp; ++b) {
        const int g = groups[b];
        ERGM_CHECK_ARG(g >= 0 && g < G, "beam_seed: group %d (entry %d) outside [0, %d)", g, b, G);
        ERGM_CHECK_ARG(!(seen[g >> 3] & (1 << (g & 7))), "beam_seed: group %d named twice", g);
        seen[g >> 3] |= (unsigned char)(1 << (g & 7));
    }
    ERGM_CHECK_ARG(n_layer >= 1 && cap_max >= 1, "beam_seed: bad shape n_layer %d cap_max %d", n_layer, cap_max);
    ERGM_CHECK_ARG(row_bytes > 0 && row_bytes % 16 == 0 && ld_seq % 16 == 0 && ld_row % 16 == 0,
                   "beam_seed: row_bytes and the strides (bytes) must be multiples of 16");
    ERGM_CHECK_ARG(ld_row >= row_bytes && ld_seq >= (int64_t)(cap_max - 1) * ld_row + row_bytes,
                   "beam_seed: stride shorter than the rows it spans");
    for (int l = 0; l < n_layer; ++l)
        ERGM_CHECK_ARG(xkv[l] && aligned16(xkv[l]), "beam_seed: layer %d cache pointer null or not 16-byte aligned", l);
    const int chunks = cdiv(cap_max, BG_ROWS);
    ERGM_CHECK_ARG(chunks <= 65535, "beam_seed: cap_max %d too large", cap_max);
    hipStream_t s = as_stream(stream);
    // the copies first: they read cap_lens[g·W] only, which the state kernel leaves alone
    for (int l0 = 0; W > 1 && l0 < n_layer; l0 += BG_MAX_LAYERS) {
        const int nl = std::min(BG_MAX_LAYERS, n_layer - l0);
        BgLayers L{};
        for (int l = 0; l < nl; ++l) L.p[l] = reinterpret_cast<char*>(xkv[l0 + l]);
        ERGM_LAUNCH(beam_seed_copy_kernel, dim3(n_grp * (W - 1), nl, chunks), dim3(256), 0, s, L, ld_seq, ld_row, row_bytes, groups_dev,
                    cap_lens, W, G, cap_max);
    }
    ERGM_LAUNCH(beam_seed_state_kernel, dim3(cdiv(n_grp * W, 256)), dim3(256), 0, s, groups_dev, n_grp, W, G, cap_max, lens, cap_lens,
                stop_lens, finished, scores);
    return check_launch("beam_seed");
}
