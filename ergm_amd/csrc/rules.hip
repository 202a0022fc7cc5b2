// Logit rules of generation (ergm_hip.h, "Logit rules"): the no-repeat n-gram ban and the bad-word ban over the ordered
// token history of every row, and the upkeep of that history: the ids of an admission or extension (hist_write), the
// token a live row just took (hist_append), and the beams' reordering (hist_follow, ergm_beam_gather's rule).
//
// Every kernel is a handful of integer compares per row and sits on the launch floor; none reads a logit.  What the
// device arrays hold is checked before it forms an address.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace ergm {

constexpr int RL_THREADS = 256;
constexpr int RL_HIST = 1024;  // history positions staged in LDS (4 KB)

// One workgroup per row.  The history [0, L) is staged in LDS; threads stride over the candidate positions of the
// n-gram rule and over the sequences of the bad-word list.  A ban is a plain 4-byte store of -inf: two threads that
// ban the same token store the same bits, so there is no atomic and no order to depend on.
__global__ __launch_bounds__(RL_THREADS) void logit_rules_kernel(float* __restrict__ logits, int ldl, int V,
                                                                 const int32_t* __restrict__ hist, int ld_hist,
                                                                 const int* __restrict__ start, const int* __restrict__ ngram,
                                                                 const int32_t* __restrict__ bad, int ld_bad,
                                                                 const int* __restrict__ lens,
                                                                 const uint8_t* __restrict__ finished, int eos_id, int max_len) {
    __shared__ int32_t h[RL_HIST];
    const int r = blockIdx.x, t = threadIdx.x;
    if (finished && finished[r]) return;  // uniform over the workgroup
    int n = ngram ? ngram[r] : 0;
    if (n < 1 || n > ERGM_NGRAM_MAX) n = 0;
    const int32_t* words = bad ? bad + (size_t)r * ld_bad : nullptr;
    const bool any_word = words && words[0] >= 1 && words[0] <= ERGM_NGRAM_MAX;
    if (n == 0 && !any_word) return;  // uniform
    const int L = max(0, min(lens[r], max_len));  // max_len <= RL_HIST <= ld_hist (host)
    const int32_t* src = hist + (size_t)r * ld_hist;
    for (int i = t; i < L; i += RL_THREADS) h[i] = src[i];
    __syncthreads();
    float* row = logits + (size_t)r * ldl;
    const float ninf = -INFINITY;
    if (n) {
        const int s0 = max(0, min(start ? start[r] : 0, L));
        const int tail = L - (n - 1);  // first position of the tail; tail >= s0 is the rule's "L - s0 >= n - 1"
        if (tail >= s0) {
            for (int i = s0 + t; i + n - 1 <= L - 1; i += RL_THREADS) {
                bool same = true;
                for (int k = 0; k < n - 1; ++k) same &= h[i + k] == h[tail + k];
                const int32_t j = h[i + n - 1];
                if (same && j >= 0 && j < V && j != eos_id) row[j] = ninf;
            }
        }
    }
    if (any_word) {
        // every thread walks the length prefixes (uniform loads); sequence number `idx` belongs to thread idx % 256
        int q = 0;
        for (int idx = 0; q < ld_bad; ++idx) {
            const int m = words[q];
            if (m < 1 || m > ERGM_NGRAM_MAX || q + m >= ld_bad) break;  // terminator, or a sequence the pool cuts off
            if (idx % RL_THREADS == t && m - 1 <= L) {
                bool same = true;
                for (int k = 0; k < m - 1; ++k) same &= h[L - (m - 1) + k] == words[q + 1 + k];
                const int32_t j = words[q + m];
                if (same && j >= 0 && j < V && j != eos_id) row[j] = ninf;
            }
            q += 1 + m;
        }
    }
}

// One workgroup per sequence: its packed ids to hist[slot][pos0 ..), nothing at or past max_len.  An id that is no
// int32 is stored as -1, which bans nothing and matches nothing in a vocabulary.
__global__ __launch_bounds__(RL_THREADS) void hist_write_kernel(const int64_t* __restrict__ ids, int total,
                                                                const int* __restrict__ slot, const int* __restrict__ start,
                                                                const int* __restrict__ len, const int* __restrict__ pos0,
                                                                int n_slots, int32_t* __restrict__ hist, int ld_hist,
                                                                int max_len) {
    const int b = blockIdx.x;
    const int sl = slot[b];
    if (sl < 0 || sl >= n_slots) return;  // uniform over the workgroup
    int n = max(0, min(len[b], total));
    const int s0 = max(0, min(start[b], total - n));
    const int p0 = max(0, min(pos0 ? pos0[b] : 0, max_len));
    n = min(n, max_len - p0);
    int32_t* dst = hist + (size_t)sl * ld_hist + p0;
    for (int i = threadIdx.x; i < n; i += RL_THREADS) {
        const int64_t id = ids[s0 + i];
        dst[i] = id < 0 || id > INT32_MAX ? -1 : (int32_t)id;
    }
}

// hist[r][lens[r]] = the token row r just took, for the rows still live; nothing at or past max_len
__global__ void hist_append_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ lens,
                                   const uint8_t* __restrict__ finished, int R, int32_t* __restrict__ hist, int ld_hist,
                                   int max_len) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || (finished && finished[r])) return;
    const int L = lens[r];
    if (L < 0 || L >= max_len) return;
    const int64_t id = tokens[r];
    hist[(size_t)r * ld_hist + L] = id < 0 || id > INT32_MAX ? -1 : (int32_t)id;
}

// One workgroup per row: positions [0, lens[parent[r]]) of row parent[r] to row r, under beam_gather_kernel's rule (a
// row moves only when its parent lies in its own group and keeps its own row), so no row is both read and written.
__global__ __launch_bounds__(RL_THREADS) void hist_follow_kernel(int32_t* __restrict__ hist, int ld_hist,
                                                                 const int* __restrict__ parent, const int* __restrict__ lens,
                                                                 int W, int max_len) {
    const int r = blockIdx.x, g0 = r - r % W;
    const int p = parent[r];
    if (p == r || p < g0 || p >= g0 + W) return;  // uniform over the workgroup
    if (parent[p] != p) return;
    const int n = max(0, min(lens[p], max_len));
    const int32_t* s = hist + (size_t)p * ld_hist;
    int32_t* d = hist + (size_t)r * ld_hist;
    for (int i = threadIdx.x; i < n; i += RL_THREADS) d[i] = s[i];
}

}  // namespace ergm

using namespace ergm;

extern "C" int ergm_logit_rules_apply(float* logits, int ldl, int R, int V, const ergm_logit_rules* rules, const int* lens,
                                      const uint8_t* finished, int64_t eos_id, int max_len, void* stream) {
    ERGM_CHECK_ARG(logits && rules && lens, "logit_rules_apply: null argument");
    ERGM_CHECK_ARG(R >= 1 && R <= 65535, "logit_rules_apply: R %d outside [1, 65535]", R);
    ERGM_CHECK_ARG(V >= 1 && V <= 53248 && ldl >= V, "logit_rules_apply: bad shape V %d (1 <= V <= 53248) ldl %d", V, ldl);
    ERGM_CHECK_ARG(max_len >= 1 && max_len <= RL_HIST, "logit_rules_apply: max_len %d outside [1, %d]", max_len, RL_HIST);
    ERGM_CHECK_ARG(eos_id >= 0 && eos_id < V, "logit_rules_apply: eos_id %lld outside [0, V %d)", (long long)eos_id, V);
    ERGM_CHECK_ARG(rules->hist && rules->ld_hist >= max_len, "logit_rules_apply: null hist or ld_hist %d < max_len %d",
                   rules->ld_hist, max_len);
    const bool words = rules->bad != nullptr;
    ERGM_CHECK_ARG(!words || rules->ld_bad >= 1, "logit_rules_apply: ld_bad %d < 1", rules->ld_bad);
    if (!rules->ngram && !words) return ERGM_OK;  // both rules off in every row: nothing to launch
    ERGM_LAUNCH(logit_rules_kernel, dim3(R), dim3(RL_THREADS), 0, as_stream(stream), logits, ldl, V, rules->hist, rules->ld_hist,
                rules->start, rules->ngram, rules->bad, rules->ld_bad, lens, finished, (int)eos_id, max_len);
    return check_launch("logit_rules_apply");
}

extern "C" int ergm_hist_write(const int64_t* ids, int total, const int* slot, const int* start, const int* len,
                               const int* pos0, int n_seq, int n_slots, int32_t* hist, int ld_hist, int max_len, void* stream) {
    ERGM_CHECK_ARG(ids && slot && start && len && hist, "hist_write: null argument");
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= 65535 && total >= 1 && n_slots >= 1, "hist_write: bad shape n_seq %d total %d n_slots %d",
                   n_seq, total, n_slots);
    ERGM_CHECK_ARG(max_len >= 1 && ld_hist >= max_len, "hist_write: max_len %d < 1 or ld_hist %d below it", max_len, ld_hist);
    ERGM_LAUNCH(hist_write_kernel, dim3(n_seq), dim3(RL_THREADS), 0, as_stream(stream), ids, total, slot, start, len, pos0,
                n_slots, hist, ld_hist, max_len);
    return check_launch("hist_write");
}

extern "C" int ergm_hist_append(const int64_t* tokens, const int* lens, const uint8_t* finished, int R, int32_t* hist,
                                int ld_hist, int max_len, void* stream) {
    ERGM_CHECK_ARG(tokens && lens && hist, "hist_append: null argument");
    ERGM_CHECK_ARG(R >= 1, "hist_append: R %d < 1", R);
    ERGM_CHECK_ARG(max_len >= 1 && ld_hist >= max_len, "hist_append: max_len %d < 1 or ld_hist %d below it", max_len, ld_hist);
    ERGM_LAUNCH(hist_append_kernel, dim3(cdiv(R, RL_THREADS)), dim3(RL_THREADS), 0, as_stream(stream), tokens, lens, finished, R,
                hist, ld_hist, max_len);
    return check_launch("hist_append");
}

extern "C" int ergm_hist_follow(int32_t* hist, int ld_hist, const int* parent, const int* lens, int R, int W, int max_len,
                                void* stream) {
    ERGM_CHECK_ARG(hist && parent && lens, "hist_follow: null argument");
    ERGM_CHECK_ARG(W >= 1 && W <= 8, "hist_follow: W %d outside [1, 8]", W);
    ERGM_CHECK_ARG(R > 0 && R % W == 0 && R <= 65535, "hist_follow: R %d is not a positive multiple of W %d up to 65535", R, W);
    ERGM_CHECK_ARG(max_len >= 1 && ld_hist >= max_len, "hist_follow: max_len %d < 1 or ld_hist %d below it", max_len, ld_hist);
    ERGM_LAUNCH(hist_follow_kernel, dim3(R), dim3(RL_THREADS), 0, as_stream(stream), hist, ld_hist, parent, lens, W, max_len);
    return check_launch("hist_follow");
}
