// ergm_lm_score (ergm_hip.h): the tied LM head and the log-softmax of every row in one pass, without the logits.
//
// For row r and the columns j < V, x_j = Σ_k X[r][k]·W[j][k] (v_mfma_f32_16x16x32_bf16, f32 accumulators, never rounded
// to bf16); the row's outputs are lse = m + logf(Σ exp(x_j - m)), the first column of the largest x_j with its value,
// and x_target - lse.  Nothing of size R x V touches memory.
//
// Decomposition.  The vocabulary is cut into partitions of LS_PW = LS_TPP·LS_BN columns, a function of V alone; a
// workgroup of 4 waves owns LS_BM rows and one partition (grid = row tiles x partitions, row tiles fastest so the
// workgroups in flight share the partition's rows of W).  Its column tiles and their K steps form one sequence of
// stages through a 3-slot LDS ring (OperandRing: LDS-DMA, counted waits, one barrier per stage), so the ring stays
// full across a column tile's end.  Wave w holds rows 16w .. 16w+15 of the row tile against all LS_BN columns: 8
// accumulator fragments, lane l with column (l & 15) + 16j of fragment j and rows 4·(l >> 4) + i.
//
// Online softmax.  A lane keeps, for each of its 4 rows, the running (max, Σexp, argmax) over the columns it has seen
// (those congruent to l & 15 mod 16), updated once per column tile: the maximum of its 8 new values, one rescale of
// the running sum, 8 __expf.  Columns at or past V are -inf by a select on the column index, so a pad row of W never
// contributes whatever it holds (it is not even read: the DMA clamps its source rows to V - 1, and rows of X to
// R - 1).  The lane that meets a row's target column stores that logit to the workspace: one writer per row.  After
// the partition's last tile the 16 lanes of a row meet in a shuffle butterfly (xor 1, 2, 4, 8; ms_combine of
// xent.hip with the argmax riding along, ties to the lower column) and lane 0 of each 16 stores the row's partial.
// A second launch, one thread per row, folds the partials in partition order 0, 1, ... and writes the outputs.
// No atomics and no arrival counters: the same bits in every run; and since the partition and every order above
// depend on (V, K) only, a row's outputs are bitwise the same whatever other rows the call holds.
#include "tiles.h"

namespace ergm {

constexpr int LS_BM = 64;            // rows of a row tile
constexpr int LS_BN = 128;           // columns of a column tile
constexpr int LS_TPP = 4;            // column tiles of a partition
constexpr int LS_PW = LS_BN * LS_TPP;
constexpr int LS_WAVES = 4;
constexpr int LS_THREADS = 64 * LS_WAVES;
constexpr int LS_NS = 3;
constexpr int LS_FN = LS_BN / 16;
constexpr int LS_VMAX = 65536;
using LsRing = OperandRing<LS_BM, LS_BN, false, false, LS_NS, LS_WAVES>;
constexpr int LS_LDS = LS_NS * LsRing::STAGE;
static_assert(LS_BM == 16 * LS_WAVES, "one 16-row fragment per wave");

struct LsArgs {
    const __bf16* A;  // X
    int lda, M;
    const __bf16* B;  // W
    int ldb, N;       // N = V: the DMA clamps its rows of W below it
    const int64_t* targets;
    int K, P;
    float* pm;        // [P][M] partial maxima
    float* ps;        // [P][M] partial Σexp(x - max)
    int* pi;          // [P][M] partial argmax
    float* xt;        // [M] target logits (scored rows only)
};

// (m, s) <- (m, s) ⊕ (m2, s2) with the argmax: the larger maximum's column, ties to the lower column
__device__ __forceinline__ void ls_combine(float& m, float& s, int& idx, float m2, float s2, int idx2) {
    if (m2 > m || (m2 == m && idx2 < idx)) idx = idx2;
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) return;
    s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
    m = mn;
}

__global__ __launch_bounds__(LS_THREADS) void lm_score_kernel(const LsArgs a) {
    constexpr int STAGE = LsRing::STAGE, A_BYTES = LsRing::A_BYTES, LPS = LsRing::LPS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int m0 = blockIdx.x * LS_BM, part = blockIdx.y;
    const int c_begin = part * LS_PW, c_end = min(a.N, c_begin + LS_PW);
    const int nt = (c_end - c_begin + LS_BN - 1) / LS_BN;
    const int nk = a.K / GEMM_BK;
    const int total = nt * nk;

    // the stage issued next: K step ik of column tile it, into slot si
    int it = 0, ik = 0, si = 0;
    auto issue_next = [&]() {
        LsRing::issue(smem + si * STAGE, a, m0, c_begin + it * LS_BN, ik * GEMM_BK, wave);
        si = si + 1 == LS_NS ? 0 : si + 1;
        if (++ik == nk) {
            ik = 0;
            ++it;
        }
    };
#pragma unroll
    for (int s = 0; s < LS_NS - 1; ++s)
        if (s < total) issue_next();

    // this lane's 4 rows, their targets (-1: not scored) and running state
    const int row_base = m0 + wave * 16 + 4 * (lane >> 4);
    int tg[4], ri[4];
    float rm[4], rs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t t = row_base + i < a.M ? a.targets[row_base + i] : -1;
        tg[i] = (t >= 0 && t < a.N) ? (int)t : -1;
        rm[i] = -INFINITY;
        rs[i] = 0.f;
        ri[i] = 0x7fffffff;
    }

    FragReader<LS_BM, false> la;
    FragReader<LS_BN, false> lb;
    f32x4 acc[LS_FN];
#pragma unroll
    for (int j = 0; j < LS_FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int kt = 0, tile = 0, sc = 0;  // the stage consumed: K step kt of column tile `tile`, in slot sc
    for (int g = 0; g < total; ++g) {
        ring_sync<LPS, LS_NS>(min(LS_NS - 2, total - 1 - g));
        if (g + LS_NS - 1 < total) issue_next();
        const char* st = smem + sc * STAGE;
        sc = sc + 1 == LS_NS ? 0 : sc + 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 fa = la.frag(st, wave * 16, ks);
            bf16x8 fb[LS_FN];
#pragma unroll
            for (int j = 0; j < LS_FN; ++j) fb[j] = lb.frag(st + A_BYTES, j * 16, ks);
#pragma unroll
            for (int j = 0; j < LS_FN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[j], acc[j], 0, 0, 0);
        }
        if (++kt < nk) continue;
        kt = 0;
        // the column tile is complete: fold its 8 values per row into the lane's running state
        const int cb = c_begin + tile * LS_BN + (lane & 15);
        ++tile;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float x[LS_FN];
            float tmax = -INFINITY;
            int tidx = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < LS_FN; ++j) {
                const int col = cb + 16 * j;
                x[j] = col < c_end ? acc[j][i] : -INFINITY;
                if (col == tg[i]) a.xt[row_base + i] = x[j];
                if (x[j] > tmax) {  // ascending columns: the first maximum stays
                    tmax = x[j];
                    tidx = col;
                }
            }
            if (tmax > rm[i]) ri[i] = tidx;
            const float mn = fmaxf(rm[i], tmax);
            if (mn != -INFINITY) {
                float s = rs[i] * __expf(rm[i] - mn);
#pragma unroll
                for (int j = 0; j < LS_FN; ++j) s += __expf(x[j] - mn);
                rs[i] = s;
                rm[i] = mn;
            }
        }
#pragma unroll
        for (int j = 0; j < LS_FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // the 16 lanes of a row (every wave is whole here: the shuffles see all of them)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float m2 = __shfl_xor(rm[i], off, 64), s2 = __shfl_xor(rs[i], off, 64);
            const int i2 = __shfl_xor(ri[i], off, 64);
            ls_combine(rm[i], rs[i], ri[i], m2, s2, i2);
        }
    }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row_base + i;
            if (row < a.M) {
                const size_t o = (size_t)part * a.M + row;
                a.pm[o] = rm[i];
                a.ps[o] = rs[i];
                a.pi[o] = ri[i];
            }
        }
    }
}

__global__ __launch_bounds__(256) void lm_score_combine_kernel(const LsArgs a, float* __restrict__ logprob,
                                                               float* __restrict__ lse_out, float* __restrict__ top1_logit,
                                                               int* __restrict__ top1) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.M) return;
    float m = a.pm[r], s = a.ps[r];
    int idx = a.pi[r];
    for (int p = 1; p < a.P; ++p) {
        const size_t o = (size_t)p * a.M + r;
        ls_combine(m, s, idx, a.pm[o], a.ps[o], a.pi[o]);
    }
    const float lse = m + logf(s);
    if (lse_out) lse_out[r] = lse;
    if (top1_logit) top1_logit[r] = m;
    if (top1) top1[r] = min(max(idx, 0), a.N - 1);
    if (logprob) {
        const int64_t t = a.targets[r];
        logprob[r] = (t >= 0 && t < a.N) ? a.xt[r] - lse : 0.0f;
    }
}

int lm_score_launches() { return 2; }  // the partition kernel and the fold

}  // namespace ergm

using namespace ergm;

static bool ls_dims_ok(int R, int V, int K) { return R >= 1 && V >= 1 && V <= LS_VMAX && K >= 64 && K % 64 == 0; }

extern "C" size_t ergm_lm_score_workspace_size(int R, int V, int K) {
    if (!ls_dims_ok(R, V, K)) return 0;
    const size_t P = (size_t)cdiv(V, LS_PW);
    return (3 * P + 1) * (size_t)R * 4;
}

extern "C" int ergm_lm_score(const void* X, int ldx, const void* W, int ldw, const int64_t* targets, int R, int V, int K,
                             float* logprob, float* lse, float* top1_logit, int* top1, void* workspace, size_t ws_bytes,
                             void* stream) {
    ERGM_CHECK_ARG(X && W && targets, "lm_score: null argument");
    ERGM_CHECK_ARG(R >= 1, "lm_score: R %d < 1", R);
    ERGM_CHECK_ARG(V >= 1 && V <= LS_VMAX, "lm_score: V %d outside [1, %d]", V, LS_VMAX);
    ERGM_CHECK_ARG(K >= 64 && K % 64 == 0, "lm_score: K %d must be a positive multiple of 64", K);
    ERGM_CHECK_ARG(ldx >= K && ldx % 8 == 0, "lm_score: ldx %d (at least K %d, a multiple of 8 elements)", ldx, K);
    ERGM_CHECK_ARG(ldw >= K && ldw % 8 == 0, "lm_score: ldw %d (at least K %d, a multiple of 8 elements)", ldw, K);
    ERGM_CHECK_ARG(aligned16(X) && aligned16(W), "lm_score: 16-byte alignment of X and W");
    const size_t need = ergm_lm_score_workspace_size(R, V, K);
    ERGM_CHECK_ARG(workspace && ws_bytes >= need, "lm_score: workspace %zu bytes < %zu", workspace ? ws_bytes : (size_t)0, need);
    ERGM_CHECK_ARG(aligned16(workspace), "lm_score: workspace must be 16-byte aligned");
    const int P = cdiv(V, LS_PW), tiles = cdiv(R, LS_BM);
    ERGM_CHECK_ARG(R <= 0x7fffffff - LS_BM, "lm_score: R %d too large", R);
    float* ws = reinterpret_cast<float*>(workspace);
    const size_t plane = (size_t)P * R;
    LsArgs a{reinterpret_cast<const __bf16*>(X), ldx, R, reinterpret_cast<const __bf16*>(W), ldw, V, targets, K, P,
             ws, ws + plane, reinterpret_cast<int*>(ws + 2 * plane), ws + 3 * plane};
    static const hipError_t once =
        hipFuncSetAttribute((const void*)lm_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS);
    (void)once;
    hipStream_t s = as_stream(stream);
    ERGM_LAUNCH(lm_score_kernel, dim3(tiles, P), dim3(LS_THREADS), LS_LDS, s, a);
    ERGM_LAUNCH(lm_score_combine_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, a, logprob, lse, top1_logit, top1);
    return check_launch("lm_score");
}
