// ergm_linear_rows (ergm_hip.h): C = epi(A'·W + bias) for a handful of rows (a decode step: M = batch <= 32),
// A' = A (bf16) or the LayerNorm of f32 rows computed by the workgroup itself.
//
// The weights are streamed once; FLOPs are not the limit, the number of workgroups and the loads in flight are.
// Decomposition: a workgroup of 8 waves owns a strip of 16 columns and a group of 32 rows (grid = N/16 x M/32).
// K is cut into 32-deep steps and the steps are dealt to the 8 waves in contiguous slices; each wave streams its
// slice of W straight from global memory into VGPRs (LR_U steps issued before the first is used) and accumulates
// 2 x v_mfma_f32_16x16x32_bf16 per step.  The 8 partial tiles meet in LDS and are summed in wave order 0..7 by the
// thread that stores the element: one launch, no workspace, no atomics, the same bits in every run.  An E x E
// projection (N = 768) runs on 48 workgroups x 8 waves with every byte of W requested in the first round trip; so
// does the K = 3072 contraction (12 steps per wave, LR_UDEEP in flight).
//
// [K][N] weights (Conv1D): the MFMA B fragment is k-strided, so a wave writes each 32 x 16 piece lane-linearly
// (ds_write_b128: lane l = row l/2, half l%2) into a private 1-KiB LDS slot and reads it back transposed with
// ds_read_b64_tr_b16 (lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3: byte 8·(4q+p) of the
// group's 128 contiguous bytes).  LDS operations of one wave execute in order: no barrier inside the loop.
// [N][K] weights (the tied LM head): the 16 bytes a lane loads are its B fragment.
//
// Rows at or past M are never loaded (their addresses are clamped to the last valid row of the group) and never
// stored; an output element is a function of its own row of A / x and its own column of W only, computed by the
// same instructions wherever the row sits: row r of an M = 32 call equals the M = 1 call on that row bitwise.
// The LayerNorm prologue: wave w computes mean and rstd of rows w, w+8, w+16, w+24 in fp32 (two passes: the sum,
// then the sum of squared deviations; for K <= 1024 over registers, all four rows loaded in one round trip, which
// took the fused c_attn launch from 13.9 to 10.6 us at B = 32) and leaves them in LDS; the A fragments are then
// formed from x, γ, β as ln_fwd forms them and rounded once to bf16.  The rows come from L2, once per column strip.
#include "common.h"

namespace ergm {

constexpr int LR_WAVES = 8;
constexpr int LR_THREADS = 64 * LR_WAVES;
constexpr int LR_BN = 16;      // columns of a strip: one MFMA fragment
constexpr int LR_ROWS = 32;    // rows of a group: two MFMA fragments
constexpr int LR_U = 4;        // K steps of W a wave requests before it uses the first (LR_UDEEP for a deep K)
constexpr int LR_UDEEP = 12;
constexpr int LR_RED_BYTES = LR_WAVES * LR_ROWS * LR_BN * 4;
constexpr int LR_STAT_BYTES = LR_ROWS * 2 * 4;
constexpr int LR_SLOT = 32 * LR_BN * 2;  // one 32 x 16 bf16 piece of W
constexpr int LR_LDS = LR_RED_BYTES + LR_STAT_BYTES + LR_WAVES * LR_U * LR_SLOT;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;  // 16 bytes of W in registers

struct LrArgs {
    const void* a;   // bf16 [M][lda], or f32 [M][lda] with the LayerNorm prologue
    int lda;
    const float* gamma;
    const float* beta;
    float eps;
    const __bf16* w;
    int ldw;
    void* c;
    int ldc;
    const float* bias;
    const float* aux;
    int ld_aux;
    int M, N, K, epi;
};

template <bool KN, bool LN, int U>
__global__ __launch_bounds__(LR_THREADS) void linear_rows_kernel(const LrArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[LR_LDS];
    float* red = reinterpret_cast<float*>(smem);                    // [wave][row][col]
    float* stat = reinterpret_cast<float*>(smem + LR_RED_BYTES);    // [row]{mean, rstd}
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // wave: scalar branches
    char* slots = smem + LR_RED_BYTES + LR_STAT_BYTES + wave * (LR_U * LR_SLOT);
    // Workgroup ids go round the 8 XCDs, each with its own L2; four neighbouring strips of [K][N] weights share every
    // 128-byte line.  Give XCD x (ids = x mod 8) a contiguous run of strips, so a line is fetched into one L2, not four
    // (a speed choice only: any placement computes the same values).
    const int nst = gridDim.x, xcd = blockIdx.x & 7, q8 = nst >> 3, r8 = nst & 7;
    const int strip = xcd * q8 + min(xcd, r8) + (blockIdx.x >> 3);
    const int n0 = strip * LR_BN, row0 = blockIdx.y * LR_ROWS;
    const int rows = min(LR_ROWS, p.M - row0);  // valid rows of this group, >= 1
    const int K = p.K;

    if constexpr (LN) {
        const float* x = reinterpret_cast<const float*>(p.a);
        const float inv_k = 1.0f / (float)K;
        if (K <= 1024) {
            // the wave's 4 rows in registers, every load issued before the first reduction: one round trip to L2.
            // Rows past the group and columns past K are clamped to valid addresses and masked out of the sums.
            float4 v[LR_ROWS / LR_WAVES][4];
#pragma unroll
            for (int rr = 0; rr < LR_ROWS / LR_WAVES; ++rr) {
                const float* xr = x + (size_t)(row0 + min(wave + LR_WAVES * rr, rows - 1)) * p.lda;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[rr][i] = *reinterpret_cast<const float4*>(xr + min((i * 64 + lane) * 4, K - 4));
            }
#pragma unroll
            for (int rr = 0; rr < LR_ROWS / LR_WAVES; ++rr) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) s += (i * 64 + lane) * 4 < K ? (v[rr][i].x + v[rr][i].y) + (v[rr][i].z + v[rr][i].w) : 0.f;
                const float mean = wave_sum(s) * inv_k;
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = v[rr][i].x - mean, b = v[rr][i].y - mean, cc = v[rr][i].z - mean, d = v[rr][i].w - mean;
                    q += (i * 64 + lane) * 4 < K ? (a * a + b * b) + (cc * cc + d * d) : 0.f;
                }
                const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_k + p.eps);
                const int r = wave + LR_WAVES * rr;
                if (lane == 0 && r < rows) {
                    stat[2 * r] = mean;
                    stat[2 * r + 1] = rstd;
                }
            }
        } else {
            for (int r = wave; r < rows; r += LR_WAVES) {
                const float* xr = x + (size_t)(row0 + r) * p.lda;
                float s = 0.f;
                for (int c = lane * 4; c < K; c += 256) {
                    const float4 v = *reinterpret_cast<const float4*>(xr + c);
                    s += (v.x + v.y) + (v.z + v.w);
                }
                const float mean = wave_sum(s) * inv_k;
                float q = 0.f;
                for (int c = lane * 4; c < K; c += 256) {
                    const float4 v = *reinterpret_cast<const float4*>(xr + c);
                    const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
                    q += (a * a + b * b) + (cc * cc + d * d);
                }
                const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_k + p.eps);
                if (lane == 0) {
                    stat[2 * r] = mean;
                    stat[2 * r + 1] = rstd;
                }
            }
        }
        __syncthreads();
    }

    // this wave's slice of the K steps
    const int steps = K >> 5, per = (steps + LR_WAVES - 1) / LR_WAVES;
    const int s0 = min(steps, wave * per), s1 = min(steps, s0 + per);
    const int fr = lane & 15, fg = lane >> 4;  // fragment row / column and k group of this lane
    // rows of the two A fragments, clamped into the group
    const int ar0 = min(fr, rows - 1), ar1 = min(16 + fr, rows - 1);
    const bool two = rows > 16;
    const __bf16* wl;  // this lane's piece of step 0
    if constexpr (KN) wl = p.w + (size_t)(lane >> 1) * p.ldw + min(n0 + 8 * (lane & 1), p.N - 8);
    else wl = p.w + (size_t)min(n0 + fr, p.N - 1) * p.ldw + 8 * fg;
    const size_t wstep = KN ? (size_t)32 * p.ldw : 32;

    auto a_frag = [&](int r, int s) -> bf16x8 {
        const int k = 32 * s + 8 * fg;
        if constexpr (!LN) {
            return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(p.a) + (size_t)(row0 + r) * p.lda + k);
        } else {
            const float* xr = reinterpret_cast<const float*>(p.a) + (size_t)(row0 + r) * p.lda + k;
            const float4 x0 = *reinterpret_cast<const float4*>(xr), x1 = *reinterpret_cast<const float4*>(xr + 4);
            const float4 g0 = *reinterpret_cast<const float4*>(p.gamma + k), g1 = *reinterpret_cast<const float4*>(p.gamma + k + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(p.beta + k), b1 = *reinterpret_cast<const float4*>(p.beta + k + 4);
            const float mean = stat[2 * r], rstd = stat[2 * r + 1];
            bf16x8 o;
            o[0] = f2bf((x0.x - mean) * rstd * g0.x + b0.x);
            o[1] = f2bf((x0.y - mean) * rstd * g0.y + b0.y);
            o[2] = f2bf((x0.z - mean) * rstd * g0.z + b0.z);
            o[3] = f2bf((x0.w - mean) * rstd * g0.w + b0.w);
            o[4] = f2bf((x1.x - mean) * rstd * g1.x + b1.x);
            o[5] = f2bf((x1.y - mean) * rstd * g1.y + b1.y);
            o[6] = f2bf((x1.z - mean) * rstd * g1.z + b1.z);
            o[7] = f2bf((x1.w - mean) * rstd * g1.w + b1.w);
            return o;
        }
    };

    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int sb = s0; sb < s1; sb += U) {  // wave-uniform bounds: EXEC stays full (the transposed read needs it)
        u32x4 wr[U];
        bf16x8 fa0[U], fa1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // steps past the slice re-load its last step (valid memory), unused
            const int s = min(sb + u, s1 - 1);
            wr[u] = *reinterpret_cast<const u32x4*>(wl + (size_t)s * wstep);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = min(sb + u, s1 - 1);
            fa0[u] = a_frag(ar0, s);
            fa1[u] = a_frag(ar1, s);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (sb + u < s1) {
                bf16x8 fb;
                if constexpr (KN) {
                    char* slot = slots + (u % LR_U) * LR_SLOT;  // in-order LDS: a slot is re-used behind its read
                    *reinterpret_cast<u32x4*>(slot + 16 * lane) = wr[u];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const char* rp = slot + 256 * fg + 8 * fr;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, rp));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, rp + 128));
                    typedef __attribute__((ext_vector_type(8))) short s16x8;
                    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    fb = __builtin_bit_cast(bf16x8, r);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();  // the next round's write to this slot stays behind the read
                } else {
                    fb = __builtin_bit_cast(bf16x8, wr[u]);
                }
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0[u], fb, acc0, 0, 0, 0);
                if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1[u], fb, acc1, 0, 0, 0);
            }
        }
    }

    // partial tiles to LDS (C fragment: column lane & 15, rows 4·(lane >> 4) + i), then the sum in wave order
    float* mine = red + wave * (LR_ROWS * LR_BN);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mine[(4 * fg + i) * LR_BN + fr] = acc0[i];
        mine[(16 + 4 * fg + i) * LR_BN + fr] = acc1[i];
    }
    __syncthreads();
    const int r = threadIdx.x >> 4, cl = threadIdx.x & 15, n = n0 + cl;
    if (r >= rows || n >= p.N) return;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < LR_WAVES; ++w) v += red[w * (LR_ROWS * LR_BN) + r * LR_BN + cl];
    const size_t m = (size_t)(row0 + r);
    if (p.epi != ERGM_EPI_NONE) v += p.bias[n];
    switch (p.epi) {
        case ERGM_EPI_NONE: reinterpret_cast<float*>(p.c)[m * p.ldc + n] = v; break;
        case ERGM_EPI_BIAS: reinterpret_cast<__bf16*>(p.c)[m * p.ldc + n] = f2bf(v); break;
        case ERGM_EPI_BIAS_GELU: reinterpret_cast<__bf16*>(p.c)[m * p.ldc + n] = f2bf(gelu_new(v)); break;
        default: reinterpret_cast<float*>(p.c)[m * p.ldc + n] = p.aux[m * p.ld_aux + n] + v; break;
    }
}

}  // namespace ergm

using namespace ergm;

extern "C" int ergm_linear_rows(const ergm_linear_rows_desc* d, const void* A, const void* W, void* C, void* stream) {
    ERGM_CHECK_ARG(d && A && W && C, "linear_rows: null argument");
    ERGM_CHECK_ARG(d->M >= 1 && d->M <= 65535 * LR_ROWS, "linear_rows: M %d outside [1, %d]", d->M, 65535 * LR_ROWS);
    ERGM_CHECK_ARG(d->K >= 64 && d->K % 64 == 0, "linear_rows: K %d must be a positive multiple of 64", d->K);
    ERGM_CHECK_ARG(d->N >= 8 && d->N % 8 == 0, "linear_rows: N %d must be a positive multiple of 8", d->N);
    ERGM_CHECK_ARG(d->w_layout == ERGM_KN || d->w_layout == ERGM_NK, "linear_rows: bad weight layout %d", d->w_layout);
    ERGM_CHECK_ARG((d->ln_gamma != nullptr) == (d->ln_beta != nullptr), "linear_rows: LayerNorm needs both gamma and beta");
    const bool ln = d->ln_gamma != nullptr;
    ERGM_CHECK_ARG(!ln || (d->ln_eps >= 0.f && d->ln_eps == d->ln_eps), "linear_rows: bad LayerNorm eps");
    ERGM_CHECK_ARG(d->lda >= d->K && d->lda % (ln ? 4 : 8) == 0, "linear_rows: lda %d (K %d; a multiple of %d elements)",
                   d->lda, d->K, ln ? 4 : 8);
    const int wmin = d->w_layout == ERGM_KN ? d->N : d->K;
    ERGM_CHECK_ARG(d->ldw >= wmin && d->ldw % 8 == 0, "linear_rows: ldw %d (at least %d, a multiple of 8 elements)", d->ldw,
                   wmin);
    ERGM_CHECK_ARG(d->ldc >= d->N, "linear_rows: ldc %d < N %d", d->ldc, d->N);
    ERGM_CHECK_ARG(aligned16(A) && aligned16(W) && (!ln || (aligned16(d->ln_gamma) && aligned16(d->ln_beta))),
                   "linear_rows: 16-byte alignment of A, W, gamma, beta");
    ERGM_CHECK_ARG(d->epilogue >= ERGM_EPI_NONE && d->epilogue <= ERGM_EPI_BIAS_RESID, "linear_rows: unsupported epilogue %d",
                   d->epilogue);
    ERGM_CHECK_ARG(d->epilogue == ERGM_EPI_NONE || d->bias, "linear_rows: the epilogue needs a bias");
    ERGM_CHECK_ARG(d->epilogue != ERGM_EPI_BIAS_RESID || (d->aux && d->ld_aux >= d->N),
                   "linear_rows: BIAS_RESID needs aux with ld_aux >= N");
    const bool c_f32 = d->epilogue == ERGM_EPI_NONE || d->epilogue == ERGM_EPI_BIAS_RESID;
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(C) & (c_f32 ? 3 : 1)) == 0, "linear_rows: C misaligned");
    LrArgs a{A, d->lda, d->ln_gamma, d->ln_beta, d->ln_eps, reinterpret_cast<const __bf16*>(W), d->ldw, C, d->ldc,
             d->bias, d->aux, d->ld_aux, d->M, d->N, d->K, d->epilogue};
    const dim3 grid(cdiv(d->N, LR_BN), cdiv(d->M, LR_ROWS));
    hipStream_t s = as_stream(stream);
    // a contraction of more than LR_U steps per wave keeps LR_UDEEP of them in flight (the LayerNorm form, whose
    // operand costs 4x the registers, stays at LR_U)
    const bool deep = !ln && cdiv(d->K / 32, LR_WAVES) > LR_U;
    if (d->w_layout == ERGM_KN) {
        if (ln) ERGM_LAUNCH((linear_rows_kernel<true, true, LR_U>), grid, dim3(LR_THREADS), 0, s, a);
        else if (deep) ERGM_LAUNCH((linear_rows_kernel<true, false, LR_UDEEP>), grid, dim3(LR_THREADS), 0, s, a);
        else ERGM_LAUNCH((linear_rows_kernel<true, false, LR_U>), grid, dim3(LR_THREADS), 0, s, a);
    } else {
        if (ln) ERGM_LAUNCH((linear_rows_kernel<false, true, LR_U>), grid, dim3(LR_THREADS), 0, s, a);
        else if (deep) ERGM_LAUNCH((linear_rows_kernel<false, false, LR_UDEEP>), grid, dim3(LR_THREADS), 0, s, a);
        else ERGM_LAUNCH((linear_rows_kernel<false, false, LR_U>), grid, dim3(LR_THREADS), 0, s, a);
    }
    return check_launch("linear_rows");
}
