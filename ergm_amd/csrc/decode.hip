// Batched KV-cache generation for gfx950: decode attention of one query per sequence over a ragged cache,
// the embedding of one token per sequence at its own position, and nucleus (top-p) sampling of a batch of
// logit rows without a sort (ergm_hip.h: ergm_attn_decode, ergm_embed_rows, ergm_topp_sample, and ergm_sample_rows
// with its per-row sampling controls).
//
// Decode attention is a GEMV over the cache: VALU work behind 16-byte loads, no MFMA.  A workgroup of 4 waves
// owns one (split, head, sequence).  8 lanes share a key row (8 bf16 of the 64-wide head each), so one wave
// load covers 8 rows and a workgroup 32 rows per step, 4 steps in flight.  Each of the 32 key slots keeps
// its own online softmax (m, l, o[8 per lane]); the slots are merged in slot order in LDS, the splits of one
// (sequence, head) in split order by a second kernel, and the appended row is added last, from the qkv row
// itself.  No float atomics anywhere: the output does not depend on scheduling.
//
// Sampling works on integers.  e_i = expf(x_i - max) is quantised to q_i = floor(e_i·2^30); every sum (the
// softmax denominator, the mass above a threshold, the running sums of the draw) is a sum of those integers,
// so LDS integer atomics and any reduction order give the same result, and the kept set is exactly the rule
// of ergm_hip.h applied to the q_i.  The threshold (the smallest kept value) is found by a three-level
// histogram over the bit pattern of e_i (monotone for positive floats): 11 + 11 + 9 bits, each level refining
// the bin in which the mass above crosses top_p.
#include "common.h"

#include <algorithm>

namespace ergm {

constexpr int DEC_SLOTS = 32;       // key slots of a workgroup: 4 waves x 8 rows per wave load
constexpr int DEC_DEPTH = 4;        // rows per slot loaded before the first is used (8 measured no faster)
constexpr int DEC_MAX_SPLITS = 32;
constexpr int DEC_PART = 66;        // floats of one split's partial: m, l, o[64]

__device__ __forceinline__ void bf8_to_f32(const uint4& r, float* f) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

// Last stage, one full wave, lane d = head dimension d: (M, L, O) is the merged state over the cache rows.
// With `append` the new row joins from the qkv row (never read back from the cache), then O / L is stored.
__device__ __forceinline__ void decode_finish(float M, float Lsum, float O, int d, const __bf16* qrow, int E, bool append,
                                              __bf16* out) {
    if (append) {
        const float s = wave_sum(bf2f(qrow[d]) * bf2f(qrow[E + d])) * 0.125f;
        const float Mn = fmaxf(M, s);
        const float c = M == -INFINITY ? 0.f : expf(M - Mn);
        const float p = expf(s - Mn);
        Lsum = Lsum * c + p;
        O = O * c + p * bf2f(qrow[2 * E + d]);
    }
    out[d] = f2bf(Lsum > 0.f ? O / Lsum : 0.f);
}

__global__ __launch_bounds__(256) void attn_decode_kernel(const __bf16* __restrict__ qkv, int ld_qkv, __bf16* kc, __bf16* vc,
                                                          int64_t ld_seq, int ld_row, const int* __restrict__ lens,
                                                          int max_len, int append, int E, int splits,
                                                          float* __restrict__ ws, __bf16* __restrict__ out, int ldo) {
    __shared__ __attribute__((aligned(16))) float sm_o[DEC_SLOTS][64];
    __shared__ float sm_m[DEC_SLOTS], sm_l[DEC_SLOTS];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, slot = lane >> 3, part = lane & 7;
    const int n = max(0, min(lens[b], max_len - append));  // rows attended; the appended row goes to row n < max_len
    const __bf16* qrow = qkv + (size_t)b * ld_qkv + 64 * h;
    __bf16* kb = kc + (int64_t)b * ld_seq + 64 * h + 8 * part;
    __bf16* vb = vc + (int64_t)b * ld_seq + 64 * h + 8 * part;
    if (append && split == 0 && threadIdx.x < 16) {  // the new K | V row of this head, bitwise
        const int which = threadIdx.x >> 3;
        const uint4 r = *reinterpret_cast<const uint4*>(qrow + (1 + which) * E + 8 * part);
        *reinterpret_cast<uint4*>((which ? vb : kb) + (int64_t)n * ld_row) = r;
    }
    // keys [k0, k1) of this split: equal chunks of a multiple of 32 rows, the last ones possibly empty
    const int chunk = (int)((((int64_t)n + splits - 1) / splits + 31) & ~(int64_t)31);
    const int k0 = (int)min((int64_t)n, (int64_t)split * chunk), k1 = min(n, k0 + chunk);
    float q[8];
    bf8_to_f32(*reinterpret_cast<const uint4*>(qrow + 8 * part), q);
    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int base = k0; base < k1; base += DEC_DEPTH * DEC_SLOTS) {
        uint4 kr[DEC_DEPTH], vr[DEC_DEPTH];
#pragma unroll
        for (int u = 0; u < DEC_DEPTH; ++u) {
            const int t = base + u * DEC_SLOTS + wave * 8 + slot;
            kr[u] = vr[u] = make_uint4(0, 0, 0, 0);
            if (t < k1) {
                kr[u] = *reinterpret_cast<const uint4*>(kb + (int64_t)t * ld_row);
                vr[u] = *reinterpret_cast<const uint4*>(vb + (int64_t)t * ld_row);
            }
        }
#pragma unroll
        for (int u = 0; u < DEC_DEPTH; ++u) {
            const int t = base + u * DEC_SLOTS + wave * 8 + slot;
            float kf[8], vf[8];
            bf8_to_f32(kr[u], kf);
            bf8_to_f32(vr[u], vf);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s += q[i] * kf[i];
            s += __shfl_xor(s, 1, 64);  // the 8 lanes of a row end with the same sum
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            s *= 0.125f;
            if (t < k1) {
                const float mn = fmaxf(m, s);
                const float c = m == -INFINITY ? 0.f : expf(m - mn);
                const float p = expf(s - mn);
                l = l * c + p;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = acc[i] * c + p * vf[i];
                m = mn;
            }
        }
    }
    const int sl = wave * 8 + slot;
#pragma unroll
    for (int i = 0; i < 8; ++i) sm_o[sl][8 * part + i] = acc[i];
    if (part == 0) {
        sm_m[sl] = m;
        sm_l[sl] = l;
    }
    __syncthreads();
    if (wave != 0) return;
    float M = -INFINITY;
    for (int j = 0; j < DEC_SLOTS; ++j) M = fmaxf(M, sm_m[j]);
    float Lsum = 0.f, O = 0.f;
    for (int j = 0; j < DEC_SLOTS; ++j) {  // slot order
        const float w = sm_m[j] == -INFINITY ? 0.f : expf(sm_m[j] - M);
        Lsum += sm_l[j] * w;
        O += sm_o[j][lane] * w;
    }
    if (splits == 1) {
        decode_finish(M, Lsum, O, lane, qrow, E, append != 0, out + (size_t)b * ldo + 64 * h);
    } else {
        float* p = ws + ((size_t)(b * gridDim.y + h) * splits + split) * DEC_PART;
        if (lane == 0) {
            p[0] = M;
            p[1] = Lsum;
        }
        p[2 + lane] = O;
    }
}

// splits > 1: merge the partials of one (sequence, head) in split order, then the appended row.
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(const __bf16* __restrict__ qkv, int ld_qkv,
                                                               const float* __restrict__ ws, int splits, int append, int E,
                                                               __bf16* __restrict__ out, int ldo) {
    const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float* p = ws + (size_t)(b * gridDim.x + h) * splits * DEC_PART;
    // lane s holds split s's (m, l) and its weight; the o rows are independent loads, summed in split order
    const float ms = lane < splits ? p[lane * DEC_PART] : -INFINITY;
    const float ls = lane < splits ? p[lane * DEC_PART + 1] : 0.f;
    const float M = wave_max(ms);
    const float w = ms == -INFINITY ? 0.f : expf(ms - M);
    float Lsum = 0.f, O = 0.f;
#pragma unroll 8
    for (int s = 0; s < splits; ++s) {
        const float ws_ = __shfl(w, s, 64);
        Lsum += __shfl(ls, s, 64) * ws_;
        O += p[s * DEC_PART + 2 + lane] * ws_;
    }
    decode_finish(M, Lsum, O, lane, qkv + (size_t)b * ld_qkv + 64 * h, E, append != 0, out + (size_t)b * ldo + 64 * h);
}

// Workgroups for the 256 CUs, while every split keeps at least 256 rows of the longest possible cache: measured at
// B·H = 12, a 1,024-row cache takes 15.7 us unsplit and 7.2 + 4 us (merge launch) in 4 splits, a 128-row cache 5.2 us
// however it is split (profiles/r08_attn_decode_splits.txt), so shorter chunks only add the merge.
static int decode_split_cap(int max_len) { return std::min(DEC_MAX_SPLITS, std::max(1, max_len / 256)); }
static int decode_auto_splits(int B, int H, int max_len) {
    const int cap = decode_split_cap(max_len);
    const int64_t bh = (int64_t)B * H;
    return (int)std::min<int64_t>(cap, std::max<int64_t>(1, (256 + bh - 1) / bh));
}

// ---- embedding of one token per sequence -----------------------------------------------------------
__global__ __launch_bounds__(256) void embed_rows_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
                                                         const int* __restrict__ pos, const float* __restrict__ wte,
                                                         const float* __restrict__ wpe, float* __restrict__ h, int E, int V,
                                                         int n_positions) {
    const int b = blockIdx.x;
    const int64_t id = min(max(ids[b], (int64_t)0), (int64_t)V - 1);
    const int64_t ty = tt ? tt[b] : -1;
    const int p = min(max(pos[b], 0), n_positions - 1);
    const bool ok_ty = ty >= 0 && ty < V;
    for (int c = threadIdx.x * 4; c < E; c += 1024) {  // ergm_embed_fwd's order: (wte[id] + wpe[p]) + wte[tt]
        float4 x = *reinterpret_cast<const float4*>(wte + (size_t)id * E + c);
        const float4 w = *reinterpret_cast<const float4*>(wpe + (size_t)p * E + c);
        x.x += w.x; x.y += w.y; x.z += w.z; x.w += w.w;
        if (ok_ty) {
            const float4 y = *reinterpret_cast<const float4*>(wte + (size_t)ty * E + c);
            x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        }
        *reinterpret_cast<float4*>(h + (size_t)b * E + c) = x;
    }
}

// ---- nucleus sampling --------------------------------------------------------------------------------
constexpr int TP_THREADS = 1024;
constexpr int TP_BINS = 2048;
constexpr int TP_CNT_SHIFT = 47;  // a histogram word: count << 47 | mass (mass <= 53,248 · 2^30 < 2^46)
constexpr unsigned long long TP_MASS_MASK = (1ull << TP_CNT_SHIFT) - 1;

struct TpShared {
    unsigned long long hist[TP_BINS];
    unsigned long long scan[TP_THREADS];
    unsigned long long pick[2];
    float red[TP_THREADS / 64];
    int sel;
    float mx;  // the row maximum, kept for the log-probability (in the struct's tail padding: the size stays 24,664 B)
};

// Exclusive prefix sum over the 1,024 threads in thread order (Hillis-Steele in LDS); `total` = the sum.
__device__ __forceinline__ unsigned long long tp_scan(unsigned long long v, unsigned long long* buf,
                                                      unsigned long long& total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < TP_THREADS; off <<= 1) {
        const unsigned long long a = t >= off ? buf[t - off] : 0ull;
        __syncthreads();
        buf[t] += a;
        __syncthreads();
    }
    total = buf[TP_THREADS - 1];
    const unsigned long long incl = buf[t];
    __syncthreads();
    return incl - v;
}

// e < 0 marks a slot that holds no token (past V, or a NaN logit): no mass, never counted
__device__ __forceinline__ unsigned long long tp_q(float e) { return (unsigned long long)(fmaxf(e, 0.f) * 1073741824.f); }
// The row lives in registers across several unrolled passes; an opaque copy per use keeps the compiler from
// carrying each pass's derived values (64-bit masses, predicates) along with it, which spills.
__device__ __forceinline__ float tp_use(float e) {
    asm volatile("" : "+v"(e));
    return e;
}

// The controls of ergm_sample_ctl (ergm_sample_rows).  NaN, infinite or <= 0 acts as 1
__device__ __forceinline__ float sm_scale(const float* p, int b) {
    const float v = p ? p[b] : 1.f;
    return (v > 0.f && v < INFINITY) ? v : 1.f;
}
// the repetition penalty on the logit of a token the row has seen
__device__ __forceinline__ float sm_penalty(float x, float rep) { return x < 0.f ? x * rep : __fdiv_rn(x, rep); }

// The sampler: one workgroup per row; thread t holds the `per` consecutive tokens from t·per in registers.
// CTL = false is nucleus sampling alone (ergm_topp_sample, ergm_topp_sample_rows): the counter's row and step are
// row_ids[b] / row_steps[b] where given, else the workgroup's own row and the call's `step`; `ctl` and `logprob` are
// not read.  CTL = true adds the controls of ergm_sample_ctl (ergm_sample_rows; row_ids and row_steps are given): the
// penalty, the eos mask and the temperature act on the registers right behind the load, so the passes below see a
// row as CTL = false sees it.  The threshold search runs once more, ahead of the mass search and with the packed
// count as its criterion, for the rows that ask for top-k (uniform over the workgroup); its result is a few uniform
// values carried across the mass search.  Everything CTL adds stands under `if constexpr`, so a row with no control
// asked of it gives the same bits from either instantiation and CTL = false pays for none of it.  The order of the
// arguments and of the first statements is measured, not free: with `logprob` and `ctl` last the arguments CTL = false
// reads keep their kernarg offsets, and the register allocation of both instantiations follows from it (DESIGN.md
// §12.4).
template <int NPT, bool CTL>
__global__ __launch_bounds__(TP_THREADS) void sample_kernel(const float* __restrict__ logits, int ldl, int V, float top_p,
                                                            uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                            const uint32_t* __restrict__ row_ids,
                                                            const uint32_t* __restrict__ row_steps, uint8_t* finished,
                                                            int64_t eos_id, int64_t* __restrict__ tokens,
                                                            int* __restrict__ kept, float* __restrict__ kept_mass,
                                                            float* __restrict__ logprob, ergm_sample_ctl ctl) {
    __shared__ TpShared sm;
    const int b = blockIdx.x, t = threadIdx.x;
    if (finished && finished[b]) {  // uniform over the workgroup
        if (t == 0) {
            tokens[b] = eos_id;
            if (kept) kept[b] = 0;
            if (kept_mass) kept_mass[b] = 0.f;
            if constexpr (CTL)
                if (logprob) logprob[b] = 0.f;
        }
        return;
    }
    const int per = (V + TP_THREADS - 1) / TP_THREADS;
    const int i0 = t * per;
    const int nv = max(0, min(per, V - i0));  // valid tokens of this thread: j < nv
    const float* row = logits + (size_t)b * ldl;
    // the counter's step: the row's own where given, else the call's; the row's bitmap (CTL)
    uint32_t cstep = step;
    uint32_t* seen = nullptr;
    if constexpr (CTL) {
        seen = ctl.seen ? ctl.seen + (size_t)b * ctl.ld_seen : nullptr;
        cstep = row_steps[b];
    }
    float e[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) e[j] = j < nv ? row[i0 + j] : -INFINITY;
    if constexpr (CTL) {
        // Steps 1 to 3 of the rule, each a pass of its own over the registers, taken only by the rows that ask for it:
        // the penalty's and the temperature's conditions are uniform over the workgroup (a factor of 1 changes no bit,
        // so skipping it is exact), the eos mask is the business of the one thread that holds eos.
        const float rep = sm_scale(ctl.rep_penalty, b);
        if (seen && rep != 1.f) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int idx = i0 + j;
                if (j < nv) {
                    if (j == 0 || (idx & 31) == 0) word = seen[idx >> 5];  // one read per 32 tokens
                    if ((word >> (idx & 31)) & 1u) e[j] = sm_penalty(e[j], rep);
                }
            }
        }
        // while the row is below its minimum length eos is a slot that holds no token, as a NaN logit is: no mass,
        // never counted
        if (ctl.min_step && cstep < ctl.min_step[b] && eos_id >= i0 && eos_id < i0 + nv) {
            const int eos_j = (int)eos_id - i0;
#pragma unroll
            for (int j = 0; j < NPT; ++j) e[j] = j == eos_j ? __builtin_nanf("") : e[j];
        }
        const float temp = sm_scale(ctl.temperature, b);
        if (temp != 1.f) {
#pragma unroll
            for (int j = 0; j < NPT; ++j) e[j] = __fdiv_rn(e[j], temp);
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPT; ++j) mx = fmaxf(mx, e[j]);
    mx = wave_max(mx);
    if ((t & 63) == 0) sm.red[t >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TP_THREADS / 64; ++w) mx = fmaxf(mx, sm.red[w]);
    if constexpr (CTL)
        if (t == 0) sm.mx = mx;
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const float x = expf(e[j] - mx);
        e[j] = (j < nv && x >= 0.f) ? x : -1.f;
        const unsigned long long q = tp_q(e[j]);
        if constexpr (CTL) mine += q ? (1ull << TP_CNT_SHIFT) | q : 0ull;  // count << 47 | mass of the tokens with mass
        else mine += q;
    }
    unsigned long long Sn;
    tp_scan(mine, sm.scan, Sn);
    const unsigned long long S = CTL ? Sn & TP_MASS_MASK : Sn;
    // the row's top_p and top-k, and the result of the top-k search (k != 0): the smallest value that remains, what
    // lies above it, its ties that remain
    float tp = top_p;
    unsigned k = 0, k_key = 0, k_ties = 0;
    unsigned long long k_above = 0;
    if constexpr (CTL) {
        if (ctl.top_p) tp = ctl.top_p[b];
        const int k_raw = ctl.top_k ? ctl.top_k[b] : 0;
        // top-k is on for 1 <= k < the number of tokens with mass
        k = (k_raw >= 1 && (unsigned long long)k_raw < (Sn >> TP_CNT_SHIFT)) ? (unsigned)k_raw : 0u;
    }
    // threshold search: after level p, `prefix` = the leading bits of the smallest kept value, `above` = count and
    // mass (packed) of the tokens whose value lies above every value with that prefix.  Pass 1 looks for the smallest
    // value with at most T of mass above it.  CTL with top-k: pass 0, ahead of it, looks for the smallest value with
    // fewer than k tokens above it, the same walk over the packed words by count.  CTL = false: the loop's condition
    // is the constant false, pass 1 is all there is.
    unsigned long long T = 0;
    unsigned prefix = 0;
    unsigned long long above = 0, in_bin = 0;
    int pass = k ? 0 : 1;
#pragma unroll 1
    do {
        const bool by_count = CTL && pass == 0;
        if (!by_count) {  // T over the mass S_k that remains under top-k
            const unsigned long long qk = tp_q(__uint_as_float(k_key));
            const unsigned long long Sk = k ? (k_above & TP_MASS_MASK) + k_ties * qk : S;
            const bool none = CTL ? !(tp > 0.f) : tp <= 0.f;  // a row's own top_p may be a NaN: the top token alone
            T = tp >= 1.f ? Sk : (none ? 0ull : (unsigned long long)((double)tp * (double)Sk));
            T = min(T, Sk);
        }
        const unsigned long long lim = by_count ? (unsigned long long)(k - 1) : T;
        prefix = 0, above = 0, in_bin = 0;
#pragma unroll 1
        for (int level = 0; level < 3; ++level) {
            const int shift = level == 0 ? 20 : (level == 1 ? 9 : 0);
            const int bits = level == 2 ? 9 : 11;
            sm.hist[t] = 0;
            sm.hist[t + TP_THREADS] = 0;
            if (t == 0) sm.sel = TP_BINS;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const float ej = tp_use(e[j]);
                const unsigned key = __float_as_uint(ej);
                if (ej >= 0.f && (level == 0 || (key >> (shift + bits)) == prefix))
                    atomicAdd(&sm.hist[(key >> shift) & ((1u << bits) - 1)], (1ull << TP_CNT_SHIFT) | tp_q(ej));
            }
            __syncthreads();
            // thread t owns bins bh > bl, the threads walk the bins downwards: an exclusive scan gives what lies above
            const int bh = TP_BINS - 1 - 2 * t, bl = bh - 1;
            const unsigned long long hh = sm.hist[bh], hl = sm.hist[bl];
            unsigned long long tot;
            const unsigned long long ah = above + tp_scan(hh + hl, sm.scan, tot), al = ah + hh;
            const unsigned long long ch = by_count ? ah >> TP_CNT_SHIFT : ah & TP_MASS_MASK;
            const unsigned long long cl = by_count ? al >> TP_CNT_SHIFT : al & TP_MASS_MASK;
            // the smallest non-empty bin whose top value still has at most `lim` above it holds the threshold
            if (hl && cl <= lim) atomicMin(&sm.sel, bl);
            else if (hh && ch <= lim) atomicMin(&sm.sel, bh);
            __syncthreads();
            const int sel = sm.sel;
            if (sel == bh || sel == bl) {
                sm.pick[0] = sel == bh ? ah : al;
                sm.pick[1] = sel == bh ? hh : hl;
            }
            __syncthreads();
            above = sm.pick[0];
            in_bin = sm.pick[1];
            prefix = (prefix << bits) | (unsigned)sel;
            __syncthreads();
        }
        if (by_count) {  // of the ties at the smallest remaining value, the k - (tokens above) lowest ids remain
            k_key = prefix, k_above = above;
            k_ties = min((unsigned)(in_bin >> TP_CNT_SHIFT), k - (unsigned)(above >> TP_CNT_SHIFT));
        }
    } while (CTL && ++pass < 2);
    // prefix = the bit pattern of the smallest kept value v; `in_bin` counts its ties, kept in token order while
    // the mass before each stays <= T
    unsigned vkey = prefix;
    const unsigned long long G = above & TP_MASS_MASK, qv = tp_q(__uint_as_float(vkey));
    const unsigned ties = (unsigned)(in_bin >> TP_CNT_SHIFT);
    unsigned keep_ties = qv == 0 ? ties : (unsigned)min((unsigned long long)ties, (T - G) / qv + 1);
    // top-p reaches past the ranks that remain under top-k (T = S_k): the top-k cut is the kept set
    if constexpr (CTL)
        if (k && (unsigned)(above >> TP_CNT_SHIFT) + keep_ties > k) vkey = k_key, above = k_above, keep_ties = k_ties;
    unsigned long long c_eq = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) c_eq += __float_as_uint(tp_use(e[j])) == vkey ? 1u : 0u;
    unsigned long long tot;
    unsigned rank = (unsigned)tp_scan(c_eq, sm.scan, tot);  // ties in lower token ids
    unsigned keepbits_lo = 0, keepbits_hi = 0;
    mine = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const float ej = tp_use(e[j]);
        const unsigned key = __float_as_uint(ej);
        bool kp = ej >= 0.f && key > vkey;
        if (key == vkey) kp = rank++ < keep_ties;
        if (kp) {
            mine += tp_q(ej);
            if (j < 32) keepbits_lo |= 1u << j;
            else keepbits_hi |= 1u << (j - 32);
        }
    }
    unsigned long long K;
    unsigned long long run = tp_scan(mine, sm.scan, K);
    // the draw: first kept token, in token order, whose running sum reaches u·K
    // the counter's row: per row where given (CTL: always), else the workgroup's own
    const uint32_t crow = CTL || row_ids ? row_ids[b] : (uint32_t)b;
    if constexpr (!CTL)
        if (row_steps) cstep = row_steps[b];
    const uint4 r = philox4x32_10(make_uint4(crow, 0u, 0xE5A3u, cstep), seed_lo, seed_hi);
    const double u = ((double)r.x + 0.5) * (1.0 / 4294967296.0);
    unsigned long long target = (unsigned long long)ceil(u * (double)K);
    target = max(1ull, min(target, K));
    if (t == 0) sm.sel = V - 1;
    __syncthreads();
    bool found = false;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const bool kp = j < 32 ? (keepbits_lo >> j) & 1u : (keepbits_hi >> (j - 32)) & 1u;
        if (kp) {
            run += tp_q(tp_use(e[j]));
            if (!found && run >= target) {
                found = true;
                atomicMin(&sm.sel, i0 + j);
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        const int tok = sm.sel;  // in [0, V): V - 1 or a valid token of some thread
        tokens[b] = tok;
        if (kept) kept[b] = (int)(above >> TP_CNT_SHIFT) + (int)keep_ties;
        if (kept_mass) kept_mass[b] = (float)((double)K / (double)S);
        if (finished && tok == eos_id) finished[b] = 1;
        if constexpr (CTL) {
            if (logprob) {  // the token's processed logit once more, from the row and the bitmap as the load saw them
                float x = row[tok];
                if (seen && (seen[tok >> 5] >> (tok & 31)) & 1u) x = sm_penalty(x, sm_scale(ctl.rep_penalty, b));
                x = __fdiv_rn(x, sm_scale(ctl.temperature, b));
                logprob[b] = (float)((double)(x - sm.mx) - log((double)S * (1.0 / 1073741824.0)));
            }
            if (seen) seen[tok >> 5] |= 1u << (tok & 31);  // this workgroup alone writes the row
        }
    }
}

// One workgroup per sequence: clear the slot's bitmap row, barrier, set the bits of the sequence's ids, and the
// turn's minimum length.  Everything read from the device arrays is checked before an address is formed.
__global__ __launch_bounds__(256) void sample_mark_kernel(const int64_t* __restrict__ ids, int total,
                                                          const int* __restrict__ slot, const int* __restrict__ start,
                                                          const int* __restrict__ len, const int* __restrict__ reset,
                                                          const int* __restrict__ min_new, int V, int n_slots,
                                                          uint32_t* __restrict__ seen, int ld_seen,
                                                          const uint32_t* __restrict__ row_steps,
                                                          uint32_t* __restrict__ min_step) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int sl = slot[b];
    if (sl < 0 || sl >= n_slots) return;  // uniform over the workgroup
    if (seen) {
        uint32_t* row = seen + (size_t)sl * ld_seen;
        if (reset && reset[b])
            for (int w = t; w < (V + 31) / 32; w += 256) row[w] = 0u;
        __syncthreads();
        const int n = max(0, min(len[b], total));
        const int s0 = max(0, min(start[b], total - n));
        for (int i = t; i < n; i += 256) {
            const int64_t id = ids[s0 + i];
            if (id >= 0 && id < V) atomicOr(&row[id >> 5], 1u << (id & 31));
        }
    }
    if (t == 0 && min_step) min_step[sl] = row_steps[sl] + (uint32_t)max(min_new ? min_new[b] : 0, 0);
}

// ---- the decode executor's integer helpers (decode_exec.cpp) -------------------------------------------
// lens[b] += !finished[b]: the sequences that have not drawn eos advance by the token just appended
__global__ void lens_advance_kernel(int* __restrict__ lens, const uint8_t* __restrict__ finished, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) lens[b] += finished[b] == 0 ? 1 : 0;
}
__global__ void fill_i64_kernel(int64_t* __restrict__ p, int64_t v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- continuous batching: packed rows into cache slots, and the slot state (decode_exec.cpp) -------------
// Row t of sequence b (packed row start[b] + t of src) goes to dst + slot[b]·ld_slot + t·ld_row; strides and
// row_bytes in bytes, 16-byte copies, one wave per row.  Everything read from the device arrays is checked before an
// address is formed: the length is clamped to [0, min(max_rows, slot_rows)], the start to the packed extent, and a
// sequence whose slot lies outside [0, n_slots) writes nothing.  dst_row0 (ergm_rows_to_slots_at; nullptr: 0): row t
// lands in slot row dst_row0[b] + t, the first row clamped to [0, slot_rows] and the length to the rows left after it.
__global__ __launch_bounds__(256) void rows_to_slots_kernel(const char* __restrict__ src, int64_t ld_src,
                                                            const int* __restrict__ start, const int* __restrict__ len,
                                                            const int* __restrict__ slot, int total_rows, int max_rows,
                                                            char* __restrict__ dst, int64_t ld_slot, int64_t ld_row,
                                                            int row_bytes, int n_slots, int slot_rows,
                                                            const int* __restrict__ dst_row0) {
    const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int d0 = dst_row0 ? max(0, min(dst_row0[b], slot_rows)) : 0;
    const int n = max(0, min(len[b], min(min(max_rows, slot_rows - d0), total_rows)));
    const int sl = slot[b];
    if (t >= n || sl < 0 || sl >= n_slots) return;
    const int r0 = max(0, min(start[b], total_rows - n));
    const char* s = src + (int64_t)(r0 + t) * ld_src;
    char* d = dst + (int64_t)sl * ld_slot + (int64_t)(d0 + t) * ld_row;
    for (int c = lane * 16; c < row_bytes; c += 64 * 16)
        *reinterpret_cast<uint4*>(d + c) = *reinterpret_cast<const uint4*>(s + c);
}

// The state of the slots an admission filled: one thread per admitted sequence.
__global__ void slots_admit_kernel(const int* __restrict__ slot, const int* __restrict__ n_tok, const int* __restrict__ n_cap,
                                   const int* __restrict__ max_new, const uint32_t* __restrict__ req, int n_seq, int n_slots,
                                   int max_len, int cap_max, int* __restrict__ lens, int* __restrict__ cap_lens,
                                   int* __restrict__ stop_lens, uint32_t* __restrict__ row_ids,
                                   uint32_t* __restrict__ row_steps, uint8_t* __restrict__ finished) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_seq) return;
    const int sl = slot[b];
    if (sl < 0 || sl >= n_slots) return;
    const int n = max(0, min(n_tok[b], max_len));
    lens[sl] = n;
    cap_lens[sl] = max(0, min(n_cap[b], cap_max));
    stop_lens[sl] = max(n, min(n + max(max_new[b], 0), max_len));
    row_ids[sl] = req[b];
    row_steps[sl] = 0u;
    finished[sl] = 0;
}

// The state of the slots an extension continued: the new length and bound, live again.  cap_lens, row_ids and
// row_steps stay: the captions are the admission's, and the request goes on drawing from fresh counters.
__global__ void slots_extend_kernel(const int* __restrict__ slot, const int* __restrict__ past, const int* __restrict__ n_new,
                                    const int* __restrict__ max_new, int n_seq, int n_slots, int max_len,
                                    int* __restrict__ lens, int* __restrict__ stop_lens, uint8_t* __restrict__ finished) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_seq) return;
    const int sl = slot[b];
    if (sl < 0 || sl >= n_slots) return;
    const int p = max(0, min(past[b], max_len));
    const int n = p + max(0, min(n_new[b], max_len - p));
    lens[sl] = n;
    stop_lens[sl] = max(n, min(n + max(max_new[b], 0), max_len));
    finished[sl] = 0;
}

// The length update of a step over every slot: a live row advances by the token just appended and its draw counter
// with it, and finishes when it reaches the bound recorded at its admission, so no row passes its bound whatever the
// host does between two looks.
__global__ void slots_advance_kernel(int* __restrict__ lens, uint32_t* __restrict__ row_steps, uint8_t* __restrict__ finished,
                                     const int* __restrict__ stop_lens, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || finished[b]) return;
    const int n = lens[b] + 1;
    lens[b] = n;
    row_steps[b] += 1u;
    if (n >= stop_lens[b]) finished[b] = 1;
}

int decode_slots_admit(const int* slot, const int* n_tok, const int* n_cap, const int* max_new, const uint32_t* req, int n_seq,
                       int n_slots, int max_len, int cap_max, int* lens, int* cap_lens, int* stop_lens, uint32_t* row_ids,
                       uint32_t* row_steps, uint8_t* finished, hipStream_t s) {
    ERGM_LAUNCH(slots_admit_kernel, dim3(cdiv(n_seq, 256)), dim3(256), 0, s, slot, n_tok, n_cap, max_new, req, n_seq, n_slots,
                max_len, cap_max, lens, cap_lens, stop_lens, row_ids, row_steps, finished);
    return check_launch("decode_slots_admit");
}
int decode_slots_extend(const int* slot, const int* past, const int* n_new, const int* max_new, int n_seq, int n_slots,
                        int max_len, int* lens, int* stop_lens, uint8_t* finished, hipStream_t s) {
    ERGM_LAUNCH(slots_extend_kernel, dim3(cdiv(n_seq, 256)), dim3(256), 0, s, slot, past, n_new, max_new, n_seq, n_slots, max_len,
                lens, stop_lens, finished);
    return check_launch("decode_slots_extend");
}
int decode_slots_advance(int* lens, uint32_t* row_steps, uint8_t* finished, const int* stop_lens, int B, hipStream_t s) {
    ERGM_LAUNCH(slots_advance_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, lens, row_steps, finished, stop_lens, B);
    return check_launch("decode_slots_advance");
}

int decode_lens_advance(int* lens, const uint8_t* finished, int B, hipStream_t s) {
    ERGM_LAUNCH(lens_advance_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, lens, finished, B);
    return check_launch("decode_lens_advance");
}
int decode_fill_i64(int64_t* p, int64_t v, int n, hipStream_t s) {
    ERGM_LAUNCH(fill_i64_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, p, v, n);
    return check_launch("decode_fill_i64");
}
// kernel launches of one ergm_attn_decode call with splits = 0
int attn_decode_launches(int B, int H, int max_len) { return decode_auto_splits(B, H, max_len) > 1 ? 2 : 1; }

}  // namespace ergm

using namespace ergm;

extern "C" size_t ergm_attn_decode_workspace_size(int B, int H, int max_len) {
    if (B <= 0 || H <= 0 || max_len <= 0) return 0;
    return (size_t)B * H * decode_split_cap(max_len) * DEC_PART * sizeof(float);
}

extern "C" int ergm_attn_decode(const void* qkv, int ld_qkv, void* kcache, void* vcache, int64_t ld_seq, int ld_row,
                                const int* lens, int B, int H, int max_len, int append, int splits, void* out, int ldo,
                                void* workspace, size_t ws_bytes, void* stream) {
    ERGM_CHECK_ARG(qkv && kcache && vcache && lens && out, "attn_decode: null argument");
    ERGM_CHECK_ARG(B > 0 && H > 0 && max_len > 0 && B <= 65535 && H <= 65535, "attn_decode: bad shape B %d H %d max_len %d",
                   B, H, max_len);
    ERGM_CHECK_ARG(append == 0 || append == 1, "attn_decode: append is 0 or 1");
    const int E = 64 * H;
    ERGM_CHECK_ARG(ld_qkv % 8 == 0 && ld_row % 8 == 0 && ld_seq % 8 == 0 && ldo % 8 == 0,
                   "attn_decode: strides must be multiples of 8 elements");
    ERGM_CHECK_ARG(ld_qkv >= (append ? 3 * E : E) && ld_row >= E && ldo >= E &&
                       ld_seq >= (int64_t)(max_len - 1) * ld_row + E,
                   "attn_decode: stride shorter than the rows it spans");
    ERGM_CHECK_ARG(aligned16(qkv) && aligned16(kcache) && aligned16(vcache) && aligned16(out),
                   "attn_decode: 16-byte alignment");
    ERGM_CHECK_ARG(splits >= 0 && splits <= DEC_MAX_SPLITS, "attn_decode: splits %d outside [0, %d]", splits,
                   DEC_MAX_SPLITS);
    if (splits == 0) splits = decode_auto_splits(B, H, max_len);
    ERGM_CHECK_ARG(splits == 1 || (workspace && ws_bytes >= (size_t)B * H * splits * DEC_PART * sizeof(float)),
                   "attn_decode: workspace too small for %d splits", splits);
    hipStream_t s = as_stream(stream);
    auto* q = reinterpret_cast<const __bf16*>(qkv);
    auto* o = reinterpret_cast<__bf16*>(out);
    ERGM_LAUNCH(attn_decode_kernel, dim3(splits, H, B), dim3(256), 0, s, q, ld_qkv, reinterpret_cast<__bf16*>(kcache),
                reinterpret_cast<__bf16*>(vcache), ld_seq, ld_row, lens, max_len, append, E, splits,
                reinterpret_cast<float*>(workspace), o, ldo);
    if (splits > 1)
        ERGM_LAUNCH(attn_decode_merge_kernel, dim3(H, B), dim3(64), 0, s, q, ld_qkv,
                    reinterpret_cast<const float*>(workspace), splits, append, E, o, ldo);
    return check_launch("attn_decode");
}

extern "C" int ergm_embed_rows(const int64_t* ids, const int64_t* tt, const int* pos, const float* wte, const float* wpe,
                               float* h, int B, int E, int V, int n_positions, void* stream) {
    ERGM_CHECK_ARG(ids && pos && wte && wpe && h, "embed_rows: null argument");
    ERGM_CHECK_ARG(B > 0 && E > 0 && E % 4 == 0 && V > 0 && n_positions > 0, "embed_rows: bad shape");
    ERGM_CHECK_ARG(aligned16(wte) && aligned16(wpe) && aligned16(h), "embed_rows: 16-byte alignment");
    ERGM_LAUNCH(embed_rows_kernel, dim3(B), dim3(256), 0, as_stream(stream), ids, tt, pos, wte, wpe, h, E, V, n_positions);
    return check_launch("embed_rows");
}

namespace {
// The one sampler launch, behind each entry point's own argument checks: sample_kernel<NPT, CTL> for the smallest
// NPT that holds the row.
template <bool CTL>
int sample_launch(const char* what, const float* logits, int ldl, int B, int V, float top_p, uint64_t seed, uint32_t step,
                  const uint32_t* row_ids, const uint32_t* row_steps, void* finished, int64_t eos_id, int64_t* tokens,
                  int* kept, float* kept_mass, const ergm_sample_ctl& ctl, float* logprob, void* stream) {
    hipStream_t s = as_stream(stream);
    auto* fin = reinterpret_cast<uint8_t*>(finished);
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    const int per = cdiv(V, TP_THREADS);
#define ERGM_SAMPLE(NPT)                                                                                              \
    ERGM_LAUNCH((sample_kernel<NPT, CTL>), dim3(B), dim3(TP_THREADS), 0, s, logits, ldl, V, top_p, lo, hi, step, row_ids, \
                row_steps, fin, eos_id, tokens, kept, kept_mass, logprob, ctl)
    if (per <= 4) ERGM_SAMPLE(4);
    else if (per <= 16) ERGM_SAMPLE(16);
    else ERGM_SAMPLE(52);
#undef ERGM_SAMPLE
    return check_launch(what);
}

// ergm_topp_sample and ergm_topp_sample_rows: nucleus sampling alone
int topp_launch(const char* what, const float* logits, int ldl, int B, int V, float top_p, uint64_t seed, uint32_t step,
                const uint32_t* row_ids, const uint32_t* row_steps, void* finished, int64_t eos_id, int64_t* tokens,
                int* kept, float* kept_mass, void* stream) {
    ERGM_CHECK_ARG(logits && tokens, "%s: null argument", what);
    ERGM_CHECK_ARG(B > 0 && V > 0 && ldl >= V, "%s: bad shape B %d V %d ldl %d", what, B, V, ldl);
    ERGM_CHECK_ARG(top_p == top_p, "%s: top_p is NaN", what);
    if (V > 52 * TP_THREADS) return fail(ERGM_EUNSUPPORTED, "%s: V %d > %d", what, V, 52 * TP_THREADS);
    return sample_launch<false>(what, logits, ldl, B, V, top_p, seed, step, row_ids, row_steps, finished, eos_id, tokens, kept,
                                kept_mass, ergm_sample_ctl{}, nullptr, stream);
}
}  // namespace

extern "C" int ergm_topp_sample(const float* logits, int ldl, int B, int V, float top_p, uint64_t seed, uint32_t step,
                                void* finished, int64_t eos_id, int64_t* tokens, int* kept, float* kept_mass,
                                void* stream) {
    return topp_launch("topp_sample", logits, ldl, B, V, top_p, seed, step, nullptr, nullptr, finished, eos_id, tokens, kept,
                       kept_mass, stream);
}

extern "C" int ergm_topp_sample_rows(const float* logits, int ldl, int B, int V, float top_p, uint64_t seed,
                                     const uint32_t* row_ids, const uint32_t* row_steps, void* finished, int64_t eos_id,
                                     int64_t* tokens, int* kept, float* kept_mass, void* stream) {
    ERGM_CHECK_ARG(row_ids && row_steps, "topp_sample_rows: null row_ids or row_steps");
    return topp_launch("topp_sample_rows", logits, ldl, B, V, top_p, seed, 0u, row_ids, row_steps, finished, eos_id, tokens,
                       kept, kept_mass, stream);
}

extern "C" int ergm_sample_rows(const float* logits, int ldl, int B, int V, float top_p, const ergm_sample_ctl* ctl,
                                uint64_t seed, const uint32_t* row_ids, const uint32_t* row_steps, void* finished,
                                int64_t eos_id, int64_t* tokens, int* kept, float* kept_mass, float* logprob, void* stream) {
    ERGM_CHECK_ARG(logits && tokens, "sample_rows: null logits or tokens");
    ERGM_CHECK_ARG(row_ids && row_steps, "sample_rows: null row_ids or row_steps");
    ERGM_CHECK_ARG(B > 0 && ldl >= V, "sample_rows: bad shape B %d V %d ldl %d", B, V, ldl);
    ERGM_CHECK_ARG(V > 0 && V <= 52 * TP_THREADS, "sample_rows: V %d outside [1, %d]", V, 52 * TP_THREADS);
    ERGM_CHECK_ARG(top_p == top_p, "sample_rows: top_p is NaN");
    ergm_sample_ctl c{};
    if (ctl) c = *ctl;
    ERGM_CHECK_ARG(!c.seen || c.ld_seen >= cdiv(V, 32), "sample_rows: ld_seen %d < the %d words of a row's bitmap", c.ld_seen,
                   cdiv(V, 32));
    return sample_launch<true>("sample_rows", logits, ldl, B, V, top_p, seed, 0u, row_ids, row_steps, finished, eos_id, tokens,
                               kept, kept_mass, c, logprob, stream);
}

extern "C" int ergm_sample_mark(const int64_t* ids, int total, const int* slot, const int* start, const int* len,
                                const int* reset, const int* min_new, int n_seq, int V, int n_slots, uint32_t* seen,
                                int ld_seen, const uint32_t* row_steps, uint32_t* min_step, void* stream) {
    ERGM_CHECK_ARG(ids && slot && start && len, "sample_mark: null argument");
    ERGM_CHECK_ARG(seen || min_step, "sample_mark: neither a bitmap nor min_step to write");
    ERGM_CHECK_ARG((min_step == nullptr) == (row_steps == nullptr), "sample_mark: min_step and row_steps go together");
    ERGM_CHECK_ARG(n_seq > 0 && n_seq <= 65535 && total > 0 && V > 0 && n_slots > 0,
                   "sample_mark: bad shape n_seq %d total %d V %d n_slots %d", n_seq, total, V, n_slots);
    ERGM_CHECK_ARG(!seen || ld_seen >= cdiv(V, 32), "sample_mark: ld_seen %d < the %d words of a row's bitmap", ld_seen,
                   cdiv(V, 32));
    ERGM_LAUNCH(sample_mark_kernel, dim3(n_seq), dim3(256), 0, as_stream(stream), ids, total, slot, start, len, reset, min_new,
                V, n_slots, seen, ld_seen, row_steps, min_step);
    return check_launch("sample_mark");
}

namespace {
int rows_to_slots_launch(const char* what, const void* src, int64_t ld_src, const int* start, const int* len, const int* slot,
                                  int n_seq, int total_rows, int max_rows, void* dst, int64_t ld_slot, int64_t ld_row,
                                  int row_bytes, int n_slots, int slot_rows, const int* dst_row0, void* stream) {
    ERGM_CHECK_ARG(src && start && len && slot && dst, "%s: null argument", what);
    ERGM_CHECK_ARG(n_seq > 0 && n_seq <= 65535 && total_rows > 0 && max_rows > 0 && max_rows <= total_rows && n_slots > 0 &&
                       slot_rows > 0,
                   "%s: bad shape n_seq %d total_rows %d max_rows %d n_slots %d slot_rows %d", what, n_seq, total_rows,
                   max_rows, n_slots, slot_rows);
    ERGM_CHECK_ARG(row_bytes > 0 && row_bytes % 16 == 0 && ld_src % 16 == 0 && ld_slot % 16 == 0 && ld_row % 16 == 0,
                   "%s: row_bytes and the strides (bytes) must be multiples of 16", what);
    ERGM_CHECK_ARG(ld_src >= row_bytes && ld_row >= row_bytes && ld_slot >= (int64_t)(slot_rows - 1) * ld_row + row_bytes,
                   "%s: stride shorter than the rows it spans", what);
    ERGM_CHECK_ARG(aligned16(src) && aligned16(dst), "%s: 16-byte alignment", what);
    ERGM_LAUNCH(rows_to_slots_kernel, dim3(cdiv(std::min(max_rows, slot_rows), 4), n_seq), dim3(256), 0, as_stream(stream),
                reinterpret_cast<const char*>(src), ld_src, start, len, slot, total_rows, max_rows,
                reinterpret_cast<char*>(dst), ld_slot, ld_row, row_bytes, n_slots, slot_rows, dst_row0);
    return check_launch(what);
}
}  // namespace

extern "C" int ergm_rows_to_slots(const void* src, int64_t ld_src, const int* start, const int* len, const int* slot,
                                  int n_seq, int total_rows, int max_rows, void* dst, int64_t ld_slot, int64_t ld_row,
                                  int row_bytes, int n_slots, int slot_rows, void* stream) {
    return rows_to_slots_launch("rows_to_slots", src, ld_src, start, len, slot, n_seq, total_rows, max_rows, dst, ld_slot, ld_row,
                                row_bytes, n_slots, slot_rows, nullptr, stream);
}

extern "C" int ergm_rows_to_slots_at(const void* src, int64_t ld_src, const int* start, const int* len, const int* slot,
                                     const int* dst_row0, int n_seq, int total_rows, int max_rows, void* dst, int64_t ld_slot,
                                     int64_t ld_row, int row_bytes, int n_slots, int slot_rows, void* stream) {
    ERGM_CHECK_ARG(dst_row0, "rows_to_slots_at: null dst_row0");
    return rows_to_slots_launch("rows_to_slots_at", src, ld_src, start, len, slot, n_seq, total_rows, max_rows, dst, ld_slot,
                                ld_row, row_bytes, n_slots, slot_rows, dst_row0, stream);
}
