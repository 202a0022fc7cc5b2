// The session store's kernels (ergm_hip.h, "Session store"): the state of a cache slot packed into one blob in HBM and
// unpacked into any slot.  The layout of a blob is stated in ergm_hip.h; DESIGN.md §12.11 has the policy above it.
//
// The cache rows move as ergm_beam_gather moves them (beam.hip): a workgroup per (session, layer, 64-row chunk), a wave
// per cache row, 16 bytes per lane, the layer pointers in the kernel arguments.  Everything else of a slot (the header,
// the controls, the seen row, the rule values, the pool row, the history) is a few KB and goes through one state kernel,
// a workgroup per session.  A save and a load are the same walks with source and destination exchanged.  Every session
// of a call owns its slot and (on a save) its blob, so nothing here is read and written by two workgroups and the three
// launches need no order among themselves beyond the stream's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace ergm {

constexpr int SS_MAX_LAYERS = 48;  // cache pointers of one launch, in the kernel arguments
constexpr int SS_ROWS = 64;        // cache rows of one workgroup
constexpr int SS_HDR = 64;         // header bytes
constexpr int SS_THREADS = 256;
struct SsLayers {
    char* p[SS_MAX_LAYERS];
};

// byte offsets of a blob's sections (0: the section is absent) and its size
struct SsLayout {
    int64_t kv, xkv, ctl, seen, rule, bad, hist, bytes;
};
__host__ __device__ inline int64_t ss_up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
__host__ __device__ inline SsLayout ss_layout(int n_layer, int row_bytes, int n, int c, int ld_seen, int bad_cap, int flags) {
    SsLayout o{};
    o.kv = SS_HDR;
    o.xkv = o.kv + (int64_t)n_layer * n * row_bytes;
    int64_t p = o.xkv + (int64_t)n_layer * c * row_bytes;
    if (flags & ERGM_SESSION_CTL) {
        o.ctl = p, p += 32;
        o.seen = p, p += ss_up16(4 * (int64_t)ld_seen);
    }
    if (flags & ERGM_SESSION_RULES) {
        o.rule = p, p += 16;
        o.bad = p, p += ss_up16(4 * (int64_t)bad_cap);
        o.hist = p, p += ss_up16(4 * (int64_t)n);
    }
    o.bytes = p;
    return o;
}

// the device's view of ergm_session_state
struct SsDev {
    int* lens;
    int* cap_lens;
    int* stop_lens;
    uint8_t* finished;
    uint32_t* row_ids;
    uint32_t* row_steps;
    uint32_t* ctl[4];  // top_p, temperature, rep_penalty (f32 bits), top_k
    uint32_t* min_step;
    uint32_t* seen;
    int ld_seen;
    int32_t* hist;
    int ld_hist;
    int* start;
    int* ngram;
    int32_t* bad;
    int ld_bad;
    int n_layer, row_bytes, max_batch, max_len, cap_max;
    int flags;  // the sections the state has
};
// the sizes every kernel checks the device meta against
struct SsDims {
    int n_layer, row_bytes, max_batch, max_len, cap_max, ld_seen, ld_bad, flags;
};
__host__ __device__ inline SsDims ss_dims(const SsDev& d) {
    return SsDims{d.n_layer, d.row_bytes, d.max_batch, d.max_len, d.cap_max, d.ld_seen, d.ld_bad, d.flags};
}

// Session b of the device meta: every value is checked or clamped here, before it forms an address: the slot against
// max_batch, the row counts to [0, max_len] / [0, cap_max], the flags masked by the state's sections, and the size of
// the blob these give against the size the meta states.  slot < 0: the session is skipped.
struct SsSess {
    int slot, n, c, flags;
    char* blob;
};
__device__ __forceinline__ SsSess ss_session(const int64_t* __restrict__ meta, int n_seq, int b, const SsDims& d) {
    SsSess s;
    const int64_t slot = meta[b];
    const int64_t n = meta[(int64_t)n_seq + b], c = meta[2 * (int64_t)n_seq + b];
    s.blob = reinterpret_cast<char*>(meta[3 * (int64_t)n_seq + b]);
    s.flags = (int)meta[4 * (int64_t)n_seq + b] & d.flags;
    const int64_t blob_bytes = meta[5 * (int64_t)n_seq + b];
    s.n = (int)max((int64_t)0, min(n, (int64_t)d.max_len));
    s.c = (int)max((int64_t)0, min(c, (int64_t)d.cap_max));
    const bool fits = ss_layout(d.n_layer, d.row_bytes, s.n, s.c, d.ld_seen, d.ld_bad, s.flags).bytes <= blob_bytes;
    s.slot = (slot >= 0 && slot < d.max_batch && s.blob != nullptr && fits) ? (int)slot : -1;
    return s;
}

// Workgroup (b, layer, chunk): rows [chunk·64, chunk·64 + 64) below the session's row count of layer l0 + layer, between
// the slot and the blob.  `cap`: the caption section (row count c, limit cap_max), else the self-attention one.
template <bool SAVE>
__global__ __launch_bounds__(SS_THREADS) void session_copy_kernel(SsLayers layers, int l0, SsDims dims, int64_t ld_seq,
                                                                  int64_t ld_row, const int64_t* __restrict__ meta, int n_seq,
                                                                  int cap) {
    const SsSess s = ss_session(meta, n_seq, blockIdx.x, dims);
    if (s.slot < 0) return;  // uniform over the workgroup
    const int rows = cap ? s.c : s.n;
    const int row_bytes = dims.row_bytes;
    const int64_t sec = SS_HDR + (cap ? (int64_t)dims.n_layer * s.n * row_bytes : 0) +
                        (int64_t)(l0 + (int)blockIdx.y) * rows * row_bytes;
    const int lane = threadIdx.x & 63;
    const int i1 = min(rows, (int)(blockIdx.z + 1) * SS_ROWS);
    char* slot_base = layers.p[blockIdx.y] + (int64_t)s.slot * ld_seq;
    char* blob_base = s.blob + sec;
    for (int i = blockIdx.z * SS_ROWS + (threadIdx.x >> 6); i < i1; i += SS_THREADS / 64) {
        char* in_slot = slot_base + (int64_t)i * ld_row;
        char* in_blob = blob_base + (int64_t)i * row_bytes;
        const char* src = SAVE ? in_slot : in_blob;
        char* dst = SAVE ? in_blob : in_slot;
        for (int k = lane * 16; k < row_bytes; k += 64 * 16)
            *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
    }
}

// words [0, n) of src to dst and zeros up to the next 16-byte boundary; the whole workgroup
__device__ __forceinline__ void ss_pack_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int n) {
    const int n4 = (n + 3) & ~3;
    for (int j = threadIdx.x; j < n4; j += SS_THREADS) dst[j] = j < n ? src[j] : 0u;
}

// Workgroup b: everything of session b but the cache rows, into its blob; then the slot goes idle.  Each value is read
// before the same thread overwrites it, and no thread reads what another writes.
__global__ __launch_bounds__(SS_THREADS) void session_save_state_kernel(SsDev st, const int64_t* __restrict__ meta, int n_seq) {
    const SsSess s = ss_session(meta, n_seq, blockIdx.x, ss_dims(st));
    if (s.slot < 0) return;
    const int t = threadIdx.x;
    const SsLayout lay = ss_layout(st.n_layer, st.row_bytes, s.n, s.c, st.ld_seen, st.ld_bad, s.flags);
    if (t < 16) {
        uint32_t w = 0;
        switch (t) {
            case 0: w = ERGM_SESSION_MAGIC; break;
            case 1: w = 1; break;
            case 2: w = (uint32_t)s.flags; break;
            case 3: w = (uint32_t)st.n_layer; break;
            case 4: w = (uint32_t)st.row_bytes; break;
            case 5: w = (uint32_t)s.n; break;
            case 6: w = (uint32_t)s.c; break;
            case 7: w = st.row_ids[s.slot]; break;
            case 8: w = st.row_steps[s.slot]; break;
            case 9: w = (s.flags & ERGM_SESSION_CTL) ? (uint32_t)st.ld_seen : 0u; break;
            case 10: w = (s.flags & ERGM_SESSION_RULES) ? (uint32_t)st.ld_bad : 0u; break;
            case 12: w = (uint32_t)lay.bytes; break;
            case 13: w = (uint32_t)((uint64_t)lay.bytes >> 32); break;
            default: break;
        }
        reinterpret_cast<uint32_t*>(s.blob)[t] = w;
    }
    if (s.flags & ERGM_SESSION_CTL) {
        if (t < 8) {
            uint32_t w = 0;
            if (t < 4) w = st.ctl[t][s.slot];
            else if (t == 4) w = st.min_step[s.slot];
            reinterpret_cast<uint32_t*>(s.blob + lay.ctl)[t] = w;
        }
        ss_pack_words(reinterpret_cast<uint32_t*>(s.blob + lay.seen), st.seen + (int64_t)s.slot * st.ld_seen, st.ld_seen);
    }
    if (s.flags & ERGM_SESSION_RULES) {
        if (t < 4) {
            uint32_t w = 0;
            if (t == 0) w = (uint32_t)st.start[s.slot], st.start[s.slot] = 0;
            if (t == 1) w = (uint32_t)st.ngram[s.slot], st.ngram[s.slot] = 0;
            reinterpret_cast<uint32_t*>(s.blob + lay.rule)[t] = w;
        }
        int32_t* pool = st.bad + (int64_t)s.slot * st.ld_bad;
        uint32_t* out = reinterpret_cast<uint32_t*>(s.blob + lay.bad);
        const int n4 = (st.ld_bad + 3) & ~3;
        for (int j = t; j < n4; j += SS_THREADS) {
            out[j] = j < st.ld_bad ? (uint32_t)pool[j] : 0u;
            if (j < st.ld_bad) pool[j] = 0;  // the next tenant inherits no rule
        }
        ss_pack_words(reinterpret_cast<uint32_t*>(s.blob + lay.hist),
                      reinterpret_cast<const uint32_t*>(st.hist + (int64_t)s.slot * st.ld_hist), s.n);
    }
    if (t == 0) {
        st.finished[s.slot] = 1;
        st.lens[s.slot] = 0;
        st.cap_lens[s.slot] = 0;
    }
}

// Workgroup b: everything of session b but the cache rows, from its blob into the slot, which is left parked.  The
// blob supplies values only; the row counts and the sections come from the (clamped, masked) meta.
__global__ __launch_bounds__(SS_THREADS) void session_load_state_kernel(SsDev st, const int64_t* __restrict__ meta, int n_seq,
                                                                        const uint32_t* __restrict__ row_ids) {
    const SsSess s = ss_session(meta, n_seq, blockIdx.x, ss_dims(st));
    if (s.slot < 0) return;
    const int t = threadIdx.x;
    const SsLayout lay = ss_layout(st.n_layer, st.row_bytes, s.n, s.c, st.ld_seen, st.ld_bad, s.flags);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(s.blob);
    if (t == 0) {
        st.lens[s.slot] = s.n;
        st.cap_lens[s.slot] = s.c;
        st.stop_lens[s.slot] = s.n;
        st.finished[s.slot] = 1;
        st.row_ids[s.slot] = row_ids ? row_ids[blockIdx.x] : hdr[7];
        st.row_steps[s.slot] = hdr[8];
    }
    if (s.flags & ERGM_SESSION_CTL) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s.blob + lay.ctl);
        if (t < 4) st.ctl[t][s.slot] = w[t];
        if (t == 4) st.min_step[s.slot] = w[4];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(s.blob + lay.seen);
        uint32_t* row = st.seen + (int64_t)s.slot * st.ld_seen;
        for (int j = t; j < st.ld_seen; j += SS_THREADS) row[j] = src[j];
    }
    if (st.flags & ERGM_SESSION_RULES) {
        const bool ruled = (s.flags & ERGM_SESSION_RULES) != 0;  // uniform: a blob without rules turns the slot's off
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s.blob + lay.rule);
        if (t == 0) st.start[s.slot] = ruled ? (int)w[0] : 0;
        if (t == 1) st.ngram[s.slot] = ruled ? (int)w[1] : 0;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(s.blob + lay.bad);
        int32_t* pool = st.bad + (int64_t)s.slot * st.ld_bad;
        for (int j = t; j < st.ld_bad; j += SS_THREADS) pool[j] = ruled ? (int32_t)src[j] : 0;
        if (ruled) {
            const uint32_t* h = reinterpret_cast<const uint32_t*>(s.blob + lay.hist);
            int32_t* row = st.hist + (int64_t)s.slot * st.ld_hist;
            for (int j = t; j < s.n; j += SS_THREADS) row[j] = (int32_t)h[j];
        }
    }
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The host checks of `state` that a save and a load share; fills the device view.
static int session_state_check(const ergm_session_state* st, const char* what, SsDev* dev) {
    ERGM_CHECK_ARG(st, "%s: null state", what);
    ERGM_CHECK_ARG(st->kv && st->xkv && st->lens && st->cap_lens && st->stop_lens && st->finished && st->row_ids && st->row_steps,
                   "%s: null pointer in the state", what);
    ERGM_CHECK_ARG(aligned4(st->lens) && aligned4(st->cap_lens) && aligned4(st->stop_lens) && aligned4(st->row_ids) &&
                       aligned4(st->row_steps),
                   "%s: a slot-state array is not 4-byte aligned", what);
    ERGM_CHECK_ARG(st->n_layer >= 1 && st->max_batch >= 1 && st->max_batch <= 65536 && st->max_len >= 1 && st->cap_max >= 1,
                   "%s: bad shape n_layer %d max_batch %d (<= 65536) max_len %d cap_max %d", what, st->n_layer, st->max_batch,
                   st->max_len, st->cap_max);
    ERGM_CHECK_ARG(st->row_bytes > 0 && st->row_bytes % 16 == 0 && st->kv_ld_seq % 16 == 0 && st->kv_ld_row % 16 == 0 &&
                       st->xkv_ld_seq % 16 == 0 && st->xkv_ld_row % 16 == 0,
                   "%s: row_bytes and the strides (bytes) must be multiples of 16", what);
    ERGM_CHECK_ARG(st->kv_ld_row >= st->row_bytes && st->kv_ld_seq >= (int64_t)(st->max_len - 1) * st->kv_ld_row + st->row_bytes &&
                       st->xkv_ld_row >= st->row_bytes &&
                       st->xkv_ld_seq >= (int64_t)(st->cap_max - 1) * st->xkv_ld_row + st->row_bytes,
                   "%s: stride shorter than the rows it spans", what);
    ERGM_CHECK_ARG(cdiv(st->max_len, SS_ROWS) <= 65535 && cdiv(st->cap_max, SS_ROWS) <= 65535, "%s: max_len or cap_max too large",
                   what);
    for (int l = 0; l < st->n_layer; ++l)
        ERGM_CHECK_ARG(st->kv[l] && aligned16(st->kv[l]) && st->xkv[l] && aligned16(st->xkv[l]),
                       "%s: layer %d cache pointer null or not 16-byte aligned", what, l);
    SsDev d{};
    d.lens = st->lens, d.cap_lens = st->cap_lens, d.stop_lens = st->stop_lens, d.finished = st->finished;
    d.row_ids = st->row_ids, d.row_steps = st->row_steps;
    d.n_layer = st->n_layer, d.row_bytes = st->row_bytes, d.max_batch = st->max_batch, d.max_len = st->max_len;
    d.cap_max = st->cap_max;
    if (const ergm_sample_ctl* c = st->ctl) {
        ERGM_CHECK_ARG(c->top_p && c->temperature && c->rep_penalty && c->top_k && c->min_step && c->seen && c->ld_seen >= 1,
                       "%s: the controls of a session state need every array and ld_seen >= 1 (null pointer)", what);
        ERGM_CHECK_ARG(aligned4(c->top_p) && aligned4(c->temperature) && aligned4(c->rep_penalty) && aligned4(c->top_k) &&
                           aligned4(c->min_step) && aligned4(c->seen),
                       "%s: a control array is not 4-byte aligned", what);
        d.ctl[0] = reinterpret_cast<uint32_t*>(const_cast<float*>(c->top_p));
        d.ctl[1] = reinterpret_cast<uint32_t*>(const_cast<float*>(c->temperature));
        d.ctl[2] = reinterpret_cast<uint32_t*>(const_cast<float*>(c->rep_penalty));
        d.ctl[3] = reinterpret_cast<uint32_t*>(const_cast<int*>(c->top_k));
        d.min_step = const_cast<uint32_t*>(c->min_step);
        d.seen = c->seen, d.ld_seen = c->ld_seen;
        d.flags |= ERGM_SESSION_CTL;
    }
    if (const ergm_logit_rules* r = st->rules) {
        ERGM_CHECK_ARG(r->hist && r->start && r->ngram && r->bad && r->ld_bad >= 1,
                       "%s: the rules of a session state need every array and ld_bad >= 1 (null pointer)", what);
        ERGM_CHECK_ARG(r->ld_hist >= st->max_len, "%s: ld_hist %d < max_len %d", what, r->ld_hist, st->max_len);
        ERGM_CHECK_ARG(aligned4(r->hist) && aligned4(r->start) && aligned4(r->ngram) && aligned4(r->bad),
                       "%s: a rule array is not 4-byte aligned", what);
        d.hist = r->hist, d.ld_hist = r->ld_hist;
        d.start = const_cast<int*>(r->start), d.ngram = const_cast<int*>(r->ngram);
        d.bad = const_cast<int32_t*>(r->bad), d.ld_bad = r->ld_bad;
        d.flags |= ERGM_SESSION_RULES;
    }
    *dev = d;
    return ERGM_OK;
}

// The host checks of one session (entry b of the call): its row counts, its flags and its blob.  Keeps the largest row
// counts for the grids.
static int session_entry_check(const ergm_session_state* st, const SsDev& d, const char* what, int b, int rows, int cap_rows,
                               int flags, const void* blob, size_t blob_bytes, int* max_rows, int* max_cap) {
    ERGM_CHECK_ARG(rows >= 1 && rows <= st->max_len, "%s: rows %d (entry %d) outside [1, max_len %d]", what, rows, b, st->max_len);
    ERGM_CHECK_ARG(cap_rows >= 1 && cap_rows <= st->cap_max, "%s: cap_rows %d (entry %d) outside [1, cap_max %d]", what, cap_rows,
                   b, st->cap_max);
    ERGM_CHECK_ARG((flags & ~d.flags) == 0 && (flags & ERGM_SESSION_CTL) == (d.flags & ERGM_SESSION_CTL),
                   "%s: flags %d (entry %d) disagree with the state's sections %d", what, flags, b, d.flags);
    ERGM_CHECK_ARG(blob && aligned16(blob), "%s: blob %d null or not 16-byte aligned", what, b);
    const size_t need = ergm_session_bytes(st->n_layer, st->row_bytes, rows, cap_rows, d.ld_seen, d.ld_bad, flags);
    ERGM_CHECK_ARG(need > 0 && blob_bytes >= need, "%s: blob %d has %zu bytes, the session needs %zu", what, b, blob_bytes, need);
    *max_rows = std::max(*max_rows, rows);
    *max_cap = std::max(*max_cap, cap_rows);
    return ERGM_OK;
}

static int session_slots_check(const ergm_session_state* st, const char* what, int n_seq, const int* slots) {
    ERGM_CHECK_ARG(n_seq >= 1 && n_seq <= st->max_batch, "%s: n_seq %d outside [1, max_batch %d]", what, n_seq, st->max_batch);
    std::vector<unsigned char> seen((size_t)st->max_batch, 0);
    for (int b = 0; b < n_seq; ++b) {
        const int s = slots[b];
        ERGM_CHECK_ARG(s >= 0 && s < st->max_batch, "%s: slot %d (entry %d) outside [0, %d)", what, s, b, st->max_batch);
        ERGM_CHECK_ARG(!seen[s], "%s: slot %d named twice", what, s);
        seen[s] = 1;
    }
    return ERGM_OK;
}

template <bool SAVE>
static void session_copies(const ergm_session_state* st, const SsDev& d, const int64_t* meta, int n_seq, int max_rows,
                           int max_cap, hipStream_t s) {
    for (int cap = 0; cap < 2; ++cap) {
        void* const* caches = cap ? st->xkv : st->kv;
        const int chunks = cdiv(cap ? max_cap : max_rows, SS_ROWS);
        for (int l0 = 0; l0 < st->n_layer; l0 += SS_MAX_LAYERS) {
            const int nl = std::min(SS_MAX_LAYERS, st->n_layer - l0);
            SsLayers L{};
            for (int l = 0; l < nl; ++l) L.p[l] = reinterpret_cast<char*>(caches[l0 + l]);
            ERGM_LAUNCH((session_copy_kernel<SAVE>), dim3(n_seq, nl, chunks), dim3(SS_THREADS), 0, s, L, l0, ss_dims(d),
                        cap ? st->xkv_ld_seq : st->kv_ld_seq, cap ? st->xkv_ld_row : st->kv_ld_row, meta, n_seq, cap);
        }
    }
}

}  // namespace ergm

using namespace ergm;

extern "C" size_t ergm_session_bytes(int n_layer, int row_bytes, int rows, int cap_rows, int ld_seen, int bad_cap, int flags) {
    if (n_layer < 1 || row_bytes <= 0 || row_bytes % 16 || rows < 1 || cap_rows < 1) return 0;
    if (flags & ~(ERGM_SESSION_CTL | ERGM_SESSION_RULES)) return 0;
    if ((flags & ERGM_SESSION_CTL) && ld_seen < 1) return 0;
    if ((flags & ERGM_SESSION_RULES) && bad_cap < 1) return 0;
    return (size_t)ss_layout(n_layer, row_bytes, rows, cap_rows, ld_seen, bad_cap, flags).bytes;
}

extern "C" int ergm_session_header(int n_layer, int row_bytes, int rows, int cap_rows, int ld_seen, int bad_cap, int flags,
                                   ergm_session_hdr* out) {
    ERGM_CHECK_ARG(out, "session_header: null argument");
    const size_t bytes = ergm_session_bytes(n_layer, row_bytes, rows, cap_rows, ld_seen, bad_cap, flags);
    ERGM_CHECK_ARG(bytes > 0, "session_header: bad shape n_layer %d row_bytes %d rows %d cap_rows %d ld_seen %d bad_cap %d flags %d",
                   n_layer, row_bytes, rows, cap_rows, ld_seen, bad_cap, flags);
    static_assert(sizeof(ergm_session_hdr) == SS_HDR, "the header is 64 bytes");
    ergm_session_hdr h{};
    h.magic = ERGM_SESSION_MAGIC, h.version = 1, h.flags = (uint32_t)flags;
    h.n_layer = n_layer, h.row_bytes = row_bytes, h.rows = rows, h.cap_rows = cap_rows;
    h.ld_seen = (flags & ERGM_SESSION_CTL) ? ld_seen : 0;
    h.bad_cap = (flags & ERGM_SESSION_RULES) ? bad_cap : 0;
    h.bytes = bytes;
    *out = h;
    return ERGM_OK;
}

extern "C" int ergm_session_launches(int n_layer) {
    if (n_layer < 1) return fail(ERGM_EINVAL, "session_launches: n_layer %d", n_layer);
    return 2 * cdiv(n_layer, SS_MAX_LAYERS) + 1;
}

extern "C" int ergm_slots_save(const ergm_session_state* state, int n_seq, const int* slots, const int* rows, const int* cap_rows,
                               const int* flags, void* const* blobs, const size_t* blob_bytes, const int64_t* meta_dev,
                               void* stream) {
    SsDev d;
    ERGM_TRY(session_state_check(state, "slots_save", &d));
    ERGM_CHECK_ARG(slots && rows && cap_rows && flags && blobs && blob_bytes && meta_dev, "slots_save: null argument");
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(meta_dev) & 7) == 0, "slots_save: meta not 8-byte aligned");
    ERGM_TRY(session_slots_check(state, "slots_save", n_seq, slots));
    int max_rows = 0, max_cap = 0;
    for (int b = 0; b < n_seq; ++b)
        ERGM_TRY(session_entry_check(state, d, "slots_save", b, rows[b], cap_rows[b], flags[b], blobs[b], blob_bytes[b], &max_rows,
                                     &max_cap));
    std::vector<const void*> sorted(blobs, blobs + n_seq);
    std::sort(sorted.begin(), sorted.end());
    ERGM_CHECK_ARG(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "slots_save: a blob is named twice");
    hipStream_t s = as_stream(stream);
    session_copies<true>(state, d, meta_dev, n_seq, max_rows, max_cap, s);
    ERGM_LAUNCH(session_save_state_kernel, dim3(n_seq), dim3(SS_THREADS), 0, s, d, meta_dev, n_seq);
    return check_launch("slots_save");
}

extern "C" int ergm_slots_load(const ergm_session_state* state, int n_seq, const int* slots, const ergm_session_hdr* hdrs,
                               void* const* blobs, const size_t* blob_bytes, const uint32_t* row_ids, const int64_t* meta_dev,
                               void* stream) {
    SsDev d;
    ERGM_TRY(session_state_check(state, "slots_load", &d));
    ERGM_CHECK_ARG(slots && hdrs && blobs && blob_bytes && meta_dev, "slots_load: null argument");
    ERGM_CHECK_ARG((reinterpret_cast<uintptr_t>(meta_dev) & 7) == 0 && aligned4(row_ids),
                   "slots_load: meta not 8-byte or row_ids not 4-byte aligned");
    ERGM_TRY(session_slots_check(state, "slots_load", n_seq, slots));
    int max_rows = 0, max_cap = 0;
    for (int b = 0; b < n_seq; ++b) {
        const ergm_session_hdr& h = hdrs[b];
        ERGM_CHECK_ARG(h.magic == ERGM_SESSION_MAGIC && h.version == 1, "slots_load: header %d is no session header (magic %#x version %u)",
                       b, h.magic, h.version);
        ERGM_CHECK_ARG(h.n_layer == state->n_layer && h.row_bytes == state->row_bytes,
                       "slots_load: header %d disagrees with the state: n_layer %d row_bytes %d, the state has %d and %d", b,
                       h.n_layer, h.row_bytes, state->n_layer, state->row_bytes);
        const int fl = (int)h.flags;
        ERGM_CHECK_ARG((h.flags & ~(uint32_t)d.flags) == 0 && (fl & ERGM_SESSION_CTL) == (d.flags & ERGM_SESSION_CTL),
                       "slots_load: header %d disagrees with the state: flags %d, the state's sections are %d", b, fl, d.flags);
        ERGM_CHECK_ARG(h.ld_seen == ((fl & ERGM_SESSION_CTL) ? d.ld_seen : 0) && h.bad_cap == ((fl & ERGM_SESSION_RULES) ? d.ld_bad : 0),
                       "slots_load: header %d disagrees with the state: ld_seen %d bad_cap %d", b, h.ld_seen, h.bad_cap);
        ERGM_TRY(session_entry_check(state, d, "slots_load", b, h.rows, h.cap_rows, fl, blobs[b], blob_bytes[b], &max_rows,
                                     &max_cap));
        ERGM_CHECK_ARG(h.bytes == ergm_session_bytes(h.n_layer, h.row_bytes, h.rows, h.cap_rows, d.ld_seen, d.ld_bad, fl),
                       "slots_load: header %d states %llu bytes, its sizes give another count", b, (unsigned long long)h.bytes);
    }
    hipStream_t s = as_stream(stream);
    session_copies<false>(state, d, meta_dev, n_seq, max_rows, max_cap, s);
    ERGM_LAUNCH(session_load_state_kernel, dim3(n_seq), dim3(SS_THREADS), 0, s, d, meta_dev, n_seq, row_ids);
    return check_launch("slots_load");
}
