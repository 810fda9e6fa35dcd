// sk_hmmstream.hip -- HMM sessions: the signal HMM's Viterbi pass continued as a read's samples arrive (gfx950).
//
// The definition (include/squigglekit_hip.h, "HMM sessions"; tests/hmmstream_ref.py restates it on top of
// tests/hmm_ref.py).  A session has one checked sk_hmm_model and `nslots` slots; a slot holds a read in progress: the six
// scores v, the six enter tuples E, n (the samples since its reset), the pushes of length > 0 and its calibration pair.
// Viterbi never looks ahead and the one-shot kernel already carries exactly v and E from sample to sample, so a push
// just goes on where the last one stopped: sample t = n, n + 1, .. of the slot takes the `linit` rule for t == 0 and the
// recurrence otherwise, and the record after the push is sk_hmm_viterbi_*'s of everything the slot has had, bit for bit.
//
// k_hmms_push<FEED, FILT>  one lane per named entry, 64 entries per wavefront (one wavefront per workgroup): k_hmm_viterbi's
//     mapping, its LDS tiles and its text (sk_hmm_dev.h: hmm_load_tile, hmm_emit, hmm_first, hmm_step).  A lane loads its
//     slot's 224 bytes, walks the `len` samples of its chunk and stores the state back; then it writes the 96-byte
//     record.  The sample index is the lane's own here -- t = n0 + position in the chunk -- so the t == 0 case is a
//     per-lane branch, no longer a scalar one: a wavefront that holds a fresh slot next to continuing ones runs both
//     bodies for the first sample of the chunk and one of them from then on.  A lane idles when its entry is a peek
//     (len 0), names a slot outside the session (device form) or a slot that is full; the wavefront runs for its longest
//     chunk.  -inf transitions and components are skipped through tmask / cmask as in the one-shot kernel (exact for the
//     reason stated in sk_hmm.hip).  Samples that would take a slot past 0x7fffff00 are ignored and the slot is counted in
//     the context's guard counter (the host form refuses such a push before anything runs).
// k_hmms_reset        the named slots (or all) back to n = 0 with a calibration pair ({0.0, 1.0}: none).
//
// A FILTERED session (SK_HMMS_FILTER; tests/hmmfilter_ref.py) also carries the forward recursion of the
// posteriors (sk_hmm_post.hip): alpha[6] per slot, 48 bytes in an array of their own beside the 224-byte
// slots, -inf after a reset.  k_hmms_push<FEED, true> loads, steps and stores it with the text k_hmm_fwd runs
// (sk_hmm_dev.h: post_fwd_step), on the x the Viterbi step of the same sample sees, so the filter after n samples is the
// one-shot record's loglik and final_post of the same prefix (beta(n - 1) = 0), bit for bit.  The forward steps of a
// tile run as a second loop over the LDS tile, behind the Viterbi steps of that tile.  The bits cannot differ from a
// fused loop's, so the resource lines chose: 154 / 144 VGPRs this way, 157 / 145 with the forward step inside the Viterbi
// loop (both without spill or scratch).  All the second loop repeats is the tile's LDS read and the emission -- a dozen
// operations against the 36 sk_exp and 6 sk_log of a step -- and the Viterbi loop's code stays the plain kernel's.
// k_hmms_push<FEED, false> is the plain session's kernel, untouched by the flag.
// k_hmms_filter       one lane per named entry: n and alpha -> sk_hmms_filt (loglik = lse_j alpha_j, post[j] =
//     sk_exp((alpha_j + 0.0) - L)); it changes nothing.
//
// Distinct slots per push are what makes the lanes independent: the host form checks it, the device form has it as the
// caller's contract.
#include "sk_hmm_dev.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int32_t HMMS_CAP = SK_HMMS_CAP;     // samples a slot can hold: the one-shot call's cap (sk_common.h: a gated
                                              // live session refuses by the same number)

struct hmms_slot {               // 224 bytes
    double  v[HS];
    int32_t E[HS][HS];
    int32_t n, pushes;
    double  offset, unit;        // {0.0, 1.0}: none
    int32_t flags, pad;
};

struct hmms_alpha { double a[HS]; };   // 48 bytes: a filtered session's forward variables, -inf at n == 0

static_assert(sizeof(hmms_slot) == 224, "hmms_slot is 224 bytes");
static_assert(sizeof(hmms_alpha) == 48, "hmms_alpha is 48 bytes");
static_assert(sizeof(sk_hmms_filt) == 64, "sk_hmms_filt is 64 bytes (include/squigglekit_hip.h)");
static_assert(sizeof(sk_hmms_rec) == 96, "sk_hmms_rec is 96 bytes (include/squigglekit_hip.h)");

struct hmms_kargs {
    hmms_slot     *state;        // [nslots]
    hmms_alpha    *alpha;        // [nslots] of a filtered session (FILT), else nullptr
    int32_t        nslots;
    int32_t        m;
    const int32_t *slots;        // [m]
    const void    *sig;          // int16 rows [m][stride], or float64 values
    int64_t        stride;
    const int32_t *len;          // int16 rows: [m]
    const int64_t *off;          // float64 values: [m + 1], chunk k = sig[off[k] .. off[k + 1])
    int32_t        vec;          // int16 rows are 16-byte aligned (base and stride)
    sk_hmms_rec   *out;          // [m]
    unsigned long long *guard;   // [1]
    hmm_kmodel     mdl;
};

__device__ __forceinline__ void hmms_first(hmms_slot &st, double offset, double unit)
{
    const double ninf = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < HS; j++) {
        st.v[j] = ninf;
#pragma unroll
        for (int q = 0; q < HS; q++) st.E[j][q] = -1;
    }
    st.n = 0; st.pushes = 0; st.offset = offset; st.unit = unit; st.flags = 0; st.pad = 0;
}

template <int FEED, bool FILT>
__global__ __launch_bounds__(64)
void k_hmms_push(const hmms_kargs a)
{
    typedef typename hmm_feed<FEED>::T T;
    constexpr int TILE = hmm_feed<FEED>::TILE, PITCH = hmm_feed<FEED>::PITCH;
    __shared__ __attribute__((aligned(16))) uint32_t tile[64 * PITCH];
    __shared__ int32_t nrow[64];
    const int lane = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    const int64_t k = k0 + lane;

    int32_t slot = k < a.m ? a.slots[k] : -1;
    if (slot < 0 || slot >= a.nslots) slot = -1;
    hmms_slot st;
    if (slot >= 0) st = a.state[slot];
    else hmms_first(st, 0.0, 1.0);
    double al[FILT ? HS : 1];
    if constexpr (FILT) {
#pragma unroll
        for (int j = 0; j < HS; j++) al[j] = slot >= 0 ? a.alpha[slot].a[j] : -__builtin_inf();
    }
    int64_t l = 0;
    if (slot >= 0) {
        if (FEED == SK_FEED_I16) {
            l = a.len[k];
            if (l > a.stride) l = a.stride;
        } else {
            l = a.off[k + 1] - a.off[k];
        }
        if (l < 0) l = 0;
        if (l > (int64_t)(HMMS_CAP - st.n)) {                   // (n <= HMMS_CAP always: nmax + TILE - 1 stays inside int32)
            l = HMMS_CAP - st.n;
            atomicAdd(a.guard, 1ull);
        }
    }
    const int32_t len = (int32_t)l, n0 = st.n;
    nrow[lane] = len;
    int32_t nmax = len;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    __syncthreads();

    const int S = a.mdl.S;
    const T *xrow = (const T *)tile + (size_t)lane * (PITCH * 4 / sizeof(T));
    const int ntiles = (nmax + TILE - 1) / TILE;
    for (int kk = 0; kk < ntiles; kk++) {
        hmm_load_tile<FEED>(a.sig, a.stride, a.off, a.vec, tile, nrow, k0, kk, lane);
        __syncthreads();
        const int32_t p0 = kk * TILE;
        const int32_t pend = nmax - p0 < TILE ? nmax - p0 : TILE;   // wave uniform
        for (int jj = 0; jj < pend; jj++) {
            const int32_t pos = p0 + jj;                        // wave uniform: the position in the chunk
            if (pos < len) {
                double x = (double)xrow[jj];
                if (FEED == SK_FEED_I16) x = sk_raw_to_pa(x, st.offset, st.unit);
                const int32_t t = n0 + pos;                     // the lane's own: the position in the read
                if (t == 0) hmm_first(a.mdl, S, x, st.v, st.E);
                else        hmm_step(a.mdl, S, x, t, st.v, st.E);
            }
        }
        if constexpr (FILT) {                                   // the forward steps of the same samples, same x
            for (int jj = 0; jj < pend; jj++) {
                const int32_t pos = p0 + jj;
                if (pos < len) {
                    double x = (double)xrow[jj];
                    if (FEED == SK_FEED_I16) x = sk_raw_to_pa(x, st.offset, st.unit);
                    if (n0 + pos == 0) {
#pragma unroll
                        for (int j = 0; j < HS; j++)
                            if (j < S) al[j] = a.mdl.linit[j] + hmm_emit(a.mdl, j, x);
                    } else {
                        post_fwd_step(a.mdl, S, x, al);
                    }
                }
            }
        }
        __syncthreads();                                        // the tile is read before the next one lands
    }

    if (len > 0) {
        st.n = n0 + len;
        st.pushes += 1;
        a.state[slot] = st;
        if constexpr (FILT) {
            hmms_alpha o;
#pragma unroll
            for (int j = 0; j < HS; j++) o.a[j] = al[j];
            a.alpha[slot] = o;
        }
    }
    if (k >= a.m) return;
    sk_hmms_rec out;
    if (st.n == 0) {
        out.score = 0.0; out.final_state = -1;
#pragma unroll
        for (int q = 0; q < HS; q++) out.enter[q] = -1;
    } else {
        hmm_result(S, st.v, st.E, out.score, out.final_state, out.enter);
    }
    out.n_used = st.n;
#pragma unroll
    for (int j = 0; j < HS; j++) out.v[j] = st.v[j];
    out.pushes = st.pushes; out.flags = 0;
    a.out[k] = out;
}

__global__ void k_hmms_reset(hmms_slot *state, hmms_alpha *alpha, int32_t nslots, const int32_t *slots, int32_t m,
                             const double *cal2)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m) return;
    const int32_t s = slots ? slots[idx] : idx;
    if (s < 0 || s >= nslots) return;
    hmms_slot st;
    hmms_first(st, cal2 ? cal2[2 * idx] : 0.0, cal2 ? cal2[2 * idx + 1] : 1.0);
    state[s] = st;
    if (alpha) {
        hmms_alpha o;
#pragma unroll
        for (int j = 0; j < HS; j++) o.a[j] = -__builtin_inf();
        alpha[s] = o;
    }
}

// the filter of the named slots as they stand: L = lse_j alpha_j in rising j < S, post[j] = sk_exp((alpha_j + 0.0) - L) --
// k_hmm_fwd's L and k_hmm_bwd's gamma at the last sample, where beta is 0.0.  n == 0 and a slot outside the session: zeros.
__global__ void k_hmms_filter(const hmms_slot *state, const hmms_alpha *alpha, int32_t nslots, int32_t S, const int32_t *slots,
                              int32_t m, sk_hmms_filt *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m) return;
    const int32_t s = slots[idx];
    const bool in = s >= 0 && s < nslots;
    const int32_t n = in ? state[s].n : 0;
    const double ninf = -__builtin_inf();
    double al[HS];
#pragma unroll
    for (int j = 0; j < HS; j++) al[j] = (in && j < S) ? alpha[s].a[j] : ninf;
    sk_hmms_filt o;
    o.loglik = 0.0; o.n_used = n; o.flags = 0;
#pragma unroll
    for (int j = 0; j < HS; j++) o.post[j] = 0.0;
    if (n > 0) {
        const double Lr = post_lse(al, (1u << S) - 1u);
        const bool live = Lr != ninf;
        const double L = live ? Lr : 0.0;
        o.loglik = Lr;
        o.flags = live ? 0 : SK_HMM_POST_IMPOSSIBLE;
#pragma unroll
        for (int j = 0; j < HS; j++)
            if (j < S) { const double g = sk_exp((al[j] + 0.0) - L); o.post[j] = live ? g : 0.0; }
    }
    out[idx] = o;
}

struct hmms_session {
    int32_t nslots = 0;
    sk_hmm_model model;
    sk_buf state;                           // hmms_slot [nslots]
    sk_buf alpha;                           // hmms_alpha [nslots] of a filtered session (SK_HMMS_FILTER), else empty
    bool filter = false;
    std::vector<int32_t> n;                 // per slot, as the host forms know them: samples since the reset
    bool mirror_stale = false;              // a device-form push has moved slots the host did not see
    sk_buf rows, args, out;                 // the host forms' staging: samples; slots, lengths / offsets, pairs; records
};

void free_buf(sk_buf *b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

void destroy(hmms_session *z)
{
    sk_buf *bufs[] = {&z->state, &z->alpha, &z->rows, &z->args, &z->out};
    for (sk_buf *b : bufs) free_buf(b);
    delete z;
}

int check_handle(int32_t handle)
{
    if (handle < 0 || handle >= SK_HMMS_MAX_SESSIONS)
        return sk_fail(SK_ERR_INVALID, "HMM session handle %d is outside [0, %d)", handle, SK_HMMS_MAX_SESSIONS);
    return SK_OK;
}

hmms_session *session_of(sk_ctx *c, int32_t handle)
{
    if (handle < 0 || handle >= SK_HMMS_MAX_SESSIONS || !c->hmms_sessions[handle]) {
        sk_fail(SK_ERR_INVALID, "unknown HMM session handle %d", handle);
        return nullptr;
    }
    return (hmms_session *)c->hmms_sessions[handle];
}

// host: the slot numbers against the ABI's limit, none twice (the later entry of a pair is named)
int check_slots_host(const int32_t *slots, int32_t m, bool twice_ok)
{
    for (int32_t i = 0; i < m; i++)
        if (slots[i] < 0 || slots[i] >= SK_HMMS_MAX_SLOTS)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, slots[i], SK_HMMS_MAX_SLOTS);
    if (twice_ok) return SK_OK;
    std::vector<int32_t> order((size_t)m);
    for (int32_t i = 0; i < m; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return slots[a] != slots[b] ? slots[a] < slots[b] : a < b; });
    int32_t twice = -1;
    for (int32_t k = 1; k < m; k++)
        if (slots[order[(size_t)k]] == slots[order[(size_t)k - 1]] && (twice < 0 || order[(size_t)k] < twice)) twice = order[(size_t)k];
    if (twice >= 0) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d appears twice in one call", twice, slots[twice]);
    return SK_OK;
}

// what the arguments of an int16 push decide (host: slots and len can be read here)
int check_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                   const sk_hmms_rec *out, bool host)
{
    if (int rc = check_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (stride < 0) return sk_fail(SK_ERR_INVALID, "stride < 0");
    if (m == 0) return SK_OK;
    if (!slots || !len) return sk_fail(SK_ERR_INVALID, "NULL slots/len");
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    if (stride > 0 && !rows) return sk_fail(SK_ERR_INVALID, "NULL rows");
    if (stride > 0x7fffffffll) return sk_fail(SK_ERR_INVALID, "stride = %lld above 2147483647", (long long)stride);
    if ((int64_t)m * (stride + 64) > ((int64_t)1 << 31))
        return sk_fail(SK_ERR_UNSUPPORTED, "HMM session push: %d rows of %lld samples in one call", m, (long long)stride);
    if (!host) return SK_OK;
    for (int32_t i = 0; i < m; i++)
        if (len[i] < 0 || len[i] > stride)
            return sk_fail(SK_ERR_INVALID, "entry %d: len = %d is outside [0, stride = %lld]", i, len[i], (long long)stride);
    return check_slots_host(slots, m, false);
}

// ... of a float64 push (host: slots and off can be read here)
int check_push_f64(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off,
                   const sk_hmms_rec *out, bool host)
{
    if (int rc = check_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m == 0) return SK_OK;
    if (!slots || !off) return sk_fail(SK_ERR_INVALID, "NULL slots/off");
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    if (!host) {
        if (!values) return sk_fail(SK_ERR_INVALID, "NULL values");
        return SK_OK;
    }
    for (int32_t i = 0; i < m; i++)
        if (off[i + 1] < off[i])
            return sk_fail(SK_ERR_INVALID, "entry %d: off decreases (%lld after %lld)", i, (long long)off[i + 1], (long long)off[i]);
    if (off[m] > off[0] && !values) return sk_fail(SK_ERR_INVALID, "NULL values");
    return check_slots_host(slots, m, false);
}

// the host's view of n after device-form pushes: read back from the slots
int refresh_mirror(sk_ctx *c, hmms_session *z)
{
    if (!z->mirror_stale) return SK_OK;
    std::vector<hmms_slot> st((size_t)z->nslots);
    SK_HIP(hipMemcpyAsync(st.data(), z->state.p, st.size() * sizeof(hmms_slot), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    for (int32_t s = 0; s < z->nslots; s++) z->n[(size_t)s] = st[(size_t)s].n;
    z->mirror_stale = false;
    return SK_OK;
}

// host forms: the slots against the session's nslots, and (len: the chunk lengths, or nullptr) the cap of a slot
int check_session_slots(sk_ctx *c, hmms_session *z, const int32_t *slots, int32_t m, const int64_t *len)
{
    if (len) { if (int rc = refresh_mirror(c, z)) return rc; }
    for (int32_t i = 0; i < m; i++) {
        const int32_t s = slots[i];
        if (s < 0 || s >= z->nslots) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, s, z->nslots);
        if (len && (int64_t)z->n[(size_t)s] + len[i] > HMMS_CAP)
            return sk_fail(SK_ERR_UNSUPPORTED, "entry %d: slot %d would hold more than %d samples", i, s, HMMS_CAP);
    }
    return SK_OK;
}

// bytes of slot state: 224 per slot, and 48 more for a filtered session's alpha
int64_t session_bytes(const hmms_session *z)
{
    return (int64_t)z->nslots * (int64_t)(sizeof(hmms_slot) + (z->filter ? sizeof(hmms_alpha) : 0));
}

int launch_reset(sk_ctx *c, hmms_session *z, const int32_t *d_slots, int32_t m, const double *d_cal2)
{
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_hmms_reset, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (hmms_slot *)z->state.p,
                       (hmms_alpha *)z->alpha.p, z->nslots, d_slots, m, d_cal2);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// the push proper, every pointer a device pointer; nothing is synchronised
int launch_push(sk_ctx *c, hmms_session *z, int feed, const int32_t *d_slots, int32_t m, const void *d_sig, int64_t stride,
                const int32_t *d_len, const int64_t *d_off, sk_hmms_rec *d_out)
{
    c->hmms_state_bytes = session_bytes(z);
    c->hmms_valid = true;
    if (m <= 0) return SK_OK;
    hmms_kargs a;
    a.state = (hmms_slot *)z->state.p; a.alpha = z->filter ? (hmms_alpha *)z->alpha.p : nullptr; a.nslots = z->nslots; a.m = m; a.slots = d_slots;
    a.sig = d_sig; a.stride = stride; a.len = d_len; a.off = d_off;
    a.vec = (feed == SK_FEED_I16 && (uintptr_t)d_sig % 16 == 0 && stride % 8 == 0) ? 1 : 0;
    a.out = d_out; a.guard = (unsigned long long *)c->hmmscnt.p; a.mdl = hmm_flatten(&z->model);
    const dim3 grid((unsigned)((m + 63) / 64));
    if (z->filter) {
        if (feed == SK_FEED_I16) hipLaunchKernelGGL((k_hmms_push<SK_FEED_I16, true>), grid, dim3(64), 0, c->stream, a);
        else                     hipLaunchKernelGGL((k_hmms_push<SK_FEED_F64_NORM, true>), grid, dim3(64), 0, c->stream, a);
    } else {
        if (feed == SK_FEED_I16) hipLaunchKernelGGL((k_hmms_push<SK_FEED_I16, false>), grid, dim3(64), 0, c->stream, a);
        else                     hipLaunchKernelGGL((k_hmms_push<SK_FEED_F64_NORM, false>), grid, dim3(64), 0, c->stream, a);
    }
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// a device-form push between the events sk_last_kernel_ms reads (no prep; main = the launch)
int timed_push(sk_ctx *c, hmms_session *z, int feed, const int32_t *d_slots, int32_t m, const void *d_sig, int64_t stride,
               const int32_t *d_len, const int64_t *d_off, sk_hmms_rec *d_out)
{
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if (int rc = launch_push(c, z, feed, d_slots, m, d_sig, stride, d_len, d_off, d_out)) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    z->mirror_stale = true;
    return SK_OK;
}

int reserve(sk_ctx *c, sk_buf *b, size_t bytes) { return sk_reserve(c, b, bytes ? bytes : 1); }

// what the arguments of a filter call decide (host: the slots can be read here; a slot may appear twice)
int check_filter(int32_t handle, const int32_t *slots, int32_t m, const sk_hmms_filt *out, bool host)
{
    if (int rc = check_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m == 0) return SK_OK;
    if (!slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    return host ? check_slots_host(slots, m, true) : SK_OK;
}

// the session of a handle, if it is open and carries alpha
hmms_session *filtered_session_of(sk_ctx *c, int32_t handle)
{
    hmms_session *z = session_of(c, handle);
    if (z && !z->filter) {
        sk_fail(SK_ERR_INVALID, "HMM session handle %d was opened without SK_HMMS_FILTER: it carries no alpha", handle);
        return nullptr;
    }
    return z;
}

// the filter proper, every pointer a device pointer; nothing is synchronised
int launch_filter(sk_ctx *c, hmms_session *z, const int32_t *d_slots, int32_t m, sk_hmms_filt *d_out)
{
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_hmms_filter, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (const hmms_slot *)z->state.p,
                       (const hmms_alpha *)z->alpha.p, z->nslots, (int32_t)z->model.nstates, d_slots, m, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// a session of nslots reset slots; filter: with alpha beside the slots (SK_HMMS_FILTER)
int session_open(sk_ctx *c, const sk_hmm_model *model, int32_t nslots, bool filter, int32_t *handle)
{
    int h = -1;
    for (int i = 0; i < SK_HMMS_MAX_SESSIONS; i++) if (!c->hmms_sessions[i]) { h = i; break; }
    if (h < 0) return sk_fail(SK_ERR_INVALID, "%d HMM sessions are open on this context already", SK_HMMS_MAX_SESSIONS);
    hmms_session *z = new hmms_session();
    z->nslots = nslots; z->model = *model; z->filter = filter;
    z->n.assign((size_t)nslots, 0);
    int rc = sk_reserve(c, &z->state, (size_t)nslots * sizeof(hmms_slot));
    if (!rc && filter) rc = sk_reserve(c, &z->alpha, (size_t)nslots * sizeof(hmms_alpha));
    if (!rc && !c->hmmscnt.p) {                             // the context's guard counter: 0 once, then it only counts
        rc = sk_reserve(c, &c->hmmscnt, sizeof(unsigned long long));
        if (!rc && hipMemsetAsync(c->hmmscnt.p, 0, sizeof(unsigned long long), c->stream) != hipSuccess)
            rc = sk_fail(SK_ERR_HIP, "clearing the guard counter failed");
    }
    if (!rc) rc = launch_reset(c, z, nullptr, nslots, nullptr);
    if (rc) { destroy(z); return rc; }
    c->hmms_sessions[h] = z;
    *handle = h;
    return SK_OK;
}

} // namespace

void sk_hmms_close_all(sk_ctx *c)
{
    for (int i = 0; i < SK_HMMS_MAX_SESSIONS; i++)
        if (c->hmms_sessions[i]) { destroy((hmms_session *)c->hmms_sessions[i]); c->hmms_sessions[i] = nullptr; }
}

// ---- the session behind sk_hmms_open, and the device forms a gated live session (sk_live.hip) drives its own with ----
int sk_hmms_session_open(sk_ctx *c, const sk_hmm_model *model, int32_t nslots, int32_t *handle)
{
    return session_open(c, model, nslots, false, handle);
}

// int16 rows, every pointer a device pointer, nothing synchronised, no event recorded
int sk_hmms_session_push_dev_i16(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows,
                                 int64_t stride, const int32_t *d_len, sk_hmms_rec *d_out)
{
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    z->mirror_stale = true;
    return launch_push(c, z, SK_FEED_I16, d_slots, m, d_rows, stride, d_len, nullptr, d_out);
}

// d_slots [m] (nullptr: all, m = nslots), d_cal2 [m][2] or nullptr: device pointers, nothing synchronised
int sk_hmms_session_reset_dev(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const double *d_cal2)
{
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    z->mirror_stale = true;
    return launch_reset(c, z, d_slots, m, d_cal2);
}

int64_t sk_hmms_session_bytes(sk_ctx *c, int32_t handle)
{
    hmms_session *z = session_of(c, handle);
    return z ? session_bytes(z) : 0;
}

int sk_hmms_session_close(sk_ctx *c, int32_t handle)
{
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipStreamSynchronize(c->stream));
    destroy(z);
    c->hmms_sessions[handle] = nullptr;
    return SK_OK;
}

// ------------------------------------------------------------------ the C ABI
// What the arguments alone decide is refused first, before a context is looked for; then what needs the session: is the
// handle open, does a slot lie below its nslots, would a slot pass its cap.
extern "C" {

int sk_hmms_open(const sk_hmm_model *model, int32_t nslots, int32_t *handle)
{
    if (const char *what = sk_hmm_model_error(model)) return sk_fail(SK_ERR_INVALID, "sk_hmm_model: %s", what);
    if (!handle) return sk_fail(SK_ERR_INVALID, "NULL handle");
    if (nslots < 1 || nslots > SK_HMMS_MAX_SLOTS)
        return sk_fail(SK_ERR_INVALID, "nslots = %d is outside 1 .. %d", nslots, SK_HMMS_MAX_SLOTS);
    SK_ENTER(c);
    return sk_hmms_session_open(c, model, nslots, handle);
}

int sk_hmms_open_ex(const sk_hmm_model *model, int32_t nslots, int32_t flags, int32_t *handle)
{
    if (flags & ~SK_HMMS_FILTER) return sk_fail(SK_ERR_INVALID, "flags = 0x%x: the only flag is SK_HMMS_FILTER", (unsigned)flags);
    if (const char *what = sk_hmm_model_error(model)) return sk_fail(SK_ERR_INVALID, "sk_hmm_model: %s", what);
    if (!handle) return sk_fail(SK_ERR_INVALID, "NULL handle");
    if (nslots < 1 || nslots > SK_HMMS_MAX_SLOTS)
        return sk_fail(SK_ERR_INVALID, "nslots = %d is outside 1 .. %d", nslots, SK_HMMS_MAX_SLOTS);
    SK_ENTER(c);
    return session_open(c, model, nslots, (flags & SK_HMMS_FILTER) != 0, handle);
}

int sk_hmms_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                         const int32_t *d_len, sk_hmms_rec *d_out)
{
    if (int rc = check_push_i16(handle, d_slots, m, d_rows, stride, d_len, d_out, false)) return rc;
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    return timed_push(c, z, SK_FEED_I16, d_slots, m, d_rows, stride, d_len, nullptr, d_out);
}

int sk_hmms_push_dev_f64(int32_t handle, const int32_t *d_slots, int32_t m, const double *d_values, const int64_t *d_off,
                         sk_hmms_rec *d_out)
{
    if (int rc = check_push_f64(handle, d_slots, m, d_values, d_off, d_out, false)) return rc;
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    return timed_push(c, z, SK_FEED_F64_NORM, d_slots, m, d_values, 0, nullptr, d_off, d_out);
}

int sk_hmms_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                     sk_hmms_rec *out)
{
    int rc = check_push_i16(handle, slots, m, rows, stride, len, out, true);
    if (rc) return rc;
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m == 0) return SK_OK;
    std::vector<int64_t> len64((size_t)m);
    int32_t maxlen = 0;
    for (int32_t i = 0; i < m; i++) { len64[(size_t)i] = len[i]; maxlen = len[i] > maxlen ? len[i] : maxlen; }
    if ((rc = check_session_slots(c, z, slots, m, len64.data()))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the staging buffers
    // the rows go up as [m][w], w = maxlen rounded up to 8 samples: 16-byte loads whatever the caller's stride
    const int64_t w = ((int64_t)maxlen + 7) / 8 * 8;
    const size_t mm = (size_t)m;
    if ((rc = reserve(c, &z->rows, mm * (size_t)w * sizeof(int16_t)))) return rc;
    if ((rc = reserve(c, &z->args, 2 * mm * sizeof(int32_t)))) return rc;
    if ((rc = reserve(c, &z->out, mm * sizeof(sk_hmms_rec)))) return rc;
    int16_t *d_rows = (int16_t *)z->rows.p;
    int32_t *d_slots = (int32_t *)z->args.p, *d_len = d_slots + mm;
    if (maxlen > 0)
        SK_HIP(hipMemcpy2DAsync(d_rows, (size_t)w * sizeof(int16_t), rows, (size_t)stride * sizeof(int16_t),
                                (size_t)maxlen * sizeof(int16_t), mm, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_slots, slots, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_len, len, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_push(c, z, SK_FEED_I16, d_slots, m, d_rows, w, d_len, nullptr, (sk_hmms_rec *)z->out.p))) return rc;
    SK_HIP(hipMemcpyAsync(out, z->out.p, mm * sizeof(sk_hmms_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    for (int32_t i = 0; i < m; i++) z->n[(size_t)slots[i]] += len[i];
    return SK_OK;
}

int sk_hmms_push_f64(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off, sk_hmms_rec *out)
{
    int rc = check_push_f64(handle, slots, m, values, off, out, true);
    if (rc) return rc;
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m == 0) return SK_OK;
    const size_t mm = (size_t)m;
    std::vector<int64_t> len64(mm), rel(mm + 1);
    for (int32_t i = 0; i < m; i++) len64[(size_t)i] = off[i + 1] - off[i];
    for (int32_t i = 0; i <= m; i++) rel[(size_t)i] = off[i] - off[0];
    if ((rc = check_session_slots(c, z, slots, m, len64.data()))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the staging buffers
    const size_t total = (size_t)rel[mm];
    if ((rc = reserve(c, &z->rows, total * sizeof(double)))) return rc;
    if ((rc = reserve(c, &z->args, (mm + 1) * sizeof(int64_t) + mm * sizeof(int32_t)))) return rc;
    if ((rc = reserve(c, &z->out, mm * sizeof(sk_hmms_rec)))) return rc;
    int64_t *d_off = (int64_t *)z->args.p;
    int32_t *d_slots = (int32_t *)(d_off + mm + 1);
    if (total) SK_HIP(hipMemcpyAsync(z->rows.p, values + off[0], total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_off, rel.data(), (mm + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_slots, slots, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_push(c, z, SK_FEED_F64_NORM, d_slots, m, z->rows.p, 0, nullptr, d_off, (sk_hmms_rec *)z->out.p))) return rc;
    SK_HIP(hipMemcpyAsync(out, z->out.p, mm * sizeof(sk_hmms_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));                // (rel is this call's memory)
    for (int32_t i = 0; i < m; i++) z->n[(size_t)slots[i]] += (int32_t)len64[(size_t)i];
    return SK_OK;
}

int sk_hmms_reset(int32_t handle, const int32_t *slots, int32_t m, const double *cal2)
{
    int rc = check_handle(handle);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    if ((rc = check_slots_host(slots, m, false))) return rc;
    if (cal2)
        for (int32_t i = 0; i < 2 * m; i++)
            if (!(cal2[i] - cal2[i] == 0.0))
                return sk_fail(SK_ERR_INVALID, "entry %d: the calibration pair {offset, unit} must be finite", i / 2);
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m == 0) return SK_OK;
    if ((rc = check_session_slots(c, z, slots, m, nullptr))) return rc;
    if ((rc = refresh_mirror(c, z))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the argument buffer
    const size_t mm = (size_t)m;
    if ((rc = reserve(c, &z->args, 2 * mm * sizeof(double) + mm * sizeof(int32_t)))) return rc;
    double *d_cal = (double *)z->args.p;
    int32_t *d_slots = (int32_t *)(d_cal + 2 * mm);
    if (cal2) SK_HIP(hipMemcpyAsync(d_cal, cal2, 2 * mm * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_slots, slots, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_reset(c, z, d_slots, m, cal2 ? d_cal : nullptr))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // (slots and cal2 are the caller's memory)
    for (int32_t i = 0; i < m; i++) z->n[(size_t)slots[i]] = 0;
    return SK_OK;
}

int sk_hmms_filter(int32_t handle, const int32_t *slots, int32_t m, sk_hmms_filt *out)
{
    int rc = check_filter(handle, slots, m, out, true);
    if (rc) return rc;
    SK_ENTER(c);
    hmms_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m > 0 && (rc = check_session_slots(c, z, slots, m, nullptr))) return rc;
    if (!(z = filtered_session_of(c, handle))) return SK_ERR_INVALID;
    if (m == 0) return SK_OK;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the staging buffers
    const size_t mm = (size_t)m;
    if ((rc = reserve(c, &z->args, mm * sizeof(int32_t)))) return rc;
    if ((rc = reserve(c, &z->out, mm * sizeof(sk_hmms_filt)))) return rc;
    SK_HIP(hipMemcpyAsync(z->args.p, slots, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_filter(c, z, (const int32_t *)z->args.p, m, (sk_hmms_filt *)z->out.p))) return rc;
    SK_HIP(hipMemcpyAsync(out, z->out.p, mm * sizeof(sk_hmms_filt), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_hmms_filter_dev(int32_t handle, const int32_t *d_slots, int32_t m, sk_hmms_filt *d_out)
{
    if (int rc = check_filter(handle, d_slots, m, d_out, false)) return rc;
    SK_ENTER(c);
    hmms_session *z = filtered_session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if (int rc = launch_filter(c, z, d_slots, m, d_out)) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

int sk_hmms_close(int32_t handle)
{
    if (int rc = check_handle(handle)) return rc;
    SK_ENTER(c);
    return sk_hmms_session_close(c, handle);
}

int sk_last_hmms_plan(int64_t *state_bytes, int64_t *guard_hits)
{
    SK_ENTER(c);
    if (state_bytes) *state_bytes = c->hmms_state_bytes;
    if (guard_hits) {
        unsigned long long g = 0;
        if (c->hmms_valid && c->hmmscnt.p) {
            SK_HIP(hipMemcpyAsync(&g, c->hmmscnt.p, sizeof(g), hipMemcpyDeviceToHost, c->stream));
            SK_HIP(hipStreamSynchronize(c->stream));
        }
        *guard_hits = (int64_t)g;
    }
    return SK_OK;
}

} // extern "C"
