// sk_evstream.hip -- event sessions: a read cut into events as its samples arrive (gfx950).
//
// The definition (include/squigglekit_hip.h, "event sessions"; tests/evstream_ref.py restates it on top of
// tests/detect_ref.py).  A session has `nslots` slots and one sk_det_params; a slot holds a read in progress: n, the
// samples it has had since its reset, the walk position i, both detectors' states and the last boundary.  A push
// appends len[k] samples to slot slots[k] and walks the positions i with i + w_long <= n: there t_short[i] and
// t_long[i] are what they will be in the finished read (k_detect_mark's DET_LAG reasoning with w_long in place of 64).
// Every mark closes the event [last boundary, pos) and emits its record at once: the marks of both detectors together
// come in strictly rising order, so nothing is buffered or sorted.  An entry flagged END walks the
// rest, i up to n - 1, under the one-shot rule (t_w[i] = 0 for i > n - w, samples at and beyond n count as 0) and emits
// the closing event [last boundary, n).  Everything a slot emits from reset to END is sk_detect_events' array of all its
// samples, byte for byte, whatever the cuts.
//
// k_evs_push    one lane per named entry, 64 entries per wavefront (one wavefront per workgroup), k_detect_mark's LDS
//               ring: 2 tiles of DET_TILE = 128 samples per row, row pitch 129 dwords.  A lane restores its slot's state;
//               the wavefront pre-fills the ring with every slot's carried tail -- its last 128 samples, 256 bytes,
//               which hold x[i - w_long .. i + w_long) of the resume position -- and streams the chunks tile by tile;
//               a row's ring index is the sample's READ position mod 256, so the 64 rows of a wavefront sit at 64
//               different phases.  Before a tile's walk a detector's forward sum takes in the samples that have become
//               known inside its window ([i, i + w) cut at the samples known so far: at most w, usually one); then the
//               lane steps the shared det_step / det_slide text.  Instead of mark bits the lane keeps the running
//               totals of x and x^2 over x[0..i) as int64 (exact: fewer than 2^31 samples of at most 2^30 each) and
//               snapshots them when a candidate moves; a mark's record is a difference of snapshots -- no sample is
//               re-read and no event's samples are kept, however long the event.  Records go to the entry's staging
//               rows (sized by fact 2: marks lie at least w_short / 2 + 1 apart), the count to cnt[k].  A lane that
//               would overrun its staging, meet a mark at or below its last boundary, or pass 2^31 - 1 samples stops
//               its slot, marks it broken and counts it (guard_hits: asserted zero by the tests, not a route).  The full
//               state goes back with plain vector stores, the tail cooperatively.
// k_evs_gather  one wavefront per entry: staging rows -> rec[off[k] ..], nothing when off[m] > cap.
// k_evs_reset   the named slots back to their first state.
//
// Lanes of one wavefront hold slots at different phases -- fresh, continuing, ending, empty chunk, ended, not named at
// all -- and every loop bound of the walk is the lane's own; only the tile loop and the cooperative loads are the
// wavefront's.
#include "sk_detect_dev.h"
#include <vector>

namespace {

enum { EVS_ENDED = 1, EVS_BROKEN = 2 };

struct evs_det {                 // a detector's part of a slot: 56 bytes
    int32_t A, B;
    int64_t Q;
    int32_t pos, masked_to;
    double  val;
    int32_t valid, pad;
    int64_t snap_s, snap_q;      // the totals over x[0..pos) of its candidate
};

struct evs_slot {                // 160 bytes (+ 256 bytes of tail)
    int32_t n, i, last, flags;
    int64_t tot_s, tot_q;        // sums of x and x^2 over x[0..i)
    int64_t last_s, last_q;      // ... over x[0..last)
    evs_det d[2];
};

static_assert(sizeof(evs_slot) == 160, "evs_slot is 160 bytes");

struct evs_kargs {
    evs_slot      *state;        // [nslots]
    int16_t       *tail;         // [nslots][DET_TILE]: x[pos] at pos mod 128, the last 128 positions
    int32_t        nslots;
    const int32_t *slots;        // [m]
    int32_t        m;
    const int16_t *rows;         // [m][stride]
    int64_t        stride;
    const int32_t *len;          // [m]
    const int32_t *end;          // [m] or nullptr
    int32_t        vec;          // rows are 16-byte aligned (base and stride): 16-byte loads
    sk_det_params  p;
    sk_det_event  *stage;        // [m][per]
    int64_t        per;
    int64_t       *cnt;          // [m]
    unsigned long long *guard;   // [1]
};

__device__ __forceinline__ void evs_load(det_state &d, const evs_det &s, int32_t w, double th)
{
    d.w = w; d.half = w / 2; d.th = th;
    d.A = s.A; d.B = s.B; d.Q = s.Q; d.pos = s.pos; d.masked_to = s.masked_to; d.val = s.val; d.valid = s.valid != 0;
}

__device__ __forceinline__ void evs_store(evs_det &s, const det_state &d)
{
    s.A = d.A; s.B = d.B; s.Q = d.Q; s.pos = d.pos; s.masked_to = d.masked_to; s.val = d.val; s.valid = d.valid ? 1 : 0;
    s.pad = 0;
}

__device__ __forceinline__ void evs_first(evs_slot &st)
{
    st.n = 0; st.i = 0; st.last = 0; st.flags = 0;
    st.tot_s = 0; st.tot_q = 0; st.last_s = 0; st.last_q = 0;
    for (int k = 0; k < 2; k++) {
        evs_det &e = st.d[k];
        e.A = 0; e.B = 0; e.Q = 0; e.pos = -1; e.masked_to = -1; e.val = __builtin_inf(); e.valid = 0; e.pad = 0;
        e.snap_s = 0; e.snap_q = 0;
    }
}

// the forward sum of a detector at position i takes in the samples [from, to) of its window [i, i + w) that have become known
__device__ __forceinline__ void evs_take(det_state &d, const int16_t *xrow, int32_t i, int32_t from, int32_t to)
{
    int32_t lo = from > i ? from : i;
    const int32_t hi = to < i + d.w ? to : i + d.w;
    for (; lo < hi; lo++) {
        const int32_t x = (int32_t)xrow[lo & (DET_RING - 1)];
        d.B += x;
        d.Q += (int64_t)(x * x);
    }
}

__global__ __launch_bounds__(64)
void k_evs_push(const evs_kargs a)
{
    __shared__ uint32_t ring[64 * DET_PITCH];
    __shared__ int32_t nold_s[64], len_s[64], slot_s[64];
    int16_t *ring16 = (int16_t *)ring;
    const int lane = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    const int64_t k = k0 + lane;

    int32_t slot = k < a.m ? a.slots[k] : -1;
    if (slot < 0 || slot >= a.nslots) slot = -1;
    evs_slot st;
    if (slot >= 0) st = a.state[slot];
    else evs_first(st);
    bool live = slot >= 0 && !(st.flags & (EVS_ENDED | EVS_BROKEN));
    int32_t len = 0;
    bool end = false;
    bool broken = false;
    if (live) {
        int64_t l = a.len[k];
        if (l < 0) l = 0;
        if (l > a.stride) l = a.stride;
        if ((int64_t)st.n + l > 0x7fffffffll) { broken = true; l = 0; }
        len = (int32_t)l;
        end = a.end && a.end[k] != 0;
    }
    const int32_t n_old = st.n, n_new = st.n + len;
    nold_s[lane] = n_old; len_s[lane] = len; slot_s[lane] = live ? slot : -1;
    int32_t maxlen = len;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(maxlen, o); maxlen = q > maxlen ? q : maxlen; }
    if (__ballot(live) == 0) {
        if (k < a.m) a.cnt[k] = 0;
        return;
    }
    __syncthreads();

    // the carried tails -> the ring, at the samples' read positions
    // (16 lanes per row, one 16-byte load each: tail entry q holds the one position of [n - 128, n) that is q mod 128)
#pragma unroll 4
    for (int it = 0; it < 16; it++) {
        const int row = it * 4 + (lane >> 4), q0 = (lane & 15) * 8;
        const int32_t s = slot_s[row];
        if (s < 0) continue;
        const int32_t lo = nold_s[row] - DET_TILE;
        const uint4 v = *(const uint4 *)(a.tail + (int64_t)s * DET_TILE + q0);
        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
        int16_t *dst = ring16 + row * (2 * DET_PITCH);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int32_t pos = lo + ((q0 + e - lo) & (DET_TILE - 1));
            if (pos >= 0) dst[pos & (DET_RING - 1)] = (int16_t)(wv[e >> 1] >> ((e & 1) * 16));
        }
    }

    const int16_t *xrow = ring16 + (size_t)lane * (2 * DET_PITCH);
    sk_det_event *mine = a.stage + (k < a.m ? k : 0) * a.per;
    const double h = a.p.peak_height;
    const int32_t wl = a.p.w_long;
    det_state ds, dl;
    evs_load(ds, st.d[0], a.p.w_short, a.p.th_short);
    evs_load(dl, st.d[1], a.p.w_long, a.p.th_long);
    int64_t ss_s = st.d[0].snap_s, ss_q = st.d[0].snap_q, sl_s = st.d[1].snap_s, sl_q = st.d[1].snap_q;
    int64_t tot_s = st.tot_s, tot_q = st.tot_q, last_s = st.last_s, last_q = st.last_q;
    int32_t i = st.i, last = st.last;
    int64_t count = 0;
    bool done = !live || broken;

    // a mark at p with the totals over x[0..p): the event [last, p)
    auto emit = [&](int32_t p, int64_t s, int64_t q) {
        if (broken) return;
        if (count >= a.per || p <= last) { broken = true; return; }
        sk_det_event e;
        e.start = last; e.length = p - last; e.sum = s - last_s; e.sumsq = q - last_q;
        mine[count++] = e;
        last = p; last_s = s; last_q = q;
    };

    const int ntiles = maxlen > 0 ? (maxlen + DET_TILE - 1) / DET_TILE : 1;
    for (int t = 0; t < ntiles; t++) {
        // tile t of the 64 chunks -> the ring
        if (a.vec) {
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int row = it * 4 + (lane >> 4);
                const int32_t c = t * DET_TILE + (lane & 15) * 8;
                const int32_t ln = len_s[row];
                if (c < ln) {
                    const uint4 v = *(const uint4 *)(a.rows + (k0 + row) * a.stride + c);
                    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
                    int16_t *dst = ring16 + row * (2 * DET_PITCH);
                    const int32_t base = nold_s[row] + c;
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        if (c + e < ln) dst[(base + e) & (DET_RING - 1)] = (int16_t)(wv[e >> 1] >> ((e & 1) * 16));
                }
            }
        } else {
            for (int row = 0; row < 64; row++) {
                const int32_t ln = len_s[row], no = nold_s[row];
                for (int cc = lane; cc < DET_TILE; cc += 64) {
                    const int32_t c = t * DET_TILE + cc;
                    if (c < ln) ring16[row * (2 * DET_PITCH) + ((no + c) & (DET_RING - 1))] = a.rows[(k0 + row) * a.stride + c];
                }
            }
        }
        __syncthreads();

        if (!done) {
            const int64_t c0 = (int64_t)t * DET_TILE, c1 = c0 + DET_TILE;
            const int32_t prev = n_old + (int32_t)(c0 < len ? c0 : len);
            const int32_t seen = n_old + (int32_t)(c1 < len ? c1 : len);
            const bool final = c1 >= len;
            evs_take(ds, xrow, i, prev, seen);
            evs_take(dl, xrow, i, prev, seen);
            const int32_t limit = (final && end) ? seen : seen - wl + 1;      // i + w_long <= seen
            for (; i < limit && !broken; i++) {
                if (i > ds.masked_to) {
                    int32_t mk = -1;
                    det_step(ds, &dl, h, i, det_t(ds, i, seen), [&](int32_t p) { mk = p; });
                    if (mk >= 0) emit(mk, ss_s, ss_q);
                    if (ds.pos == i) { ss_s = tot_s; ss_q = tot_q; }
                }
                if (i > dl.masked_to) {
                    int32_t mk = -1;
                    det_step(dl, nullptr, h, i, det_t(dl, i, seen), [&](int32_t p) { mk = p; });
                    if (mk >= 0) emit(mk, sl_s, sl_q);
                    if (dl.pos == i) { sl_s = tot_s; sl_q = tot_q; }
                }
                const int32_t xi = (int32_t)xrow[i & (DET_RING - 1)];
                det_slide(ds, xrow, i, seen, xi);
                det_slide(dl, xrow, i, seen, xi);
                tot_s += xi; tot_q += (int64_t)(xi * xi);
            }
            if (final || broken) done = true;
        }
        __syncthreads();                                        // the ring's other half is read before tile t + 1 lands
    }

    if (live) {
        if (end && !broken) {
            if (n_new > 0) {
                if (count >= a.per) broken = true;
                else {
                    sk_det_event e;
                    e.start = last; e.length = n_new - last; e.sum = tot_s - last_s; e.sumsq = tot_q - last_q;
                    mine[count++] = e;
                    last = n_new; last_s = tot_s; last_q = tot_q;
                }
            }
            st.flags |= EVS_ENDED;
        }
        if (broken) {
            st.flags |= EVS_BROKEN;
            atomicAdd(a.guard, 1ull);
        }
        st.n = n_new; st.i = i; st.last = last;
        st.tot_s = tot_s; st.tot_q = tot_q; st.last_s = last_s; st.last_q = last_q;
        evs_store(st.d[0], ds); st.d[0].snap_s = ss_s; st.d[0].snap_q = ss_q;
        evs_store(st.d[1], dl); st.d[1].snap_s = sl_s; st.d[1].snap_q = sl_q;
        a.state[slot] = st;
    }
    if (k < a.m) a.cnt[k] = count;

    // the last 128 samples of every row -> its slot's tail
    // (a row that got samples rewrites its whole tail, 16 lanes with a 16-byte store each: the ring holds all of
    // [n - 128, n) -- restored or new; entries of positions below 0 are written as 0 and never read)
#pragma unroll 4
    for (int it = 0; it < 16; it++) {
        const int row = it * 4 + (lane >> 4), q0 = (lane & 15) * 8;
        const int32_t s = slot_s[row];
        if (s < 0 || len_s[row] == 0) continue;
        const int32_t lo = nold_s[row] + len_s[row] - DET_TILE;
        const int16_t *src = ring16 + row * (2 * DET_PITCH);
        uint32_t wv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int32_t pos = lo + ((q0 + e - lo) & (DET_TILE - 1));
            const uint32_t x = pos >= 0 ? (uint32_t)(uint16_t)src[pos & (DET_RING - 1)] : 0u;
            wv[e >> 1] |= x << ((e & 1) * 16);
        }
        *(uint4 *)(a.tail + (int64_t)s * DET_TILE + q0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    }
}

__global__ __launch_bounds__(64)
void k_evs_gather(const sk_det_event *__restrict__ stage, int64_t per, const int64_t *__restrict__ off, int32_t m,
                  sk_det_event *__restrict__ rec, int64_t cap)
{
    const int64_t k = blockIdx.x;
    if (k >= m || !rec || off[m] > cap) return;
    const int64_t at = off[k], cnt = off[k + 1] - at;
    const sk_det_event *src = stage + k * per;
    for (int64_t j = threadIdx.x; j < cnt && j < per; j += 64) rec[at + j] = src[j];
}

__global__ void k_evs_reset(evs_slot *state, int32_t nslots, const int32_t *slots, int32_t m)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m) return;
    const int32_t s = slots ? slots[idx] : idx;
    if (s < 0 || s >= nslots) return;
    evs_slot st;
    evs_first(st);
    state[s] = st;
}

struct evs_session {
    int32_t nslots = 0;
    sk_det_params p;
    sk_buf state, tail;                     // evs_slot [nslots], int16 [nslots][128]
    std::vector<int32_t> n;                 // per slot, as the host form knows them: samples since the reset,
    std::vector<uint8_t> ended;             // END seen
    bool mirror_stale = false;              // a device-form push has moved slots the host did not see
    // the last push: its staging rows, counts / offsets and block sums stay until the next one
    sk_buf stage, off, args, out;           // records [m][per]; off [m + 1] then the scan's block sums; the host form's
                                            // slots / len / end and its rows; the compact records of a host push or fetch
    sk_buf rows;
    int32_t last_m = 0;
    int64_t last_per = 0;
    bool    pushed = false;
};

void free_buf(sk_buf *b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

void destroy(evs_session *z)
{
    sk_buf *bufs[] = {&z->state, &z->tail, &z->stage, &z->off, &z->args, &z->out, &z->rows};
    for (sk_buf *b : bufs) free_buf(b);
    delete z;
}

evs_session *session_of(sk_ctx *c, int32_t handle)
{
    if (handle < 0 || handle >= SK_EVS_MAX_SESSIONS || !c->evs_sessions[handle]) {
        sk_fail(SK_ERR_INVALID, "unknown event session handle %d", handle);
        return nullptr;
    }
    return (evs_session *)c->evs_sessions[handle];
}

int launch_reset(sk_ctx *c, evs_session *z, const int32_t *d_slots, int32_t m)
{
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_evs_reset, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (evs_slot *)z->state.p, z->nslots,
                       d_slots, m);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// the host's view of n / ended after device-form pushes: read back from the slots
int refresh_mirror(sk_ctx *c, evs_session *z)
{
    if (!z->mirror_stale) return SK_OK;
    std::vector<evs_slot> st((size_t)z->nslots);
    SK_HIP(hipMemcpyAsync(st.data(), z->state.p, st.size() * sizeof(evs_slot), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    for (int32_t s = 0; s < z->nslots; s++) {
        z->n[(size_t)s] = st[(size_t)s].n;
        z->ended[(size_t)s] = (st[(size_t)s].flags & EVS_ENDED) ? 1 : 0;
    }
    z->mirror_stale = false;
    return SK_OK;
}

} // namespace

// staging rows of an entry of at most maxlen samples: its push walks at most maxlen + w_long positions, marks lie at
// least w_short / 2 + 1 apart (fact 2: k walked positions emit at most k / (w_short / 2 + 1) + 2 events), and END adds
// the closing event
int64_t sk_evs_session_rows(sk_ctx *c, int32_t handle, int64_t maxlen)
{
    evs_session *z = session_of(c, handle);
    if (!z) return 0;
    return (maxlen + z->p.w_long) / (z->p.w_short / 2 + 1) + 3;
}

int sk_evs_session_open(sk_ctx *c, const sk_det_params *p, int32_t nslots, int32_t *handle)
{
    int h = -1;
    for (int i = 0; i < SK_EVS_MAX_SESSIONS; i++) if (!c->evs_sessions[i]) { h = i; break; }
    if (h < 0) return sk_fail(SK_ERR_INVALID, "%d event sessions are open on this context already", SK_EVS_MAX_SESSIONS);
    evs_session *z = new evs_session();
    z->nslots = nslots; z->p = *p;
    z->n.assign((size_t)nslots, 0);
    z->ended.assign((size_t)nslots, 0);
    int rc = sk_reserve(c, &z->state, (size_t)nslots * sizeof(evs_slot));
    if (!rc) rc = sk_reserve(c, &z->tail, (size_t)nslots * DET_TILE * sizeof(int16_t));
    // (the tails need no clearing: an entry is read only for a position the slot has been given)
    if (!rc && !c->evscnt.p) {                              // the context's guard counter: 0 once, then it only counts
        rc = sk_reserve(c, &c->evscnt, sizeof(unsigned long long));
        if (!rc && hipMemsetAsync(c->evscnt.p, 0, sizeof(unsigned long long), c->stream) != hipSuccess)
            rc = sk_fail(SK_ERR_HIP, "clearing the guard counter failed");
    }
    if (!rc) rc = launch_reset(c, z, nullptr, nslots);
    if (rc) { destroy(z); return rc; }
    c->evs_sessions[h] = z;
    *handle = h;
    return SK_OK;
}

int sk_evs_session_info(sk_ctx *c, int32_t handle, int32_t *nslots)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (nslots) *nslots = z->nslots;
    return SK_OK;
}

// host form: slots against the session's nslots (a push has been checked for a slot named twice; a reset may name one
// twice), samples for an ended slot, a total past 2^31 - 1
int sk_evs_session_check(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const int32_t *len)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (int rc = refresh_mirror(c, z)) return rc;
    for (int32_t i = 0; i < m; i++) {
        const int32_t s = slots[i];
        if (s < 0 || s >= z->nslots) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, s, z->nslots);
        if (!len) continue;
        if (z->ended[(size_t)s] && len[i] > 0)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d has ended and takes no samples until it is reset", i, s);
        if ((int64_t)z->n[(size_t)s] + len[i] > 0x7fffffffll)
            return sk_fail(SK_ERR_UNSUPPORTED, "entry %d: slot %d would hold more than 2147483647 samples", i, s);
    }
    return SK_OK;
}

// host form of a session that keeps a second, smaller sample cap per slot (a gated live session: the HMM side's)
int sk_evs_session_check_cap(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const int32_t *len, int64_t cap)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (int rc = refresh_mirror(c, z)) return rc;
    for (int32_t i = 0; i < m; i++) {
        const int32_t s = slots[i];
        if (s < 0 || s >= z->nslots) continue;
        if ((int64_t)z->n[(size_t)s] + len[i] > cap)
            return sk_fail(SK_ERR_UNSUPPORTED, "entry %d: slot %d would hold more than %lld samples", i, s, (long long)cap);
    }
    return SK_OK;
}

int sk_evs_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    sk_buf *b = which == 0 ? &z->rows : which == 1 ? &z->args : which == 2 ? &z->out : nullptr;
    if (!b) return sk_fail(SK_ERR_INVALID, "internal: staging buffer %d", which);
    const int rc = sk_reserve(c, b, bytes ? bytes : 1);
    if (rc) return rc;
    *p = b->p;
    return SK_OK;
}

// the push proper, every pointer a device pointer: walk, scan (d_off [m + 1], also kept by the session).  per: staging
// rows per entry.  host_len: the host form's lengths and END flags (nullptr: a device-form push), for the host's view.
int sk_evs_session_push(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                        const int32_t *d_len, const int32_t *d_end, int64_t per, int64_t *d_off, const int32_t *host_slots,
                        const int32_t *host_len, const int32_t *host_end)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    int rc;
    const size_t off_bytes = ((size_t)m + 1 + (size_t)sk_scan_blocks(m > 0 ? m : 1)) * sizeof(int64_t);
    if ((rc = sk_reserve(c, &z->stage, (size_t)(m > 0 ? m : 1) * (size_t)per * sizeof(sk_det_event)))) return rc;
    if ((rc = sk_reserve(c, &z->off, off_bytes))) return rc;
    int64_t *k_off = (int64_t *)z->off.p, *d_bsum = k_off + m + 1;
    z->last_m = m; z->last_per = per; z->pushed = true;
    c->evs_state_bytes = (int64_t)z->nslots * (int64_t)(sizeof(evs_slot) + DET_TILE * sizeof(int16_t));
    c->evs_staged = (int64_t)m * per;
    c->evs_valid = true;
    if (m == 0) {
        SK_HIP(hipMemsetAsync(k_off, 0, sizeof(int64_t), c->stream));
        if (d_off) SK_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), c->stream));
        return SK_OK;
    }
    evs_kargs a;
    a.state = (evs_slot *)z->state.p; a.tail = (int16_t *)z->tail.p; a.nslots = z->nslots;
    a.slots = d_slots; a.m = m; a.rows = d_rows; a.stride = stride; a.len = d_len; a.end = d_end;
    a.vec = ((uintptr_t)d_rows % 16 == 0 && stride % 8 == 0) ? 1 : 0;
    a.p = z->p; a.stage = (sk_det_event *)z->stage.p; a.per = per; a.cnt = k_off;
    a.guard = (unsigned long long *)c->evscnt.p;
    hipLaunchKernelGGL(k_evs_push, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    if ((rc = sk_launch_scan_i64(c, k_off, m, d_bsum, k_off))) return rc;
    if (d_off)
        SK_HIP(hipMemcpyAsync(d_off, k_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
    if (host_len) {
        for (int32_t i = 0; i < m; i++) {
            const size_t s = (size_t)host_slots[i];
            if (z->ended[s]) continue;
            z->n[s] += host_len[i];
            if (host_end && host_end[i]) z->ended[s] = 1;
        }
    } else {
        z->mirror_stale = true;
    }
    return SK_OK;
}

// the records of the last push, compact, at d_rec (device) -- on the device nothing happens when off[m] > cap
int sk_evs_session_gather(sk_ctx *c, int32_t handle, sk_det_event *d_rec, int64_t cap)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (!z->pushed || z->last_m <= 0 || !d_rec || cap <= 0) return SK_OK;
    hipLaunchKernelGGL(k_evs_gather, dim3((unsigned)z->last_m), dim3(64), 0, c->stream, (const sk_det_event *)z->stage.p,
                       z->last_per, (const int64_t *)z->off.p, z->last_m, d_rec, cap);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// the last push's off (device, [m + 1]) and m; m = 0 before the first push
int sk_evs_session_last(sk_ctx *c, int32_t handle, const int64_t **d_off, int32_t *m)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    *d_off = (const int64_t *)z->off.p;
    *m = z->pushed ? z->last_m : 0;
    return SK_OK;
}

// the last push's staging rows (device, [m][per]: entry k's new events are its first off[k + 1] - off[k] rows) and per
int sk_evs_session_staging(sk_ctx *c, int32_t handle, const sk_det_event **d_stage, int64_t *per)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    *d_stage = (const sk_det_event *)z->stage.p;
    *per = z->pushed ? z->last_per : 0;
    return SK_OK;
}

int sk_evs_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    int rc;
    if ((rc = sk_evs_session_check(c, handle, slots, m, nullptr))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier call may still read the argument buffer
    if ((rc = sk_reserve(c, &z->args, (size_t)m * sizeof(int32_t)))) return rc;
    SK_HIP(hipMemcpyAsync(z->args.p, slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_reset(c, z, (const int32_t *)z->args.p, m))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));               // (slots is the caller's memory)
    for (int32_t i = 0; i < m; i++) { z->n[(size_t)slots[i]] = 0; z->ended[(size_t)slots[i]] = 0; }
    return SK_OK;
}

int sk_evs_session_close(sk_ctx *c, int32_t handle)
{
    evs_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipStreamSynchronize(c->stream));
    destroy(z);
    c->evs_sessions[handle] = nullptr;
    return SK_OK;
}

void sk_evs_close_all(sk_ctx *c)
{
    for (int i = 0; i < SK_EVS_MAX_SESSIONS; i++)
        if (c->evs_sessions[i]) { destroy((evs_session *)c->evs_sessions[i]); c->evs_sessions[i] = nullptr; }
}
