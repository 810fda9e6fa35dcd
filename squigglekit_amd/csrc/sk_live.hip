// sk_live.hip -- live mapping sessions: samples in, mapping records and decisions out (gfx950).
//
// The definition (include/squigglekit_hip.h, "Live mapping sessions"; tests/live_ref.py restates it on top of
// evstream_ref and mapstream_ref).  A live session owns an event session and a mapping session -- opened through their
// internal functions, so it holds one handle of each table -- and joins them on the device: a push cuts events with
// k_evs_push, unchanged, and sweeps with k_sdtw, unchanged.  What is new is the BRIDGE between them and the DECISION
// SUMMARY behind them.
//
// k_live_count  one wavefront per named entry.  Reads the entry's staging rows of the event session's push (its new
//               events), restores the slot's record, and while the slot is CALIBRATING appends the new levels
//               (double)sum / (double)length to the slot's hold buffer (C doubles).  When calibration completes -- C
//               levels, or END -- the wavefront takes np.mean and np.std of the head with wave_np_sum (sk_prepw_dev.h:
//               np.add.reduce's order, a leaf per lane, the tree in 256 doubles of LDS), two passes, and the slot becomes
//               MAPPING or UNDECIDABLE.  Writes the slot's record back, info[k] and the entry's output length cnt[k].
// (scan)        sk_launch_scan_i64: cnt -> off [m + 1].
// k_live_fill   one wavefront per entry: (level - mean) / sd, compact at values[off[k] ..]: the held levels first (an
//               entry whose slot has just become MAPPING), then the new ones.
// k_live_best   one lane per entry: api.map_decide's rule over the [T][m] records of the push, expression for
//               expression (single float64 divides and compares).  The records of a fixed target are contiguous over
//               the entries, so a wavefront's loads coalesce; T is small wherever a device rule is used (whole targets).
//
// The order of a push: event push, count, scan, fill, the read-back of off (m + 1 int64: sk_map_session_push plans on the
// host from lengths), the mapping push on the compact values, the summary.  Every division is a correctly rounded IEEE
// operation (-ffp-contract=off is the build's rule), so the values are numpy's bit for bit.
//
// A GATED session ("Gated live sessions" in the header; kernels in sk_livegate.hip) also owns an HMM session.  Its push:
// event push, the HMM chunk lengths, the HMM push (k_hmms_push, unchanged, on the same rows), the gate, a scan of the
// released counts -- and then count, scan, fill and the rest exactly as above, with stage / per / eoff pointing at the
// released rows instead of the event push's staging rows.  The read-back stays the m + 1 offsets.
#include "sk_common.h"
#include "sk_prepw_dev.h"
#include <math.h>
#include <vector>

namespace {

static_assert(sizeof(sk_live_info) == 40 && sizeof(sk_live_best) == 40, "sk_live_info and sk_live_best are 40 bytes");
static_assert(SK_LIVE_MAX_CALIB <= NPY_REDUCE_CHUNK, "the head is one numpy reduction buffer");

// a slot's record is an sk_live_info (new_events: of the last push that named it)
__device__ __forceinline__ sk_live_info live_first()
{
    sk_live_info s;
    s.mean = __builtin_nan(""); s.sd = __builtin_nan("");
    s.events = 0; s.mapped = 0; s.held = 0; s.state = SK_LIVE_CALIBRATING; s.ended = 0; s.new_events = 0;
    return s;
}

__device__ __forceinline__ double live_level(const sk_det_event &e) { return (double)e.sum / (double)e.length; }

struct live_kargs {
    sk_live_info        *state;     // [nslots]
    double              *hold;      // [nslots][C]
    int32_t              nslots, C;
    const int32_t       *slots;     // [m]
    int32_t              m;
    const int32_t       *end;       // [m] or nullptr
    const sk_det_event  *stage;     // [m][per]: the event push's staging rows
    int64_t              per;
    const int64_t       *eoff;      // [m + 1]: the event push's offsets
    int64_t             *cnt;       // [m] out: levels entry k hands to the mapping side
    sk_live_info        *info;      // [m] out
};

__global__ __launch_bounds__(64)
void k_live_count(const live_kargs a)
{
    __shared__ double nodes[256];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (k >= a.m) return;
    const int32_t slot = a.slots[k];
    if (slot < 0 || slot >= a.nslots) {                     // (never: both entry points check the slot numbers)
        if (lane == 0) { a.cnt[k] = 0; a.info[k] = live_first(); }
        return;
    }
    sk_live_info st = a.state[slot];
    int64_t n64 = a.eoff[k + 1] - a.eoff[k];
    if (n64 < 0) n64 = 0;
    if (n64 > a.per) n64 = a.per;
    const int32_t n = (int32_t)n64, C = a.C;
    const int32_t E0 = st.events, E = E0 + n;
    const sk_det_event *mine = a.stage + k * a.per;
    double *hold = a.hold + (int64_t)slot * C;
    const bool ended = st.ended != 0 || (a.end && a.end[k] != 0);
    int64_t outlen = 0;

    if (st.state == SK_LIVE_CALIBRATING) {
        // the new levels -> the hold buffer, as far as the head reaches (E0 < C here: a slot with C levels has decided)
        for (int32_t j = lane; j < n && E0 + j < C; j += 64) hold[E0 + j] = live_level(mine[j]);
        if (E < C && !ended) {
            st.held = E;
        } else {
            const int32_t h = E < C ? E : C;
            __syncthreads();                                // the wavefront's stores to hold are read by all its lanes
            double mean = __builtin_nan(""), sd = __builtin_nan("");
            bool ok = false;
            if (h >= 2) {
                mean = wave_np_sum<true>(h, nodes, lane, [&](int j) { return hold[j]; }) / (double)h;
                const double ssq = wave_np_sum(h, nodes, lane, [&](int j) { const double q = hold[j] - mean; return q * q; });
                sd = sqrt(ssq / (double)h);
                ok = sd > 0;
            }
            st.held = 0;
            if (ok) {
                st.state = SK_LIVE_MAPPING; st.mean = mean; st.sd = sd;
                outlen = E; st.mapped = E;
            } else {
                st.state = SK_LIVE_UNDECIDABLE; st.mean = __builtin_nan(""); st.sd = __builtin_nan("");
            }
        }
    } else if (st.state == SK_LIVE_MAPPING) {
        outlen = n; st.mapped += n;
    }
    st.events = E; st.ended = ended ? 1 : 0; st.new_events = n;
    if (lane == 0) { a.state[slot] = st; a.info[k] = st; a.cnt[k] = outlen; }
}

__global__ __launch_bounds__(64)
void k_live_fill(const live_kargs a, const int64_t *__restrict__ off, double *__restrict__ values)
{
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (k >= a.m) return;
    const int64_t at = off[k], len = off[k + 1] - at;
    if (len <= 0) return;
    const int32_t slot = a.slots[k];
    if (slot < 0 || slot >= a.nslots) return;
    const sk_live_info st = a.info[k];
    int64_t fresh = st.new_events;                          // the tail of the chunk: this push's events
    if (fresh > len) fresh = len;
    if (fresh > a.per) fresh = a.per;
    int64_t held = len - fresh;                             // in front of them: what the slot held back (< C)
    if (held > a.C) held = a.C;
    const double mean = st.mean, sd = st.sd;
    const double *hold = a.hold + (int64_t)slot * a.C;
    const sk_det_event *mine = a.stage + k * a.per;
    for (int64_t j = lane; j < held; j += 64) values[at + j] = (hold[j] - mean) / sd;
    for (int64_t j = lane; j < fresh; j += 64) values[at + held + j] = (live_level(mine[j]) - mean) / sd;
}

__global__ void k_live_best(const sk_map_rec *__restrict__ rec, int32_t m, int32_t T, const sk_live_rule rule,
                            sk_live_best *__restrict__ best)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double inf = __builtin_inf();
    auto dist_of = [&](int32_t t) { const double d = rec[(int64_t)t * m + i].dist; return d != d ? inf : d; };
    // np.argmin of the column: the first of the smallest; has: some dist is a number
    int32_t b = 0;
    double db = dist_of(0);
    bool has = rec[i].dist == rec[i].dist;
    for (int32_t t = 1; t < T; t++) {
        const double raw = rec[(int64_t)t * m + i].dist;
        has = has || raw == raw;
        const double d = raw != raw ? inf : raw;
        if (d < db) { db = d; b = t; }
    }
    // ... and of the column with the best set to +inf
    int32_t s = -1;
    double ds = inf;
    if (T > 1) {
        s = 0; ds = b == 0 ? inf : dist_of(0);
        for (int32_t t = 1; t < T; t++) {
            const double d = t == b ? inf : dist_of(t);
            if (d < ds) { ds = d; s = t; }
        }
    }
    const sk_map_rec rb = rec[(int64_t)b * m + i];
    const double rows = (double)rb.rows;
    bool accept = has && rows >= (double)rule.min_rows && db / rows <= rule.max_dist_per_row;
    if (T > 1) accept = accept && (ds - db) / rows >= rule.min_margin;
    sk_live_best o;
    o.dist = has ? rb.dist : __builtin_nan("");
    o.second_dist = s >= 0 ? rec[(int64_t)s * m + i].dist : __builtin_nan("");
    o.target = has ? b : -1;
    o.start = has ? rb.start : -1;
    o.end = has ? rb.end : -1;
    o.rows = rb.rows;
    o.second_target = s;
    o.decision = accept ? 1 : (has && rows >= (double)rule.give_up_rows) ? -1 : 0;
    best[i] = o;
}

__global__ void k_live_reset(sk_live_info *state, int32_t nslots, const int32_t *slots, int32_t m)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m) return;
    const int32_t s = slots ? slots[idx] : idx;
    if (s < 0 || s >= nslots) return;
    state[s] = live_first();
}

struct live_session {
    int32_t nslots = 0, C = 0, T = 0;
    int32_t evs = -1, map = -1;             // the inner sessions' handles
    sk_buf state, hold;                     // sk_live_info [nslots], double [nslots][C]
    // the last push: the chunk lengths / offsets (then the scan's block sums) and the compact normalised levels
    sk_buf off, values;
    sk_buf host[4];                         // the host entry points' staging: records, info, best, reset slots
    std::vector<int64_t> hoff;              // off on the host (kept alive for the plan)
    int32_t last_m = 0;
    bool    pushed = false;
    hipEvent_t ev_best[2] = {nullptr, nullptr};     // around the last push's summary kernel (sk_live_last_ms)
    bool    best_timed = false;
    // a gated session (sk_livegate.hip): its HMM session, the rule, and per slot a gate record and a ring of G events
    bool    gated = false;
    int32_t hmms = -1, G = 0;
    sk_live_gate rule = {};
    sk_buf gstate, ring;                    // sk_gate_slot [nslots], sk_det_event [nslots][G]
    // the last push: HMM chunk lengths, HMM records, gate records, released rows [m][G + per], their counts / offsets
    sk_buf hlen, hrec, ginfo, rel, roff;
    hipEvent_t ev_gate[4] = {nullptr, nullptr, nullptr, nullptr};   // around the HMM side, around the gate and its scan
    bool    gate_timed = false;
};

void free_buf(sk_buf *b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

void destroy(live_session *z)
{
    sk_buf *bufs[] = {&z->state, &z->hold, &z->off, &z->values, &z->host[0], &z->host[1], &z->host[2], &z->host[3],
                      &z->gstate, &z->ring, &z->hlen, &z->hrec, &z->ginfo, &z->rel, &z->roff};
    for (sk_buf *b : bufs) free_buf(b);
    for (hipEvent_t e : z->ev_best) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : z->ev_gate) if (e) (void)hipEventDestroy(e);
    delete z;
}

live_session *session_of(sk_ctx *c, int32_t handle)
{
    if (handle < 0 || handle >= SK_LIVE_MAX_SESSIONS || !c->live_sessions[handle]) {
        sk_fail(SK_ERR_INVALID, "unknown live session handle %d", handle);
        return nullptr;
    }
    return (live_session *)c->live_sessions[handle];
}

int launch_reset(sk_ctx *c, live_session *z, const int32_t *d_slots, int32_t m)
{
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_live_reset, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (sk_live_info *)z->state.p,
                       z->nslots, d_slots, m);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

} // namespace

int sk_live_session_open(sk_ctx *c, const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off,
                         int32_t ntargets, int32_t nslots, const sk_hmm_model *model, const sk_live_gate *gate, int32_t *handle)
{
    int h = -1;
    for (int i = 0; i < SK_LIVE_MAX_SESSIONS; i++) if (!c->live_sessions[i]) { h = i; break; }
    if (h < 0) return sk_fail(SK_ERR_INVALID, "%d live sessions are open on this context already", SK_LIVE_MAX_SESSIONS);
    live_session *z = new live_session();
    z->nslots = nslots; z->C = calib; z->T = ntargets;
    int rc = sk_evs_session_open(c, p, nslots, &z->evs);
    if (rc) { destroy(z); return rc; }
    if ((rc = sk_map_session_open(c, targets, target_off, ntargets, nslots, &z->map))) {
        (void)sk_evs_session_close(c, z->evs);
        destroy(z);
        return rc;
    }
    if (model && (rc = sk_hmms_session_open(c, model, nslots, &z->hmms))) {
        (void)sk_evs_session_close(c, z->evs);
        (void)sk_map_session_close(c, z->map);
        destroy(z);
        return rc;
    }
    rc = sk_reserve(c, &z->state, (size_t)nslots * sizeof(sk_live_info));
    if (!rc) rc = sk_reserve(c, &z->hold, (size_t)nslots * (size_t)calib * sizeof(double));
    // (the hold buffers need no clearing: an entry is read only below the slot's event count)
    for (int i = 0; i < 2 && !rc; i++)
        if (hipEventCreate(&z->ev_best[i]) != hipSuccess) rc = sk_fail(SK_ERR_HIP, "creating the summary's events failed");
    if (!rc) rc = launch_reset(c, z, nullptr, nslots);
    if (!rc && model) {
        z->gated = true; z->rule = *gate; z->G = gate->hold;
        rc = sk_reserve(c, &z->gstate, (size_t)nslots * sizeof(sk_gate_slot));
        // (the rings need no clearing: an entry is read only below the slot's ring count)
        if (!rc) rc = sk_reserve(c, &z->ring, (size_t)nslots * (size_t)z->G * sizeof(sk_det_event));
        if (!rc) rc = sk_livegate_reset(c, (sk_gate_slot *)z->gstate.p, nslots, nullptr, nslots);
        for (int i = 0; i < 4 && !rc; i++)
            if (hipEventCreate(&z->ev_gate[i]) != hipSuccess) rc = sk_fail(SK_ERR_HIP, "creating the gate's events failed");
    }
    if (rc) {
        (void)sk_evs_session_close(c, z->evs);
        (void)sk_map_session_close(c, z->map);
        if (z->hmms >= 0) (void)sk_hmms_session_close(c, z->hmms);
        destroy(z);
        return rc;
    }
    c->live_sessions[h] = z;
    *handle = h;
    return SK_OK;
}

int sk_live_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *ntargets, int32_t *evs, int32_t *map)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (nslots) *nslots = z->nslots;
    if (ntargets) *ntargets = z->T;
    if (evs) *evs = z->evs;
    if (map) *map = z->map;
    return SK_OK;
}

int sk_live_session_gate_last(sk_ctx *c, int32_t handle, const sk_live_gate_info **d_gate, const sk_hmms_rec **d_rec, int32_t *m)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (!z->gated) return sk_fail(SK_ERR_INVALID, "live session %d has no gate", handle);
    *d_gate = (const sk_live_gate_info *)z->ginfo.p;
    *d_rec = (const sk_hmms_rec *)z->hrec.p;
    *m = z->pushed ? z->last_m : 0;
    return SK_OK;
}

// what a push is refused for by the session: slots against nslots and for doubles, (len given: the host form) samples
// for an ended slot and a total past 2^31 - 1, a stride whose events could pass the mapping side's chunk limit
int sk_live_session_check(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, int64_t stride, const int32_t *len)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    int rc;
    if ((rc = sk_map_session_check_slots(c, z->map, slots, m))) return rc;
    if (len && (rc = sk_evs_session_check(c, z->evs, slots, m, len))) return rc;
    if (len && z->gated && (rc = sk_evs_session_check_cap(c, z->evs, slots, m, len, SK_HMMS_CAP))) return rc;
    if (stride >= 0) {
        const int64_t per = sk_evs_session_rows(c, z->evs, stride);
        if (z->gated && (int64_t)(z->C - 1) + z->G + per > SK_MAP_MAX_CHUNK)
            return sk_fail(SK_ERR_UNSUPPORTED, "live session push: calib - 1 = %d held levels, hold = %d gated events and up to %lld "
                           "events of %lld samples could make a chunk above %d points", z->C - 1, z->G, (long long)per,
                           (long long)stride, SK_MAP_MAX_CHUNK);
        if ((int64_t)(z->C - 1) + per > SK_MAP_MAX_CHUNK)
            return sk_fail(SK_ERR_UNSUPPORTED, "live session push: calib - 1 = %d held levels and up to %lld events of %lld samples "
                           "could make a chunk above %d points", z->C - 1, (long long)per, (long long)stride, SK_MAP_MAX_CHUNK);
    }
    return SK_OK;
}

int sk_live_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (which < 0 || which >= 4) return sk_fail(SK_ERR_INVALID, "internal: staging buffer %d", which);
    const int rc = sk_reserve(c, &z->host[which], bytes ? bytes : 1);
    if (rc) return rc;
    *p = z->host[which].p;
    return SK_OK;
}

int sk_live_session_push(sk_ctx *c, int32_t handle, const int32_t *host_slots, const int32_t *d_slots, int32_t m,
                         const int16_t *d_rows, int64_t stride, const int32_t *d_len, const int32_t *d_end, int64_t per,
                         const int32_t *host_len, const int32_t *host_end, const sk_live_rule *rule, sk_map_rec *d_out,
                         sk_live_info *d_info, sk_live_best *d_best)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    int rc;
    // everything the push needs of its own is reserved before anything moves
    const size_t off_bytes = ((size_t)m + 1 + (size_t)sk_scan_blocks(m)) * sizeof(int64_t);
    if ((rc = sk_reserve(c, &z->off, off_bytes))) return rc;
    const int64_t rper = z->gated ? (int64_t)z->G + per : per;      // rows per entry the bridge reads: released, or staged
    if ((rc = sk_reserve(c, &z->values, (size_t)m * (size_t)((int64_t)(z->C - 1) + rper) * sizeof(double)))) return rc;
    int64_t *d_off = (int64_t *)z->off.p, *d_bsum = d_off + m + 1;
    double *d_values = (double *)z->values.p;
    if (z->gated) {
        if ((rc = sk_reserve(c, &z->hlen, (size_t)m * sizeof(int32_t)))) return rc;
        if ((rc = sk_reserve(c, &z->hrec, (size_t)m * sizeof(sk_hmms_rec)))) return rc;
        if ((rc = sk_reserve(c, &z->ginfo, (size_t)m * sizeof(sk_live_gate_info)))) return rc;
        if ((rc = sk_reserve(c, &z->rel, (size_t)m * (size_t)rper * sizeof(sk_det_event)))) return rc;
        if ((rc = sk_reserve(c, &z->roff, off_bytes))) return rc;
    }

    SK_HIP(hipEventRecord(c->ev[2], c->stream));            // sk_last_kernel_ms: main = the whole push, prep = the bridge
    if ((rc = sk_evs_session_push(c, z->evs, d_slots, m, d_rows, stride, d_len, d_end, per, nullptr, host_slots, host_len, host_end)))
        return rc;
    live_kargs a;
    a.state = (sk_live_info *)z->state.p; a.hold = (double *)z->hold.p; a.nslots = z->nslots; a.C = z->C;
    a.slots = d_slots; a.m = m; a.end = d_end; a.per = per; a.cnt = d_off; a.info = d_info;
    int32_t em = 0;
    if ((rc = sk_evs_session_last(c, z->evs, &a.eoff, &em))) return rc;
    int64_t eper = 0;
    if ((rc = sk_evs_session_staging(c, z->evs, &a.stage, &eper))) return rc;
    if (em != m || eper != per) return sk_fail(SK_ERR_INVALID, "internal: the event push left %d entries of %lld rows", em, (long long)eper);
    sk_gate_args g;
    if (z->gated) {
        // the HMM side: lengths masked by the gate's state and the slot's END (both as the push before left them: the
        // event push above touches neither), then k_hmms_push on the same rows
        g.state = (sk_gate_slot *)z->gstate.p; g.ring = (sk_det_event *)z->ring.p; g.live = (const sk_live_info *)z->state.p;
        g.nslots = z->nslots; g.G = z->G; g.slots = d_slots; g.m = m; g.len = d_len; g.end = d_end;
        g.hrec = (const sk_hmms_rec *)z->hrec.p; g.stage = a.stage; g.per = per; g.eoff = a.eoff;
        g.rel = (sk_det_event *)z->rel.p; g.rcnt = (int64_t *)z->roff.p; g.ginfo = (sk_live_gate_info *)z->ginfo.p;
        g.rule = z->rule;
        z->gate_timed = false;
        SK_HIP(hipEventRecord(z->ev_gate[0], c->stream));
        if ((rc = sk_livegate_lengths(c, g, (int32_t *)z->hlen.p))) return rc;
        // (the internal form makes none of sk_hmms_push_dev_i16's argument checks.  Its limit m * (stride + 64) <= 2^31
        // holds because check_evs_push (sk_api.hip) has put the SAME bound on the same m and stride before any live push
        // gets here: whoever loosens the event session's limit must check k_hmms_push's indexing, or bound it here.)
        if ((rc = sk_hmms_session_push_dev_i16(c, z->hmms, d_slots, m, d_rows, stride, (const int32_t *)z->hlen.p,
                                               (sk_hmms_rec *)z->hrec.p)))
            return rc;
        SK_HIP(hipEventRecord(z->ev_gate[1], c->stream));
    }
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    if (z->gated) {
        // the gate, then the bridge below on the released rows in place of the staged ones
        SK_HIP(hipEventRecord(z->ev_gate[2], c->stream));
        if ((rc = sk_livegate_release(c, g))) return rc;
        if ((rc = sk_launch_scan_i64(c, g.rcnt, m, g.rcnt + m + 1, g.rcnt))) return rc;
        SK_HIP(hipEventRecord(z->ev_gate[3], c->stream));
        z->gate_timed = true;
        a.stage = g.rel; a.per = rper; a.eoff = g.rcnt;
    }
    hipLaunchKernelGGL(k_live_count, dim3((unsigned)m), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    if ((rc = sk_launch_scan_i64(c, d_off, m, d_bsum, d_off))) return rc;
    hipLaunchKernelGGL(k_live_fill, dim3((unsigned)m), dim3(64), 0, c->stream, a, (const int64_t *)d_off, d_values);
    SK_HIP(hipGetLastError());
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    z->hoff.resize((size_t)m + 1);
    SK_HIP(hipMemcpyAsync(z->hoff.data(), d_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    z->last_m = m; z->pushed = true;
    if ((rc = sk_map_session_push(c, z->map, host_slots, m, d_values, z->hoff.data(), d_out))) return rc;
    int64_t launches = 2 + c->map_launches;
    z->best_timed = false;
    if (rule) {
        SK_HIP(hipEventRecord(z->ev_best[0], c->stream));
        hipLaunchKernelGGL(k_live_best, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream, (const sk_map_rec *)d_out, m, z->T,
                           *rule, d_best);
        SK_HIP(hipGetLastError());
        SK_HIP(hipEventRecord(z->ev_best[1], c->stream));
        z->best_timed = true;
        launches++;
    }
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    c->live_state_bytes = c->evs_state_bytes + c->map_state_bytes             // (both inner pushes have just set theirs)
                          + (int64_t)z->nslots * ((int64_t)z->C * 8 + (int64_t)sizeof(sk_live_info));
    if (z->gated) {                                         // + the HMM session, the rings and gate slots; lengths, HMM push, gate
        c->live_state_bytes += sk_hmms_session_bytes(c, z->hmms)
                               + (int64_t)z->nslots * ((int64_t)z->G * (int64_t)sizeof(sk_det_event) + (int64_t)sizeof(sk_gate_slot));
        launches += 3;
    }
    c->live_levels = z->hoff[(size_t)m];
    c->live_launches = launches;
    return SK_OK;
}

// the last push's off (device, [m + 1]) and compact values; m = 0 before the first push
int sk_live_session_last(sk_ctx *c, int32_t handle, const int64_t **d_off, const double **d_values, int32_t *m)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    *d_off = (const int64_t *)z->off.p;
    *d_values = (const double *)z->values.p;
    *m = z->pushed ? z->last_m : 0;
    return SK_OK;
}

// milliseconds of the last push's summary kernel (0 when it had no rule), from the session's own events
int sk_live_session_best_ms(sk_ctx *c, int32_t handle, float *ms)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    *ms = 0.f;
    if (!z->best_timed) return SK_OK;
    SK_HIP(hipEventSynchronize(z->ev_best[1]));
    SK_HIP(hipEventElapsedTime(ms, z->ev_best[0], z->ev_best[1]));
    return SK_OK;
}

// milliseconds of the last push's HMM side (lengths, k_hmms_push) and of its gate (k_live_gate, the scan), from the
// session's own events
int sk_live_session_gate_ms(sk_ctx *c, int32_t handle, float *hmm_ms, float *gate_ms)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (!z->gated) return sk_fail(SK_ERR_INVALID, "live session %d has no gate", handle);
    *hmm_ms = 0.f; *gate_ms = 0.f;
    if (!z->gate_timed) return SK_OK;
    SK_HIP(hipEventSynchronize(z->ev_gate[3]));
    SK_HIP(hipEventElapsedTime(hmm_ms, z->ev_gate[0], z->ev_gate[1]));
    SK_HIP(hipEventElapsedTime(gate_ms, z->ev_gate[2], z->ev_gate[3]));
    return SK_OK;
}

int sk_live_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const double *cal2)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (cal2 && !z->gated) return sk_fail(SK_ERR_INVALID, "live session %d has no gate: it takes no calibration pairs", handle);
    if (m <= 0) return SK_OK;
    int rc;
    if ((rc = sk_map_session_check_slots(c, z->map, slots, m))) return rc;   // (before either inner session moves)
    if ((rc = sk_evs_session_reset(c, z->evs, slots, m))) return rc;         // (waits for the stream)
    if ((rc = sk_map_session_reset(c, z->map, slots, m))) return rc;
    void *stage;                                            // the pairs (gated, given), then the slots
    const size_t cal_bytes = cal2 ? 2 * (size_t)m * sizeof(double) : 0;
    if ((rc = sk_live_session_stage(c, handle, 3, cal_bytes + (size_t)m * sizeof(int32_t), &stage))) return rc;
    double *d_cal2 = cal2 ? (double *)stage : nullptr;
    void *d_slots = (char *)stage + cal_bytes;
    SK_HIP(hipMemcpyAsync(d_slots, slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (z->gated) {
        if (cal2) SK_HIP(hipMemcpyAsync(d_cal2, cal2, cal_bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = sk_hmms_session_reset_dev(c, z->hmms, (const int32_t *)d_slots, m, d_cal2))) return rc;
        if ((rc = sk_livegate_reset(c, (sk_gate_slot *)z->gstate.p, z->nslots, (const int32_t *)d_slots, m))) return rc;
    }
    if ((rc = launch_reset(c, z, (const int32_t *)d_slots, m))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));               // (slots is the caller's memory)
    return SK_OK;
}

int sk_live_session_close(sk_ctx *c, int32_t handle)
{
    live_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipStreamSynchronize(c->stream));
    (void)sk_evs_session_close(c, z->evs);
    (void)sk_map_session_close(c, z->map);
    if (z->hmms >= 0) (void)sk_hmms_session_close(c, z->hmms);
    destroy(z);
    c->live_sessions[handle] = nullptr;
    return SK_OK;
}

// (the inner sessions go with their own tables, right after this)
void sk_live_close_all(sk_ctx *c)
{
    for (int i = 0; i < SK_LIVE_MAX_SESSIONS; i++)
        if (c->live_sessions[i]) { destroy((live_session *)c->live_sessions[i]); c->live_sessions[i] = nullptr; }
}
