// sk_mapstream.hip -- mapping sessions: the pair-list DTW continued as a query's points arrive (gfx950).
//
// A session keeps `nslots` queries in progress against `ntargets` targets that stay on the device.  Per (slot, target) it
// keeps the LAST ROW of the DTW matrix of the rows swept so far -- D (f64) and the back-trace start S (i32) per target
// column, 12 bytes a column -- and the last record.  A push appends a chunk of points to every named slot: the chunk's
// rows are swept over every target by k_sdtw's MODE_PAIRS_CHAIN (sk_sdtw.hip), entering where the stored row left off
// (MODE_CHAIN's row hand-over, decided per lane group) or, for a slot's first points, under the virtual row -1
// (MODE_PAIRS).  Every cell is one correctly rounded add of correctly rounded operands and the tie order of the start
// propagation is a per-cell rule, so the rows are those of the one-shot sweep over the concatenation, bit for bit; the
// record is the first argmin of the current last row, which the sweep's last lane keeps anyway -- no running best is
// carried from push to push.
//
// The plan of a push is sk_pairs_run's: a chunk (cut into pieces of 1 024 rows where it is longer: launch_chained's
// loop) is laid out per lane ONCE, by k_pairs_layout, and shared by its T targets; a piece's (L, R) is sk_exact_shape's
// for the push's entry count; the entries of one piece index are grouped by (L, R), ordered inside a group by target
// length (longest first) and swept with one launch per group; piece index p + 1 follows p on the same stream.  The row
// state is rewritten in place (why that is safe: the head of sk_sdtw.hip).
//
// Where the counters live: the plan needs every slot's "fresh or continuing" on the host, so rows and pushes per slot
// are host-side members of the session and a reset is bookkeeping alone -- there is no reset kernel; the stored row of a
// reset slot is simply never read again (its next entry is fresh).  k_map_emit gathers the records of a push -- the stored
// last record of (slot, target), or the empty record for a slot without points -- which is also what a peek returns.
#include "sk_sdtw_dev.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int MAP_PIECE = 64 * 16;  // rows a wavefront keeps in registers

struct map_work {                   // one per entry of a push: what the emit writes beside the stored record
    int32_t slot, rows, pushes, pad;
};

__global__ void k_map_emit(const map_work *__restrict__ work, int m, int T, const sk_hit *__restrict__ last,
                           const int32_t *__restrict__ tlen, sk_map_rec *__restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * T) return;
    const int t = idx / m, i = idx % m;
    const map_work w = work[i];
    sk_map_rec r;
    r.dist = __builtin_nan(""); r.start = -1; r.end = -1; r.n = tlen[t]; r.flags = 0;
    r.rows = w.rows; r.pushes = w.pushes;
    if (w.rows > 0) {
        const sk_hit h = last[(int64_t)w.slot * T + t];
        r.dist = h.dist; r.start = h.start; r.end = h.end; r.n = h.n; r.flags = h.flags;
    }
    out[idx] = r;
}

struct map_session {
    int32_t nslots = 0, T = 0;
    int64_t sumM = 0;
    std::vector<int64_t> toff;              // [T + 1]
    std::vector<int32_t> rows, pushes;      // per slot, since its reset
    sk_buf targets, tlen, stD, stS, last;   // the pool, the lengths, the row state [nslots][sumM], sk_hit [nslots][T]
    // per push
    sk_buf plan;                            // layouts, then the entry table, the query table, the work table
    std::vector<sk_map_entry>  table;       // (kept alive for the async H2D)
    std::vector<sk_pair_query> query;
    std::vector<map_work>      work;
    sk_buf host[2];                         // the host entry point's staging (values, records)
};

void free_buf(sk_buf *b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

void destroy(map_session *z)
{
    sk_buf *bufs[] = {&z->targets, &z->tlen, &z->stD, &z->stS, &z->last, &z->plan, &z->host[0], &z->host[1]};
    for (sk_buf *b : bufs) free_buf(b);
    delete z;
}

map_session *session_of(sk_ctx *c, int32_t handle)
{
    if (handle < 0 || handle >= SK_MAP_MAX_SESSIONS || !c->map_sessions[handle]) {
        sk_fail(SK_ERR_INVALID, "unknown mapping session handle %d", handle);
        return nullptr;
    }
    return (map_session *)c->map_sessions[handle];
}

} // namespace

int sk_map_session_open(sk_ctx *c, const double *targets, const int64_t *target_off, int32_t ntargets, int32_t nslots,
                        int32_t *handle)
{
    int h = -1;
    for (int i = 0; i < SK_MAP_MAX_SESSIONS; i++) if (!c->map_sessions[i]) { h = i; break; }
    if (h < 0) return sk_fail(SK_ERR_INVALID, "%d mapping sessions are open on this context already", SK_MAP_MAX_SESSIONS);
    map_session *z = new map_session();
    z->nslots = nslots; z->T = ntargets;
    z->toff.resize((size_t)ntargets + 1);
    std::vector<int32_t> tlen((size_t)ntargets);
    for (int32_t t = 0; t <= ntargets; t++) z->toff[(size_t)t] = target_off[t] - target_off[0];
    for (int32_t t = 0; t < ntargets; t++) tlen[(size_t)t] = (int32_t)(target_off[t + 1] - target_off[t]);
    z->sumM = z->toff[(size_t)ntargets];
    z->rows.assign((size_t)nslots, 0);
    z->pushes.assign((size_t)nslots, 0);
    const size_t cols = (size_t)nslots * (size_t)z->sumM;
    int rc = sk_reserve(c, &z->targets, (size_t)z->sumM * sizeof(double));
    if (!rc) rc = sk_reserve(c, &z->tlen, (size_t)ntargets * sizeof(int32_t));
    if (!rc) rc = sk_reserve(c, &z->stD, cols * sizeof(double));
    if (!rc) rc = sk_reserve(c, &z->stS, cols * sizeof(int32_t));
    if (!rc) rc = sk_reserve(c, &z->last, (size_t)nslots * (size_t)ntargets * sizeof(sk_hit));
    if (!rc && hipMemcpy(z->targets.p, targets + target_off[0], (size_t)z->sumM * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = sk_fail(SK_ERR_HIP, "uploading the targets failed");
    if (!rc && hipMemcpy(z->tlen.p, tlen.data(), tlen.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        rc = sk_fail(SK_ERR_HIP, "uploading the target lengths failed");
    if (rc) { destroy(z); return rc; }
    c->map_sessions[h] = z;
    *handle = h;
    return SK_OK;
}

int sk_map_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *ntargets)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (nslots) *nslots = z->nslots;
    if (ntargets) *ntargets = z->T;
    return SK_OK;
}

int sk_map_session_check_slots(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    std::vector<uint8_t> seen((size_t)z->nslots, 0);
    for (int32_t i = 0; i < m; i++) {
        if (slots[i] < 0 || slots[i] >= z->nslots)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, slots[i], z->nslots);
        if (seen[(size_t)slots[i]]) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d appears twice in one call", i, slots[i]);
        seen[(size_t)slots[i]] = 1;
    }
    return SK_OK;
}

int sk_map_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (which < 0 || which >= 2) return sk_fail(SK_ERR_INVALID, "internal: staging buffer %d", which);
    const int rc = sk_reserve(c, &z->host[which], bytes ? bytes : 1);
    if (rc) return rc;
    *p = z->host[which].p;
    return SK_OK;
}

int sk_map_session_push(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const double *d_values,
                        const int64_t *off, sk_map_rec *d_out)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    int rc;
    if ((rc = sk_map_session_check_slots(c, handle, slots, m))) return rc;
    const int T = z->T;
    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier push may still read the old plan

    // ---- pieces: every chunk cut into runs of at most 1 024 rows, laid out once each -------------------------------------
    int64_t live = 0, npieces_max = 0;
    for (int32_t i = 0; i < m; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len > 0) { live++; npieces_max = std::max(npieces_max, (len + MAP_PIECE - 1) / MAP_PIECE); }
    }
    const int64_t count = live * T;                        // entries of a piece index at most: what sk_exact_shape sizes for
    z->query.clear();
    z->table.clear();
    z->work.resize((size_t)m);
    struct run { int64_t first, count; int L, R; };
    std::vector<run> runs;
    std::vector<int32_t> order;
    int64_t nlay = 0;
    for (int64_t p = 0; p < npieces_max; p++) {
        // the chunks that have a piece p: its shape, its layout's place
        std::vector<int32_t> chunk_of, key_of, n_of;
        std::vector<int64_t> xoff_of;
        int64_t cnt[32] = {0};
        for (int32_t i = 0; i < m; i++) {
            const int64_t len = off[i + 1] - off[i];
            if (len <= p * MAP_PIECE) continue;
            const int N = (int)std::min<int64_t>(MAP_PIECE, len - p * MAP_PIECE);
            int L, R;
            sk_exact_shape(N, count, &L, &R);
            sk_pair_query q;
            q.src = off[i] - off[0] + p * MAP_PIECE; q.xoff = nlay; q.N = N; q.L = L; q.R = R; q.pad = 0;
            z->query.push_back(q);
            chunk_of.push_back(i);
            n_of.push_back(N);
            key_of.push_back((L == 64 ? 16 : 0) + R - 1);
            xoff_of.push_back(nlay);
            nlay += (int64_t)L * R;
            cnt[key_of.back()] += T;
        }
        // the entries of piece index p: (L, R) group after group, longest target first
        for (int g = 0; g < 32; g++) {
            if (!cnt[g]) continue;
            const int L = g >= 16 ? 64 : 16, R = (g & 15) + 1;
            order.clear();
            for (size_t k = 0; k < chunk_of.size(); k++)
                if (key_of[k] == g) for (int t = 0; t < T; t++) order.push_back((int32_t)(k * (size_t)T + (size_t)t));
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
                const int ta = a % T, tb = b % T;
                return z->toff[(size_t)ta + 1] - z->toff[(size_t)ta] > z->toff[(size_t)tb + 1] - z->toff[(size_t)tb];
            });
            run r;
            r.first = (int64_t)z->table.size(); r.count = (int64_t)order.size(); r.L = L; r.R = R;
            runs.push_back(r);
            for (int32_t o : order) {
                const size_t k = (size_t)(o / T);
                const int t = o % T, i = chunk_of[k], s = slots[i];
                sk_map_entry e;
                e.toff = z->toff[(size_t)t]; e.xoff = xoff_of[k];
                e.soff = (int64_t)s * z->sumM + z->toff[(size_t)t];
                e.n = (int32_t)(z->toff[(size_t)t + 1] - z->toff[(size_t)t]);
                e.P = L * R - n_of[k];
                e.rec = s * T + t;
                e.cont = (p > 0 || z->rows[(size_t)s] > 0) ? 1 : 0;
                z->table.push_back(e);
            }
        }
    }
    // ---- the counters of the slots named, as the records will state them -------------------------------------------------
    for (int32_t i = 0; i < m; i++) {
        const int64_t len = off[i + 1] - off[i];
        const int32_t s = slots[i];
        map_work w;
        w.slot = s; w.rows = z->rows[(size_t)s] + (int32_t)len; w.pushes = z->pushes[(size_t)s] + (len > 0 ? 1 : 0); w.pad = 0;
        if ((int64_t)z->rows[(size_t)s] + len > 0x7fffff00)
            return sk_fail(SK_ERR_UNSUPPORTED, "entry %d: slot %d would hold more than 2147483392 points", i, s);
        z->work[(size_t)i] = w;
    }
    // ---- upload, lay out, sweep, emit ---------------------------------------------------------------------------------------
    const size_t nq = z->query.size(), ne = z->table.size();
    const size_t b_lay = (size_t)nlay * sizeof(double), b_tab = ne * sizeof(sk_map_entry), b_q = nq * sizeof(sk_pair_query);
    if ((rc = sk_reserve(c, &z->plan, b_lay + b_tab + b_q + (size_t)m * sizeof(map_work) + 16))) return rc;
    double *d_lay = (double *)z->plan.p;
    sk_map_entry *d_mp = (sk_map_entry *)((char *)z->plan.p + b_lay);
    sk_pair_query *d_qt = (sk_pair_query *)((char *)d_mp + b_tab);
    map_work *d_work = (map_work *)((char *)d_qt + b_q);
    if (ne) SK_HIP(hipMemcpyAsync(d_mp, z->table.data(), b_tab, hipMemcpyHostToDevice, c->stream));
    if (nq) SK_HIP(hipMemcpyAsync(d_qt, z->query.data(), b_q, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_work, z->work.data(), (size_t)m * sizeof(map_work), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_launch_pairs_layout(c, d_values, d_qt, (int)nq, d_lay))) return rc;
    for (const run &r : runs)
        if ((rc = sk_launch_sdtw_map(c, r.L, r.R, (const double *)z->targets.p, d_lay, d_mp + r.first, (int32_t)r.count,
                                     (double *)z->stD.p, (int32_t *)z->stS.p, (sk_hit *)z->last.p)))
            return rc;
    const int64_t recs = (int64_t)m * T;
    hipLaunchKernelGGL(k_map_emit, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, c->stream, (const map_work *)d_work, m, T,
                       (const sk_hit *)z->last.p, (const int32_t *)z->tlen.p, d_out);
    SK_HIP(hipGetLastError());
    // everything is enqueued: the slots have their points
    for (int32_t i = 0; i < m; i++) {
        z->rows[(size_t)slots[i]] = z->work[(size_t)i].rows;
        z->pushes[(size_t)slots[i]] = z->work[(size_t)i].pushes;
    }
    c->map_state_bytes = (int64_t)z->nslots * z->sumM * 12;
    c->map_entries = (int64_t)ne;
    c->map_launches = (int64_t)runs.size();
    return SK_OK;
}

int sk_map_session_reset(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    if (int rc = sk_map_session_check_slots(c, handle, slots, m)) return rc;
    for (int32_t i = 0; i < m; i++) { z->rows[(size_t)slots[i]] = 0; z->pushes[(size_t)slots[i]] = 0; }
    return SK_OK;
}

// Hit lists from the stored rows (sk_pairhits.hip): one table entry per (target, named slot), list index t * m + i, the
// row where the pushes left it.  A slot without points has no row: count 0, the empty record of k_map_emit in every
// place.  Reads the row state and writes the caller's buffers only.
int sk_map_session_hits(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, int32_t K, double max_dist, sk_hit *d_out,
                        int32_t *d_count)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    int rc;
    if ((rc = sk_map_session_check_slots(c, handle, slots, m))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier call may still read the old table
    const int64_t nrows = (int64_t)z->T * m;
    c->rowhit_table.resize((size_t)nrows);
    for (int32_t t = 0; t < z->T; t++)
        for (int32_t i = 0; i < m; i++) {
            const int32_t s = slots[i];
            sk_rowhit_entry e;
            e.col0 = (int64_t)s * z->sumM + z->toff[(size_t)t];
            e.list = (int64_t)t * m + i;
            e.n = (int32_t)(z->toff[(size_t)t + 1] - z->toff[(size_t)t]);
            e.flags = z->rows[(size_t)s] > 0 ? 0 : SK_ROWHIT_NOROW;
            c->rowhit_table[(size_t)e.list] = e;
        }
    if ((rc = sk_rowhits_reserve(c, nrows))) return rc;
    c->pairhits_long_rows = 0;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // sk_last_kernel_ms: no prep, main = the table's copy + the select
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if ((rc = sk_launch_rowhits(c, c->rowhit_table.data(), 0, (int32_t)nrows, (const double *)z->stD.p, (const int32_t *)z->stS.p,
                                K, max_dist, d_out, d_count, &c->pairhits_long_rows))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    c->pairhits_row_bytes = (int64_t)m * z->sumM * 12;
    c->pairhits_slices = 1;
    return SK_OK;
}

int sk_map_session_close(sk_ctx *c, int32_t handle)
{
    map_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipStreamSynchronize(c->stream));
    destroy(z);
    c->map_sessions[handle] = nullptr;
    return SK_OK;
}

void sk_map_close_all(sk_ctx *c)
{
    for (int i = 0; i < SK_MAP_MAX_SESSIONS; i++)
        if (c->map_sessions[i]) { destroy((map_session *)c->map_sessions[i]); c->map_sessions[i] = nullptr; }
}
