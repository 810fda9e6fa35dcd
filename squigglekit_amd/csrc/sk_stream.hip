// sk_stream.hip -- MotifSeq sessions: subsequence DTW continued chunk by chunk (gfx950).
//
// A session keeps, per slot (one read in progress) and motif, the LAST COLUMN of the DTW matrix: D[N] (f64) and the
// back-trace starts S[N] (i32), plus the running first minimum of the last row (best, bestS, bestJ).  That is all the
// recurrence of sk_sdtw.hip needs to go on: every cell is one correctly rounded add of correctly rounded operands, so a
// sweep that enters at column j0 with that state computes bit for bit the cells the one-shot sweep computes there.
//
// k_stream_sweep is the systolic layout of k_sdtw (L lanes per slot, R rows per lane, sample and the neighbour's bottom
// row by DPP, FP64 add / sub / min / select, the tie order of its FULL mode); new is entering and leaving a column range:
//   * entering: lane l reaches column j0 at step l.  Its cells' left neighbours are its own saved state; the diagonal
//     neighbour of its top row is the saved bottom row of lane l - 1, read from memory before anything is stored.  Lane
//     0's row above is the virtual row -1, (D = 0, S = j + 1) in the read's kept coordinates.  At j0 == 0 there is no
//     state: D = +inf, S = -1, which leaves column 0 its "up" neighbour only.
//   * leaving: a lane computes only while its column lies inside the range (step - l in [0, cols)); outside it the
//     lane's cells, bottom row and diagonal stay untouched -- the shifts still run in every lane, they carry the
//     samples.  After the skewed drain every lane stands on the range's last column and the state is stored unskewed.
//   * four slots share a wavefront at L = 16 and run in lockstep over ranges of different lengths, empty ones included.
// The columns of one sweep come from two places: the calibration buffer (a slot whose calibration ends in this push
// sweeps what it buffered) and then the chunk.
//
// Per push: k_stream_ingest (filter + compaction of the chunk, calibration buffer, counters), sk_launch_prep_i16 over
// the buffered rows of the slots whose calibration ends (the statistics of the one-shot path, unchanged),
// k_stream_adopt (their center / scale), one k_stream_sweep per motif, k_stream_emit (the records).  One stream.
//
// Host side shared with the one-shot path: a motif's (L, R) is sk_exact_shape's for nslots reads and its per-lane layout
// is sk_lane_layout's, so a session's lanes hold the rows the one-shot sweep's lanes hold.  The sweep itself stays a
// kernel of its own ("One text per thing").
#include "sk_sdtw_dev.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

enum { ST_CALIBRATING = 0, ST_SEARCHING = 1, ST_DEAD = 2 };

struct stream_slot {                // 40 bytes per slot
    int32_t n, seen, chunks, flags; // kept / pushed samples, pushes of len > 0, SK_FLAG_* (EMPTY is added by the emit)
    int32_t state, flushed;         // flushed: 1 after a flush, 2 where that flush ended the calibration on a MAD of 0
    double  center, scale;
};
struct stream_work {                // one per entry of a push: what its sweeps cover
    int32_t slot;                   // -1: skipped (out of range)
    int32_t lenA;                   // columns from the calibration buffer, [0, lenA)
    int32_t skipB, lenB;            // then the chunk's kept samples [skipB, skipB + lenB)
};
struct stream_best {                // running first minimum of the last row
    double  best;
    int32_t bestS, bestJ;
};
struct stream_motif_dev {           // where the emit finds motif k's state
    const double      *D;
    const stream_best *best;
    int32_t            L, R;
};

struct stream_kargs {
    const stream_slot *slots;
    const stream_work *work;
    int                m;
    const int16_t     *cal;         // [nslots][wpad]
    int64_t            wpad;
    const int16_t     *comp;        // [m][cstride]: the chunks' kept samples
    int64_t            cstride;
    const double      *xlay;        // the motif laid out per lane [L][R] (sk_sdtw.hip's layout: the first P lanes are short)
    int                P;
    double            *D;           // [nslots][R][L]
    int32_t           *S;
    stream_best       *best;        // [nslots]
};

__global__ void k_stream_reset(stream_slot *slots, int nslots, const int32_t *list, int m, const double *center,
                               const double *scale)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int s = list ? list[i] : i;
    if (s < 0 || s >= nslots) return;
    stream_slot st;
    st.n = 0; st.seen = 0; st.chunks = 0; st.flushed = 0;
    if (center) { st.state = ST_SEARCHING; st.flags = 0; st.center = center[i]; st.scale = scale[i]; }
    else { st.state = ST_CALIBRATING; st.flags = SK_FLAG_CALIBRATING; st.center = __builtin_nan(""); st.scale = __builtin_nan(""); }
    slots[s] = st;
}

// One workgroup per entry: the chunk's kept samples (lo < x < hi) to comp row i, the slot's counters, and for a
// calibrating slot its buffer; a slot whose calibration ends here also gets its buffered row copied to stage row i (the
// input of the statistics) with statlen[i] = its length -- every other entry has statlen 0.
__global__ __launch_bounds__(256)
void k_stream_ingest(stream_slot *slots, int nslots, const int32_t *d_slots, int m, const int16_t *rows, int64_t stride,
                     const int32_t *d_len, int lo, int hi, int W, int64_t wpad, int flush, int16_t *cal, int16_t *comp,
                     int64_t cstride, int16_t *stage, int32_t *statlen, stream_work *work)
{
    __shared__ int wsum[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = d_slots[i];
    if (s < 0 || s >= nslots) {
        if (tid == 0) { stream_work wk; wk.slot = -1; wk.lenA = 0; wk.skipB = 0; wk.lenB = 0; work[i] = wk; statlen[i] = 0; }
        return;
    }
    int len = 0;
    if (rows) { len = d_len[i]; if (len < 0) len = 0; if ((int64_t)len > stride) len = (int)stride; }
    const int16_t *row = rows + (int64_t)i * stride;
    int16_t *crow = comp + (int64_t)i * cstride;
    int run = 0;
    for (int base = 0; base < len; base += 256) {
        const int idx = base + tid;
        const int x = (idx < len) ? (int)row[idx] : 0;
        const bool keep = idx < len && x > lo && x < hi;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) { const int v = wsum[q]; if (q < w) wbase += v; tot += v; }
        if (keep) crow[run + wbase + __popcll(b & ((1ull << lane) - 1ull))] = (int16_t)x;
        run += tot;
        __syncthreads();
    }
    const int mk = run;
    const stream_slot st0 = slots[s];
    __syncthreads();                                        // comp row complete; everybody has read the slot
    stream_slot st = st0;
    stream_work wk;
    wk.slot = s; wk.lenA = 0; wk.skipB = 0; wk.lenB = 0;
    int slen = 0;
    st.seen += len;
    if (len > 0) st.chunks += 1;
    st.n += mk;
    if (flush) st.flushed = 1;
    if (st0.state == ST_CALIBRATING) {
        int app = W - st0.n;                                // st0.n < W while calibrating
        if (app > mk) app = mk;
        int16_t *crow_cal = cal + (int64_t)s * wpad;
        for (int t = tid; t < app; t += 256) crow_cal[st0.n + t] = crow[t];
        if (st.n >= W || (flush && st.n >= 1)) {            // calibration ends: statistics over the first min(n, W)
            slen = st.n < W ? st.n : W;
            wk.lenA = slen; wk.skipB = app; wk.lenB = mk - app;
            __syncthreads();
            int16_t *srow = stage + (int64_t)i * wpad;
            for (int t = tid; t < slen; t += 256) srow[t] = crow_cal[t];
        } else if (flush) {                                 // flushed with nothing: no statistics, ever
            st.state = ST_DEAD; st.flags = SK_FLAG_EMPTY;
        }
    } else if (st0.state == ST_SEARCHING) {
        wk.lenB = mk;
    }
    if (tid == 0) { slots[s] = st; work[i] = wk; statlen[i] = slen; }
}

// the statistics of the slots whose calibration ended in this push: center / scale become the slot's for good
__global__ void k_stream_adopt(stream_slot *slots, stream_work *work, const int32_t *statlen, const sk_prep *prep, int m)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || statlen[i] <= 0) return;
    stream_work wk = work[i];
    const sk_prep pr = prep[i];
    stream_slot st = slots[wk.slot];
    st.center = pr.center; st.scale = pr.scale;
    if (pr.flags & SK_FLAG_DEGENERATE) {
        st.state = ST_DEAD; st.flags = SK_FLAG_DEGENERATE;
        if (st.flushed) st.flushed = 2;                     // a flush ended this calibration: the one-shot record (emit)
        wk.lenA = 0; wk.lenB = 0;
        work[i] = wk;
    } else {
        st.state = ST_SEARCHING; st.flags = 0;
    }
    slots[wk.slot] = st;
}

template <int L, int R>
__global__ __launch_bounds__(256)
void k_stream_sweep(const stream_kargs a)
{
    static_assert(L == 16 || L == 64, "lanes per slot");
    constexpr int G = 64 / L;
    constexpr int SHR = (L == 16) ? DPP_ROW_SHR1 : DPP_WAVE_SHR1;
    constexpr int ROL = (L == 16) ? DPP_ROW_ROL1 : DPP_WAVE_ROL1;
    const double INF = __builtin_huge_val();

    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int g = lane / L, l = lane % L;
    const int i = wave * G + g;

    // ---- this group's column range -----------------------------------------------------------------------------
    int s = 0, lenA = 0, skipB = 0, cols = 0, j0 = 0;
    double center = 0.0, scale = 1.0;
    if (i < a.m) {
        const stream_work wk = a.work[i];
        if (wk.slot >= 0 && wk.lenA + wk.lenB > 0) {
            s = wk.slot; lenA = wk.lenA; skipB = wk.skipB; cols = wk.lenA + wk.lenB;
            const stream_slot st = a.slots[s];
            center = st.center; scale = st.scale;
            j0 = st.n - cols;                               // columns swept before: the ingest has counted this push in
        }
    }
    const bool has = cols > 0;
    int nsteps = has ? cols + L - 1 : 0;                    // wave-uniform step count
#pragma unroll
    for (int d = L; d < 64; d <<= 1) nsteps = max(nsteps, __shfl_xor(nsteps, d));
    nsteps = __builtin_amdgcn_readfirstlane(nsteps);
    if (nsteps == 0) return;
    const int nblk = (nsteps + L - 1) / L;

    // ---- motif rows and the saved column ---------------------------------------------------------------------------
    double x[R];
#pragma unroll
    for (int k = 0; k < R; k++) x[k] = a.xlay[l * R + k];
    const bool shortlane = l < a.P;
    const bool resume = has && j0 > 0;
    const int64_t sbase = (int64_t)s * R * L;
    double D[R];
    int    S[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        D[k] = resume ? a.D[sbase + k * L + l] : INF;
        S[k] = resume ? a.S[sbase + k * L + l] : -1;
    }
    // (i - 1, j0 - 1) of my top row: lane l - 1's saved bottom row -- or the virtual row -1, which lane 0 has above it
    // and which the row-less lanes of a short motif (R == 1, N < L) hand on: (D = 0, S = column + 1)
    double diagD = INF;
    int    diagS = -1;
    if (l == 0 || (R == 1 && l - 1 < a.P)) { diagD = 0.0; diagS = j0; }
    else if (resume) {
        const int kb = (R >= 2 && l - 1 < a.P) ? R - 2 : R - 1;
        diagD = a.D[sbase + kb * L + l - 1];
        diagS = a.S[sbase + kb * L + l - 1];
    }
    double best = INF;  int bestS = -1, bestJ = -1;
    if (resume) { const stream_best b = a.best[s]; best = b.best; bestS = b.bestS; bestJ = b.bestJ; }
    double botD = INF;  int botS = -1;                      // (taken by lane l + 1 only after I have set them)
    double y = 0.0;

    const int16_t *calrow = a.cal + (int64_t)s * a.wpad;
    const int16_t *chunk = a.comp + (int64_t)(has ? i : 0) * a.cstride + skipB - lenA;   // column c >= lenA: chunk[c]
    auto fetch = [&](int c) -> double {                     // normalised sample of column j0 + c (anything finite outside)
        int16_t raw = 0;
        if (c < lenA) raw = calrow[c];
        else if (c < cols) raw = chunk[c];
        return ((double)raw - center) / scale;
    };

    double F = fetch(l);
    for (int blk = 0; blk < nblk; blk++) {
        const double Fnext = fetch((blk + 1) * L + l);      // in flight during the L steps below
#pragma unroll 2
        for (int q = 0; q < L; q++) {
            const int t = blk * L + q;
            // ---- systolic shift, in every lane: sample and lane l - 1's bottom row arrive -------------------------
            y = dpp_f64<SHR>(F, y);
            F = dpp_f64<ROL>(F, F);
            const double upD = dpp_f64<SHR>(0.0, botD);     // lane 0: virtual row -1 at column j0 + t
            const int    upS = dpp_i32<SHR>(j0 + t + 1, botS);
            const int c = t - l;                            // my column inside the range
            if ((unsigned)c < (unsigned)cols) {
                double dgD = diagD;  int dgS = diagS;       // (i-1, j-1)
                double uD = upD;     int uS = upS;          // (i-1, j)
#pragma unroll
                for (int k = 0; k < R; k++) {
                    const double lfD = D[k];                // (i, j-1)
                    const int    lfS = S[k];
                    const double cost = fabs(x[k] - y);
                    const bool lt1 = lfD < dgD;             // diag wins ties over left
                    const double m1 = vmin(lfD, dgD);
                    const int    s1 = lt1 ? lfS : dgS;
                    const bool lt2 = uD < m1;               // up only if strictly smaller
                    const double mm = vmin(uD, m1);
                    const int    sv = lt2 ? uS : s1;
                    const double nd = cost + mm;
                    dgS = lfS;  S[k] = sv;  uS = sv;
                    dgD = lfD;  D[k] = nd;  uD = nd;
                }
                diagD = upD;  diagS = upS;
                if constexpr (R >= 2) {
                    botD = shortlane ? D[R - 2] : D[R - 1];
                    botS = shortlane ? S[R - 2] : S[R - 1];
                } else {
                    botD = shortlane ? upD : D[0];          // a lane with no rows just forwards
                    botS = shortlane ? upS : S[0];
                }
                if (D[R - 1] < best) { best = D[R - 1]; bestS = S[R - 1]; bestJ = j0 + c; }   // (meaningful in lane L-1)
            }
        }
        F = Fnext;
    }

    if (has) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            a.D[sbase + k * L + l] = D[k];
            a.S[sbase + k * L + l] = S[k];
        }
        if (l == L - 1) { stream_best b; b.best = best; b.bestS = bestS; b.bestJ = bestJ; a.best[s] = b; }
    }
}

__global__ void k_stream_emit(const stream_slot *slots, const stream_work *work, int m, const stream_motif_dev *mot, int K,
                              sk_stream_rec *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * K) return;
    const int k = idx / m, i = idx % m;
    sk_stream_rec r;
    r.dist = __builtin_nan(""); r.tail = __builtin_nan(""); r.start = -1; r.end = -1;
    r.n = 0; r.seen = 0; r.flags = 0; r.chunks = 0;
    const int s = work[i].slot;
    if (s >= 0) {
        const stream_slot st = slots[s];
        r.n = st.n; r.seen = st.seen; r.chunks = st.chunks;
        r.flags = st.flags | ((st.flushed && st.n == 0) ? SK_FLAG_EMPTY : 0);
        // a read that was flushed before it had W kept samples has the record of the one-shot call on the whole read,
        // field for field: where its MAD is 0 that kernel's running minimum never left +inf (every cell is NaN)
        if (st.flushed == 2) r.dist = __builtin_huge_val();
        if (st.state == ST_SEARCHING && st.n > 0) {
            const stream_motif_dev md = mot[k];
            const stream_best b = md.best[s];
            r.dist = b.best; r.start = b.bestS; r.end = b.bestJ;
            r.tail = md.D[(int64_t)s * md.R * md.L + (md.R - 1) * md.L + md.L - 1];   // row N-1: last slot of the last lane
        }
    }
    out[(int64_t)k * m + i] = r;
}

typedef void (*sweep_fn)(const stream_kargs);

template <int L>
sweep_fn pick_sweep_r(int R)
{
#define SK_KERNEL(RR) k_stream_sweep<L, RR>
    switch (R) { SK_R_CASES_1_16(SK_KERNEL) }
#undef SK_KERNEL
    return nullptr;
}

struct stream_motif {
    int N = 0, L = 0, R = 0, P = 0;
    sweep_fn fn = nullptr;
    sk_buf xlay, D, S, best;
};

struct stream_session {
    sk_stream_params p;
    int64_t wpad = 0;
    std::vector<stream_motif> motifs;
    sk_buf slots, cal, table;
    // per call
    sk_buf work, statlen, comp, stage, stage2, prep;
    sk_buf host[4];                 // the host entry points' staging (slots, rows, len / center + scale, records)
};

void free_buf(sk_buf *b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

void destroy(stream_session *z)
{
    for (stream_motif &mo : z->motifs) { free_buf(&mo.xlay); free_buf(&mo.D); free_buf(&mo.S); free_buf(&mo.best); }
    sk_buf *bufs[] = {&z->slots, &z->cal, &z->table, &z->work, &z->statlen, &z->comp, &z->stage, &z->stage2, &z->prep,
                      &z->host[0], &z->host[1], &z->host[2], &z->host[3]};
    for (sk_buf *b : bufs) free_buf(b);
    delete z;
}

stream_session *session_of(sk_ctx *c, int32_t handle)
{
    if (handle < 0 || handle >= SK_STREAM_MAX_SESSIONS || !c->sessions[handle]) {
        sk_fail(SK_ERR_INVALID, "unknown session handle %d", handle);
        return nullptr;
    }
    return (stream_session *)c->sessions[handle];
}

} // namespace

int sk_stream_session_open(sk_ctx *c, const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                           const sk_stream_params *p, int32_t *handle)
{
    int h = -1;
    for (int i = 0; i < SK_STREAM_MAX_SESSIONS; i++) if (!c->sessions[i]) { h = i; break; }
    if (h < 0) return sk_fail(SK_ERR_INVALID, "%d sessions are open on this context already", SK_STREAM_MAX_SESSIONS);
    stream_session *z = new stream_session();
    z->p = *p;
    z->wpad = ((int64_t)p->calib + 7) & ~(int64_t)7;
    z->motifs.resize((size_t)nmotifs);
    int rc = SK_OK;
    std::vector<stream_motif_dev> table((size_t)nmotifs);
    std::vector<double> lay;
    for (int32_t k = 0; k < nmotifs && !rc; k++) {
        stream_motif &mo = z->motifs[(size_t)k];
        const double *x = motifs + motif_off[k];
        mo.N = motif_off[k + 1] - motif_off[k];
        sk_exact_shape(mo.N, p->nslots, &mo.L, &mo.R);     // the one-shot call's shape for nslots reads
        mo.P = mo.L * mo.R - mo.N;
        mo.fn = (mo.L == 16) ? pick_sweep_r<16>(mo.R) : pick_sweep_r<64>(mo.R);
        if (!mo.fn) { rc = sk_fail(SK_ERR_UNSUPPORTED, "no session kernel for L=%d R=%d", mo.L, mo.R); break; }
        lay.resize((size_t)mo.L * mo.R);
        if (!sk_lane_layout(x, mo.N, mo.L, mo.R, lay.data())) { rc = sk_fail(SK_ERR_INVALID, "internal: motif layout mismatch"); break; }
        const size_t cells = (size_t)p->nslots * (size_t)mo.L * (size_t)mo.R;
        if ((rc = sk_reserve(c, &mo.xlay, lay.size() * sizeof(double)))) break;
        if ((rc = sk_reserve(c, &mo.D, cells * sizeof(double)))) break;
        if ((rc = sk_reserve(c, &mo.S, cells * sizeof(int32_t)))) break;
        if ((rc = sk_reserve(c, &mo.best, (size_t)p->nslots * sizeof(stream_best)))) break;
        if (hipMemcpy(mo.xlay.p, lay.data(), lay.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            rc = sk_fail(SK_ERR_HIP, "uploading a motif failed");
            break;
        }
        table[(size_t)k].D = (const double *)mo.D.p; table[(size_t)k].best = (const stream_best *)mo.best.p;
        table[(size_t)k].L = mo.L; table[(size_t)k].R = mo.R;
    }
    if (!rc) rc = sk_reserve(c, &z->slots, (size_t)p->nslots * sizeof(stream_slot));
    if (!rc) rc = sk_reserve(c, &z->cal, (size_t)p->nslots * (size_t)z->wpad * sizeof(int16_t));
    if (!rc) rc = sk_reserve(c, &z->table, table.size() * sizeof(stream_motif_dev));
    if (!rc && hipMemcpy(z->table.p, table.data(), table.size() * sizeof(stream_motif_dev), hipMemcpyHostToDevice) != hipSuccess)
        rc = sk_fail(SK_ERR_HIP, "uploading the motif table failed");
    if (!rc) {
        hipLaunchKernelGGL(k_stream_reset, dim3((p->nslots + 255) / 256), dim3(256), 0, c->stream, (stream_slot *)z->slots.p,
                           p->nslots, (const int32_t *)nullptr, p->nslots, (const double *)nullptr, (const double *)nullptr);
        if (hipGetLastError() != hipSuccess) rc = sk_fail(SK_ERR_HIP, "launching the slot reset failed");
    }
    if (rc) { destroy(z); return rc; }
    c->sessions[h] = z;
    *handle = h;
    return SK_OK;
}

int sk_stream_session_info(sk_ctx *c, int32_t handle, int32_t *nslots, int32_t *nmotifs)
{
    stream_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (nslots) *nslots = z->p.nslots;
    if (nmotifs) *nmotifs = (int32_t)z->motifs.size();
    return SK_OK;
}

int sk_stream_session_stage(sk_ctx *c, int32_t handle, int which, size_t bytes, void **p)
{
    stream_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (which < 0 || which >= 4) return sk_fail(SK_ERR_INVALID, "internal: staging buffer %d", which);
    const int rc = sk_reserve(c, &z->host[which], bytes ? bytes : 1);
    if (rc) return rc;
    *p = z->host[which].p;
    return SK_OK;
}

int sk_stream_session_push(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows,
                           int64_t stride, const int32_t *d_len, int flush, sk_stream_rec *d_out)
{
    stream_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    const int K = (int)z->motifs.size();
    const int64_t cstride = d_rows ? stride : 1;
    int rc;
    if ((rc = sk_reserve(c, &z->work, (size_t)m * sizeof(stream_work)))) return rc;
    if ((rc = sk_reserve(c, &z->statlen, (size_t)m * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &z->comp, (size_t)m * (size_t)cstride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &z->stage, (size_t)m * (size_t)z->wpad * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &z->stage2, (size_t)m * (size_t)z->wpad * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &z->prep, (size_t)m * sizeof(sk_prep)))) return rc;
    stream_slot *slots = (stream_slot *)z->slots.p;
    stream_work *work = (stream_work *)z->work.p;
    int32_t *statlen = (int32_t *)z->statlen.p;

    hipLaunchKernelGGL(k_stream_ingest, dim3(m), dim3(256), 0, c->stream, slots, z->p.nslots, d_slots, m, d_rows, stride,
                       d_len, z->p.scale_low, z->p.scale_hi, z->p.calib, z->wpad, flush, (int16_t *)z->cal.p,
                       (int16_t *)z->comp.p, cstride, (int16_t *)z->stage.p, statlen, work);
    SK_HIP(hipGetLastError());
    // the statistics of the one-shot path over the buffered rows; entries whose calibration does not end here have length 0
    const int mode = z->p.scale_mode == SK_SCALE_MEDMAD ? SK_PREP_MEDMAD : SK_PREP_ZSCALE;
    if ((rc = sk_launch_prep_i16(c, (const int16_t *)z->stage.p, z->wpad, statlen, m, z->p.scale_low, z->p.scale_hi, mode,
                                 0.0, (int16_t *)z->stage2.p, (sk_prep *)z->prep.p, nullptr, 0))) return rc;
    hipLaunchKernelGGL(k_stream_adopt, dim3((m + 255) / 256), dim3(256), 0, c->stream, slots, work, statlen,
                       (const sk_prep *)z->prep.p, m);
    SK_HIP(hipGetLastError());
    for (const stream_motif &mo : z->motifs) {
        stream_kargs a;
        a.slots = slots; a.work = work; a.m = m; a.cal = (const int16_t *)z->cal.p; a.wpad = z->wpad;
        a.comp = (const int16_t *)z->comp.p; a.cstride = cstride; a.xlay = (const double *)mo.xlay.p; a.P = mo.P;
        a.D = (double *)mo.D.p; a.S = (int32_t *)mo.S.p; a.best = (stream_best *)mo.best.p;
        const int per_block = 4 * (64 / mo.L);
        hipLaunchKernelGGL(mo.fn, dim3((m + per_block - 1) / per_block), dim3(256), 0, c->stream, a);
        SK_HIP(hipGetLastError());
    }
    const int64_t recs = (int64_t)m * K;
    hipLaunchKernelGGL(k_stream_emit, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, c->stream, (const stream_slot *)slots,
                       (const stream_work *)work, m, (const stream_motif_dev *)z->table.p, K, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_stream_session_reset(sk_ctx *c, int32_t handle, const int32_t *d_slots, int32_t m, const double *d_center,
                            const double *d_scale)
{
    stream_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_stream_reset, dim3((m + 255) / 256), dim3(256), 0, c->stream, (stream_slot *)z->slots.p, z->p.nslots,
                       d_slots, m, d_center, d_scale);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_stream_session_close(sk_ctx *c, int32_t handle)
{
    stream_session *z = session_of(c, handle);
    if (!z) return SK_ERR_INVALID;
    SK_HIP(hipStreamSynchronize(c->stream));
    destroy(z);
    c->sessions[handle] = nullptr;
    return SK_OK;
}

void sk_stream_close_all(sk_ctx *c)
{
    for (int i = 0; i < SK_STREAM_MAX_SESSIONS; i++)
        if (c->sessions[i]) { destroy((stream_session *)c->sessions[i]); c->sessions[i] = nullptr; }
}
