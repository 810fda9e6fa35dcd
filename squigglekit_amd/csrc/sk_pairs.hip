// sk_pairs.hip -- DTW over a pair list for gfx950: a pool of float64 sequences and (query, target) index pairs.
//
// Every other DTW entry point sweeps ONE query (or a short list of motifs) over many reads.  Here the query differs from
// pair to pair: a read's event levels searched in a reference squiggle, a barcode of its own per read, the extracted spans
// of two hits against each other.  The cell arithmetic is k_sdtw's (sk_sdtw.hip), bit for bit; what is new is where a lane
// group finds its rows and its samples -- an entry of a per-call device table (sk_pair_entry) instead of the launch's one
// layout and the read index.
//
//   SK_PAIRS_SUBSEQUENCE   the record sk_dtw_subsequence(values[q], values[t]) returns (k_sdtw, MODE_PAIRS)
//   SK_PAIRS_GLOBAL        both ends pinned: D[0][0] = |x0 - y0|, first row and column accumulate, dist = D[N-1][M-1],
//                          start = 0, end = M - 1 (k_sdtw, MODE_PAIRS_GLOBAL).  This is mlpy's dtw_std(x, y,
//                          dist_only=True) as published; it is unpinned in the sense of SURVEY.md rows D1-D3 (no mlpy
//                          build to compare against): the tests hold it to a plain double-loop DP.
//
// The plan (host): every distinct query index gets its (L, R) from sk_exact_shape(N, npairs) and is laid out once, however
// many pairs use it; the pairs are grouped by (L, R), ordered inside a group by target length (longest first, ties by pair
// index: the groups of a wavefront run to the longest of them) and swept with one launch per group.  Records are
// scattered to out[pair index].  Nothing of the screening scheme is involved: no guard, no audit.
#include "sk_sdtw_dev.h"
#include <algorithm>
#include <vector>

namespace {

// ---- k_pairs_layout ----------------------------------------------------------------------------------------------------
// One workgroup per distinct query: its points, wherever they lie in the pool, into the per-lane layout sk_lane_layout
// states (row 0 in slot 0 of lane 0, the first P = L*R - N lanes one row short, their last slot a 0.0 pad).  The pool is
// on the device in both forms of the call, so the layouts are made there: no query travels back to the host.
__global__ __launch_bounds__(256)
void k_pairs_layout(const double *__restrict__ values, const sk_pair_query *__restrict__ qt, int nq, double *__restrict__ lay)
{
    const int i = blockIdx.x;
    if (i >= nq) return;
    const sk_pair_query q = qt[i];
    const int P = q.L * q.R - q.N;
    const double *src = values + q.src;
    double *dst = lay + q.xoff;
    for (int idx = threadIdx.x; idx < q.L * q.R; idx += blockDim.x) {
        const int l = idx / q.R, k = idx % q.R;
        const int cnt = (l < P) ? q.R - 1 : q.R;
        const int row = l * q.R - min(l, P) + k;            // lanes below l hold l*R rows less one per short lane
        dst[idx] = (k < cnt) ? src[row] : 0.0;
    }
}

} // namespace

int sk_launch_pairs_layout(sk_ctx *c, const double *d_values, const sk_pair_query *d_qt, int nq, double *d_lay)
{
    if (nq <= 0) return SK_OK;
    hipLaunchKernelGGL(k_pairs_layout, dim3((unsigned)nq), dim3(256), 0, c->stream, d_values, d_qt, nq, d_lay);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_pairs_check(const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs, int32_t mode, const void *out)
{
    if (mode != SK_PAIRS_SUBSEQUENCE && mode != SK_PAIRS_GLOBAL) return sk_fail(SK_ERR_INVALID, "unknown pairs mode %d", mode);
    if (npairs < 0 || nseq < 0) return sk_fail(SK_ERR_INVALID, "npairs or nseq < 0");
    if (npairs > ((int64_t)1 << 27)) return sk_fail(SK_ERR_UNSUPPORTED, "npairs %lld above 134217728", (long long)npairs);
    if (npairs == 0) return SK_OK;
    if (!off || !pairs || !out) return sk_fail(SK_ERR_INVALID, "NULL off/pairs/out");
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query, t = pairs[p].target;
        if (q < 0 || q >= nseq) return sk_fail(SK_ERR_INVALID, "pair %lld: query index %d outside [0, %d)", (long long)p, q, nseq);
        if (t < 0 || t >= nseq) return sk_fail(SK_ERR_INVALID, "pair %lld: target index %d outside [0, %d)", (long long)p, t, nseq);
        const int64_t N = off[q + 1] - off[q], M = off[t + 1] - off[t];
        if (N < 0 || M < 0 || M > 0x7fffff00)
            return sk_fail(SK_ERR_INVALID, "pair %lld: bad length (query %lld, target %lld)", (long long)p, (long long)N, (long long)M);
        if (N == 0) return sk_fail(SK_ERR_INVALID, "pair %lld: empty query (sequence %d)", (long long)p, q);
        if (N > 64 * 16)
            return sk_fail(SK_ERR_UNSUPPORTED, "pair %lld: query of %lld points (sequence %d; at most 1024)", (long long)p, (long long)N, q);
    }
    return SK_OK;
}

int sk_pairs_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                 int64_t npairs, int32_t mode, sk_hit *d_out)
{
    if (int rc0 = sk_pairs_check(off, nseq, pairs, npairs, mode, d_out)) return rc0;
    if (npairs == 0) return SK_OK;
    if (!d_values) return sk_fail(SK_ERR_INVALID, "NULL values");

    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier call may still read the old plan
    // ---- distinct queries: shape and layout, once each ------------------------------------------------------------------
    std::vector<int64_t> xoff_of((size_t)nseq, -1);
    std::vector<uint8_t> key_of((size_t)nseq, 0);           // (L == 64) * 16 + R - 1
    c->pairs_query.clear();
    int64_t nlay = 0;
    int64_t cnt[32] = {0};
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query;
        if (xoff_of[q] < 0) {
            const int N = (int)(off[q + 1] - off[q]);
            int L, R;
            sk_exact_shape(N, npairs, &L, &R);
            xoff_of[q] = nlay;
            key_of[q] = (uint8_t)((L == 64 ? 16 : 0) + R - 1);
            sk_pair_query e;
            e.src = off[q] - off0; e.xoff = nlay; e.N = N; e.L = L; e.R = R; e.pad = 0;
            c->pairs_query.push_back(e);
            nlay += (int64_t)L * R;
        }
        cnt[key_of[q]]++;
    }
    // ---- the table: group after group, longest target first --------------------------------------------------------------
    int64_t first[33];
    first[0] = 0;
    for (int g = 0; g < 32; g++) first[g + 1] = first[g] + cnt[g];
    std::vector<int32_t> order((size_t)npairs);
    {
        int64_t cur[32];
        for (int g = 0; g < 32; g++) cur[g] = first[g];
        for (int64_t p = 0; p < npairs; p++) order[(size_t)cur[key_of[pairs[p].query]]++] = (int32_t)p;
    }
    for (int g = 0; g < 32; g++)
        std::stable_sort(order.begin() + first[g], order.begin() + first[g + 1], [&](int32_t a, int32_t b) {
            const int32_t ta = pairs[a].target, tb = pairs[b].target;
            return off[ta + 1] - off[ta] > off[tb + 1] - off[tb];
        });
    c->pairs_table.resize((size_t)npairs);
    for (int64_t i = 0; i < npairs; i++) {
        const int32_t p = order[(size_t)i], q = pairs[p].query, t = pairs[p].target;
        const int key = key_of[q], L = key >= 16 ? 64 : 16, R = (key & 15) + 1;
        sk_pair_entry e;
        e.toff = off[t] - off0; e.xoff = xoff_of[q]; e.n = (int32_t)(off[t + 1] - off[t]);
        e.P = L * R - (int32_t)(off[q + 1] - off[q]); e.pair = p; e.pad = 0;
        c->pairs_table[(size_t)i] = e;
    }
    // ---- upload the two tables, lay the queries out on the device --------------------------------------------------------
    const size_t nq = c->pairs_query.size();
    int rc = sk_reserve(c, &c->pairs, (size_t)nlay * sizeof(double) + (size_t)npairs * sizeof(sk_pair_entry) +
                                      nq * sizeof(sk_pair_query) + 16);
    if (rc) return rc;
    double *d_lay = (double *)c->pairs.p;
    sk_pair_entry *d_pt = (sk_pair_entry *)(d_lay + nlay);
    sk_pair_query *d_qt = (sk_pair_query *)(d_pt + npairs);
    SK_HIP(hipMemcpyAsync(d_pt, c->pairs_table.data(), (size_t)npairs * sizeof(sk_pair_entry), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_qt, c->pairs_query.data(), nq * sizeof(sk_pair_query), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_launch_pairs_layout(c, d_values, d_qt, (int)nq, d_lay))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // (no prep kernels: sk_last_kernel_ms reports 0 for them)
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    for (int g = 0; g < 32; g++) {
        if (!cnt[g]) continue;
        const int L = g >= 16 ? 64 : 16, R = (g & 15) + 1;
        if ((rc = sk_launch_sdtw_pairs(c, L, R, mode == SK_PAIRS_GLOBAL, d_values, d_lay, d_pt + first[g], (int32_t)cnt[g], d_out)))
            return rc;
    }
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->last_retry = 0;
    c->retry_dev = false;                                   // (no screening counters: sk_last_dtw_guard reads none)
    c->prof_chunks = 0;
    c->ev_valid = true;
    return SK_OK;
}

// ---- hit lists over the list (the select: sk_pairhits.hip) -------------------------------------------------------------
// The queries are shaped and laid out as above, once each.  The list is cut, in list order, into slices whose last rows
// (12 B per target column: D f64, S i32) fit the budget of sk_hits' row buffer (SK_HITS_ROW_BYTES, 2 GiB; a slice holds at
// least one pair).  A slice's pairs are swept as FRESH sk_map_entry entries (k_sdtw, MODE_PAIRS_CHAIN: the virtual row -1
// enters, the last row is stored at soff) -- one launch per (L, R) group, longest target first -- and its rows go through
// the select; the next slice follows on the same stream and reuses the buffer.  An empty target is not swept: its entry
// of the select carries SK_FLAG_EMPTY.
int sk_pairs_hits_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                      int64_t npairs, int32_t K, double max_dist, sk_hit *d_out, int32_t *d_count)
{
    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier call may still read the old plan
    size_t budget = (size_t)2 << 30;
    if (const char *e = sk_tune("SK_HITS_ROW_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
    const int64_t budget_cols = (int64_t)(budget / 12);
    // ---- distinct queries: shape and layout, once each ------------------------------------------------------------------
    std::vector<int64_t> xoff_of((size_t)nseq, -1);
    std::vector<uint8_t> key_of((size_t)nseq, 0);           // (L == 64) * 16 + R - 1
    c->pairs_query.clear();
    int64_t nlay = 0;
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query;
        if (xoff_of[q] >= 0) continue;
        const int N = (int)(off[q + 1] - off[q]);
        int L, R;
        sk_exact_shape(N, npairs, &L, &R);
        xoff_of[q] = nlay;
        key_of[q] = (uint8_t)((L == 64 ? 16 : 0) + R - 1);
        sk_pair_query e;
        e.src = off[q] - off0; e.xoff = nlay; e.N = N; e.L = L; e.R = R; e.pad = 0;
        c->pairs_query.push_back(e);
        nlay += (int64_t)L * R;
    }
    // ---- slices, and per slice the sweep's entries group after group and the select's table ---------------------------
    struct run { int64_t first; int32_t count; int L, R; };
    struct slice { int64_t p0, p1; size_t run0, run1; };
    std::vector<slice> slices;
    std::vector<run> runs;
    c->pairhits_sweep.clear();
    c->rowhit_table.resize((size_t)npairs);
    int64_t max_cols = 0, max_pairs = 0;
    std::vector<int32_t> order;
    for (int64_t p0 = 0; p0 < npairs;) {
        int64_t cols = 0, p1 = p0;
        while (p1 < npairs) {
            const int32_t t = pairs[p1].target;
            const int64_t M = off[t + 1] - off[t];
            if (p1 > p0 && cols + M > budget_cols) break;
            c->rowhit_table[(size_t)p1] = {cols, p1, (int32_t)M, M == 0 ? SK_FLAG_EMPTY : 0};
            cols += M;
            p1++;
        }
        slice sl;
        sl.p0 = p0; sl.p1 = p1; sl.run0 = runs.size();
        for (int g = 0; g < 32; g++) {
            order.clear();
            for (int64_t p = p0; p < p1; p++)
                if (key_of[pairs[p].query] == g && c->rowhit_table[(size_t)p].n > 0) order.push_back((int32_t)p);
            if (order.empty()) continue;
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
                return c->rowhit_table[(size_t)a].n > c->rowhit_table[(size_t)b].n;
            });
            const int L = g >= 16 ? 64 : 16, R = (g & 15) + 1;
            runs.push_back({(int64_t)c->pairhits_sweep.size(), (int32_t)order.size(), L, R});
            for (int32_t p : order) {
                const int32_t q = pairs[p].query, t = pairs[p].target;
                sk_map_entry e;
                e.toff = off[t] - off0; e.xoff = xoff_of[q]; e.soff = c->rowhit_table[(size_t)p].col0;
                e.n = c->rowhit_table[(size_t)p].n; e.P = L * R - (int32_t)(off[q + 1] - off[q]);
                e.rec = (int32_t)(p - p0); e.cont = 0;
                c->pairhits_sweep.push_back(e);
            }
        }
        sl.run1 = runs.size();
        slices.push_back(sl);
        max_cols = std::max(max_cols, cols);
        max_pairs = std::max(max_pairs, p1 - p0);
        p0 = p1;
    }
    // ---- room: layouts + the two tables of the queries and the sweep; the row buffer; the select's table ---------------
    const size_t nq = c->pairs_query.size(), ne = c->pairhits_sweep.size();
    int rc = sk_reserve(c, &c->pairs, (size_t)nlay * sizeof(double) + ne * sizeof(sk_map_entry) + nq * sizeof(sk_pair_query) + 16);
    if (rc) return rc;
    const size_t colsD = (size_t)(max_cols > 0 ? max_cols : 1), colsS = (colsD + 1) & ~(size_t)1;
    if ((rc = sk_reserve(c, &c->hitrows, colsD * sizeof(double) + colsS * sizeof(int32_t) + (size_t)max_pairs * sizeof(sk_hit)))) return rc;
    if ((rc = sk_rowhits_reserve(c, npairs))) return rc;
    double *d_lay = (double *)c->pairs.p;
    sk_map_entry *d_mp = (sk_map_entry *)(d_lay + nlay);
    sk_pair_query *d_qt = (sk_pair_query *)(d_mp + ne);
    double *rowD = (double *)c->hitrows.p;
    int32_t *rowS = (int32_t *)(rowD + colsD);
    sk_hit *d_last = (sk_hit *)(rowS + colsS);              // the sweep's own records: hit 1 of the select says the same
    if (ne) SK_HIP(hipMemcpyAsync(d_mp, c->pairhits_sweep.data(), ne * sizeof(sk_map_entry), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_qt, c->pairs_query.data(), nq * sizeof(sk_pair_query), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_launch_pairs_layout(c, d_values, d_qt, (int)nq, d_lay))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // (no prep kernels: sk_last_kernel_ms reports 0 for them)
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    c->pairhits_long_rows = 0;
    for (const slice &sl : slices) {
        for (size_t i = sl.run0; i < sl.run1; i++)
            if ((rc = sk_launch_sdtw_map(c, runs[i].L, runs[i].R, d_values, d_lay, d_mp + runs[i].first, runs[i].count, rowD, rowS,
                                         d_last))) return rc;
        if ((rc = sk_launch_rowhits(c, c->rowhit_table.data() + sl.p0, sl.p0, (int32_t)(sl.p1 - sl.p0), rowD, rowS, K, max_dist,
                                    d_out, d_count, &c->pairhits_long_rows))) return rc;
    }
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->pairhits_row_bytes = max_cols * 12;
    c->pairhits_slices = (int64_t)slices.size();
    c->last_retry = 0;
    c->retry_dev = false;                                   // (no screening counters: sk_last_dtw_guard reads none)
    c->prof_chunks = 0;
    c->ev_valid = true;
    return SK_OK;
}
