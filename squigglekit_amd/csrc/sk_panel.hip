// sk_panel.hip -- MotifSeq over a search region, many motifs ranked per read, for gfx950.
//
// "Which of these K signals sits in the first (or last) few thousand samples?"  The reference answers it one motif and
// one whole read at a time: the `for name in m_order` loop around mlpy.dtw_subsequence
// (/root/reference/MotifSeq.py:436-439), the filter before it (:274, :317-324), medmad / zscale (:186-200), and the
// ranking quantity Z = (dist - mod_mean) / mod_stdev (:441-443) the caller then sorts by.  Here:
//
//   k_region_rows   cuts every read as the Python slice raw[begin:end] (or its own win row) BEFORE the filter and packs
//                   the cuts into window rows of one stride, so that filter + statistics (the existing prep kernels) run
//                   once per read over the slice and every later kernel touches window samples only.
//   k_sdtw          (sk_sdtw.hip) in its MODE_PANEL: the exact FP64 single pass over all (read, motif) pairs of a shape
//                   group in ONE grid: blockIdx.y picks the motif, whose per-lane layout and short-lane count come
//                   from a device table uploaded once per call.  Motifs with the same (L, R) lane layout form a group.
//                   No screening scheme: windows are short, and its certificate machinery is sized for long reads.
//   k_panel_rank    per read: score[k] = (dist_k - mean[k]) / sd[k] as one correctly rounded subtraction and one
//                   correctly rounded division (__dsub_rn / __ddiv_rn: the very double Python prints as Z-score), the
//                   smallest score (ties: the smallest k), then the smallest of the rest.
#include "sk_sdtw_dev.h"
#include <vector>

namespace {

// ---- k_region_rows -----------------------------------------------------------------------------------------------------
// One workgroup per read; a thread moves 8 samples at a time: 8 two-byte loads (the slice starts anywhere), one 16-byte
// store (window rows are 16-byte aligned, wstride is a multiple of 8).  The tail of the row is zeroed.
__global__ __launch_bounds__(256)
void k_region_rows(const int16_t *__restrict__ sig, int64_t stride, const int32_t *__restrict__ len, int nreads,
                   int begin, int end, const int32_t *__restrict__ win, int16_t *__restrict__ rows, int wstride,
                   int32_t *__restrict__ wlen, int32_t *__restrict__ from)
{
    const int r = blockIdx.x;
    if (r >= nreads) return;
    int n = len[r];
    n = n < 0 ? 0 : (n > stride ? (int)stride : n);
    const int b = win ? win[2 * r] : begin, e = win ? win[2 * r + 1] : end;
    int lo, hi;
    sk_slice_indices(n, b, e, &lo, &hi);
    int m = hi > lo ? hi - lo : 0;
    if (m > wstride) m = wstride;
    const int16_t *src = sig + (int64_t)r * stride + lo;
    int16_t *dst = rows + (int64_t)r * wstride;
    for (int i = threadIdx.x * 8; i < wstride; i += blockDim.x * 8) {
        union { int16_t s[8]; uint4 v; } u;
#pragma unroll
        for (int q = 0; q < 8; q++) u.s[q] = (i + q < m) ? src[i + q] : (int16_t)0;
        *(uint4 *)(dst + i) = u.v;
    }
    if (threadIdx.x == 0) {
        wlen[r] = m;
        if (from) from[r] = lo;
    }
}

__global__ __launch_bounds__(256)
void k_region_rows_f64(const double *__restrict__ sig, const int64_t *__restrict__ src, const int64_t *__restrict__ woff,
                       int nreads, double *__restrict__ out)
{
    const int r = blockIdx.x;
    if (r >= nreads) return;
    const int64_t o = woff[r], m = woff[r + 1] - o;
    const double *s = sig + src[r];
    for (int64_t i = threadIdx.x; i < m; i += blockDim.x) out[o + i] = s[i];
}

// ---- k_panel_rank ------------------------------------------------------------------------------------------------------
// One thread per read.  Z = (dist - mean) / sd with the reference's two operations (MotifSeq.py:441-443), each correctly
// rounded and never fused.  NaN scores are skipped; the strict < over ascending k keeps the smallest k of a tie.
__global__ __launch_bounds__(256)
void k_panel_rank(const sk_hit *__restrict__ rec, int64_t rec_stride, int nreads, int K, const double *__restrict__ mean,
                  const double *__restrict__ sd, sk_panel_rec *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    const sk_hit h0 = rec[r];
    const double qnan = __builtin_nan("");
    int best = -1, second = -1;
    double sb = qnan, ss = qnan;
    if (!(h0.flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE))) {
        for (int k = 0; k < K; k++) {
            const double s = __ddiv_rn(__dsub_rn(rec[(int64_t)k * rec_stride + r].dist, mean[k]), sd[k]);
            if (s == s && (best < 0 || s < sb)) { best = k; sb = s; }
        }
        for (int k = 0; k < K; k++) {
            if (k == best) continue;
            const double s = __ddiv_rn(__dsub_rn(rec[(int64_t)k * rec_stride + r].dist, mean[k]), sd[k]);
            if (s == s && (second < 0 || s < ss)) { second = k; ss = s; }
        }
    }
    sk_panel_rec o;
    o.best = best; o.second = second; o.score_best = sb; o.score_second = ss;
    if (best >= 0) o.hit = rec[(int64_t)best * rec_stride + r];
    else { o.hit.dist = qnan; o.hit.start = -1; o.hit.end = -1; o.hit.n = h0.n; o.hit.flags = h0.flags; }
    out[r] = o;
}

} // namespace

int sk_launch_region_rows_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              int32_t begin, int32_t end, const int32_t *d_win, int16_t *d_rows, int64_t wstride,
                              int32_t *d_wlen, int32_t *d_from)
{
    if (nreads <= 0) return SK_OK;
    if (wstride < 8 || wstride % 8 || wstride > 0x7ffffff8 || ((uintptr_t)d_rows & 15))
        return sk_fail(SK_ERR_INVALID, "internal: window rows need a 16-byte base and a stride that is a multiple of 8");
    hipLaunchKernelGGL(k_region_rows, dim3(nreads), dim3(256), 0, c->stream, d_sig, stride, d_len, nreads, begin, end,
                       d_win, d_rows, (int)wstride, d_wlen, d_from);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_launch_region_rows_f64(sk_ctx *c, const double *d_sig, const int64_t *d_src, const int64_t *d_woff, int32_t nreads,
                              double *d_out)
{
    if (nreads <= 0) return SK_OK;
    hipLaunchKernelGGL(k_region_rows_f64, dim3(nreads), dim3(256), 0, c->stream, d_sig, d_src, d_woff, nreads, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// c->panel: [layouts: doubles][mean: K doubles][sd: K doubles][table: sk_panel_motif per short motif]
static size_t panel_layout_doubles(const sk_ctx *c) { return c->panel_host.size(); }

int sk_panel_plan(sk_ctx *c, const double *motifs, const int32_t *motif_off, int32_t nmotifs, const double *mean,
                  const double *sd, int64_t pairs)
{
    // (L, R) per motif: the exact single pass's choice for `pairs` reads
    std::vector<int> Ls(nmotifs), Rs(nmotifs);
    c->panel_long.clear();
    c->panel_groups.clear();
    c->panel_table.clear();
    for (int32_t k = 0; k < nmotifs; k++) {
        const int N = motif_off[k + 1] - motif_off[k];
        if (N > 64 * 16) { c->panel_long.push_back(k); Ls[k] = 0; Rs[k] = 0; continue; }
        sk_exact_shape(N, pairs, &Ls[k], &Rs[k]);
    }
    SK_HIP(hipStreamSynchronize(c->stream));               // an earlier call may still read the old plan
    c->panel_host.clear();
    for (int32_t k = 0; k < nmotifs; k++) {                // groups in the order of their first member
        if (!Ls[k]) continue;
        bool seen = false;
        for (const sk_panel_group &g : c->panel_groups) seen = seen || (g.L == Ls[k] && g.R == Rs[k]);
        if (seen) continue;
        sk_panel_group g;
        g.L = Ls[k]; g.R = Rs[k]; g.first = (int32_t)c->panel_table.size(); g.count = 0;
        for (int32_t q = k; q < nmotifs; q++) {
            if (Ls[q] != g.L || Rs[q] != g.R) continue;
            const int N = motif_off[q + 1] - motif_off[q];
            sk_panel_motif t;
            t.xoff = (int32_t)c->panel_host.size(); t.P = g.L * g.R - N; t.k = q; t.pad = 0;
            c->panel_host.resize(c->panel_host.size() + (size_t)g.L * g.R);
            if (!sk_lane_layout(motifs + motif_off[q], N, g.L, g.R, &c->panel_host[(size_t)t.xoff]))
                return sk_fail(SK_ERR_INVALID, "internal: motif layout mismatch");
            c->panel_table.push_back(t);
            g.count++;
        }
        c->panel_groups.push_back(g);
    }
    const size_t nlay = panel_layout_doubles(c);
    const size_t bytes = (nlay + 2 * (size_t)nmotifs) * sizeof(double) + c->panel_table.size() * sizeof(sk_panel_motif) + 16;
    int rc = sk_reserve(c, &c->panel, bytes);
    if (rc) return rc;
    double *d = (double *)c->panel.p;
    if (nlay) SK_HIP(hipMemcpyAsync(d, c->panel_host.data(), nlay * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d + nlay, mean, (size_t)nmotifs * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d + nlay + nmotifs, sd, (size_t)nmotifs * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (!c->panel_table.empty())
        SK_HIP(hipMemcpyAsync(d + nlay + 2 * (size_t)nmotifs, c->panel_table.data(),
                              c->panel_table.size() * sizeof(sk_panel_motif), hipMemcpyHostToDevice, c->stream));
    return SK_OK;
}

// Long windows over many reads: there the default path's fixed-point screening + certified exact window (sk_sdtwq.hip)
// returns the same records -- bit for bit, that is its contract -- for a fraction of the exact sweep's cells, so such a
// group is delegated to it, one launch set per motif.  The one-grid exact kernel takes what the default
// path would sweep exactly anyway: short windows and small batches.  N0: the points of the group's first motif.
static bool delegates(const sk_sdtw_args *base, int N0)
{
    return base->nreads >= 256 && base->max_len >= 4 * (int64_t)(N0 + N0 / 8 + 8 + 128) && sk_tune("SK_PANEL_EXACT") == nullptr;
}

int sk_launch_panel_dtw(sk_ctx *c, const sk_sdtw_args *base, const double *motifs, const int32_t *motif_off,
                        sk_hit *d_all, int64_t out_stride)
{
    if (base->nreads <= 0) return SK_OK;
    int rc;
    // one launch set of the default path for motif k (it records the main-pass events itself)
    int accumulate = base->accumulate;
    auto one_motif = [&](int32_t k, int force_single) -> int {
        sk_sdtw_args a = *base;
        a.motif = motifs + motif_off[k]; a.nmotif = motif_off[k + 1] - motif_off[k];
        a.out = d_all + (size_t)k * (size_t)out_stride; a.last_row = nullptr; a.force_single = force_single;
        a.accumulate = force_single ? 0 : accumulate; a.fuse = nullptr;
        return sk_launch_sdtw(c, &a);
    };
    // motifs of more than 1 024 points: the chained launcher, one motif at a time
    for (int32_t k : c->panel_long)
        if ((rc = one_motif(k, 1))) return rc;
    bool delegated = !c->panel_long.empty();
    std::vector<char> screen;                               // per group: delegated?
    for (const sk_panel_group &g : c->panel_groups) {
        const int k0 = c->panel_table[g.first].k;
        screen.push_back(delegates(base, motif_off[k0 + 1] - motif_off[k0]));
    }
    for (size_t i = 0; i < c->panel_groups.size(); i++) {
        const sk_panel_group &g = c->panel_groups[i];
        if (!screen[i]) continue;
        for (int32_t q = 0; q < g.count; q++) {
            if ((rc = one_motif(c->panel_table[g.first + q].k, 0))) return rc;
            accumulate = 1;
            delegated = true;
        }
    }
    if (!delegated) SK_HIP(hipEventRecord(c->ev[2], c->stream));
    const size_t nlay = panel_layout_doubles(c);
    const int32_t nmot = (int32_t)(c->panel_table.size() + c->panel_long.size());
    const sk_panel_motif *d_table = (const sk_panel_motif *)((const double *)c->panel.p + nlay + 2 * (size_t)nmot);
    for (size_t i = 0; i < c->panel_groups.size(); i++) {
        const sk_panel_group &g = c->panel_groups[i];
        if (screen[i]) continue;
        if ((rc = sk_launch_sdtw_panel(c, base, g.L, g.R, (const double *)c->panel.p, d_table + g.first, g.count, d_all,
                                       out_stride))) return rc;
    }
    if (!delegated) {
        c->last_retry = 0;
        c->retry_dev = false;                               // (no screening counters: sk_last_dtw_guard reads none)
        c->prof_chunks = 0;
    }
    return SK_OK;
}

int sk_launch_panel_rank(sk_ctx *c, const sk_hit *d_all, int64_t out_stride, int32_t nreads, int32_t nmotifs,
                         sk_panel_rec *d_out)
{
    if (nreads <= 0) return SK_OK;
    const double *d_mean = (const double *)c->panel.p + panel_layout_doubles(c);
    hipLaunchKernelGGL(k_panel_rank, dim3((nreads + 255) / 256), dim3(256), 0, c->stream, d_all, out_stride, nreads, nmotifs,
                       d_mean, d_mean + nmotifs, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
