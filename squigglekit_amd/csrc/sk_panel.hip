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
//   k_panel_dtw     the exact FP64 subsequence DTW of sk_sdtw.hip's single pass (same cell arithmetic, same tie order:
//                   diagonal, then left, then up; first argmin of the last row) over all (read, motif) pairs of a shape
//                   group in ONE grid: blockIdx.y picks the motif, whose per-lane layout and short-lane count come
//                   from a device table uploaded once per call.  Motifs with the same (L, R) lane layout form a group.
//                   No screening scheme: windows are short, and its certificate machinery is sized for long reads.
//   k_panel_rank    per read: score[k] = (dist_k - mean[k]) / sd[k] as one correctly rounded subtraction and one
//                   correctly rounded division (__dsub_rn / __ddiv_rn: the very double Python prints as Z-score), the
//                   smallest score (ties: the smallest k), then the smallest of the rest.
#include "sk_sdtw_dev.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
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

// ---- k_panel_dtw -------------------------------------------------------------------------------------------------------
struct panel_kargs {
    const void    *samples;      // filtered window samples: int16 rows or float64 ragged
    const void    *samples_raw;  // float64: the unfiltered windows, read for reads flagged SK_IFLAG_INPLACE
    int64_t        stride;
    const int64_t *off;
    const sk_prep *prep;
    int            nreads;
    const double  *xlay;         // the panel's layouts, motif after motif
    const sk_panel_motif *mt;    // this group's table entries; blockIdx.y indexes them
    sk_hit        *out;          // record of (motif k, read r) at out[k * out_stride + r]
    int64_t        out_stride;
};

// The single exact pass of sk_sdtw.hip (k_sdtw, MODE_FULL) for one (read group, motif) per lane group: L lanes own one
// read, lane l owns R consecutive motif rows with their D (f64) and S (the column where the cell's back-trace reaches
// row 0); at step t lane l computes column t - l.  See sk_sdtw.hip for the boundary conventions.
template <int L, int R, int FEED>
__global__ __launch_bounds__(256)
void k_panel_dtw(const panel_kargs a)
{
    static_assert(L == 16 || L == 64, "lanes per read");
    constexpr int G = 64 / L;
    constexpr int SHR = (L == 16) ? DPP_ROW_SHR1 : DPP_WAVE_SHR1;
    constexpr int ROL = (L == 16) ? DPP_ROW_ROL1 : DPP_WAVE_ROL1;
    const double INF = __builtin_huge_val();

    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int g = lane / L, l = lane % L;
    int slot = wave * G + g;
    const bool live = slot < a.nreads;
    if (!live) slot = a.nreads - 1;
    const int r = slot;
    const sk_panel_motif mt = a.mt[blockIdx.y];          // (block-uniform: scalar loads)

    int n, flags;
    double center, scale, rc1 = 0.0, rc2 = 0.0;
    const int16_t *s16 = nullptr;
    const double  *s64 = nullptr;
    {
        const sk_prep pr = a.prep[r];
        n = pr.n; flags = pr.flags & SK_FLAG_PUBLIC; center = pr.center; scale = pr.scale;
        if constexpr (FEED == SK_FEED_I16) {
            s16 = (const int16_t *)a.samples + (int64_t)r * a.stride;
        } else {
            rc1 = pr.top; rc2 = pr.bot;                  // zscale re-centring terms (0.0 unless sklearn applied them)
            s64 = (const double *)(((pr.flags & SK_IFLAG_INPLACE) && a.samples_raw) ? a.samples_raw : a.samples) + a.off[r];
        }
    }
    if (!live) n = 0;

    int nsteps = n > 0 ? n + L - 1 : 0;                  // wave-uniform step count
#pragma unroll
    for (int d = L; d < 64; d <<= 1) nsteps = max(nsteps, __shfl_xor(nsteps, d));
    nsteps = __builtin_amdgcn_readfirstlane(nsteps);
    const int nblk = (nsteps + L - 1) / L;

    double x[R];
#pragma unroll
    for (int k = 0; k < R; k++) x[k] = a.xlay[mt.xoff + l * R + k];
    const bool shortlane = l < mt.P;

    double D[R];
    int    S[R];
#pragma unroll
    for (int k = 0; k < R; k++) { D[k] = INF; S[k] = -1; }
    double botD = (R == 1 && l == 0 && shortlane) ? 0.0 : INF;
    int    botS = (R == 1 && l == 0 && shortlane) ? 0 : -1;
    double diagD = (l == 0) ? 0.0 : INF;
    int    diagS = (l == 0) ? 0 : -1;
    double y = INF;
    double best = INF;  int bestS = -1, bestJ = -1;

    auto fetch = [&](int idx) -> double {                // normalised sample idx of my read, +inf outside
        if constexpr (FEED == SK_FEED_I16) {
            int16_t raw = (idx < n) ? s16[idx] : (int16_t)0;
            double v = ((double)raw - center) / scale;
            return (idx < n) ? v : INF;
        } else {
            double raw = (idx < n) ? s64[idx] : 0.0;
            double v = ((raw - center) - rc1) / scale - rc2;
            return (idx < n) ? v : INF;
        }
    };

    double F = fetch(l);
    for (int blk = 0; blk < nblk; blk++) {
        const double Fnext = fetch((blk + 1) * L + l);   // in flight during the L steps below
#pragma unroll 2
        for (int q = 0; q < L; q++) {
            const int t = blk * L + q;
            y = dpp_f64<SHR>(F, y);                      // lane 0 takes sample t from the feed
            F = dpp_f64<ROL>(F, F);
            const double upD = dpp_f64<SHR>(0.0, botD);  // lane 0: virtual row -1 (D = 0, S = column + 1)
            const int    upS = dpp_i32<SHR>(t + 1, botS);
            double dgD = diagD;  int dgS = diagS;        // (i-1, j-1)
            double uD = upD;     int uS = upS;           // (i-1, j)
#pragma unroll
            for (int k = 0; k < R; k++) {
                const double lfD = D[k];                 // (i, j-1)
                const int    lfS = S[k];
                const double c = fabs(x[k] - y);
                const bool lt1 = lfD < dgD;              // diag wins ties over left
                double m1;
                if constexpr (FEED == SK_FEED_I16) m1 = vmin(lfD, dgD); else m1 = lt1 ? lfD : dgD;
                const int s1 = lt1 ? lfS : dgS;
                const bool lt2 = uD < m1;                // up only if strictly smaller
                double m;
                if constexpr (FEED == SK_FEED_I16) m = vmin(uD, m1); else m = lt2 ? uD : m1;
                const int s = lt2 ? uS : s1;
                const double nd = c + m;
                dgS = lfS;  S[k] = s;  uS = s;
                dgD = lfD;  D[k] = nd; uD = nd;
            }
            diagD = upD;  diagS = upS;
            if constexpr (R >= 2) {
                botD = shortlane ? D[R - 2] : D[R - 1];
                botS = shortlane ? S[R - 2] : S[R - 1];
            } else {
                botD = shortlane ? upD : D[0];           // a lane with no rows just forwards
                botS = shortlane ? upS : S[0];
            }
            if (D[R - 1] < best) { best = D[R - 1]; bestJ = t - l; bestS = S[R - 1]; }   // first argmin (lane L-1's counts)
        }
        F = Fnext;
    }

    if (live && l == L - 1) {
        sk_hit h;
        if (n > 0) { h.dist = best; h.start = bestS; h.end = bestJ; }
        else       { h.dist = __builtin_nan(""); h.start = -1; h.end = -1; }
        h.n = n;
        h.flags = flags;
        a.out[(int64_t)mt.k * a.out_stride + r] = h;
    }
}

typedef void (*panel_fn)(const panel_kargs);

template <int L, int FEED>
panel_fn pick_r(int R)
{
    switch (R) {
#define SK_CASE(RR) case RR: return k_panel_dtw<L, RR, FEED>;
        SK_CASE(1) SK_CASE(2) SK_CASE(3) SK_CASE(4) SK_CASE(5) SK_CASE(6) SK_CASE(7) SK_CASE(8)
        SK_CASE(9) SK_CASE(10) SK_CASE(11) SK_CASE(12) SK_CASE(13) SK_CASE(14) SK_CASE(15) SK_CASE(16)
#undef SK_CASE
    }
    return nullptr;
}

panel_fn pick(int feed, int L, int R)
{
    if (feed == SK_FEED_I16) return L == 16 ? pick_r<16, SK_FEED_I16>(R) : pick_r<64, SK_FEED_I16>(R);
    if (feed == SK_FEED_F64_NORM) return L == 16 ? pick_r<16, SK_FEED_F64_NORM>(R) : pick_r<64, SK_FEED_F64_NORM>(R);
    return nullptr;
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
    // (L, R) per motif as the exact single pass picks them (sk_sdtw.hip, exact_shape): four reads per wavefront for
    // motifs of up to 256 points unless the call is too small to fill the chip that way
    int small_max = 2048;
    if (const char *e = sk_tune("SK_DTW_SMALL_MAX")) { int v = atoi(e); if (v >= 0) small_max = v; }
    const bool spread = pairs <= small_max && !sk_tune("SK_DTW_NO_SMALL");
    std::vector<int> Ls(nmotifs), Rs(nmotifs);
    c->panel_long.clear();
    c->panel_groups.clear();
    c->panel_table.clear();
    for (int32_t k = 0; k < nmotifs; k++) {
        const int N = motif_off[k + 1] - motif_off[k];
        if (N > 64 * 16) { c->panel_long.push_back(k); Ls[k] = 0; Rs[k] = 0; continue; }
        if (N <= 16 * 16 && !(spread && N >= 32)) { Ls[k] = 16; Rs[k] = (N + 15) / 16; }
        else                                      { Ls[k] = 64; Rs[k] = (N + 63) / 64; }
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
            const double *m = motifs + motif_off[q];
            sk_panel_motif t;
            t.xoff = (int32_t)c->panel_host.size(); t.P = g.L * g.R - N; t.k = q; t.pad = 0;
            c->panel_host.resize(c->panel_host.size() + (size_t)g.L * g.R, 0.0);
            int row = 0;
            for (int l = 0; l < g.L; l++) {
                const int cnt = (l < t.P) ? g.R - 1 : g.R;
                for (int i = 0; i < cnt; i++) c->panel_host[(size_t)t.xoff + (size_t)l * g.R + i] = m[row++];
            }
            if (row != N) return sk_fail(SK_ERR_INVALID, "internal: motif layout mismatch");
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

int sk_launch_panel_dtw(sk_ctx *c, const sk_sdtw_args *base, const double *motifs, const int32_t *motif_off,
                        sk_hit *d_all, int64_t out_stride)
{
    if (base->nreads <= 0) return SK_OK;
    int rc;
    // motifs of more than 1 024 points: the chained launcher, one motif at a time (it records the main-pass events itself)
    for (int32_t k : c->panel_long) {
        sk_sdtw_args a = *base;
        a.motif = motifs + motif_off[k]; a.nmotif = motif_off[k + 1] - motif_off[k];
        a.out = d_all + (size_t)k * (size_t)out_stride; a.last_row = nullptr; a.force_single = 1; a.accumulate = 0;
        a.fuse = nullptr;
        if ((rc = sk_launch_sdtw(c, &a))) return rc;
    }
    // Long windows over many reads: there the default path's fixed-point screening + certified exact window
    // (sk_sdtwq.hip) returns the same records -- bit for bit, that is its contract -- for a fraction of the exact
    // sweep's cells, so such a call delegates to it, one launch set per motif.  The one-grid exact
    // kernel takes what the default path would sweep exactly anyway: short windows and small batches.
    int accumulate = base->accumulate;
    bool delegated = !c->panel_long.empty();
    const size_t nlay = panel_layout_doubles(c);
    const int32_t nmot = (int32_t)(c->panel_table.size() + c->panel_long.size());
    const sk_panel_motif *d_table = (const sk_panel_motif *)((const double *)c->panel.p + nlay + 2 * (size_t)nmot);
    for (const sk_panel_group &g : c->panel_groups) {
        const int k0 = c->panel_table[g.first].k;
        const int N0 = motif_off[k0 + 1] - motif_off[k0];
        const bool screen = base->nreads >= 256 && base->max_len >= 4 * (int64_t)(N0 + N0 / 8 + 8 + 128) &&
                            sk_tune("SK_PANEL_EXACT") == nullptr;
        if (screen) {
            for (int32_t q = 0; q < g.count; q++) {
                const int32_t k = c->panel_table[g.first + q].k;
                sk_sdtw_args a = *base;
                a.motif = motifs + motif_off[k]; a.nmotif = motif_off[k + 1] - motif_off[k];
                a.out = d_all + (size_t)k * (size_t)out_stride; a.last_row = nullptr; a.force_single = 0;
                a.accumulate = accumulate; a.fuse = nullptr;
                if ((rc = sk_launch_sdtw(c, &a))) return rc;
                accumulate = 1;
                delegated = true;
            }
            continue;
        }
    }
    if (!delegated) SK_HIP(hipEventRecord(c->ev[2], c->stream));
    for (const sk_panel_group &g : c->panel_groups) {
        const int k0 = c->panel_table[g.first].k;
        const int N0 = motif_off[k0 + 1] - motif_off[k0];
        if (base->nreads >= 256 && base->max_len >= 4 * (int64_t)(N0 + N0 / 8 + 8 + 128) && sk_tune("SK_PANEL_EXACT") == nullptr)
            continue;
        panel_fn fn = pick(base->feed, g.L, g.R);
        if (!fn) return sk_fail(SK_ERR_UNSUPPORTED, "no panel kernel for L=%d R=%d", g.L, g.R);
        panel_kargs k;
        memset(&k, 0, sizeof k);
        k.samples = base->samples; k.samples_raw = base->samples_raw; k.stride = base->stride; k.off = base->off;
        k.prep = base->prep; k.nreads = base->nreads; k.xlay = (const double *)c->panel.p; k.mt = d_table + g.first;
        k.out = d_all; k.out_stride = out_stride;
        const int reads_per_block = 4 * (64 / g.L);
        const dim3 grid((base->nreads + reads_per_block - 1) / reads_per_block, g.count);
        hipLaunchKernelGGL(fn, grid, dim3(256), 0, c->stream, k);
        SK_HIP(hipGetLastError());
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
