// sk_api.hip -- the C-ABI entry points of include/squigglekit_hip.h.
// Host logic only: argument checks, scratch sizing, H2D / launches / D2H on the bound
// device's stream.  No arithmetic on sample data happens on the host.
#include "sk_common.h"
#include <math.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

int check_i16(const void *sig, int64_t stride, const int32_t *len, int32_t nreads)
{
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    if (nreads && (!sig || !len)) return sk_fail(SK_ERR_INVALID, "NULL sig/len");
    if (stride <= 0) return sk_fail(SK_ERR_INVALID, "stride must be positive");
    return SK_OK;
}

// host-buffer entry points: every len[r] must lie in [0, stride] -- the kernels use it as a trip count
// over the read's row (the *_dev_* entry points cannot look at device memory; the kernels clamp there)
int check_len_host(const int32_t *len, int32_t nreads, int64_t stride)
{
    for (int32_t r = 0; r < nreads; r++)
        if (len[r] < 0 || (int64_t)len[r] > stride)
            return sk_fail(SK_ERR_INVALID, "len[%d] = %d is outside [0, stride = %lld]", r, len[r], (long long)stride);
    return SK_OK;
}

int check_seg_params(const sk_seg_params *p)
{
    if (!p) return sk_fail(SK_ERR_INVALID, "NULL sk_seg_params");
    if (p->corrector < 0)
        return sk_fail(SK_ERR_INVALID, "corrector must be >= 0 (the reference divides by zero otherwise)");
    return SK_OK;
}

// clamp the outlier limits to what an int16 can hold (no sample can lie outside)
void clamp_limits(int32_t *lo, int32_t *hi)
{
    if (*lo < -32769) *lo = -32769;
    if (*hi > 32768) *hi = 32768;
}

__global__ void k_normalise_i16(const int16_t *__restrict__ comp, const sk_prep *__restrict__ prep,
                                double *__restrict__ out)
{
    const sk_prep pr = prep[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pr.n; i += gridDim.x * blockDim.x)
        out[i] = ((double)comp[i] - pr.center) / pr.scale;     // MotifSeq.py:199 / sklearn.scale
}

__global__ void k_normalise_f64(const double *__restrict__ comp, const sk_prep *__restrict__ prep,
                                double *__restrict__ out)
{
    const sk_prep pr = prep[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pr.n; i += gridDim.x * blockDim.x)
        out[i] = ((comp[i] - pr.center) - pr.top) / pr.scale - pr.bot;   // top / bot: sklearn's re-centring, 0 unless applied
}

// mlpy 3.5.0's subsequence() / subsequence_path() arithmetic restated LITERALLY, for inputs that hold inf / nan (medmad
// of a read whose MAD is 0, MotifSeq.py:196-199): `min3` is "m = a; if (b < m) m = b; if (c < m) m = c" and every
// comparison with a NaN is false, exactly as the C code behaves; np.argmin returns the first NaN.  The systolic kernels
// use v_min_f64, which drops NaNs -- they are never given such input (SK_FLAG_DEGENERATE).  One lane walks the whole
// matrix: this runs for the handful of degenerate reads `MotifSeq.py --strict-compat` prints.
__device__ __forceinline__ double cref_min3(double a, double b, double c)
{
    double m = a;
    if (b < m) m = b;
    if (c < m) m = c;
    return m;
}

__global__ void k_dtw_cref(const double *__restrict__ x, int n, const double *__restrict__ y, int m,
                           double *__restrict__ cost, sk_hit *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    cost[0] = fabs(x[0] - y[0]);
    for (int i = 1; i < n; i++) cost[(size_t)i * m] = fabs(x[i] - y[0]) + cost[(size_t)(i - 1) * m];
    for (int j = 1; j < m; j++) cost[j] = fabs(x[0] - y[j]);                       // free start
    for (int i = 1; i < n; i++) {
        const double *up = cost + (size_t)(i - 1) * m;
        double *row = cost + (size_t)i * m;
        for (int j = 1; j < m; j++) row[j] = fabs(x[i] - y[j]) + cref_min3(up[j], up[j - 1], row[j - 1]);
    }
    const double *last = cost + (size_t)(n - 1) * m;
    int idx = 0;                                                                    // np.argmin: first NaN, else first minimum
    double best = last[0];
    if (!(best != best))
        for (int j = 1; j < m; j++) {
            if (last[j] != last[j]) { idx = j; break; }
            if (last[j] < best) { best = last[j]; idx = j; }
        }
    int i = n - 1, j = idx;                                                         // subsequence_path: while i > 0
    while (i > 0) {
        if (j == 0) { i--; continue; }
        const double up = cost[(size_t)(i - 1) * m + j], dg = cost[(size_t)(i - 1) * m + j - 1], lf = cost[(size_t)i * m + j - 1];
        const double mc = cref_min3(up, dg, lf);
        if (dg == mc)      { i--; j--; }
        else if (lf == mc) { j--; }
        else               { i--; }
    }
    sk_hit h;
    h.dist = last[idx]; h.start = j; h.end = idx; h.n = m; h.flags = 0;
    out[0] = h;
}

// The host entry points move a large batch in sub-batches: the H2D copy of sub-batch k + 1 (second stream) runs
// under the kernels of sub-batch k.  Pageable caller memory: hipMemcpyAsync stages it and returns, the kernels
// launched before keep running meanwhile.  Memory from sk_host_alloc() (pinned): plain DMA at PCIe speed.
struct SubBatches {
    int32_t per = 0, n = 1;
};
SubBatches sub_batches(int32_t nreads, int64_t stride)
{
    SubBatches sb;
    int64_t target = (int64_t)256 << 20;                    // bytes of samples per sub-batch
    if (const char *e = sk_tune("SK_INGEST_MB")) { const long v = atol(e); if (v > 0) target = (int64_t)v << 20; }
    int64_t per = target / (stride * (int64_t)sizeof(int16_t));
    if (per < 4096) per = 4096;
    if (per * 2 > nreads) { sb.per = nreads; sb.n = 1; return sb; }
    sb.n = (int32_t)((nreads + per - 1) / per);
    sb.per = (int32_t)(((int64_t)nreads + sb.n - 1) / sb.n);
    return sb;
}

// The sub-batch loop: copies the host rows of each sub-batch of B to d_rows (and, when len is given, their lengths to
// c->len), then runs step(r0, nr, d_sig, d_len) -- the sub-batch's kernels on the main stream.
template <class Step>
int ingest_rows(sk_ctx *c, const SubBatches &B, int16_t *d_rows, const int16_t *sig, int64_t stride, const int32_t *len,
                int32_t nreads, Step step)
{
    int rc;
    if (B.n > 1 && (rc = sk_second_stream(c))) return rc;
    const hipStream_t cs = B.n > 1 ? c->stream2 : c->stream;
    for (int32_t bi = 0; bi < B.n; bi++) {
        const int32_t r0 = bi * B.per;
        const int32_t nr = (nreads - r0 < B.per) ? nreads - r0 : B.per;
        if (nr <= 0) break;
        int16_t *d_sig = d_rows + (size_t)r0 * (size_t)stride;
        int32_t *d_len = (int32_t *)c->len.p + r0;
        SK_HIP(hipMemcpyAsync(d_sig, sig + (size_t)r0 * (size_t)stride, (size_t)nr * (size_t)stride * sizeof(int16_t),
                              hipMemcpyHostToDevice, cs));
        if (len) SK_HIP(hipMemcpyAsync(d_len, len + r0, (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice, cs));
        if (B.n > 1) {                                      // the kernels of this sub-batch wait for its copy only
            SK_HIP(hipEventRecord(c->ev_chunk[bi & 7], cs));
            SK_HIP(hipStreamWaitEvent(c->stream, c->ev_chunk[bi & 7], 0));
        }
        if ((rc = step(r0, nr, d_sig, d_len))) return rc;
    }
    return SK_OK;
}

// The redo record (sk_ctx::redo) of a MotifSeq / segmenter call.  redo_forget drops the last call's (the int16
// MotifSeq calls write none); redo_begin does so and makes room for `lists` lists of `nreads` reads in all (one list
// per sub-batch); redo_list hands the next list, of nr reads, to the statistics route that fills it; redo_count sums
// the counters of the call if `route` wrote them, else -1.
void redo_forget(sk_ctx *c)
{
    c->redo_route = SK_REDO_NONE;
    c->redo_off.clear();
    c->redo_used = 0;
}

int redo_begin(sk_ctx *c, int32_t nreads, int32_t lists)
{
    redo_forget(c);
    return sk_reserve(c, &c->redo, ((size_t)nreads + 16 * (size_t)lists) * sizeof(int32_t));
}

int redo_list(sk_ctx *c, int route, int32_t nr, int32_t **list)
{
    const size_t end = c->redo_used + (size_t)nr + 16;
    if (end * sizeof(int32_t) > c->redo.cap) return sk_fail(SK_ERR_INVALID, "internal: redo list past its reservation");
    *list = (int32_t *)c->redo.p + c->redo_used;
    c->redo_used = end;
    c->redo_route = route;
    return SK_OK;
}

int redo_count(sk_ctx *c, int route)
{
    if (c->redo_route != route) return -1;
    SK_HIP(hipStreamSynchronize(c->stream));
    int total = 0;
    for (size_t o : c->redo_off) {
        int32_t v = 0;
        SK_HIP(hipMemcpy(&v, (const int32_t *)c->redo.p + o, sizeof v, hipMemcpyDeviceToHost));
        total += v;
    }
    return total;
}

// The checks every segmenter entry point makes after those of its input: parameters, max_segs, and -- when there are
// reads -- its outputs (null_out: one of them is NULL; `what` names them).  SK_NOTHING: no reads, nothing to do.
enum { SK_NOTHING = 1 };
int check_seg(const sk_seg_params *p, int32_t max_segs, int32_t nreads, bool null_out, const char *what)
{
    int rc = check_seg_params(p);
    if (rc) return rc;
    if (max_segs <= 0) return sk_fail(SK_ERR_INVALID, "max_segs must be positive");
    if (nreads == 0) return SK_NOTHING;
    if (null_out) return sk_fail(SK_ERR_INVALID, "NULL %s", what);
    return SK_OK;
}

// The tail of the segmenter batch entry points: segments (c->out) and counts (c->out2) back to the caller, then the
// check that no read has more than max_segs.
int read_segs(sk_ctx *c, int32_t nreads, int32_t max_segs, int32_t *segs, int32_t *nsegs)
{
    SK_HIP(hipMemcpyAsync(segs, c->out.p, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t), hipMemcpyDeviceToHost,
                          c->stream));
    SK_HIP(hipMemcpyAsync(nsegs, c->out2.p, (size_t)nreads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    for (int32_t r = 0; r < nreads; r++)
        if (nsegs[r] > max_segs)
            return sk_fail(SK_ERR_OVERFLOW, "read %d has %d segments, max_segs is %d", r, nsegs[r], max_segs);
    return SK_OK;
}

// ------------------------------------------------------------------ MotifSeq: what every family shares
int prep_mode(int32_t scale_mode) { return scale_mode == SK_SCALE_MEDMAD ? SK_PREP_MEDMAD : SK_PREP_ZSCALE; }

// Last step of the host-facing DTW entry points: the guard counters of the screening scheme (sk_last_dtw_guard) ride
// with the final synchronisation, and an alarm -- something that cannot happen in a healthy build -- is said out loud
// once per call (the records are right either way: the library redid the call with the exact pass).
int finish_dtw_host(sk_ctx *c)
{
    int32_t g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c->retry_dev && c->dtwcnt.p)
        SK_HIP(hipMemcpyAsync(g, (const int32_t *)c->dtwcnt.p + 8, sizeof g, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (g[4])
        fprintf(stderr, "squigglekit: DTW screening guard: %d premise violation(s), %d audit mismatch(es) of %d audited reads -- "
                        "the launch set(s) concerned and every later one of this call were %s by the exact pass; please report this\n",
                g[0], g[2], g[1], g[5] ? "redone" : "NOT redone");
    return SK_OK;
}

int check_multi(const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode)
{
    if (!motifs || !motif_off || nmotifs <= 0) return sk_fail(SK_ERR_INVALID, "no motifs");
    for (int32_t k = 0; k < nmotifs; k++)
        if (motif_off[k + 1] <= motif_off[k]) return sk_fail(SK_ERR_INVALID, "motif %d is empty", k);
    if (scale_mode != SK_SCALE_MEDMAD && scale_mode != SK_SCALE_ZSCALE)
        return sk_fail(SK_ERR_INVALID, "unknown scale mode %d", scale_mode);
    return SK_OK;
}

// Stage a ragged float64 batch: samples -> c->sig, zero-based offsets -> c->off.
// Returns the total sample count in *total and the longest read in *maxlen.
// centi: `sig` holds int32 centi-units (sk_tsv_parse_centi) -- half the bytes over PCIe; the float64 image
// (c / 100.0 = float("ddd.dd"), sk_synth.hip k_centi_to_f64) is made on the device, and what follows is the same.
int stage_ragged_f64(sk_ctx *c, const void *sig_any, const int64_t *off, int32_t nreads, int64_t *total, int64_t *maxlen,
                     bool centi = false)
{
    const double *sig = (const double *)sig_any;
    if (!sig || !off) return sk_fail(SK_ERR_INVALID, "NULL sig/off");
    std::vector<int64_t> rel((size_t)nreads + 1);
    int64_t mx = 0;
    for (int32_t r = 0; r <= nreads; r++) rel[r] = off[r] - off[0];
    for (int32_t r = 0; r < nreads; r++) {
        const int64_t n = rel[r + 1] - rel[r];
        if (n < 0 || n > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "bad length for read %d", r);
        if (n > mx) mx = n;
    }
    *total = rel[nreads];
    *maxlen = mx;
    int rc;
    if ((rc = sk_reserve(c, &c->sig, (size_t)(*total > 0 ? *total : 1) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->off, rel.size() * sizeof(int64_t)))) return rc;
    if (centi) {
        if ((rc = sk_reserve(c, &c->misc, (size_t)(*total > 0 ? *total : 1) * sizeof(int32_t) + 16))) return rc;
        SK_HIP(hipMemcpyAsync(c->misc.p, (const int32_t *)sig_any + off[0], (size_t)*total * sizeof(int32_t),
                              hipMemcpyHostToDevice, c->stream));
        if ((rc = sk_launch_centi_to_f64(c, (const int32_t *)c->misc.p, *total, (double *)c->sig.p))) return rc;
    } else
        SK_HIP(hipMemcpyAsync(c->sig.p, sig + off[0], (size_t)*total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->off.p, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));        // rel goes out of scope
    return SK_OK;
}

// The two prepare helpers, one per input kind: filter + statistics of one (sub-)batch on the device between ev[0] and
// ev[1], and that batch as the DTW launchers take it -- *a gets feed, samples (+ samples_raw), stride / off, prep,
// nreads and max_len, with last_row, force_single and fuse cleared; motif, out and accumulate are the caller's.
//
// int16 rows.  d_comp / d_prep: where this (sub-)batch's filtered samples / statistics go.  fz: nullptr, or room for
// the fused prologue where the caller allows it: when it applies (sk_sdtw_fuse_ok: medmad with the usual limits,
// zscale on short rows) nothing is launched here, a->fuse = fz, and filter + statistics ride in the screening pass of
// the first sk_launch_sdtw (sk_sdtwq.hip; it runs them as a kernel of their own when it does not take the screening
// scheme).  ev0_set: the caller has recorded ev[0] already (the panel: its gather lies inside the interval).
int prep_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nr, int32_t scale_mode,
             int32_t scale_low, int32_t scale_hi, int16_t *d_comp, sk_prep *d_prep, sk_prep_fuse *fz, bool ev0_set,
             sk_sdtw_args *a)
{
    const int mode = prep_mode(scale_mode);
    const bool fuse = fz && sk_sdtw_fuse_ok(scale_low, scale_hi, mode, stride);
    if (!ev0_set) SK_HIP(hipEventRecord(c->ev[0], c->stream));
    if (fuse) {
        fz->raw = d_sig; fz->len = d_len; fz->lo = scale_low; fz->hi = scale_hi; fz->mode = mode;
    } else {
        const int rc = sk_launch_prep_i16(c, d_sig, stride, d_len, nr, scale_low, scale_hi, mode, 0.0, d_comp, d_prep,
                                          nullptr, 0);
        if (rc) return rc;
    }
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    a->feed = SK_FEED_I16; a->samples = d_comp; a->samples_raw = nullptr; a->stride = stride; a->off = nullptr;
    a->prep = d_prep; a->nreads = nr; a->max_len = stride; a->last_row = nullptr; a->force_single = 0;
    a->fuse = fuse ? fz : nullptr;
    return SK_OK;
}

// A staged ragged float64 batch (d_sig / d_off: zero based, nreads + 1): normalisation terms to c->prep, filtered
// samples to c->comp (reads the filter left whole are not copied: SK_IFLAG_INPLACE, read from samples_raw).
int prep_f64(sk_ctx *c, const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t maxlen,
             int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_sdtw_args *a)
{
    int rc;
    if ((rc = sk_reserve(c, &c->comp, (size_t)(total > 0 ? total : 1) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    if (scale_mode == SK_SCALE_MEDMAD && sk_f64_fast_applies(maxlen, 1.0)) {
        // streaming statistics (sk_f64stat.hip), then the general kernel over the (almost always empty) list of reads
        // whose median / MAD bin it could not resolve
        int32_t *retry;
        if ((rc = redo_list(c, SK_REDO_F64, nreads, &retry))) return rc;
        c->redo_off.push_back((size_t)(retry - (int32_t *)c->redo.p));
        rc = sk_launch_f64_stats(c, d_sig, d_off, nullptr, nreads, maxlen, (double)scale_low, (double)scale_hi, SK_PREP_MEDMAD,
                                 0.0, (sk_prep *)c->prep.p, nullptr, 0, nullptr, retry, (double *)c->comp.p);
        if (rc) return rc;
        rc = sk_launch_prep_f64_listed(c, d_sig, d_off, retry + 1, retry, nreads < 2 * c->num_cu ? nreads : 2 * c->num_cu,
                                       (double)scale_low, (double)scale_hi, SK_PREP_MEDMAD, 0.0, (double *)c->comp.p, 0,
                                       (sk_prep *)c->prep.p, nullptr, 0);
    } else {
        rc = sk_launch_prep_f64(c, d_sig, d_off, nreads, (double)scale_low, (double)scale_hi, prep_mode(scale_mode), 0.0,
                                (double *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0);
    }
    if (rc) return rc;
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    a->feed = SK_FEED_F64_NORM; a->samples = c->comp.p; a->samples_raw = d_sig; a->stride = 0; a->off = d_off;
    a->prep = (const sk_prep *)c->prep.p; a->nreads = nreads; a->max_len = maxlen; a->last_row = nullptr;
    a->force_single = 0; a->fuse = nullptr;
    return SK_OK;
}

// ------------------------------------------------------------------ MotifSeq first match
// scale_outliers + medmad / zscale + dtw_subsequence (MotifSeq.py:186-200, 436-439): one record per read and motif.
// Several motifs against the same reads (the `for name in m_order` loop of :436) share one filter + statistics pass;
// a single-motif entry point is the same call with a two-element motif_off on its stack.
struct fm_req {
    const double  *motifs;          // motif k = motifs[motif_off[k] .. motif_off[k + 1])
    const int32_t *motif_off;
    int32_t        nmotifs;
    int32_t        scale_mode, scale_low, scale_hi;
    sk_hit        *out;             // [nmotifs][nreads]: device memory for a *_dev_* entry point, else host memory
};
// the request of an entry point from its parameters (all eight name scaling and out alike)
#define FM_REQ(motifs, motif_off, nmotifs) fm_req{motifs, motif_off, nmotifs, scale_mode, scale_low, scale_hi, out}

// after the checks of the input.  Without reads out may be NULL.
int fm_check(const fm_req &q, int32_t nreads)
{
    const int rc = check_multi(q.motifs, q.motif_off, q.nmotifs, q.scale_mode);
    if (rc) return rc;
    if (nreads && !q.out) return sk_fail(SK_ERR_INVALID, "NULL out");
    return SK_OK;
}

// One prepared (sub-)batch (a: from a prepare helper): one DTW launch set per motif, motif k's records to
// d_out + k * out_stride.  The first launch set of a call starts the retry total, every other one (later_batch: of a
// later sub-batch) adds to it; a fused prologue runs with the first motif, the later ones find samples and statistics
// in place.
int fm_core(sk_ctx *c, sk_sdtw_args a, const fm_req &q, sk_hit *d_out, int64_t out_stride, bool later_batch)
{
    for (int32_t k = 0; k < q.nmotifs; k++) {
        a.motif = q.motifs + q.motif_off[k]; a.nmotif = q.motif_off[k + 1] - q.motif_off[k];
        a.out = d_out + (size_t)k * (size_t)out_stride;
        a.accumulate = (later_batch || k > 0) ? 1 : 0;
        if (k > 0) a.fuse = nullptr;
        const int rc = sk_launch_sdtw(c, &a);
        if (rc) return rc;
    }
    c->ev_valid = true;
    return SK_OK;
}

// The four bodies, one per input.  Device-resident int16 rows: q.out is the caller's device buffer.
int fm_dev_i16(fm_req q, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads)
{
    SK_ENTER(c);
    int rc;
    if ((rc = check_i16(d_sig, stride, d_len, nreads)) || (rc = fm_check(q, nreads))) return rc;
    if (nreads == 0) return SK_OK;
    clamp_limits(&q.scale_low, &q.scale_hi);
    redo_forget(c);
    if ((rc = sk_reserve(c, &c->comp, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    sk_prep_fuse fz;
    sk_sdtw_args a;
    if ((rc = prep_i16(c, d_sig, stride, d_len, nreads, q.scale_mode, q.scale_low, q.scale_hi, (int16_t *)c->comp.p,
                       (sk_prep *)c->prep.p, &fz, false, &a))) return rc;
    return fm_core(c, a, q, q.out, nreads, false);
}

// int16 rows in host memory, in sub-batches (ingest_rows).  whole: c->comp / c->prep hold the filtered samples and
// statistics of the whole call, each sub-batch at its reads' place, as the hit family lays them out; otherwise every
// sub-batch reuses the room of one.  sk_motifseq_batch_i16 is the one entry point that asks for the latter, and it
// has to: its batches go up to 1 M x 4 000 samples, where the whole-call layout would cost 8 GB more.  It also
// answers an empty batch before it looks at the motif, as it always has.
int fm_host_i16(fm_req q, const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, bool whole)
{
    SK_ENTER(c);
    int rc;
    if ((rc = check_i16(sig, stride, len, nreads)) || (rc = check_len_host(len, nreads, stride))) return rc;
    if (nreads == 0 && !whole) return SK_OK;
    if ((rc = fm_check(q, nreads))) return rc;
    if (nreads == 0) return SK_OK;
    clamp_limits(&q.scale_low, &q.scale_hi);
    const SubBatches B = sub_batches(nreads, stride);
    const size_t rows = whole ? nreads : B.per, ob = (size_t)nreads * (size_t)q.nmotifs * sizeof(sk_hit);
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, rows * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, rows * sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->out, ob))) return rc;
    redo_forget(c);
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         const size_t at = whole ? r0 : 0;
                         sk_prep_fuse fz;
                         sk_sdtw_args a;
                         const int rc = prep_i16(c, d_sig, stride, d_len, nr, q.scale_mode, q.scale_low, q.scale_hi,
                                                 (int16_t *)c->comp.p + at * (size_t)stride, (sk_prep *)c->prep.p + at,
                                                 &fz, false, &a);
                         return rc ? rc : fm_core(c, a, q, (sk_hit *)c->out.p + r0, nreads, r0 > 0);
                     });
    if (rc) return rc;
    SK_HIP(hipMemcpyAsync(q.out, c->out.p, ob, hipMemcpyDeviceToHost, c->stream));
    return finish_dtw_host(c);
}

// ragged float64 reads in host memory (pA TSV / BLOW5 in pA): read r = sig[off[r] .. off[r+1]), staged once.  centi:
// int32 centi-units, made float64 on the device (stage_ragged_f64)
int fm_ragged(fm_req q, const void *sig, bool centi, const int64_t *off, int32_t nreads)
{
    SK_ENTER(c);
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = fm_check(q, nreads);
    if (rc) return rc;
    if (nreads == 0) return SK_OK;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, sig, off, nreads, &total, &maxlen, centi))) return rc;
    const size_t ob = (size_t)nreads * (size_t)q.nmotifs * sizeof(sk_hit);
    if ((rc = sk_reserve(c, &c->out, ob))) return rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    sk_sdtw_args a;
    if ((rc = prep_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, total, maxlen, q.scale_mode,
                       q.scale_low, q.scale_hi, &a))) return rc;
    if ((rc = fm_core(c, a, q, (sk_hit *)c->out.p, nreads, false))) return rc;
    SK_HIP(hipMemcpyAsync(q.out, c->out.p, ob, hipMemcpyDeviceToHost, c->stream));
    return finish_dtw_host(c);
}

// the same batch already on the device: d_sig / d_off (zero based, nreads + 1) and q.out are device pointers
int fm_dev_f64(fm_req q, const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t max_len)
{
    SK_ENTER(c);
    if (nreads < 0 || total < 0 || max_len < 0 || max_len > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "bad sizes");
    int rc = fm_check(q, nreads);
    if (rc) return rc;
    if (nreads == 0) return SK_OK;
    if (!d_sig || !d_off) return sk_fail(SK_ERR_INVALID, "NULL sig/off");
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    sk_sdtw_args a;
    if ((rc = prep_f64(c, d_sig, d_off, nreads, total, max_len, q.scale_mode, q.scale_low, q.scale_hi, &a))) return rc;
    return fm_core(c, a, q, q.out, nreads, false);
}


// ------------------------------------------------------------------ MotifSeq hit lists (sk_hits.hip)
// Up to K disjoint matches per read and motif instead of the first argmin only (MotifSeq.py:437-439 keeps that one;
// view_region, :506-513, plots the whole last row they come from).  Reads are prepared once (filter + statistics, the
// kernels of the default path); per motif, chunks of reads go through the exact pass that stores the last rows
// (MODE_ROWS; the chained pass beyond 1 024 points) and k_hits_select.  The row buffer (12 B per column) is capped at
// 2 GiB (SK_HITS_ROW_BYTES) and reused chunk after chunk, motif after motif.
//
// On top of the hit lists a call may return, in any combination:
//   read background (sk_bg.hip)   the statistics of each read's whole last row, bg [nmotifs][nreads];
//   alignment paths (sk_path.hip) per hit the spans of its warping path: which columns [a_i, b_i] each motif point i
//                                 covers (mlpy's subsequence_path, MotifSeq.py:437, as a fixed-size record).  Motif k's
//                                 block of `spans` begins at 2 * max_hits * nreads * motif_off[k] int32, inside it
//                                 [read][hit][N_k][2];
//   events (sk_events.hip)        one sk_event per motif point where the paths have a span: the same layout with one
//                                 record where the spans have two ints.  Events are made from spans: a call that
//                                 returns events and no spans keeps its spans in c->pathspans.
// A call that asks for none of them launches and reserves nothing for them.
struct hits_out {
    sk_hit    *out;                 // [nmotifs][nreads][max_hits]
    int32_t   *count;               // [nmotifs][nreads]
    sk_bg_rec *bg;
    int32_t   *spans;
    sk_event  *events;
};
enum { HITS_BG = 1, HITS_SPANS = 2, HITS_EVENTS = 4 };
struct hits_req {
    const double  *motifs;          // motif k = motifs[motif_off[k] .. motif_off[k + 1])
    const int32_t *motif_off;
    int32_t        nmotifs;
    int32_t        scale_mode, scale_low, scale_hi, max_hits;
    double         max_dist;
    hits_out       to;              // the caller's buffers: device memory for a *_dev_* entry point, else host memory
    int            want;            // HITS_*: what the entry point promises besides out / count (the rest of `to` is ignored)
};
// the request of an entry point from its parameters -- all sixteen name them alike -- and what it adds to the hit lists
#define HITS_REQ(want, bg, spans, events)                                                                             \
    hits_req{motifs, motif_off, nmotifs, scale_mode, scale_low, scale_hi, max_hits, max_dist,                         \
             {out, count, bg, spans, events}, want}

// after the checks of the input.  Without reads the outputs may be NULL -- bg excepted (squigglekit_hip.h).
int hits_check(const hits_req &q, int32_t nreads)
{
    const int rc = check_multi(q.motifs, q.motif_off, q.nmotifs, q.scale_mode);
    if (rc) return rc;
    if (q.max_hits < 1 || q.max_hits > 64) return sk_fail(SK_ERR_INVALID, "max_hits %d outside 1..64", q.max_hits);
    if (q.max_dist != q.max_dist) return sk_fail(SK_ERR_INVALID, "max_dist is NaN");
    if (nreads && (!q.to.out || !q.to.count)) return sk_fail(SK_ERR_INVALID, "NULL out/count");
    if ((q.want & HITS_BG) && !q.to.bg) return sk_fail(SK_ERR_INVALID, "NULL bg");
    if (nreads && (q.want & HITS_SPANS) && !q.to.spans) return sk_fail(SK_ERR_INVALID, "NULL spans");
    if (nreads && (q.want & HITS_EVENTS) && !q.to.events) return sk_fail(SK_ERR_INVALID, "NULL events");
    return SK_OK;
}

// what a call that makes paths needs before its first launch: the mismatch counter zeroed (sk_path_begin) and its
// motifs, flat, on the device
int paths_begin(sk_ctx *c, const double *motifs, const int32_t *motif_off, int32_t nmotifs)
{
    int rc = sk_path_begin(c);
    if (rc) return rc;
    const size_t mb = (size_t)motif_off[nmotifs] * sizeof(double);
    if ((rc = sk_reserve(c, &c->pathmotif, mb))) return rc;
    SK_HIP(hipMemcpyAsync(c->pathmotif.p, motifs + motif_off[0], mb, hipMemcpyHostToDevice, c->stream));
    return SK_OK;
}

// how every body opens once its input is checked: hits_check, then paths_begin if it applies (also without reads)
int hits_begin(sk_ctx *c, const hits_req &q, int32_t nreads)
{
    const int rc = hits_check(q, nreads);
    if (rc || !(q.want & (HITS_SPANS | HITS_EVENTS))) return rc;
    return paths_begin(c, q.motifs, q.motif_off, q.nmotifs);
}

struct hits_sizes { size_t out, count, bg, spans, events; };      // bytes of a call's outputs
hits_sizes hits_bytes(const hits_req &q, int32_t nreads)
{
    const size_t lists = (size_t)nreads * (size_t)q.nmotifs;
    const size_t points = (size_t)q.max_hits * (size_t)nreads * (size_t)(q.motif_off[q.nmotifs] - q.motif_off[0]);
    return {lists * (size_t)q.max_hits * sizeof(sk_hit), lists * sizeof(int32_t), lists * sizeof(sk_bg_rec),
            points * 2 * sizeof(int32_t), points * sizeof(sk_event)};
}

// host entry points: room on the device for what the request names (d: where; nullptr for the rest) ...
int hits_reserve(sk_ctx *c, const hits_req &q, const hits_sizes &z, hits_out *d)
{
    const bool bg = q.want & HITS_BG, events = q.want & HITS_EVENTS, spans = events || (q.want & HITS_SPANS);
    int rc;
    if ((rc = sk_reserve(c, &c->out, z.out))) return rc;
    if ((rc = sk_reserve(c, &c->out2, z.count))) return rc;
    if (bg && (rc = sk_reserve(c, &c->bgrec, z.bg))) return rc;
    if (spans && (rc = sk_reserve(c, &c->pathspans, z.spans))) return rc;
    if (events && (rc = sk_reserve(c, &c->events, z.events))) return rc;
    *d = {(sk_hit *)c->out.p, (int32_t *)c->out2.p, bg ? (sk_bg_rec *)c->bgrec.p : nullptr,
          spans ? (int32_t *)c->pathspans.p : nullptr, events ? (sk_event *)c->events.p : nullptr};
    return SK_OK;
}

// ... and, after the launches, those outputs back to the caller
int hits_copy_back(sk_ctx *c, const hits_req &q, const hits_sizes &z, const hits_out &d)
{
    SK_HIP(hipMemcpyAsync(q.to.out, d.out, z.out, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(q.to.count, d.count, z.count, hipMemcpyDeviceToHost, c->stream));
    if (q.want & HITS_BG) SK_HIP(hipMemcpyAsync(q.to.bg, d.bg, z.bg, hipMemcpyDeviceToHost, c->stream));
    if (q.want & HITS_SPANS) SK_HIP(hipMemcpyAsync(q.to.spans, d.spans, z.spans, hipMemcpyDeviceToHost, c->stream));
    if (q.want & HITS_EVENTS) SK_HIP(hipMemcpyAsync(q.to.events, d.events, z.events, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// One prepared (sub-)batch.  base: feed, samples (+ samples_raw), stride / off, prep, max_len and nreads of prepared
// reads.  d: the call's outputs on the device, laid out for the out_reads reads of the whole call (bg / spans / events:
// nullptr = not made; events need spans); read0: the (sub-)batch's first read among them.  Motif k's records of read r
// go to d.out[(k * out_reads + read0 + r) * K ..], its count and its row's statistics (k_row_background) to
// [k * out_reads + read0 + r], its spans and events into motif k's block (above) from read read0 + r on.
int hits_core(sk_ctx *c, const sk_sdtw_args &base, const hits_req &q, const hits_out &d, int64_t out_reads, int64_t read0)
{
    const int32_t K = q.max_hits;
    const int64_t row_stride = base.max_len > 0 ? base.max_len : 1;
    const size_t per_read = sizeof(sk_hit) + (size_t)row_stride * (sizeof(double) + sizeof(int32_t));
    size_t budget = (size_t)2 << 30;
    if (const char *e = sk_tune("SK_HITS_ROW_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
    int64_t chunk = (int64_t)(budget / per_read);
    if (chunk < 1) chunk = 1;
    if (chunk > base.nreads) chunk = base.nreads;
    int rc = sk_reserve(c, &c->hitrows, (size_t)chunk * per_read);
    if (rc) return rc;
    sk_hit *rec = (sk_hit *)c->hitrows.p;
    double *rowD = (double *)(rec + chunk);
    int32_t *rowS = (int32_t *)(rowD + (size_t)chunk * row_stride);
    for (int32_t k = 0; k < q.nmotifs; k++) {
        for (int64_t r0 = 0; r0 < base.nreads; r0 += chunk) {
            sk_sdtw_args a = base;
            a.nreads = (int32_t)(base.nreads - r0 < chunk ? base.nreads - r0 : chunk);
            a.prep = base.prep + r0;
            if (base.feed == SK_FEED_I16) a.samples = (const int16_t *)base.samples + r0 * base.stride;
            else a.off = base.off + r0;
            a.motif = q.motifs + q.motif_off[k]; a.nmotif = q.motif_off[k + 1] - q.motif_off[k];
            a.out = rec; a.last_row = nullptr; a.force_single = 1; a.accumulate = 0; a.fuse = nullptr;
            if ((rc = sk_launch_sdtw_rows(c, &a, rowD, rowS))) return rc;
            const int64_t o = (int64_t)k * out_reads + read0 + r0;
            if (d.bg && (rc = sk_launch_row_background(c, rowD, row_stride, rec, a.nreads, d.bg + o))) return rc;
            if ((rc = sk_launch_hits_select(c, rowD, rowS, row_stride, rec, a.nreads, K, q.max_dist, d.out + o * K,
                                            d.count + o))) return rc;
        }
    }
    c->retry_dev = false;                               // (no screening counters: finish_dtw_host reads none)
    c->ev_valid = true;
    for (int32_t k = 0; d.spans && k < q.nmotifs; k++) {
        const int64_t m0 = q.motif_off[k] - q.motif_off[0], N = q.motif_off[k + 1] - q.motif_off[k];
        const int64_t at = (int64_t)K * out_reads * m0 + read0 * K * N;      // in motif points
        sk_path_args p;
        p.feed = base.feed; p.samples = base.samples; p.samples_raw = base.samples_raw; p.stride = base.stride;
        p.off = base.off; p.prep = base.prep; p.nreads = base.nreads; p.max_len = base.max_len;
        p.d_motif = (const double *)c->pathmotif.p + m0; p.nmotif = (int32_t)N;
        p.hits = d.out + ((int64_t)k * out_reads + read0) * K; p.K = K;
        p.spans = d.spans + 2 * at;
        if ((rc = sk_launch_paths(c, &p))) return rc;
        if (d.events && (rc = sk_launch_events(c, &p, d.events + at))) return rc;
    }
    return SK_OK;
}

// Reads [read0, read0 + nr) of a call on int16 rows, on the device: filter + statistics (the kernels of the default path)
// into their rows of c->comp / c->prep, then the core.
int hits_rows_i16(sk_ctx *c, const hits_req &q, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nr,
                  const hits_out &d, int64_t out_reads, int64_t read0)
{
    sk_sdtw_args a;
    const int rc = prep_i16(c, d_sig, stride, d_len, nr, q.scale_mode, q.scale_low, q.scale_hi,
                            (int16_t *)c->comp.p + (size_t)read0 * (size_t)stride, (sk_prep *)c->prep.p + read0, nullptr,
                            false, &a);
    return rc ? rc : hits_core(c, a, q, d, out_reads, read0);
}

// The three bodies, one per input kind.  Device-resident int16 rows: the outputs are the caller's device buffers.
int hits_dev_i16(hits_req q, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads)
{
    SK_ENTER(c);
    int rc;
    if ((rc = check_i16(d_sig, stride, d_len, nreads)) || (rc = hits_begin(c, q, nreads))) return rc;
    if (nreads == 0) return SK_OK;
    clamp_limits(&q.scale_low, &q.scale_hi);
    redo_forget(c);
    if ((rc = sk_reserve(c, &c->comp, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    hits_out d = {q.to.out, q.to.count, (q.want & HITS_BG) ? q.to.bg : nullptr, (q.want & HITS_SPANS) ? q.to.spans : nullptr,
                  (q.want & HITS_EVENTS) ? q.to.events : nullptr};
    if (d.events && !d.spans) {
        if ((rc = sk_reserve(c, &c->pathspans, hits_bytes(q, nreads).spans))) return rc;
        d.spans = (int32_t *)c->pathspans.p;
    }
    return hits_rows_i16(c, q, d_sig, stride, d_len, nreads, d, nreads, 0);
}

// int16 rows in host memory; sub-batches and the whole-call layout of c->comp / c->prep as fm_host_i16.  Every sub-batch writes its reads' places in
// the outputs of the whole call, so these come back in one piece.
int hits_host_i16(hits_req q, const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads)
{
    SK_ENTER(c);
    int rc;
    if ((rc = check_i16(sig, stride, len, nreads)) || (rc = check_len_host(len, nreads, stride)) ||
        (rc = hits_begin(c, q, nreads))) return rc;
    if (nreads == 0) return SK_OK;
    clamp_limits(&q.scale_low, &q.scale_hi);
    const hits_sizes z = hits_bytes(q, nreads);
    const size_t sb = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    hits_out d;
    if ((rc = sk_reserve(c, &c->sig, sb))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, sb))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if ((rc = hits_reserve(c, q, z, &d))) return rc;
    redo_forget(c);
    rc = ingest_rows(c, sub_batches(nreads, stride), (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return hits_rows_i16(c, q, d_sig, stride, d_len, nr, d, nreads, r0);
                     });
    if (rc) return rc;
    return hits_copy_back(c, q, z, d);
}

// ragged float64 reads (pA TSV / BLOW5 in pA): read r = sig[off[r] .. off[r+1]).  centi: int32 centi-units, made
// float64 on the device (stage_ragged_f64)
int hits_ragged(hits_req q, const void *sig, bool centi, const int64_t *off, int32_t nreads)
{
    SK_ENTER(c);
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = hits_begin(c, q, nreads);
    if (rc) return rc;
    if (nreads == 0) return SK_OK;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, sig, off, nreads, &total, &maxlen, centi))) return rc;
    const hits_sizes z = hits_bytes(q, nreads);
    hits_out d;
    if ((rc = hits_reserve(c, q, z, &d))) return rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    sk_sdtw_args a;
    if ((rc = prep_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, total, maxlen, q.scale_mode,
                       q.scale_low, q.scale_hi, &a))) return rc;
    if ((rc = hits_core(c, a, q, d, nreads, 0))) return rc;
    return hits_copy_back(c, q, z, d);
}

} // namespace

extern "C" {

// ------------------------------------------------------------------ pinned host memory for callers
void *sk_host_alloc(size_t bytes)
{
    sk_entry entry;
    if (!entry.c) return nullptr;
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        sk_fail(SK_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

int sk_host_free(void *p)
{
    if (p) SK_HIP(hipHostFree(p));
    return SK_OK;
}

// ------------------------------------------------------------------ MotifSeq first match: the entry points
// *_dev_*: every buffer is device memory.  Multi-motif forms: out is [nmotifs][nreads].
int sk_motifseq_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                        const double *motif, int32_t nmotif, int32_t scale_mode,
                        int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    const int32_t motif_off[2] = {0, nmotif};
    return fm_dev_i16(FM_REQ(motif, motif_off, 1), d_sig, stride, d_len, nreads);
}
int sk_motifseq_multi_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                              int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    return fm_dev_i16(FM_REQ(motifs, motif_off, nmotifs), d_sig, stride, d_len, nreads);
}
int sk_motifseq_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const double *motif, int32_t nmotif, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    const int32_t motif_off[2] = {0, nmotif};
    return fm_host_i16(FM_REQ(motif, motif_off, 1), sig, stride, len, nreads, false);
}
int sk_motifseq_multi_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                                const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    return fm_host_i16(FM_REQ(motifs, motif_off, nmotifs), sig, stride, len, nreads, true);
}
int sk_motifseq_batch_f64(const double *sig, const int64_t *off, int32_t nreads,
                          const double *motif, int32_t nmotif, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    const int32_t motif_off[2] = {0, nmotif};
    return fm_ragged(FM_REQ(motif, motif_off, 1), sig, false, off, nreads);
}
int sk_motifseq_multi_batch_f64(const double *sig, const int64_t *off, int32_t nreads,
                                const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    return fm_ragged(FM_REQ(motifs, motif_off, nmotifs), sig, false, off, nreads);
}
int sk_motifseq_multi_batch_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                                  const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                                  int32_t scale_mode, int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    return fm_ragged(FM_REQ(motifs, motif_off, nmotifs), centi, true, off, nreads);
}
int sk_motifseq_dev_f64(const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t max_len,
                        const double *motif, int32_t nmotif, int32_t scale_mode,
                        int32_t scale_low, int32_t scale_hi, sk_hit *out)
{
    const int32_t motif_off[2] = {0, nmotif};
    return fm_dev_f64(FM_REQ(motif, motif_off, 1), d_sig, d_off, nreads, total, max_len);
}


// The entry points: hit lists, then their twins with the read background, the alignment paths, the events.  *_dev_i16:
// every buffer is device memory.
int sk_motifseq_hits_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                             int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                             int32_t *count)
{
    return hits_dev_i16(HITS_REQ(0, nullptr, nullptr, nullptr), d_sig, stride, d_len, nreads);
}
int sk_motifseq_hits_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                         int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                         int32_t *count)
{
    return hits_host_i16(HITS_REQ(0, nullptr, nullptr, nullptr), sig, stride, len, nreads);
}
int sk_motifseq_hits_f64(const double *sig, const int64_t *off, int32_t nreads,
                         const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                         int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                         int32_t *count)
{
    return hits_ragged(HITS_REQ(0, nullptr, nullptr, nullptr), sig, false, off, nreads);
}
int sk_motifseq_hits_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count)
{
    return hits_ragged(HITS_REQ(0, nullptr, nullptr, nullptr), centi, true, off, nreads);
}

int sk_motifseq_background_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                                   const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                                   int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                                   int32_t *count, sk_bg_rec *bg)
{
    return hits_dev_i16(HITS_REQ(HITS_BG, bg, nullptr, nullptr), d_sig, stride, d_len, nreads);
}
int sk_motifseq_background_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                               int32_t *count, sk_bg_rec *bg)
{
    return hits_host_i16(HITS_REQ(HITS_BG, bg, nullptr, nullptr), sig, stride, len, nreads);
}
int sk_motifseq_background_f64(const double *sig, const int64_t *off, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                               int32_t *count, sk_bg_rec *bg)
{
    return hits_ragged(HITS_REQ(HITS_BG, bg, nullptr, nullptr), sig, false, off, nreads);
}
int sk_motifseq_background_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                                 const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                                 int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                                 int32_t *count, sk_bg_rec *bg)
{
    return hits_ragged(HITS_REQ(HITS_BG, bg, nullptr, nullptr), centi, true, off, nreads);
}

int sk_motifseq_paths_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                              int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                              int32_t *count, int32_t *spans)
{
    return hits_dev_i16(HITS_REQ(HITS_SPANS, nullptr, spans, nullptr), d_sig, stride, d_len, nreads);
}
int sk_motifseq_paths_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                          int32_t *count, int32_t *spans)
{
    return hits_host_i16(HITS_REQ(HITS_SPANS, nullptr, spans, nullptr), sig, stride, len, nreads);
}
int sk_motifseq_paths_f64(const double *sig, const int64_t *off, int32_t nreads,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                          int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                          int32_t *count, int32_t *spans)
{
    return hits_ragged(HITS_REQ(HITS_SPANS, nullptr, spans, nullptr), sig, false, off, nreads);
}
int sk_motifseq_paths_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                            const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                            int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                            int32_t *count, int32_t *spans)
{
    return hits_ragged(HITS_REQ(HITS_SPANS, nullptr, spans, nullptr), centi, true, off, nreads);
}

int sk_motifseq_events_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                               const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                               int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                               int32_t *count, sk_event *events)
{
    return hits_dev_i16(HITS_REQ(HITS_EVENTS, nullptr, nullptr, events), d_sig, stride, d_len, nreads);
}
int sk_motifseq_events_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count, sk_event *events)
{
    return hits_host_i16(HITS_REQ(HITS_EVENTS, nullptr, nullptr, events), sig, stride, len, nreads);
}
int sk_motifseq_events_f64(const double *sig, const int64_t *off, int32_t nreads,
                           const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                           int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                           int32_t *count, sk_event *events)
{
    return hits_ragged(HITS_REQ(HITS_EVENTS, nullptr, nullptr, events), sig, false, off, nreads);
}
int sk_motifseq_events_centi(const int32_t *centi, const int64_t *off, int32_t nreads,
                             const double *motifs, const int32_t *motif_off, int32_t nmotifs, int32_t scale_mode,
                             int32_t scale_low, int32_t scale_hi, int32_t max_hits, double max_dist, sk_hit *out,
                             int32_t *count, sk_event *events)
{
    return hits_ragged(HITS_REQ(HITS_EVENTS, nullptr, nullptr, events), centi, true, off, nreads);
}

// ------------------------------------------------------------------ pooled events (sk_events.hip)
// c->pool: the result [N] (host form), then the count, the mask (host form), the list of selected hits
static int pool_core(sk_ctx *c, const sk_event *d_ev, const uint8_t *use, bool use_on_host, int64_t nhits, int32_t N,
                     sk_pool_rec *d_out, sk_pool_rec *host_out)
{
    const size_t rb = ((size_t)N * sizeof(sk_pool_rec) + 15) & ~(size_t)15;
    const size_t ub = ((size_t)(use && use_on_host ? nhits : 0) + 15) & ~(size_t)15;
    int rc = sk_reserve(c, &c->pool, rb + 16 + ub + (size_t)(nhits > 0 ? nhits : 1) * sizeof(int32_t));
    if (rc) return rc;
    char *base = (char *)c->pool.p;
    int32_t *d_cnt = (int32_t *)(base + rb);
    uint8_t *d_use = (uint8_t *)(base + rb + 16);
    int32_t *d_idx = (int32_t *)(base + rb + 16 + ub);
    if (use && use_on_host) SK_HIP(hipMemcpyAsync(d_use, use, (size_t)nhits, hipMemcpyHostToDevice, c->stream));
    const uint8_t *mask = !use ? nullptr : (use_on_host ? d_use : use);
    if (!d_out) d_out = (sk_pool_rec *)base;
    if ((rc = sk_launch_events_pool(c, d_ev, mask, nhits, N, d_idx, d_cnt, d_out))) return rc;
    if (host_out) SK_HIP(hipMemcpyAsync(host_out, d_out, (size_t)N * sizeof(sk_pool_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

static int check_pool(const void *ev, int64_t nhits, int32_t N, const void *out)
{
    if (nhits < 0 || nhits > 0x7fff0000) return sk_fail(SK_ERR_INVALID, "nhits %lld outside 0..2147418112", (long long)nhits);
    if (N < 1) return sk_fail(SK_ERR_INVALID, "N < 1");
    if (!out || (nhits && !ev)) return sk_fail(SK_ERR_INVALID, "NULL ev/out");
    return SK_OK;
}

int sk_events_pool(const sk_event *ev, const uint8_t *use, int64_t nhits, int32_t N, sk_pool_rec *out)
{
    SK_ENTER(c);
    int rc = check_pool(ev, nhits, N, out);
    if (rc) return rc;
    const size_t eb = (size_t)nhits * (size_t)N * sizeof(sk_event);
    if ((rc = sk_reserve(c, &c->poolev, eb ? eb : 16))) return rc;
    if (eb) SK_HIP(hipMemcpyAsync(c->poolev.p, ev, eb, hipMemcpyHostToDevice, c->stream));
    return pool_core(c, (const sk_event *)c->poolev.p, use, true, nhits, N, nullptr, out);
}

int sk_events_pool_dev(const sk_event *d_ev, const uint8_t *d_use, int64_t nhits, int32_t N, sk_pool_rec *d_out)
{
    SK_ENTER(c);
    const int rc = check_pool(d_ev, nhits, N, d_out);
    if (rc) return rc;
    return pool_core(c, d_ev, d_use, false, nhits, N, d_out, nullptr);
}

// hits of the last paths call whose path failed the self-check (window corner == dist bit for bit, a_0 == start,
// b_{N-1} == end) and got spans -1; a healthy build reports 0.  -1: no paths call yet on this context.
int sk_last_path_mismatches(void)
{
    SK_ENTER(c);
    if (!c->path_valid || !c->pathcnt.p) return -1;
    SK_HIP(hipStreamSynchronize(c->stream));
    int32_t v = 0;
    SK_HIP(hipMemcpy(&v, c->pathcnt.p, sizeof v, hipMemcpyDeviceToHost));
    return v;
}

// ------------------------------------------------------------------ mlpy boundary (pre-normalised f64)
int sk_dtw_subsequence_batch(const double *x, int32_t nx, const double *y, const int64_t *off,
                             int32_t nreads, sk_hit *out)
{
    SK_ENTER(c);
    if (nreads < 0 || nx <= 0 || !x) return sk_fail(SK_ERR_INVALID, "bad query");
    if (nreads == 0) return SK_OK;
    if (!y || !off || !out) return sk_fail(SK_ERR_INVALID, "NULL y/off/out");
    const int64_t total = off[nreads] - off[0];
    if (total < 0) return sk_fail(SK_ERR_INVALID, "offsets not increasing");
    int64_t maxlen = 0;
    for (int32_t r = 0; r < nreads; r++) {
        const int64_t n = off[r + 1] - off[r];
        if (n < 0 || n > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "bad length for read %d", r);
        if (n > maxlen) maxlen = n;
    }
    int rc;
    if ((rc = sk_reserve(c, &c->sig, (size_t)(total > 0 ? total : 1) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->off, (size_t)(nreads + 1) * sizeof(int64_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, (size_t)nreads * sizeof(sk_hit)))) return rc;
    std::vector<int64_t> rel((size_t)nreads + 1);
    for (int32_t r = 0; r <= nreads; r++) rel[r] = off[r] - off[0];
    SK_HIP(hipMemcpyAsync(c->sig.p, y + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->off.p, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));        // rel is about to go out of scope
    sk_sdtw_args a;
    a.feed = SK_FEED_F64_RAW; a.samples = c->sig.p; a.stride = 0; a.off = (const int64_t *)c->off.p;
    a.prep = nullptr; a.nreads = nreads; a.motif = x; a.nmotif = nx; a.out = (sk_hit *)c->out.p;
    a.last_row = nullptr; a.max_len = maxlen; a.force_single = 0;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    if ((rc = sk_launch_sdtw(c, &a))) return rc;
    c->ev_valid = true;
    SK_HIP(hipMemcpyAsync(out, c->out.p, (size_t)nreads * sizeof(sk_hit), hipMemcpyDeviceToHost, c->stream));
    if ((rc = finish_dtw_host(c))) return rc;
    return SK_OK;
}

// ------------------------------------------------------------------ DTW over a pair list (sk_pairs.hip)
int sk_dtw_pairs_dev(const double *d_values, const int64_t *off, int32_t nseq,
                     const sk_pair *pairs, int64_t npairs, int32_t mode, sk_hit *d_out)
{
    SK_ENTER(c);
    return sk_pairs_run(c, d_values, off, 0, nseq, pairs, npairs, mode, d_out);
}

int sk_dtw_pairs(const double *values, const int64_t *off, int32_t nseq,
                 const sk_pair *pairs, int64_t npairs, int32_t mode, sk_hit *out)
{
    SK_ENTER(c);
    int rc;
    if ((rc = sk_pairs_check(off, nseq, pairs, npairs, mode, out))) return rc;   // before anything is copied or launched
    if (npairs == 0) return SK_OK;
    if (!values) return sk_fail(SK_ERR_INVALID, "NULL values");
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] < off[s]) return sk_fail(SK_ERR_INVALID, "offsets not increasing at sequence %d", s);
    const int64_t total = nseq ? off[nseq] - off[0] : 0;
    const size_t vb = (((size_t)(total > 0 ? total : 1) * sizeof(double)) + 15) & ~(size_t)15;
    if ((rc = sk_reserve(c, &c->pairsval, vb + (size_t)npairs * sizeof(sk_hit)))) return rc;
    double *d_values = (double *)c->pairsval.p;
    sk_hit *d_out = (sk_hit *)((char *)c->pairsval.p + vb);
    if (total > 0)
        SK_HIP(hipMemcpyAsync(d_values, values + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_pairs_run(c, d_values, off, nseq ? off[0] : 0, nseq, pairs, npairs, mode, d_out))) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, (size_t)npairs * sizeof(sk_hit), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// ... and the warping paths of the list (sk_pairpath.hip): spans [sum N][2], pair after pair
int sk_dtw_pairs_paths_dev(const double *d_values, const int64_t *off, int32_t nseq,
                           const sk_pair *pairs, int64_t npairs, int32_t mode,
                           sk_hit *d_records, int32_t have_records, int32_t *d_spans)
{
    SK_ENTER(c);
    return sk_pair_paths_run(c, d_values, off, 0, nseq, pairs, npairs, mode, d_records, have_records, d_spans);
}

int sk_dtw_pairs_paths(const double *values, const int64_t *off, int32_t nseq,
                       const sk_pair *pairs, int64_t npairs, int32_t mode,
                       sk_hit *records, int32_t have_records, int32_t *spans)
{
    SK_ENTER(c);
    int rc;
    if ((rc = sk_pairs_check(off, nseq, pairs, npairs, mode, records))) return rc;   // before anything is copied or launched
    if (!spans) return sk_fail(SK_ERR_INVALID, "NULL spans");
    if (npairs == 0) return SK_OK;
    if (!values) return sk_fail(SK_ERR_INVALID, "NULL values");
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] < off[s]) return sk_fail(SK_ERR_INVALID, "offsets not increasing at sequence %d", s);
    int64_t rows = 0;
    for (int64_t p = 0; p < npairs; p++) rows += off[pairs[p].query + 1] - off[pairs[p].query];
    const int64_t total = nseq ? off[nseq] - off[0] : 0;
    const size_t vb = (((size_t)(total > 0 ? total : 1) * sizeof(double)) + 15) & ~(size_t)15;
    const size_t sb = (size_t)rows * 2 * sizeof(int32_t);
    if ((rc = sk_reserve(c, &c->pairsval, vb + (size_t)npairs * sizeof(sk_hit)))) return rc;
    if ((rc = sk_reserve(c, &c->pathspans, sb))) return rc;
    double *d_values = (double *)c->pairsval.p;
    sk_hit *d_rec = (sk_hit *)((char *)c->pairsval.p + vb);
    int32_t *d_spans = (int32_t *)c->pathspans.p;
    if (total > 0)
        SK_HIP(hipMemcpyAsync(d_values, values + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (have_records)
        SK_HIP(hipMemcpyAsync(d_rec, records, (size_t)npairs * sizeof(sk_hit), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_pair_paths_run(c, d_values, off, nseq ? off[0] : 0, nseq, pairs, npairs, mode, d_rec, have_records, d_spans)))
        return rc;
    if (!have_records)
        SK_HIP(hipMemcpyAsync(records, d_rec, (size_t)npairs * sizeof(sk_hit), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(spans, d_spans, sb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// the tiers of the last sk_dtw_pairs_paths* call on this context: pairs left to the scratch tier, bytes of one slab,
// wavefronts of the scratch launch (all 0 when every pair fitted the LDS tier)
int sk_last_pair_paths_tiers(int64_t *listed, int64_t *slab_bytes, int64_t *waves)
{
    SK_ENTER(c);
    if (listed) *listed = c->pairpath_listed;
    if (slab_bytes) *slab_bytes = c->pairpath_slab_bytes;
    if (waves) *waves = c->pairpath_waves;
    return SK_OK;
}

// ------------------------------------------------------------------ hit lists over a pair list (sk_pairs.hip, sk_pairhits.hip)
// hits_check's rules for max_hits and max_dist, with its words
static int check_hit_limits(int32_t max_hits, double max_dist)
{
    if (max_hits < 1 || max_hits > 64) return sk_fail(SK_ERR_INVALID, "max_hits %d outside 1..64", max_hits);
    if (max_dist != max_dist) return sk_fail(SK_ERR_INVALID, "max_dist is NaN");
    return SK_OK;
}

// what the arguments alone decide, before a context is looked for: sk_pairs_check's rules, then the hit lists'
static int check_pairs_hits(const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs, int32_t max_hits,
                            double max_dist, const void *out, const void *count)
{
    int rc;
    if ((rc = sk_pairs_check(off, nseq, pairs, npairs, SK_PAIRS_SUBSEQUENCE, off))) return rc;   // (out and count: below)
    if ((rc = check_hit_limits(max_hits, max_dist))) return rc;
    if (npairs && (!out || !count)) return sk_fail(SK_ERR_INVALID, "NULL out/count");
    return SK_OK;
}

int sk_dtw_pairs_hits_dev(const double *d_values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                          int32_t max_hits, double max_dist, sk_hit *d_out, int32_t *d_count)
{
    int rc;
    if ((rc = check_pairs_hits(off, nseq, pairs, npairs, max_hits, max_dist, d_out, d_count))) return rc;
    if (npairs == 0) return SK_OK;
    if (!d_values) return sk_fail(SK_ERR_INVALID, "NULL values");
    SK_ENTER(c);
    return sk_pairs_hits_run(c, d_values, off, 0, nseq, pairs, npairs, max_hits, max_dist, d_out, d_count);
}

int sk_dtw_pairs_hits(const double *values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                      int32_t max_hits, double max_dist, sk_hit *out, int32_t *count)
{
    int rc;
    if ((rc = check_pairs_hits(off, nseq, pairs, npairs, max_hits, max_dist, out, count))) return rc;
    if (npairs == 0) return SK_OK;
    if (!values) return sk_fail(SK_ERR_INVALID, "NULL values");
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] < off[s]) return sk_fail(SK_ERR_INVALID, "offsets not increasing at sequence %d", s);
    SK_ENTER(c);
    const int64_t total = nseq ? off[nseq] - off[0] : 0;
    const size_t vb = (((size_t)(total > 0 ? total : 1) * sizeof(double)) + 15) & ~(size_t)15;
    const size_t ob = (size_t)npairs * (size_t)max_hits * sizeof(sk_hit), cb = (size_t)npairs * sizeof(int32_t);
    if ((rc = sk_reserve(c, &c->pairsval, vb + ob + cb))) return rc;
    double *d_values = (double *)c->pairsval.p;
    sk_hit *d_out = (sk_hit *)((char *)c->pairsval.p + vb);
    int32_t *d_count = (int32_t *)((char *)d_out + ob);
    if (total > 0)
        SK_HIP(hipMemcpyAsync(d_values, values + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_pairs_hits_run(c, d_values, off, off[0], nseq, pairs, npairs, max_hits, max_dist, d_out, d_count))) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(count, d_count, cb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// the last sk_dtw_pairs_hits* / sk_map_hits* call on this context: bytes of last rows selected from at a time, slices of
// the pair list (1 for a session), rows that took the long tier
int sk_last_pair_hits_plan(int64_t *row_bytes, int64_t *slices, int64_t *long_rows)
{
    SK_ENTER(c);
    if (row_bytes) *row_bytes = c->pairhits_row_bytes;
    if (slices) *slices = c->pairhits_slices;
    if (long_rows) *long_rows = c->pairhits_long_rows;
    return SK_OK;
}

// ------------------------------------------------------------------ adaptive-band DTW over a pair list (sk_band.hip)
// The argument checks run before the context is looked at: a refused call names its reason on any machine.
int sk_dtw_band_dev(const double *d_values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                    int32_t band, int32_t end_mode, sk_hit *d_records, int32_t *d_spans)
{
    if (int rc = sk_band_check(off, nseq, pairs, npairs, band, end_mode, d_records)) return rc;
    SK_ENTER(c);
    return sk_band_run(c, d_values, off, 0, nseq, pairs, npairs, band, end_mode, d_records, d_spans);
}

int sk_dtw_band(const double *values, const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs,
                int32_t band, int32_t end_mode, sk_hit *records, int32_t *spans)
{
    int rc;
    if ((rc = sk_band_check(off, nseq, pairs, npairs, band, end_mode, records))) return rc;
    if (npairs > 0) {
        if (!values) return sk_fail(SK_ERR_INVALID, "NULL values");
        for (int32_t s = 0; s < nseq; s++)
            if (off[s + 1] < off[s]) return sk_fail(SK_ERR_INVALID, "offsets not increasing at sequence %d", s);
    }
    SK_ENTER(c);
    if (npairs == 0) return SK_OK;
    int64_t rows = 0;
    for (int64_t p = 0; p < npairs; p++) rows += off[pairs[p].query + 1] - off[pairs[p].query];
    const int64_t total = nseq ? off[nseq] - off[0] : 0;
    const size_t vb = (((size_t)(total > 0 ? total : 1) * sizeof(double)) + 15) & ~(size_t)15;
    const size_t sb = (size_t)rows * 2 * sizeof(int32_t);
    if ((rc = sk_reserve(c, &c->pairsval, vb + (size_t)npairs * sizeof(sk_hit)))) return rc;
    if (spans && (rc = sk_reserve(c, &c->pathspans, sb))) return rc;
    double *d_values = (double *)c->pairsval.p;
    sk_hit *d_rec = (sk_hit *)((char *)c->pairsval.p + vb);
    int32_t *d_spans = spans ? (int32_t *)c->pathspans.p : nullptr;
    if (total > 0)
        SK_HIP(hipMemcpyAsync(d_values, values + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_band_run(c, d_values, off, off[0], nseq, pairs, npairs, band, end_mode, d_rec, d_spans))) return rc;
    SK_HIP(hipMemcpyAsync(records, d_rec, (size_t)npairs * sizeof(sk_hit), hipMemcpyDeviceToHost, c->stream));
    if (spans) SK_HIP(hipMemcpyAsync(spans, d_spans, sb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// the plan of the last sk_dtw_band* call on this context: bytes of one slab (0: records only), wavefronts, the longest
// listed pair's bands
int sk_last_band_plan(int64_t *slab_bytes, int64_t *waves, int64_t *steps_max)
{
    SK_ENTER(c);
    if (slab_bytes) *slab_bytes = c->band_slab_bytes;
    if (waves) *waves = c->band_waves;
    if (steps_max) *steps_max = c->band_steps;
    return SK_OK;
}

int sk_dtw_subsequence(const double *x, int32_t nx, const double *y, int32_t ny,
                       double *dist, int32_t *start, int32_t *end, double *cost_last_row)
{
    SK_ENTER(c);
    if (!x || !y || nx <= 0 || ny <= 0) return sk_fail(SK_ERR_INVALID, "empty x or y");
    int rc;
    if ((rc = sk_reserve(c, &c->sig, (size_t)ny * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->off, 2 * sizeof(int64_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, sizeof(sk_hit)))) return rc;
    if (cost_last_row && (rc = sk_reserve(c, &c->misc, (size_t)ny * sizeof(double)))) return rc;
    const int64_t rel[2] = {0, ny};
    SK_HIP(hipMemcpyAsync(c->sig.p, y, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->off.p, rel, sizeof rel, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    sk_sdtw_args a;
    a.feed = SK_FEED_F64_RAW; a.samples = c->sig.p; a.stride = 0; a.off = (const int64_t *)c->off.p;
    a.prep = nullptr; a.nreads = 1; a.motif = x; a.nmotif = nx; a.out = (sk_hit *)c->out.p;
    a.last_row = cost_last_row ? (double *)c->misc.p : nullptr;
    a.max_len = ny; a.force_single = 1;
    if ((rc = sk_launch_sdtw(c, &a))) return rc;
    sk_hit h;
    SK_HIP(hipMemcpyAsync(&h, c->out.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (cost_last_row)
        SK_HIP(hipMemcpyAsync(cost_last_row, c->misc.p, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (dist) *dist = h.dist;
    if (start) *start = h.start;
    if (end) *end = h.end;
    return SK_OK;
}

// One already-normalised pair with the path of its match: dist / start / end as sk_dtw_subsequence, spans [nx][2]
// (mlpy's path: (i, j) for j = spans[i][0] .. spans[i][1], i ascending).  All -1: no path (NaN distance).
int sk_dtw_subsequence_path(const double *x, int32_t nx, const double *y, int32_t ny,
                            double *dist, int32_t *start, int32_t *end, int32_t *spans)
{
    SK_ENTER(c);
    if (!x || !y || nx <= 0 || ny <= 0) return sk_fail(SK_ERR_INVALID, "empty x or y");
    const int32_t moff[2] = {0, nx};
    if (!spans) return sk_fail(SK_ERR_INVALID, "NULL spans");
    int rc = paths_begin(c, x, moff, 1);
    if (rc) return rc;
    if ((rc = sk_reserve(c, &c->sig, (size_t)ny * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->off, 2 * sizeof(int64_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, sizeof(sk_hit)))) return rc;
    if ((rc = sk_reserve(c, &c->pathspans, (size_t)nx * 2 * sizeof(int32_t)))) return rc;
    const int64_t rel[2] = {0, ny};
    SK_HIP(hipMemcpyAsync(c->sig.p, y, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->off.p, rel, sizeof rel, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    sk_sdtw_args a;
    a.feed = SK_FEED_F64_RAW; a.samples = c->sig.p; a.stride = 0; a.off = (const int64_t *)c->off.p;
    a.prep = nullptr; a.nreads = 1; a.motif = x; a.nmotif = nx; a.out = (sk_hit *)c->out.p;
    a.last_row = nullptr; a.max_len = ny; a.force_single = 1;
    if ((rc = sk_launch_sdtw(c, &a))) return rc;
    sk_path_args p;
    p.feed = a.feed; p.samples = a.samples; p.off = a.off; p.nreads = 1; p.max_len = ny;
    p.d_motif = (const double *)c->pathmotif.p; p.nmotif = nx; p.hits = (const sk_hit *)c->out.p; p.K = 1;
    p.spans = (int32_t *)c->pathspans.p;
    if ((rc = sk_launch_paths(c, &p))) return rc;
    sk_hit h;
    SK_HIP(hipMemcpyAsync(&h, c->out.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(spans, c->pathspans.p, (size_t)nx * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (dist) *dist = h.dist;
    if (start) *start = h.start;
    if (end) *end = h.end;
    return SK_OK;
}

int sk_normalise_i16(const int16_t *sig, int32_t len, int32_t scale_mode,
                     int32_t scale_low, int32_t scale_hi, double *out, int32_t *n_out)
{
    SK_ENTER(c);
    if (len < 0 || (len && (!sig || !out))) return sk_fail(SK_ERR_INVALID, "bad arguments");
    if (scale_mode != SK_SCALE_MEDMAD && scale_mode != SK_SCALE_ZSCALE)
        return sk_fail(SK_ERR_INVALID, "unknown scale mode %d", scale_mode);
    if (len == 0) { if (n_out) *n_out = 0; return SK_OK; }
    clamp_limits(&scale_low, &scale_hi);
    const int64_t stride = ((int64_t)len + 7) & ~7ll;
    int rc;
    if ((rc = sk_reserve(c, &c->sig, (size_t)stride * 2))) return rc;
    if ((rc = sk_reserve(c, &c->len, sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, (size_t)stride * 2))) return rc;
    if ((rc = sk_reserve(c, &c->prep, sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->misc, (size_t)len * sizeof(double)))) return rc;
    SK_HIP(hipMemcpyAsync(c->sig.p, sig, (size_t)len * 2, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->len.p, &len, sizeof len, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    rc = sk_launch_prep_i16(c, (const int16_t *)c->sig.p, stride, (const int32_t *)c->len.p, 1, scale_low,
                            scale_hi, prep_mode(scale_mode), 0.0,
                            (int16_t *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_normalise_i16, dim3(64), dim3(256), 0, c->stream, (const int16_t *)c->comp.p,
                       (const sk_prep *)c->prep.p, (double *)c->misc.p);
    SK_HIP(hipGetLastError());
    sk_prep pr;
    SK_HIP(hipMemcpyAsync(&pr, c->prep.p, sizeof pr, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (pr.n > 0)
        SK_HIP(hipMemcpy(out, c->misc.p, (size_t)pr.n * sizeof(double), hipMemcpyDeviceToHost));
    if (n_out) *n_out = pr.n;
    return SK_OK;
}

int sk_normalise_f64(const double *sig, int32_t len, int32_t scale_mode,
                     int32_t scale_low, int32_t scale_hi, double *out, int32_t *n_out)
{
    SK_ENTER(c);
    if (len < 0 || (len && (!sig || !out))) return sk_fail(SK_ERR_INVALID, "bad arguments");
    if (scale_mode != SK_SCALE_MEDMAD && scale_mode != SK_SCALE_ZSCALE)
        return sk_fail(SK_ERR_INVALID, "unknown scale mode %d", scale_mode);
    if (len == 0) { if (n_out) *n_out = 0; return SK_OK; }
    const int64_t off[2] = {0, len};
    int64_t total, maxlen;
    int rc = stage_ragged_f64(c, sig, off, 1, &total, &maxlen);
    if (rc) return rc;
    if ((rc = sk_reserve(c, &c->comp, (size_t)len * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->misc, (size_t)len * sizeof(double)))) return rc;
    rc = sk_launch_prep_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, 1, (double)scale_low,
                            (double)scale_hi, prep_mode(scale_mode),
                            0.0, (double *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_normalise_f64, dim3(64), dim3(256), 0, c->stream, (const double *)c->comp.p,
                       (const sk_prep *)c->prep.p, (double *)c->misc.p);
    SK_HIP(hipGetLastError());
    sk_prep pr;
    SK_HIP(hipMemcpyAsync(&pr, c->prep.p, sizeof pr, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (pr.n > 0)
        SK_HIP(hipMemcpy(out, c->misc.p, (size_t)pr.n * sizeof(double), hipMemcpyDeviceToHost));
    if (n_out) *n_out = pr.n;
    return SK_OK;
}

// ------------------------------------------------------------------ segmenter
} // extern "C"

// device-resident core of the int16 segmenter path (d_segs zeroed here)
static int segment_dev_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                           const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                           int *row16_out = nullptr)
{
    int rc;
    int32_t lo = p->lim_low, hi = p->lim_hi;
    clamp_limits(&lo, &hi);
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    // slots past nsegs[r] read as zero, whatever the buffer held before
    SK_HIP(hipMemsetAsync(d_segs, 0, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t), c->stream));
    if (sk_segment_fast_applies(d_sig, stride, lo, hi, p->std_scale)) {
        // streaming statistics (sk_segstat.hip): reads of up to 4 096 samples, exact integer sums, certified
        // integer thresholds; the numpy-order kernel redoes the (almost always empty) list of uncertified reads
        const size_t mb = (size_t)nreads * (size_t)sk_segment_fast_row16(stride) * 16;
        if (row16_out) *row16_out = sk_segment_fast_row16(stride);
        if ((rc = sk_reserve(c, &c->mask, mb))) return rc;
        int32_t *redo;
        if ((rc = redo_list(c, SK_REDO_I16, nreads, &redo))) return rc;
        rc = sk_launch_segment_fast(c, d_sig, stride, d_len, nreads, p, lo, hi, (sk_prep *)c->prep.p, c->mask.p,
                                    redo, d_segs, d_nsegs, max_segs);
        if (rc) return rc;
        c->ev_valid = true;
        return SK_OK;
    }
    // the numpy-order kernel for every read: it writes the streaming path's {in band, kept} entries, the same walk follows
    const int row16 = (int)((stride + 63) / 64);
    if (row16_out) *row16_out = row16;
    if ((rc = sk_reserve(c, &c->comp, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)row16 * 16))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    rc = sk_launch_prep_i16(c, d_sig, stride, d_len, nreads, lo, hi, SK_PREP_SEGMENT, p->std_scale,
                            (int16_t *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0, 0, 0x7fffffff, nullptr, nullptr,
                            c->mask.p, row16);
    if (rc) return rc;
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    rc = sk_launch_seg_walk_masks(c, c->mask.p, row16, d_len, nreads, p, d_segs, d_nsegs, max_segs);
    if (rc) return rc;
    c->ev_valid = true;
    return SK_OK;
}

// The statistics and masks of the float64 segmenter path (d_off zero based): {in band, kept} entries in c->mask (*row16
// per read) and each read's raw length in c->len.  Records ev[0] .. ev[1].  d_zero (bytes): zeroed first, on the stream.
static int segment_masks_f64(sk_ctx *c, const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total,
                             int64_t maxlen, int32_t lim_low, int32_t lim_hi, double std_scale, const int32_t *d_rlen,
                             int *row16_out, void *d_zero = nullptr, size_t zero_bytes = 0)
{
    int rc;
    // streaming statistics with certified comparisons (sk_f64stat.hip) and the numpy-order kernel over the (almost
    // always empty) list of uncertified reads -- or, outside the streaming kernel's range, the numpy-order kernel for
    // every read.  Either writes {in band, kept} entries and raw lengths; the run-hopping walk of the int16 path follows.
    const bool fast = sk_f64_fast_applies(maxlen, std_scale);
    const int row16 = sk_f64_row16(maxlen > 0 ? maxlen : 1);
    *row16_out = row16;
    const int grid = nreads < 2 * c->num_cu ? nreads : 2 * c->num_cu;
    const int64_t srow = (maxlen + 7) & ~(int64_t)7;
    // compacted samples: one scratch row per workgroup of the listed redo, or every read's
    const size_t cb = fast ? (size_t)grid * (size_t)(srow > 0 ? srow : 8) * sizeof(double)
                           : (size_t)(total > 0 ? total : 1) * sizeof(double);
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)row16 * 16))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, cb))) return rc;
    int32_t *retry = nullptr;
    if (fast) {
        if ((rc = redo_list(c, SK_REDO_F64, nreads, &retry))) return rc;
        c->redo_off.push_back((size_t)(retry - (int32_t *)c->redo.p));
    }
    if (d_zero) SK_HIP(hipMemsetAsync(d_zero, 0, zero_bytes, c->stream));
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    if (fast) {
        rc = sk_launch_f64_stats(c, d_sig, d_off, d_rlen, nreads, maxlen, (double)lim_low, (double)lim_hi, SK_PREP_SEGMENT,
                                 std_scale, (sk_prep *)c->prep.p, c->mask.p, row16, (int32_t *)c->len.p, retry, nullptr);
        if (rc) return rc;
        rc = sk_launch_prep_f64_listed(c, d_sig, d_off, retry + 1, retry, grid, (double)lim_low, (double)lim_hi,
                                       SK_PREP_SEGMENT, std_scale, (double *)c->comp.p, srow, (sk_prep *)c->prep.p,
                                       c->mask.p, row16, d_rlen);
    } else {
        rc = sk_launch_prep_f64(c, d_sig, d_off, nreads, (double)lim_low, (double)lim_hi, SK_PREP_SEGMENT,
                                std_scale, (double *)c->comp.p, (sk_prep *)c->prep.p, c->mask.p, row16,
                                (int32_t *)c->len.p, d_rlen);
    }
    if (rc) return rc;
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    return SK_OK;
}

// device-resident core of the float64 segmenter path (d_off zero based; d_segs zeroed here)
static int segment_dev_f64(sk_ctx *c, const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total,
                           int64_t maxlen, const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                           const int32_t *d_rlen = nullptr, int *row16_out = nullptr)
{
    int row16;
    int rc = segment_masks_f64(c, d_sig, d_off, nreads, total, maxlen, p->lim_low, p->lim_hi, p->std_scale, d_rlen, &row16,
                               d_segs, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t));
    if (rc) return rc;
    if (row16_out) *row16_out = row16;
    rc = sk_launch_seg_walk_masks(c, c->mask.p, row16, (const int32_t *)c->len.p, nreads, p, d_segs, d_nsegs, max_segs);
    if (rc) return rc;
    c->ev_valid = true;
    return SK_OK;
}

// Device-resident core.  Since round 6 the values stay int16: the pA conversion is a monotone map of the sample, so
// limits, median, std and the two thresholds are found in the raw domain (k_seg_stats<.., PA>, sk_segstat.hip: 2 bytes a
// sample instead of 8; reads it cannot certify are redone from their float64 values in numpy's order).  Rows the
// streaming kernel does not take (stride not a multiple of 8, unaligned): the float64 image of every row, then the
// float64 segmenter path -- what every call did before round 6.
static int segment_dev_i16_pa(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const double *d_cal2, const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    int rc;
    if (sk_segment_pa_applies(d_sig, stride, p->std_scale)) {
        const size_t mb = (size_t)nreads * (size_t)sk_segment_fast_row16(stride) * 16;
        if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
        if ((rc = sk_reserve(c, &c->mask, mb))) return rc;
        if ((rc = sk_reserve(c, &c->comp, (size_t)c->num_cu * (size_t)stride * sizeof(double)))) return rc;
        int32_t *redo;
        if ((rc = redo_list(c, SK_REDO_PA, nreads, &redo))) return rc;
        SK_HIP(hipMemsetAsync(d_segs, 0, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t), c->stream));
        rc = sk_launch_segment_fast(c, d_sig, stride, d_len, nreads, p, p->lim_low, p->lim_hi, (sk_prep *)c->prep.p, c->mask.p,
                                    redo, d_segs, d_nsegs, max_segs, d_cal2, (double *)c->comp.p);
        if (rc) return rc;
        c->ev_valid = true;
        return SK_OK;
    }
    // every read in a slot of `stride` doubles; the cut to len[r] is the float64 path's per-read length
    const int64_t total = (int64_t)nreads * stride;
    c->pa_off_host.resize((size_t)nreads + 1);
    for (int32_t r = 0; r <= nreads; r++) c->pa_off_host[r] = (int64_t)r * stride;
    if ((rc = sk_reserve(c, &c->sig, (size_t)(total > 0 ? total : 1) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->off, c->pa_off_host.size() * sizeof(int64_t)))) return rc;
    SK_HIP(hipMemcpyAsync(c->off.p, c->pa_off_host.data(), c->pa_off_host.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));                 // (the vector may be resized by the next call)
    rc = sk_launch_rows_to_pa(c, d_sig, stride, nreads, (const int64_t *)c->off.p, d_cal2, (double *)c->sig.p);
    if (rc) return rc;
    return segment_dev_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, total, stride, p,
                           d_segs, d_nsegs, max_segs, d_len);
}

// ------------------------------------------------------------------ segment levels
// What the levels entry points add to their segmenter twin: where the records go.  `on` distinguishes "not asked for"
// (the plain segmenter entry points: both NULL) from a NULL the caller must not pass.
struct levels_req {
    bool          on = false;
    sk_seg_level *levels = nullptr;       // [nreads][max_segs]: host (the batch entry points) or device (_dev)
    sk_seg_level *read_level = nullptr;   // [nreads]
};
static levels_req levels_of(sk_seg_level *levels, sk_seg_level *read_level)
{
    levels_req q;
    q.on = true; q.levels = levels; q.read_level = read_level;
    return q;
}

// The records of nr reads whose segmenter route has just run on the stream (entries in c->mask, row16 per read):
// d_levels / d_read_level are device pointers.
static int levels_launch(sk_ctx *c, int feed, const void *d_samples, int64_t stride, const int64_t *d_off, int row16,
                         const int32_t *d_len, int64_t mmax, int32_t nr, const int32_t *d_segs, const int32_t *d_nsegs,
                         int32_t max_segs, sk_seg_level *d_levels, sk_seg_level *d_read_level)
{
    int rc;
    if ((rc = sk_reserve(c, &c->seglevwork, sk_seglev_work_bytes(c, nr, max_segs, mmax)))) return rc;
    return sk_launch_seg_levels(c, feed, d_samples, stride, d_off, c->mask.p, row16, d_len, mmax, nr, d_segs, d_nsegs,
                                max_segs, c->seglevwork.p, d_levels, d_read_level);
}

// host entry points: room for the records of the whole call in c->seglev, and their way back (before read_segs: an
// overflowing call returns its truncated records like its truncated segs)
static int levels_reserve(sk_ctx *c, const levels_req &q, int32_t nreads, int32_t max_segs)
{
    if (!q.on) return SK_OK;
    return sk_reserve(c, &c->seglev, (size_t)nreads * ((size_t)max_segs + 1) * sizeof(sk_seg_level));
}
static sk_seg_level *levels_dev(sk_ctx *c, int32_t r0, int32_t max_segs) { return (sk_seg_level *)c->seglev.p + (size_t)r0 * (size_t)max_segs; }
static sk_seg_level *read_level_dev(sk_ctx *c, int32_t nreads, int32_t r0, int32_t max_segs)
{
    return (sk_seg_level *)c->seglev.p + (size_t)nreads * (size_t)max_segs + r0;
}
static int levels_copy_back(sk_ctx *c, const levels_req &q, int32_t nreads, int32_t max_segs)
{
    if (!q.on) return SK_OK;
    SK_HIP(hipMemcpyAsync(q.levels, levels_dev(c, 0, max_segs), (size_t)nreads * (size_t)max_segs * sizeof(sk_seg_level),
                          hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(q.read_level, read_level_dev(c, nreads, 0, max_segs), (size_t)nreads * sizeof(sk_seg_level),
                          hipMemcpyDeviceToHost, c->stream));
    return SK_OK;
}

// int16 rows on the device: the segmenter route, then (when asked for) the records
static int levels_rows_i16(sk_ctx *c, const levels_req &q, const int16_t *d_sig, int64_t stride, const int32_t *d_len,
                           int32_t nr, const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                           sk_seg_level *d_levels, sk_seg_level *d_read_level)
{
    int row16 = 0;
    int rc = segment_dev_i16(c, d_sig, stride, d_len, nr, p, d_segs, d_nsegs, max_segs, &row16);
    if (rc || !q.on) return rc;
    return levels_launch(c, SK_FEED_I16, d_sig, stride, nullptr, row16, d_len, stride, nr, d_segs, d_nsegs, max_segs,
                         d_levels, d_read_level);
}

static int segment_host_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const sk_seg_params *p,
                            int32_t *segs, int32_t *nsegs, int32_t max_segs, const levels_req &q)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (!rc) rc = check_len_host(len, nreads, stride);
    if (!rc) rc = check_seg(p, max_segs, nreads, !segs || !nsegs, "segs/nsegs");
    if (!rc && q.on && (!q.levels || !q.read_level)) rc = sk_fail(SK_ERR_INVALID, "NULL levels/read_level");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    const SubBatches B = sub_batches(nreads, stride);
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out2, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = levels_reserve(c, q, nreads, max_segs))) return rc;
    if ((rc = redo_begin(c, nreads, B.n))) return rc;
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return levels_rows_i16(c, q, d_sig, stride, d_len, nr, p,
                                                (int32_t *)c->out.p + (size_t)r0 * 2 * (size_t)max_segs, (int32_t *)c->out2.p + r0,
                                                max_segs, q.on ? levels_dev(c, r0, max_segs) : nullptr,
                                                q.on ? read_level_dev(c, nreads, r0, max_segs) : nullptr);
                     });
    if (rc) return rc;
    if ((rc = levels_copy_back(c, q, nreads, max_segs))) return rc;
    return read_segs(c, nreads, max_segs, segs, nsegs);
}

static int segment_batch_ragged(const void *sig, bool centi, const int64_t *off, const int32_t *len, int32_t nreads,
                                const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                                const levels_req &q = levels_req())
{
    SK_ENTER(c);
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_seg(p, max_segs, nreads, !segs || !nsegs, "segs/nsegs");
    if (!rc && q.on && (!q.levels || !q.read_level)) rc = sk_fail(SK_ERR_INVALID, "NULL levels/read_level");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, sig, off, nreads, &total, &maxlen, centi))) return rc;
    const int32_t *d_rlen = nullptr;
    if (len) {                                      // the caller's sig[:Num] cut: read r is its first len[r] samples
        for (int32_t r = 0; r < nreads; r++)
            if (len[r] < 0 || (int64_t)len[r] > off[r + 1] - off[r])
                return sk_fail(SK_ERR_INVALID, "len[%d] = %d is outside [0, %lld]", r, len[r], (long long)(off[r + 1] - off[r]));
        // (a buffer of its own: segment_dev_f64 hands c->len to the statistics kernel as the place for the lengths the
        // walk reads, and the numpy-order redo looks at the cut again afterwards)
        if ((rc = sk_reserve(c, &c->rlen, (size_t)nreads * sizeof(int32_t)))) return rc;
        SK_HIP(hipMemcpyAsync(c->rlen.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        d_rlen = (const int32_t *)c->rlen.p;
        // the cut, not the slot, decides the mask row size and which statistics kernel runs (-n 3000 on 40 000-sample
        // lines takes the 4 096-sample kernel)
        maxlen = 0;
        for (int32_t r = 0; r < nreads; r++) if (len[r] > maxlen) maxlen = len[r];
    }
    if ((rc = sk_reserve(c, &c->out, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out2, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = levels_reserve(c, q, nreads, max_segs))) return rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    int row16 = 0;
    rc = segment_dev_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, total, maxlen, p,
                         (int32_t *)c->out.p, (int32_t *)c->out2.p, max_segs, d_rlen, &row16);
    if (rc) return rc;
    if (q.on) {                                      // (c->len: each read's raw length after the cut, as the walk read it)
        rc = levels_launch(c, SK_FEED_F64_NORM, c->sig.p, 0, (const int64_t *)c->off.p, row16, (const int32_t *)c->len.p,
                           maxlen, nreads, (const int32_t *)c->out.p, (const int32_t *)c->out2.p, max_segs,
                           levels_dev(c, 0, max_segs), read_level_dev(c, nreads, 0, max_segs));
        if (rc) return rc;
        if ((rc = levels_copy_back(c, q, nreads, max_segs))) return rc;
    }
    return read_segs(c, nreads, max_segs, segs, nsegs);
}

extern "C" {

int sk_segment_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                       const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (!rc) rc = check_seg(p, max_segs, nreads, !d_segs || !d_nsegs, "segs/nsegs");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    return segment_dev_i16(c, d_sig, stride, d_len, nreads, p, d_segs, d_nsegs, max_segs);
}

int sk_segment_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    return segment_host_i16(sig, stride, len, nreads, p, segs, nsegs, max_segs, levels_req());
}

int sk_segment_levels_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                          sk_seg_level *levels, sk_seg_level *read_level)
{
    return segment_host_i16(sig, stride, len, nreads, p, segs, nsegs, max_segs, levels_of(levels, read_level));
}
int sk_segment_levels_f64_len(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                              const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                              sk_seg_level *levels, sk_seg_level *read_level)
{
    return segment_batch_ragged(sig, false, off, len, nreads, p, segs, nsegs, max_segs, levels_of(levels, read_level));
}
int sk_segment_levels_centi_len(const int32_t *centi, const int64_t *off, const int32_t *len, int32_t nreads,
                                const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs,
                                sk_seg_level *levels, sk_seg_level *read_level)
{
    return segment_batch_ragged(centi, true, off, len, nreads, p, segs, nsegs, max_segs, levels_of(levels, read_level));
}
int sk_segment_levels_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs,
                              sk_seg_level *d_levels, sk_seg_level *d_read_level)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (!rc) rc = check_seg(p, max_segs, nreads, !d_segs || !d_nsegs, "segs/nsegs");
    if (!rc && (!d_levels || !d_read_level)) rc = sk_fail(SK_ERR_INVALID, "NULL levels/read_level");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    return levels_rows_i16(c, levels_of(d_levels, d_read_level), d_sig, stride, d_len, nreads, p, d_segs, d_nsegs, max_segs,
                           d_levels, d_read_level);
}

int sk_segment_batch_f64_len(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                             const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    return segment_batch_ragged(sig, false, off, len, nreads, p, segs, nsegs, max_segs);
}
int sk_segment_batch_centi_len(const int32_t *centi, const int64_t *off, const int32_t *len, int32_t nreads,
                               const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    return segment_batch_ragged(centi, true, off, len, nreads, p, segs, nsegs, max_segs);
}
int sk_segment_batch_f64(const double *sig, const int64_t *off, int32_t nreads, const sk_seg_params *p,
                         int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    return segment_batch_ragged(sig, false, off, nullptr, nreads, p, segs, nsegs, max_segs);
}

// Raw reads through the pA route: what segmenter.py does with fast5 / slow5 input unless --raw_signal is given
// (segmenter.py:345-349, 366-370: np.round(convert_to_pA_numpy(sig, digitisation, range, offset), 2) with range first
// cut to two decimals, float("{0:.2f}".format(range)), :385).  calib[3 r ..] = digitisation, offset, range of read r
// (what a fast5 / BLOW5 record carries) -> cal2[2 r ..] = {offset, raw_unit = range / digitisation}.
int sk_pa_calib(const double *calib, int32_t nreads, double *cal2)
{
    if (nreads < 0 || (nreads > 0 && (!calib || !cal2))) return sk_fail(SK_ERR_INVALID, "NULL calib / cal2");
    for (int32_t r = 0; r < nreads; r++) {
        const double dig = calib[3 * r], ofs = calib[3 * r + 1], rng = calib[3 * r + 2];
        char txt[512];
        snprintf(txt, sizeof txt, "%.2f", rng);              // float("{0:.2f}".format(range))
        cal2[2 * r] = ofs;
        cal2[2 * r + 1] = strtod(txt, nullptr) / dig;        // raw_unit = range / digitisation
    }
    return SK_OK;
}

// Reads of the most recent sk_segment_*_i16_pa call (all its sub-batches) that the raw-domain kernel could not certify
// and that were redone from their float64 values; -1 when that call expanded every read to float64 instead, or when a
// MotifSeq / segmenter call of another route came after it.
int sk_last_pa_retries(void)
{
    SK_ENTER(c);
    return redo_count(c, SK_REDO_PA);
}

int sk_segment_dev_i16_pa(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                          const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (!rc) rc = check_seg(p, max_segs, nreads, !d_cal2 || !d_segs || !d_nsegs, "cal2/segs/nsegs");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    return segment_dev_i16_pa(c, d_sig, stride, d_len, nreads, d_cal2, p, d_segs, d_nsegs, max_segs);
}

int sk_segment_batch_i16_pa(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *calib,
                            const sk_seg_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (!rc) rc = check_len_host(len, nreads, stride);
    if (!rc) rc = check_seg(p, max_segs, nreads, !calib || !segs || !nsegs, "calib/segs/nsegs");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    std::vector<double> cal((size_t)nreads * 2);
    if ((rc = sk_pa_calib(calib, nreads, cal.data()))) return rc;
    if ((rc = sk_reserve(c, &c->misc, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->pacal, cal.size() * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->out, (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out2, (size_t)nreads * sizeof(int32_t)))) return rc;
    SK_HIP(hipMemcpyAsync(c->pacal.p, cal.data(), cal.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->len.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));                 // cal goes out of scope; len / cal are there for every sub-batch
    // rows in sub-batches as sk_segment_batch_i16 (the rows in c->misc: the float64 fallback puts its image in c->sig);
    // the float64 fallback takes them in one piece and keeps its lengths in c->len as well: it gets a copy of its own
    const bool raw_domain = sk_segment_pa_applies(c->misc.p, stride, p->std_scale);
    if (!raw_domain) {
        if ((rc = sk_reserve(c, &c->rlen, (size_t)nreads * sizeof(int32_t)))) return rc;
        SK_HIP(hipMemcpyAsync(c->rlen.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const SubBatches B = raw_domain ? sub_batches(nreads, stride) : SubBatches{nreads, 1};
    if ((rc = redo_begin(c, nreads, B.n))) return rc;
    rc = ingest_rows(c, B, (int16_t *)c->misc.p, sig, stride, nullptr, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return segment_dev_i16_pa(c, d_sig, stride, raw_domain ? d_len : (const int32_t *)c->rlen.p + r0,
                                                   nr, (const double *)c->pacal.p + 2 * (size_t)r0, p,
                                                   (int32_t *)c->out.p + (size_t)r0 * 2 * (size_t)max_segs,
                                                   (int32_t *)c->out2.p + r0, max_segs);
                     });
    if (rc) return rc;
    return read_segs(c, nreads, max_segs, segs, nsegs);
}

int sk_segment_dev_f64(const double *d_sig, const int64_t *d_off, int32_t nreads, int64_t total, int64_t max_len,
                       const sk_seg_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    if (nreads < 0 || total < 0 || max_len < 0 || max_len > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "bad sizes");
    int rc = check_seg(p, max_segs, nreads, !d_sig || !d_off || !d_segs || !d_nsegs, "sig/off/segs/nsegs");
    if (rc) return rc == SK_NOTHING ? SK_OK : rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    return segment_dev_f64(c, d_sig, d_off, nreads, total, max_len, p, d_segs, d_nsegs, max_segs);
}

// ------------------------------------------------------------------ dRNA adapter segmenter
// ------------------------------------------------------------------ dRNA --signal branch (rolling mean)
// device-resident cores of the two dRNA branches (d_sig / d_len / outputs are device pointers)
// ------------------------------------------------------------------ segmenter parameter sweep
} // extern "C"

// The sets as sk_segment_batch_i16 checks its params (check_seg_params), the failure naming the set.
static int check_sweep(const sk_seg_sweep_set *sets, int32_t nsets, bool null_sums)
{
    if (nsets < 0) return sk_fail(SK_ERR_INVALID, "nsets < 0");
    if (nsets && (!sets || null_sums)) return sk_fail(SK_ERR_INVALID, "NULL sets/sums");
    for (int32_t k = 0; k < nsets; k++)
        if (sets[k].seg.corrector < 0)
            return sk_fail(SK_ERR_INVALID, "set %d: corrector must be >= 0 (the reference divides by zero otherwise)", k);
    return SK_OK;
}

// The plan's lanes to the device (c->sweep), followed by room for nsets summaries (*d_sums_scratch) when asked
static int sweep_stage(sk_ctx *c, const sk_seg_sweep_set *sets, int32_t nsets, std::vector<sk_sweep_group> &groups,
                       sk_sweep_lane **d_lanes, sk_seg_sweep_sum **d_sums_scratch)
{
    std::vector<sk_sweep_lane> lanes;
    sk_sweep_plan(sets, nsets, groups, lanes);
    const size_t lb = ((lanes.size() * sizeof(sk_sweep_lane)) + 255) & ~(size_t)255;
    int rc = sk_reserve(c, &c->sweep, lb + (size_t)nsets * sizeof(sk_seg_sweep_sum));
    if (rc) return rc;
    *d_lanes = (sk_sweep_lane *)c->sweep.p;
    SK_HIP(hipMemcpyAsync(c->sweep.p, lanes.data(), lanes.size() * sizeof(sk_sweep_lane), hipMemcpyHostToDevice, c->stream));
    if (d_sums_scratch) {
        *d_sums_scratch = (sk_seg_sweep_sum *)((char *)c->sweep.p + lb);
        SK_HIP(hipMemsetAsync(*d_sums_scratch, 0, (size_t)nsets * sizeof(sk_seg_sweep_sum), c->stream));
    }
    SK_HIP(hipStreamSynchronize(c->stream));                 // (lanes goes out of scope)
    return SK_OK;
}

// The two walks of one group over the masks in c->mask (the run-hopping sets, then the others)
static int sweep_walk_group(sk_ctx *c, const sk_sweep_group &g, const sk_sweep_lane *d_lanes, int row16, const int32_t *d_len,
                            int64_t mmax, int32_t nreads, sk_seg_sweep_sum *d_sums, sk_seg_sweep_rec *d_recs, int64_t rec_stride)
{
    int rc = sk_launch_seg_sweep_walk(c, c->mask.p, row16, d_len, mmax, nreads, d_lanes + g.first, g.nfast, true, d_sums,
                                      d_recs, rec_stride);
    if (rc) return rc;
    return sk_launch_seg_sweep_walk(c, c->mask.p, row16, d_len, mmax, nreads, d_lanes + g.first + g.nfast, g.ngen, false,
                                    d_sums, d_recs, rec_stride);
}

// Device-resident core of the int16 sweep: per group the statistics and masks of segment_dev_i16 without its walk (the
// streaming kernel and the numpy-order redo of its uncertified reads, or the numpy-order kernel for every read), then
// the group's walks.  Records of read r at d_recs[set * rec_stride + r] (d_recs: already offset to this block's reads).
static int sweep_dev_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const sk_seg_sweep_set *sets, const std::vector<sk_sweep_group> &groups, const sk_sweep_lane *d_lanes,
                         sk_seg_sweep_sum *d_sums, sk_seg_sweep_rec *d_recs, int64_t rec_stride)
{
    int rc;
    if (nreads <= 0) return SK_OK;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    for (const sk_sweep_group &g : groups) {
        const sk_seg_params &p = sets[g.rep].seg;
        int32_t lo = p.lim_low, hi = p.lim_hi;
        clamp_limits(&lo, &hi);
        int row16;
        if (sk_segment_fast_applies(d_sig, stride, lo, hi, p.std_scale)) {
            row16 = sk_segment_fast_row16(stride);
            if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)row16 * 16))) return rc;
            if ((rc = redo_begin(c, nreads, 1))) return rc;
            int32_t *redo;
            if ((rc = redo_list(c, SK_REDO_I16, nreads, &redo))) return rc;
            rc = sk_launch_segment_masks(c, d_sig, stride, d_len, nreads, p.std_scale, lo, hi, (sk_prep *)c->prep.p,
                                         c->mask.p, redo);
        } else {
            row16 = (int)((stride + 63) / 64);
            if ((rc = sk_reserve(c, &c->comp, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
            if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)row16 * 16))) return rc;
            rc = sk_launch_prep_i16(c, d_sig, stride, d_len, nreads, lo, hi, SK_PREP_SEGMENT, p.std_scale,
                                    (int16_t *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0, 0, 0x7fffffff, nullptr, nullptr,
                                    c->mask.p, row16);
        }
        if (rc) return rc;
        if ((rc = sweep_walk_group(c, g, d_lanes, row16, d_len, stride, nreads, d_sums, d_recs, rec_stride))) return rc;
    }
    return SK_OK;
}

// Reads per block of a device-resident sweep: one group's masks (and the numpy-order route's compacted rows) stay
// within 1 GiB, or SK_SWEEP_BLOCK reads when set (tests)
static int32_t sweep_block_reads(int64_t stride, int32_t nreads)
{
    const int64_t per = (int64_t)((stride + 63) / 64) * 16 + stride * (int64_t)sizeof(int16_t) + (int64_t)sizeof(sk_prep);
    int64_t b = ((int64_t)1 << 30) / per;
    if (b < 4096) b = 4096;
    return b >= nreads ? nreads : (int32_t)b;
}

extern "C" {

// segmenter.py's whole pipeline (:207-211 scale_outliers + get_segs, :473-494 test_segs) once per set of a grid:
// sk_seg_sweep_sum / sk_seg_sweep_rec in the header.  The masks are built once per (lim_low, lim_hi, std_scale) group.
int sk_segment_sweep_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *d_sums, sk_seg_sweep_rec *d_recs)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (!rc) rc = check_sweep(sets, nsets, !d_sums);
    if (rc) return rc;
    if (nsets == 0) return SK_OK;
    c->ev_valid = false;
    std::vector<sk_sweep_group> groups;
    sk_sweep_lane *d_lanes;
    if ((rc = sweep_stage(c, sets, nsets, groups, &d_lanes, nullptr))) return rc;
    SK_HIP(hipMemsetAsync(d_sums, 0, (size_t)nsets * sizeof(sk_seg_sweep_sum), c->stream));
    const int32_t blk = sweep_block_reads(stride, nreads);
    for (int32_t r0 = 0; r0 < nreads; r0 += blk) {
        const int32_t nr = nreads - r0 < blk ? nreads - r0 : blk;
        rc = sweep_dev_i16(c, d_sig + (int64_t)r0 * stride, stride, d_len + r0, nr, sets, groups, d_lanes, d_sums,
                           d_recs ? d_recs + r0 : nullptr, nreads);
        if (rc) return rc;
    }
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_segment_sweep_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *sums, sk_seg_sweep_rec *recs)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (!rc) rc = check_len_host(len, nreads, stride);
    if (!rc) rc = check_sweep(sets, nsets, !sums);
    if (rc) return rc;
    if (nsets == 0) return SK_OK;
    c->ev_valid = false;
    std::vector<sk_sweep_group> groups;
    sk_sweep_lane *d_lanes;
    sk_seg_sweep_sum *d_sums;
    if ((rc = sweep_stage(c, sets, nsets, groups, &d_lanes, &d_sums))) return rc;
    sk_seg_sweep_rec *d_recs = nullptr;
    const size_t rb = (size_t)nsets * (size_t)nreads * sizeof(sk_seg_sweep_rec);
    if (recs && nreads) {
        if ((rc = sk_reserve(c, &c->sweeprec, rb))) return rc;
        d_recs = (sk_seg_sweep_rec *)c->sweeprec.p;
    }
    if (nreads) {
        // sub-batches of the host rows as sk_segment_batch_i16's, each small enough for sweep_block_reads' budget
        SubBatches B = sub_batches(nreads, stride);
        const int32_t blk = sweep_block_reads(stride, nreads);
        if (B.per > blk) {
            B.n = (nreads + blk - 1) / blk;
            B.per = (int32_t)(((int64_t)nreads + B.n - 1) / B.n);
        }
        if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
        if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
        rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                         [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                             return sweep_dev_i16(c, d_sig, stride, d_len, nr, sets, groups, d_lanes, d_sums,
                                                  d_recs ? d_recs + r0 : nullptr, nreads);
                         });
        if (rc) return rc;
    }
    SK_HIP(hipMemcpyAsync(sums, d_sums, (size_t)nsets * sizeof(sk_seg_sweep_sum), hipMemcpyDeviceToHost, c->stream));
    if (d_recs) SK_HIP(hipMemcpyAsync(recs, d_recs, rb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// The float64 route (pA TSVs, converted fast5 / BLOW5 reads): as sk_segment_batch_f64_len, every group through the
// statistics of segment_dev_f64 without its walk.
int sk_segment_sweep_f64(const double *sig, const int64_t *off, const int32_t *len, int32_t nreads,
                         const sk_seg_sweep_set *sets, int32_t nsets, sk_seg_sweep_sum *sums, sk_seg_sweep_rec *recs)
{
    SK_ENTER(c);
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_sweep(sets, nsets, !sums);
    if (rc) return rc;
    if (nsets == 0) return SK_OK;
    c->ev_valid = false;
    std::vector<sk_sweep_group> groups;
    sk_sweep_lane *d_lanes;
    sk_seg_sweep_sum *d_sums;
    if ((rc = sweep_stage(c, sets, nsets, groups, &d_lanes, &d_sums))) return rc;
    sk_seg_sweep_rec *d_recs = nullptr;
    const size_t rb = (size_t)nsets * (size_t)nreads * sizeof(sk_seg_sweep_rec);
    if (nreads) {
        int64_t total, maxlen;
        if ((rc = stage_ragged_f64(c, sig, off, nreads, &total, &maxlen))) return rc;
        const int32_t *d_rlen = nullptr;
        if (len) {                                  // read r is its first len[r] samples (segment_batch_ragged)
            for (int32_t r = 0; r < nreads; r++)
                if (len[r] < 0 || (int64_t)len[r] > off[r + 1] - off[r])
                    return sk_fail(SK_ERR_INVALID, "len[%d] = %d is outside [0, %lld]", r, len[r], (long long)(off[r + 1] - off[r]));
            if ((rc = sk_reserve(c, &c->rlen, (size_t)nreads * sizeof(int32_t)))) return rc;
            SK_HIP(hipMemcpyAsync(c->rlen.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            d_rlen = (const int32_t *)c->rlen.p;
            maxlen = 0;
            for (int32_t r = 0; r < nreads; r++) if (len[r] > maxlen) maxlen = len[r];
        }
        if (recs) {
            if ((rc = sk_reserve(c, &c->sweeprec, rb))) return rc;
            d_recs = (sk_seg_sweep_rec *)c->sweeprec.p;
        }
        for (const sk_sweep_group &g : groups) {
            const sk_seg_params &p = sets[g.rep].seg;
            if ((rc = redo_begin(c, nreads, 1))) return rc;
            int row16;
            rc = segment_masks_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, total, maxlen, p.lim_low,
                                   p.lim_hi, p.std_scale, d_rlen, &row16);
            if (rc) return rc;
            rc = sweep_walk_group(c, g, d_lanes, row16, (const int32_t *)c->len.p, (int64_t)row16 * 64, nreads, d_sums, d_recs,
                                  nreads);
            if (rc) return rc;
        }
    }
    SK_HIP(hipMemcpyAsync(sums, d_sums, (size_t)nsets * sizeof(sk_seg_sweep_sum), hipMemcpyDeviceToHost, c->stream));
    if (d_recs) SK_HIP(hipMemcpyAsync(recs, d_recs, rb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

static int drna_roll_dev(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const sk_roll_params *p, int32_t *d_xy, int32_t *d_found)
{
    int rc;
    int32_t lo = p->lim_low, hi = p->lim_hi;
    clamp_limits(&lo, &hi);
    const int64_t words = (stride + 63) / 64;
    const size_t sb = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)words * 2 * sizeof(uint64_t)))) return rc;
    uint64_t *below = (uint64_t *)c->mask.p, *above = below + (size_t)nreads * (size_t)words;
    // one look (round 5): a workgroup per read, prefix sums in LDS -- rows of up to ~35 000 samples, w < 65 536
    // ... or as a stream, a wavefront per read with certified thresholds (windows of up to 12 000 samples, rows of any length)
    const bool stream = sk_roll_stream_ok(stride, p->w, lo, hi) && sk_tune("SK_ROLL_ONE_LOOK") == nullptr;
    if ((stream || sk_roll_one_lds(stride, p->w)) && sk_tune("SK_ROLL_TWO_KERNELS") == nullptr && sk_tune("SK_DRNA_STEP") == nullptr) {
        if (stream && (rc = sk_reserve(c, &c->misc, ((size_t)nreads + 2) * sizeof(int32_t)))) return rc;
        SK_HIP(hipEventRecord(c->ev[0], c->stream));
        if (stream)
            rc = sk_launch_roll_stream(c, d_sig, stride, d_len, nreads, lo, hi, p->w, p->std_scale, (sk_prep *)c->prep.p,
                                       below, above, (int32_t *)c->misc.p);
        else
            rc = sk_launch_roll_one(c, d_sig, stride, d_len, nreads, lo, hi, p->w, p->std_scale, (sk_prep *)c->prep.p,
                                    below, above);
        if (rc) return rc;
        SK_HIP(hipEventRecord(c->ev[1], c->stream));
        if ((rc = sk_launch_roll_walk(c, below, stream ? below + 1 : above, (const sk_prep *)c->prep.p, nreads, p, d_xy,
                                      d_found, stream ? words : 0))) return rc;
        c->ev_valid = true;
        return SK_OK;
    }
    if ((rc = sk_reserve(c, &c->comp, sb))) return rc;
    // prefix sums of the filtered samples: 4 bytes each when every window sum fits 31 bits (sk_launch_roll_stats)
    const size_t pbytes = (p->w < 65536 && sk_tune("SK_DRNA_STEP") == nullptr) ? sizeof(uint32_t) : sizeof(int64_t);
    if ((rc = sk_reserve(c, &c->misc, (size_t)nreads * (size_t)(stride + 1) * pbytes))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    // filter + order-preserving compaction (the medmad kernel: its statistics are not used here)
    rc = sk_launch_prep_i16(c, d_sig, stride, d_len, nreads, lo, hi,
                            SK_PREP_MEDMAD, 0.0, (int16_t *)c->comp.p, (sk_prep *)c->prep.p, nullptr, 0);
    if (rc) return rc;
    rc = sk_launch_roll_stats(c, (const int16_t *)c->comp.p, stride, (sk_prep *)c->prep.p, nreads, p->w,
                              p->std_scale, (int64_t *)c->misc.p, below, above);
    if (rc) return rc;
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    rc = sk_launch_roll_walk(c, below, above, (const sk_prep *)c->prep.p, nreads, p, d_xy, d_found);
    if (rc) return rc;
    c->ev_valid = true;
    return SK_OK;
}

static int drna_segment_dev(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                            const sk_drna_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    int rc;
    int32_t lo = p->lim_low, hi = p->lim_hi;
    clamp_limits(&lo, &hi);
    const int64_t words = (stride + 63) / 64;
    const size_t sb = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    const size_t gb = (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t);
    if ((rc = sk_reserve(c, &c->comp, sb))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->mask, (size_t)nreads * (size_t)words * sizeof(uint64_t)))) return rc;
    SK_HIP(hipMemsetAsync(d_segs, 0, gb, c->stream));
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    rc = sk_launch_prep_i16(c, d_sig, stride, d_len, nreads, lo, hi,
                            SK_PREP_DRNA, p->std_scale, (int16_t *)c->comp.p, (sk_prep *)c->prep.p,
                            (uint64_t *)c->mask.p, nreads, p->t_start, p->t_end);
    if (rc) return rc;
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    rc = sk_launch_drna_walk(c, (const uint64_t *)c->mask.p, nreads, (const sk_prep *)c->prep.p, nreads, p,
                             d_segs, d_nsegs, max_segs);
    if (rc) return rc;
    c->ev_valid = true;
    return SK_OK;
}

static int check_roll(const sk_roll_params *p)
{
    if (!p) return sk_fail(SK_ERR_INVALID, "NULL sk_roll_params");
    if (p->w <= 0) return sk_fail(SK_ERR_INVALID, "the rolling window w must be positive");
    return SK_OK;
}

static int check_drna(const sk_drna_params *p, int32_t max_segs)
{
    if (!p) return sk_fail(SK_ERR_INVALID, "NULL sk_drna_params");
    if (p->w <= 0) return sk_fail(SK_ERR_INVALID, "w must be positive (the scan takes c %% w)");
    if (p->t_start < 0 || p->t_end < p->t_start) return sk_fail(SK_ERR_INVALID, "bad statistics window");
    if (max_segs <= 0) return sk_fail(SK_ERR_INVALID, "max_segs must be positive");
    return SK_OK;
}

int sk_drna_roll_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const sk_roll_params *p, int32_t *d_xy, int32_t *d_found)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_roll(p))) return rc;
    if (nreads == 0) return SK_OK;
    if (!d_xy || !d_found) return sk_fail(SK_ERR_INVALID, "NULL xy/found");
    return drna_roll_dev(c, d_sig, stride, d_len, nreads, p, d_xy, d_found);
}

int sk_drna_segment_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                            const sk_drna_params *p, int32_t *d_segs, int32_t *d_nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_drna(p, max_segs))) return rc;
    if (nreads == 0) return SK_OK;
    if (!d_segs || !d_nsegs) return sk_fail(SK_ERR_INVALID, "NULL segs/nsegs");
    return drna_segment_dev(c, d_sig, stride, d_len, nreads, p, d_segs, d_nsegs, max_segs);
}

int sk_drna_roll_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                           const sk_roll_params *p, int32_t *xy, int32_t *found)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    if ((rc = check_roll(p))) return rc;
    if (nreads == 0) return SK_OK;
    if (!xy || !found) return sk_fail(SK_ERR_INVALID, "NULL xy/found");
    const size_t sb = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    if ((rc = sk_reserve(c, &c->sig, sb))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, (size_t)nreads * 2 * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out2, (size_t)nreads * sizeof(int32_t)))) return rc;
    SK_HIP(hipMemcpyAsync(c->sig.p, sig, sb, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->len.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = drna_roll_dev(c, (const int16_t *)c->sig.p, stride, (const int32_t *)c->len.p, nreads, p,
                            (int32_t *)c->out.p, (int32_t *)c->out2.p))) return rc;
    SK_HIP(hipMemcpyAsync(xy, c->out.p, (size_t)nreads * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(found, c->out2.p, (size_t)nreads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_drna_segment_batch_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                              const sk_drna_params *p, int32_t *segs, int32_t *nsegs, int32_t max_segs)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    if ((rc = check_drna(p, max_segs))) return rc;
    if (nreads == 0) return SK_OK;
    if (!segs || !nsegs) return sk_fail(SK_ERR_INVALID, "NULL segs/nsegs");
    const size_t sb = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    const size_t gb = (size_t)nreads * 2 * (size_t)max_segs * sizeof(int32_t);
    if ((rc = sk_reserve(c, &c->sig, sb))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, gb))) return rc;
    if ((rc = sk_reserve(c, &c->out2, (size_t)nreads * sizeof(int32_t)))) return rc;
    SK_HIP(hipMemcpyAsync(c->sig.p, sig, sb, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->len.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = drna_segment_dev(c, (const int16_t *)c->sig.p, stride, (const int32_t *)c->len.p, nreads, p,
                               (int32_t *)c->out.p, (int32_t *)c->out2.p, max_segs))) return rc;
    return read_segs(c, nreads, max_segs, segs, nsegs);
}

// ------------------------------------------------------------------ bench input
int sk_synth_squiggles_dev(int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples,
                           uint64_t seed, const double *motif, int32_t nmotif)
{
    SK_ENTER(c);
    if (!d_sig || stride < nsamples || nreads < 0 || nsamples < 0)
        return sk_fail(SK_ERR_INVALID, "bad arguments");
    const int16_t *d_m = nullptr;
    if (motif && nmotif > 0) {
        std::vector<int16_t> mi((size_t)nmotif);
        for (int i = 0; i < nmotif; i++) {
            double v = rint(motif[i] * 93.4 + 511.0);
            mi[i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
        }
        int rc = sk_reserve(c, &c->misc, mi.size() * 2);
        if (rc) return rc;
        SK_HIP(hipMemcpyAsync(c->misc.p, mi.data(), mi.size() * 2, hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipStreamSynchronize(c->stream));
        d_m = (const int16_t *)c->misc.p;
    }
    int rc = sk_launch_synth(c, d_sig, stride, nreads, nsamples, seed, d_m, nmotif);
    if (rc) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_synth_variant_dev(int16_t *d_sig, int64_t stride, int32_t nreads, int32_t nsamples, uint64_t seed,
                         const double *motif, int32_t nmotif, const sk_synth_opts *o)
{
    SK_ENTER(c);
    if (!d_sig || !o || stride < nsamples || nreads < 0 || nsamples < 0 || o->row0 < 0)
        return sk_fail(SK_ERR_INVALID, "bad arguments");
    int rc;
    if (o->tmpl && o->ntmpl > 0) {                       // windows of a measured squiggle + noise
        if ((rc = sk_reserve(c, &c->misc, (size_t)o->ntmpl * 2))) return rc;
        SK_HIP(hipMemcpyAsync(c->misc.p, o->tmpl, (size_t)o->ntmpl * 2, hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipStreamSynchronize(c->stream));
        rc = sk_launch_synth_windows(c, d_sig, stride, nreads, nsamples, seed, o->row0, (const int16_t *)c->misc.p,
                                     o->ntmpl, (float)o->tmpl_noise);
    } else {
        const int16_t *d_m = nullptr;
        if (motif && nmotif > 0) {
            std::vector<int16_t> mi((size_t)nmotif);
            for (int i = 0; i < nmotif; i++) {
                double v = rint(motif[i] * 93.4 + 511.0);
                mi[i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
            }
            if ((rc = sk_reserve(c, &c->misc, mi.size() * 2))) return rc;
            SK_HIP(hipMemcpyAsync(c->misc.p, mi.data(), mi.size() * 2, hipMemcpyHostToDevice, c->stream));
            SK_HIP(hipStreamSynchronize(c->stream));
            d_m = (const int16_t *)c->misc.p;
        }
        rc = sk_launch_synth(c, d_sig, stride, nreads, nsamples, seed, d_m, nmotif, o->row0, o->hit_permille,
                             o->stretch_permille, o->stretch);
    }
    if (rc) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// The float64 pA image of an int16 batch, as SquigglePull.py:183-189,238-240 writes it (bench / test input for the
// float64 entry points): d_out[nreads * nsamples] doubles, d_off[nreads + 1] zero-based offsets.
int sk_synth_pa_dev(const int16_t *d_raw, int64_t stride, int32_t nreads, int32_t nsamples,
                    double offset, double range, double digitisation, double *d_out, int64_t *d_off)
{
    SK_ENTER(c);
    if (!d_raw || !d_out || !d_off || stride < nsamples || nreads < 0 || nsamples < 0 || !(digitisation > 0))
        return sk_fail(SK_ERR_INVALID, "bad arguments");
    int rc = sk_launch_raw_to_pa(c, d_raw, stride, nreads, nsamples, offset, range / digitisation, d_out, d_off);
    if (rc) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// Reads of the most recent float64 call (segmenter or MotifSeq medmad) that the streaming statistics kernel handed
// to the numpy-order kernel (diagnostic); -1 when that call did not take the streaming kernel, or when a MotifSeq /
// segmenter call of another route came after it.
int sk_last_f64_retries(void)
{
    SK_ENTER(c);
    return redo_count(c, SK_REDO_F64);
}

// mlpy.dtw_subsequence(x, y) in the reference's own C arithmetic, NaN / inf included (k_dtw_cref above): what
// `MotifSeq.py --strict-compat` prints for reads whose MAD is 0.  Full cost matrix in device memory, one lane.
int sk_dtw_subsequence_cref(const double *x, int32_t nx, const double *y, int32_t ny,
                            double *dist, int32_t *start, int32_t *end)
{
    SK_ENTER(c);
    if (!x || !y || nx <= 0 || ny <= 0) return sk_fail(SK_ERR_INVALID, "empty x or y");
    const size_t cells = (size_t)nx * (size_t)ny;
    if (cells > ((size_t)1 << 28)) return sk_fail(SK_ERR_UNSUPPORTED, "%d x %d cost matrix is over 2 GB", nx, ny);
    int rc;
    if ((rc = sk_reserve(c, &c->sig, ((size_t)nx + (size_t)ny) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->misc, cells * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->out, sizeof(sk_hit)))) return rc;
    double *d_x = (double *)c->sig.p, *d_y = d_x + nx;
    SK_HIP(hipMemcpyAsync(d_x, x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_y, y, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dtw_cref, dim3(1), dim3(64), 0, c->stream, (const double *)d_x, nx, (const double *)d_y, ny,
                       (double *)c->misc.p, (sk_hit *)c->out.p);
    SK_HIP(hipGetLastError());
    sk_hit h;
    SK_HIP(hipMemcpyAsync(&h, c->out.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (dist) *dist = h.dist;
    if (start) *start = h.start;
    if (end) *end = h.end;
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ SquigglePull text (sk_pull.hip)
namespace {

struct PullScratch {
    int32_t *err;
    int64_t *tile0, *tb, *lines, *bsum;
    int64_t  tile_cap;
};

int check_pull(int32_t mode, int64_t capacity, const void *text, const int64_t *total)
{
    if (mode != SK_PULL_RAW && mode != SK_PULL_PA) return sk_fail(SK_ERR_INVALID, "mode must be SK_PULL_RAW or SK_PULL_PA");
    if (!total) return sk_fail(SK_ERR_INVALID, "NULL total");
    if (capacity < 0) return sk_fail(SK_ERR_INVALID, "capacity < 0");
    if (capacity > 0 && !text) return sk_fail(SK_ERR_INVALID, "NULL text with a capacity");
    return SK_OK;
}

// pass 1 and the scans; *total = the text's size (synchronises), SK_ERR_UNSUPPORTED for a value the formatter cannot
// print, SK_ERR_OVERFLOW past `capacity`
int pull_count(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal,
               const int64_t *d_poff, int64_t capacity, int64_t *total, PullScratch *s)
{
    int rc;
    s->tile_cap = sk_pull_tile_cap(nreads, stride);
    const int64_t nb = sk_scan_blocks(s->tile_cap > nreads ? s->tile_cap : nreads);
    const size_t items = (size_t)(nreads + 1) * 2 + (size_t)(s->tile_cap + 1) + (size_t)nb;
    if ((rc = sk_reserve(c, &c->pull, 16 + items * sizeof(int64_t)))) return rc;
    s->err = (int32_t *)c->pull.p;
    s->tile0 = (int64_t *)((char *)c->pull.p + 16);
    s->tb = s->tile0 + nreads + 1;
    s->lines = s->tb + s->tile_cap + 1;
    s->bsum = s->lines + nreads + 1;
    SK_HIP(hipMemsetAsync(s->err, 0, 16, c->stream));
    if ((rc = sk_launch_pull_count(c, d_sig, stride, d_len, nreads, d_cal, d_poff, s->tile0, s->tb, s->tile_cap, s->bsum,
                                   s->lines, s->err)))
        return rc;
    int64_t t = 0;
    int32_t bad = 0;
    SK_HIP(hipMemcpyAsync(&t, s->lines + nreads, sizeof t, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(&bad, s->err, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    *total = t;
    if (bad) return sk_fail(SK_ERR_UNSUPPORTED, "a pA value is not finite or has |value| >= 1e13 (calibration out of range)");
    if (t > capacity)
        return sk_fail(SK_ERR_OVERFLOW, "the text needs %lld bytes, capacity is %lld", (long long)t, (long long)capacity);
    return SK_OK;
}

} // namespace

int sk_pull_text_dev(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                     int32_t mode, const char *d_prefix, const int64_t *d_prefix_off, char *d_text, int64_t capacity,
                     int64_t *total, int64_t *d_line_off)
{
    SK_ENTER(c);
    int rc = check_pull(mode, capacity, d_text, total);
    if (!rc) rc = check_i16(d_sig, stride, d_len, nreads);
    if (!rc && nreads && (!d_prefix || !d_prefix_off || !d_line_off)) rc = sk_fail(SK_ERR_INVALID, "NULL prefix / prefix_off / line_off");
    if (!rc && nreads && mode == SK_PULL_PA && !d_cal2) rc = sk_fail(SK_ERR_INVALID, "NULL cal2 in pA mode");
    if (rc) return rc;
    *total = 0;
    if (nreads == 0) {
        if (d_line_off) SK_HIP(hipMemsetAsync(d_line_off, 0, sizeof(int64_t), c->stream));
        return SK_OK;
    }
    const double *cal = mode == SK_PULL_PA ? d_cal2 : nullptr;
    PullScratch s;
    if ((rc = pull_count(c, d_sig, stride, d_len, nreads, cal, d_prefix_off, capacity, total, &s))) return rc;
    if ((rc = sk_launch_pull_write(c, d_sig, stride, d_len, nreads, cal, d_prefix, d_prefix_off, s.tile0, s.tb, s.tile_cap,
                                   s.lines, d_text)))
        return rc;
    SK_HIP(hipMemcpyAsync(d_line_off, s.lines, (size_t)(nreads + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
    return SK_OK;
}

int sk_pull_text(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *calib, int32_t mode,
                 const char *prefix, const int64_t *prefix_off, char *text, int64_t capacity, int64_t *total,
                 int64_t *line_off)
{
    SK_ENTER(c);
    int rc = check_pull(mode, capacity, text, total);
    if (!rc) rc = check_i16(sig, stride, len, nreads);
    if (!rc) rc = check_len_host(len, nreads, stride);
    if (!rc && nreads && !prefix_off) rc = sk_fail(SK_ERR_INVALID, "NULL prefix_off");
    if (!rc && nreads && mode == SK_PULL_PA && !calib) rc = sk_fail(SK_ERR_INVALID, "NULL calib in pA mode");
    if (rc) return rc;
    *total = 0;
    if (nreads == 0) {
        if (line_off) line_off[0] = 0;
        return SK_OK;
    }
    if (prefix_off[0] < 0) return sk_fail(SK_ERR_INVALID, "prefix_off[0] < 0");
    for (int32_t r = 0; r < nreads; r++)
        if (prefix_off[r + 1] < prefix_off[r]) return sk_fail(SK_ERR_INVALID, "prefix_off decreases at read %d", r);
    const int64_t pbytes = prefix_off[nreads];
    if (pbytes > 0 && !prefix) return sk_fail(SK_ERR_INVALID, "NULL prefix");
    std::vector<double> cal;
    if (mode == SK_PULL_PA) {
        cal.resize((size_t)nreads * 2);
        if ((rc = sk_pa_calib(calib, nreads, cal.data()))) return rc;
    }
    const size_t row_bytes = (size_t)nreads * (size_t)stride * sizeof(int16_t);
    const size_t poff_bytes = (size_t)(nreads + 1) * sizeof(int64_t);
    if ((rc = sk_reserve(c, &c->sig, row_bytes))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->out, poff_bytes + (size_t)pbytes))) return rc;
    if (!cal.empty() && (rc = sk_reserve(c, &c->pacal, cal.size() * sizeof(double)))) return rc;
    int64_t *d_poff = (int64_t *)c->out.p;
    char *d_prefix = (char *)c->out.p + poff_bytes;
    SK_HIP(hipMemcpyAsync(c->sig.p, sig, row_bytes, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(c->len.p, len, (size_t)nreads * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_poff, prefix_off, poff_bytes, hipMemcpyHostToDevice, c->stream));
    if (pbytes > 0) SK_HIP(hipMemcpyAsync(d_prefix, prefix, (size_t)pbytes, hipMemcpyHostToDevice, c->stream));
    if (!cal.empty())
        SK_HIP(hipMemcpyAsync(c->pacal.p, cal.data(), cal.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *d_cal = cal.empty() ? nullptr : (const double *)c->pacal.p;
    const int16_t *d_sig = (const int16_t *)c->sig.p;
    const int32_t *d_len = (const int32_t *)c->len.p;
    PullScratch s;
    if ((rc = pull_count(c, d_sig, stride, d_len, nreads, d_cal, d_poff, capacity, total, &s))) return rc;   // (synchronises:
    if ((rc = sk_reserve(c, &c->pulltext, (size_t)*total))) return rc;                                           //  cal is safe)
    if ((rc = sk_launch_pull_write(c, d_sig, stride, d_len, nreads, d_cal, d_prefix, d_poff, s.tile0, s.tb, s.tile_cap, s.lines,
                                   (char *)c->pulltext.p)))
        return rc;
    SK_HIP(hipMemcpyAsync(text, c->pulltext.p, (size_t)*total, hipMemcpyDeviceToHost, c->stream));
    if (line_off) SK_HIP(hipMemcpyAsync(line_off, s.lines, (size_t)(nreads + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

// ------------------------------------------------------------------ MotifSeq panel inside a search region (sk_panel.hip)
// Per read: the slice raw[begin:end] (or the read's own win row) is cut BEFORE scale_outliers (MotifSeq.py:274,317-324),
// filter + medmad / zscale (:186-200) run once over the slice, every motif's dtw_subsequence (:436-439) runs over the
// window in one grid per shape group, and the Z-scores of :441-443 are formed and ranked on the device.
namespace {

int check_panel(const double *motifs, const int32_t *motif_off, int32_t nmotifs, const double *mean, const double *sd,
                int32_t scale_mode)
{
    if (nmotifs < 1 || nmotifs > 256) return sk_fail(SK_ERR_INVALID, "nmotifs %d outside 1..256", nmotifs);
    int rc = check_multi(motifs, motif_off, nmotifs, scale_mode);
    if (rc) return rc;
    if (!mean || !sd) return sk_fail(SK_ERR_INVALID, "NULL mean/sd");
    for (int32_t k = 0; k < nmotifs; k++) {
        if (!isfinite(mean[k]) || !isfinite(sd[k])) return sk_fail(SK_ERR_INVALID, "mean / sd of motif %d is not finite", k);
        if (sd[k] == 0.0) return sk_fail(SK_ERR_INVALID, "sd of motif %d is 0", k);
    }
    return SK_OK;
}

// Read r's window on the host: resolved begin and length.  A win row whose resolved begin lies behind its end is an
// error unless both ends were cut to the read (what a slice does with a row that lies outside the read altogether).
int panel_window(int32_t r, int32_t len, int32_t begin, int32_t end, const int32_t *win, int32_t *lo, int32_t *m)
{
    int32_t hi;
    int cl;
    sk_slice_indices(len, win ? win[2 * r] : begin, win ? win[2 * r + 1] : end, lo, &hi, &cl);
    if (win && *lo > hi && cl != 3)
        return sk_fail(SK_ERR_INVALID, "win[%d] = (%d, %d): begin lies behind end in a read of %d samples", r, win[2 * r],
                       win[2 * r + 1], len);
    *m = hi > *lo ? hi - *lo : 0;
    return SK_OK;
}

int64_t round8(int64_t v) { return v < 8 ? 8 : (v + 7) / 8 * 8; }

// What one int16 call asks of each of its (sub-)batches, and where the call keeps its per-read buffers on the device:
// read r of the call has slot r of each (d_win: nullptr = the begin / end pair; d_all / d_out: [nmotifs][nreads] and
// [nreads]).  comp / prep are c->comp / c->prep, laid out for the whole call like the rest.
struct panel_req {
    int32_t        begin, end;
    const int32_t *d_win;
    const double  *motifs;
    const int32_t *motif_off;
    int32_t        nmotifs, scale_mode, scale_low, scale_hi;
    int32_t        nreads;          // of the whole call
    int64_t        wstride;
    int16_t       *d_rows;          // window rows, stride wstride
    int32_t       *d_wlen, *d_from;
    sk_hit        *d_all;
    sk_panel_rec  *d_out;
};

// Reads [r0, r0 + nr) of the call, everything device resident: gather, filter + statistics over the windows (never
// fused: the panel's DTW has no screening pass), DTW of every motif, ranking.
int panel_dev_i16(sk_ctx *c, const panel_req &q, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nr,
                  int32_t r0)
{
    int rc;
    int16_t *d_rows = q.d_rows + (size_t)r0 * (size_t)q.wstride;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = sk_launch_region_rows_i16(c, d_sig, stride, d_len, nr, q.begin, q.end, q.d_win ? q.d_win + 2 * (size_t)r0 : nullptr,
                                        d_rows, q.wstride, q.d_wlen + r0, q.d_from + r0))) return rc;
    sk_sdtw_args a;
    if ((rc = prep_i16(c, d_rows, q.wstride, q.d_wlen + r0, nr, q.scale_mode, q.scale_low, q.scale_hi,
                       (int16_t *)c->comp.p + (size_t)r0 * (size_t)q.wstride, (sk_prep *)c->prep.p + r0, nullptr, true, &a)))
        return rc;
    a.motif = nullptr; a.nmotif = 0; a.out = nullptr; a.force_single = 1; a.accumulate = r0 > 0;
    if ((rc = sk_launch_panel_dtw(c, &a, q.motifs, q.motif_off, q.d_all + r0, q.nreads))) return rc;
    if ((rc = sk_launch_panel_rank(c, q.d_all + r0, q.nreads, nr, q.nmotifs, q.d_out + r0))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

} // namespace

extern "C" {

int sk_motifseq_panel_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                              int32_t begin, int32_t end, const int32_t *d_win,
                              const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                              const double *mean, const double *sd,
                              int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                              sk_panel_rec *d_out, int32_t *d_from, sk_hit *d_all)
{
    SK_ENTER(c);
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_panel(motifs, motif_off, nmotifs, mean, sd, scale_mode))) return rc;
    if (nreads == 0) return SK_OK;
    if (!d_out) return sk_fail(SK_ERR_INVALID, "NULL out");
    clamp_limits(&scale_low, &scale_hi);
    redo_forget(c);
    // the longest slice any read can resolve to, from the per-call pair alone (the lengths live on the device)
    int64_t bound = stride;
    if (!d_win) {
        const int64_t b = begin, e = end;
        if (b >= 0 && e >= 0 && end != INT32_MAX) bound = e > b ? e - b : 0;
        else if (b < 0 && end == INT32_MAX) bound = -b;
        else if (b < 0 && e < 0) bound = e > b ? e - b : 0;
        if (bound > stride) bound = stride;
    }
    const int64_t wstride = round8(bound);
    if ((rc = sk_reserve(c, &c->panelwin, (size_t)nreads * (size_t)wstride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->panelaux, (size_t)nreads * 2 * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, (size_t)nreads * (size_t)wstride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if (!d_all) {
        if ((rc = sk_reserve(c, &c->panelrec, (size_t)nreads * (size_t)nmotifs * sizeof(sk_hit)))) return rc;
        d_all = (sk_hit *)c->panelrec.p;
    }
    if ((rc = sk_panel_plan(c, motifs, motif_off, nmotifs, mean, sd, (int64_t)nreads * nmotifs))) return rc;
    int32_t *d_wlen = (int32_t *)c->panelaux.p;
    const panel_req q = {begin, end, d_win, motifs, motif_off, nmotifs, scale_mode, scale_low, scale_hi, nreads, wstride,
                         (int16_t *)c->panelwin.p, d_wlen, d_from ? d_from : d_wlen + nreads, d_all, d_out};
    return panel_dev_i16(c, q, d_sig, stride, d_len, nreads, 0);
}

int sk_motifseq_panel_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                          int32_t begin, int32_t end, const int32_t *win,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                          const double *mean, const double *sd,
                          int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                          sk_panel_rec *out, int32_t *from, sk_hit *all)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    if ((rc = check_panel(motifs, motif_off, nmotifs, mean, sd, scale_mode))) return rc;
    if (nreads == 0) return SK_OK;
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    clamp_limits(&scale_low, &scale_hi);
    int64_t longest = 0;
    for (int32_t r = 0; r < nreads; r++) {
        int32_t lo, m;
        if ((rc = panel_window(r, len[r], begin, end, win, &lo, &m))) return rc;
        if (m > longest) longest = m;
    }
    const int64_t wstride = round8(longest);
    const size_t wb = (size_t)nreads * (size_t)wstride * sizeof(int16_t);
    const size_t ab = (size_t)nreads * (size_t)nmotifs * sizeof(sk_hit);
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->panelwin, wb))) return rc;
    if ((rc = sk_reserve(c, &c->panelaux, (size_t)nreads * 4 * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->comp, wb))) return rc;
    if ((rc = sk_reserve(c, &c->prep, (size_t)nreads * sizeof(sk_prep)))) return rc;
    if ((rc = sk_reserve(c, &c->panelrec, ab + (size_t)nreads * sizeof(sk_panel_rec)))) return rc;
    redo_forget(c);
    const SubBatches B = sub_batches(nreads, stride);
    if ((rc = sk_panel_plan(c, motifs, motif_off, nmotifs, mean, sd, (int64_t)B.per * nmotifs))) return rc;
    int32_t *d_wlen = (int32_t *)c->panelaux.p, *d_from = d_wlen + nreads, *d_win = nullptr;
    if (win) {
        d_win = d_from + nreads;
        SK_HIP(hipMemcpyAsync(d_win, win, (size_t)nreads * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    sk_hit *d_all = (sk_hit *)c->panelrec.p;
    sk_panel_rec *d_out = (sk_panel_rec *)(d_all + (size_t)nreads * (size_t)nmotifs);
    const panel_req q = {begin, end, d_win, motifs, motif_off, nmotifs, scale_mode, scale_low, scale_hi, nreads, wstride,
                         (int16_t *)c->panelwin.p, d_wlen, d_from, d_all, d_out};
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return panel_dev_i16(c, q, d_sig, stride, d_len, nr, r0);
                     });
    if (rc) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, (size_t)nreads * sizeof(sk_panel_rec), hipMemcpyDeviceToHost, c->stream));
    if (from) SK_HIP(hipMemcpyAsync(from, d_from, (size_t)nreads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (all) SK_HIP(hipMemcpyAsync(all, d_all, ab, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_motifseq_panel_f64(const double *sig, const int64_t *off, int32_t nreads,
                          int32_t begin, int32_t end, const int32_t *win,
                          const double *motifs, const int32_t *motif_off, int32_t nmotifs,
                          const double *mean, const double *sd,
                          int32_t scale_mode, int32_t scale_low, int32_t scale_hi,
                          sk_panel_rec *out, int32_t *from, sk_hit *all)
{
    SK_ENTER(c);
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_panel(motifs, motif_off, nmotifs, mean, sd, scale_mode);
    if (rc) return rc;
    if (nreads == 0) return SK_OK;
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, sig, off, nreads, &total, &maxlen))) return rc;     // (checks sig / off and the lengths)
    // the windows, resolved on the host: source offset of each and the ragged offsets of the gathered batch
    std::vector<int64_t> aux(2 * (size_t)nreads + 1);
    int64_t *src = aux.data(), *woff = src + nreads;
    std::vector<int32_t> lo_host((size_t)nreads);
    int64_t wtotal = 0, wmax = 0;
    for (int32_t r = 0; r < nreads; r++) {
        int32_t lo, m;
        if ((rc = panel_window(r, (int32_t)(off[r + 1] - off[r]), begin, end, win, &lo, &m))) return rc;
        src[r] = off[r] - off[0] + lo;
        woff[r] = wtotal;
        wtotal += m;
        if (m > wmax) wmax = m;
        lo_host[r] = lo;
    }
    woff[nreads] = wtotal;
    const size_t ab = (size_t)nreads * (size_t)nmotifs * sizeof(sk_hit);
    if ((rc = sk_reserve(c, &c->panelwin, (size_t)(wtotal > 0 ? wtotal : 1) * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->panelaux, aux.size() * sizeof(int64_t)))) return rc;
    if ((rc = sk_reserve(c, &c->panelrec, ab + (size_t)nreads * sizeof(sk_panel_rec)))) return rc;
    if ((rc = redo_begin(c, nreads, 1))) return rc;
    if ((rc = sk_panel_plan(c, motifs, motif_off, nmotifs, mean, sd, (int64_t)nreads * nmotifs))) return rc;
    const int64_t *d_src = (const int64_t *)c->panelaux.p, *d_woff = d_src + nreads;
    double *d_wsig = (double *)c->panelwin.p;
    SK_HIP(hipMemcpyAsync(c->panelaux.p, aux.data(), aux.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_launch_region_rows_f64(c, (const double *)c->sig.p, d_src, d_woff, nreads, d_wsig))) return rc;
    sk_sdtw_args a;
    if ((rc = prep_f64(c, d_wsig, d_woff, nreads, wtotal, wmax, scale_mode, scale_low, scale_hi, &a))) return rc;
    a.motif = nullptr; a.nmotif = 0; a.out = nullptr; a.force_single = 1;
    sk_hit *d_all = (sk_hit *)c->panelrec.p;
    sk_panel_rec *d_out = (sk_panel_rec *)(d_all + (size_t)nreads * (size_t)nmotifs);
    if ((rc = sk_launch_panel_dtw(c, &a, motifs, motif_off, d_all, nreads))) return rc;
    if ((rc = sk_launch_panel_rank(c, d_all, nreads, nreads, nmotifs, d_out))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    SK_HIP(hipMemcpyAsync(out, d_out, (size_t)nreads * sizeof(sk_panel_rec), hipMemcpyDeviceToHost, c->stream));
    if (all) SK_HIP(hipMemcpyAsync(all, d_all, ab, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));                      // (aux goes out of scope)
    if (from) memcpy(from, lo_host.data(), (size_t)nreads * sizeof(int32_t));
    return SK_OK;
}

int sk_region_rows_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                       int32_t begin, int32_t end, const int32_t *win, int64_t wstride,
                       int16_t *rows, int32_t *wlen, int32_t *from)
{
    SK_ENTER(c);
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    if (wstride < 8 || wstride % 8) return sk_fail(SK_ERR_INVALID, "wstride must be a positive multiple of 8");
    if (nreads == 0) return SK_OK;
    if (!rows || !wlen) return sk_fail(SK_ERR_INVALID, "NULL rows/wlen");
    for (int32_t r = 0; r < nreads; r++) {
        int32_t lo, m;
        if ((rc = panel_window(r, len[r], begin, end, win, &lo, &m))) return rc;
        if (m > wstride) return sk_fail(SK_ERR_INVALID, "read %d: a window of %d samples does not fit wstride %lld", r, m, (long long)wstride);
    }
    const size_t wb = (size_t)nreads * (size_t)wstride * sizeof(int16_t);
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->panelwin, wb))) return rc;
    if ((rc = sk_reserve(c, &c->panelaux, (size_t)nreads * 4 * sizeof(int32_t)))) return rc;
    int32_t *d_wlen = (int32_t *)c->panelaux.p, *d_from = d_wlen + nreads, *d_win = nullptr;
    if (win) {
        d_win = d_from + nreads;
        SK_HIP(hipMemcpyAsync(d_win, win, (size_t)nreads * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    rc = ingest_rows(c, sub_batches(nreads, stride), (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return sk_launch_region_rows_i16(c, d_sig, stride, d_len, nr, begin, end,
                                                          d_win ? d_win + 2 * (size_t)r0 : nullptr,
                                                          (int16_t *)c->panelwin.p + (size_t)r0 * (size_t)wstride, wstride,
                                                          d_wlen + r0, d_from + r0);
                     });
    if (rc) return rc;
    SK_HIP(hipMemcpyAsync(rows, c->panelwin.p, wb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(wlen, d_wlen, (size_t)nreads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (from) SK_HIP(hipMemcpyAsync(from, d_from, (size_t)nreads * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ event detection (sk_detect.hip)
// The definition: include/squigglekit_hip.h, "event detection".  Mark and count per sub-batch, one scan over the whole
// call, then the records.
namespace {

// the ranges of sk_det_params (sk_detect_events_*, sk_evs_open)
int check_det_params(const sk_det_params *p)
{
    if (!p) return sk_fail(SK_ERR_INVALID, "NULL sk_det_params");
    if (p->w_short < 1 || p->w_short > p->w_long || p->w_long > 64)
        return sk_fail(SK_ERR_INVALID, "windows must satisfy 1 <= w_short <= w_long <= 64 (got %d, %d)", p->w_short, p->w_long);
    if (!isfinite(p->th_short) || !isfinite(p->th_long)) return sk_fail(SK_ERR_INVALID, "the thresholds must be finite");
    if (!isfinite(p->peak_height) || p->peak_height < 0) return sk_fail(SK_ERR_INVALID, "peak_height must be finite and >= 0");
    return SK_OK;
}

int check_detect(const void *sig, int64_t stride, const int32_t *len, int32_t nreads, const sk_det_params *p,
                 const int64_t *off, const sk_det_event *rec, int64_t cap)
{
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_det_params(p))) return rc;
    if (!off) return sk_fail(SK_ERR_INVALID, "NULL off");
    if (cap < 0) return sk_fail(SK_ERR_INVALID, "cap < 0");
    if (cap > 0 && !rec) return sk_fail(SK_ERR_INVALID, "NULL rec with a cap");
    if ((int64_t)nreads * sk_detect_words(stride) > ((int64_t)1 << 40))
        return sk_fail(SK_ERR_UNSUPPORTED, "detect: %d rows of %lld samples in one call", nreads, (long long)stride);
    return SK_OK;
}

} // namespace

extern "C" {

int sk_detect_events_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const sk_det_params *p, int64_t *d_off, sk_det_event *d_rec, int64_t cap)
{
    int rc = check_detect(d_sig, stride, d_len, nreads, p, d_off, d_rec, cap);
    if (rc) return rc;
    SK_ENTER(c);
    if (nreads == 0) {
        SK_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), c->stream));
        return SK_OK;
    }
    if ((rc = sk_reserve(c, &c->detect, sk_detect_work_bytes(nreads, stride)))) return rc;
    int64_t *d_bsum = (int64_t *)c->detect.p + (size_t)nreads * (size_t)sk_detect_words(stride);
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // sk_last_kernel_ms: no prep, main = mark + scan + fill
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if ((rc = sk_launch_detect_mark(c, d_sig, stride, d_len, nreads, p, c->detect.p, d_off))) return rc;
    if ((rc = sk_launch_detect_scan(c, nreads, d_bsum, d_off))) return rc;
    if ((rc = sk_launch_detect_fill(c, d_sig, stride, d_len, nreads, p, c->detect.p, d_off, d_rec, cap))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

int sk_detect_events_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads,
                         const sk_det_params *p, int64_t *off, sk_det_event *rec, int64_t cap)
{
    int rc = check_detect(sig, stride, len, nreads, p, off, rec, cap);
    if (rc) return rc;
    SK_ENTER(c);
    off[0] = 0;
    if (nreads == 0) return SK_OK;
    const SubBatches B = sub_batches(nreads, stride);
    const int64_t W = sk_detect_words(stride);
    const size_t off_bytes = ((size_t)nreads + 2) / 2 * 2 * sizeof(int64_t);         // (the records start 16-byte aligned)
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->detect, sk_detect_work_bytes(nreads, stride)))) return rc;
    if ((rc = sk_reserve(c, &c->detectout, off_bytes + (size_t)cap * sizeof(sk_det_event)))) return rc;
    uint64_t *d_words = (uint64_t *)c->detect.p;
    int64_t *d_bsum = (int64_t *)c->detect.p + (size_t)nreads * (size_t)W;
    int64_t *d_off = (int64_t *)c->detectout.p;
    sk_det_event *d_rec = cap > 0 ? (sk_det_event *)((char *)c->detectout.p + off_bytes) : nullptr;
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return sk_launch_detect_mark(c, d_sig, stride, d_len, nr, p, d_words + (size_t)r0 * (size_t)W, d_off + r0);
                     });
    if (rc) return rc;
    if ((rc = sk_launch_detect_scan(c, nreads, d_bsum, d_off))) return rc;
    SK_HIP(hipMemcpyAsync(off, d_off, ((size_t)nreads + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    const int64_t total = off[nreads];
    if (total > cap)
        return sk_fail(SK_ERR_OVERFLOW, "the reads hold %lld events, cap is %lld", (long long)total, (long long)cap);
    if (total == 0) return SK_OK;
    if ((rc = sk_launch_detect_fill(c, (const int16_t *)c->sig.p, stride, (const int32_t *)c->len.p, nreads, p, d_words, d_off,
                                    d_rec, cap)))
        return rc;
    SK_HIP(hipMemcpyAsync(rec, d_rec, (size_t)total * sizeof(sk_det_event), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ signal HMM (sk_hmm.hip)
// The definition: include/squigglekit_hip.h, "signal HMM".  One kernel per sub-batch; the records of the whole call come
// back in one copy.
namespace {

int check_hmm(const sk_hmm_model *model, int32_t limit, int32_t nreads, const sk_hmm_rec *rec)
{
    if (const char *what = sk_hmm_model_error(model)) return sk_fail(SK_ERR_INVALID, "sk_hmm_model: %s", what);
    if (limit < 0) return sk_fail(SK_ERR_INVALID, "limit < 0");
    if (nreads && !rec) return sk_fail(SK_ERR_INVALID, "NULL rec");
    return SK_OK;
}

} // namespace

extern "C" {

int sk_hmm_viterbi_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                           const sk_hmm_model *model, int32_t limit, sk_hmm_rec *d_rec)
{
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm(model, limit, nreads, d_rec))) return rc;
    SK_ENTER(c);
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // sk_last_kernel_ms: no prep, main = the kernel
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if ((rc = sk_launch_hmm_i16(c, d_sig, stride, d_len, nreads, d_cal2, model, limit, d_rec))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

int sk_hmm_viterbi_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                       const sk_hmm_model *model, int32_t limit, sk_hmm_rec *rec)
{
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm(model, limit, nreads, rec))) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    SK_ENTER(c);
    if (nreads == 0) return SK_OK;
    const size_t rec_bytes = (size_t)nreads * sizeof(sk_hmm_rec);                     // (40 bytes each: the pairs stay 8-byte aligned)
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->hmm, rec_bytes + (size_t)nreads * 2 * sizeof(double)))) return rc;
    sk_hmm_rec *d_rec = (sk_hmm_rec *)c->hmm.p;
    double *d_cal = cal2 ? (double *)((char *)c->hmm.p + rec_bytes) : nullptr;
    if (d_cal) SK_HIP(hipMemcpyAsync(d_cal, cal2, (size_t)nreads * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = ingest_rows(c, sub_batches(nreads, stride), (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return sk_launch_hmm_i16(c, d_sig, stride, d_len, nr, d_cal ? d_cal + 2 * (size_t)r0 : nullptr, model,
                                                  limit, d_rec + r0);
                     });
    if (rc) return rc;
    SK_HIP(hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_hmm_viterbi_f64_len(const double *values, const int64_t *off, int32_t nreads, const sk_hmm_model *model,
                           int32_t limit, sk_hmm_rec *rec)
{
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_hmm(model, limit, nreads, rec);
    if (rc) return rc;
    SK_ENTER(c);
    if (nreads == 0) return SK_OK;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, values, off, nreads, &total, &maxlen))) return rc;  // (checks values / off and the lengths)
    const size_t rec_bytes = (size_t)nreads * sizeof(sk_hmm_rec);
    if ((rc = sk_reserve(c, &c->hmm, rec_bytes))) return rc;
    sk_hmm_rec *d_rec = (sk_hmm_rec *)c->hmm.p;
    if ((rc = sk_launch_hmm_f64(c, (const double *)c->sig.p, (const int64_t *)c->off.p, nreads, model, limit, d_rec))) return rc;
    SK_HIP(hipMemcpyAsync(rec, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ signal HMM: state paths (sk_hmm.hip)
// The definition: include/squigglekit_hip.h, "signal HMM: state paths".  Per sub-batch and per slice of whole 64-read
// groups: the forward pass that keeps the back pointers, the running scan of the segment counts, the backward sweep;
// then the statistics of the whole call in one launch.
namespace {

int check_hmm_segments(const sk_hmm_model *model, int32_t limit, int32_t nreads, const sk_hmm_rec *rec, const int64_t *off,
                       const void *seg, int64_t cap)
{
    int rc = check_hmm(model, limit, nreads, rec);
    if (rc) return rc;
    if (!off) return sk_fail(SK_ERR_INVALID, "NULL off");
    if (cap < 0) return sk_fail(SK_ERR_INVALID, "cap < 0");
    if (cap > 0 && !seg) return sk_fail(SK_ERR_INVALID, "NULL seg with a cap");
    return SK_OK;
}

// off [nreads + 1] of a host entry point on the device, the records behind it (16-byte aligned)
size_t hmm_off_bytes(int32_t nreads) { return ((size_t)nreads + 2) / 2 * 2 * sizeof(int64_t); }

// rec, off and -- unless they overflow cap -- the segments of a host entry point, from the device
int hmm_segments_finish(sk_ctx *c, int32_t nreads, const sk_hmm_rec *d_rec, const int64_t *d_off, const void *d_seg,
                        sk_hmm_rec *rec, int64_t *off, void *seg, int64_t cap)
{
    SK_HIP(hipMemcpyAsync(rec, d_rec, (size_t)nreads * sizeof(sk_hmm_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(off, d_off, ((size_t)nreads + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    const int64_t total = off[nreads];
    if (total > cap)
        return sk_fail(SK_ERR_OVERFLOW, "the reads hold %lld segments, cap is %lld", (long long)total, (long long)cap);
    if (total == 0) return SK_OK;
    SK_HIP(hipMemcpyAsync(seg, d_seg, (size_t)total * sizeof(sk_hmm_seg), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // namespace

extern "C" {

int sk_hmm_segments_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads, const double *d_cal2,
                            const sk_hmm_model *model, int32_t limit, sk_hmm_rec *d_rec, int64_t *d_off, sk_hmm_seg *d_seg,
                            int64_t cap)
{
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm_segments(model, limit, nreads, d_rec, d_off, d_seg, cap))) return rc;
    SK_ENTER(c);
    if (nreads == 0) {
        SK_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), c->stream));
        return SK_OK;
    }
    const int64_t npad = sk_hmm_npad(stride, limit);
    if ((rc = sk_reserve(c, &c->hmmpath, sk_hmm_path_work_bytes(nreads, npad)))) return rc;
    if ((rc = sk_launch_hmm_paths(c, SK_FEED_I16, d_sig, stride, d_len, nullptr, nreads, d_cal2, model, limit, npad,
                                  c->hmmpath.p, 1, d_rec, d_off, d_seg, cap)))
        return rc;
    return sk_launch_hmm_stats(c, SK_FEED_I16, d_sig, stride, nullptr, nreads, d_cal2, model, d_off, d_seg, cap);
}

int sk_hmm_segments_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                        const sk_hmm_model *model, int32_t limit, sk_hmm_rec *rec, int64_t *off, sk_hmm_seg *seg, int64_t cap)
{
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm_segments(model, limit, nreads, rec, off, seg, cap))) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    SK_ENTER(c);
    off[0] = 0;
    if (nreads == 0) return SK_OK;
    const SubBatches B = sub_batches(nreads, stride);
    const int64_t npad = sk_hmm_npad(stride, limit);
    const size_t rec_bytes = (size_t)nreads * sizeof(sk_hmm_rec), off_bytes = hmm_off_bytes(nreads);
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->hmm, rec_bytes + (size_t)nreads * 2 * sizeof(double)))) return rc;
    if ((rc = sk_reserve(c, &c->hmmpath, sk_hmm_path_work_bytes(B.per, npad)))) return rc;
    if ((rc = sk_reserve(c, &c->hmmseg, off_bytes + (size_t)cap * sizeof(sk_hmm_seg)))) return rc;
    sk_hmm_rec *d_rec = (sk_hmm_rec *)c->hmm.p;
    double *d_cal = cal2 ? (double *)((char *)c->hmm.p + rec_bytes) : nullptr;
    int64_t *d_off = (int64_t *)c->hmmseg.p;
    sk_hmm_seg *d_seg = cap > 0 ? (sk_hmm_seg *)((char *)c->hmmseg.p + off_bytes) : nullptr;
    if (d_cal) SK_HIP(hipMemcpyAsync(d_cal, cal2, (size_t)nreads * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return sk_launch_hmm_paths(c, SK_FEED_I16, d_sig, stride, d_len, nullptr, nr,
                                                    d_cal ? d_cal + 2 * (size_t)r0 : nullptr, model, limit, npad, c->hmmpath.p,
                                                    r0 == 0, d_rec + r0, d_off + r0, d_seg, cap);
                     });
    if (rc) return rc;
    if ((rc = sk_launch_hmm_stats(c, SK_FEED_I16, c->sig.p, stride, nullptr, nreads, d_cal, model, d_off, d_seg, cap))) return rc;
    return hmm_segments_finish(c, nreads, d_rec, d_off, d_seg, rec, off, seg, cap);
}

int sk_hmm_segments_f64_len(const double *values, const int64_t *in_off, int32_t nreads, const sk_hmm_model *model,
                            int32_t limit, sk_hmm_rec *rec, int64_t *off, sk_hmm_segf *seg, int64_t cap)
{
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_hmm_segments(model, limit, nreads, rec, off, seg, cap);
    if (rc) return rc;
    if (!values || !in_off) return sk_fail(SK_ERR_INVALID, "NULL values/off");
    SK_ENTER(c);
    off[0] = 0;
    if (nreads == 0) return SK_OK;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, values, in_off, nreads, &total, &maxlen))) return rc;   // (checks the lengths)
    const int64_t npad = sk_hmm_npad(maxlen, limit);
    const size_t rec_bytes = (size_t)nreads * sizeof(sk_hmm_rec), off_bytes = hmm_off_bytes(nreads);
    if ((rc = sk_reserve(c, &c->hmm, rec_bytes))) return rc;
    if ((rc = sk_reserve(c, &c->hmmpath, sk_hmm_path_work_bytes(nreads, npad)))) return rc;
    if ((rc = sk_reserve(c, &c->hmmseg, off_bytes + (size_t)cap * sizeof(sk_hmm_segf)))) return rc;
    sk_hmm_rec *d_rec = (sk_hmm_rec *)c->hmm.p;
    int64_t *d_off = (int64_t *)c->hmmseg.p;
    sk_hmm_segf *d_seg = cap > 0 ? (sk_hmm_segf *)((char *)c->hmmseg.p + off_bytes) : nullptr;
    if ((rc = sk_launch_hmm_paths(c, SK_FEED_F64_NORM, c->sig.p, 0, nullptr, (const int64_t *)c->off.p, nreads, nullptr, model,
                                  limit, npad, c->hmmpath.p, 1, d_rec, d_off, (sk_hmm_seg *)d_seg, cap)))
        return rc;
    if ((rc = sk_launch_hmm_stats(c, SK_FEED_F64_NORM, c->sig.p, 0, (const int64_t *)c->off.p, nreads, nullptr, model, d_off,
                                  d_seg, cap)))
        return rc;
    return hmm_segments_finish(c, nreads, d_rec, d_off, d_seg, rec, off, seg, cap);
}

} // extern "C"

// ------------------------------------------------------------------ signal HMM: posteriors (sk_hmm_post.hip)
// The definition: include/squigglekit_hip.h, "signal HMM: posteriors".  Per sub-batch and per slice of whole 64-read
// groups: the forward kernel, then the backward kernel; records, counts and dense rows of the whole call come back in one
// copy each.
namespace {

int check_hmm_post(const sk_hmm_model *model, int32_t limit, int32_t nreads, const sk_hmm_post *post, const int64_t *goff,
                   const double *gamma)
{
    if (const char *what = sk_hmm_model_error(model)) return sk_fail(SK_ERR_INVALID, "sk_hmm_model: %s", what);
    if (limit < 0) return sk_fail(SK_ERR_INVALID, "limit < 0");
    if (nreads && !post) return sk_fail(SK_ERR_INVALID, "NULL post");
    if ((goff == nullptr) != (gamma == nullptr)) return sk_fail(SK_ERR_INVALID, "goff and gamma must both be given or both be NULL");
    return SK_OK;
}

// host forms: goff must be the running sum of the samples each read uses, from 0 -- the kernel writes by it
template <class Len>
int check_goff_host(const int64_t *goff, int32_t nreads, int32_t limit, Len len_of)
{
    if (!goff) return SK_OK;
    if (goff[0] != 0) return sk_fail(SK_ERR_INVALID, "goff[0] must be 0");
    for (int32_t r = 0; r < nreads; r++) {
        int64_t n = len_of(r);
        if (n > 0x7fffff00) n = 0x7fffff00;
        if (limit > 0 && n > limit) n = limit;
        if (goff[r + 1] - goff[r] != n)
            return sk_fail(SK_ERR_INVALID, "goff[%d + 1] - goff[%d] = %lld, the read uses %lld samples", r, r,
                           (long long)(goff[r + 1] - goff[r]), (long long)n);
    }
    return SK_OK;
}

// the device side of a host form's outputs in c->hmm (records, then calibration pairs) and c->hmmpostout (counts, goff,
// dense rows)
struct PostOut {
    sk_hmm_post   *post = nullptr;
    double        *cal = nullptr;
    sk_hmm_counts *counts = nullptr;
    int64_t       *goff = nullptr;
    double        *gamma = nullptr;
    size_t         gamma_bytes = 0;
};

int post_out_reserve(sk_ctx *c, int32_t nreads, const double *cal2, bool counts, const int64_t *goff, PostOut *o)
{
    int rc;
    const size_t post_bytes = (size_t)nreads * sizeof(sk_hmm_post);
    if ((rc = sk_reserve(c, &c->hmm, post_bytes + (size_t)nreads * 2 * sizeof(double)))) return rc;
    o->post = (sk_hmm_post *)c->hmm.p;
    if (cal2) {
        o->cal = (double *)((char *)c->hmm.p + post_bytes);
        SK_HIP(hipMemcpyAsync(o->cal, cal2, (size_t)nreads * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    const size_t cnt_bytes = counts ? (size_t)nreads * sizeof(sk_hmm_counts) : 0;
    const size_t goff_bytes = goff ? ((size_t)nreads + 1) * sizeof(int64_t) : 0;
    o->gamma_bytes = goff ? (size_t)goff[nreads] * SK_HMM_STATES * sizeof(double) : 0;
    if ((rc = sk_reserve(c, &c->hmmpostout, cnt_bytes + goff_bytes + o->gamma_bytes + 16))) return rc;
    char *p = (char *)c->hmmpostout.p;
    if (counts) o->counts = (sk_hmm_counts *)p;
    if (goff) {
        o->goff = (int64_t *)(p + cnt_bytes);
        o->gamma = (double *)(p + cnt_bytes + goff_bytes);
        SK_HIP(hipMemcpyAsync(o->goff, goff, goff_bytes, hipMemcpyHostToDevice, c->stream));
    }
    return SK_OK;
}

int post_out_finish(sk_ctx *c, int32_t nreads, const PostOut &o, sk_hmm_post *post, sk_hmm_counts *counts, double *gamma)
{
    SK_HIP(hipMemcpyAsync(post, o.post, (size_t)nreads * sizeof(sk_hmm_post), hipMemcpyDeviceToHost, c->stream));
    if (counts) SK_HIP(hipMemcpyAsync(counts, o.counts, (size_t)nreads * sizeof(sk_hmm_counts), hipMemcpyDeviceToHost, c->stream));
    if (gamma && o.gamma_bytes) SK_HIP(hipMemcpyAsync(gamma, o.gamma, o.gamma_bytes, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // namespace

extern "C" {

int sk_hmm_posterior_dev_i16(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                             const double *d_cal2, const sk_hmm_model *model, int32_t limit, sk_hmm_post *d_post,
                             sk_hmm_counts *d_counts, const int64_t *d_goff, double *d_gamma)
{
    int rc = check_i16(d_sig, stride, d_len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm_post(model, limit, nreads, d_post, d_goff, d_gamma))) return rc;
    SK_ENTER(c);
    if (nreads == 0) return SK_OK;
    const int64_t npad = sk_hmm_npad(stride, limit);
    if ((rc = sk_reserve(c, &c->hmmpost, sk_hmm_post_work_bytes(nreads, npad)))) return rc;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // sk_last_kernel_ms: no prep, main = the kernels
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if ((rc = sk_launch_hmm_post(c, SK_FEED_I16, d_sig, stride, d_len, nullptr, nreads, d_cal2, model, limit, npad,
                                 c->hmmpost.p, d_post, d_counts, d_goff, d_gamma)))
        return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

int sk_hmm_posterior_i16(const int16_t *sig, int64_t stride, const int32_t *len, int32_t nreads, const double *cal2,
                         const sk_hmm_model *model, int32_t limit, sk_hmm_post *post, sk_hmm_counts *counts,
                         const int64_t *goff, double *gamma)
{
    int rc = check_i16(sig, stride, len, nreads);
    if (rc) return rc;
    if ((rc = check_hmm_post(model, limit, nreads, post, goff, gamma))) return rc;
    if ((rc = check_len_host(len, nreads, stride))) return rc;
    if ((rc = check_goff_host(goff, nreads, limit, [&](int32_t r) { return (int64_t)len[r]; }))) return rc;
    SK_ENTER(c);
    if (nreads == 0) return SK_OK;
    const SubBatches B = sub_batches(nreads, stride);
    const int64_t npad = sk_hmm_npad(stride, limit);
    PostOut o;
    if ((rc = sk_reserve(c, &c->sig, (size_t)nreads * (size_t)stride * sizeof(int16_t)))) return rc;
    if ((rc = sk_reserve(c, &c->len, (size_t)nreads * sizeof(int32_t)))) return rc;
    if ((rc = sk_reserve(c, &c->hmmpost, sk_hmm_post_work_bytes(B.per, npad)))) return rc;
    if ((rc = post_out_reserve(c, nreads, cal2, counts != nullptr, goff, &o))) return rc;
    rc = ingest_rows(c, B, (int16_t *)c->sig.p, sig, stride, len, nreads,
                     [&](int32_t r0, int32_t nr, const int16_t *d_sig, const int32_t *d_len) {
                         return sk_launch_hmm_post(c, SK_FEED_I16, d_sig, stride, d_len, nullptr, nr,
                                                   o.cal ? o.cal + 2 * (size_t)r0 : nullptr, model, limit, npad, c->hmmpost.p,
                                                   o.post + r0, o.counts ? o.counts + r0 : nullptr,
                                                   o.goff ? o.goff + r0 : nullptr, o.gamma);
                     });
    if (rc) return rc;
    return post_out_finish(c, nreads, o, post, counts, gamma);
}

int sk_hmm_posterior_f64_len(const double *values, const int64_t *off, int32_t nreads, const sk_hmm_model *model,
                             int32_t limit, sk_hmm_post *post, sk_hmm_counts *counts, const int64_t *goff, double *gamma)
{
    if (nreads < 0) return sk_fail(SK_ERR_INVALID, "nreads < 0");
    int rc = check_hmm_post(model, limit, nreads, post, goff, gamma);
    if (rc) return rc;
    if (nreads && (!values || !off)) return sk_fail(SK_ERR_INVALID, "NULL values/off");
    for (int32_t r = 0; r < nreads; r++)
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "bad length for read %d", r);
    if ((rc = check_goff_host(goff, nreads, limit, [&](int32_t r) { return off[r + 1] - off[r]; }))) return rc;
    SK_ENTER(c);
    if (nreads == 0) return SK_OK;
    int64_t total, maxlen;
    if ((rc = stage_ragged_f64(c, values, off, nreads, &total, &maxlen))) return rc;
    const int64_t npad = sk_hmm_npad(maxlen, limit);
    PostOut o;
    if ((rc = sk_reserve(c, &c->hmmpost, sk_hmm_post_work_bytes(nreads, npad)))) return rc;
    if ((rc = post_out_reserve(c, nreads, nullptr, counts != nullptr, goff, &o))) return rc;
    if ((rc = sk_launch_hmm_post(c, SK_FEED_F64_NORM, c->sig.p, 0, nullptr, (const int64_t *)c->off.p, nreads, nullptr, model,
                                 limit, npad, c->hmmpost.p, o.post, o.counts, o.goff, o.gamma)))
        return rc;
    return post_out_finish(c, nreads, o, post, counts, gamma);
}

} // extern "C"

// ------------------------------------------------------------------ MotifSeq sessions (sk_stream.hip)
// Chunk-by-chunk search: the host forms check what the caller handed over, stage it in the session's own buffers and
// run the device form; the records come back behind one synchronisation.
namespace {

int check_stream_slots(int32_t nslots, const int32_t *slots, int32_t m, std::vector<uint8_t> &seen)
{
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    seen.assign((size_t)nslots, 0);
    for (int32_t i = 0; i < m; i++) {
        if (slots[i] < 0 || slots[i] >= nslots)
            return sk_fail(SK_ERR_INVALID, "slots[%d] = %d is outside [0, %d)", i, slots[i], nslots);
        if (seen[(size_t)slots[i]]) return sk_fail(SK_ERR_INVALID, "slot %d appears twice in one call", slots[i]);
        seen[(size_t)slots[i]] = 1;
    }
    return SK_OK;
}

// slots (and rows, len when given) to the session's staging, the device form, the records back
int stream_host_call(sk_ctx *c, int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                     const int32_t *len, int flush, sk_stream_rec *out)
{
    int32_t nslots = 0, K = 0;
    int rc = sk_stream_session_info(c, handle, &nslots, &K);
    if (rc) return rc;
    std::vector<uint8_t> seen;
    if ((rc = check_stream_slots(nslots, slots, m, seen))) return rc;
    if (m == 0) return SK_OK;
    if (!out) return sk_fail(SK_ERR_INVALID, "NULL out");
    if (rows || !flush) {
        if (!rows || !len) return sk_fail(SK_ERR_INVALID, "NULL rows/len");
        if (stride <= 0) return sk_fail(SK_ERR_INVALID, "stride must be positive");
        if ((rc = check_len_host(len, m, stride))) return rc;
    }
    void *d_slots, *d_rows = nullptr, *d_len = nullptr, *d_out;
    const size_t ob = (size_t)m * (size_t)K * sizeof(sk_stream_rec);
    if ((rc = sk_stream_session_stage(c, handle, 0, (size_t)m * sizeof(int32_t), &d_slots))) return rc;
    if ((rc = sk_stream_session_stage(c, handle, 3, ob, &d_out))) return rc;
    SK_HIP(hipMemcpyAsync(d_slots, slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (rows) {
        if ((rc = sk_stream_session_stage(c, handle, 1, (size_t)m * (size_t)stride * sizeof(int16_t), &d_rows))) return rc;
        if ((rc = sk_stream_session_stage(c, handle, 2, (size_t)m * sizeof(int32_t), &d_len))) return rc;
        // only the samples of each row that count travel
        int64_t longest = 0;
        for (int32_t i = 0; i < m; i++) if (len[i] > longest) longest = len[i];
        if (longest > 0)
            SK_HIP(hipMemcpy2DAsync(d_rows, (size_t)stride * sizeof(int16_t), rows, (size_t)stride * sizeof(int16_t),
                                    (size_t)longest * sizeof(int16_t), (size_t)m, hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipMemcpyAsync(d_len, len, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = sk_stream_session_push(c, handle, (const int32_t *)d_slots, m, (const int16_t *)d_rows, rows ? stride : 1,
                                     (const int32_t *)d_len, flush, (sk_stream_rec *)d_out))) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

} // namespace

extern "C" {

int sk_stream_open(const double *motifs, const int32_t *motif_off, int32_t nmotifs, const sk_stream_params *p,
                   int32_t *handle)
{
    // the arguments are checked before the device is looked at
    if (!p || !handle) return sk_fail(SK_ERR_INVALID, "NULL params/handle");
    int rc = check_multi(motifs, motif_off, nmotifs, p->scale_mode);
    if (rc) return rc;
    for (int32_t k = 0; k < nmotifs; k++)
        if (motif_off[k + 1] - motif_off[k] > 1024)
            return sk_fail(SK_ERR_UNSUPPORTED, "motif %d has %d points: a session takes motifs of at most 1024", k,
                           motif_off[k + 1] - motif_off[k]);
    if (p->calib < 1 || p->calib > SK_STREAM_MAX_CALIB)
        return sk_fail(SK_ERR_INVALID, "calib = %d is outside 1 .. %d", p->calib, SK_STREAM_MAX_CALIB);
    if (p->nslots < 1 || p->nslots > 65536) return sk_fail(SK_ERR_INVALID, "nslots = %d is outside 1 .. 65536", p->nslots);
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return sk_fail(SK_ERR_INVALID, "reserved words must be 0");
    SK_ENTER(c);
    sk_stream_params q = *p;
    clamp_limits(&q.scale_low, &q.scale_hi);
    return sk_stream_session_open(c, motifs, motif_off, nmotifs, &q, handle);
}

int sk_stream_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride,
                       const int32_t *len, sk_stream_rec *out)
{
    SK_ENTER(c);
    return stream_host_call(c, handle, slots, m, rows, stride, len, 0, out);
}

int sk_stream_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                           const int32_t *d_len, sk_stream_rec *d_out)
{
    SK_ENTER(c);
    int rc = sk_stream_session_info(c, handle, nullptr, nullptr);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m == 0) return SK_OK;
    if (!d_slots || !d_rows || !d_len || !d_out) return sk_fail(SK_ERR_INVALID, "NULL pointer");
    if (stride <= 0) return sk_fail(SK_ERR_INVALID, "stride must be positive");
    return sk_stream_session_push(c, handle, d_slots, m, d_rows, stride, d_len, 0, d_out);
}

int sk_stream_flush(int32_t handle, const int32_t *slots, int32_t m, sk_stream_rec *out)
{
    SK_ENTER(c);
    return stream_host_call(c, handle, slots, m, nullptr, 0, nullptr, 1, out);
}

int sk_stream_reset(int32_t handle, const int32_t *slots, int32_t m, const double *center, const double *scale)
{
    SK_ENTER(c);
    int32_t nslots = 0;
    int rc = sk_stream_session_info(c, handle, &nslots, nullptr);
    if (rc) return rc;
    std::vector<uint8_t> seen;
    if ((rc = check_stream_slots(nslots, slots, m, seen))) return rc;
    if ((center == nullptr) != (scale == nullptr)) return sk_fail(SK_ERR_INVALID, "center and scale: both or neither");
    for (int32_t i = 0; center && i < m; i++)
        if (!isfinite(center[i]) || !isfinite(scale[i]) || scale[i] == 0.0)
            return sk_fail(SK_ERR_INVALID, "slot %d: center %g / scale %g (both finite, scale not 0)", slots[i], center[i], scale[i]);
    if (m == 0) return SK_OK;
    void *d_slots, *d_cs = nullptr;
    if ((rc = sk_stream_session_stage(c, handle, 0, (size_t)m * sizeof(int32_t), &d_slots))) return rc;
    SK_HIP(hipMemcpyAsync(d_slots, slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (center) {
        if ((rc = sk_stream_session_stage(c, handle, 2, 2 * (size_t)m * sizeof(double), &d_cs))) return rc;
        SK_HIP(hipMemcpyAsync(d_cs, center, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipMemcpyAsync((double *)d_cs + m, scale, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    rc = sk_stream_session_reset(c, handle, (const int32_t *)d_slots, m, (const double *)d_cs,
                                 d_cs ? (const double *)d_cs + m : nullptr);
    if (rc) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_stream_close(int32_t handle)
{
    SK_ENTER(c);
    return sk_stream_session_close(c, handle);
}

} // extern "C"

// ------------------------------------------------------------------ mapping sessions (sk_mapstream.hip)
// What the arguments alone decide is refused here, before the device is looked at; what needs the session (is the
// handle open, does a slot lie below its nslots) in sk_mapstream.hip.
namespace {

int check_map_handle(int32_t handle)
{
    if (handle < 0 || handle >= SK_MAP_MAX_SESSIONS)
        return sk_fail(SK_ERR_INVALID, "mapping session handle %d is outside [0, %d)", handle, SK_MAP_MAX_SESSIONS);
    return SK_OK;
}

// the targets and the slot count of a mapping session (sk_map_open, sk_live_open): counts, lengths, the caps
int check_map_shape(const int64_t *target_off, int32_t ntargets, int32_t nslots)
{
    if (ntargets < 1 || ntargets > SK_MAP_MAX_TARGETS)
        return sk_fail(SK_ERR_INVALID, "ntargets = %d is outside 1 .. %d", ntargets, SK_MAP_MAX_TARGETS);
    if (nslots < 1 || nslots > SK_MAP_MAX_SLOTS)
        return sk_fail(SK_ERR_INVALID, "nslots = %d is outside 1 .. %d", nslots, SK_MAP_MAX_SLOTS);
    for (int32_t t = 0; t < ntargets; t++) {
        const int64_t M = target_off[t + 1] - target_off[t];
        if (M == 0) return sk_fail(SK_ERR_INVALID, "target %d is empty", t);
        if (M < 0 || M > 0x7fffff00) return sk_fail(SK_ERR_INVALID, "target %d: bad length %lld", t, (long long)M);
    }
    if ((int64_t)nslots * ntargets > ((int64_t)1 << 30))
        return sk_fail(SK_ERR_UNSUPPORTED, "nslots * ntargets = %lld above 1073741824", (long long)nslots * ntargets);
    const int64_t sumM = target_off[ntargets] - target_off[0];
    if (sumM > SK_MAP_MAX_STATE_BYTES / 12 / nslots)
        return sk_fail(SK_ERR_UNSUPPORTED, "row state of %lld bytes (%d slots x %lld target points x 12) above the cap of %lld",
                       (long long)nslots * (long long)sumM * 12, nslots, (long long)sumM, (long long)SK_MAP_MAX_STATE_BYTES);
    return SK_OK;
}

// host_slots: the slot numbers can be read here (range against the ABI's limit, none twice)
int check_map_push(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off, const void *out,
                   bool host_slots)
{
    if (int rc = check_map_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m == 0) return SK_OK;
    if (!slots || !off || !out) return sk_fail(SK_ERR_INVALID, "NULL slots/off/out");
    for (int32_t i = 0; i < m; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len < 0) return sk_fail(SK_ERR_INVALID, "entry %d: offsets not increasing", i);
        if (len > SK_MAP_MAX_CHUNK)
            return sk_fail(SK_ERR_UNSUPPORTED, "entry %d: chunk of %lld points (at most %d per push)", i, (long long)len,
                           SK_MAP_MAX_CHUNK);
    }
    if (off[m] > off[0] && !values) return sk_fail(SK_ERR_INVALID, "NULL values");
    if (!host_slots) return SK_OK;
    std::vector<uint8_t> seen((size_t)SK_MAP_MAX_SLOTS, 0);
    for (int32_t i = 0; i < m; i++) {
        if (slots[i] < 0 || slots[i] >= SK_MAP_MAX_SLOTS)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, slots[i], SK_MAP_MAX_SLOTS);
        if (seen[(size_t)slots[i]]) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d appears twice in one call", i, slots[i]);
        seen[(size_t)slots[i]] = 1;
    }
    return SK_OK;
}

} // namespace

extern "C" {

int sk_map_open(const double *targets, const int64_t *target_off, int32_t ntargets, int32_t nslots, int32_t *handle)
{
    if (!targets || !target_off || !handle) return sk_fail(SK_ERR_INVALID, "NULL targets/target_off/handle");
    if (int rc = check_map_shape(target_off, ntargets, nslots)) return rc;
    SK_ENTER(c);
    return sk_map_session_open(c, targets, target_off, ntargets, nslots, handle);
}

int sk_map_push_dev(int32_t handle, const int32_t *d_slots, int32_t m, const double *d_values, const int64_t *off,
                    sk_map_rec *d_out)
{
    int rc = check_map_push(handle, d_slots, m, d_values, off, d_out, false);
    if (rc) return rc;
    SK_ENTER(c);
    if ((rc = sk_map_session_info(c, handle, nullptr, nullptr))) return rc;
    if (m == 0) return SK_OK;
    std::vector<int32_t> slots((size_t)m);                  // the plan is made on the host: the slot numbers come back
    SK_HIP(hipMemcpyAsync(slots.data(), d_slots, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return sk_map_session_push(c, handle, slots.data(), m, d_values, off, d_out);
}

int sk_map_push(int32_t handle, const int32_t *slots, int32_t m, const double *values, const int64_t *off, sk_map_rec *out)
{
    int rc = check_map_push(handle, slots, m, values, off, out, true);
    if (rc) return rc;
    SK_ENTER(c);
    int32_t T = 0;
    if ((rc = sk_map_session_info(c, handle, nullptr, &T))) return rc;
    if (m == 0) return SK_OK;
    if ((rc = sk_map_session_check_slots(c, handle, slots, m))) return rc;
    const int64_t total = off[m] - off[0];
    const size_t ob = (size_t)m * (size_t)T * sizeof(sk_map_rec);
    void *d_values, *d_out;
    if ((rc = sk_map_session_stage(c, handle, 0, (size_t)total * sizeof(double), &d_values))) return rc;
    if ((rc = sk_map_session_stage(c, handle, 1, ob, &d_out))) return rc;
    if (total > 0)
        SK_HIP(hipMemcpyAsync(d_values, values + off[0], (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = sk_map_session_push(c, handle, slots, m, (const double *)d_values, off, (sk_map_rec *)d_out))) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_map_reset(int32_t handle, const int32_t *slots, int32_t m)
{
    int rc = check_map_handle(handle);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    SK_ENTER(c);
    if ((rc = sk_map_session_info(c, handle, nullptr, nullptr))) return rc;
    return sk_map_session_reset(c, handle, slots, m);
}

// hit lists from a session's stored rows: what the arguments alone decide, in sk_map_push's order, then the hit lists' rules
static int check_map_hits(int32_t handle, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist, const void *out,
                          const void *count, bool host_slots)
{
    if (int rc = check_map_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (int rc = check_hit_limits(max_hits, max_dist)) return rc;
    if (m == 0) return SK_OK;
    if (!slots || !out || !count) return sk_fail(SK_ERR_INVALID, "NULL slots/out/count");
    if (!host_slots) return SK_OK;
    std::vector<uint8_t> seen((size_t)SK_MAP_MAX_SLOTS, 0);
    for (int32_t i = 0; i < m; i++) {
        if (slots[i] < 0 || slots[i] >= SK_MAP_MAX_SLOTS)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, slots[i], SK_MAP_MAX_SLOTS);
        if (seen[(size_t)slots[i]]) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d appears twice in one call", i, slots[i]);
        seen[(size_t)slots[i]] = 1;
    }
    return SK_OK;
}

// the host form of the hit lists of an open mapping session (sk_map_hits, sk_live_hits on its inner session): m >= 1
static int map_hits_host(sk_ctx *c, int32_t handle, int32_t T, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist,
                         sk_hit *out, int32_t *count)
{
    int rc;
    if ((rc = sk_map_session_check_slots(c, handle, slots, m))) return rc;
    const size_t ob = (size_t)m * (size_t)T * (size_t)max_hits * sizeof(sk_hit), cb = (size_t)m * (size_t)T * sizeof(int32_t);
    void *d_out;
    if ((rc = sk_map_session_stage(c, handle, 1, ob + cb, &d_out))) return rc;
    int32_t *d_count = (int32_t *)((char *)d_out + ob);
    if ((rc = sk_map_session_hits(c, handle, slots, m, max_hits, max_dist, (sk_hit *)d_out, d_count))) return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(count, d_count, cb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_map_hits_dev(int32_t handle, const int32_t *d_slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *d_out,
                    int32_t *d_count)
{
    int rc = check_map_hits(handle, d_slots, m, max_hits, max_dist, d_out, d_count, false);
    if (rc) return rc;
    SK_ENTER(c);
    if ((rc = sk_map_session_info(c, handle, nullptr, nullptr))) return rc;
    if (m == 0) return SK_OK;
    std::vector<int32_t> slots((size_t)m);                  // the table is made on the host: the slot numbers come back
    SK_HIP(hipMemcpyAsync(slots.data(), d_slots, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return sk_map_session_hits(c, handle, slots.data(), m, max_hits, max_dist, d_out, d_count);
}

int sk_map_hits(int32_t handle, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *out, int32_t *count)
{
    int rc = check_map_hits(handle, slots, m, max_hits, max_dist, out, count, true);
    if (rc) return rc;
    SK_ENTER(c);
    int32_t T = 0;
    if ((rc = sk_map_session_info(c, handle, nullptr, &T))) return rc;
    if (m == 0) return SK_OK;
    return map_hits_host(c, handle, T, slots, m, max_hits, max_dist, out, count);
}

int sk_map_close(int32_t handle)
{
    if (int rc = check_map_handle(handle)) return rc;
    SK_ENTER(c);
    return sk_map_session_close(c, handle);
}

int sk_last_map_plan(int64_t *state_bytes, int64_t *entries, int64_t *launches)
{
    SK_ENTER(c);
    if (state_bytes) *state_bytes = c->map_state_bytes;
    if (entries) *entries = c->map_entries;
    if (launches) *launches = c->map_launches;
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ event sessions (sk_evstream.hip)
// What the arguments alone decide is refused here, before a context is looked for; what needs the session (is the handle
// open, does a slot lie below its nslots, has it ended, how many samples has it had) in sk_evstream.hip.
namespace {

int check_evs_handle(int32_t handle)
{
    if (handle < 0 || handle >= SK_EVS_MAX_SESSIONS)
        return sk_fail(SK_ERR_INVALID, "event session handle %d is outside [0, %d)", handle, SK_EVS_MAX_SESSIONS);
    return SK_OK;
}

// host: slots, len can be read here (len in [0, stride], slots inside the ABI's limit, none twice)
int check_evs_push(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                   const int64_t *off, const sk_det_event *rec, int64_t cap, bool host)
{
    if (int rc = check_evs_handle(handle)) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (!off) return sk_fail(SK_ERR_INVALID, "NULL off");
    if (cap < 0) return sk_fail(SK_ERR_INVALID, "cap < 0");
    if (cap > 0 && !rec) return sk_fail(SK_ERR_INVALID, "NULL rec with a cap");
    if (stride < 0) return sk_fail(SK_ERR_INVALID, "stride < 0");
    if (m == 0) return SK_OK;
    if (!slots || !len) return sk_fail(SK_ERR_INVALID, "NULL slots/len");
    if (stride > 0 && !rows) return sk_fail(SK_ERR_INVALID, "NULL rows");
    if (stride > 0x7fffffffll) return sk_fail(SK_ERR_INVALID, "stride = %lld above 2147483647", (long long)stride);
    if ((int64_t)m * (stride + 64) > ((int64_t)1 << 31))
        return sk_fail(SK_ERR_UNSUPPORTED, "event session push: %d rows of %lld samples in one call", m, (long long)stride);
    if (!host) return SK_OK;
    for (int32_t i = 0; i < m; i++)
        if (len[i] < 0 || len[i] > stride)
            return sk_fail(SK_ERR_INVALID, "entry %d: len = %d is outside [0, stride = %lld]", i, len[i], (long long)stride);
    for (int32_t i = 0; i < m; i++)
        if (slots[i] < 0 || slots[i] >= SK_EVS_MAX_SLOTS)
            return sk_fail(SK_ERR_INVALID, "entry %d: slot %d is outside [0, %d)", i, slots[i], SK_EVS_MAX_SLOTS);
    // none twice: the entries ordered by slot (and by entry among equals), so that the later entry of a pair is named
    std::vector<int32_t> order((size_t)m);
    for (int32_t i = 0; i < m; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return slots[a] != slots[b] ? slots[a] < slots[b] : a < b; });
    int32_t twice = -1;
    for (int32_t k = 1; k < m; k++)
        if (slots[order[(size_t)k]] == slots[order[(size_t)k - 1]] && (twice < 0 || order[(size_t)k] < twice)) twice = order[(size_t)k];
    if (twice >= 0) return sk_fail(SK_ERR_INVALID, "entry %d: slot %d appears twice in one call", twice, slots[twice]);
    return SK_OK;
}

} // namespace

extern "C" {

int sk_evs_open(const sk_det_params *p, int32_t nslots, int32_t *handle)
{
    if (int rc = check_det_params(p)) return rc;
    if (!handle) return sk_fail(SK_ERR_INVALID, "NULL handle");
    if (nslots < 1 || nslots > SK_EVS_MAX_SLOTS)
        return sk_fail(SK_ERR_INVALID, "nslots = %d is outside 1 .. %d", nslots, SK_EVS_MAX_SLOTS);
    SK_ENTER(c);
    return sk_evs_session_open(c, p, nslots, handle);
}

int sk_evs_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                        const int32_t *d_len, const int32_t *d_end, int64_t *d_off, sk_det_event *d_rec, int64_t cap)
{
    int rc = check_evs_push(handle, d_slots, m, d_rows, stride, d_len, d_off, d_rec, cap, false);
    if (rc) return rc;
    SK_ENTER(c);
    if ((rc = sk_evs_session_info(c, handle, nullptr))) return rc;
    const int64_t per = sk_evs_session_rows(c, handle, stride);
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // sk_last_kernel_ms: no prep, main = walk + scan + gather
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if ((rc = sk_evs_session_push(c, handle, d_slots, m, d_rows, stride, d_len, d_end, per, d_off, nullptr, nullptr, nullptr)))
        return rc;
    if ((rc = sk_evs_session_gather(c, handle, d_rec, cap))) return rc;
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    return SK_OK;
}

int sk_evs_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                    const int32_t *end, int64_t *off, sk_det_event *rec, int64_t cap)
{
    int rc = check_evs_push(handle, slots, m, rows, stride, len, off, rec, cap, true);
    if (rc) return rc;
    SK_ENTER(c);
    if ((rc = sk_evs_session_info(c, handle, nullptr))) return rc;
    if ((rc = sk_evs_session_check(c, handle, slots, m, len))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the staging buffers
    int32_t maxlen = 0;
    for (int32_t i = 0; i < m; i++) maxlen = len[i] > maxlen ? len[i] : maxlen;
    // the rows go up as [m][w], w = maxlen rounded up to 8 samples: 16-byte loads whatever the caller's stride
    const int64_t w = ((int64_t)maxlen + 7) / 8 * 8;
    const size_t mm = (size_t)(m > 0 ? m : 1);
    void *d_rows_v, *d_args_v;
    if ((rc = sk_evs_session_stage(c, handle, 0, mm * (size_t)w * sizeof(int16_t), &d_rows_v))) return rc;
    if ((rc = sk_evs_session_stage(c, handle, 1, 3 * mm * sizeof(int32_t), &d_args_v))) return rc;
    int16_t *d_rows = (int16_t *)d_rows_v;
    int32_t *d_slots = (int32_t *)d_args_v, *d_len = d_slots + mm, *d_end = d_len + mm;
    if (m > 0) {
        if (maxlen > 0)
            SK_HIP(hipMemcpy2DAsync(d_rows, (size_t)w * sizeof(int16_t), rows, (size_t)stride * sizeof(int16_t),
                                    (size_t)maxlen * sizeof(int16_t), (size_t)m, hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipMemcpyAsync(d_slots, slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        SK_HIP(hipMemcpyAsync(d_len, len, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (end) SK_HIP(hipMemcpyAsync(d_end, end, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const int64_t per = sk_evs_session_rows(c, handle, maxlen);
    const int64_t *k_off = nullptr;
    int32_t km = 0;
    if ((rc = sk_evs_session_push(c, handle, d_slots, m, d_rows, w, d_len, end ? d_end : nullptr, per, nullptr, slots, len, end)))
        return rc;
    if ((rc = sk_evs_session_last(c, handle, &k_off, &km))) return rc;
    SK_HIP(hipMemcpyAsync(off, k_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    const int64_t total = off[m];
    if (total > cap)
        return sk_fail(SK_ERR_OVERFLOW, "the push made %lld events, cap is %lld (sk_evs_fetch has them)", (long long)total,
                       (long long)cap);
    if (total == 0) return SK_OK;
    void *d_out;
    if ((rc = sk_evs_session_stage(c, handle, 2, (size_t)total * sizeof(sk_det_event), &d_out))) return rc;
    if ((rc = sk_evs_session_gather(c, handle, (sk_det_event *)d_out, total))) return rc;
    SK_HIP(hipMemcpyAsync(rec, d_out, (size_t)total * sizeof(sk_det_event), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_evs_fetch(int32_t handle, sk_det_event *rec, int64_t cap)
{
    int rc = check_evs_handle(handle);
    if (rc) return rc;
    if (cap < 0) return sk_fail(SK_ERR_INVALID, "cap < 0");
    if (cap > 0 && !rec) return sk_fail(SK_ERR_INVALID, "NULL rec with a cap");
    SK_ENTER(c);
    const int64_t *k_off = nullptr;
    int32_t m = 0;
    if ((rc = sk_evs_session_last(c, handle, &k_off, &m))) return rc;
    if (m == 0) return SK_OK;
    int64_t total = 0;
    SK_HIP(hipMemcpyAsync(&total, k_off + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if (total > cap)
        return sk_fail(SK_ERR_OVERFLOW, "the last push made %lld events, cap is %lld", (long long)total, (long long)cap);
    if (total == 0) return SK_OK;
    void *d_out;
    if ((rc = sk_evs_session_stage(c, handle, 2, (size_t)total * sizeof(sk_det_event), &d_out))) return rc;
    if ((rc = sk_evs_session_gather(c, handle, (sk_det_event *)d_out, total))) return rc;
    SK_HIP(hipMemcpyAsync(rec, d_out, (size_t)total * sizeof(sk_det_event), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_evs_reset(int32_t handle, const int32_t *slots, int32_t m)
{
    int rc = check_evs_handle(handle);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    SK_ENTER(c);
    if ((rc = sk_evs_session_info(c, handle, nullptr))) return rc;
    return sk_evs_session_reset(c, handle, slots, m);
}

int sk_evs_close(int32_t handle)
{
    if (int rc = check_evs_handle(handle)) return rc;
    SK_ENTER(c);
    return sk_evs_session_close(c, handle);
}

int sk_last_evs_plan(int64_t *state_bytes, int64_t *staged_records, int64_t *guard_hits)
{
    SK_ENTER(c);
    if (state_bytes) *state_bytes = c->evs_state_bytes;
    if (staged_records) *staged_records = c->evs_staged;
    if (guard_hits) {
        unsigned long long g = 0;
        if (c->evs_valid && c->evscnt.p) {
            SK_HIP(hipMemcpyAsync(&g, c->evscnt.p, sizeof(g), hipMemcpyDeviceToHost, c->stream));
            SK_HIP(hipStreamSynchronize(c->stream));
        }
        *guard_hits = (int64_t)g;
    }
    return SK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ live mapping sessions (sk_live.hip)
// What the arguments alone decide is refused here, before a context is looked for, in the order of sk_evs_push_i16 /
// sk_map_open; what needs the session (is the handle open, does a slot lie below its nslots, has it ended, does the
// stride fit the mapping side's chunk limit) in sk_live.hip.
namespace {

int check_live_handle(int32_t handle)
{
    if (handle < 0 || handle >= SK_LIVE_MAX_SESSIONS)
        return sk_fail(SK_ERR_INVALID, "live session handle %d is outside [0, %d)", handle, SK_LIVE_MAX_SESSIONS);
    return SK_OK;
}

int check_live_push(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                    const sk_live_rule *rule, const void *out, const void *info, const void *best, bool host)
{
    if (int rc = check_live_handle(handle)) return rc;
    const int64_t off_stands_in = 0;                        // (sk_evs_push's checks of off / rec / cap have nothing to find)
    if (int rc = check_evs_push(0, slots, m, rows, stride, len, &off_stands_in, nullptr, 0, host)) return rc;
    if (m > 0 && (!out || !info)) return sk_fail(SK_ERR_INVALID, "NULL out/info");
    if (best && !rule) return sk_fail(SK_ERR_INVALID, "best without a rule");
    if (rule && !best && m > 0) return sk_fail(SK_ERR_INVALID, "a rule without best");
    if (rule) {
        if (rule->max_dist_per_row != rule->max_dist_per_row || rule->min_margin != rule->min_margin)
            return sk_fail(SK_ERR_INVALID, "rule: max_dist_per_row and min_margin must be numbers");
        if (rule->give_up_rows < 1) return sk_fail(SK_ERR_INVALID, "rule: give_up_rows = %d is below 1", rule->give_up_rows);
    }
    return SK_OK;
}

} // namespace

extern "C" {

int sk_live_open(const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off, int32_t ntargets,
                 int32_t nslots, int32_t *handle)
{
    if (int rc = check_det_params(p)) return rc;
    if (!handle) return sk_fail(SK_ERR_INVALID, "NULL handle");
    if (calib < 2 || calib > SK_LIVE_MAX_CALIB)
        return sk_fail(SK_ERR_INVALID, "calib = %d is outside 2 .. %d", calib, SK_LIVE_MAX_CALIB);
    if (!targets || !target_off) return sk_fail(SK_ERR_INVALID, "NULL targets/target_off");
    if (int rc = check_map_shape(target_off, ntargets, nslots)) return rc;
    SK_ENTER(c);
    return sk_live_session_open(c, p, calib, targets, target_off, ntargets, nslots, nullptr, nullptr, handle);
}

int sk_live_open_gated(const sk_det_params *p, int32_t calib, const double *targets, const int64_t *target_off, int32_t ntargets,
                       int32_t nslots, const sk_hmm_model *model, const sk_live_gate *gate, int32_t *handle)
{
    if (int rc = check_det_params(p)) return rc;
    if (!handle) return sk_fail(SK_ERR_INVALID, "NULL handle");
    if (calib < 2 || calib > SK_LIVE_MAX_CALIB)
        return sk_fail(SK_ERR_INVALID, "calib = %d is outside 2 .. %d", calib, SK_LIVE_MAX_CALIB);
    if (!targets || !target_off) return sk_fail(SK_ERR_INVALID, "NULL targets/target_off");
    if (int rc = check_map_shape(target_off, ntargets, nslots)) return rc;
    if (!model || !gate) return sk_fail(SK_ERR_INVALID, "NULL model/gate");
    if (const char *what = sk_hmm_model_error(model)) return sk_fail(SK_ERR_INVALID, "sk_hmm_model: %s", what);
    if (gate->state < 0 || gate->state >= model->nstates)
        return sk_fail(SK_ERR_INVALID, "gate: state = %d is outside [0, nstates = %d)", gate->state, model->nstates);
    if (gate->min_body < 1) return sk_fail(SK_ERR_INVALID, "gate: min_body = %d is below 1", gate->min_body);
    if (gate->hold < 1 || gate->hold > SK_LIVE_MAX_GATE_HOLD)
        return sk_fail(SK_ERR_INVALID, "gate: hold = %d is outside 1 .. %d", gate->hold, SK_LIVE_MAX_GATE_HOLD);
    if (gate->min_margin != gate->min_margin) return sk_fail(SK_ERR_INVALID, "gate: min_margin must be a number");
    SK_ENTER(c);
    return sk_live_session_open(c, p, calib, targets, target_off, ntargets, nslots, model, gate, handle);
}

int sk_live_push_dev_i16(int32_t handle, const int32_t *d_slots, int32_t m, const int16_t *d_rows, int64_t stride,
                         const int32_t *d_len, const int32_t *d_end, const sk_live_rule *rule, sk_map_rec *d_out,
                         sk_live_info *d_info, sk_live_best *d_best)
{
    int rc = check_live_push(handle, d_slots, m, d_rows, stride, d_len, rule, d_out, d_info, d_best, false);
    if (rc) return rc;
    SK_ENTER(c);
    int32_t evs = -1;
    if ((rc = sk_live_session_info(c, handle, nullptr, nullptr, &evs, nullptr))) return rc;
    if (m == 0) return SK_OK;
    std::vector<int32_t> slots((size_t)m);                  // the sweep is planned on the host: the slot numbers come back
    SK_HIP(hipMemcpyAsync(slots.data(), d_slots, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = sk_live_session_check(c, handle, slots.data(), m, stride, nullptr))) return rc;
    const int64_t per = sk_evs_session_rows(c, evs, stride);
    return sk_live_session_push(c, handle, slots.data(), d_slots, m, d_rows, stride, d_len, d_end, per, nullptr, nullptr, rule,
                                d_out, d_info, d_best);
}

int sk_live_push_i16(int32_t handle, const int32_t *slots, int32_t m, const int16_t *rows, int64_t stride, const int32_t *len,
                     const int32_t *end, const sk_live_rule *rule, sk_map_rec *out, sk_live_info *info, sk_live_best *best)
{
    int rc = check_live_push(handle, slots, m, rows, stride, len, rule, out, info, best, true);
    if (rc) return rc;
    SK_ENTER(c);
    int32_t evs = -1, T = 0;
    if ((rc = sk_live_session_info(c, handle, nullptr, &T, &evs, nullptr))) return rc;
    if (m == 0) return SK_OK;
    if ((rc = sk_live_session_check(c, handle, slots, m, stride, len))) return rc;
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the staging buffers
    int32_t maxlen = 0;
    for (int32_t i = 0; i < m; i++) maxlen = len[i] > maxlen ? len[i] : maxlen;
    // the rows go up as [m][w], w = maxlen rounded up to 8 samples, as in sk_evs_push_i16
    const int64_t w = ((int64_t)maxlen + 7) / 8 * 8;
    const size_t mm = (size_t)m;
    const size_t ob = mm * (size_t)T * sizeof(sk_map_rec), ib = mm * sizeof(sk_live_info), bb = mm * sizeof(sk_live_best);
    void *d_rows_v, *d_args_v, *d_out, *d_info, *d_best = nullptr;
    if ((rc = sk_evs_session_stage(c, evs, 0, mm * (size_t)w * sizeof(int16_t), &d_rows_v))) return rc;
    if ((rc = sk_evs_session_stage(c, evs, 1, 3 * mm * sizeof(int32_t), &d_args_v))) return rc;
    if ((rc = sk_live_session_stage(c, handle, 0, ob, &d_out))) return rc;
    if ((rc = sk_live_session_stage(c, handle, 1, ib, &d_info))) return rc;
    if (rule && (rc = sk_live_session_stage(c, handle, 2, bb, &d_best))) return rc;
    int16_t *d_rows = (int16_t *)d_rows_v;
    int32_t *d_slots = (int32_t *)d_args_v, *d_len = d_slots + mm, *d_end = d_len + mm;
    if (maxlen > 0)
        SK_HIP(hipMemcpy2DAsync(d_rows, (size_t)w * sizeof(int16_t), rows, (size_t)stride * sizeof(int16_t),
                                (size_t)maxlen * sizeof(int16_t), mm, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_slots, slots, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemcpyAsync(d_len, len, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (end) SK_HIP(hipMemcpyAsync(d_end, end, mm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const int64_t per = sk_evs_session_rows(c, evs, maxlen);
    if ((rc = sk_live_session_push(c, handle, slots, d_slots, m, d_rows, w, d_len, end ? d_end : nullptr, per, len, end, rule,
                                   (sk_map_rec *)d_out, (sk_live_info *)d_info, (sk_live_best *)d_best)))
        return rc;
    SK_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipMemcpyAsync(info, d_info, ib, hipMemcpyDeviceToHost, c->stream));
    if (rule) SK_HIP(hipMemcpyAsync(best, d_best, bb, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_live_fetch(int32_t handle, int64_t *off, double *values, int64_t cap)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    if (!off) return sk_fail(SK_ERR_INVALID, "NULL off");
    if (cap < 0) return sk_fail(SK_ERR_INVALID, "cap < 0");
    if (cap > 0 && !values) return sk_fail(SK_ERR_INVALID, "NULL values with a cap");
    SK_ENTER(c);
    const int64_t *k_off = nullptr;
    const double *k_values = nullptr;
    int32_t m = 0;
    if ((rc = sk_live_session_last(c, handle, &k_off, &k_values, &m))) return rc;
    if (m == 0) return SK_OK;
    SK_HIP(hipMemcpyAsync(off, k_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    const int64_t total = off[m];
    if (total > cap)
        return sk_fail(SK_ERR_OVERFLOW, "the last push made %lld normalised levels, cap is %lld", (long long)total, (long long)cap);
    if (total == 0) return SK_OK;
    SK_HIP(hipMemcpyAsync(values, k_values, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_live_hits(int32_t handle, const int32_t *slots, int32_t m, int32_t max_hits, double max_dist, sk_hit *out, int32_t *count)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    if ((rc = check_map_hits(0, slots, m, max_hits, max_dist, out, count, true))) return rc;
    SK_ENTER(c);
    int32_t T = 0, map = -1;
    if ((rc = sk_live_session_info(c, handle, nullptr, &T, nullptr, &map))) return rc;
    if (m == 0) return SK_OK;
    return map_hits_host(c, map, T, slots, m, max_hits, max_dist, out, count);
}

int sk_live_reset(int32_t handle, const int32_t *slots, int32_t m)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    SK_ENTER(c);
    if ((rc = sk_live_session_info(c, handle, nullptr, nullptr, nullptr, nullptr))) return rc;
    return sk_live_session_reset(c, handle, slots, m, nullptr);
}

int sk_live_reset_cal(int32_t handle, const int32_t *slots, int32_t m, const double *cal2)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    if (m < 0) return sk_fail(SK_ERR_INVALID, "m < 0");
    if (m && !slots) return sk_fail(SK_ERR_INVALID, "NULL slots");
    if (!cal2) return sk_fail(SK_ERR_INVALID, "NULL cal2");
    for (int32_t i = 0; i < 2 * m; i++)
        if (!(cal2[i] - cal2[i] == 0.0))
            return sk_fail(SK_ERR_INVALID, "entry %d: the calibration pair {offset, unit} must be finite", i / 2);
    SK_ENTER(c);
    if ((rc = sk_live_session_info(c, handle, nullptr, nullptr, nullptr, nullptr))) return rc;
    return sk_live_session_reset(c, handle, slots, m, cal2);
}

int sk_live_gate_fetch(int32_t handle, sk_live_gate_info *gate, sk_hmms_rec *rec)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    SK_ENTER(c);
    const sk_live_gate_info *k_gate = nullptr;
    const sk_hmms_rec *k_rec = nullptr;
    int32_t m = 0;
    if ((rc = sk_live_session_gate_last(c, handle, &k_gate, &k_rec, &m))) return rc;
    if (m == 0) return SK_OK;
    if (gate) SK_HIP(hipMemcpyAsync(gate, k_gate, (size_t)m * sizeof(sk_live_gate_info), hipMemcpyDeviceToHost, c->stream));
    if (rec) SK_HIP(hipMemcpyAsync(rec, k_rec, (size_t)m * sizeof(sk_hmms_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_live_gate_fetch_dev(int32_t handle, sk_live_gate_info *d_gate, sk_hmms_rec *d_rec)
{
    int rc = check_live_handle(handle);
    if (rc) return rc;
    SK_ENTER(c);
    const sk_live_gate_info *k_gate = nullptr;
    const sk_hmms_rec *k_rec = nullptr;
    int32_t m = 0;
    if ((rc = sk_live_session_gate_last(c, handle, &k_gate, &k_rec, &m))) return rc;
    if (m == 0) return SK_OK;
    if (d_gate) SK_HIP(hipMemcpyAsync(d_gate, k_gate, (size_t)m * sizeof(sk_live_gate_info), hipMemcpyDeviceToDevice, c->stream));
    if (d_rec) SK_HIP(hipMemcpyAsync(d_rec, k_rec, (size_t)m * sizeof(sk_hmms_rec), hipMemcpyDeviceToDevice, c->stream));
    return SK_OK;
}

int sk_live_close(int32_t handle)
{
    if (int rc = check_live_handle(handle)) return rc;
    SK_ENTER(c);
    return sk_live_session_close(c, handle);
}

int sk_live_last_ms(int32_t handle, float *bridge_ms, float *summary_ms)
{
    if (int rc = check_live_handle(handle)) return rc;
    SK_ENTER(c);
    float best = 0.f, prep = 0.f;
    if (int rc = sk_live_session_best_ms(c, handle, &best)) return rc;
    if (!c->ev_valid) return sk_fail(SK_ERR_INVALID, "no timed call yet");
    SK_HIP(hipEventSynchronize(c->ev[3]));
    SK_HIP(hipEventElapsedTime(&prep, c->ev[0], c->ev[1]));
    if (bridge_ms) *bridge_ms = prep;
    if (summary_ms) *summary_ms = best;
    return SK_OK;
}

int sk_live_gate_last_ms(int32_t handle, float *hmm_ms, float *gate_ms)
{
    if (int rc = check_live_handle(handle)) return rc;
    SK_ENTER(c);
    float h = 0.f, g = 0.f;
    if (int rc = sk_live_session_gate_ms(c, handle, &h, &g)) return rc;
    if (hmm_ms) *hmm_ms = h;
    if (gate_ms) *gate_ms = g;
    return SK_OK;
}

int sk_last_live_plan(int64_t *state_bytes, int64_t *bridged_levels, int64_t *launches)
{
    SK_ENTER(c);
    if (state_bytes) *state_bytes = c->live_state_bytes;
    if (bridged_levels) *bridged_levels = c->live_levels;
    if (launches) *launches = c->live_launches;
    return SK_OK;
}

} // extern "C"
