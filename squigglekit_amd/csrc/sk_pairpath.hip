// sk_pairpath.hip -- warping paths over a pair list for gfx950: which target points every query point of a pair covers.
//
// sk_pairs.hip says where a query matches its target: (dist, start, end) per pair.  This file says how: the SPANS of the
// pair's warping path, int32 [N][2] per pair, query point i covering the target points [a_i, b_i] (the meaning of
// sk_path.hip, whose kernel this one follows).  The spans of pair p start at row span_off[p] = sum of the query lengths
// of the pairs before it, in list order, of one [sum N][2] array.
//
//   SK_PAIRS_SUBSEQUENCE   mlpy's subsequence_path from (N-1, end): while i > 0 -- at j == 0 up; else diag if it equals
//                          min3(up, diag, left), else left if it does, else up.  a_0 = b_0 = start, b_{N-1} = end.
//   SK_PAIRS_GLOBAL        mlpy's path() from (N-1, M-1): while i > 0 || j > 0 -- at i == 0 left, at j == 0 up, else the
//                          same order.  a_0 = 0, b_{N-1} = M - 1.  mlpy as published, like the record itself (sk_pairs.hip).
//
// The window argument of sk_path.hip carries over.  Subsequence mode recomputes the DTW on target[start .. end] alone
// (free start on row 0, "up" on the left edge); the traced path lies inside that window, so it is the same path shifted by
// `start` and the window's corner has the bits of `dist`.  It holds for any [start, end] that holds the match, hence for
// the merged records of a tiled search traced against the whole target.  Global mode has no window to cut: the "window" is
// the whole target (start == 0, end == M - 1 or the record is a mismatch), row -1 is +inf but for the diagonal of cell
// (0, 0), so row 0 accumulates leftwards and column 0 upwards -- D[0][j] = D[0][j-1] + c, D[i][0] = D[i-1][0] + c, the
// record's own sums -- and the trace runs on along row 0 to column 0.
//
// Self-check per pair: the corner has the bits of the record's dist and the trace ends on the record's start (column 0 of
// the window; trivially cell (0, 0) in global mode, whose check is the corner and the window).  A pair that fails gets
// spans -1 and is counted (sk_last_path_mismatches()); so is a record whose start / end lie outside [0, M) or end < start
// -- checked before any sample is loaded.  A record with NaN dist or SK_FLAG_EMPTY gets spans -1 and is not counted.
//
// One wavefront per pair; the schedule is trace_hit's (stripes of 64 query rows, DPP wave_shr:1 hand-off, `brow` between
// stripes, 16 cells per direction word), the cell arithmetic the exact pass's.  The query (1 .. 1 024 points: 1 .. 16
// stripes) and the target come from the pool, already normalised.  Tiers as in sk_path.hip -- LDS while the direction
// words and the window fit, the rest listed for a second launch with a slab of device memory per wavefront -- but the
// slab is sized from the LISTED pairs (widest window, most direction words: three atomicMax in the first launch, one
// 32-byte read-back between the two), not from the longest target: queries of a few hundred points searched in a
// 100 000-point reference have windows of a few hundred columns.
#include "sk_sdtw_dev.h"
#include <stdlib.h>
#include <vector>

namespace {

// the LDS budget of sk_path.hip: 25 600 B of direction words + 8 KiB of boundary row, four wavefronts to a CU
constexpr int PP_LDS_BYTES = 2 * 200 * 512 / 8;
constexpr int PP_LDS_WORDS = PP_LDS_BYTES / 4;
constexpr int PP_LDS_COLS  = 1024;

enum { DIR_DIAG = 0, DIR_LEFT = 1, DIR_UP = 2 };
// the list header (int32 words): count, widest listed window, longest listed query, -, most direction words (uint64), -, -
enum { PL_COUNT = 0, PL_MAXW = 1, PL_MAXN = 2, PL_WORDS = 4, PL_FIRST = 8 };

struct pp_kargs {
    const double              *values;  // the pool (device); sequence offsets in `tab` are relative to it
    const sk_pairpath_entry   *tab;     // [npairs]
    const sk_hit              *rec;     // [npairs]
    int32_t                   *spans;   // [sum N][2]
    int                        npairs;
    int                        global;
    int32_t                   *mism;    // += pairs that failed the self-check
    int32_t                   *list;    // PL_* header, then the pairs left to the scratch tier
    int                        lds_words;   // LDS tier: direction words a pair may take (0: every pair goes to the list)
    uint32_t                  *slab;    // scratch tier: per wavefront slab_words words: brow (brow_cols doubles), then the words
    int64_t                    slab_words;
    int64_t                    brow_cols;
};

enum { PP_NONE = 0, PP_BAD = 1, PP_OK = 2 };
struct pp_win {
    int what;       // PP_NONE: no path, not counted; PP_BAD: a mismatch; PP_OK: trace it
    int start, W;
};

// what the record asks for, decided from the record and the lengths alone (no sample is touched)
__device__ __forceinline__ pp_win load_pair(const pp_kargs &a, const sk_pairpath_entry &e, const sk_hit &h)
{
    pp_win p;
    p.start = 0;
    p.W = 0;
    if (!(h.dist == h.dist) || (h.flags & SK_FLAG_EMPTY)) p.what = PP_NONE;
    else if (h.start < 0 || h.end < h.start || h.end >= e.M) p.what = PP_BAD;
    else if (a.global && (h.start != 0 || h.end != e.M - 1)) p.what = PP_BAD;
    else { p.what = PP_OK; p.start = h.start; p.W = h.end - h.start + 1; }   // (0 <= start <= end < M: no overflow)
    return p;
}

__device__ __forceinline__ void no_path(const pp_kargs &a, const sk_pairpath_entry &e, int lane)
{
    int32_t *sp = a.spans + e.span_off * 2;
    for (int k = lane; k < e.N * 2; k += 64) sp[k] = -1;
}

// The window DTW and the back-trace of one pair by one wavefront.  dirs: N * ceil(W / 16) words, brow: W doubles (LDS or
// device memory: generic pointers).  Every lane of the wavefront calls it.
__device__ void trace_pair(const pp_kargs &a, const sk_pairpath_entry &e, const pp_win p, const double dist,
                           uint32_t *dirs, double *brow)
{
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63;
    const int N = e.N, W = p.W, WW = (W + 15) >> 4;
    const double *x = a.values + e.qoff;
    const double *y0 = a.values + e.toff + p.start;
    const double row_m1 = a.global ? INF : 0.0;     // row -1 of the window: free start, or pinned
    auto fetch = [&](int j) -> double { return j < W ? y0[j] : INF; };

    const int nstripes = (N + 63) >> 6;
    const int nblk = (W + 63 + 63) >> 6;            // steps 0 .. W + 62 in blocks of 64
    double corner = 0.0;
    for (int s = 0; s < nstripes; s++) {
        const int i = (s << 6) + lane;
        const bool rowlive = i < N;
        const double xi = rowlive ? x[i] : 0.0;
        const bool last_stripe = s + 1 == nstripes;
        double D = INF;                             // my cell one column back (column -1: +inf)
        double y = INF;
        double diag = (s == 0 && lane == 0) ? 0.0 : INF;   // the cell above, one column back: 0 for cell (0, 0) in both modes
        uint32_t word = 0;
        double F = fetch(lane);
        double B = (s > 0 && lane < W) ? brow[lane] : INF; // the stripe above's last row (lane 0 consumes it)
        for (int blk = 0; blk < nblk; blk++) {
            const int nxt = ((blk + 1) << 6) + lane;
            const double Fn = fetch(nxt);
            const double Bn = (s > 0 && nxt < W) ? brow[nxt] : INF;
            for (int q = 0; q < 64; q++) {
                const int t = (blk << 6) + q;
                y = dpp_f64<DPP_WAVE_SHR1>(F, y);               // lane 0 takes sample t
                F = dpp_f64<DPP_WAVE_ROL1>(F, F);
                const double top = (s == 0) ? row_m1 : B;
                B = dpp_f64<DPP_WAVE_ROL1>(B, B);
                const double up = dpp_f64<DPP_WAVE_SHR1>(top, D);
                const double lf = D;
                const double c = fabs(xi - y);
                const bool lt1 = lf < diag;                     // diag wins ties over left
                const double m1 = lt1 ? lf : diag;
                const bool lt2 = up < m1;                       // up only if strictly smaller
                const double m = lt2 ? up : m1;
                const double nd = c + m;
                const uint32_t dir = lt2 ? DIR_UP : (lt1 ? DIR_LEFT : DIR_DIAG);
                diag = up;
                D = nd;
                const int j = t - lane;
                if (j >= 0 && j < W && rowlive) {
                    word |= dir << (2 * (j & 15));
                    if ((j & 15) == 15 || j == W - 1) { dirs[(int64_t)i * WW + (j >> 4)] = word; word = 0; }
                    if (!last_stripe && lane == 63) brow[j] = nd;
                    if (i == N - 1 && j == W - 1) corner = nd;
                }
            }
            F = Fn;  B = Bn;
        }
        __syncthreads();                            // (one wavefront per block) brow / dirs stores before the loads below
    }
    corner = __shfl(corner, (N - 1) & 63);

    // back-trace, the same on every lane; lane 0 stores.  Row 0 of the global mode is all "left" and its column 0 all
    // "up" by the +inf border, so the loop is the same in both modes; the global trace then runs on to column 0.
    int32_t *sp = a.spans + e.span_off * 2;
    int i = N - 1, j = W - 1, b = W - 1;
    int64_t have = -1;
    uint32_t w = 0;
    while (i > 0) {
        int d = DIR_UP;                             // the left edge of the window: up
        if (j > 0) {
            const int64_t wi = (int64_t)i * WW + (j >> 4);
            if (wi != have) { w = dirs[wi]; have = wi; }
            d = (w >> (2 * (j & 15))) & 3;
        }
        if (d == DIR_LEFT) { j--; continue; }
        if (lane == 0) { sp[2 * i] = p.start + j; sp[2 * i + 1] = p.start + b; }
        i--;
        if (d == DIR_DIAG) j--;
        b = j;
    }
    if (a.global) j = 0;
    if (lane == 0) { sp[0] = p.start + j; sp[1] = p.start + b; }
    // self-check: the window's corner has the bits of the record's distance and the trace ends on the record's start
    const bool ok = __double_as_longlong(corner) == __double_as_longlong(dist) && j == 0;
    if (!ok) {
        __syncthreads();
        no_path(a, e, lane);
        if (lane == 0) atomicAdd(a.mism, 1);
    }
}

// LDS tier: one wavefront (one block) per pair; what does not fit goes to the list, with what a slab must hold for it
__global__ __launch_bounds__(64)
void k_pairpath_lds(const pp_kargs a)
{
    __shared__ uint32_t dirs[PP_LDS_WORDS];
    __shared__ double brow[PP_LDS_COLS];
    const int id = blockIdx.x;
    const int lane = threadIdx.x;
    if (id >= a.npairs) return;
    const sk_pairpath_entry e = a.tab[id];
    const sk_hit h = a.rec[id];
    const pp_win p = load_pair(a, e, h);
    if (p.what != PP_OK) {
        no_path(a, e, lane);
        if (p.what == PP_BAD && lane == 0) atomicAdd(a.mism, 1);
        return;
    }
    const int64_t words = (int64_t)e.N * ((p.W + 15) >> 4);
    if (words > a.lds_words || p.W > PP_LDS_COLS) {
        if (lane == 0) {
            a.list[PL_FIRST + atomicAdd(&a.list[PL_COUNT], 1)] = id;
            atomicMax(&a.list[PL_MAXW], p.W);
            atomicMax(&a.list[PL_MAXN], e.N);
            atomicMax((unsigned long long *)(a.list + PL_WORDS), (unsigned long long)words);
        }
        return;
    }
    trace_pair(a, e, p, h.dist, dirs, brow);
}

// scratch tier: gridDim.x wavefronts share the listed pairs, each with its own slab
__global__ __launch_bounds__(64)
void k_pairpath_scratch(const pp_kargs a)
{
    const int cnt = a.list[PL_COUNT];
    uint32_t *mine = a.slab + (int64_t)blockIdx.x * a.slab_words;
    double *brow = (double *)mine;
    uint32_t *dirs = mine + 2 * a.brow_cols;
    for (int k = blockIdx.x; k < cnt; k += gridDim.x) {
        const int id = a.list[PL_FIRST + k];
        const sk_pairpath_entry e = a.tab[id];
        const sk_hit h = a.rec[id];
        const pp_win p = load_pair(a, e, h);        // (PP_OK: the LDS tier listed it)
        const int64_t words = (int64_t)e.N * ((p.W + 15) >> 4);
        if (p.what != PP_OK || p.W > a.brow_cols || 2 * a.brow_cols + words > a.slab_words) continue;   // (never: the slab was sized for it)
        trace_pair(a, e, p, h.dist, dirs, brow);
        __syncthreads();
    }
}

} // namespace

// The spans of a checked pair list (sk_pairs_check passed, npairs > 0): d_values / d_rec / d_spans on the device, off / pairs
// on the host; sequence s is d_values[off[s] - off0 .. off[s + 1] - off0).  have_records == 0: the records are made first
// (sk_pairs_run into d_rec).  Synchronises once between its two launches (the slab's size comes from the first).
int sk_pair_paths_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                      int64_t npairs, int32_t mode, sk_hit *d_rec, int32_t have_records, int32_t *d_spans)
{
    int rc;
    if ((rc = sk_pairs_check(off, nseq, pairs, npairs, mode, d_rec))) return rc;
    if (!d_spans) return sk_fail(SK_ERR_INVALID, "NULL spans");
    if (npairs == 0) return SK_OK;
    if (!d_values) return sk_fail(SK_ERR_INVALID, "NULL values");
    if ((rc = sk_path_begin(c))) return rc;
    if (!have_records) {
        if ((rc = sk_pairs_run(c, d_values, off, off0, nseq, pairs, npairs, mode, d_rec))) return rc;
    } else {
        SK_HIP(hipStreamSynchronize(c->stream));            // an earlier call may still read the old table
        SK_HIP(hipEventRecord(c->ev[0], c->stream));
        SK_HIP(hipEventRecord(c->ev[1], c->stream));
        SK_HIP(hipEventRecord(c->ev[2], c->stream));
        c->last_retry = 0; c->retry_dev = false; c->prof_chunks = 0;
    }
    c->pairpath_table.resize((size_t)npairs);
    int64_t rows = 0;
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query, t = pairs[p].target;
        sk_pairpath_entry e;
        e.qoff = off[q] - off0; e.toff = off[t] - off0; e.span_off = rows;
        e.N = (int32_t)(off[q + 1] - off[q]); e.M = (int32_t)(off[t + 1] - off[t]);
        c->pairpath_table[(size_t)p] = e;
        rows += e.N;
    }
    if ((rc = sk_reserve(c, &c->pairpath, (size_t)npairs * sizeof(sk_pairpath_entry)))) return rc;
    if ((rc = sk_reserve(c, &c->pathlist, (size_t)(npairs + PL_FIRST) * sizeof(int32_t)))) return rc;
    SK_HIP(hipMemcpyAsync(c->pairpath.p, c->pairpath_table.data(), (size_t)npairs * sizeof(sk_pairpath_entry),
                          hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipMemsetAsync(c->pathlist.p, 0, PL_FIRST * sizeof(int32_t), c->stream));

    pp_kargs k;
    k.values = d_values; k.tab = (const sk_pairpath_entry *)c->pairpath.p; k.rec = d_rec; k.spans = d_spans;
    k.npairs = (int)npairs; k.global = mode == SK_PAIRS_GLOBAL; k.mism = (int32_t *)c->pathcnt.p;
    k.list = (int32_t *)c->pathlist.p;
    k.lds_words = PP_LDS_WORDS;
    if (const char *e = sk_tune("SK_PATH_LDS_BYTES")) { const long v = atol(e); if (v >= 0 && v / 4 < PP_LDS_WORDS) k.lds_words = (int)(v / 4); }
    k.slab = nullptr; k.slab_words = 0; k.brow_cols = 0;
    hipLaunchKernelGGL(k_pairpath_lds, dim3((unsigned)npairs), dim3(64), 0, c->stream, k);
    SK_HIP(hipGetLastError());

    // what the listed pairs need: the one read-back of the call
    int32_t head[PL_FIRST];
    SK_HIP(hipMemcpyAsync(head, c->pathlist.p, sizeof head, hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    const int64_t listed = head[PL_COUNT];
    c->pairpath_listed = listed; c->pairpath_slab_bytes = 0; c->pairpath_waves = 0;
    if (listed > 0) {
        unsigned long long words = 0;
        memcpy(&words, head + PL_WORDS, sizeof words);
        const int64_t cols = head[PL_MAXW] > 0 ? head[PL_MAXW] : 1;
        const int64_t slab_words = (2 * cols + (int64_t)words + 1) & ~(int64_t)1;
        size_t budget = (size_t)1 << 30;
        if (const char *e = sk_tune("SK_PATH_SCRATCH_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
        int64_t waves = (int64_t)(budget / ((size_t)slab_words * 4));
        if (waves > 8 * (int64_t)c->num_cu) waves = 8 * (int64_t)c->num_cu;
        if (waves > listed) waves = listed;
        if (waves < 1) waves = 1;
        if ((rc = sk_reserve(c, &c->pathscratch, (size_t)waves * (size_t)slab_words * 4))) return rc;
        k.slab = (uint32_t *)c->pathscratch.p; k.slab_words = slab_words; k.brow_cols = cols;
        c->pairpath_slab_bytes = slab_words * 4; c->pairpath_waves = waves;
        hipLaunchKernelGGL(k_pairpath_scratch, dim3((unsigned)waves), dim3(64), 0, c->stream, k);
        SK_HIP(hipGetLastError());
    }
    SK_HIP(hipEventRecord(c->ev[3], c->stream));            // (the main interval now ends behind the paths)
    c->ev_valid = true;
    return SK_OK;
}
