// sk_path.hip -- MotifSeq alignment paths: which samples of a hit belong to which point of the motif, for gfx950.
//
// mlpy.dtw_subsequence hands back the whole warping path (MotifSeq.py:437); the records and hit lists of this build
// keep its two ends.  The path of a hit (dist, start, end) is the back-trace of subsequence_path() in the full N x n
// matrix from (N-1, end): while i > 0 -- at j == 0 up; else diag if it equals min3(up, diag, left), else left if it
// does, else up.  In it every motif point i covers one contiguous column range [a_i, b_i]; those SPANS are what this
// file writes, int32 [N][2] per hit (a_0 = b_0 = start, b_{N-1} = end, a_{i+1} is b_i or b_i + 1).
//
// The kernel never sees the N x n matrix.  It recomputes subsequence DTW on the window y[start .. end] alone (W columns,
// free start on row 0, "up" on the left edge) and back-traces from (N-1, W-1): the traced path lies inside the window,
// its cells see the same sums in the same order, every cell of the window is >= its twin in the full matrix (add and min
// are monotone) and a neighbour that lost a tie-free comparison there loses it here too -- so the path is the same one,
// shifted by `start`, and D_w[N-1][W-1] has the bits of `dist`.  That last fact, a_0 == start and
// b_{N-1} == end are checked per hit; a hit that fails gets spans -1 and is counted (sk_last_path_mismatches()).
//
// One wavefront per hit.  The motif is swept in stripes of 64 rows, lane l owning row 64 s + l; at step t lane l is at
// window column t - l, the sample and the cell above arrive from lane l - 1 by DPP wave_shr:1 as in k_sdtw, and the last
// row of a stripe goes through `brow` (W doubles, overwritten in place: lane 63 stores column t - 63 long after lane 0
// read it) into the next.  The cell arithmetic is the exact pass's: c = |x_i - y_j|, D = c + min, one rounded operation
// each, samples normalised on the fly with the exact pass's expression.  Each cell leaves two direction bits (0 diag,
// 1 left, 2 up), 16 cells of a row to a word a lane assembles in a register; the back-trace then reads a word per 16
// columns of a leftward run and one per row change.
//
// Two tiers.  PATH_LDS_BYTES: the direction words of a hit live in LDS while N * ceil(W / 16) words fit and W <=
// PATH_LDS_COLS; every other hit is appended to a list that a second launch works through with the words (and brow) in
// a slab of device memory per wavefront, sized for W = the longest read.  As many such wavefronts run as fit the byte
// budget SK_PATH_SCRATCH_BYTES (default 1 GiB), at least one: wide windows are slow, not wrong.
#include "sk_sdtw_dev.h"
#include <stdlib.h>

namespace {

// LDS budget of a wavefront: the default window is 200 motif points x 512 columns x 2 bits = 25 600 B of direction
// words, plus the stripe boundary row of PATH_LDS_COLS doubles (8 KiB): 33 792 B, so four wavefronts (one per SIMD)
// share a CU's 160 KiB.  The C4 batch's median window is 200 x 73 (tools/paths_throughput.py reports the distribution).
constexpr int PATH_LDS_BYTES = 2 * 200 * 512 / 8;
constexpr int PATH_LDS_WORDS = PATH_LDS_BYTES / 4;
constexpr int PATH_LDS_COLS  = 1024;

enum { DIR_DIAG = 0, DIR_LEFT = 1, DIR_UP = 2 };

struct path_kargs {
    int            feed;        // sk_feed
    const void    *samples;     // int16 or double samples (filtered)
    const void    *samples_raw; // float64 feeds: the unfiltered input for reads flagged SK_IFLAG_INPLACE (or nullptr)
    int64_t        stride;      // row stride (SK_FEED_I16)
    const int64_t *off;         // ragged offsets (float64 feeds)
    const sk_prep *prep;        // per read (not SK_FEED_F64_RAW)
    const double  *x;           // the motif, N points (device)
    int            N;
    const sk_hit  *hits;        // [nreads][K]
    int            K;
    int            nhits;       // nreads * K
    int32_t       *spans;       // [nreads][K][N][2]
    int32_t       *mism;        // += hits that failed the self-check
    int32_t       *list;        // [0] = count, [2 ..] = hits left to the scratch tier
    int            lds_words;   // LDS tier: direction words a hit may take (0: every hit goes to the list)
    uint32_t      *slab;        // scratch tier: per wavefront slab_words words: brow, then the direction words
    int64_t        slab_words;
    int64_t        max_len;     // the longest read: what a slab is sized for
};

struct path_hit {
    bool valid;
    int  start, W;
};

__device__ __forceinline__ path_hit load_hit(const path_kargs &a, int id, int &n, const sk_prep *&pr)
{
    const sk_hit h = a.hits[id];
    const int r = id / a.K;
    int flags = 0;
    pr = nullptr;
    if (a.feed == SK_FEED_F64_RAW) {
        n = (int)(a.off[r + 1] - a.off[r]);
    } else {
        pr = a.prep + r;
        n = pr->n; flags = pr->flags;
    }
    path_hit p;
    p.valid = !(flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE)) && h.dist == h.dist && h.start >= 0 && h.end >= h.start &&
              h.end < n && (int64_t)n <= a.max_len;
    p.start = h.start;
    p.W = h.end - h.start + 1;
    return p;
}

__device__ __forceinline__ void no_path(const path_kargs &a, int id, int lane)
{
    int32_t *sp = a.spans + (int64_t)id * a.N * 2;
    for (int64_t k = lane; k < (int64_t)a.N * 2; k += 64) sp[k] = -1;
}

// The window DTW and the back-trace of one hit by one wavefront.  dirs: N * ceil(W / 16) words, brow: W doubles (LDS or
// device memory: generic pointers).  Every lane of the wavefront calls it.
__device__ void trace_hit(const path_kargs &a, int id, const path_hit p, const sk_prep *pr, uint32_t *dirs, double *brow)
{
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63;
    const int N = a.N, W = p.W, WW = (W + 15) >> 4;
    const int r = id / a.K;
    const double dist = a.hits[id].dist;

    double center = 0.0, scale = 1.0, rc1 = 0.0, rc2 = 0.0;
    const int16_t *s16 = nullptr;
    const double  *s64 = nullptr;
    if (a.feed == SK_FEED_I16) {
        center = pr->center; scale = pr->scale;
        s16 = (const int16_t *)a.samples + (int64_t)r * a.stride + p.start;
    } else if (a.feed == SK_FEED_F64_NORM) {
        center = pr->center; scale = pr->scale; rc1 = pr->top; rc2 = pr->bot;
        s64 = (const double *)(((pr->flags & SK_IFLAG_INPLACE) && a.samples_raw) ? a.samples_raw : a.samples) + a.off[r] + p.start;
    } else {
        s64 = (const double *)a.samples + a.off[r] + p.start;
    }
    auto fetch = [&](int j) -> double {             // normalised sample of window column j (the exact pass's expression)
        if (j >= W) return INF;
        if (a.feed == SK_FEED_I16) return ((double)s16[j] - center) / scale;
        if (a.feed == SK_FEED_F64_NORM) return ((s64[j] - center) - rc1) / scale - rc2;
        return s64[j];
    };

    const int nstripes = (N + 63) >> 6;
    const int nblk = (W + 63 + 63) >> 6;            // steps 0 .. W + 62 in blocks of 64
    double corner = 0.0;
    for (int s = 0; s < nstripes; s++) {
        const int i = (s << 6) + lane;
        const bool rowlive = i < N;
        const double xi = rowlive ? a.x[i] : 0.0;
        const bool last_stripe = s + 1 == nstripes;
        double D = INF;                             // my cell one column back (column -1: +inf)
        double y = INF;
        double diag = (s == 0 && lane == 0) ? 0.0 : INF;   // the cell above, one column back
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
                const double top = (s == 0) ? 0.0 : B;          // row -1 of the window: free start
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

    // back-trace, the same on every lane; lane 0 stores
    int32_t *sp = a.spans + (int64_t)id * N * 2;
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
    if (lane == 0) { sp[0] = p.start + j; sp[1] = p.start + b; }
    // self-check: the window's corner has the bits of the record's distance and the trace ends on the record's start
    const bool ok = __double_as_longlong(corner) == __double_as_longlong(dist) && j == 0;
    if (!ok) {
        __syncthreads();
        no_path(a, id, lane);
        if (lane == 0) atomicAdd(a.mism, 1);
    }
}

// LDS tier: one wavefront (one block) per hit; what does not fit goes to the list
__global__ __launch_bounds__(64)
void k_path_lds(const path_kargs a)
{
    __shared__ uint32_t dirs[PATH_LDS_WORDS];
    __shared__ double brow[PATH_LDS_COLS];
    const int id = blockIdx.x;
    const int lane = threadIdx.x;
    int n;
    const sk_prep *pr;
    const path_hit p = load_hit(a, id, n, pr);
    if (!p.valid) { no_path(a, id, lane); return; }
    const int64_t words = (int64_t)a.N * ((p.W + 15) >> 4);
    if (words > a.lds_words || p.W > PATH_LDS_COLS) {
        if (lane == 0) a.list[2 + atomicAdd(&a.list[0], 1)] = id;
        return;
    }
    trace_hit(a, id, p, pr, dirs, brow);
}

// scratch tier: gridDim.x wavefronts share the listed hits, each with its own slab
__global__ __launch_bounds__(64)
void k_path_scratch(const path_kargs a)
{
    const int cnt = a.list[0];
    uint32_t *mine = a.slab + (int64_t)blockIdx.x * a.slab_words;
    double *brow = (double *)mine;
    uint32_t *dirs = mine + 2 * a.max_len;
    for (int k = blockIdx.x; k < cnt; k += gridDim.x) {
        const int id = a.list[2 + k];
        int n;
        const sk_prep *pr;
        const path_hit p = load_hit(a, id, n, pr);   // (valid: the LDS tier listed it)
        trace_hit(a, id, p, pr, dirs, brow);
        __syncthreads();
    }
}

} // namespace

int sk_path_begin(sk_ctx *c)
{
    int rc = sk_reserve(c, &c->pathcnt, 16 * sizeof(int32_t));
    if (rc) return rc;
    SK_HIP(hipMemsetAsync(c->pathcnt.p, 0, 16 * sizeof(int32_t), c->stream));
    c->path_valid = true;
    return SK_OK;
}

int sk_launch_paths(sk_ctx *c, const sk_path_args *p)
{
    if (p->nreads <= 0) return SK_OK;
    const int64_t nhits = (int64_t)p->nreads * p->K;
    if (nhits > 0x7fff0000) return sk_fail(SK_ERR_INVALID, "paths: %lld hits in one launch", (long long)nhits);
    const int64_t max_len = p->max_len > 0 ? p->max_len : 1;
    int rc;
    if ((rc = sk_reserve(c, &c->pathlist, (size_t)(nhits + 2) * sizeof(int32_t)))) return rc;
    // slab of a scratch-tier wavefront: brow (max_len doubles), then N * ceil(max_len / 16) direction words
    const int64_t slab_words = (2 * max_len + (int64_t)p->nmotif * ((max_len + 15) / 16) + 1) & ~(int64_t)1;
    size_t budget = (size_t)1 << 30;
    if (const char *e = sk_tune("SK_PATH_SCRATCH_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
    int64_t waves = (int64_t)(budget / ((size_t)slab_words * 4));
    if (waves > 8 * (int64_t)c->num_cu) waves = 8 * (int64_t)c->num_cu;
    if (waves > nhits) waves = nhits;
    if (waves < 1) waves = 1;
    if ((rc = sk_reserve(c, &c->pathscratch, (size_t)waves * (size_t)slab_words * 4))) return rc;

    path_kargs k;
    k.feed = p->feed; k.samples = p->samples; k.samples_raw = p->samples_raw; k.stride = p->stride; k.off = p->off;
    k.prep = p->prep; k.x = p->d_motif; k.N = p->nmotif; k.hits = p->hits; k.K = p->K; k.nhits = (int)nhits;
    k.spans = p->spans; k.mism = (int32_t *)c->pathcnt.p; k.list = (int32_t *)c->pathlist.p;
    k.lds_words = PATH_LDS_WORDS;
    if (const char *e = sk_tune("SK_PATH_LDS_BYTES")) { const long v = atol(e); if (v >= 0 && v / 4 < PATH_LDS_WORDS) k.lds_words = (int)(v / 4); }
    k.slab = (uint32_t *)c->pathscratch.p; k.slab_words = slab_words; k.max_len = max_len;
    SK_HIP(hipMemsetAsync(c->pathlist.p, 0, 2 * sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(k_path_lds, dim3((unsigned)nhits), dim3(64), 0, c->stream, k);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_path_scratch, dim3((unsigned)waves), dim3(64), 0, c->stream, k);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
