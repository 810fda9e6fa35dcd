// sk_events.hip -- MotifSeq events: what the signal did in the samples of each motif point of a hit, and the model the
// hits of a run show when pooled, for gfx950.
//
// sk_path.hip says which samples [a_i, b_i] of a hit belong to motif point i.  k_events turns each span into one
// sk_event -- with y the read's filtered, normalised samples (the exact pass's expression, as trace_hit's fetch) and
// w = y[a_i : b_i + 1]: sum = np.sum(w), std = np.std(w), cost = np.sum(np.abs(x[i] - w)), start = a_i, dwell =
// b_i - a_i + 1 -- the row an eventalign / resquiggle table has per base.  k_pool reduces the events of many hits, column
// by column, to one sk_pool_rec per motif point: the level the reads really show there (sample weighted: one step of DTW
// barycentre averaging), its spread, the noise inside an event, the dwell.  Every double is bit for bit numpy's.
//
// numpy's order (np.add.reduce over a contiguous float64 array, as sk_bg_rec documents it): fewer than 8 terms -- a
// serial loop; up to 128 -- eight accumulators over the blocks of 8, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
// (r6 + r7)), then the remainder serially; above -- halves split at a multiple of 8, recursively; above 8 192 -- one such
// tree per buffer of 8 192, the buffers added serially.  np.std is two passes: sqrt(sum((w - sum / n)^2) / n).
//
// k_events: one wavefront per hit, a lane per motif point (64 points at a time).  The hit windows of the C4 batch have a
// median of 73 columns for 200 points (tools/paths_throughput.py): nearly every span is one or two samples and the work
// of a point is a handful of loads, so a lane per point keeps all 64 lanes busy and the records of a hit leave as
// consecutive 32-byte stores.  A span of up to 128 samples is one leaf of numpy's tree and stays with its lane (three
// looks at the samples: sum, squares, cost).  A longer span -- a stalled point can take the whole window -- would hold 63
// lanes idle behind one, so the lanes that met one vote and the wavefront takes those points one after the other with
// the routine the read background uses on a last row (wave_np_sum, sk_prepw_dev.h: a leaf per lane, the tree in LDS).
//
// k_pool: the selected hits are first listed in hit order by one workgroup (k_pool_select: ballot + prefix, a hit with
// dwell == 0 or use[h] == 0 is left out), then one wavefront per motif point walks that list with wave_np_sum, seven looks
// at its column.  A column is read with a stride of N records; nothing is staged: the list of hits may be millions long.
#include "sk_common.h"
#include "sk_prepw_dev.h"

namespace {

struct ev_kargs {
    int            feed;        // sk_feed
    const void    *samples;     // int16 or double samples (filtered)
    const void    *samples_raw; // float64 feeds: the unfiltered input for reads flagged SK_IFLAG_INPLACE (or nullptr)
    int64_t        stride;      // row stride (SK_FEED_I16)
    const int64_t *off;         // ragged offsets (float64 feeds)
    const sk_prep *prep;        // per read (not SK_FEED_F64_RAW)
    const double  *x;           // the motif, N points (device)
    int            N;
    int            K;
    const int32_t *spans;       // [nreads][K][N][2], as sk_path.hip left them
    sk_event      *events;      // [nreads][K][N]
};

__device__ __forceinline__ sk_event no_event()
{
    sk_event e;
    e.sum = e.std = e.cost = __builtin_nan("");
    e.start = -1; e.dwell = 0;
    return e;
}

// np.add.reduce over term(0) .. term(len - 1), len <= 128 (one leaf of numpy's tree), by one lane
template <typename Term>
__device__ __forceinline__ double lane_np_leaf(int len, Term term)
{
    double res = 0.0;
    if (len < 8) {
        for (int i = 0; i < len; i++) res += term(i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = term(j);
    const int full = len - (len % 8);
    for (int i = 8; i < full; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] += term(i + j);
    }
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = full; i < len; i++) res += term(i);
    return res;
}

__global__ __launch_bounds__(64)
void k_events(const ev_kargs a)
{
    __shared__ double nodes[256];
    const int lane = threadIdx.x;
    const int id = blockIdx.x;
    const int N = a.N;
    const int r = id / a.K;
    const int32_t *sp = a.spans + (int64_t)id * N * 2;
    sk_event *ev = a.events + (int64_t)id * N;

    int n = 0;
    double center = 0.0, scale = 1.0, rc1 = 0.0, rc2 = 0.0;
    const int16_t *s16 = nullptr;
    const double  *s64 = nullptr;
    if (a.feed == SK_FEED_I16) {
        const sk_prep *pr = a.prep + r;
        n = pr->n; center = pr->center; scale = pr->scale;
        s16 = (const int16_t *)a.samples + (int64_t)r * a.stride;
    } else if (a.feed == SK_FEED_F64_NORM) {
        const sk_prep *pr = a.prep + r;
        n = pr->n; center = pr->center; scale = pr->scale; rc1 = pr->top; rc2 = pr->bot;
        s64 = (const double *)(((pr->flags & SK_IFLAG_INPLACE) && a.samples_raw) ? a.samples_raw : a.samples) + a.off[r];
    } else {
        n = (int)(a.off[r + 1] - a.off[r]);
        s64 = (const double *)a.samples + a.off[r];
    }
    auto fetch = [&](int j) -> double {             // normalised sample j of the read (the exact pass's expression)
        if (a.feed == SK_FEED_I16) return ((double)s16[j] - center) / scale;
        if (a.feed == SK_FEED_F64_NORM) return ((s64[j] - center) - rc1) / scale - rc2;
        return s64[j];
    };

    const bool path = sp[0] >= 0;                   // (wave-uniform: a hit without a path has every span -1)
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const bool live = i < N;
        int lo = -1, d = 0;
        double xi = 0.0;
        if (live && path) {
            const int2 ab = *(const int2 *)(sp + 2 * i);
            if (ab.x >= 0 && ab.y >= ab.x && ab.y < n) { lo = ab.x; d = ab.y - ab.x + 1; }   // (never past the read)
            xi = a.x[i];
        }
        if (live && d <= 128) {
            sk_event e = no_event();
            if (d > 0) {
                const double sum = lane_np_leaf(d, [&](int j) { return fetch(lo + j); });
                const double mean = sum / (double)d;
                const double ssq = lane_np_leaf(d, [&](int j) { const double q = fetch(lo + j) - mean; return q * q; });
                e.sum = sum;
                e.std = sqrt(ssq / (double)d);
                e.cost = lane_np_leaf(d, [&](int j) { return fabs(xi - fetch(lo + j)); });
                e.start = lo; e.dwell = d;
            }
            ev[i] = e;
        }
        unsigned long long wide = __ballot(live && d > 128);
        while (wide) {                              // (wave-uniform) the long spans of these 64 points, one at a time
            const int src = (int)__builtin_ctzll(wide);
            wide &= wide - 1;
            const int wlo = bcast_from(lo, src), wd = bcast_from(d, src);
            const double wx = __shfl(xi, src);
            const double sum = wave_np_sum<true>(wd, nodes, lane, [&](int j) { return fetch(wlo + j); });
            const double mean = sum / (double)wd;
            const double ssq = wave_np_sum<true>(wd, nodes, lane, [&](int j) {
                const double q = fetch(wlo + j) - mean; return q * q; });
            const double cost = wave_np_sum<true>(wd, nodes, lane, [&](int j) { return fabs(wx - fetch(wlo + j)); });
            if (lane == 0) {
                sk_event e;
                e.sum = sum; e.std = sqrt(ssq / (double)wd); e.cost = cost; e.start = wlo; e.dwell = wd;
                ev[i0 + src] = e;
            }
        }
    }
}

// ---- pooling ----------------------------------------------------------------------------------------------------------
constexpr int POOL_SELECT_THREADS = 1024;

// idx[0 .. *cnt) = the hits h with use[h] != 0 (or no mask) and a path (dwell > 0 in their first record), ascending
__global__ __launch_bounds__(POOL_SELECT_THREADS)
void k_pool_select(const sk_event *__restrict__ ev, const uint8_t *__restrict__ use, int64_t H, int N,
                   int32_t *__restrict__ idx, int32_t *__restrict__ cnt)
{
    __shared__ int wsum[POOL_SELECT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;                                   // selected so far (the same in every thread)
    for (int64_t h0 = 0; h0 < H; h0 += POOL_SELECT_THREADS) {
        const int64_t h = h0 + tid;
        const bool sel = h < H && (!use || use[h]) && ev[h * N].dwell > 0;
        const unsigned long long b = __ballot(sel);
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int pre = 0, total = 0;
#pragma unroll
        for (int k = 0; k < POOL_SELECT_THREADS / 64; k++) { const int v = wsum[k]; pre += k < w ? v : 0; total += v; }
        if (sel) idx[base + pre + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)h;
        base += total;
        __syncthreads();                            // wsum is read before the next round overwrites it
    }
    if (tid == 0) *cnt = base;
}

// one wavefront per motif point i: the column i of the listed hits -> out[i]
__global__ __launch_bounds__(64)
void k_pool(const sk_event *__restrict__ ev, const int32_t *__restrict__ idx, const int32_t *__restrict__ cnt, int N,
            sk_pool_rec *__restrict__ out)
{
    __shared__ double nodes[256];
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int64_t H = *cnt;
    sk_pool_rec p;
    p.hits = (int32_t)H; p.pad = 0;
    if (H == 0) {
        p.level = p.level_sd = p.sd_mean = p.dwell_mean = p.dwell_sd = p.cost_mean = __builtin_nan("");
        if (lane == 0) out[i] = p;
        return;
    }
    auto at = [&](int64_t k) -> const sk_event & { return ev[(int64_t)idx[k] * N + i]; };
    long long total = 0;                            // exact
    for (int64_t k = lane; k < H; k += 64) total += at(k).dwell;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) total += __shfl_xor(total, o);
    const double cntd = (double)H;
    p.level = wave_np_sum<true>(H, nodes, lane, [&](int64_t k) { return at(k).sum; }) / (double)total;
    const double mmean = wave_np_sum<true>(H, nodes, lane, [&](int64_t k) {
        const sk_event &e = at(k); return e.sum / (double)e.dwell; }) / cntd;
    p.level_sd = sqrt(wave_np_sum<true>(H, nodes, lane, [&](int64_t k) {
        const sk_event &e = at(k); const double q = e.sum / (double)e.dwell - mmean; return q * q; }) / cntd);
    p.sd_mean = wave_np_sum<true>(H, nodes, lane, [&](int64_t k) { return at(k).std; }) / cntd;
    // np.std of the dwells as float64: their sum is exact in float64, so its mean is total / hits
    p.dwell_mean = (double)total / cntd;
    const double dmean = p.dwell_mean;
    p.dwell_sd = sqrt(wave_np_sum<true>(H, nodes, lane, [&](int64_t k) {
        const double q = (double)at(k).dwell - dmean; return q * q; }) / cntd);
    p.cost_mean = wave_np_sum<true>(H, nodes, lane, [&](int64_t k) { return at(k).cost; }) / cntd;
    if (lane == 0) out[i] = p;
}

} // namespace

static_assert(sizeof(sk_event) == 32, "sk_event is 32 bytes (include/squigglekit_hip.h)");
static_assert(sizeof(sk_pool_rec) == 56, "sk_pool_rec is 56 bytes (include/squigglekit_hip.h)");

int sk_launch_events(sk_ctx *c, const sk_path_args *p, sk_event *events)
{
    if (p->nreads <= 0) return SK_OK;
    const int64_t nhits = (int64_t)p->nreads * p->K;
    if (nhits > 0x7fff0000) return sk_fail(SK_ERR_INVALID, "events: %lld hits in one launch", (long long)nhits);
    ev_kargs k;
    k.feed = p->feed; k.samples = p->samples; k.samples_raw = p->samples_raw; k.stride = p->stride; k.off = p->off;
    k.prep = p->prep; k.x = p->d_motif; k.N = p->nmotif; k.K = p->K; k.spans = p->spans; k.events = events;
    hipLaunchKernelGGL(k_events, dim3((unsigned)nhits), dim3(64), 0, c->stream, k);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// d_ev [nhits][N], d_use [nhits] or nullptr, d_idx nhits ints, d_cnt one int, d_out [N] -- all on the device
int sk_launch_events_pool(sk_ctx *c, const sk_event *d_ev, const uint8_t *d_use, int64_t nhits, int32_t N,
                          int32_t *d_idx, int32_t *d_cnt, sk_pool_rec *d_out)
{
    hipLaunchKernelGGL(k_pool_select, dim3(1), dim3(POOL_SELECT_THREADS), 0, c->stream, d_ev, d_use, nhits, (int)N, d_idx,
                       d_cnt);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pool, dim3((unsigned)N), dim3(64), 0, c->stream, d_ev, (const int32_t *)d_idx,
                       (const int32_t *)d_cnt, (int)N, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
