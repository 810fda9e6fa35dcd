// sk_seglev.hip -- segment levels: per-segment and per-read signal statistics and raw coordinates, for gfx950.
//
// get_segs returns index pairs into the filtered signal (segmenter.py:399-470) and nothing about what the segment is or
// where it lies in the raw read.  The segmenter routes leave, per read, the {in band, kept} entries of sk_segstat.hip --
// 64 raw samples per 16-byte entry -- and the walk's [start, end] pairs.  With y the read after scale_outliers
// (segmenter.py:311-318), kept[i] the raw index of y[i] and w = y[s:e], two launches turn every pair, and the whole
// read [0, n), into one sk_seg_level: np.mean(w), np.std(w), np.median(w), np.median(np.abs(w - median)), min, max --
// bit for bit numpy's on w in its own dtype -- and raw_start = kept[s], raw_end = kept[e - 1] + 1, n = e - s.
//
// k_seglev_map: one wavefront per read.  A first look at the kept words counts the survivors; the slots that hold no
// span (e <= s, unused, a read with no survivor) get their final record -- six NaNs, -1, -1, 0 -- and every other slot
// its n and a place in the work list (ballot + prefix count, one atomic per 64 slots; the whole-read item first).  A
// second look, 64 entries a round with a popcount prefix scan over the wavefront, finds the entry and the bit that hold
// the s-th and the (e - 1)-th survivor of each span and writes raw_start / raw_end.
//
// k_seglev_stats: a persistent grid, one wavefront per work item.  It streams raw[raw_start:raw_end] through the kept
// words, 64 raw samples a step, and squeezes the survivors together as float64 -- in LDS for spans of up to
// SEGLEV_LDS_COLS samples, in a scratch row of its own in global memory above (the whole-read item of the 36 978-sample
// example read; such a row stays in L2).  An int16 sample is exact in float64, and numpy's results on an int64 array are
// those on its float64 image: np.mean adds in float64 (every partial sum is an exact integer), np.std subtracts the
// float64 mean first, np.median averages the two middle values in float64.  So one body serves both input kinds, and it
// is the read background's (sk_bg.hip) with the lanes of the wavefront on numpy's pairwise leaves:
//   mean, std   wave_np_sum (sk_prepw_dev.h): np.add.reduce's order, a leaf per lane, the tree in LDS; two passes.
//   median, MAD wave_select2 (sk_select_dev.h): radix select with a 256-bin LDS histogram -- for int16 input that is
//               a counting histogram of the values between lim_low and lim_hi in two digits.  The samples may have
//               either sign (a negative lim_low), so the median's keys are the order-preserving image of the float64
//               bits (key_of_double); |w - median| is never negative.
//   min, max    one look, a wavefront reduction.
#include "sk_common.h"
#include "sk_prepw_dev.h"
#include "sk_select_dev.h"

namespace {

constexpr int SEGLEV_LDS_COLS = 4096;                    // 32 KB of staged samples: four items in flight per CU

struct seglev_kargs {
    int            feed;        // SK_FEED_I16 or SK_FEED_F64_NORM
    const void    *samples;     // int16 rows of `stride`, or float64 with read r at off[r]
    int64_t        stride;
    const int64_t *off;
    const uint4   *mask2;       // [nreads][row16] {in band lo, hi, kept lo, hi}
    int            row16;
    const int32_t *len;         // raw samples per read (clamped to mmax)
    int64_t        mmax;
    int            nreads;
    const int32_t *segs;        // [nreads][max_segs][2]
    const int32_t *nsegs;
    int            max_segs;
    int32_t       *count;       // work items
    int2          *work;        // (read, slot); slot -1: the whole read
    double        *scratch;     // rows of scratch_stride doubles, one per workgroup of k_seglev_stats (long items)
    int64_t        scratch_stride;
    sk_seg_level  *levels;
    sk_seg_level  *read_level;
};

__device__ __forceinline__ sk_seg_level no_level()
{
    sk_seg_level v;
    v.mean = v.std = v.median = v.mad = v.min = v.max = __builtin_nan("");
    v.raw_start = v.raw_end = -1; v.n = 0; v.pad = 0;
    return v;
}

__device__ __forceinline__ int read_len(const seglev_kargs &a, int r)
{
    const int64_t cap = a.mmax < (int64_t)a.row16 * 64 ? a.mmax : (int64_t)a.row16 * 64;
    const int l = a.len[r];
    return l < 0 ? 0 : ((int64_t)l < cap ? l : (int)cap);
}

// the kept word of entry e of a read of M raw samples (bits at and above M cleared)
__device__ __forceinline__ u64 kept_word(const uint4 *mrow, int e, int M)
{
    const uint4 q = mrow[e];
    u64 kp = ((u64)q.w << 32) | q.z;
    const int left = M - e * 64;
    if (left < 64) kp &= (1ull << left) - 1ull;
    return kp;
}

// position of the t-th set bit of w (t < popcount(w))
__device__ __forceinline__ int nth_set_bit(u64 w, int t)
{
    for (int i = 0; i < t; i++) w &= w - 1ull;
    return (int)__builtin_ctzll(w);
}

// the span of slot k of a read with `total` survivors: s < e, or s = e = 0 when the slot holds none
__device__ __forceinline__ void slot_span(const int32_t *sg, int k, int ns, int total, int &s, int &e)
{
    s = e = 0;
    if (k >= ns) return;
    const int a = sg[2 * k], b = sg[2 * k + 1] < total ? sg[2 * k + 1] : total;
    if (a >= 0 && a < b) { s = a; e = b; }
}

__global__ __launch_bounds__(64)
void k_seglev_map(const seglev_kargs a)
{
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    if (r >= a.nreads) return;
    const int M = read_len(a, r);
    const int nent = (M + 63) >> 6;
    const uint4 *mrow = a.mask2 + (int64_t)r * a.row16;
    const int32_t *sg = a.segs + (int64_t)r * 2 * a.max_segs;
    sk_seg_level *lv = a.levels + (int64_t)r * a.max_segs;
    int ns = a.nsegs[r];
    ns = ns < 0 ? 0 : (ns < a.max_segs ? ns : a.max_segs);

    int total = 0;
    for (int e = lane; e < nent; e += 64) total += __popcll(kept_word(mrow, e, M));
    total = bcast_from(wave_incl_scan(total), 63);

    // the records without a span, the n of the others, the work list (slot -1 first)
    for (int k0 = -1; k0 < a.max_segs; k0 += 64) {
        const int k = k0 + lane;
        int s = 0, e = 0;
        if (k < 0) e = total;
        else if (k < a.max_segs) slot_span(sg, k, ns, total, s, e);
        const bool live = k < a.max_segs, item = live && e > s;
        sk_seg_level *rec = k < 0 ? a.read_level + r : lv + k;
        if (live && !item) *rec = no_level();
        if (item) { rec->raw_start = rec->raw_end = -1; rec->n = e - s; rec->pad = 0; }
        const u64 b = __ballot(item);
        if (b) {                                             // (wave-uniform)
            int base = 0;
            if (lane == 0) base = atomicAdd(a.count, __popcll(b));
            base = bcast_from(base, 0);
            if (item) a.work[base + __popcll(b & ((1ull << lane) - 1ull))] = make_int2(r, k);
        }
    }
    if (total == 0) return;
    __syncthreads();                                         // (the -1 marks land before an end found by another lane)

    // raw_start / raw_end: the entry and the bit of the s-th and the (e - 1)-th survivor
    int run = 0;
    for (int e0 = 0; e0 < nent; e0 += 64) {
        const int ent = e0 + lane;
        const u64 kp = ent < nent ? kept_word(mrow, ent, M) : 0ull;
        const int cnt = __popcll(kp);
        const int inc = wave_incl_scan(cnt);
        const int mine = run + inc - cnt;                    // survivors before my entry
        const int next = run + bcast_from(inc, 63);
        for (int k = -1; k < ns; k++) {                      // (wave-uniform)
            int s = 0, e = total;
            if (k >= 0) slot_span(sg, k, ns, total, s, e);
            if (e <= s || e - 1 < run || s >= next) continue;
            sk_seg_level *rec = k < 0 ? a.read_level + r : lv + k;
            if (s >= mine && s < mine + cnt) rec->raw_start = ent * 64 + nth_set_bit(kp, s - mine);
            if (e - 1 >= mine && e - 1 < mine + cnt) rec->raw_end = ent * 64 + nth_set_bit(kp, e - 1 - mine) + 1;
        }
        run = next;
    }
}

__device__ __forceinline__ double wave_min_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double q = __shfl_xor(v, o); v = q < v ? q : v; }
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double q = __shfl_xor(v, o); v = q > v ? q : v; }
    return v;
}

__global__ __launch_bounds__(64)
void k_seglev_stats(const seglev_kargs a)
{
    __shared__ double nodes[256];
    __shared__ __attribute__((aligned(16))) unsigned hist[256];
    __shared__ double lrow[SEGLEV_LDS_COLS];
    const int lane = threadIdx.x;
    const int items = *a.count;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int2 rk = a.work[it];
        const int r = rk.x;
        sk_seg_level *rec = rk.y < 0 ? a.read_level + r : a.levels + (int64_t)r * a.max_segs + rk.y;
        const int rs = rec->raw_start, re = rec->raw_end;
        const int M = read_len(a, r);
        if (rs < 0 || re <= rs || re > M) {                  // (never: k_seglev_map found both ends)
            if (lane == 0) *rec = no_level();
            continue;
        }
        const uint4 *mrow = a.mask2 + (int64_t)r * a.row16;
        const int16_t *s16 = a.feed == SK_FEED_I16 ? (const int16_t *)a.samples + (int64_t)r * a.stride : nullptr;
        const double *s64 = a.feed == SK_FEED_I16 ? nullptr : (const double *)a.samples + a.off[r];
        const bool staged = rec->n <= SEGLEV_LDS_COLS;
        if (!staged && (!a.scratch || (int64_t)rec->n > a.scratch_stride)) {      // (never: the rows hold mmax samples)
            if (lane == 0) *rec = no_level();
            continue;
        }
        double *w = staged ? lrow : a.scratch + (int64_t)blockIdx.x * a.scratch_stride;

        // the survivors of raw[rs:re], squeezed together
        int n = 0;
        for (int ent = rs >> 6; ent <= (re - 1) >> 6; ent++) {
            u64 kp = kept_word(mrow, ent, M);
            if (ent == rs >> 6) kp &= ~0ull << (rs & 63);
            if (ent == (re - 1) >> 6 && (re & 63)) kp &= (1ull << (re & 63)) - 1ull;
            const int idx = ent * 64 + lane;
            if ((kp >> lane) & 1ull) {
                const int at = n + __popcll(kp & ((1ull << lane) - 1ull));
                if (at < rec->n) w[at] = s16 ? (double)s16[idx] : s64[idx];
            }
            n += __popcll(kp);
        }
        if (n > rec->n) n = rec->n;                          // (never: the span has rec->n survivors)
        __syncthreads();

        const double mean = wave_np_sum<true>(n, nodes, lane, [&](int j) { return w[j]; }) / (double)n;
        const double ssq = wave_np_sum(n, nodes, lane, [&](int j) { const double q = w[j] - mean; return q * q; });
        const double sd = sqrt(ssq / (double)n);
        double mn = w[0], mx = w[0];
        for (int j = lane; j < n; j += 64) { const double v = w[j]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
        mn = wave_min_f64(mn); mx = wave_max_f64(mx);

        const int k1 = (n - 1) / 2, k2 = n / 2;
        u64 ka, kb;
        wave_select2<true>(n, k1, k2, hist, lane, [&](int j) { return key_of_double(w[j]); }, ka, kb);
        const double ma = double_of_key(ka), mb = double_of_key(kb);
        const double med = k1 != k2 ? (ma + mb) / 2.0 : ma;
        wave_select2(n, k1, k2, hist, lane, [&](int j) { return (u64)__double_as_longlong(fabs(w[j] - med)); }, ka, kb);
        const double mad = median_of(ka, kb, k1 != k2);
        if (lane == 0) {
            rec->mean = mean; rec->std = sd; rec->median = med; rec->mad = mad; rec->min = mn; rec->max = mx;
        }
        __syncthreads();                                     // the staged samples are read before the next item's arrive
    }
}

int seglev_grid(sk_ctx *c, int32_t nreads, int32_t max_segs, int64_t mmax, int64_t *scratch_stride)
{
    int64_t grid = (int64_t)(c->num_cu > 0 ? c->num_cu : 64) * 16;
    const int64_t slots = (int64_t)nreads * ((int64_t)max_segs + 1);
    if (grid > slots) grid = slots;
    *scratch_stride = 0;
    if (mmax > SEGLEV_LDS_COLS) {                            // long items: a scratch row per workgroup, 1 GB in all
        *scratch_stride = (mmax + 7) & ~(int64_t)7;
        const int64_t fit = ((int64_t)1 << 30) / (*scratch_stride * (int64_t)sizeof(double));
        if (grid > fit) grid = fit;
    }
    return (int)(grid < 1 ? 1 : grid);
}

} // namespace

static_assert(sizeof(sk_seg_level) == 64, "sk_seg_level is 64 bytes (include/squigglekit_hip.h)");

// [0] the item counter (16 bytes), the work list, the scratch rows
size_t sk_seglev_work_bytes(sk_ctx *c, int32_t nreads, int32_t max_segs, int64_t mmax)
{
    int64_t ss;
    const int grid = seglev_grid(c, nreads, max_segs, mmax, &ss);
    return 16 + (size_t)nreads * ((size_t)max_segs + 1) * sizeof(int2) + (size_t)grid * (size_t)ss * sizeof(double);
}

int sk_launch_seg_levels(sk_ctx *c, int feed, const void *samples, int64_t stride, const int64_t *d_off,
                         const void *d_mask2, int row16, const int32_t *d_len, int64_t mmax, int32_t nreads,
                         const int32_t *d_segs, const int32_t *d_nsegs, int32_t max_segs, void *d_work,
                         sk_seg_level *levels, sk_seg_level *read_level)
{
    if (nreads <= 0) return SK_OK;
    if ((int64_t)nreads * ((int64_t)max_segs + 1) > 0x7fff0000)
        return sk_fail(SK_ERR_INVALID, "levels: %d reads x %d slots in one launch", nreads, max_segs);
    seglev_kargs a;
    int64_t ss;
    const int grid = seglev_grid(c, nreads, max_segs, mmax, &ss);
    a.feed = feed; a.samples = samples; a.stride = stride; a.off = d_off; a.mask2 = (const uint4 *)d_mask2; a.row16 = row16;
    a.len = d_len; a.mmax = mmax; a.nreads = nreads; a.segs = d_segs; a.nsegs = d_nsegs; a.max_segs = max_segs;
    a.count = (int32_t *)d_work;
    a.work = (int2 *)((char *)d_work + 16);
    a.scratch = ss ? (double *)((char *)d_work + 16 + (size_t)nreads * ((size_t)max_segs + 1) * sizeof(int2)) : nullptr;
    a.scratch_stride = ss;
    a.levels = levels; a.read_level = read_level;
    SK_HIP(hipMemsetAsync(a.count, 0, 16, c->stream));
    hipLaunchKernelGGL(k_seglev_map, dim3((unsigned)nreads), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_seglev_stats, dim3((unsigned)grid), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
