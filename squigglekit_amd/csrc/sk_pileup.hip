// sk_pileup.hip -- reference pile-up for gfx950: the event alignment table turned round.
//
// sk_pairpath.hip / sk_band.hip say which target points every query point (event) of a pair covers: spans [rows][2], keyed
// by event.  This file inverts that table: for every point of every target the rows that cover it, in ascending row order
// (the reading order of the table), and one sk_pile_rec of statistics per point, every double in numpy's order of
// summation (wave_np_sum, sk_prepw_dev.h) and bit for bit.  The contract is the header's "Reference pile-up";
// tests/pileup_ref.py states it in numpy.
//
//   k_pile_count    one lane per row (and per pair): the checks -- span_off, target, span order, span range; the lowest
//                   offending pair by atomicMin, so the verdict does not depend on the launch order -- and, for the rows
//                   that pass, +1 on an int64 counter per covered point.  A span is nearly always 1 .. 3 points and the
//                   lane walks it; rows of more than 64 points are voted on and taken by the whole wavefront, one
//                   after the other.  Writes scratch only: the row's pair (-1: not an entry) and the counters.
//   (scan)          sk_launch_scan_i64 (sk_pull.hip): the counters -> ent_off [Mtot + 1], in place.
//   k_pile_plan     one lane per point: the longest list, the lists beyond the LDS tier and their chunks.
//   -- the one read-back of the call: verdict, entries, plan.  Nothing has touched the caller's arrays so far. --
//   k_pile_fill     one lane per row again: a slot from a uint32 cursor per point.  The order inside a list is arbitrary.
//   k_pile_sort     one wavefront per point puts a list of up to `tier` entries (4 096 = 16 KiB of LDS; fewer under
//                   SK_PILE_LDS_ENTRIES) in ascending row order: bitonic network in LDS, padded to a power of two.
//                   Longer lists take the merge tier: the wavefront lists the list's chunks of `tier` entries instead.
//   k_pile_sort_chunks / k_pile_merge   the merge tier: every listed chunk sorted in LDS, then passes that merge runs of
//                   W = tier, 2 tier, 4 tier .. entries pairwise through device memory, between the entry array and a
//                   second copy of it: an entry's place is its index in its own run plus its rank in the sibling run
//                   (binary search; rows are unique inside a list, so there are no ties).  Every long list takes the
//                   passes the longest one needs (a finished list is copied), plus a copying pass when that number is odd.
//   k_pile_reduce   one wavefront per point: one look for min / max / first NaN / the exact int64 dwell sum / depth
//                   (changes of pair along the list) / shared, then wave_np_sum twice per np.std.
//
// Integer atomics only (counts and cursors, order-independent); no double is formed by an atomic.
#include "sk_prepw_dev.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

constexpr int     PILE_LDS_ENTRIES = 4096;
constexpr int     PILE_THREADS = 256;
constexpr int64_t PILE_MAX_FLAT = (int64_t)1 << 40;
constexpr unsigned PILE_MAX_GRID = 1u << 24;

// the call's counters (uint64 words)
enum { PS_ERR_OFF = 0, PS_ERR_ROW = 1, PS_LONGEST = 2, PS_NLONG = 3, PS_NCHUNKS = 4, PS_CHUNK_CUR = 5, PS_WORDS = 8 };
// what is wrong, in the low two bits of an error word under the pair index
enum { PO_FIRST = 0, PO_ORDER = 1, PO_END = 2 };            // PS_ERR_OFF
enum { PR_TARGET = 0, PR_ORDER = 1, PR_RANGE = 2 };         // PS_ERR_ROW

struct pile_kargs {
    const int64_t *span_off;        // [npairs + 1]
    const int32_t *spans;           // [nrows][2]
    const double  *value;           // [nrows]
    const int32_t *dwell;           // [nrows] or nullptr (ones)
    const int32_t *target, *shift;  // [npairs] or nullptr (zeros)
    const uint8_t *use;             // [npairs] or nullptr (ones)
    int32_t        npairs, ntargets;
    int64_t        nrows, mtot;
    const int64_t *toff;            // [ntargets + 1]
    unsigned long long *stat;       // PS_*
    int64_t       *off;             // [mtot + 1]: counts, then their exclusive scan
    uint32_t      *cur;             // [mtot]
    int32_t       *rowpair;         // [nrows]: the row's pair, -1 when it is no entry
    int32_t       *ent;             // [entries]
    int64_t       *chunks;          // [chunks][2]: {point, chunk of its list}
    int32_t        tier;
    sk_pile_rec   *out;
};

// the largest p in [0, P) with span_off[p] <= e (P >= 1); stays inside the array whatever it holds
__device__ __forceinline__ int pair_of_row(const int64_t *__restrict__ so, int P, int64_t e)
{
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
        if (so[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// f(point, row) for every point of this lane's row [base, base + len) (len == 0: none): the lane walks a span of up to 64
// points itself, longer ones are taken by the whole wavefront one after the other.  Every lane of the wavefront calls it.
template <typename F>
__device__ __forceinline__ void for_each_point(int64_t base, int64_t len, int32_t row, int lane, F f)
{
    if (len <= 64)
        for (int64_t k = 0; k < len; k++) f(base + k, row);
    unsigned long long m = __ballot(len > 64);
    while (m) {
        const int src = (int)__builtin_ctzll(m);
        m &= m - 1;
        const int64_t b = __shfl(base, src), n = __shfl(len, src);
        const int32_t e = __shfl(row, src);
        for (int64_t k = lane; k < n; k += 64) f(b + k, e);
    }
}

__global__ __launch_bounds__(PILE_THREADS)
void k_pile_count(const pile_kargs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * PILE_THREADS + threadIdx.x;
    const int T = a.ntargets;
    if (i < a.npairs) {
        const unsigned long long key = (unsigned long long)i << 2;
        const int64_t s0 = a.span_off[i], s1 = a.span_off[i + 1];
        if (i == 0 && s0 != 0) atomicMin(&a.stat[PS_ERR_OFF], key | PO_FIRST);
        if (s1 < s0) atomicMin(&a.stat[PS_ERR_OFF], key | PO_ORDER);
        if (i == a.npairs - 1 && s1 != a.nrows) atomicMin(&a.stat[PS_ERR_OFF], key | PO_END);
        if ((a.target ? a.target[i] : 0) >= T) atomicMin(&a.stat[PS_ERR_ROW], key | PR_TARGET);
    }
    int64_t base = 0, len = 0;
    if (i < a.nrows) {
        const int p = pair_of_row(a.span_off, a.npairs, i);
        const int t = a.target ? a.target[p] : 0;
        const int32_t lo = a.spans[2 * i], hi = a.spans[2 * i + 1];
        int32_t mine = -1;
        if (t >= 0 && t < T && (!a.use || a.use[p]) && lo >= 0) {
            const unsigned long long key = (unsigned long long)p << 2;
            const int64_t sh = a.shift ? a.shift[p] : 0;
            const int64_t tl = a.toff[t + 1] - a.toff[t];
            if (hi < lo) atomicMin(&a.stat[PS_ERR_ROW], key | PR_ORDER);
            else if (lo + sh < 0 || hi + sh >= tl) atomicMin(&a.stat[PS_ERR_ROW], key | PR_RANGE);
            else { mine = p; base = a.toff[t] + lo + sh; len = (int64_t)hi - lo + 1; }     // inside [0, mtot)
        }
        a.rowpair[i] = mine;
    }
    for_each_point(base, len, 0, lane, [&](int64_t pt, int32_t) { atomicAdd((unsigned long long *)&a.off[pt], 1ull); });
}

__global__ __launch_bounds__(PILE_THREADS)
void k_pile_plan(const pile_kargs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * PILE_THREADS + threadIdx.x;
    long long n = 0;
    if (i < a.mtot) n = a.off[i + 1] - a.off[i];
    long long mx = n, nl = n > a.tier ? 1 : 0, nc = n > a.tier ? (n + a.tier - 1) / a.tier : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long m2 = __shfl_xor(mx, o);
        mx = m2 > mx ? m2 : mx;
        nl += __shfl_xor(nl, o);
        nc += __shfl_xor(nc, o);
    }
    if (lane == 0) {
        if (mx > 0) atomicMax(&a.stat[PS_LONGEST], (unsigned long long)mx);
        if (nl > 0) { atomicAdd(&a.stat[PS_NLONG], (unsigned long long)nl); atomicAdd(&a.stat[PS_NCHUNKS], (unsigned long long)nc); }
    }
}

__global__ __launch_bounds__(PILE_THREADS)
void k_pile_fill(const pile_kargs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * PILE_THREADS + threadIdx.x;
    int64_t base = 0, len = 0;
    if (i < a.nrows) {
        const int p = a.rowpair[i];
        if (p >= 0) {                                       // checked by k_pile_count: the span lies inside its target
            const int t = a.target ? a.target[p] : 0;
            const int32_t lo = a.spans[2 * i], hi = a.spans[2 * i + 1];
            base = a.toff[t] + lo + (a.shift ? a.shift[p] : 0);
            len = (int64_t)hi - lo + 1;
        }
    }
    for_each_point(base, len, (int32_t)i, lane, [&](int64_t pt, int32_t e) {
        const int64_t at = (int64_t)atomicAdd(&a.cur[pt], 1u);
        if (at < a.off[pt + 1] - a.off[pt]) a.ent[a.off[pt] + at] = e;      // (always: the count pass saw the same rows)
    });
}

// g[0 .. n) into ascending order, 2 <= n <= PILE_LDS_ENTRIES, by one wavefront (one block): bitonic network over the next
// power of two, the pad above every row index
__device__ void sort_run(int32_t *g, int n, int32_t *keys, int lane)
{
    int m = 2;
    while (m < n) m <<= 1;
    for (int i = lane; i < m; i += 64) keys[i] = i < n ? g[i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (m >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));        // pair t of the step: bit j clear / set
                const int q = i | j;
                const int32_t x = keys[i], y = keys[q];
                const bool up = (i & k) == 0;
                if ((x > y) == up) { keys[i] = y; keys[q] = x; }
            }
            __syncthreads();
        }
    for (int i = lane; i < n; i += 64) g[i] = keys[i];
    __syncthreads();
}

__global__ __launch_bounds__(64)
void k_pile_sort(const pile_kargs a)
{
    __shared__ int32_t keys[PILE_LDS_ENTRIES];
    const int lane = threadIdx.x;
    for (int64_t pt = blockIdx.x; pt < a.mtot; pt += gridDim.x) {
        const int64_t B = a.off[pt], n = a.off[pt + 1] - B;
        if (n < 2) continue;
        if (n <= a.tier) { sort_run(a.ent + B, (int)n, keys, lane); continue; }
        const int64_t nch = (n + a.tier - 1) / a.tier;      // the merge tier: list the chunks (k_pile_plan counted them)
        unsigned long long c0 = 0;
        if (lane == 0) c0 = atomicAdd(&a.stat[PS_CHUNK_CUR], (unsigned long long)nch);
        c0 = __shfl(c0, 0);
        for (int64_t c = lane; c < nch; c += 64) { a.chunks[2 * (c0 + c)] = pt; a.chunks[2 * (c0 + c) + 1] = c; }
    }
}

__global__ __launch_bounds__(64)
void k_pile_sort_chunks(const pile_kargs a, int64_t nchunks)
{
    __shared__ int32_t keys[PILE_LDS_ENTRIES];
    const int lane = threadIdx.x;
    for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
        const int64_t pt = a.chunks[2 * k], c = a.chunks[2 * k + 1];
        const int64_t B = a.off[pt], N = a.off[pt + 1] - B, g0 = c * a.tier;
        const int64_t n = N - g0 < a.tier ? N - g0 : a.tier;
        if (n >= 2) sort_run(a.ent + B + g0, (int)n, keys, lane);
    }
}

// one pass of the merge tier: the sorted runs of W entries of every listed list, pairwise, src -> dst
__global__ __launch_bounds__(PILE_THREADS)
void k_pile_merge(const pile_kargs a, int64_t nchunks, const int32_t *__restrict__ src, int32_t *__restrict__ dst, int64_t W)
{
    for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
        const int64_t pt = a.chunks[2 * k], c = a.chunks[2 * k + 1];
        const int64_t B = a.off[pt], N = a.off[pt + 1] - B, g0 = c * a.tier;
        const int64_t n = N - g0 < a.tier ? N - g0 : a.tier;
        for (int64_t i = threadIdx.x; i < n; i += PILE_THREADS) {
            const int64_t g = g0 + i;
            const int32_t key = src[B + g];
            const int64_t r0 = (g / W) * W;                 // my run, its sibling [s0, s1)
            const int64_t s0 = ((g / W) ^ 1) * W;
            const int64_t s1 = s0 + W < N ? s0 + W : N;
            int64_t lo = s0, hi = s1 > s0 ? s1 : s0;        // entries of the sibling below key: [s0, lo)
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (src[B + mid] < key) lo = mid + 1; else hi = mid;
            }
            dst[B + (r0 < s0 ? r0 : s0) + (g - r0) + (lo - s0)] = key;
        }
    }
}

__global__ __launch_bounds__(64)
void k_pile_reduce(const pile_kargs a)
{
    __shared__ double nodes[256];
    const int lane = threadIdx.x;
    const double INF = __builtin_huge_val();
    for (int64_t pt = blockIdx.x; pt < a.mtot; pt += gridDim.x) {
        const int64_t B = a.off[pt], n = a.off[pt + 1] - B;
        sk_pile_rec r;
        r.pad = 0;
        if (n == 0) {
            r.level = r.level_sd = r.vmin = r.vmax = r.dwell_mean = r.dwell_sd = __builtin_nan("");
            r.depth = r.n = r.shared = 0;
            if (lane == 0) a.out[pt] = r;
            continue;
        }
        const int32_t *rows = a.ent + B;
        // one look: extremes, the first NaN, the exact dwell sum, changes of pair, rows that cover more than one point
        double mn = INF, mx = -INF;
        long long nan_at = 0x7fffffffffffffffll, dsum = 0, dabs = 0;
        int depth = 0, shared = 0;
        for (int64_t k = lane; k < n; k += 64) {
            const int32_t e = rows[k];
            const double v = a.value[e];
            if (v != v) { if (k < nan_at) nan_at = k; }
            else { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
            const long long d = a.dwell ? a.dwell[e] : 1;
            dsum += d; dabs += d < 0 ? -d : d;
            if (k == 0 || a.rowpair[rows[k - 1]] != a.rowpair[e]) depth++;
            shared += a.spans[2 * (int64_t)e + 1] > a.spans[2 * (int64_t)e] ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double mn2 = __shfl_xor(mn, o), mx2 = __shfl_xor(mx, o);
            mn = mn2 < mn ? mn2 : mn; mx = mx2 > mx ? mx2 : mx;
            const long long na2 = __shfl_xor(nan_at, o);
            nan_at = na2 < nan_at ? na2 : nan_at;
            dsum += __shfl_xor(dsum, o); dabs += __shfl_xor(dabs, o);
            depth += __shfl_xor(depth, o); shared += __shfl_xor(shared, o);
        }
        const bool has_nan = nan_at < n;
        // a NaN result: the list's first NaN, quieted; one the arithmetic made (inf - inf) has numpy's bits on x86-64
        double nanv = __longlong_as_double((long long)0xFFF8000000000000ull);
        if (has_nan) nanv = __longlong_as_double(__double_as_longlong(a.value[rows[nan_at]]) | 0x0008000000000000ll);
        auto fix = [&](double x) { return x == x ? x : nanv; };
        const double cnt = (double)n;
        auto val = [&](int64_t k) { return a.value[rows[k]]; };
        const double mean = wave_np_sum<true>(n, nodes, lane, val) / cnt;
        const double ssq = wave_np_sum<true>(n, nodes, lane, [&](int64_t k) { const double q = val(k) - mean; return q * q; });
        r.level = fix(mean);
        r.level_sd = fix(sqrt(ssq / cnt));
        r.vmin = has_nan ? nanv : mn;
        r.vmax = has_nan ? nanv : mx;
        auto dw = [&](int64_t k) { return a.dwell ? (double)a.dwell[rows[k]] : 1.0; };
        r.dwell_mean = (double)dsum / cnt;
        // np.std's mean is the float64 sum over n: the exact sum again while every partial sum is below 2^53
        const double dmean = dabs < (1ll << 53) ? r.dwell_mean : wave_np_sum<true>(n, nodes, lane, dw) / cnt;
        r.dwell_sd = sqrt(wave_np_sum<true>(n, nodes, lane, [&](int64_t k) { const double q = dw(k) - dmean; return q * q; }) / cnt);
        r.depth = depth; r.n = (int32_t)n; r.shared = shared;
        if (lane == 0) a.out[pt] = r;
    }
}

inline size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }
inline unsigned grid_for(int64_t items, int per)
{
    const int64_t g = (items + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > PILE_MAX_GRID ? PILE_MAX_GRID : g));
}

// what the arguments alone decide (nothing is read through a data pointer but tlen)
int pile_check_args(const int64_t *span_off, const int32_t *spans, const double *value, int32_t npairs, int64_t nrows,
                    const int64_t *tlen, int32_t ntargets, const void *out, const void *ent_off, const void *ent_row,
                    int64_t ent_cap, int64_t *mtot)
{
    if (npairs < 0 || nrows < 0 || ntargets < 0) return sk_fail(SK_ERR_INVALID, "pile-up: negative npairs, nrows or ntargets");
    if (!span_off || (ntargets > 0 && !tlen)) return sk_fail(SK_ERR_INVALID, "pile-up: NULL span_off or tlen");
    if (nrows > 0 && (!spans || !value)) return sk_fail(SK_ERR_INVALID, "pile-up: NULL spans or value");
    if ((ent_off == nullptr) != (ent_row == nullptr)) return sk_fail(SK_ERR_INVALID, "pile-up: ent_off and ent_row go together");
    if (ent_cap < 0) return sk_fail(SK_ERR_INVALID, "pile-up: negative ent_cap");
    int64_t m = 0;
    for (int32_t t = 0; t < ntargets; t++) {
        if (tlen[t] < 0) return sk_fail(SK_ERR_INVALID, "pile-up: target %d has the negative length %lld", t, (long long)tlen[t]);
        if (tlen[t] > PILE_MAX_FLAT || (m += tlen[t]) > PILE_MAX_FLAT)
            return sk_fail(SK_ERR_UNSUPPORTED, "pile-up: more than 2^40 target points");
    }
    if (m > 0 && !out) return sk_fail(SK_ERR_INVALID, "pile-up: NULL out");
    if (nrows > 0x7fffffffll) return sk_fail(SK_ERR_UNSUPPORTED, "pile-up: more than 2^31 - 1 rows");
    *mtot = m;
    return SK_OK;
}

} // namespace

static_assert(sizeof(sk_pile_rec) == 64, "sk_pile_rec is 64 bytes (include/squigglekit_hip.h)");

int sk_pileup_run(sk_ctx *c, const int64_t *d_span_off, const int32_t *d_spans, const double *d_value, const int32_t *d_dwell,
                  const int32_t *d_target, const int32_t *d_shift, const uint8_t *d_use, int32_t npairs, int64_t nrows,
                  const int64_t *tlen, int32_t ntargets, sk_pile_rec *d_out, int64_t *d_ent_off, int32_t *d_ent_row,
                  int64_t ent_cap)
{
    int rc;
    int64_t mtot = 0;
    if ((rc = pile_check_args(d_span_off, d_spans, d_value, npairs, nrows, tlen, ntargets, d_out, d_ent_off, d_ent_row,
                              ent_cap, &mtot))) return rc;
    int tier = PILE_LDS_ENTRIES;
    if (const char *e = sk_tune("SK_PILE_LDS_ENTRIES")) { const long v = atol(e); if (v >= 2 && v <= PILE_LDS_ENTRIES) tier = (int)v; }
    const bool work = npairs > 0 && nrows > 0;

    // scratch: counters | target offsets | offsets | the scan's block sums | cursors | row pairs
    const size_t b_stat = PS_WORDS * 8, b_toff = ((size_t)ntargets + 1) * 8, b_off = ((size_t)mtot + 1) * 8;
    const size_t b_bsum = (size_t)sk_scan_blocks(mtot) * 8, b_cur = up8((size_t)mtot * 4), b_rp = up8((size_t)nrows * 4);
    if ((rc = sk_reserve(c, &c->pile, b_stat + b_toff + b_off + b_bsum + b_cur + b_rp))) return rc;
    char *base = (char *)c->pile.p;
    pile_kargs k;
    k.span_off = d_span_off; k.spans = d_spans; k.value = d_value; k.dwell = d_dwell; k.target = d_target; k.shift = d_shift;
    k.use = d_use; k.npairs = npairs; k.ntargets = ntargets; k.nrows = nrows; k.mtot = mtot;
    k.stat = (unsigned long long *)base;
    k.toff = (const int64_t *)(base + b_stat);
    k.off = (int64_t *)(base + b_stat + b_toff);
    int64_t *d_bsum = (int64_t *)(base + b_stat + b_toff + b_off);
    k.cur = (uint32_t *)(base + b_stat + b_toff + b_off + b_bsum);
    k.rowpair = (int32_t *)(base + b_stat + b_toff + b_off + b_bsum + b_cur);
    k.ent = nullptr; k.chunks = nullptr; k.tier = tier; k.out = d_out;

    std::vector<int64_t> head(PS_WORDS + (size_t)ntargets + 1);
    for (int i = 0; i < PS_WORDS; i++) head[i] = i <= PS_ERR_ROW ? -1 : 0;
    head[PS_WORDS] = 0;
    for (int32_t t = 0; t < ntargets; t++) head[PS_WORDS + t + 1] = head[PS_WORDS + t] + tlen[t];
    SK_HIP(hipMemcpyAsync(base, head.data(), head.size() * 8, hipMemcpyHostToDevice, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));                // (head is a local; an earlier call has also finished with the scratch)
    SK_HIP(hipEventRecord(c->ev[0], c->stream));
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    SK_HIP(hipMemsetAsync(k.off, 0, b_off, c->stream));
    if (mtot > 0) SK_HIP(hipMemsetAsync(k.cur, 0, (size_t)mtot * 4, c->stream));
    c->pile_entries = 0; c->pile_longest = 0; c->pile_long_lists = 0;
    c->pile_scratch_bytes = (int64_t)(b_stat + b_toff + b_off + b_bsum + b_cur + b_rp);

    unsigned long long stat[PS_WORDS] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0};
    int64_t total = 0;
    if (work) {
        const int64_t items = nrows > npairs ? nrows : (int64_t)npairs;
        hipLaunchKernelGGL(k_pile_count, dim3((unsigned)((items + PILE_THREADS - 1) / PILE_THREADS)), dim3(PILE_THREADS), 0,
                           c->stream, k);
        SK_HIP(hipGetLastError());
        if ((rc = sk_launch_scan_i64(c, k.off, mtot, d_bsum, k.off))) return rc;
        if (mtot > 0) {
            hipLaunchKernelGGL(k_pile_plan, dim3((unsigned)((mtot + PILE_THREADS - 1) / PILE_THREADS)), dim3(PILE_THREADS), 0,
                               c->stream, k);
            SK_HIP(hipGetLastError());
        }
        // the one read-back: the verdict, the entries, the plan
        SK_HIP(hipMemcpyAsync(stat, k.stat, sizeof stat, hipMemcpyDeviceToHost, c->stream));
        SK_HIP(hipMemcpyAsync(&total, k.off + mtot, 8, hipMemcpyDeviceToHost, c->stream));
        SK_HIP(hipStreamSynchronize(c->stream));
        if (stat[PS_ERR_OFF] != ~0ull) {
            const long long p = (long long)(stat[PS_ERR_OFF] >> 2);
            switch ((int)(stat[PS_ERR_OFF] & 3)) {
            case PO_FIRST: return sk_fail(SK_ERR_INVALID, "pile-up: span_off[0] is not 0 (pair 0)");
            case PO_ORDER: return sk_fail(SK_ERR_INVALID, "pile-up: span_off decreases at pair %lld", p);
            default:       return sk_fail(SK_ERR_INVALID, "pile-up: span_off[npairs] is not nrows (pair %lld)", p);
            }
        }
        if (stat[PS_ERR_ROW] != ~0ull) {
            const long long p = (long long)(stat[PS_ERR_ROW] >> 2);
            switch ((int)(stat[PS_ERR_ROW] & 3)) {
            case PR_TARGET: return sk_fail(SK_ERR_INVALID, "pile-up: pair %lld names a target beyond the %d given", p, ntargets);
            case PR_ORDER:  return sk_fail(SK_ERR_INVALID, "pile-up: pair %lld has a row whose span ends before it begins", p);
            default:        return sk_fail(SK_ERR_INVALID, "pile-up: pair %lld has a row whose shifted span leaves its target", p);
            }
        }
        if (total > PILE_MAX_FLAT) return sk_fail(SK_ERR_UNSUPPORTED, "pile-up: more than 2^40 entries");
        if (stat[PS_LONGEST] > 0x7fffffffull) return sk_fail(SK_ERR_UNSUPPORTED, "pile-up: more than 2^31 - 1 entries on one point");
    }
    if (d_ent_row && ent_cap < total)
        return sk_fail(SK_ERR_INVALID, "pile-up: ent_cap %lld is below the %lld entries", (long long)ent_cap, (long long)total);

    const int64_t nlong = (int64_t)stat[PS_NLONG], nchunks = (int64_t)stat[PS_NCHUNKS], longest = (int64_t)stat[PS_LONGEST];
    if ((rc = sk_reserve(c, &c->pileent, (size_t)(total > 0 ? total : 1) * 4))) return rc;
    k.ent = (int32_t *)c->pileent.p;
    c->pile_scratch_bytes += total * 4;
    int32_t *alt = nullptr;
    if (nlong > 0) {
        if ((rc = sk_reserve(c, &c->pilealt, (size_t)nchunks * 16 + (size_t)total * 4))) return rc;
        k.chunks = (int64_t *)c->pilealt.p;
        alt = (int32_t *)((char *)c->pilealt.p + (size_t)nchunks * 16);
        c->pile_scratch_bytes += nchunks * 16 + total * 4;
    }
    if (total > 0) {
        hipLaunchKernelGGL(k_pile_fill, dim3((unsigned)((nrows + PILE_THREADS - 1) / PILE_THREADS)), dim3(PILE_THREADS), 0,
                           c->stream, k);
        hipLaunchKernelGGL(k_pile_sort, dim3(grid_for(mtot, 1)), dim3(64), 0, c->stream, k);
        SK_HIP(hipGetLastError());
        if (nlong > 0) {
            hipLaunchKernelGGL(k_pile_sort_chunks, dim3(grid_for(nchunks, 1)), dim3(64), 0, c->stream, k, nchunks);
            int passes = 0;
            for (int64_t W = tier; W < longest; W *= 2) passes++;
            const int32_t *src = k.ent;
            int32_t *dst = alt;
            int64_t W = tier;
            for (int p = 0; p < passes + (passes & 1); p++, W *= 2) {      // (an odd count: one more pass copies the lists back)
                hipLaunchKernelGGL(k_pile_merge, dim3(grid_for(nchunks, 1)), dim3(PILE_THREADS), 0, c->stream, k, nchunks, src,
                                   dst, W);
                int32_t *t = (int32_t *)src; src = dst; dst = t;
            }
            SK_HIP(hipGetLastError());
        }
    }
    if (mtot > 0) {
        hipLaunchKernelGGL(k_pile_reduce, dim3(grid_for(mtot, 1)), dim3(64), 0, c->stream, k);
        SK_HIP(hipGetLastError());
    }
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->ev_valid = true;
    if (d_ent_off) {
        SK_HIP(hipMemcpyAsync(d_ent_off, k.off, b_off, hipMemcpyDefault, c->stream));
        if (total > 0) SK_HIP(hipMemcpyAsync(d_ent_row, k.ent, (size_t)total * 4, hipMemcpyDefault, c->stream));
    }
    c->pile_entries = total; c->pile_longest = longest; c->pile_long_lists = nlong;
    return SK_OK;
}

extern "C" {

int sk_pileup_dev(const int64_t *d_span_off, const int32_t *d_spans, const double *d_value, const int32_t *d_dwell,
                  const int32_t *d_target, const int32_t *d_shift, const uint8_t *d_use, int32_t npairs, int64_t nrows,
                  const int64_t *tlen, int32_t ntargets, sk_pile_rec *d_out, int64_t *d_ent_off, int32_t *d_ent_row,
                  int64_t ent_cap)
{
    SK_ENTER(c);
    return sk_pileup_run(c, d_span_off, d_spans, d_value, d_dwell, d_target, d_shift, d_use, npairs, nrows, tlen, ntargets,
                         d_out, d_ent_off, d_ent_row, ent_cap);
}

int sk_pileup(const int64_t *span_off, const int32_t *spans, const double *value, const int32_t *dwell,
              const int32_t *target, const int32_t *shift, const uint8_t *use, int32_t npairs, int64_t nrows,
              const int64_t *tlen, int32_t ntargets, sk_pile_rec *out, int64_t *ent_off, int32_t *ent_row, int64_t ent_cap)
{
    SK_ENTER(c);
    int rc;
    int64_t mtot = 0;
    if ((rc = pile_check_args(span_off, spans, value, npairs, nrows, tlen, ntargets, out, ent_off, ent_row, ent_cap, &mtot)))
        return rc;                                          // before anything is copied or launched
    // the inputs, one after the other in c->pilein (8-byte aligned each); the records in c->pileout
    const size_t P = (size_t)npairs, E = (size_t)nrows;
    const size_t b_so = (P + 1) * 8, b_sp = E * 8, b_v = E * 8, b_d = dwell ? up8(E * 4) : 0, b_t = target ? up8(P * 4) : 0;
    const size_t b_s = shift ? up8(P * 4) : 0, b_u = use ? up8(P) : 0;
    if ((rc = sk_reserve(c, &c->pilein, b_so + b_sp + b_v + b_d + b_t + b_s + b_u + 8))) return rc;
    if ((rc = sk_reserve(c, &c->pileout, (size_t)(mtot > 0 ? mtot : 1) * sizeof(sk_pile_rec)))) return rc;
    char *p = (char *)c->pilein.p;
    auto put = [&](const void *src, size_t bytes, size_t room) -> void * {
        void *at = p;
        if (bytes > 0 && hipMemcpyAsync(at, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return nullptr;
        p += room;
        return at;
    };
    const int64_t *d_so = (const int64_t *)put(span_off, b_so, b_so);
    const int32_t *d_sp = (const int32_t *)put(spans, E * 8, b_sp);
    const double  *d_v = (const double *)put(value, E * 8, b_v);
    const int32_t *d_d = dwell ? (const int32_t *)put(dwell, E * 4, b_d) : nullptr;
    const int32_t *d_t = target ? (const int32_t *)put(target, P * 4, b_t) : nullptr;
    const int32_t *d_s = shift ? (const int32_t *)put(shift, P * 4, b_s) : nullptr;
    const uint8_t *d_u = use ? (const uint8_t *)put(use, P, b_u) : nullptr;
    if (!d_so || !d_sp || !d_v || (dwell && !d_d) || (target && !d_t) || (shift && !d_s) || (use && !d_u))
        return sk_fail(SK_ERR_HIP, "pile-up: the upload failed: %s", hipGetErrorString(hipGetLastError()));
    sk_pile_rec *d_out = (sk_pile_rec *)c->pileout.p;
    if ((rc = sk_pileup_run(c, d_so, d_sp, d_v, d_d, d_t, d_s, d_u, npairs, nrows, tlen, ntargets, d_out, ent_off, ent_row,
                            ent_cap))) return rc;
    if (mtot > 0)
        SK_HIP(hipMemcpyAsync(out, d_out, (size_t)mtot * sizeof(sk_pile_rec), hipMemcpyDeviceToHost, c->stream));
    SK_HIP(hipStreamSynchronize(c->stream));
    return SK_OK;
}

int sk_last_pileup_plan(int64_t *entries, int64_t *longest_list, int64_t *lists_in_long_tier, int64_t *scratch_bytes)
{
    SK_ENTER(c);
    if (entries) *entries = c->pile_entries;
    if (longest_list) *longest_list = c->pile_longest;
    if (lists_in_long_tier) *lists_in_long_tier = c->pile_long_lists;
    if (scratch_bytes) *scratch_bytes = c->pile_scratch_bytes;
    return SK_OK;
}

} // extern "C"
