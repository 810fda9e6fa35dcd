// sk_pairhits.hip -- hit lists over a pair list and over the stored rows of a mapping session, for gfx950.
//
// sk_hits.hip selects up to K disjoint matches from last rows that share one stride.  The rows of a pair list are ragged
// (one per pair, as long as the pair's target) and those of a mapping session lie inside the session's row state, and
// either may be far longer than the 4 096 columns a wavefront can keep in registers.  k_rowhits_* take a TABLE of rows
// (sk_rowhit_entry: first column inside the D / S arrays, length, list index, flags) and apply sk_hits.hip's rule word
// for word: K rounds, each takes the smallest admissible d_j (ties: the smallest j); a column is admissible if
// d_j <= max_dist and [s_j, j] is disjoint from every interval taken before.  d >= 0, so the bits of d ordered as an
// unsigned integer order the values and (bits, j) is an exact lexicographic key.
//
//   short tier  rows of up to 4 096 columns: one wavefront per row, the row cached in registers, a column that overlaps
//               an accepted interval cleared there (k_hits_select<true>'s scheme; its body is restated here so that
//               sk_hits.hip and its code object stay as they are).
//   long tier   any n: one workgroup of W wavefronts per row, each wavefront owning a contiguous stripe of whole
//               64-column blocks.  Per round every wavefront forms the minimum of its stripe as the one-wavefront
//               kernel does (the row is read again, four loads in flight per lane, candidates tested against the
//               interval list), lane 0 of each leaves it in LDS, one barrier, and every wavefront reduces the W minima
//               again -- so all of them hold the winner and append it to their own copy of the interval list (lane h:
//               interval h); no second barrier: the LDS slots alternate between two sets by round parity.
//               W = 16, the most one workgroup holds.  One wavefront per row keeps four loads in flight per lane and
//               waits out their latency round after round; 16 per row keep the memory system busy instead (measured,
//               tools/pair_hits_throughput.py: 1 024 rows of 100 000 columns, K = 2, 0.34 ms against 0.66 ms with one
//               wavefront each -- about 4.8 TB/s of row reads).  The kernel needs 30 registers, so two such workgroups
//               fit a CU (8 waves per SIMD, the hardware's limit): a session of 1 024 rows fills the chip in two passes
//               at full occupancy, and a lone row -- one read against one reference -- still gets 16 wavefronts, not
//               one.  SK_ROWHITS_ONE_WAVE=1 runs the same kernel with W = 1 (the A/B of that tool).
// Both tiers take their tables longest row first.
#include "sk_common.h"
#include <limits.h>
#include <algorithm>

namespace {

constexpr int RH_CACHE = 64;            // columns per lane kept in registers: rows of up to 4 096 columns
constexpr int RH_WAVES = 16;            // wavefronts per row of the long tier

struct hit_cand {
    unsigned long long key;             // bits of d (~0: none)
    int j, s;
};

__device__ __forceinline__ bool admissible(int j, int s, int nh, int hs, int he)
{
    for (int h = 0; h < nh; h++) {
        const int a0 = __builtin_amdgcn_readlane(hs, h), e0 = __builtin_amdgcn_readlane(he, h);
        if (!(j < a0 || s > e0)) return false;
    }
    return true;
}

__device__ __forceinline__ bool before(const hit_cand &q, const hit_cand &c)
{
    return q.key < c.key || (q.key == c.key && q.j < c.j);
}

// (key, j) lexicographic minimum over the wave; every lane ends with the winner
__device__ __forceinline__ hit_cand wave_min(hit_cand c)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        hit_cand q;
        q.key = __shfl_xor(c.key, o);
        q.j = __shfl_xor(c.j, o);
        q.s = __shfl_xor(c.s, o);
        if (before(q, c)) c = q;
    }
    return c;
}

__device__ __forceinline__ void put_hit(sk_hit *o, unsigned long long key, int s, int j, int n, int flags)
{
    sk_hit h;
    h.dist = __longlong_as_double((long long)key); h.start = s; h.end = j; h.n = n; h.flags = flags;
    *o = h;
}

__device__ __forceinline__ void put_unused(sk_hit *o, int from, int step, int K, int n, int flags)
{
    for (int k = from; k < K; k += step) {            // unused slots: no match, the row's n and flags
        sk_hit h;
        h.dist = __builtin_nan(""); h.start = -1; h.end = -1; h.n = n; h.flags = flags;
        o[k] = h;
    }
}

// ---- short tier: one wavefront per row, the row in registers -----------------------------------------------------------
__global__ __launch_bounds__(256)
void k_rowhits_select(const double *__restrict__ rowD, const int32_t *__restrict__ rowS, const sk_rowhit_entry *__restrict__ tab,
                      int nrows, int K, double max_dist, sk_hit *__restrict__ out, int32_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nrows) return;                           // (wave-uniform)
    const sk_rowhit_entry e = tab[r];
    const int n = e.n, flags = e.flags & SK_FLAG_PUBLIC;
    const double *d = rowD + e.col0;
    const int32_t *s = rowS + e.col0;
    sk_hit *o = out + e.list * K;
    int nh = 0;
    if (n > 0 && !(e.flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE | SK_ROWHIT_NOROW))) {
        unsigned long long ck[RH_CACHE];
        int cs[RH_CACHE];
#pragma unroll
        for (int i = 0; i < RH_CACHE; i++) {
            const int j = lane + 64 * i;
            const double v = (j < n) ? d[j] : 0.0;
            ck[i] = (j < n && v <= max_dist) ? (unsigned long long)__double_as_longlong(v) : ~0ull;
            cs[i] = (j < n) ? s[j] : 0;
        }
        while (nh < K) {
            hit_cand b;
            b.key = ~0ull; b.j = INT_MAX; b.s = -1;
#pragma unroll
            for (int i = 0; i < RH_CACHE; i++)        // increasing j per lane: a strict < keeps the smallest j
                if (ck[i] < b.key) { b.key = ck[i]; b.j = lane + 64 * i; b.s = cs[i]; }
            b = wave_min(b);
            if (b.j == INT_MAX) break;                // nothing admissible is left
#pragma unroll
            for (int i = 0; i < RH_CACHE; i++)        // a column that overlaps the new interval is out for good
                if (!(lane + 64 * i < b.s || cs[i] > b.j)) ck[i] = ~0ull;
            if (lane == 0) put_hit(o + nh, b.key, b.s, b.j, n, flags);
            nh++;
        }
    }
    put_unused(o, nh + lane, 64, K, n, flags);
    if (lane == 0) count[e.list] = nh;
}

// ---- long tier: W wavefronts per row, a contiguous stripe each ---------------------------------------------------------
template <int W>
__global__ __launch_bounds__(64 * W)
void k_rowhits_select_long(const double *__restrict__ rowD, const int32_t *__restrict__ rowS,
                           const sk_rowhit_entry *__restrict__ tab, int nrows, int K, double max_dist,
                           sk_hit *__restrict__ out, int32_t *__restrict__ count)
{
    __shared__ hit_cand meet[2][W];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.x;
    if (r >= nrows) return;                           // (block-uniform)
    const sk_rowhit_entry e = tab[r];                 // (block-uniform, and so is everything decided from it below)
    const int n = e.n, flags = e.flags & SK_FLAG_PUBLIC;
    const double *d = rowD + e.col0;
    const int32_t *s = rowS + e.col0;
    sk_hit *o = out + e.list * K;
    int nh = 0;
    int hs = -1, he = -1;                             // lane h of EVERY wavefront: the interval of hit h
    if (n > 0 && !(e.flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE | SK_ROWHIT_NOROW))) {
        // stripes of whole 64-column blocks: wavefront w owns [lo, hi)
        const int64_t blocks = ((int64_t)n + 63) / 64, per = (blocks + W - 1) / W;
        const int lo = (int)min((int64_t)n, per * 64 * w), hi = (int)min((int64_t)n, per * 64 * (w + 1));
        while (nh < K) {
            hit_cand b;
            b.key = ~0ull; b.j = INT_MAX; b.s = -1;
            for (int64_t j0 = (int64_t)lo + lane; j0 < hi; j0 += 256) {     // increasing j per lane: a strict < keeps the smallest
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int64_t jj = j0 + 64 * u;
                    v[u] = (jj < hi) ? d[jj] : __builtin_nan("");           // NaN fails the test below
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!(v[u] <= max_dist)) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(v[u]);
                    if (key < b.key) {
                        const int j = (int)(j0 + 64 * u), sj = s[j];
                        if (admissible(j, sj, nh, hs, he)) { b.key = key; b.j = j; b.s = sj; }
                    }
                }
            }
            b = wave_min(b);
            if constexpr (W > 1) {
                hit_cand *m = meet[nh & 1];
                if (lane == 0) m[w] = b;
                __syncthreads();
                hit_cand q;
                q.key = ~0ull; q.j = INT_MAX; q.s = -1;
                if (lane < W) q = m[lane];
                b = wave_min(q);
            }
            if (b.j == INT_MAX) break;                // nothing admissible is left (every wavefront sees the same winner)
            if (lane == nh) { hs = b.s; he = b.j; }
            if (threadIdx.x == 0) put_hit(o + nh, b.key, b.s, b.j, n, flags);
            nh++;
        }
    }
    if (w == 0) put_unused(o, nh + lane, 64, K, n, flags);
    if (threadIdx.x == 0) count[e.list] = nh;
}

} // namespace

// The select over `nrows` table entries (host, any order; reordered here): the table goes to c->rowhit at entry
// `at` on (room for it reserved by the caller through sk_rowhits_reserve), longest first, short tier then long tier.
int sk_rowhits_reserve(sk_ctx *c, int64_t nrows)
{
    return sk_reserve(c, &c->rowhit, (size_t)(nrows > 0 ? nrows : 1) * sizeof(sk_rowhit_entry));
}

int sk_launch_rowhits(sk_ctx *c, sk_rowhit_entry *tab, int64_t at, int32_t nrows, const double *rowD, const int32_t *rowS,
                      int32_t K, double max_dist, sk_hit *out, int32_t *count, int64_t *long_rows)
{
    if (nrows <= 0) return SK_OK;
    std::stable_sort(tab, tab + nrows, [](const sk_rowhit_entry &a, const sk_rowhit_entry &b) { return a.n > b.n; });
    int32_t nl = 0;
    while (nl < nrows && tab[nl].n > 64 * RH_CACHE) nl++;
    if (long_rows) *long_rows += nl;
    sk_rowhit_entry *d_tab = (sk_rowhit_entry *)c->rowhit.p + at;
    SK_HIP(hipMemcpyAsync(d_tab, tab, (size_t)nrows * sizeof(sk_rowhit_entry), hipMemcpyHostToDevice, c->stream));
    if (nl > 0) {
        if (sk_tune("SK_ROWHITS_ONE_WAVE"))
            hipLaunchKernelGGL(k_rowhits_select_long<1>, dim3((unsigned)nl), dim3(64), 0, c->stream, rowD, rowS,
                               (const sk_rowhit_entry *)d_tab, nl, K, max_dist, out, count);
        else
            hipLaunchKernelGGL(k_rowhits_select_long<RH_WAVES>, dim3((unsigned)nl), dim3(64 * RH_WAVES), 0, c->stream, rowD, rowS,
                               (const sk_rowhit_entry *)d_tab, nl, K, max_dist, out, count);
        SK_HIP(hipGetLastError());
    }
    const int32_t ns = nrows - nl;
    if (ns > 0) {
        hipLaunchKernelGGL(k_rowhits_select, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, c->stream, rowD, rowS,
                           (const sk_rowhit_entry *)(d_tab + nl), ns, K, max_dist, out, count);
        SK_HIP(hipGetLastError());
    }
    return SK_OK;
}
