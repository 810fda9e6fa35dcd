// sk_hits.hip -- MotifSeq hit lists: up to K non-overlapping matches per read and motif, for gfx950.
//
// MotifSeq reports the first argmin of the DTW last row (/root/reference/MotifSeq.py:437-439); view_region plots that
// whole row (:506-513).  A hit list keeps going: from the row of costs d_j = D[N-1][j] and the back-trace starts
// s_j (sk_sdtw.hip, MODE_ROWS) it takes, K times, the smallest admissible d_j (ties: the smallest j), where a column is
// admissible if d_j <= max_dist and its interval [s_j, j] is disjoint from every interval taken before.  Hit 1 is
// the first argmin of the row, i.e. today's (dist, start, end).
//
// k_hits_select: one wavefront per read.  Lane l owns the columns l, l + 64, ...; each round every lane keeps its best
// admissible (d, j) and a wave reduction picks the winner.  d >= 0, so the bit pattern of d ordered as an unsigned
// integer orders the values too and (bits, j) is an exact lexicographic key.  The accepted intervals are wave-uniform
// (lane h holds interval h, read back with v_readlane).  Rows of up to 64 * CACHE columns are loaded into registers
// once, and a column that overlaps an accepted interval has its key cleared there, so a round is a plain minimum;
// longer rows are read again from memory each round and tested against the intervals.
#include "sk_common.h"
#include <limits.h>

namespace {

constexpr int HIT_CACHE = 64;           // columns per lane kept in registers: rows of up to 4 096 columns

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

// (key, j) lexicographic minimum over the wave; every lane ends with the winner
__device__ __forceinline__ hit_cand wave_min(hit_cand c)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        hit_cand q;
        q.key = __shfl_xor(c.key, o);
        q.j = __shfl_xor(c.j, o);
        q.s = __shfl_xor(c.s, o);
        if (q.key < c.key || (q.key == c.key && q.j < c.j)) c = q;
    }
    return c;
}

template <bool CACHED>
__global__ __launch_bounds__(256)
void k_hits_select(const double *rowD, const int32_t *rowS, int64_t row_stride, const sk_hit *rec, int nreads, int K,
                   double max_dist, sk_hit *out, int32_t *count)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nreads) return;                          // (wave-uniform)
    const sk_hit h0 = rec[r];
    const int n = h0.n, flags = h0.flags;
    const double *d = rowD + (int64_t)r * row_stride;
    const int32_t *s = rowS + (int64_t)r * row_stride;
    sk_hit *o = out + (int64_t)r * K;
    int nh = 0;
    int hs = -1, he = -1;                             // lane h: the interval of hit h
    if (n > 0 && !(flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE))) {
        unsigned long long ck[CACHED ? HIT_CACHE : 1];
        int cs[CACHED ? HIT_CACHE : 1];
        if constexpr (CACHED) {
#pragma unroll
            for (int i = 0; i < HIT_CACHE; i++) {
                const int j = lane + 64 * i;
                const double v = (j < n) ? d[j] : 0.0;
                ck[i] = (j < n && v <= max_dist) ? (unsigned long long)__double_as_longlong(v) : ~0ull;
                cs[i] = (j < n) ? s[j] : 0;
            }
        }
        while (nh < K) {
            hit_cand b;
            b.key = ~0ull; b.j = INT_MAX; b.s = -1;
            if constexpr (CACHED) {
#pragma unroll
                for (int i = 0; i < HIT_CACHE; i++)   // increasing j per lane: a strict < keeps the smallest j
                    if (ck[i] < b.key) { b.key = ck[i]; b.j = lane + 64 * i; b.s = cs[i]; }
            } else {
                for (int j = lane; j < n; j += 64) {
                    const double v = d[j];
                    if (!(v <= max_dist)) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(v);
                    if (key < b.key && admissible(j, s[j], nh, hs, he)) { b.key = key; b.j = j; b.s = s[j]; }
                }
            }
            b = wave_min(b);
            if (b.j == INT_MAX) break;                // nothing admissible is left
            if constexpr (CACHED) {
                // a cached column that overlaps the new interval is out for good: its key becomes "none", so each
                // round is a plain minimum over the registers and a column meets each interval once
#pragma unroll
                for (int i = 0; i < HIT_CACHE; i++)
                    if (!(lane + 64 * i < b.s || cs[i] > b.j)) ck[i] = ~0ull;
            }
            if (lane == nh) { hs = b.s; he = b.j; }
            if (lane == 0) {
                sk_hit h;
                h.dist = __longlong_as_double((long long)b.key); h.start = b.s; h.end = b.j; h.n = n; h.flags = flags;
                o[nh] = h;
            }
            nh++;
        }
    }
    for (int k = nh + lane; k < K; k += 64) {         // unused slots: no match, the read's n and flags
        sk_hit h;
        h.dist = __builtin_nan(""); h.start = -1; h.end = -1; h.n = n; h.flags = flags;
        o[k] = h;
    }
    if (lane == 0) count[r] = nh;
}

} // namespace

int sk_launch_hits_select(sk_ctx *c, const double *rowD, const int32_t *rowS, int64_t row_stride, const sk_hit *rec,
                          int32_t nreads, int32_t K, double max_dist, sk_hit *out, int32_t *count)
{
    if (nreads <= 0) return SK_OK;
    const dim3 grid((nreads + 3) / 4), block(256);
    if (row_stride <= 64 * HIT_CACHE)
        hipLaunchKernelGGL(k_hits_select<true>, grid, block, 0, c->stream, rowD, rowS, row_stride, rec, nreads, K, max_dist,
                           out, count);
    else
        hipLaunchKernelGGL(k_hits_select<false>, grid, block, 0, c->stream, rowD, rowS, row_stride, rec, nreads, K,
                           max_dist, out, count);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
