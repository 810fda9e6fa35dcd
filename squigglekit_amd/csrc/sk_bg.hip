// sk_bg.hip -- MotifSeq read background: the statistics of each read's whole last DTW row, for gfx950.
//
// view_region draws a hit against its read's own row of distance scores (MotifSeq.py:507-513:
// M = np.mean(cost[-1,]), S = np.std(cost[-1,]), lines at M and M - S).  The hit-list path has that row on the device
// for a chunk of reads at a time (rowD of sk_launch_sdtw_rows); k_row_background reduces each row d[0 .. n) to one
// sk_bg_rec -- mean, std, median, MAD, the count below mean - std -- bit for bit what numpy gives on it.
//
// Shape: one wavefront (a workgroup of 64) per row, five looks at the same n values.  Rows of up to BG_LDS_COLS columns
// are copied once into LDS (32 KB at 4 000 columns: four rows in flight per CU) and every later look reads LDS; longer
// rows (the 36 977-column example read, up to the 1 M-sample limit) are read again from global memory, where a row of a
// few hundred KB stays in L2.
//   mean, std   np.add.reduce's order -- serial over chunks of 8 192, numpy's pairwise tree inside a chunk, one leaf
//               per lane (wave_pairwise_terms, sk_prepw_dev.h: the tree walk the zscale prologue uses); np.std is the
//               two-pass form sqrt(sum((d - mean)^2) / n).
//   median, MAD exact selection of the ranks (n - 1) / 2 and n / 2.  d >= 0 and |d - median| >= 0, so the bit pattern as
//               an unsigned integer orders the values (as k_hits_select relies on).  Scheme: a radix select over the
//               64-bit keys with a 256-bin histogram in LDS.  A first look takes the smallest and largest key; the bits
//               they share are settled without a pass, and the digits start right below them, where the keys of a row
//               do differ.  Each pass counts the digit of the keys that still match the prefix (LDS atomics), lane l
//               scans bins 4 l .. 4 l + 3 and the wave finds the bin holding the rank.  The passes stop when one key is
//               left (two or three digits for a few thousand columns) and one last look fetches that key and, for an
//               even n whose upper middle value is a different key, the smallest key above it.
//               Per-lane registers (k_hits_select<CACHED>) were the other candidate: 64 keys per lane hold 4 096
//               columns at most and cost 128 VGPRs before any work, and every probe of a bisection would still be a
//               full look; the histogram form has one code path for every row length and needs 1 KB of LDS.
//   below       one more look: d[j] < mean - std, strict.
#include "sk_common.h"
#include "sk_prepw_dev.h"
#include "sk_select_dev.h"

namespace {

constexpr int BG_STATIC_LDS = 256 * 8 + 256 * 4;         // the tree's partial sums + the digit histogram
constexpr int BG_LDS_COLS = (160 * 1024 - BG_STATIC_LDS) / 8;   // 20 096 columns fit beside them

template <bool STAGED>
__global__ __launch_bounds__(64)
void k_row_background(const double *__restrict__ rowD, int64_t row_stride, const sk_hit *__restrict__ rec, int nreads,
                      sk_bg_rec *__restrict__ out)
{
    __shared__ double nodes[256];
    __shared__ __attribute__((aligned(16))) unsigned hist[256];
    extern __shared__ double lrow[];
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    if (r >= nreads) return;
    const sk_hit h = rec[r];
    const int n = h.n < 0 ? 0 : (int)((int64_t)h.n < row_stride ? h.n : row_stride);   // never past the row
    if (n == 0 || (h.flags & (SK_FLAG_EMPTY | SK_FLAG_DEGENERATE))) {
        if (lane == 0) {
            sk_bg_rec b;
            b.mean = b.std = b.median = b.mad = __builtin_nan("");
            b.below = -1; b.n = h.n; b.reserved[0] = b.reserved[1] = 0;
            out[r] = b;
        }
        return;
    }
    const double *g = rowD + (int64_t)r * row_stride;
    if constexpr (STAGED) {
        for (int j = lane; j < n; j += 64) lrow[j] = g[j];
        __syncthreads();
    }
    auto at = [&](int j) -> double { if constexpr (STAGED) return lrow[j]; else return g[j]; };
    auto np_sum = [&](auto f) {                          // np.add.reduce over f(d[j])
        return wave_np_sum(n, nodes, lane, [&](int j) { return f(at(j)); });
    };
    const double mean = np_sum([](double v) { return v; }) / (double)n;
    const double ssq = np_sum([&](double v) { const double e = v - mean; return e * e; });
    const double sd = sqrt(ssq / (double)n);
    const double thr = mean - sd;
    int below = 0;
    for (int j = lane; j < n; j += 64) below += at(j) < thr ? 1 : 0;
    below = bcast_from(wave_incl_scan(below), 63);

    const int k1 = (n - 1) / 2, k2 = n / 2;
    u64 ka, kb;
    wave_select2(n, k1, k2, hist, lane, [&](int j) { return (u64)__double_as_longlong(at(j)); }, ka, kb);
    const double med = median_of(ka, kb, k1 != k2);
    wave_select2(n, k1, k2, hist, lane, [&](int j) { return (u64)__double_as_longlong(fabs(at(j) - med)); }, ka, kb);
    const double mad = median_of(ka, kb, k1 != k2);
    if (lane == 0) {
        sk_bg_rec b;
        b.mean = mean; b.std = sd; b.median = med; b.mad = mad; b.below = below; b.n = h.n;
        b.reserved[0] = b.reserved[1] = 0;
        out[r] = b;
    }
}

} // namespace

static_assert(sizeof(sk_bg_rec) == 48, "sk_bg_rec is 48 bytes (include/squigglekit_hip.h)");

int sk_launch_row_background(sk_ctx *c, const double *rowD, int64_t row_stride, const sk_hit *rec, int32_t nreads,
                             sk_bg_rec *out)
{
    if (nreads <= 0) return SK_OK;
    const dim3 grid(nreads), block(64);
    if (row_stride <= BG_LDS_COLS) {
        const size_t lds = (size_t)row_stride * sizeof(double);
        if (lds + BG_STATIC_LDS > 64 * 1024)
            SK_HIP(hipFuncSetAttribute((const void *)k_row_background<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_row_background<true>, grid, block, lds, c->stream, rowD, row_stride, rec, nreads, out);
    } else {
        hipLaunchKernelGGL(k_row_background<false>, grid, block, 0, c->stream, rowD, row_stride, rec, nreads, out);
    }
    SK_HIP(hipGetLastError());
    return SK_OK;
}
