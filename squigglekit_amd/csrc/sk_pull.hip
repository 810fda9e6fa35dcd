// sk_pull.hip -- SquigglePull's text output made on the device (SquigglePull.py:178-179, 211-212, 238-253).
//
// Per read r the line is  prefix[r] + tok(s0) + '\t' + tok(s1) + ... + tok(s_{n-1}) + '\n'  (an empty read: prefix +
// '\n'); the prefix (file name, read id, the -i columns, trailing tab) comes from the host.
//   raw mode: tok(d) = str(int(d)).
//   pA mode : t = (double)d + offset; t = t * raw_unit; t = t * 100.0; k = rint(t)   -- np.round((d + offset) *
//             raw_unit, 2) as numpy evaluates it (multiply by 10**2, round half to even, divide) -- and tok = str of the
//             float64 k / 100.0.  For |k| < 1e15 that string is the decimal of the integer k with two decimals and the
//             trailing zero dropped (at least one decimal kept): k / 100 is the double nearest that decimal, and no
//             shorter decimal lies as near.  A negative zero from rint (-0.5 <= t <= -0.0) prints as "-0.0".
//             Every operation is one correctly rounded IEEE operation (the Makefile's -ffp-contract=off: no FMA).
//
// The samples go in tiles of PULL_T = 64 lanes x PULL_S samples; a read of n samples has ceil(n / PULL_T) tiles.
//   1. k_pull_ntiles : tiles per read                      -> exclusive scan: tile0[r]
//   2. k_pull_count  : bytes per tile (tokens + separators) -> exclusive scan: tb[g]
//   3. k_pull_lines  : bytes per line                       -> exclusive scan: the line offsets (the caller's)
//   4. k_pull_write  : one wave per tile formats its tokens into LDS at the tile's output alignment, then stores the
//                      aligned middle with 16-byte vector stores (only the head and tail bytes go one by one);
//      k_pull_prefix : one wave per read copies the prefix (and the '\n' of an empty read).
// Tiles are taken by a fixed grid of waves (the tile count stays on the device); a tile finds its read by a binary
// search over tile0.
#include "sk_common.h"

#define PULL_S 4                       // samples per lane and tile
#define PULL_T (SK_WAVE * PULL_S)      // samples per tile
#define PULL_TOK_MAX 18                // "-" + 13 digits + "." + 2 decimals + separator (|k| < 1e15)
#define PULL_LDS (PULL_T * PULL_TOK_MAX + 16)
#define PULL_K_LIMIT 1e15              // |k| at or past this (or not finite): SK_ERR_UNSUPPORTED
#define SCAN_THREADS 256
#define SCAN_ITEMS 16
#define SCAN_BLOCK (SCAN_THREADS * SCAN_ITEMS)

namespace {

// ---------------------------------------------------------------- int64 exclusive scan over many workgroups
__device__ __forceinline__ int64_t wave_incl_scan(int64_t v)
{
    const int lane = threadIdx.x & (SK_WAVE - 1);
#pragma unroll
    for (int d = 1; d < SK_WAVE; d <<= 1) {
        const int64_t o = __shfl_up(v, d, SK_WAVE);
        if (lane >= d) v += o;
    }
    return v;
}

// inclusive scan over the block (blockDim.x = SCAN_THREADS); *total = the block's sum
__device__ int64_t block_incl_scan(int64_t v, int64_t *sh, int64_t *total)
{
    const int lane = threadIdx.x & (SK_WAVE - 1), w = threadIdx.x / SK_WAVE;
    v = wave_incl_scan(v);
    if (lane == SK_WAVE - 1) sh[w] = v;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int i = 0; i < SCAN_THREADS / SK_WAVE; i++) {
        if (i < w) before += sh[i];
        all += sh[i];
    }
    __syncthreads();
    *total = all;
    return v + before;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_up(const int64_t *__restrict__ v, int64_t n, int64_t *__restrict__ bsum)
{
    __shared__ int64_t sh[SCAN_THREADS / SK_WAVE];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++)
        if (base + i < n) s += v[base + i];
    int64_t total;
    block_incl_scan(s, sh, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the nb block sums in place
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_top(int64_t *__restrict__ bsum, int64_t nb)
{
    __shared__ int64_t sh[SCAN_THREADS / SK_WAVE];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t x = i < nb ? bsum[i] : 0;
        int64_t total;
        const int64_t inc = block_incl_scan(x, sh, &total);
        if (i < nb) bsum[i] = carry + inc - x;
        carry += total;
    }
}

// out[i] = sum of v[0 .. i) for i in [0, n]; out may be v (each workgroup reads its items before it writes them)
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_down(const int64_t *v, int64_t n, const int64_t *__restrict__ bsum,
                                                            int64_t *out)
{
    __shared__ int64_t sh[SCAN_THREADS / SK_WAVE];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t x[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        x[i] = base + i < n ? v[base + i] : 0;
        s += x[i];
    }
    int64_t total;
    int64_t run = bsum[blockIdx.x] + block_incl_scan(s, sh, &total) - s;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        if (base + i < n) out[base + i] = run;
        run += x[i];
    }
    if (base < n && base + SCAN_ITEMS >= n) out[n] = run;     // the thread holding the last item: the total
}

// ---------------------------------------------------------------- per-read geometry
__device__ __forceinline__ int32_t read_len(const int32_t *len, int32_t r, int64_t stride)
{
    int64_t n = len[r];
    if (n < 0) n = 0;
    if (n > stride) n = stride;
    return (int32_t)n;
}

__device__ __forceinline__ int64_t prefix_len(const int64_t *poff, int32_t r)
{
    const int64_t p = poff[r + 1] - poff[r];
    return p > 0 ? p : 0;
}

// the read that tile g belongs to: the largest r with tile0[r] <= g (tile0[nreads] > g)
__device__ __forceinline__ int32_t tile_read(const int64_t *tile0, int32_t nreads, int64_t g)
{
    int32_t lo = 0, hi = nreads;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi + 1) >> 1);
        if (tile0[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void k_pull_ntiles(const int32_t *__restrict__ len, int32_t nreads, int64_t stride, int64_t *__restrict__ nt)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (int64_t)gridDim.x * blockDim.x)
        nt[r] = (read_len(len, (int32_t)r, stride) + PULL_T - 1) / PULL_T;
}

// ---------------------------------------------------------------- one token
struct tok {
    uint64_t u;      // |value| (pA: |k|, centi-units)
    int32_t  neg;    // a leading '-'
    int32_t  len;    // characters, separator not counted
};

__device__ __forceinline__ int ndigits(uint64_t u)
{
    int d = 1;
    uint64_t p = 10;
#pragma unroll 1
    while (d < 20 && u >= p) { d++; p *= 10; }
    return d;
}

// |k| of an integer-valued double with |k| < 2^53, from its bits (integer operations only: the compiler's own
// double -> uint64 conversion goes through an FMA)
__device__ __forceinline__ uint64_t int_of(double k)
{
    const uint64_t b = (uint64_t)__double_as_longlong(k);
    const int e = (int)((b >> 52) & 0x7ff);
    if (e < 1023) return 0;                                 // |k| < 1: zero (k is integer-valued)
    const uint64_t m = (b & 0xfffffffffffffull) | (1ull << 52);
    return m >> (1075 - e);                                  // e <= 1075 for |k| < 2^53: no bits below the point
}

// pA: k = rint(((d + offset) * raw_unit) * 100); *bad set when |k| >= PULL_K_LIMIT or not finite
template <bool PA>
__device__ __forceinline__ tok make_tok(int16_t d, double ofs, double unit, int *bad)
{
    tok t;
    if (PA) {
        double x = sk_raw_to_pa((double)d, ofs, unit);
        x = x * 100.0;
        const double k = rint(x);
        if (!(fabs(k) < PULL_K_LIMIT)) { *bad = 1; t.u = 0; t.neg = 0; t.len = 3; return t; }
        t.neg = signbit(k) ? 1 : 0;
        t.u = int_of(k);
        const uint64_t ip = t.u / 100, fp = t.u - ip * 100;
        t.len = t.neg + ndigits(ip) + 1 + ((fp % 10) ? 2 : 1);
    } else {
        t.neg = d < 0;
        t.u = (uint64_t)(d < 0 ? -(int32_t)d : (int32_t)d);
        t.len = t.neg + ndigits(t.u);
    }
    return t;
}

// digits of u, right to left, ending just before `end`; returns the new end
__device__ __forceinline__ int put_digits(unsigned char *b, int end, uint64_t u)
{
    if (u < 0x100000000ull) {                       // the usual case: 32-bit division by 10 (a multiply-high)
        uint32_t v = (uint32_t)u;
        do { const uint32_t q = v / 10u; b[--end] = (unsigned char)('0' + (v - q * 10u)); v = q; } while (v);
    } else {
        do { const uint64_t q = u / 10u; b[--end] = (unsigned char)('0' + (u - q * 10u)); u = q; } while (u);
    }
    return end;
}

template <bool PA>
__device__ __forceinline__ void write_tok(unsigned char *b, int pos, const tok &t)
{
    int end = pos + t.len;
    if (PA) {
        const uint64_t ip = t.u / 100;
        const uint32_t fp = (uint32_t)(t.u - ip * 100);
        if (fp % 10u) { b[--end] = (unsigned char)('0' + fp % 10u); b[--end] = (unsigned char)('0' + fp / 10u); }
        else b[--end] = (unsigned char)('0' + fp / 10u);
        b[--end] = '.';
        end = put_digits(b, end, ip);
    } else {
        end = put_digits(b, end, t.u);
    }
    if (t.neg) b[pos] = '-';
}

// ---------------------------------------------------------------- pass 1: bytes per tile
template <bool PA>
__global__ void __launch_bounds__(SK_WAVE) k_pull_count(const int16_t *__restrict__ sig, int64_t stride,
                                                        const int32_t *__restrict__ len, int32_t nreads,
                                                        const double *__restrict__ cal, const int64_t *__restrict__ tile0,
                                                        int64_t ntiles_cap, int64_t *__restrict__ tb, int32_t *__restrict__ err)
{
    const int64_t ntiles = tile0[nreads];
    const int lane = threadIdx.x;
    int bad = 0;
    for (int64_t g = blockIdx.x; g < ntiles_cap; g += gridDim.x) {
        if (g >= ntiles) {                           // the scan runs over the capacity: zeros past the last tile
            if (lane == 0) tb[g] = 0;
            continue;
        }
        const int32_t r = tile_read(tile0, nreads, g);
        const int32_t n = read_len(len, r, stride);
        const int64_t i0 = (g - tile0[r]) * PULL_T + (int64_t)lane * PULL_S;
        const int16_t *row = sig + (int64_t)r * stride;
        double ofs = 0.0, unit = 0.0;
        if (PA) { ofs = cal[2 * (int64_t)r]; unit = cal[2 * (int64_t)r + 1]; }
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < PULL_S; i++)
            if (i0 + i < n) s += make_tok<PA>(row[i0 + i], ofs, unit, &bad).len + 1;
#pragma unroll
        for (int d = SK_WAVE / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, SK_WAVE);
        if (lane == 0) tb[g] = s;
    }
    if (bad) atomicOr(err, 1);
}

// line bytes: prefix + the read's tile bytes (tokens, tabs and its '\n') + 1 for the '\n' of an empty read
__global__ void k_pull_lines(const int32_t *__restrict__ len, int32_t nreads, int64_t stride, const int64_t *__restrict__ poff,
                             const int64_t *__restrict__ tile0, const int64_t *__restrict__ tbx, int64_t *__restrict__ lines)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t n = read_len(len, (int32_t)r, stride);
        lines[r] = prefix_len(poff, (int32_t)r) + (tbx[tile0[r + 1]] - tbx[tile0[r]]) + (n == 0 ? 1 : 0);
    }
}

// ---------------------------------------------------------------- pass 2: the text
template <bool PA>
__global__ void __launch_bounds__(SK_WAVE) k_pull_write(const int16_t *__restrict__ sig, int64_t stride,
                                                        const int32_t *__restrict__ len, int32_t nreads,
                                                        const double *__restrict__ cal, const int64_t *__restrict__ poff,
                                                        const int64_t *__restrict__ tile0, const int64_t *__restrict__ tbx,
                                                        const int64_t *__restrict__ line_off, char *__restrict__ out)
{
    __shared__ uint4 lds4[(PULL_LDS + 15) / 16];
    unsigned char *lds = (unsigned char *)lds4;
    const int64_t ntiles = tile0[nreads];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ntiles; g += gridDim.x) {
        const int32_t r = tile_read(tile0, nreads, g);
        const int32_t n = read_len(len, r, stride);
        const int64_t i0 = (g - tile0[r]) * PULL_T + (int64_t)lane * PULL_S;
        const int16_t *row = sig + (int64_t)r * stride;
        double ofs = 0.0, unit = 0.0;
        if (PA) { ofs = cal[2 * (int64_t)r]; unit = cal[2 * (int64_t)r + 1]; }
        int bad = 0;
        tok t[PULL_S];
        int mine = 0;
#pragma unroll
        for (int i = 0; i < PULL_S; i++) {
            t[i] = make_tok<PA>(i0 + i < n ? row[i0 + i] : (int16_t)0, ofs, unit, &bad);
            if (i0 + i < n) mine += t[i].len + 1;
        }
        const int incl = (int)wave_incl_scan(mine);
        const int tile_bytes = __shfl(incl, SK_WAVE - 1, SK_WAVE);
        const int64_t dst = line_off[r] + prefix_len(poff, r) + (tbx[g] - tbx[tile0[r]]);
        const int base = (int)(dst & 15);            // the tile sits in LDS at the alignment it has in `out`
        int pos = base + incl - mine;
        __syncthreads();                             // (the previous tile's bytes have left the LDS)
#pragma unroll
        for (int i = 0; i < PULL_S; i++) {
            if (i0 + i < n) {
                write_tok<PA>(lds, pos, t[i]);
                pos += t[i].len;
                lds[pos++] = (i0 + i == (int64_t)n - 1) ? '\n' : '\t';
            }
        }
        __syncthreads();
        // out[dst .. dst + tile_bytes): narrow head up to the first 16-byte boundary, 16-byte body, narrow tail
        const int64_t end = dst + tile_bytes;
        int64_t a0 = (dst + 15) & ~(int64_t)15, a1 = end & ~(int64_t)15;
        if (a0 > a1) a0 = a1 = end;
        if (lane < a0 - dst) out[dst + lane] = (char)lds[base + lane];
        if (lane < end - a1) out[a1 + lane] = (char)lds[base + (a1 - dst) + lane];
        const int64_t nv = (a1 - a0) >> 4;
        const uint4 *src = lds4 + ((base + (a0 - dst)) >> 4);
        uint4 *dv = (uint4 *)(out + a0);
        for (int64_t v = lane; v < nv; v += SK_WAVE) dv[v] = src[v];
    }
}

// prefix[r] to the start of line r (and the '\n' of an empty read)
__global__ void __launch_bounds__(SK_WAVE) k_pull_prefix(const int32_t *__restrict__ len, int32_t nreads, int64_t stride,
                                                         const char *__restrict__ prefix, const int64_t *__restrict__ poff,
                                                         const int64_t *__restrict__ line_off, char *__restrict__ out)
{
    for (int64_t r = blockIdx.x; r < nreads; r += gridDim.x) {
        const int64_t p = prefix_len(poff, (int32_t)r), o = line_off[r];
        const char *src = prefix + poff[r];
        for (int64_t i = threadIdx.x; i < p; i += SK_WAVE) out[o + i] = src[i];
        if (threadIdx.x == 0 && read_len(len, (int32_t)r, stride) == 0) out[o + p] = '\n';
    }
}

} // namespace

// exclusive scan of v[0 .. n) into out[0 .. n] (out may be v, which then needs n + 1 entries); bsum: scratch of
// sk_scan_blocks(n) entries
int64_t sk_scan_blocks(int64_t n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK + 1; }

int sk_launch_scan_i64(sk_ctx *c, const int64_t *v, int64_t n, int64_t *bsum, int64_t *out)
{
    const int64_t nb = n > 0 ? (n + SCAN_BLOCK - 1) / SCAN_BLOCK : 0;
    if (nb == 0) {
        SK_HIP(hipMemsetAsync(out, 0, sizeof(int64_t), c->stream));
        return SK_OK;
    }
    if (nb > 0x7fffffff) return sk_fail(SK_ERR_INVALID, "scan of %lld items is too long", (long long)n);
    hipLaunchKernelGGL(k_scan_up, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, c->stream, v, n, bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_THREADS), 0, c->stream, bsum, nb);
    hipLaunchKernelGGL(k_scan_down, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, c->stream, v, n, (const int64_t *)bsum, out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int64_t sk_pull_tile_cap(int32_t nreads, int64_t stride) { return (int64_t)nreads * ((stride + PULL_T - 1) / PULL_T); }

// Scratch (device, int64): nt (nreads + 1), tb (tile_cap + 1), lines (nreads + 1 -- may be line_off itself), bsum
int sk_launch_pull_count(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const double *d_cal, const int64_t *d_poff, int64_t *d_tile0, int64_t *d_tb, int64_t tile_cap,
                         int64_t *d_bsum, int64_t *d_line_off, int32_t *d_err)
{
    int rc;
    const int grid_r = (int)((nreads + 255) / 256 < 4096 ? (nreads + 255) / 256 : 4096);
    const int waves = c->num_cu > 0 ? c->num_cu * 16 : 4096;
    if (nreads > 0) hipLaunchKernelGGL(k_pull_ntiles, dim3(grid_r), dim3(256), 0, c->stream, d_len, nreads, stride, d_tile0);
    if ((rc = sk_launch_scan_i64(c, d_tile0, nreads, d_bsum, d_tile0))) return rc;
    if (tile_cap > 0) {
        const int grid_t = (int)(tile_cap < waves ? tile_cap : waves);
        if (d_cal)
            hipLaunchKernelGGL(k_pull_count<true>, dim3(grid_t), dim3(SK_WAVE), 0, c->stream, d_sig, stride, d_len, nreads,
                               d_cal, (const int64_t *)d_tile0, tile_cap, d_tb, d_err);
        else
            hipLaunchKernelGGL(k_pull_count<false>, dim3(grid_t), dim3(SK_WAVE), 0, c->stream, d_sig, stride, d_len, nreads,
                               d_cal, (const int64_t *)d_tile0, tile_cap, d_tb, d_err);
    }
    if ((rc = sk_launch_scan_i64(c, d_tb, tile_cap, d_bsum, d_tb))) return rc;
    if (nreads > 0)
        hipLaunchKernelGGL(k_pull_lines, dim3(grid_r), dim3(256), 0, c->stream, d_len, nreads, stride, d_poff,
                           (const int64_t *)d_tile0, (const int64_t *)d_tb, d_line_off);
    if ((rc = sk_launch_scan_i64(c, d_line_off, nreads, d_bsum, d_line_off))) return rc;
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_launch_pull_write(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                         const double *d_cal, const char *d_prefix, const int64_t *d_poff, const int64_t *d_tile0,
                         const int64_t *d_tb, int64_t tile_cap, const int64_t *d_line_off, char *d_out)
{
    if (nreads <= 0) return SK_OK;
    const int waves = c->num_cu > 0 ? c->num_cu * 16 : 4096;
    if (tile_cap > 0) {
        const int grid_t = (int)(tile_cap < waves ? tile_cap : waves);
        if (d_cal)
            hipLaunchKernelGGL(k_pull_write<true>, dim3(grid_t), dim3(SK_WAVE), 0, c->stream, d_sig, stride, d_len, nreads,
                               d_cal, d_poff, d_tile0, d_tb, d_line_off, d_out);
        else
            hipLaunchKernelGGL(k_pull_write<false>, dim3(grid_t), dim3(SK_WAVE), 0, c->stream, d_sig, stride, d_len, nreads,
                               d_cal, d_poff, d_tile0, d_tb, d_line_off, d_out);
    }
    const int grid_p = nreads < waves ? nreads : waves;
    hipLaunchKernelGGL(k_pull_prefix, dim3(grid_p), dim3(SK_WAVE), 0, c->stream, d_len, nreads, stride, d_prefix, d_poff,
                       d_line_off, d_out);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
