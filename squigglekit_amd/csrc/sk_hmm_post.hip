// sk_hmm_post.hip -- signal HMM posteriors: forward-backward in the log domain, soft counts and dense posteriors, for gfx950.
//
// The definition is the project's own (include/squigglekit_hip.h, "signal HMM: posteriors"; DESIGN.md 4.24;
// tests/hmm_post_ref.py restates it in numpy).  Model, samples, calibration, limit and the emission e_j(x) are those of
// the Viterbi pass (sk_hmm_dev.h), unchanged.  The sums of probabilities need exp and log; both are stated as short, fixed
// sequences of correctly rounded float64 operations (sk_exp, sk_log in sk_hmm_dev.h -- add, multiply, one IEEE division,
// rint, ldexp; the file is compiled with -ffp-contract=off like the rest), so a numpy statement of the same operations in
// the same order gives the same bits.  sk_exp, sk_log, post_lse and the forward step post_fwd_step live in sk_hmm_dev.h:
// a filtered HMM session (sk_hmmstream.hip) carries alpha from push to push with the same text.
//
// One lane per read, 64 reads per wavefront, one wavefront per workgroup -- k_hmm_viterbi's mapping, tiles and feeds --
// so every sum of a read is sequential in t, which is what the definition asks.  Alpha cannot be kept for every sample
// (48 bytes each), so it is kept at every B-th sample and recomputed block by block:
//   k_hmm_fwd<FEED>          alpha in six registers; alpha(b * B) -> ck [group][b][state][lane]; L = lse_j alpha_j(n - 1) -> L.
//   k_hmm_bwd<FEED, COUNTS>  walks the blocks of B samples from the last to the first.  Per block: alpha from the block's
//                            checkpoint, sample by sample into the wavefront's slab [t][state][lane] (the same step text as
//                            the forward kernel: the same bits), then the block backwards -- beta, gamma, xi and the
//                            accumulators, in registers.  w_j = e_j(x_t) + beta_j(t) is carried from t to t - 1, so the
//                            sweep reads sample t only.  A lane reads from the slab what it wrote itself.
// Nothing depends on B (SK_HMM_POST_BLOCK, a multiple of 128 so that blocks start at tile seams of both feeds).
// A transition of -inf is skipped by a scalar branch on tmask -- exact: such a candidate is never strictly greater than the
// maximum in hand, and where the maximum is finite it would add sk_exp(-inf) = 0.0, which changes no sum; its xi stays
// 0.0.  States at and above S are skipped the same way.
//
// No NaN is written: alpha, beta and L are finite or -inf (valid input gives no +inf, as in the Viterbi pass); lse returns
// -inf without forming -inf - -inf; a read with L = -inf is answered with zeros and its sweep runs on L = 0.0 with every
// result dropped; sk_exp sees finite arguments or -inf and returns 0.0 for the latter.
//
// Scratch per 64-read group: 512 bytes of L, 3 072 bytes per checkpoint, 3 072 * B bytes of slab (393 216 at B = 128).  A
// call is worked through in slices of whole groups within SK_HMM_SCRATCH_MB (16 GiB by default).
#include "sk_hmm_dev.h"

namespace {

// The constants of the definition (the head of the file; include/squigglekit_hip.h, tests/hmm_post_ref.py) against the ones
// sk_exp and sk_log of sk_hmm_dev.h run on: bit pattern for bit pattern, checked where the one-shot kernels are compiled.
static_assert(SK_LOG2E == 0x3FF71547652B82FEull && SK_LN2_HI == 0x3FE62E42FEE00000ull && SK_LN2_LO == 0x3DEA39EF35793C76ull,
              "sk_exp: LOG2E, LN2_HI, LN2_LO");
static_assert(SK_SQRT2 == 0x3FF6A09E667F3BCDull && SK_LN2 == 0x3FE62E42FEFA39EFull, "sk_log: SQRT2, LN2");
static_assert(SK_EXP_C0 == 0x3FF0000000000000ull && SK_EXP_C1 == 0x3FF0000000000000ull && SK_EXP_C2 == 0x3FE0000000000000ull,
              "sk_exp: the doubles nearest 1 / q!");
static_assert(SK_EXP_C3 == 0x3FC5555555555555ull && SK_EXP_C4 == 0x3FA5555555555555ull && SK_EXP_C5 == 0x3F81111111111111ull,
              "sk_exp: the doubles nearest 1 / q!");
static_assert(SK_EXP_C6 == 0x3F56C16C16C16C17ull && SK_EXP_C7 == 0x3F2A01A01A01A01Aull && SK_EXP_C8 == 0x3EFA01A01A01A01Aull,
              "sk_exp: the doubles nearest 1 / q!");
static_assert(SK_EXP_C9 == 0x3EC71DE3A556C734ull && SK_EXP_C10 == 0x3E927E4FB7789F5Cull && SK_EXP_C11 == 0x3E5AE64567F544E4ull,
              "sk_exp: the doubles nearest 1 / q!");
static_assert(SK_EXP_C12 == 0x3E21EED8EFF8D898ull && SK_EXP_C13 == 0x3DE6124613A86D09ull,
              "sk_exp: the doubles nearest 1 / q!");
static_assert(SK_LOG_D1 == 0x3FF0000000000000ull && SK_LOG_D3 == 0x3FD5555555555555ull && SK_LOG_D5 == 0x3FC999999999999Aull,
              "sk_log: the doubles nearest 1 / q, q odd");
static_assert(SK_LOG_D7 == 0x3FC2492492492492ull && SK_LOG_D9 == 0x3FBC71C71C71C71Cull && SK_LOG_D11 == 0x3FB745D1745D1746ull,
              "sk_log: the doubles nearest 1 / q, q odd");
static_assert(SK_LOG_D13 == 0x3FB3B13B13B13B14ull && SK_LOG_D15 == 0x3FB1111111111111ull && SK_LOG_D17 == 0x3FAE1E1E1E1E1E1Eull,
              "sk_log: the doubles nearest 1 / q, q odd");
static_assert(SK_LOG_D19 == 0x3FAAF286BCA1AF28ull && SK_LOG_D21 == 0x3FA8618618618618ull && SK_LOG_D23 == 0x3FA642C8590B2164ull,
              "sk_log: the doubles nearest 1 / q, q odd");

struct post_kargs {
    const void    *sig;           // int16 rows of `stride`, or float64 values
    int64_t        stride;
    const int32_t *len;           // int16 rows
    const int64_t *off;           // float64 values: read r = sig[off[r] .. off[r + 1])
    const double  *cal;           // {offset, unit} per read, or nullptr
    int32_t        nreads;
    int32_t        limit;
    int32_t        vec;           // int16 rows are 16-byte aligned (base and stride)
    int32_t        B;             // samples per block (a multiple of 128)
    int64_t        nblk;          // checkpoints per group: no read of the launch has more blocks
    double        *L;             // [group][lane]
    double        *ck;            // [group][block][state][lane]: alpha(block * B)
    double        *slab;          // [group][t - block * B][state][lane]
    sk_hmm_post   *post;
    sk_hmm_counts *counts;        // nullptr: none wanted (COUNTS false)
    const int64_t *goff;          // with gamma: the rows of read r start at gamma + goff[r] * 6
    double        *gamma;
    hmm_kmodel     m;
};

template <int FEED>
__device__ __forceinline__ int32_t post_len(const post_kargs &a, int64_t r)
{
    if (r >= a.nreads) return 0;
    int64_t n;
    if (FEED == SK_FEED_I16) {
        n = a.len[r];
        if (n > a.stride) n = a.stride;
    } else {
        n = a.off[r + 1] - a.off[r];
    }
    if (n > 0x7fffff00) n = 0x7fffff00;
    if (n < 0) n = 0;
    if (a.limit > 0 && n > a.limit) n = a.limit;
    return (int32_t)n;
}

template <int FEED>
__global__ __launch_bounds__(64)
void k_hmm_fwd(const post_kargs a)
{
    typedef typename hmm_feed<FEED>::T T;
    constexpr int TILE = hmm_feed<FEED>::TILE, PITCH = hmm_feed<FEED>::PITCH;
    __shared__ __attribute__((aligned(16))) uint32_t tile[64 * PITCH];
    __shared__ int32_t nrow[64];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int64_t r = r0 + lane;
    const int32_t n = post_len<FEED>(a, r);
    nrow[lane] = n;
    int32_t nmax = n;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    __syncthreads();

    const int S = a.m.S;
    const double ninf = -__builtin_inf();
    double ofs = 0.0, unit = 1.0;                               // (x + 0.0) * 1.0 == x for every int16 x
    if (FEED == SK_FEED_I16 && a.cal && r < a.nreads) { ofs = a.cal[2 * r]; unit = a.cal[2 * r + 1]; }
    double al[HS];
#pragma unroll
    for (int j = 0; j < HS; j++) al[j] = ninf;
    double *ck = a.ck + (size_t)blockIdx.x * (size_t)a.nblk * (HS * 64) + lane;

    const T *xrow = (const T *)tile + (size_t)lane * (PITCH * 4 / sizeof(T));
    const int ntiles = (nmax + TILE - 1) / TILE;
    for (int k = 0; k < ntiles; k++) {
        hmm_load_tile<FEED>(a.sig, a.stride, a.off, a.vec, tile, nrow, r0, k, lane);
        __syncthreads();
        const int32_t t0 = k * TILE;
        const int32_t tend = nmax - t0 < TILE ? nmax - t0 : TILE;   // wave uniform
        for (int jj = 0; jj < tend; jj++) {
            const int32_t t = t0 + jj;                          // wave uniform
            if (t < n) {
                double x = (double)xrow[jj];
                if (FEED == SK_FEED_I16) x = sk_raw_to_pa(x, ofs, unit);
                if (t == 0) {
#pragma unroll
                    for (int j = 0; j < HS; j++)
                        if (j < S) al[j] = a.m.linit[j] + hmm_emit(a.m, j, x);
                } else {
                    post_fwd_step(a.m, S, x, al);
                }
                if (t % a.B == 0) {                             // t / B < ceil(n / B) <= nblk: inside the group's checkpoints
                    double *o = ck + (size_t)(t / a.B) * (HS * 64);
#pragma unroll
                    for (int j = 0; j < HS; j++)
                        if (j < S) o[j * 64] = al[j];
                }
            }
        }
        __syncthreads();                                        // the tile is read before the next one lands
    }
    a.L[r0 + lane] = n > 0 ? post_lse(al, (1u << S) - 1u) : 0.0;   // (L has a slot for every lane of the group)
}

template <int FEED, bool COUNTS>
__global__ __launch_bounds__(64)
void k_hmm_bwd(const post_kargs a)
{
    typedef typename hmm_feed<FEED>::T T;
    constexpr int TILE = hmm_feed<FEED>::TILE, PITCH = hmm_feed<FEED>::PITCH;
    __shared__ __attribute__((aligned(16))) uint32_t tile[64 * PITCH];
    __shared__ int32_t nrow[64];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int64_t r = r0 + lane;
    const int32_t n = post_len<FEED>(a, r);
    nrow[lane] = n;
    int32_t nmax = n;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    __syncthreads();

    const int S = a.m.S;
    const int32_t B = a.B;
    const double ninf = -__builtin_inf();
    double ofs = 0.0, unit = 1.0;
    if (FEED == SK_FEED_I16 && a.cal && r < a.nreads) { ofs = a.cal[2 * r]; unit = a.cal[2 * r + 1]; }
    const double Lr = a.L[r0 + lane];
    const bool live = Lr != ninf;                               // false: the model gives this read probability 0
    const double L = live ? Lr : 0.0;
    double *gam = nullptr;
    if (a.gamma && r < a.nreads) gam = a.gamma + (size_t)a.goff[r] * HS;

    double al[HS], w[HS], occ[HS], fpost[HS], ginit[HS];
    double cn[COUNTS ? HS : 1][2], csx[COUNTS ? HS : 1][2], csxx[COUNTS ? HS : 1][2], cxi[COUNTS ? HS : 1][COUNTS ? HS : 1];
#pragma unroll
    for (int j = 0; j < HS; j++) { al[j] = ninf; w[j] = 0.0; occ[j] = 0.0; fpost[j] = 0.0; ginit[j] = 0.0; }
    if constexpr (COUNTS) {
#pragma unroll
        for (int j = 0; j < HS; j++) {
            cn[j][0] = cn[j][1] = csx[j][0] = csx[j][1] = csxx[j][0] = csxx[j][1] = 0.0;
#pragma unroll
            for (int q = 0; q < HS; q++) cxi[j][q] = 0.0;
        }
    }
    const double *ck = a.ck + (size_t)blockIdx.x * (size_t)a.nblk * (HS * 64) + lane;
    double *slab = a.slab + (size_t)blockIdx.x * (size_t)B * (HS * 64) + lane;

    const T *xrow = (const T *)tile + (size_t)lane * (PITCH * 4 / sizeof(T));
    for (int32_t b = (nmax + B - 1) / B - 1; b >= 0; b--) {
        const int32_t t0 = b * B;                               // a multiple of TILE
        const int32_t tend = nmax - t0 < B ? nmax : t0 + B;     // wave uniform
        const int k0 = t0 / TILE, k1 = (tend - 1) / TILE;
        // alpha of the block, from its checkpoint, into the slab
        if (t0 < n) {
#pragma unroll
            for (int j = 0; j < HS; j++)
                if (j < S) al[j] = ck[((size_t)b * HS + j) * 64];
        }
        for (int k = k0; k <= k1; k++) {
            hmm_load_tile<FEED>(a.sig, a.stride, a.off, a.vec, tile, nrow, r0, k, lane);
            __syncthreads();
            const int32_t te = (k + 1) * TILE < tend ? (k + 1) * TILE : tend;
            for (int32_t t = k * TILE; t < te; t++) {
                if (t < n) {
                    if (t > t0) {
                        double x = (double)xrow[t - k * TILE];
                        if (FEED == SK_FEED_I16) x = sk_raw_to_pa(x, ofs, unit);
                        post_fwd_step(a.m, S, x, al);
                    }
                    double *o = slab + (size_t)(t - t0) * (HS * 64);   // t - t0 < B: inside the wavefront's slab
#pragma unroll
                    for (int j = 0; j < HS; j++)
                        if (j < S) o[j * 64] = al[j];
                }
            }
            __syncthreads();
        }
        // the block backwards
        for (int k = k1; k >= k0; k--) {
            hmm_load_tile<FEED>(a.sig, a.stride, a.off, a.vec, tile, nrow, r0, k, lane);
            __syncthreads();
            const int32_t te = (k + 1) * TILE < tend ? (k + 1) * TILE : tend;
            for (int32_t t = te - 1; t >= k * TILE; t--) {
                if (t < n) {
                    const bool last = t == n - 1;
                    double x = (double)xrow[t - k * TILE];
                    if (FEED == SK_FEED_I16) x = sk_raw_to_pa(x, ofs, unit);
                    const double *o = slab + (size_t)(t - t0) * (HS * 64);
#pragma unroll
                    for (int j = 0; j < HS; j++)
                        if (j < S) al[j] = o[j * 64];
                    // beta_i(t) = lse_j u_ij, u_ij = ltrans[i][j] + w_j with w_j = e_j(x_{t+1}) + beta_j(t+1); 0.0 at t = n - 1
                    double be[HS];
#pragma unroll
                    for (int i = 0; i < HS; i++) {
                        be[i] = ninf;
                        if (i < S) {
                            double u[HS];
                            const uint32_t mask = (uint32_t)(a.m.tmask >> (i * HS)) & 63u;
#pragma unroll
                            for (int j = 0; j < HS; j++) {
                                u[j] = ninf;
                                if ((mask >> j) & 1u) u[j] = a.m.ltrans[i * HS + j] + w[j];
                            }
                            const double v = post_lse(u, mask);
                            be[i] = last ? 0.0 : v;
                            if constexpr (COUNTS) {
#pragma unroll
                                for (int j = 0; j < HS; j++)
                                    if ((mask >> j) & 1u) {
                                        const double xi = sk_exp((al[i] + u[j]) - L);
                                        cxi[i][j] = last ? cxi[i][j] : cxi[i][j] + xi;
                                    }
                            }
                        }
                    }
                    double g[HS];
#pragma unroll
                    for (int j = 0; j < HS; j++) {
                        g[j] = 0.0;
                        if (j < S) {
                            g[j] = sk_exp((al[j] + be[j]) - L);
                            occ[j] = occ[j] + g[j];
                            fpost[j] = last ? g[j] : fpost[j];
                            ginit[j] = g[j];                    // (the last one written is t = 0's)
                            const double d0 = x - a.m.mu[2 * j];
                            const double a0 = a.m.c[2 * j] - (d0 * d0) * a.m.h[2 * j];
                            double e = a0;
                            bool m1 = false;
                            if ((a.m.cmask >> j) & 1u) {
                                const double d1 = x - a.m.mu[2 * j + 1];
                                const double a1 = a.m.c[2 * j + 1] - (d1 * d1) * a.m.h[2 * j + 1];
                                m1 = a1 > a0;
                                e = m1 ? a1 : a0;
                            }
                            if constexpr (COUNTS) {
                                const double gx = g[j] * x, gxx = g[j] * (x * x);
                                cn[j][0] = m1 ? cn[j][0] : cn[j][0] + g[j];
                                cn[j][1] = m1 ? cn[j][1] + g[j] : cn[j][1];
                                csx[j][0] = m1 ? csx[j][0] : csx[j][0] + gx;
                                csx[j][1] = m1 ? csx[j][1] + gx : csx[j][1];
                                csxx[j][0] = m1 ? csxx[j][0] : csxx[j][0] + gxx;
                                csxx[j][1] = m1 ? csxx[j][1] + gxx : csxx[j][1];
                            }
                            w[j] = e + be[j];                   // e = e_j(x_t), hmm_emit's operations in its order
                        }
                    }
                    if (gam) {                                  // rows [goff[r], goff[r] + n) are the caller's promise
                        double *q = gam + (size_t)t * HS;
#pragma unroll
                        for (int j = 0; j < HS; j++) q[j] = live ? g[j] : 0.0;
                    }
                }
            }
            __syncthreads();
        }
    }

    if (r >= a.nreads) return;
    const bool keep = live && n > 0;
    sk_hmm_post out;
    out.loglik = Lr;                                            // 0.0 at n == 0
    out.n_used = n;
    out.flags = live ? 0 : SK_HMM_POST_IMPOSSIBLE;
#pragma unroll
    for (int j = 0; j < HS; j++) { out.final_post[j] = keep ? fpost[j] : 0.0; out.occ[j] = keep ? occ[j] : 0.0; }
    a.post[r] = out;
    if constexpr (COUNTS) {
        sk_hmm_counts *cc = a.counts + r;
#pragma unroll
        for (int j = 0; j < HS; j++) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                cc->n[j][q] = keep ? cn[j][q] : 0.0;
                cc->sx[j][q] = keep ? csx[j][q] : 0.0;
                cc->sxx[j][q] = keep ? csxx[j][q] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < HS; q++) cc->xi[j][q] = keep ? cxi[j][q] : 0.0;
            cc->init[j] = keep ? ginit[j] : 0.0;
        }
    }
}

// samples per block: 128, or SK_HMM_POST_BLOCK (a multiple of 128 up to 4 096)
int32_t post_block()
{
    if (const char *e = sk_tune("SK_HMM_POST_BLOCK")) { const long v = atol(e); if (v >= 128 && v <= 4096 && v % 128 == 0) return (int32_t)v; }
    return 128;
}

// bytes of scratch the slices of one call may hold: the state paths' budget (16 GiB, or SK_HMM_SCRATCH_MB)
size_t post_budget()
{
    size_t budget = (size_t)16 << 30;
    if (const char *e = sk_tune("SK_HMM_SCRATCH_MB")) { const long v = atol(e); if (v > 0) budget = (size_t)v << 20; }
    return budget;
}

size_t post_group_bytes(int64_t npad, int32_t B)
{
    const int64_t nblk = (npad + B - 1) / B;
    return (size_t)64 * sizeof(double) + ((size_t)nblk + (size_t)B) * (HS * 64 * sizeof(double));
}

int64_t post_slice_groups(int32_t nreads, int64_t npad, int32_t B)
{
    const int64_t groups = ((int64_t)nreads + 63) / 64;
    int64_t g = (int64_t)(post_budget() / post_group_bytes(npad, B));
    if (g < 1) g = 1;
    return g < groups ? g : groups;
}

} // namespace

static_assert(sizeof(sk_hmm_post) == 112, "sk_hmm_post is 112 bytes (include/squigglekit_hip.h)");
static_assert(sizeof(sk_hmm_counts) == 624, "sk_hmm_counts is 624 bytes (include/squigglekit_hip.h)");

// scratch of a posterior call over nreads reads of at most npad samples (sk_hmm_npad): one slice's L, checkpoints, slabs
size_t sk_hmm_post_work_bytes(int32_t nreads, int64_t npad)
{
    const int32_t B = post_block();
    return (size_t)post_slice_groups(nreads, npad, B) * post_group_bytes(npad, B);
}

// The posteriors of nreads reads, slice by slice: records -> d_post, soft counts -> d_counts (or nullptr), dense rows ->
// d_gamma + d_goff[r] * 6 (or both nullptr).  d_work: sk_hmm_post_work_bytes(nreads, npad) bytes.  feed SK_FEED_I16: d_sig
// rows of `stride`, d_len, d_cal; SK_FEED_F64_NORM: d_sig values, d_roff.
int sk_launch_hmm_post(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int32_t *d_len, const int64_t *d_roff,
                       int32_t nreads, const double *d_cal, const sk_hmm_model *m, int32_t limit, int64_t npad, void *d_work,
                       sk_hmm_post *d_post, sk_hmm_counts *d_counts, const int64_t *d_goff, double *d_gamma)
{
    if (nreads <= 0) return SK_OK;
    post_kargs a;
    a.B = post_block();
    a.nblk = (npad + a.B - 1) / a.B;
    const int64_t G = post_slice_groups(nreads, npad, a.B);
    a.L = (double *)d_work;
    a.ck = a.L + (size_t)G * 64;
    a.slab = a.ck + (size_t)G * (size_t)a.nblk * (HS * 64);
    a.stride = stride; a.limit = limit; a.m = hmm_flatten(m); a.gamma = d_gamma;
    for (int64_t r0 = 0; r0 < nreads; r0 += G * 64) {
        const int32_t nr = (int32_t)(nreads - r0 < G * 64 ? nreads - r0 : G * 64);
        const dim3 grid((unsigned)((nr + 63) / 64)), block(64);
        a.nreads = nr; a.post = d_post + r0; a.counts = d_counts ? d_counts + r0 : nullptr; a.goff = d_goff ? d_goff + r0 : nullptr;
        if (feed == SK_FEED_I16) {
            const int16_t *sig = (const int16_t *)d_sig + (size_t)r0 * (size_t)stride;
            a.sig = sig; a.len = d_len + r0; a.off = nullptr; a.cal = d_cal ? d_cal + 2 * (size_t)r0 : nullptr;
            a.vec = ((uintptr_t)sig % 16 == 0 && stride % 8 == 0) ? 1 : 0;
            hipLaunchKernelGGL(k_hmm_fwd<SK_FEED_I16>, grid, block, 0, c->stream, a);
            if (d_counts) hipLaunchKernelGGL((k_hmm_bwd<SK_FEED_I16, true>), grid, block, 0, c->stream, a);
            else          hipLaunchKernelGGL((k_hmm_bwd<SK_FEED_I16, false>), grid, block, 0, c->stream, a);
        } else {
            a.sig = d_sig; a.len = nullptr; a.off = d_roff + r0; a.cal = nullptr; a.vec = 0;
            hipLaunchKernelGGL(k_hmm_fwd<SK_FEED_F64_NORM>, grid, block, 0, c->stream, a);
            if (d_counts) hipLaunchKernelGGL((k_hmm_bwd<SK_FEED_F64_NORM, true>), grid, block, 0, c->stream, a);
            else          hipLaunchKernelGGL((k_hmm_bwd<SK_FEED_F64_NORM, false>), grid, block, 0, c->stream, a);
        }
        SK_HIP(hipGetLastError());
    }
    return SK_OK;
}
