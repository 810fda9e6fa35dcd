// sk_hmm.hip -- signal HMM: the best path of every read through a model of up to six states, for gfx950.
//
// The definition is the project's own (include/squigglekit_hip.h, "signal HMM"; tests/hmm_ref.py restates
// it in numpy).  Per read x[0..n) and per state j:
//     e_j(x)  = max_m ( c[j][m] - ((x - mu[j][m]) * (x - mu[j][m])) * h[j][m] )          m = 0, 1
//     v_j(0)  = linit[j] + e_j(x_0)
//     v_j(t)  = max_i ( v_i(t-1) + ltrans[i][j] ) + e_j(x_t)                             the lowest i wins ties
// with max(a, b) = (b > a ? b : a), one correctly rounded float64 operation at a time (the file is compiled with
// -ffp-contract=off like the rest) and no log / exp.  Instead of a back-trace every state carries enter[0..6): the first
// sample at which its best path was in state k (-1: never) -- the winning predecessor's tuple is copied forward, as the
// DTW kernels carry their start column.
//
// k_hmm_viterbi<FEED>   one lane per read, 64 reads per wavefront (one wavefront per workgroup), k_detect_mark's mapping.
//     The wavefront loads a tile of its 64 rows into LDS and every lane then walks its own row:
//       int16 rows     tile of 128 samples, 16-byte loads (16 lanes per row; rows that are not 16-byte aligned take 2-byte
//                      loads), pitch 65 dwords: the 2-byte reads of the lanes -- all at the same position of their own
//                      rows -- fall into distinct banks;
//       float64 ragged tile of 32 values, 8-byte loads (32 lanes per row: a ragged row is 8-byte aligned and no more),
//                      pitch 66 dwords: the 8-byte reads of 32 lanes fall into distinct bank pairs.
//     The six scores and the six tuples of six sample indices stay in registers: every loop over states is unrolled, the
//     winning predecessor is chosen by compare-and-select.  The model is a kernel argument, so its constants are wave
//     uniform and the compiler holds them in scalar registers.  A wavefront has 102 of them and the model alone is 78
//     doubles, so 188 scalar values are spilled: parked in lanes of vector registers (v_writelane once, v_readlane at
//     each use inside the sample loop; no scratch, no memory access -- profiles/hmm_kernel_resources.txt).  That costs
//     vector ALU issue slots in a loop bound by them and is not removed yet.  A transition or a second
//     component of -inf is skipped by a scalar branch on a bit mask made on the host -- exact: such a candidate is -inf and
//     never strictly greater than the one in hand (predecessor 0 and component 0 are always taken, so ties at -inf
//     resolve as the definition says).  States at and above S are skipped the same way.  The sample index is the same
//     for all lanes, so t == 0 is a scalar branch too.  A lane whose read has ended idles; the wavefront leaves after
//     the tile that ends its longest read.  Global traffic: the samples once, 40 bytes per read out.
//
// The work per sample is about S^2 compare-and-selects of a tuple: the kernel is bound by vector ALU issue, not by
// memory, which is why one tile (no ring) and two barriers per tile are enough.  A call of a few hundred reads fills a
// few of the 1 024 SIMDs only: the lane-per-read mapping is for batches.
//
// The second half of the file adds the state paths: the same body instantiated with back pointers, the
// backward sweep and the statistics fill that turn them into segments.
//
// The model as the kernel takes it, the tile loads, the emission and the step without back pointers are in sk_hmm_dev.h:
// the HMM sessions (sk_hmmstream.hip) run the same text on state they carry from push to push.
#include "sk_hmm_dev.h"

namespace {

struct hmm_kargs {
    const void    *sig;           // int16 rows of `stride`, or float64 values
    int64_t        stride;
    const int32_t *len;           // int16 rows
    const int64_t *off;           // float64 values: read r = sig[off[r] .. off[r + 1])
    const double  *cal;           // {offset, unit} per read, or nullptr
    int32_t        nreads;
    int32_t        limit;
    int32_t        vec;           // int16 rows are 16-byte aligned (base and stride)
    sk_hmm_rec    *rec;
    hmm_kmodel     m;
    // the back-pointer instantiation only (k_hmm_viterbi<FEED, true>)
    uint32_t      *bp;            // [group][t][lane]: the six 3-bit arg_j(t) of read 64 * group + lane, npad rows per group
    int64_t        npad;          // rows per group: no read of the launch uses more samples
    int64_t       *cnt;           // segments of the best path, per read
};

template <int FEED>
__device__ __forceinline__ int32_t hmm_len(const hmm_kargs &a, int64_t r)
{
    if (r >= a.nreads) return 0;
    int64_t n;
    if (FEED == SK_FEED_I16) {
        n = a.len[r];
        if (n > a.stride) n = a.stride;
    } else {
        n = a.off[r + 1] - a.off[r];
    }
    if (n > 0x7fffff00) n = 0x7fffff00;                         // either feed: nmax + TILE - 1 stays inside int32
    if (n < 0) n = 0;
    if (a.limit > 0 && n > a.limit) n = a.limit;
    return (int32_t)n;
}

// BP: the instantiation that keeps the back pointers.  It carries, instead of the enter tuples, the winning predecessor
// and the number of segments of the best path into every state: one word of six 3-bit predecessors per sample goes to
// a.bp (the 64 lanes' words of one t are one 256-byte line), the count of the final state to a.cnt, and the record's
// enter[] is left to the backward sweep (k_hmm_back), which reads it off the path.
template <int FEED, bool BP>
__global__ __launch_bounds__(64)
void k_hmm_viterbi(const hmm_kargs a)
{
    typedef typename hmm_feed<FEED>::T T;
    constexpr int TILE = hmm_feed<FEED>::TILE, PITCH = hmm_feed<FEED>::PITCH;
    __shared__ __attribute__((aligned(16))) uint32_t tile[64 * PITCH];
    __shared__ int32_t nrow[64];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int64_t r = r0 + lane;
    const int32_t n = hmm_len<FEED>(a, r);
    nrow[lane] = n;
    int32_t nmax = n;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    __syncthreads();

    const int S = a.m.S;
    const double ninf = -__builtin_inf();
    double ofs = 0.0, unit = 1.0;                               // (x + 0.0) * 1.0 == x for every int16 x
    if (FEED == SK_FEED_I16 && a.cal && r < a.nreads) { ofs = a.cal[2 * r]; unit = a.cal[2 * r + 1]; }

    double v[HS];
    int32_t E[HS][HS];
    int32_t NS[HS];                                             // BP: segments of the best path into state j
#pragma unroll
    for (int j = 0; j < HS; j++) {
        v[j] = ninf;
        NS[j] = 0;
#pragma unroll
        for (int q = 0; q < HS; q++) E[j][q] = -1;
    }
    uint32_t *bprow = nullptr;
    if (BP) bprow = a.bp + (size_t)blockIdx.x * (size_t)a.npad * 64 + lane;

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
                        if (j < S) { v[j] = a.m.linit[j] + hmm_emit(a.m, j, x); E[j][j] = 0; NS[j] = 1; }
                } else if (!BP) {
                    hmm_step(a.m, S, x, t, v, E);
                } else {
                    double nv[HS];
                    int32_t NN[HS];
                    uint32_t argw = 0;
#pragma unroll
                    for (int j = 0; j < HS; j++) {
                        nv[j] = ninf;
                        NN[j] = 0;
                        if (j < S) {
                            double b = v[0] + a.m.ltrans[j];    // predecessor 0: always taken
                            int32_t arg = 0, ns = NS[0];
#pragma unroll
                            for (int i = 1; i < HS; i++)
                                if (i < S && ((a.m.tmask >> (i * HS + j)) & 1ull)) {
                                    const double cand = v[i] + a.m.ltrans[i * HS + j];
                                    const bool w = cand > b;
                                    b = w ? cand : b;
                                    arg = w ? i : arg;
                                    ns = w ? NS[i] : ns;
                                }
                            NN[j] = ns + (arg != j ? 1 : 0);
                            argw |= (uint32_t)arg << (3 * j);
                            nv[j] = b + hmm_emit(a.m, j, x);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < HS; j++) { v[j] = nv[j]; NS[j] = NN[j]; }
                    bprow[(size_t)t * 64] = argw;                // t < n <= npad: inside the group's rows
                }
            }
        }
        __syncthreads();                                        // the tile is read before the next one lands
    }

    if (r >= a.nreads) return;
    sk_hmm_rec out;
    int32_t nseg = 0;
    if (n == 0) {
        out.score = 0.0; out.final_state = -1; out.n_used = 0;
#pragma unroll
        for (int q = 0; q < HS; q++) out.enter[q] = -1;
    } else {
        double best = v[0];
        int32_t f = 0;
        int32_t en[HS];
        nseg = NS[0];
#pragma unroll
        for (int q = 0; q < HS; q++) en[q] = E[0][q];
#pragma unroll
        for (int j = 1; j < HS; j++)
            if (j < S) {
                const bool w = v[j] > best;
                best = w ? v[j] : best;
                f = w ? j : f;
                if (BP) nseg = w ? NS[j] : nseg;
#pragma unroll
                for (int q = 0; q < HS; q++) en[q] = w ? E[j][q] : en[q];
            }
        out.score = best; out.final_state = f; out.n_used = n;
#pragma unroll
        for (int q = 0; q < HS; q++) out.enter[q] = en[q];
    }
    a.rec[r] = out;                                             // BP: enter[] is k_hmm_back's to fill
    if (BP) a.cnt[r] = nseg;
}

} // namespace

static_assert(sizeof(sk_hmm_rec) == 40, "sk_hmm_rec is 40 bytes (include/squigglekit_hip.h)");
static_assert(sizeof(sk_hmm_model) == 632, "sk_hmm_model is 632 bytes (include/squigglekit_hip.h)");

// The rules of the header's "signal HMM" section; nullptr when the model keeps them, else what it breaks.
const char *sk_hmm_model_error(const sk_hmm_model *m)
{
    if (!m) return "NULL sk_hmm_model";
    const int S = m->nstates;
    if (S < 1 || S > HS) return "nstates must lie in [1, 6]";
    const double inf = __builtin_inf();
    bool any = false;
    for (int j = 0; j < S; j++) {
        const double li = m->linit[j];
        if (li != li || li == inf) return "linit must be finite or -inf";
        if (li != -inf) any = true;
        for (int i = 0; i < S; i++) {
            const double lt = m->ltrans[i][j];
            if (lt != lt || lt == inf) return "ltrans must be finite or -inf";
        }
        bool comp = false;
        for (int q = 0; q < 2; q++) {
            const double c = m->c[j][q], mu = m->mu[j][q], h = m->h[j][q];
            if (c != c || c == inf) return "c must be finite or -inf";
            if (c != -inf) comp = true;
            if (!(mu - mu == 0.0)) return "mu must be finite";
            if (!(h - h == 0.0) || h < 0.0) return "h must be finite and >= 0";
        }
        if (!comp) return "every state needs a component with a finite c";
    }
    if (!any) return "at least one linit must be finite";
    return nullptr;
}

// the records of nreads int16 rows (d_cal: {offset, unit} per read or nullptr) -> d_rec[0 .. nreads)
int sk_launch_hmm_i16(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                      const double *d_cal, const sk_hmm_model *m, int32_t limit, sk_hmm_rec *d_rec)
{
    if (nreads <= 0) return SK_OK;
    hmm_kargs a;
    a.sig = d_sig; a.stride = stride; a.len = d_len; a.off = nullptr; a.cal = d_cal; a.nreads = nreads; a.limit = limit;
    a.vec = ((uintptr_t)d_sig % 16 == 0 && stride % 8 == 0) ? 1 : 0;
    a.rec = d_rec; a.m = hmm_flatten(m); a.bp = nullptr; a.npad = 0; a.cnt = nullptr;
    hipLaunchKernelGGL((k_hmm_viterbi<SK_FEED_I16, false>), dim3((unsigned)((nreads + 63) / 64)), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// ... of nreads ragged float64 reads, read r = d_values[d_off[r] .. d_off[r + 1])
int sk_launch_hmm_f64(sk_ctx *c, const double *d_values, const int64_t *d_off, int32_t nreads, const sk_hmm_model *m,
                      int32_t limit, sk_hmm_rec *d_rec)
{
    if (nreads <= 0) return SK_OK;
    hmm_kargs a;
    a.sig = d_values; a.stride = 0; a.len = nullptr; a.off = d_off; a.cal = nullptr; a.nreads = nreads; a.limit = limit;
    a.vec = 0; a.rec = d_rec; a.m = hmm_flatten(m); a.bp = nullptr; a.npad = 0; a.cnt = nullptr;
    hipLaunchKernelGGL((k_hmm_viterbi<SK_FEED_F64_NORM, false>), dim3((unsigned)((nreads + 63) / 64)), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// ------------------------------------------------------------------ state paths: segments of the best path
// The definition: include/squigglekit_hip.h, "signal HMM: state paths" (tests/hmm_path_ref.py).
//
// k_hmm_viterbi<FEED, true>  the forward pass above with one back-pointer word per sample and the segment count per read.
// k_hmm_off      the running scan: the slice's scanned counts + the offset the slices before it reached -> off.
// k_hmm_back     one lane per read, the forward pass's groups of 64.  All lanes step t = nmax - 1 .. 1 together, so the 64
//                words of one t are one 256-byte line again; the address does not depend on the state, the loads are
//                unrolled ahead of the dependent shift-and-mask chain.  Where the state changes, the lane writes state,
//                start and length of the segment that ends -- the k-th from the end at off[r + 1] - 1 - k -- and notes the
//                start as enter[state] (the last such note is the first entry).  Nothing goes to seg when the read's
//                segments end past cap; enter[] is written either way.
// k_hmm_stats    one wavefront per read.  int16: the wavefront shares a segment, lanes take samples start + lane, + 64, ..;
//                exact int64 sums, so the order is free; a shuffle tree adds the lanes.  float64: the rising-t order is
//                part of the definition, so a lane takes a whole segment (lanes = segments off[r] + lane, + 64, ..).
namespace {

static_assert(sizeof(sk_hmm_seg) == 48 && sizeof(sk_hmm_segf) == 48, "sk_hmm_seg / sk_hmm_segf are 48 bytes");

__global__ __launch_bounds__(256)
void k_hmm_off(const int64_t *scanned, int64_t *off, int32_t nreads, int first)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nreads) return;
    if (i == 0) { if (first) off[0] = 0; return; }              // (a later slice starts where the one before ended)
    const int64_t base = first ? 0 : off[0];
    off[i] = base + scanned[i];
}

struct hmm_back_args {
    sk_hmm_rec     *rec;          // the slice's records: n_used and final_state in, enter[] out
    const uint32_t *bp;
    int64_t         npad;
    const int64_t  *off;          // the slice's offsets [nreads + 1], in records of seg
    sk_hmm_seg     *seg;          // the call's records (nullptr: none wanted)
    int64_t         cap;
    int32_t         nreads;
};

__global__ __launch_bounds__(64)
void k_hmm_back(const hmm_back_args a)
{
    const int lane = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * 64 + lane;
    int32_t n = 0, s = 0;
    int64_t pos = 0, lo = 0;
    bool put = false;
    if (r < a.nreads) {
        n = a.rec[r].n_used;
        s = a.rec[r].final_state;
        lo = a.off[r];
        pos = a.off[r + 1] - 1;
        put = a.seg != nullptr && a.off[r + 1] <= a.cap;
    }
    int32_t nmax = n;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    if (nmax == 0) return;
    const uint32_t *row = a.bp + (size_t)blockIdx.x * (size_t)a.npad * 64 + lane;
    int32_t en[HS];
#pragma unroll
    for (int q = 0; q < HS; q++) en[q] = -1;
    int32_t end = n;                                            // one past the last sample of the open segment
#pragma unroll 4
    for (int32_t t = nmax - 1; t >= 1; t--) {
        const uint32_t w = row[(size_t)t * 64];                 // t < nmax <= npad: inside the group's rows (unwritten for t >= n)
        if (t < n) {
            const int32_t p = (int32_t)((w >> (3 * s)) & 7u);
            if (p != s) {
                if (put && pos >= lo) {                         // (the forward pass counted these: pos stays in [lo, off[r + 1]))
                    sk_hmm_seg *o = a.seg + pos;
                    o->state = s; o->start = t; o->length = end - t;
                }
#pragma unroll
                for (int q = 0; q < HS; q++) en[q] = q == s ? t : en[q];
                pos--;
                end = t;
                s = p;
            }
        }
    }
    if (n > 0) {
        if (put && pos >= lo) {
            sk_hmm_seg *o = a.seg + pos;
            o->state = s; o->start = 0; o->length = end;
        }
#pragma unroll
        for (int q = 0; q < HS; q++) en[q] = q == s ? 0 : en[q];
#pragma unroll
        for (int q = 0; q < HS; q++) a.rec[r].enter[q] = en[q];
    }
}

struct hmm_stat_args {
    const void    *sig;
    int64_t        stride;
    const int64_t *roff;          // float64 values: read r starts at sig[roff[r]]
    const double  *cal;
    const int64_t *off;           // [nreads + 1]
    void          *seg;           // sk_hmm_seg (int16 rows) or sk_hmm_segf (float64 values)
    int64_t        cap;
    double         c[HS * 2], mu[HS * 2], h[HS * 2];
};

// the winning component of x in state j: a_1 > a_0, by e_j(x)'s operations in e_j(x)'s order
__device__ __forceinline__ bool hmm_comp1(const double *c, const double *mu, const double *h, int j, double x)
{
    const double d0 = x - mu[2 * j];
    const double a0 = c[2 * j] - (d0 * d0) * h[2 * j];
    const double d1 = x - mu[2 * j + 1];
    const double a1 = c[2 * j + 1] - (d1 * d1) * h[2 * j + 1];
    return a1 > a0;
}

template <int FEED>
__global__ __launch_bounds__(64)
void k_hmm_stats(const hmm_stat_args a)
{
    __shared__ double mc[HS * 2], mm[HS * 2], mh[HS * 2];      // the model, indexed by a state that is data
    const int lane = threadIdx.x;
    if (lane < HS * 2) { mc[lane] = a.c[lane]; mm[lane] = a.mu[lane]; mh[lane] = a.h[lane]; }
    __syncthreads();
    const int64_t r = blockIdx.x;
    const int64_t q0 = a.off[r], q1 = a.off[r + 1];
    if (q1 > a.cap || q1 <= q0) return;
    if (FEED == SK_FEED_I16) {
        const int16_t *x = (const int16_t *)a.sig + r * a.stride;
        sk_hmm_seg *seg = (sk_hmm_seg *)a.seg;
        double ofs = 0.0, unit = 1.0;
        if (a.cal) { ofs = a.cal[2 * r]; unit = a.cal[2 * r + 1]; }
        for (int64_t q = q0; q < q1; q++) {
            const int32_t j = seg[q].state, t0 = seg[q].start, len = seg[q].length;
            long long s0 = 0, s1 = 0, w0 = 0, w1 = 0;
            int32_t n1 = 0;
            for (int32_t i = lane; i < len; i += 64) {
                const long long raw = x[(int64_t)t0 + i];
                const bool m = hmm_comp1(mc, mm, mh, j, sk_raw_to_pa((double)raw, ofs, unit));
                s1 += m ? raw : 0;        s0 += m ? 0 : raw;
                w1 += m ? raw * raw : 0;  w0 += m ? 0 : raw * raw;
                n1 += m ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o);
                w0 += __shfl_xor(w0, o); w1 += __shfl_xor(w1, o);
                n1 += __shfl_xor(n1, o);
            }
            if (lane == 0) {
                seg[q].n1 = n1;
                seg[q].sum[0] = s0; seg[q].sum[1] = s1;
                seg[q].sumsq[0] = w0; seg[q].sumsq[1] = w1;
            }
        }
    } else {
        const double *x = (const double *)a.sig + a.roff[r];
        sk_hmm_segf *seg = (sk_hmm_segf *)a.seg;
        for (int64_t q = q0 + lane; q < q1; q += 64) {
            const int32_t j = seg[q].state, t0 = seg[q].start, len = seg[q].length;
            double s0 = 0.0, s1 = 0.0, w0 = 0.0, w1 = 0.0;
            int32_t n1 = 0;
            for (int32_t i = 0; i < len; i++) {
                const double xv = x[(int64_t)t0 + i];
                const double sq = xv * xv;
                if (hmm_comp1(mc, mm, mh, j, xv)) { s1 += xv; w1 += sq; n1++; }
                else                              { s0 += xv; w0 += sq; }
            }
            seg[q].n1 = n1;
            seg[q].sum[0] = s0; seg[q].sum[1] = s1;
            seg[q].sumsq[0] = w0; seg[q].sumsq[1] = w1;
        }
    }
}

// bytes of back pointers the slices of one call may hold: 16 GiB of the 288, or SK_HMM_SCRATCH_MB.  A slice of the
// throughput workload's rows (stride 30 000: 7.7 MB per group) then holds 2 236 groups, about the 2 304 wavefronts the
// chip keeps resident at nine 17 KB tiles per CU -- one full round; smaller slices would leave SIMDs idle while each
// slice's longest reads finish
size_t hmm_bp_budget()
{
    size_t budget = (size_t)16 << 30;
    if (const char *e = sk_tune("SK_HMM_SCRATCH_MB")) { const long v = atol(e); if (v > 0) budget = (size_t)v << 20; }
    return budget;
}

} // namespace

// the most samples a read of the call can use: the rows of the back-pointer scratch per group
int64_t sk_hmm_npad(int64_t maxlen, int32_t limit)
{
    int64_t n = maxlen;
    if (n > 0x7fffff00) n = 0x7fffff00;
    if (limit > 0 && n > limit) n = limit;
    return n > 1 ? n : 1;
}

// groups of 64 reads per slice, and with them the bytes of sk_ctx::hmmpath: the back pointers of a slice, its counts
// (reads + 1) and the scan's block sums
int64_t sk_hmm_slice_groups(int32_t nreads, int64_t npad)
{
    const int64_t groups = ((int64_t)nreads + 63) / 64;
    int64_t g = (int64_t)(hmm_bp_budget() / ((size_t)npad * 256));
    if (g < 1) g = 1;
    return g < groups ? g : groups;
}

size_t sk_hmm_path_work_bytes(int32_t nreads, int64_t npad)
{
    const int64_t g = sk_hmm_slice_groups(nreads, npad);
    return (size_t)g * (size_t)npad * 256 + ((size_t)g * 64 + 2 + (size_t)sk_scan_blocks(g * 64)) * sizeof(int64_t);
}

// The segments' topology of nreads reads, slice by slice: records (enter[] included) -> d_rec, offsets -> d_off[0 ..
// nreads] continuing from d_off[0] (first != 0: from 0), state / start / length -> d_seg[d_off[r] ..] for every read
// whose segments end at or below cap.  d_work: sk_hmm_path_work_bytes(nreads, npad) bytes.  feed SK_FEED_I16: d_sig rows
// of `stride`, d_len, d_cal; SK_FEED_F64_NORM: d_sig values, d_roff.
int sk_launch_hmm_paths(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int32_t *d_len, const int64_t *d_roff,
                        int32_t nreads, const double *d_cal, const sk_hmm_model *m, int32_t limit, int64_t npad, void *d_work,
                        int first, sk_hmm_rec *d_rec, int64_t *d_off, sk_hmm_seg *d_seg, int64_t cap)
{
    if (nreads <= 0) return SK_OK;
    const int64_t G = sk_hmm_slice_groups(nreads, npad);
    uint32_t *d_bp = (uint32_t *)d_work;
    int64_t *d_cnt = (int64_t *)((char *)d_work + (size_t)G * (size_t)npad * 256);
    int64_t *d_bsum = d_cnt + G * 64 + 2;
    hmm_kargs a;
    a.stride = stride; a.limit = limit; a.m = hmm_flatten(m); a.bp = d_bp; a.npad = npad; a.cnt = d_cnt;
    for (int64_t r0 = 0; r0 < nreads; r0 += G * 64) {
        const int32_t nr = (int32_t)(nreads - r0 < G * 64 ? nreads - r0 : G * 64);
        const unsigned grid = (unsigned)((nr + 63) / 64);
        a.nreads = nr; a.rec = d_rec + r0;
        if (feed == SK_FEED_I16) {
            const int16_t *sig = (const int16_t *)d_sig + (size_t)r0 * (size_t)stride;
            a.sig = sig; a.len = d_len + r0; a.off = nullptr; a.cal = d_cal ? d_cal + 2 * (size_t)r0 : nullptr;
            a.vec = ((uintptr_t)sig % 16 == 0 && stride % 8 == 0) ? 1 : 0;
            hipLaunchKernelGGL((k_hmm_viterbi<SK_FEED_I16, true>), dim3(grid), dim3(64), 0, c->stream, a);
        } else {
            a.sig = d_sig; a.len = nullptr; a.off = d_roff + r0; a.cal = nullptr; a.vec = 0;
            hipLaunchKernelGGL((k_hmm_viterbi<SK_FEED_F64_NORM, true>), dim3(grid), dim3(64), 0, c->stream, a);
        }
        SK_HIP(hipGetLastError());
        int rc = sk_launch_scan_i64(c, d_cnt, nr, d_bsum, d_cnt);
        if (rc) return rc;
        hipLaunchKernelGGL(k_hmm_off, dim3((unsigned)((nr + 256) / 256)), dim3(256), 0, c->stream, (const int64_t *)d_cnt,
                           d_off + r0, nr, (first && r0 == 0) ? 1 : 0);
        hmm_back_args b;
        b.rec = d_rec + r0; b.bp = d_bp; b.npad = npad; b.off = d_off + r0; b.seg = d_seg; b.cap = cap; b.nreads = nr;
        hipLaunchKernelGGL(k_hmm_back, dim3(grid), dim3(64), 0, c->stream, b);
        SK_HIP(hipGetLastError());
    }
    return SK_OK;
}

// n1, sum and sumsq of every segment of nreads reads whose topology is in d_seg (reads whose segments end past cap are
// left alone)
int sk_launch_hmm_stats(sk_ctx *c, int feed, const void *d_sig, int64_t stride, const int64_t *d_roff, int32_t nreads,
                        const double *d_cal, const sk_hmm_model *m, const int64_t *d_off, void *d_seg, int64_t cap)
{
    if (nreads <= 0 || !d_seg || cap <= 0) return SK_OK;
    const hmm_kmodel k = hmm_flatten(m);
    hmm_stat_args a;
    a.sig = d_sig; a.stride = stride; a.roff = d_roff; a.cal = d_cal; a.off = d_off; a.seg = d_seg; a.cap = cap;
    for (int i = 0; i < HS * 2; i++) { a.c[i] = k.c[i]; a.mu[i] = k.mu[i]; a.h[i] = k.h[i]; }
    if (feed == SK_FEED_I16) hipLaunchKernelGGL(k_hmm_stats<SK_FEED_I16>, dim3((unsigned)nreads), dim3(64), 0, c->stream, a);
    else                     hipLaunchKernelGGL(k_hmm_stats<SK_FEED_F64_NORM>, dim3((unsigned)nreads), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
