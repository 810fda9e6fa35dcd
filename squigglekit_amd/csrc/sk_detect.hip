// sk_detect.hip -- event detection: a raw read cut into events wherever the current steps, for gfx950.
//
// The definition is the project's own ("Event detection"; tests/detect_ref.py restates it in numpy).  Per
// read x[0..n) of int16 samples and per window w (short and long), with s1 / s2 the sums and q1 / q2 the sums of squares
// of x[i-w..i) and x[i..i+w):
//     t_w[i] = sqrt( double((s2-s1)^2 * w) / double(max(w*(q1+q2) - s1^2 - s2^2, 1)) )      for w <= i <= n - w, else 0
// -- exact integers under one correctly rounded division and one correctly rounded square root; no multiply-add (the
// file is compiled with -ffp-contract=off like the rest).  Two peak detectors walk t_short and t_long and mark
// positions; the boundaries are 0, the marks, n; a record holds start, length, sum and sum of squares of an event.
//
// The detector itself -- its window sums and peak state, t from the sums, the step, the slide of the sums -- is in
// sk_detect_dev.h, the text the event sessions (sk_evstream.hip) run too.
//
// k_detect_mark   one lane per read, 64 reads per wavefront (one wavefront per workgroup).  The wavefront loads a tile
//                 of DET_TILE = 128 samples of each of its 64 rows with 16-byte loads (16 lanes per row; rows that are not
//                 16-byte aligned take 2-byte loads) into a ring of two tiles per row in LDS.  A row's pitch is 129
//                 dwords, so the 2-byte reads of the 64 lanes -- all at the same position of their own rows -- fall into
//                 distinct banks.  A lane runs DET_LAG = 64 positions behind the newest sample (t_long[i] looks at
//                 x[i-64 .. i+64)), slides A = sum x[i-w..i), B = sum x[i..i+w) and Q = q1 + q2 per detector in
//                 registers, forms t and steps the detector.  t is never stored.  A detector's marks come in rising
//                 order, so each detector gathers the bits of one 64-sample word in a register and ORs the word into the
//                 read's row of mark words (zeroed beforehand; the lane is the row's only writer) when it moves on: at
//                 most two 8-byte read-modify-writes per 64 samples.  A lane whose read has ended idles; the wavefront
//                 leaves after the tile that ends its longest read.
// k_detect_count  one wavefront per read: events = marks in (0, n) + 1 (0 for an empty read), as int64 -- the input of
//                 the exclusive scan (sk_launch_scan_i64, sk_pull.hip) that gives off[0..R].
// k_detect_fill   one wavefront per read, 4 096 samples a round (staged in LDS, pitch 33 dwords per lane: no bank
//                 conflicts).  Each lane owns 64 samples and one mark word: it writes the events that begin and end inside
//                 its samples itself, and the wavefront joins the open pieces -- an inclusive scan of the sums before each
//                 lane's first mark, a ballot of the lanes that hold a mark, the tail of the nearest such lane below.
//                 Records go to rec[off[r] ..]; nothing is written when off[R] > cap.
//
// The mark words lie row by row ([read][word], not transposed like the segmenter's maskT): k_detect_fill and
// k_detect_count then read them coalesced, a sub-batch of a host call is a slice, and k_detect_mark's rare word
// updates do not care.  Global traffic: 2 bytes per sample twice (mark, fill), 1/8 byte per sample of mark words written
// and read twice, 24 bytes per event.
#include "sk_detect_dev.h"

namespace {

constexpr int FILL_ROUND = 4096;              // samples per round of k_detect_fill (64 per lane)
constexpr int FILL_PITCH = 33;                // dwords per lane in LDS

struct detect_kargs {
    const int16_t *sig;
    int64_t        stride;
    const int32_t *len;
    int32_t        nreads;
    int32_t        vec;          // rows are 16-byte aligned (base and stride): 16-byte loads
    sk_det_params  p;
    uint64_t      *words;        // [nreads][nwords]
    int64_t        nwords;
    int64_t       *off;          // [nreads + 1]: counts, then their exclusive scan
    sk_det_event  *rec;
    int64_t        cap;
};

__device__ __forceinline__ int32_t det_len(const detect_kargs &a, int64_t r)
{
    if (r >= a.nreads) return 0;
    int64_t n = a.len[r];
    if (n < 0) n = 0;
    if (n > a.stride) n = a.stride;
    return (int32_t)n;
}

// the mark word a detector (det_state, det_step, det_slide: sk_detect_dev.h) is gathering
struct det_word {
    int64_t  widx = -1;          // (-1: none)
    uint64_t wbits = 0;
};

__device__ __forceinline__ void det_flush(det_word &d, uint64_t *wrow)
{
    if (d.wbits) wrow[d.widx] |= d.wbits;
    d.wbits = 0;
}

__device__ __forceinline__ void det_mark(det_word &d, uint64_t *wrow, int32_t p)
{
    const int64_t wi = p >> 6;
    if (wi != d.widx) { det_flush(d, wrow); d.widx = wi; }
    d.wbits |= 1ull << (p & 63);
}

__global__ __launch_bounds__(64)
void k_detect_mark(const detect_kargs a)
{
    __shared__ uint32_t ring[64 * DET_PITCH];
    __shared__ int32_t nrow[64];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int32_t n = det_len(a, r0 + lane);
    nrow[lane] = n;
    int32_t nmax = n;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t q = __shfl_xor(nmax, o); nmax = q > nmax ? q : nmax; }
    if (nmax == 0) return;
    __syncthreads();

    const int16_t *xrow = (const int16_t *)ring + (size_t)lane * (2 * DET_PITCH);
    uint64_t *wrow = a.words + (r0 + lane < a.nreads ? (r0 + lane) * a.nwords : 0);
    const double h = a.p.peak_height;
    det_state ds, dl;
    det_word ws, wl;
    det_init(ds, a.p.w_short, a.p.th_short);
    det_init(dl, a.p.w_long, a.p.th_long);
    int32_t i = 0;

    const int ntiles = (nmax + DET_TILE - 1) / DET_TILE;
    for (int k = 0; k < ntiles; k++) {
        // tile k of the 64 rows -> its half of the ring
        if (a.vec) {
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int row = it * 4 + (lane >> 4);
                const int32_t pos = k * DET_TILE + (lane & 15) * 8;
                if (pos < nrow[row]) {
                    const uint4 v = *(const uint4 *)(a.sig + (r0 + row) * a.stride + pos);
                    uint32_t *dst = ring + row * DET_PITCH + ((pos & (DET_RING - 1)) >> 1);
                    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
                }
            }
        } else {
            int16_t *ring16 = (int16_t *)ring;
            for (int row = 0; row < 64; row++) {
                const int32_t nr = nrow[row];
                for (int cc = lane; cc < DET_TILE; cc += 64) {
                    const int32_t pos = k * DET_TILE + cc;
                    if (pos < nr) ring16[row * (2 * DET_PITCH) + (pos & (DET_RING - 1))] = a.sig[(r0 + row) * a.stride + pos];
                }
            }
        }
        __syncthreads();

        if (k == 0)                                             // B(0) of both detectors: the first w samples
            for (int j = 0; j < 64; j++) {
                const int32_t x = j < n ? (int32_t)xrow[j] : 0;
                if (j < ds.w) { ds.B += x; ds.Q += (int64_t)(x * x); }
                if (j < dl.w) { dl.B += x; dl.Q += (int64_t)(x * x); }
            }
        const int32_t seen = (k + 1) * DET_TILE;
        const int32_t limit = seen >= n ? n : seen - DET_LAG;
        for (; i < limit; i++) {
            if (i > ds.masked_to) det_step(ds, &dl, h, i, det_t(ds, i, n), [&](int32_t p) { det_mark(ws, wrow, p); });
            if (i > dl.masked_to) det_step(dl, nullptr, h, i, det_t(dl, i, n), [&](int32_t p) { det_mark(wl, wrow, p); });
            const int32_t xi = (int32_t)xrow[i & (DET_RING - 1)];
            det_slide(ds, xrow, i, n, xi);
            det_slide(dl, xrow, i, n, xi);
        }
        __syncthreads();                                        // the ring's other half is read before tile k + 1 lands
    }
    det_flush(ws, wrow);
    det_flush(wl, wrow);
}

// mark word wi of a read of n samples: bits at and above n and position 0 cleared
__device__ __forceinline__ uint64_t mark_word(const uint64_t *wrow, int64_t wi, int32_t n)
{
    const int64_t left = (int64_t)n - wi * 64;
    if (left <= 0) return 0;
    uint64_t m = wrow[wi];
    if (left < 64) m &= (1ull << left) - 1ull;
    if (wi == 0) m &= ~1ull;
    return m;
}

__device__ __forceinline__ int64_t wave_incl_scan_i64(int64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t q = __shfl_up((long long)v, o);
        if (lane >= o) v += q;
    }
    return v;
}

__global__ __launch_bounds__(64)
void k_detect_count(const detect_kargs a)
{
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (r >= a.nreads) return;
    const int32_t n = det_len(a, r);
    const uint64_t *wrow = a.words + r * a.nwords;
    const int64_t nw = ((int64_t)n + 63) >> 6;
    int64_t c = 0;
    for (int64_t wi = lane; wi < nw; wi += 64) c += __popcll(mark_word(wrow, wi, n));
    c = wave_incl_scan_i64(c, lane);
    if (lane == 63) a.off[r] = n > 0 ? c + 1 : 0;
}

__device__ __forceinline__ void put_event(const detect_kargs &a, int64_t at, int32_t start, int32_t end, int64_t s, int64_t q)
{
    if (at < 0 || at >= a.cap) return;                          // (never: the count and the fill read the same words)
    sk_det_event e;
    e.start = start; e.length = end - start; e.sum = s; e.sumsq = q;
    a.rec[at] = e;
}

__global__ __launch_bounds__(64)
void k_detect_fill(const detect_kargs a)
{
    __shared__ uint32_t stage[64 * FILL_PITCH];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (r >= a.nreads || !a.rec || a.off[a.nreads] > a.cap) return;
    const int32_t n = det_len(a, r);
    if (n == 0) return;
    const int16_t *row = a.sig + r * a.stride;
    const uint64_t *wrow = a.words + r * a.nwords;
    const int16_t *mine = (const int16_t *)stage + lane * (2 * FILL_PITCH);
    const int64_t base = a.off[r];

    int64_t carry_s = 0, carry_q = 0, marks = 0;
    int32_t carry_start = 0;
    for (int32_t p0 = 0; p0 < n; p0 += FILL_ROUND) {
        if (a.vec) {
            for (int j = lane * 8; j < FILL_ROUND && p0 + j < n; j += 512) {
                const uint4 v = *(const uint4 *)(row + p0 + j);
                uint32_t *dst = stage + (j >> 6) * FILL_PITCH + ((j & 63) >> 1);
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
        } else {
            int16_t *st16 = (int16_t *)stage;
            for (int j = lane; j < FILL_ROUND && p0 + j < n; j += 64) st16[(j >> 6) * (2 * FILL_PITCH) + (j & 63)] = row[p0 + j];
        }
        __syncthreads();

        const int32_t lb = p0 + lane * 64;                      // my first sample
        const uint64_t m = mark_word(wrow, (int64_t)(p0 >> 6) + lane, n);
        const int c = __popcll(m);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int q = __shfl_up(incl, o); if (lane >= o) incl += q; }
        const int64_t ev = base + marks + (incl - c);           // the event that ends at my first mark
        const int cnt = n - lb < 0 ? 0 : (n - lb < 64 ? n - lb : 64);

        int64_t cur_s = 0, cur_q = 0, head_s = 0, head_q = 0;
        int32_t last = -1;
        int k = 0;
        for (int b = 0; b < cnt; b++) {
            const int32_t x = (int32_t)mine[b];
            if ((m >> b) & 1ull) {
                if (k == 0) { head_s = cur_s; head_q = cur_q; }
                else put_event(a, ev + k, last, lb + b, cur_s, cur_q);
                k++; last = lb + b; cur_s = 0; cur_q = 0;
            }
            cur_s += x; cur_q += (int64_t)(x * x);
        }
        if (c == 0) { head_s = cur_s; head_q = cur_q; }          // no mark: all of it joins its neighbours
        const int64_t g_s = wave_incl_scan_i64(head_s, lane), g_q = wave_incl_scan_i64(head_q, lane);
        const uint64_t marked = __ballot(c > 0);
        const uint64_t below = marked & ((1ull << lane) - 1ull);
        const int P = below ? 63 - (int)__builtin_clzll(below) : 0;
        const int64_t tp_s = __shfl((long long)cur_s, P), tp_q = __shfl((long long)cur_q, P);
        const int64_t gp_s = __shfl((long long)g_s, P), gp_q = __shfl((long long)g_q, P);
        const int32_t tp_start = __shfl(last, P);
        if (c > 0) {
            const int32_t first = lb + (int)__builtin_ctzll(m);
            if (below) put_event(a, ev, tp_start, first, tp_s + g_s - gp_s, tp_q + g_q - gp_q);
            else       put_event(a, ev, carry_start, first, carry_s + g_s, carry_q + g_q);
        }
        const int Qn = marked ? 63 - (int)__builtin_clzll(marked) : 0;
        const int64_t tq_s = __shfl((long long)cur_s, Qn), tq_q = __shfl((long long)cur_q, Qn);
        const int64_t gq_s = __shfl((long long)g_s, Qn), gq_q = __shfl((long long)g_q, Qn);
        const int64_t ge_s = __shfl((long long)g_s, 63), ge_q = __shfl((long long)g_q, 63);
        const int32_t tq_start = __shfl(last, Qn);
        if (marked) { carry_s = tq_s + ge_s - gq_s; carry_q = tq_q + ge_q - gq_q; carry_start = tq_start; }
        else        { carry_s += ge_s; carry_q += ge_q; }
        marks += __shfl(incl, 63);
        __syncthreads();                                        // the staged samples are read before the next round's land
    }
    if (lane == 0) put_event(a, base + marks, carry_start, n, carry_s, carry_q);
}

} // namespace

static_assert(sizeof(sk_det_event) == 24, "sk_det_event is 24 bytes (include/squigglekit_hip.h)");
static_assert(sizeof(sk_det_params) == 32, "sk_det_params is 32 bytes (include/squigglekit_hip.h)");

int64_t sk_detect_words(int64_t stride) { return (stride + 63) / 64; }

size_t sk_detect_work_bytes(int32_t nreads, int64_t stride)
{
    return ((size_t)nreads * (size_t)sk_detect_words(stride) + (size_t)sk_scan_blocks(nreads)) * sizeof(int64_t);
}

static detect_kargs detect_args(const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                                const sk_det_params *p, void *d_work, int64_t *d_off, sk_det_event *d_rec, int64_t cap)
{
    detect_kargs a;
    a.sig = d_sig; a.stride = stride; a.len = d_len; a.nreads = nreads;
    a.vec = ((uintptr_t)d_sig % 16 == 0 && stride % 8 == 0) ? 1 : 0;
    a.p = *p;
    a.words = (uint64_t *)d_work; a.nwords = sk_detect_words(stride);
    a.off = d_off; a.rec = d_rec; a.cap = cap;
    return a;
}

// marks and event counts of nreads rows: the mark words of read r at d_words + r * sk_detect_words(stride) (8 bytes each),
// the count (int64) at d_cnt[r]
int sk_launch_detect_mark(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                          const sk_det_params *p, void *d_words, int64_t *d_cnt)
{
    if (nreads <= 0) return SK_OK;
    const detect_kargs a = detect_args(d_sig, stride, d_len, nreads, p, d_words, d_cnt, nullptr, 0);
    SK_HIP(hipMemsetAsync(d_words, 0, (size_t)nreads * (size_t)a.nwords * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_detect_mark, dim3((unsigned)((nreads + 63) / 64)), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_detect_count, dim3((unsigned)nreads), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

// d_off[0 .. nreads]: the counts sk_launch_detect_mark left in d_off[0 .. nreads) -> their exclusive scan
int sk_launch_detect_scan(sk_ctx *c, int32_t nreads, int64_t *d_bsum, int64_t *d_off)
{
    return sk_launch_scan_i64(c, d_off, nreads, d_bsum, d_off);
}

// the records of nreads marked rows at d_rec[d_off[r] ..] -- on the device nothing happens when d_off[nreads] > cap
int sk_launch_detect_fill(sk_ctx *c, const int16_t *d_sig, int64_t stride, const int32_t *d_len, int32_t nreads,
                          const sk_det_params *p, const void *d_words, const int64_t *d_off, sk_det_event *d_rec, int64_t cap)
{
    if (nreads <= 0 || !d_rec || cap <= 0) return SK_OK;
    const detect_kargs a = detect_args(d_sig, stride, d_len, nreads, p, (void *)d_words, (int64_t *)d_off, d_rec, cap);
    hipLaunchKernelGGL(k_detect_fill, dim3((unsigned)nreads), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
