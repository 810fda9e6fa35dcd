// sk_sweep.hip -- the segmenter's parameter sweep: many get_segs parameter sets over masks that are already built.
//
// The {in band, kept} entries every segmenter route ends in depend only on (lim_low, lim_hi, std_scale);
// error, corrector, window, seg_dist and stall_len act only in get_segs' state machine (segmenter.py:420-464), stall_start
// and gap_dist only on a read's first two segments (test_segs, :473-494).  So the host builds the masks once per group of
// sets that share the first three (sk_launch_segment_masks, or the float64 statistics kernels), and k_seg_sweep_walk
// walks them once for every set of the group:
//   * the lane is the set.  A wavefront takes one read and up to 64 sets, or -- with fewer sets than that -- 64 / P reads
//     and P sets (P: the set count rounded up to a power of two), lane = (read, set);
//   * the lanes of one read load the same 16-byte entries (one address per read: a 128-byte line serves 8 entries for
//     all of them) and squeeze the dropped samples out of the same bits;
//   * each lane runs the state machine with its own parameters, held in registers, over the same 32-bit words: the
//     run-hopping form of k_seg_walk3 (run_word32) for sets with error < corrector, corrector, window, first_len >= 1, the
//     per-sample form of k_seg_walk2 (walk_general32) for the others.  The host launches the two kinds apart, so that a
//     wavefront holds only one.
// Only the first two segments are kept (in registers), with the exact count after merges.  The summary counters go
// from registers (per lane) to LDS (per workgroup) to memory: one 64-bit vector atomic per workgroup, set and counter.
// The helpers below are the ones of sk_segstat.hip with the segment store replaced by the two-segment record.
#include "sk_common.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int SW_WPB = 4;              // wavefronts per workgroup
constexpr int SW_NCNT = 7;             // counters of sk_seg_sweep_sum before `reserved`

// A lane's first two segments and its segment count (report_segment / run_report of sk_segstat.hip, max_segs = 2)
struct Seg2 {
    int nseg, last_end, s0s, s0e, s1s, s1e;
};

__device__ __forceinline__ void seg2_report(Seg2 &g, int start, int end, int seg_dist)
{
    // (selects, not branches: with branches the compiler turns the four fields into an indexed array in scratch)
    const bool merge = g.nseg > 0 && start - g.last_end < seg_dist;           // segmenter.py:451 merge
    const int n = g.nseg;
    g.s0s = (!merge && n == 0) ? start : g.s0s;
    g.s0e = (n == (merge ? 1 : 0)) ? end : g.s0e;
    g.s1s = (!merge && n == 1) ? start : g.s1s;
    g.s1e = (n == (merge ? 2 : 1)) ? end : g.s1e;
    g.nseg = merge ? n : n + 1;
    g.last_end = end;
}

// per-sample step (walk_general32, sk_segstat.hip): any parameters, samples at index >= n ignored
struct GenState {
    int prev, err, prev_err, c, w, start;
};

__device__ __forceinline__ void gen_word32(GenState &st, Seg2 &g, unsigned bits, int i0, int n, const sk_sweep_lane &p)
{
    int prev = st.prev, err = st.err, prev_err = st.prev_err, c = st.c, w = st.w, start = st.start;
#pragma unroll 4
    for (int b = 0; b < 32; b++) {
        const int i = i0 + b;
        const int valid = i < n;
        const int inb = (int)((bits >> b) & 1u) & valid;                           // :431 in band
        const int tol = (inb ^ 1) & prev & (int)(err < p.error) & valid;           // :442 tolerated
        const int act = inb | tol;
        const int closing = prev & (act ^ 1) & valid;                              // :448 / :458
        if (closing && (c >= p.window || (g.nseg == 0 && c >= p.first_len)))
            seg2_report(g, start, i - prev_err, p.seg_dist);                      // :449
        start = (inb & (prev ^ 1)) ? i : start;
        c = act ? c + 1 : (valid ? 0 : c);
        w += inb;
        err = tol ? err + 1 : (act ? err : (valid ? 0 : err));
        prev_err = tol ? prev_err + 1 : (valid ? 0 : prev_err);
        prev = valid ? act : prev;
        if (act && c >= p.window && c >= w) {                                      // :439 / :446
            if ((c % w) == 0) err--;
        }
    }
    st.prev = prev; st.err = err; st.prev_err = prev_err; st.c = c; st.w = w; st.start = start;
}

// run-hopping step (run_word32, sk_segstat.hip): error < corrector, positive thresholds; 32 samples, all valid
struct RunState {
    int in_run, zl, start, last1;
    unsigned thr;                      // report threshold: min(window, first_len) until the first segment (:448)
};

__device__ __forceinline__ void run_word32(RunState &st, Seg2 &g, unsigned W, int base, int E1, const sk_sweep_lane &p)
{
    int pos = 0;
    while (pos < 32) {
        if (!st.in_run) {
            const unsigned m = W >> pos;
            if (m == 0u) break;                                   // nothing opens in the rest of the word
            pos += __builtin_ctz(m);
            st.in_run = 1; st.start = base + pos; st.zl = E1; st.last1 = st.start;
        }
        const unsigned ones = W >> pos;                           // (pos < 32)
        unsigned Z = ~W >> pos;                                   // out-of-band samples at >= pos
        const int nz = __builtin_popcount(Z);
        if (nz < st.zl) {                                         // the run outlives this word
            st.zl -= nz;
            if (ones) st.last1 = base + 31 - __builtin_clz(W);
            break;
        }
        for (int i = 1; i < st.zl; i++) Z &= Z - 1u;              // the zl-th out-of-band sample closes the run
        const int q = __builtin_ctz(Z);
        const unsigned before = ones & ((1u << q) - 1u);          // in-band samples of [pos, z)
        if (before) st.last1 = base + pos + 31 - __builtin_clz(before);
        const int z = base + pos + q;
        if ((unsigned)(z - st.start) >= st.thr) {                 // :448-454
            seg2_report(g, st.start, st.last1 + 1, p.seg_dist);
            st.thr = (unsigned)p.window;
        }
        st.in_run = 0;
        pos += q + 1;
    }
}

// an entry's in-band bits with the dropped samples' bits deleted (squeeze_entry, sk_segstat.hip); returns the kept count
__device__ __forceinline__ int squeeze_entry(unsigned long long &inb, unsigned long long kp)
{
    int cnt = 64;
    if (kp != ~0ull) {
        if (kp == 0ull) { cnt = 0; kp = ~0ull; }
        const int hz = __builtin_clzll(kp);
        if (hz > 0) { cnt -= hz; kp |= ~0ull << (64 - hz); }
        while (kp != ~0ull) {
            const int pos = __builtin_ctzll(~kp);
            const unsigned long long below = (1ull << pos) - 1ull;
            inb = (inb & below) | ((inb >> 1) & ~below);
            kp = (kp & below) | ((kp >> 1) & ~below) | (1ull << 63);
            cnt--;
        }
        if (cnt < 64) inb &= (1ull << cnt) - 1ull;
    }
    return cnt;
}

// grid: x over the reads (persistent), y over slices of 64 sets.  setw: lanes per read (a power of two, 64 when the
// launch has 64 sets or more), so a wavefront walks 64 / setw reads at once.
template <bool FAST>
__global__ __launch_bounds__(64 * SW_WPB)
void k_seg_sweep_walk(const uint4 *__restrict__ mask2, int row16, const int32_t *__restrict__ len, int mmax, int nreads,
                      const sk_sweep_lane *__restrict__ lanes, int nlanes, int setw, sk_seg_sweep_sum *__restrict__ sums,
                      sk_seg_sweep_rec *__restrict__ recs, long long rec_stride)
{
    __shared__ unsigned long long acc[64][SW_NCNT];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < 64 * SW_NCNT; i += 64 * SW_WPB) (&acc[0][0])[i] = 0ull;
    __syncthreads();

    const int si = lane & (setw - 1);                   // my set within the slice
    const int ri = lane / setw;                         // my read within the wavefront's group of reads
    const int rpw = 64 / setw;
    const int k = blockIdx.y * 64 + si;
    const bool has_set = si < 64 && k < nlanes;
    const sk_sweep_lane p = lanes[has_set ? k : 0];    // (a lane without a set walks nothing: M = 0 below)
    const int E1 = max(p.error, 0) + 1;

    long long c_reads = 0, c_with = 0, c_segs = 0, c_stall = 0, c_gap = 0, c_both = 0, c_end = 0;
    const int nw = gridDim.x * SW_WPB;
    for (long long rb = (long long)(blockIdx.x * SW_WPB + w) * rpw; rb < nreads; rb += (long long)nw * rpw) {
        const int r = (int)rb + ri;
        const bool live = has_set && r < nreads;
        const int M = live ? min(max(len[r], 0), mmax) : 0;
        const uint4 *mrow = mask2 + (int64_t)(live ? r : 0) * row16;
        const int nent = (M + 63) >> 6;
        int nmax = nent;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) nmax = max(nmax, __shfl_xor(nmax, d));

        Seg2 g;
        g.nseg = 0; g.last_end = 0; g.s0s = -1; g.s0e = -1; g.s1s = -1; g.s1e = -1;
        RunState rs;
        rs.in_run = 0; rs.zl = 0; rs.start = 0; rs.last1 = 0; rs.thr = (unsigned)min(p.window, p.first_len);
        GenState gs;
        gs.prev = 0; gs.err = 0; gs.prev_err = 0; gs.c = 0; gs.w = p.corrector; gs.start = 0;   // :424

        unsigned long long qlo = 0ull, qhi = 0ull;      // bit queue: `fill` bits, oldest at bit 0 of qlo
        int fill = 0, done = 0;                         // done: filtered samples already walked
        for (int e0 = 0; e0 < nmax; e0 += 8) {
            uint4 buf[8];                               // eight entries = one 128-byte line of the read's row
#pragma unroll
            for (int j = 0; j < 8; j++) buf[j] = (e0 + j < nent) ? mrow[e0 + j] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (e0 + j >= nmax) break;              // (wave-uniform)
                if (e0 + j < nent) {
                    unsigned long long inb = ((unsigned long long)buf[j].y << 32) | buf[j].x;
                    const int cnt = squeeze_entry(inb, ((unsigned long long)buf[j].w << 32) | buf[j].z);
                    if (fill == 0) { qlo = inb; qhi = 0ull; }
                    else { qlo |= inb << fill; qhi = inb >> (64 - fill); }
                    fill += cnt;
                }
                if (fill >= 64) {
                    if constexpr (FAST) {
                        run_word32(rs, g, (unsigned)qlo, done, E1, p);
                        run_word32(rs, g, (unsigned)(qlo >> 32), done + 32, E1, p);
                    } else {
                        gen_word32(gs, g, (unsigned)qlo, done, 0x7fffffff, p);
                        gen_word32(gs, g, (unsigned)(qlo >> 32), done + 32, 0x7fffffff, p);
                    }
                    done += 64; fill -= 64;
                    qlo = qhi; qhi = 0ull;
                }
            }
        }
        if (fill > 0) {
            if constexpr (FAST) {
                // slots past the read's end count as in band: they can extend an open run (dropped at EOF, :466) but
                // never close one
                const unsigned long long wq = qlo | (~0ull << fill);
                run_word32(rs, g, (unsigned)wq, done, E1, p);
                run_word32(rs, g, (unsigned)(wq >> 32), done + 32, E1, p);
            } else {
                gen_word32(gs, g, (unsigned)qlo, done, done + fill, p);
                gen_word32(gs, g, (unsigned)(qlo >> 32), done + 32, done + fill, p);
            }
        }
        if (live) {
            const bool any = g.nseg >= 1;
            const bool stall = any && g.s0s <= p.stall_start;                                         // :480-483
            const bool gap = any && (g.nseg == 1 || (long long)g.s1s <= (long long)g.s0e + p.gap_dist);   // :485-492
            c_reads++;
            c_with += any;
            c_segs += g.nseg;
            c_stall += stall;
            c_gap += gap;
            c_both += stall && gap;
            c_end += any ? g.s0e : 0;
            if (recs) {
                sk_seg_sweep_rec *o = recs + (long long)p.index * rec_stride + r;
                int2 *o2 = (int2 *)o;                   // (records are 8-byte aligned)
                o2[0] = make_int2(g.nseg, g.s0s);
                o2[1] = make_int2(g.s0e, g.s1s);
                o2[2] = make_int2(g.s1e, 0);
            }
        }
    }

    // the lanes of one set (one per read of the wavefront's group) -> LDS -> memory
    auto red = [&](long long x) -> unsigned long long {
        unsigned long long u = (unsigned long long)x;
        for (int d = setw; d < 64; d <<= 1) u += __shfl_xor(u, d);
        return u;
    };
    const unsigned long long v0 = red(c_reads), v1 = red(c_with), v2 = red(c_segs), v3 = red(c_stall), v4 = red(c_gap),
                             v5 = red(c_both), v6 = red(c_end);
    if (ri == 0 && has_set) {
        if (v0) atomicAdd(&acc[si][0], v0);
        if (v1) atomicAdd(&acc[si][1], v1);
        if (v2) atomicAdd(&acc[si][2], v2);
        if (v3) atomicAdd(&acc[si][3], v3);
        if (v4) atomicAdd(&acc[si][4], v4);
        if (v5) atomicAdd(&acc[si][5], v5);
        if (v6) atomicAdd(&acc[si][6], v6);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * SW_NCNT; i += 64 * SW_WPB) {
        const int s = i / SW_NCNT, j = i % SW_NCNT;
        const int kk = blockIdx.y * 64 + s;
        const unsigned long long x = acc[s][j];
        if (s < setw && kk < nlanes && x)
            atomicAdd((unsigned long long *)&sums[lanes[kk].index] + j, x);
    }
}

} // namespace

void sk_sweep_plan(const sk_seg_sweep_set *sets, int32_t nsets, std::vector<sk_sweep_group> &groups,
                   std::vector<sk_sweep_lane> &lanes)
{
    groups.clear();
    lanes.clear();
    std::vector<int32_t> gid(nsets, -1);
    for (int32_t k = 0; k < nsets; k++) {                  // groups by the bit patterns of (lim_low, lim_hi, std_scale)
        for (size_t q = 0; q < groups.size() && gid[k] < 0; q++) {
            const sk_seg_params &a = sets[groups[q].rep].seg, &b = sets[k].seg;
            if (a.lim_low == b.lim_low && a.lim_hi == b.lim_hi && memcmp(&a.std_scale, &b.std_scale, sizeof(double)) == 0)
                gid[k] = (int32_t)q;
        }
        if (gid[k] < 0) {
            gid[k] = (int32_t)groups.size();
            groups.push_back(sk_sweep_group{k, 0, 0, 0});
        }
    }
    for (size_t q = 0; q < groups.size(); q++) {
        groups[q].first = (int32_t)lanes.size();
        for (int pass = 0; pass < 2; pass++)               // the run-hopping sets first, then the others
            for (int32_t k = 0; k < nsets; k++) {
                if (gid[k] != (int32_t)q) continue;
                const sk_seg_params &s = sets[k].seg;
                sk_sweep_lane L;
                L.error = s.error; L.corrector = s.corrector; L.window = s.window; L.seg_dist = s.seg_dist;
                const double fl = (double)s.window * s.stall_len;                // segmenter.py:448 (walk_params)
                if (!(fl == fl))           L.first_len = 0x7fffffff;
                else if (fl > 2147483000.) L.first_len = 0x7fffffff;
                else if (fl < -2147483000.) L.first_len = -0x7fffffff;
                else                       L.first_len = (int)ceil(fl);
                L.stall_start = sets[k].stall_start; L.gap_dist = sets[k].gap_dist; L.index = k;
                // (corrector >= 1: with corrector 0 and a negative error the first run has c == w, the corrector test
                // fires and err falls below `error` -- tolerance the run-hopping form does not have)
                const bool fast = L.error < L.corrector && L.corrector >= 1 && L.window >= 1 && L.first_len >= 1 &&
                                  sk_tune("SK_WALK_GENERAL") == nullptr;
                if (fast != (pass == 0)) continue;
                lanes.push_back(L);
                if (fast) groups[q].nfast++; else groups[q].ngen++;
            }
    }
}

int sk_launch_seg_sweep_walk(sk_ctx *c, const void *d_mask2, int row16, const int32_t *d_len, int64_t mmax, int32_t nreads,
                             const sk_sweep_lane *d_lanes, int32_t nlanes, bool fast, sk_seg_sweep_sum *d_sums,
                             sk_seg_sweep_rec *d_recs, int64_t rec_stride)
{
    if (nreads <= 0 || nlanes <= 0) return SK_OK;
    int setw = 1;
    while (setw < nlanes && setw < 64) setw <<= 1;
    const int rpw = 64 / setw;
    const int slices = (nlanes + 63) / 64;
    const long long waves = ((long long)nreads + rpw - 1) / rpw;
    long long gx = (waves + SW_WPB - 1) / SW_WPB;
    const long long cap = (long long)c->num_cu * 8 / slices + 1;            // persistent: about 8 workgroups per CU in all
    if (gx > cap) gx = cap;
    const int mm = (int)std::min<int64_t>(mmax, (int64_t)row16 * 64);
    auto fn = fast ? k_seg_sweep_walk<true> : k_seg_sweep_walk<false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)gx, (unsigned)slices), dim3(64 * SW_WPB), 0, c->stream, (const uint4 *)d_mask2,
                       row16, d_len, mm, nreads, d_lanes, nlanes, setw, d_sums, d_recs, (long long)rec_stride);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
