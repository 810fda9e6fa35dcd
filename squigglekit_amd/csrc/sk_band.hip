// sk_band.hip -- adaptive-band DTW over a pair list for gfx950: records and warping paths of whole reads in one pass.
//
// sk_pairs.hip / sk_pairpath.hip pay for the full N x M matrix and stop at queries of 1 024 points.  Here one wavefront
// sweeps a pair's anti-diagonals inside a band of W = 64 * K cells (K = 1, 2, 4) that moves towards whichever of its
// ends is cheaper (the Suzuki-Kasahara scheme of nanopolish / f5c, with this library's |x - y| cost and min-of-three tie
// order): (N + M - 1) * W cells and (N + M - 1) * W / 4 bytes of direction words per pair, whatever N and M are.
//
// The statement (tests/band_ref.py is its numpy form; the kernel equals it bit for bit):
//   band b = 0 .. N + M - 2 has a lower-left corner (I_b, J_b), (I_0, J_0) = (h, -h), h = W / 2; offset o of band b is the
//   cell (I_b - o, J_b + o).  A cell outside the matrix holds +inf.  D(0, 0) = |x0 - y0|; otherwise up = D(i-1, j) and
//   left = D(i, j-1) come from band b - 1, diag = D(i-1, j-1) from band b - 2, at the offsets of those cells, +inf outside
//   [0, W).  m1 = left < diag ? left : diag; m = up < m1 ? up : m1; D = |x_i - y_j| + m; the direction is UP if up < m1,
//   else LEFT if left < diag, else DIAG.  After band b: ur = D_b[W-1] < ll = D_b[0] moves right (J + 1), ll < ur moves
//   down (I + 1), anything else moves right for even b and down for odd b.
//   pinned end: dist = D(N-1, M-1) if the last band holds it, else +inf; end = M - 1.  free end: over the bands in
//   ascending order the first strictly smallest D of row N - 1.  dist == +inf: the band lost the corner (SK_FLAG_BAND_LOST).
//
// Lane l owns offsets l*K .. l*K + K - 1.  A move is wave-uniform (two v_readlane and scalar compares), so one of up /
// left is the same register of band b - 1 and the other its neighbour: a register rename inside the lane and ONE wave
// shift (DPP wave_shr:1 / wave_shl:1) of the lane's edge value across lanes, chosen by a uniform branch.  The neighbour
// array of band b - 1 is kept one more step: the diagonal of band b is that array when the last two moves agree and
// band b - 2 itself when they differ -- (i-1, j-1) is the `up` of the left cell and the `left` of the upper one -- so the
// diagonal costs no shift.  x moves one offset up on a down move, y one offset down on a right move; the new sample
// enters at lane 0 / lane 63 from a 64-sample register block that is rotated as F is in k_sdtw and refilled, one block
// ahead, behind a uniform counter: no load sits on the step's dependency chain.  No LDS in the forward sweep.
//
// Paths: 2 bits per cell; a lane packs its K cells of 16 / K steps into one word and stores it, coalesced, to row
// b / (16 / K) of the wavefront's slab; the moves go one bit per step into 64-bit words behind the direction rows.  The
// back-trace stages 16 rows of direction words (256 / K bands) and the move words around them in LDS, walks inside the
// block (every lane the same walk, on the scalar unit; lane 0 stores), rebuilds I_b from the move bits going backwards
// and ends, as a self-check, on cell (0, 0) at offset h of band 0; a walk that leaves the band or the matrix, or ends
// elsewhere, gives spans -1 and is counted (sk_last_path_mismatches()), as is a pair that lost the corner.
//
// Budget: K = 4 holds 5 band arrays + 2 sample arrays of 4 doubles and four stream blocks.  As compiled: 68 / 92 / 130
// VGPRs with paths (7 / 5 / 3 wavefronts per SIMD for K = 1 / 2 / 4), 42 / 64 / 102 without (8 / 8 / 4); no scratch;
// 4 160 bytes of LDS per wavefront with paths (the back-trace's block), none without.  A slab is
// ceil(steps * K / 16) * 64 + 2 * ceil(steps / 64) + 2 words, sized from the longest listed pair (at most 128 MiB +
// 256 KiB: N = M = 2^20, W = 256); the slabs of one call take at most BAND_SLAB_BUDGET = 8 GiB.  The launch has as many
// wavefronts as the device holds at a time (at most 32 per CU), one wavefront per block, striding over the table
// (longest first).
#include "sk_sdtw_dev.h"
#include <algorithm>
#include <stdlib.h>
#include <vector>

namespace {

enum { DIR_DIAG = 0, DIR_LEFT = 1, DIR_UP = 2 };
constexpr int     BT_ROWS = 16;                 // direction rows the back-trace stages at a time
constexpr int     BT_MV   = 16;                 // move words (32 bits) staged with them: 256 / 32 + 1 below, rounded up
constexpr int64_t BAND_SLAB_BUDGET = (int64_t)8 << 30;
constexpr int     BAND_MAX_LEN = 1 << 20;

struct band_kargs {
    const double        *values;    // the pool (device); sequence offsets in `tab` are relative to it
    const sk_band_entry *tab;       // [npairs], longest N + M first
    sk_hit              *rec;       // [npairs], by the caller's pair index
    int32_t             *spans;     // [sum N][2] (PATHS)
    int                  npairs;
    int                  free_end;
    int32_t             *mism;      // (PATHS) += pairs without a path that should have one
    uint32_t            *slab;      // (PATHS) per wavefront slab_words words: dir_words of direction rows, then the move words
    int64_t              slab_words;
    int64_t              dir_words;
};

__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

template <int K, bool PATHS>
__global__ __launch_bounds__(64)
void k_band(const band_kargs a)
{
    constexpr int W = 64 * K, H = W / 2, S = 16 / K;        // S: steps per direction word
    __shared__ uint32_t bt_dirs[PATHS ? BT_ROWS * 64 : 1];
    __shared__ uint32_t bt_mv[PATHS ? BT_MV : 1];
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x;
    uint32_t *dirs = PATHS ? a.slab + (int64_t)blockIdx.x * a.slab_words : nullptr;
    uint32_t *mvw = PATHS ? dirs + a.dir_words : nullptr;

    for (int id = blockIdx.x; id < a.npairs; id += gridDim.x) {
        const sk_band_entry e = a.tab[id];
        const int N = e.N, M = e.M;
        int32_t *sp = PATHS ? a.spans + e.span_off * 2 : nullptr;
        if (M == 0) {                                       // an empty target: the record of sk_dtw_pairs, no path, not counted
            if (lane == 0) {
                sk_hit h;
                h.dist = __builtin_nan(""); h.start = -1; h.end = -1; h.n = 0; h.flags = SK_FLAG_EMPTY;
                a.rec[e.pair] = h;
            }
            if (PATHS) for (int k = lane; k < N * 2; k += 64) sp[k] = -1;
            continue;
        }
        const double *x = a.values + e.qoff;
        const double *y = a.values + e.toff;
        const int steps = N + M - 1;
        auto ldx = [&](int i) -> double { return i < N ? x[i] : 0.0; };     // (i >= 0 at every call)
        auto ldy = [&](int j) -> double { return j < M ? y[j] : 0.0; };

        // ---- band 0: corner (H, -H), cell (0, 0) at offset H -------------------------------------------------------------
        double D1[K], D2[K], S2[K], X[K], Y[K];             // band b-1, band b-2, b-1's neighbour array, the cells' samples
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int o = lane * K + k;
            const int xi = H - o, yj = o - H;
            X[k] = (xi >= 0 && xi < N) ? x[xi] : 0.0;
            Y[k] = (yj >= 0 && yj < M) ? y[yj] : 0.0;
            D1[k] = INF;
            D2[k] = S2[k] = (o == H) ? 0.0 : INF;           // the diagonal of cell (0, 0)
        }
        int xn = H + 1, yn = H;                             // the next x / y sample to enter the band
        double FX = ldx(xn + lane), FXn = ldx(xn + 64 + lane);          // lane 0 holds the next x
        double FY = ldy(yn + ((lane + 1) & 63)), FYn = ldy(yn + 64 + ((lane + 1) & 63));   // lane 63 holds the next y
        int cx = 0, cy = 0;
        int I = H, J = -H;
        int mv = 0, mvprev = 0;                             // the move into band b / into band b-1: 1 = down
        uint32_t word = 0;
        uint64_t mbits = 0;
        double best = INF;
        int best_end = -1, best_I = H;

        for (int b = 0; b < steps; b++) {
            double Sh[K], Dn[K];
            if (b == 0) {
#pragma unroll
                for (int k = 0; k < K; k++) Sh[k] = INF;
            } else if (mv) {                                // down: x one offset up, `left` is the offset below
                I++;
                const double x0 = dpp_f64<DPP_WAVE_SHR1>(FX, X[K - 1]);
                const double s0 = dpp_f64<DPP_WAVE_SHR1>(INF, D1[K - 1]);
#pragma unroll
                for (int k = K - 1; k > 0; k--) { X[k] = X[k - 1]; Sh[k] = D1[k - 1]; }
                X[0] = x0; Sh[0] = s0;
                FX = dpp_f64<DPP_WAVE_ROL1>(FX, FX);
                if (++cx == 64) { cx = 0; xn += 64; FX = FXn; FXn = ldx(xn + 64 + lane); }
            } else {                                        // right: y one offset down, `up` is the offset above
                J++;
                const double yl = dpp_f64<DPP_WAVE_SHL1>(FY, Y[0]);
                const double sl = dpp_f64<DPP_WAVE_SHL1>(INF, D1[0]);
#pragma unroll
                for (int k = 0; k < K - 1; k++) { Y[k] = Y[k + 1]; Sh[k] = D1[k + 1]; }
                Y[K - 1] = yl; Sh[K - 1] = sl;
                FY = dpp_f64<DPP_WAVE_ROL1>(FY, FY);
                if (++cy == 64) { cy = 0; yn += 64; FY = FYn; FYn = ldy(yn + 64 + ((lane + 1) & 63)); }
            }
            // live offsets [lo, lo + cnt]: 0 <= I - o < N and 0 <= J + o < M (scalar)
            int lo = max(I - N + 1, -J);
            const int hi = min(I, M - 1 - J);
            unsigned cnt = 0;
            if (hi >= lo) cnt = (unsigned)(hi - lo); else lo = W + 1;
            const int sh0 = (b % S) * K * 2;
            auto cells = [&](const double *up, const double *left, const double *diag) {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const double c = fabs(X[k] - Y[k]);
                    const bool lt1 = left[k] < diag[k];             // diag wins ties over left
                    const double m1 = lt1 ? left[k] : diag[k];
                    const bool lt2 = up[k] < m1;                    // up only if strictly smaller
                    const double m = lt2 ? up[k] : m1;
                    const bool live = (unsigned)(lane * K + k - lo) <= cnt;
                    Dn[k] = live ? c + m : INF;
                    if (PATHS) word |= (uint32_t)(lt2 ? DIR_UP : (lt1 ? DIR_LEFT : DIR_DIAG)) << (sh0 + 2 * k);
                }
            };
            if (mv) { if (mvprev) cells(D1, Sh, S2); else cells(D1, Sh, D2); }
            else    { if (mvprev) cells(Sh, D1, D2); else cells(Sh, D1, S2); }
#pragma unroll
            for (int k = 0; k < K; k++) { S2[k] = Sh[k]; D2[k] = D1[k]; D1[k] = Dn[k]; }
            mvprev = mv;
            if (PATHS && ((b % S) == S - 1 || b == steps - 1)) { dirs[(int64_t)(b / S) * 64 + lane] = word; word = 0; }

            const int oe = I - (N - 1);                     // row N - 1 in this band
            if (a.free_end && oe >= 0 && oe < W && b >= N - 1) {
                double v = D1[0];
#pragma unroll
                for (int k = 1; k < K; k++) if (oe % K == k) v = D1[k];
                v = readlane_f64(v, oe / K);
                if (v < best) { best = v; best_end = b - (N - 1); best_I = I; }
            }
            if (b < steps - 1) {
                const double ll = readlane_f64(D1[0], 0), ur = readlane_f64(D1[K - 1], 63);
                mv = ur < ll ? 0 : (ll < ur ? 1 : (b & 1));
                if (PATHS) mbits |= (uint64_t)mv << (b & 63);
            }
            if (PATHS && ((b & 63) == 63 || b == steps - 1)) {
                if (lane < 2) mvw[2 * (b >> 6) + lane] = lane ? (uint32_t)(mbits >> 32) : (uint32_t)mbits;
                mbits = 0;
            }
        }
        if (!a.free_end) {
            const int oe = I - (N - 1);
            if (oe >= 0 && oe < W) {
                double v = D1[0];
#pragma unroll
                for (int k = 1; k < K; k++) if (oe % K == k) v = D1[k];
                best = readlane_f64(v, oe / K);
            }
            best_end = M - 1; best_I = I;
        }
        const bool lost = best == INF;
        if (lane == 0) {
            sk_hit h;
            h.dist = best; h.start = lost ? -1 : 0; h.end = lost ? -1 : best_end; h.n = M; h.flags = lost ? SK_FLAG_BAND_LOST : 0;
            a.rec[e.pair] = h;
        }
        if (!PATHS) continue;

        // ---- back-trace: blocks of BT_ROWS direction rows in LDS, I_b rebuilt from the move bits ---------------------------
        __syncthreads();                                    // (one wavefront per block) the slab's stores before its loads
        bool ok = !lost;
        int i = N - 1, j = best_end, top = best_end, Ic = best_I;
        const int nrows = (steps + S - 1) / S, nmv = 2 * ((steps + 63) >> 6);
        while (ok && (i > 0 || j > 0)) {
            const int c = (i + j) / (BT_ROWS * S), blo = c * BT_ROWS * S;
            const int w0 = blo >= 32 ? blo / 32 - 1 : 0;    // the moves of bands blo - 2, blo - 1 lie one word below
#pragma unroll
            for (int r = 0; r < BT_ROWS; r++) {
                const int row = c * BT_ROWS + r;
                bt_dirs[r * 64 + lane] = row < nrows ? dirs[(int64_t)row * 64 + lane] : 0u;
            }
            if (lane < BT_MV) bt_mv[lane] = w0 + lane < nmv ? mvw[w0 + lane] : 0u;
            __syncthreads();
            // (every lane reads the same word: readfirstlane keeps the walk on the scalar unit)
            auto moved = [&](int t) -> int {                // down after band t
                return (int)((__builtin_amdgcn_readfirstlane(bt_mv[(t >> 5) - w0]) >> (t & 31)) & 1u);
            };
            while (i > 0 || j > 0) {
                const int b = i + j;
                if (b < blo) break;
                const int o = Ic - i;
                if (o < 0 || o >= W) { ok = false; break; }
                const uint32_t w = __builtin_amdgcn_readfirstlane(bt_dirs[(b / S - c * BT_ROWS) * 64 + o / K]);
                const int d = (int)((w >> (((b % S) * K + o % K) * 2)) & 3u);
                if (d == DIR_LEFT) {
                    if (j == 0) { ok = false; break; }
                    j--; Ic -= moved(b - 1);
                    continue;
                }
                if (i == 0 || (d == DIR_DIAG && j == 0)) { ok = false; break; }
                if (lane == 0) { sp[2 * i] = j; sp[2 * i + 1] = top; }
                i--; Ic -= moved(b - 1);
                if (d == DIR_DIAG) { j--; Ic -= moved(b - 2); }
                top = j;
            }
            __syncthreads();
        }
        if (lane == 0) { sp[0] = 0; sp[1] = top; }
        if (!(ok && Ic == H)) {                             // self-check: the walk ends on offset H of band 0
            __syncthreads();
            for (int k = lane; k < N * 2; k += 64) sp[k] = -1;
            if (lane == 0) atomicAdd(a.mism, 1);
        }
        __syncthreads();
    }
}

template <int K>
void launch_band(const band_kargs &k, bool paths, int64_t waves, hipStream_t st)
{
    if (paths) hipLaunchKernelGGL((k_band<K, true>), dim3((unsigned)waves), dim3(64), 0, st, k);
    else       hipLaunchKernelGGL((k_band<K, false>), dim3((unsigned)waves), dim3(64), 0, st, k);
}

// wavefronts of one instantiation a CU holds at a time: more would queue behind the whole lists of those that run
template <int K>
int resident_band(bool paths)
{
    int n = 0;
    const hipError_t e = paths ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_band<K, true>, 64, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_band<K, false>, 64, 0);
    return (e == hipSuccess && n > 0) ? n : 8;
}

} // namespace

int sk_band_check(const int64_t *off, int32_t nseq, const sk_pair *pairs, int64_t npairs, int32_t band, int32_t end_mode,
                  const void *out)
{
    if (band != 64 && band != 128 && band != 256) return sk_fail(SK_ERR_INVALID, "band width %d: need 64, 128 or 256", band);
    if (end_mode != SK_BAND_PINNED && end_mode != SK_BAND_FREE) return sk_fail(SK_ERR_INVALID, "unknown band end mode %d", end_mode);
    if (npairs < 0 || nseq < 0) return sk_fail(SK_ERR_INVALID, "npairs or nseq < 0");
    if (npairs > ((int64_t)1 << 27)) return sk_fail(SK_ERR_UNSUPPORTED, "npairs %lld above 134217728", (long long)npairs);
    if (npairs == 0) return SK_OK;
    if (!off || !pairs || !out) return sk_fail(SK_ERR_INVALID, "NULL off/pairs/out");
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query, t = pairs[p].target;
        if (q < 0 || q >= nseq) return sk_fail(SK_ERR_INVALID, "pair %lld: query index %d outside [0, %d)", (long long)p, q, nseq);
        if (t < 0 || t >= nseq) return sk_fail(SK_ERR_INVALID, "pair %lld: target index %d outside [0, %d)", (long long)p, t, nseq);
        const int64_t N = off[q + 1] - off[q], M = off[t + 1] - off[t];
        if (N < 0 || M < 0)
            return sk_fail(SK_ERR_INVALID, "pair %lld: bad length (query %lld, target %lld)", (long long)p, (long long)N, (long long)M);
        if (N == 0) return sk_fail(SK_ERR_INVALID, "pair %lld: empty query (sequence %d)", (long long)p, q);
        if (N > BAND_MAX_LEN)
            return sk_fail(SK_ERR_UNSUPPORTED, "pair %lld: query of %lld points (sequence %d; at most 1048576)", (long long)p, (long long)N, q);
        if (M > BAND_MAX_LEN)
            return sk_fail(SK_ERR_UNSUPPORTED, "pair %lld: target of %lld points (sequence %d; at most 1048576)", (long long)p, (long long)M, t);
    }
    return SK_OK;
}

int sk_band_run(sk_ctx *c, const double *d_values, const int64_t *off, int64_t off0, int32_t nseq, const sk_pair *pairs,
                int64_t npairs, int32_t band, int32_t end_mode, sk_hit *d_rec, int32_t *d_spans)
{
    int rc;
    if ((rc = sk_band_check(off, nseq, pairs, npairs, band, end_mode, d_rec))) return rc;
    if (npairs == 0) return SK_OK;
    if (!d_values) return sk_fail(SK_ERR_INVALID, "NULL values");
    const bool paths = d_spans != nullptr;
    const int K = band / 64;

    // ---- the plan: the table longest N + M first, the slab from the longest pair, the wavefronts from the budget ----------
    SK_HIP(hipStreamSynchronize(c->stream));                // an earlier call may still read the old table
    std::vector<sk_band_entry> list((size_t)npairs);
    int64_t rows = 0, steps_max = 0;
    for (int64_t p = 0; p < npairs; p++) {
        const int32_t q = pairs[p].query, t = pairs[p].target;
        sk_band_entry e;
        e.qoff = off[q] - off0; e.toff = off[t] - off0; e.span_off = rows;
        e.N = (int32_t)(off[q + 1] - off[q]); e.M = (int32_t)(off[t + 1] - off[t]); e.pair = (int32_t)p; e.pad = 0;
        list[(size_t)p] = e;
        rows += e.N;
        if (e.M > 0 && (int64_t)e.N + e.M - 1 > steps_max) steps_max = (int64_t)e.N + e.M - 1;
    }
    std::stable_sort(list.begin(), list.end(), [](const sk_band_entry &u, const sk_band_entry &v) {
        return (int64_t)u.N + u.M > (int64_t)v.N + v.M;
    });
    const int64_t steps = steps_max > 0 ? steps_max : 1;
    const int64_t dir_words = ((steps * K + 15) / 16) * 64;
    const int64_t slab_words = dir_words + 2 * ((steps + 63) / 64) + 2;
    const int per_cu = K == 1 ? resident_band<1>(paths) : K == 2 ? resident_band<2>(paths) : resident_band<4>(paths);
    int64_t waves = (int64_t)(per_cu < 32 ? per_cu : 32) * c->num_cu;
    if (waves < 1) waves = 1;
    if (paths) {
        if (slab_words * 4 > BAND_SLAB_BUDGET)
            return sk_fail(SK_ERR_NOMEM, "band: a slab of %lld bytes above the budget of %lld", (long long)(slab_words * 4), (long long)BAND_SLAB_BUDGET);
        waves = std::min(waves, BAND_SLAB_BUDGET / (slab_words * 4));
    }
    if (const char *s = sk_tune("SK_BAND_WAVES")) { const long long v = atoll(s); if (v > 0 && v < waves) waves = v; }
    if (waves > npairs) waves = npairs;
    if ((rc = sk_reserve(c, &c->band, (size_t)npairs * sizeof(sk_band_entry)))) return rc;
    if (paths) {
        if ((rc = sk_reserve(c, &c->bandslab, (size_t)waves * (size_t)slab_words * 4))) return rc;
        if ((rc = sk_path_begin(c))) return rc;
    }
    c->band_table.swap(list);
    c->band_slab_bytes = paths ? slab_words * 4 : 0; c->band_waves = waves; c->band_steps = steps_max;
    SK_HIP(hipMemcpyAsync(c->band.p, c->band_table.data(), (size_t)npairs * sizeof(sk_band_entry), hipMemcpyHostToDevice, c->stream));

    band_kargs k;
    k.values = d_values; k.tab = (const sk_band_entry *)c->band.p; k.rec = d_rec; k.spans = d_spans;
    k.npairs = (int)npairs; k.free_end = end_mode == SK_BAND_FREE;
    k.mism = paths ? (int32_t *)c->pathcnt.p : nullptr;
    k.slab = paths ? (uint32_t *)c->bandslab.p : nullptr; k.slab_words = slab_words; k.dir_words = dir_words;
    SK_HIP(hipEventRecord(c->ev[0], c->stream));            // (no prep kernels: sk_last_kernel_ms reports 0 for them)
    SK_HIP(hipEventRecord(c->ev[1], c->stream));
    SK_HIP(hipEventRecord(c->ev[2], c->stream));
    if (K == 1) launch_band<1>(k, paths, waves, c->stream);
    else if (K == 2) launch_band<2>(k, paths, waves, c->stream);
    else launch_band<4>(k, paths, waves, c->stream);
    SK_HIP(hipGetLastError());
    SK_HIP(hipEventRecord(c->ev[3], c->stream));
    c->last_retry = 0; c->retry_dev = false; c->prof_chunks = 0;
    c->ev_valid = true;
    return SK_OK;
}
