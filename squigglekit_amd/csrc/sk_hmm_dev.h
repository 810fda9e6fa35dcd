// sk_hmm_dev.h -- the device text of the signal HMM that the one-shot kernels (sk_hmm.hip) and the HMM sessions
// (sk_hmmstream.hip) share: the model as a kernel takes it, the LDS tile of a wavefront's 64 rows, the emission, and the
// recurrence's step without back pointers.  One text, so that a session's scores and tuples are the one-shot call's by
// construction.  The definition: include/squigglekit_hip.h, "signal HMM".
#pragma once
#include "sk_common.h"

namespace {

constexpr int HS = SK_HMM_STATES;

template <int FEED> struct hmm_feed;
template <> struct hmm_feed<SK_FEED_I16> {
    typedef int16_t T;
    static constexpr int TILE = 128;              // samples per row and load round
    static constexpr int PITCH = TILE / 2 + 1;    // dwords per row in LDS (odd: lane l at position j -> bank (l + j / 2) mod 32)
};
template <> struct hmm_feed<SK_FEED_F64_NORM> {
    typedef double T;
    static constexpr int TILE = 32;
    static constexpr int PITCH = TILE * 2 + 2;    // lane l at position j -> dwords 66 l + 2 j, + 1: bank pair 2 (l + j) mod 64
};

// the model as the kernel takes it: flat arrays, and which transitions / second components are not -inf
struct hmm_kmodel {
    double   linit[HS];
    double   ltrans[HS * HS];     // [from * 6 + to]
    double   c[HS * 2], mu[HS * 2], h[HS * 2];
    uint64_t tmask;               // bit from * 6 + to: ltrans is not -inf
    uint32_t cmask;               // bit j: component 1 of state j is not -inf
    int32_t  S;
};

// tile k of the wavefront's 64 rows -> LDS; row `row` holds its samples [k * TILE, min((k + 1) * TILE, nrow[row])).
// int16: row r0 + row starts at sig + (r0 + row) * stride (vec: base and stride are 16-byte aligned); float64: at
// sig + off[r0 + row].  A row with nrow == 0 is not touched, and neither is its off entry.
template <int FEED>
__device__ __forceinline__ void hmm_load_tile(const void *sigv, int64_t stride, const int64_t *off, int32_t vec, uint32_t *tile,
                                              const int32_t *nrow, int64_t r0, int k, int lane)
{
    constexpr int TILE = hmm_feed<FEED>::TILE, PITCH = hmm_feed<FEED>::PITCH;
    if (FEED == SK_FEED_I16) {
        const int16_t *sig = (const int16_t *)sigv;
        if (vec) {
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int row = it * 4 + (lane >> 4);
                const int32_t pos = k * TILE + (lane & 15) * 8;
                if (pos < nrow[row]) {                          // (a row of the batch: nrow is 0 past nreads)
                    const uint4 v = *(const uint4 *)(sig + (r0 + row) * stride + pos);
                    uint32_t *dst = tile + row * PITCH + ((lane & 15) * 4);
                    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
                }
            }
        } else {
            // Knowingly slow: 2-byte loads, 128 bytes per load instruction, one row after the other.  Taken only when the
            // base or the stride breaks the 16-byte alignment; the loop over samples, not this one, bounds the kernel.
            int16_t *t16 = (int16_t *)tile;
            for (int row = 0; row < 64; row++) {
                const int32_t nr = nrow[row];
                for (int cc = lane; cc < TILE; cc += 64) {
                    const int32_t pos = k * TILE + cc;
                    if (pos < nr) t16[row * (2 * PITCH) + cc] = sig[(r0 + row) * stride + pos];
                }
            }
        }
    } else {
        const double *sig = (const double *)sigv;
#pragma unroll 4
        for (int it = 0; it < 32; it++) {
            const int row = it * 2 + (lane >> 5);
            const int32_t pos = k * TILE + (lane & 31);
            if (pos < nrow[row]) {
                const double v = sig[off[r0 + row] + pos];
                *(double *)(tile + row * PITCH + (lane & 31) * 2) = v;
            }
        }
    }
}

__device__ __forceinline__ double hmm_emit(const hmm_kmodel &m, int j, double x)
{
    const double d0 = x - m.mu[2 * j];
    double e = m.c[2 * j] - (d0 * d0) * m.h[2 * j];
    if ((m.cmask >> j) & 1u) {
        const double d1 = x - m.mu[2 * j + 1];
        const double e1 = m.c[2 * j + 1] - (d1 * d1) * m.h[2 * j + 1];
        if (e1 > e) e = e1;
    }
    return e;
}

// t == 0: v_j = linit[j] + e_j(x), enter_j[j] = 0 (v and E come in as -inf and -1)
__device__ __forceinline__ void hmm_first(const hmm_kmodel &m, int S, double x, double (&v)[HS], int32_t (&E)[HS][HS])
{
#pragma unroll
    for (int j = 0; j < HS; j++)
        if (j < S) { v[j] = m.linit[j] + hmm_emit(m, j, x); E[j][j] = 0; }
}

// t >= 1: v and E of sample t - 1 -> of sample t.  Predecessor 0 is always taken; a transition of -inf and a state at or
// above S is skipped by a scalar branch on the masks (exact: see sk_hmm.hip).
__device__ __forceinline__ void hmm_step(const hmm_kmodel &m, int S, double x, int32_t t, double (&v)[HS], int32_t (&E)[HS][HS])
{
    const double ninf = -__builtin_inf();
    double nv[HS];
    int32_t NE[HS][HS];
#pragma unroll
    for (int j = 0; j < HS; j++) {
        nv[j] = ninf;
#pragma unroll
        for (int q = 0; q < HS; q++) NE[j][q] = -1;
        if (j < S) {
            double b = v[0] + m.ltrans[j];                      // predecessor 0: always taken
#pragma unroll
            for (int q = 0; q < HS; q++) NE[j][q] = E[0][q];
#pragma unroll
            for (int i = 1; i < HS; i++)
                if (i < S && ((m.tmask >> (i * HS + j)) & 1ull)) {
                    const double cand = v[i] + m.ltrans[i * HS + j];
                    const bool w = cand > b;
                    b = w ? cand : b;
#pragma unroll
                    for (int q = 0; q < HS; q++) NE[j][q] = w ? E[i][q] : NE[j][q];
                }
            NE[j][j] = NE[j][j] < 0 ? t : NE[j][j];
            nv[j] = b + hmm_emit(m, j, x);
        }
    }
#pragma unroll
    for (int j = 0; j < HS; j++) {
        v[j] = nv[j];
#pragma unroll
        for (int q = 0; q < HS; q++) E[j][q] = NE[j][q];
    }
}

// the lowest j with the largest v_j, its score and its tuple -> the 40 bytes of sk_hmm_rec (n > 0)
__device__ __forceinline__ void hmm_result(int S, const double (&v)[HS], const int32_t (&E)[HS][HS], double &score, int32_t &f,
                                           int32_t (&en)[HS])
{
    double best = v[0];
    f = 0;
#pragma unroll
    for (int q = 0; q < HS; q++) en[q] = E[0][q];
#pragma unroll
    for (int j = 1; j < HS; j++)
        if (j < S) {
            const bool w = v[j] > best;
            best = w ? v[j] : best;
            f = w ? j : f;
#pragma unroll
            for (int q = 0; q < HS; q++) en[q] = w ? E[j][q] : en[q];
        }
    score = best;
}

// host: the kernel's model of a checked sk_hmm_model
inline hmm_kmodel hmm_flatten(const sk_hmm_model *m)
{
    hmm_kmodel k;
    const double ninf = -__builtin_inf();
    const int S = m->nstates;
    k.S = S; k.tmask = 0; k.cmask = 0;
    for (int i = 0; i < HS; i++) {
        const bool in = i < S;
        k.linit[i] = in ? m->linit[i] : ninf;
        for (int j = 0; j < HS; j++) {
            const double lt = (in && j < S) ? m->ltrans[i][j] : ninf;
            k.ltrans[i * HS + j] = lt;
            if (lt != ninf) k.tmask |= 1ull << (i * HS + j);
        }
        for (int q = 0; q < 2; q++) {
            k.c[2 * i + q] = in ? m->c[i][q] : ninf;
            k.mu[2 * i + q] = in ? m->mu[i][q] : 0.0;
            k.h[2 * i + q] = in ? m->h[i][q] : 0.0;
        }
        if (k.c[2 * i + 1] != ninf) k.cmask |= 1u << i;
    }
    return k;
}

} // namespace
