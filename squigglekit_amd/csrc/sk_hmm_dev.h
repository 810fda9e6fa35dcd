// sk_hmm_dev.h -- the device text of the signal HMM that the one-shot kernels (sk_hmm.hip) and the HMM sessions
// (sk_hmmstream.hip) share: the model as a kernel takes it, the LDS tile of a wavefront's 64 rows, the emission, and the
// recurrence's step without back pointers; and the text of the posteriors that sk_hmm_post.hip and a filtered session
// share: sk_exp, sk_log, the log-sum-exp and the forward step.  One text, so that a session's scores, tuples and alpha are
// the one-shot calls' by construction.  The definition: include/squigglekit_hip.h, "signal HMM" and "signal HMM: posteriors".
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

// ---- the sums of probabilities (signal HMM: posteriors) that the one-shot kernels (sk_hmm_post.hip) and a
// filtered HMM session (sk_hmmstream.hip) share: one text, so that a session's alpha is the one-shot call's by construction.
#define SK_F64(bits) __longlong_as_double((long long)(bits))

// The constants of sk_exp and sk_log by their bit patterns (include/squigglekit_hip.h and tests/hmm_post_ref.py state the
// same ones; sk_hmm_post.hip pins them with static_asserts).  SK_EXP_Cq: the double nearest 1 / q!; SK_LOG_Dq: the double
// nearest 1 / q.
#define SK_LOG2E  0x3FF71547652B82FEull
#define SK_LN2_HI 0x3FE62E42FEE00000ull
#define SK_LN2_LO 0x3DEA39EF35793C76ull
#define SK_SQRT2  0x3FF6A09E667F3BCDull
#define SK_LN2    0x3FE62E42FEFA39EFull
#define SK_EXP_C0  0x3FF0000000000000ull
#define SK_EXP_C1  0x3FF0000000000000ull
#define SK_EXP_C2  0x3FE0000000000000ull
#define SK_EXP_C3  0x3FC5555555555555ull
#define SK_EXP_C4  0x3FA5555555555555ull
#define SK_EXP_C5  0x3F81111111111111ull
#define SK_EXP_C6  0x3F56C16C16C16C17ull
#define SK_EXP_C7  0x3F2A01A01A01A01Aull
#define SK_EXP_C8  0x3EFA01A01A01A01Aull
#define SK_EXP_C9  0x3EC71DE3A556C734ull
#define SK_EXP_C10 0x3E927E4FB7789F5Cull
#define SK_EXP_C11 0x3E5AE64567F544E4ull
#define SK_EXP_C12 0x3E21EED8EFF8D898ull
#define SK_EXP_C13 0x3DE6124613A86D09ull
#define SK_LOG_D1  0x3FF0000000000000ull
#define SK_LOG_D3  0x3FD5555555555555ull
#define SK_LOG_D5  0x3FC999999999999Aull
#define SK_LOG_D7  0x3FC2492492492492ull
#define SK_LOG_D9  0x3FBC71C71C71C71Cull
#define SK_LOG_D11 0x3FB745D1745D1746ull
#define SK_LOG_D13 0x3FB3B13B13B13B14ull
#define SK_LOG_D15 0x3FB1111111111111ull
#define SK_LOG_D17 0x3FAE1E1E1E1E1E1Eull
#define SK_LOG_D19 0x3FAAF286BCA1AF28ull
#define SK_LOG_D21 0x3FA8618618618618ull
#define SK_LOG_D23 0x3FA642C8590B2164ull

// sk_exp(d), d <= 0 (or a rounding error above): 0.0 unless d >= -700.0; else k = rint(d * LOG2E), r = (d - k * LN2_HI)
// - k * LN2_LO, a degree-13 Horner sum of r with the doubles nearest 1 / q!, scaled by 2^k.  No result is subnormal.
__device__ __forceinline__ double sk_exp(double d)
{
    const bool ok = d >= -700.0;                                // false for -inf (and for a NaN, which never comes)
    const double dd = ok ? d : 0.0;
    const double k = rint(dd * SK_F64(SK_LOG2E));               // round half to even
    const double r = (dd - k * SK_F64(SK_LN2_HI)) - k * SK_F64(SK_LN2_LO);
    double p = SK_F64(SK_EXP_C13);                              // 1 / 13!
    p = p * r + SK_F64(SK_EXP_C12);
    p = p * r + SK_F64(SK_EXP_C11);
    p = p * r + SK_F64(SK_EXP_C10);
    p = p * r + SK_F64(SK_EXP_C9);
    p = p * r + SK_F64(SK_EXP_C8);
    p = p * r + SK_F64(SK_EXP_C7);
    p = p * r + SK_F64(SK_EXP_C6);
    p = p * r + SK_F64(SK_EXP_C5);
    p = p * r + SK_F64(SK_EXP_C4);
    p = p * r + SK_F64(SK_EXP_C3);
    p = p * r + SK_F64(SK_EXP_C2);
    p = p * r + SK_F64(SK_EXP_C1);
    p = p * r + SK_F64(SK_EXP_C0);
    const double v = ldexp(p, (int)k);
    return ok ? v : 0.0;
}

// sk_log(s), 1 <= s < 8: three conditional halvings bring f into (sqrt(1/2), sqrt(2)], then 2 atanh((f - 1) / (f + 1)) as a
// Horner sum in z^2 with the doubles nearest 1 / q, q = 23, 21, .., 1.  The division is the IEEE one.
__device__ __forceinline__ double sk_log(double s)
{
    const double SQRT2 = SK_F64(SK_SQRT2);
    double f = s, k = 0.0;
#pragma unroll
    for (int it = 0; it < 3; it++) {
        const bool big = f > SQRT2;
        f = big ? f * 0.5 : f;
        k = big ? k + 1.0 : k;
    }
    const double z = (f - 1.0) / (f + 1.0);
    const double z2 = z * z;
    double p = SK_F64(SK_LOG_D23);                              // 1 / 23
    p = p * z2 + SK_F64(SK_LOG_D21);
    p = p * z2 + SK_F64(SK_LOG_D19);
    p = p * z2 + SK_F64(SK_LOG_D17);
    p = p * z2 + SK_F64(SK_LOG_D15);
    p = p * z2 + SK_F64(SK_LOG_D13);
    p = p * z2 + SK_F64(SK_LOG_D11);
    p = p * z2 + SK_F64(SK_LOG_D9);
    p = p * z2 + SK_F64(SK_LOG_D7);
    p = p * z2 + SK_F64(SK_LOG_D5);
    p = p * z2 + SK_F64(SK_LOG_D3);
    p = p * z2 + SK_F64(SK_LOG_D1);
    return k * SK_F64(SK_LN2) + (z + z) * p;
}

// lse of the candidates c[i] whose bit is set in `mask` (wave uniform; a candidate left out is -inf, see the head of the
// file): m = the maximum in rising i by `>`, -inf if that is -inf, else m + sk_log(sum of sk_exp(c[i] - m) in rising i).
// Where m is -inf the differences are NaN, sk_exp answers 0.0 and the sum is dropped.
__device__ __forceinline__ double post_lse(const double (&c)[HS], uint32_t mask)
{
    const double ninf = -__builtin_inf();
    double m = ninf;
#pragma unroll
    for (int i = 0; i < HS; i++)
        if ((mask >> i) & 1u) m = c[i] > m ? c[i] : m;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < HS; i++)
        if ((mask >> i) & 1u) s = s + sk_exp(c[i] - m);
    const double v = m + sk_log(s);
    return m == ninf ? ninf : v;
}

// alpha of sample t - 1 -> of sample t (t >= 1)
__device__ __forceinline__ void post_fwd_step(const hmm_kmodel &m, int S, double x, double (&al)[HS])
{
    const double ninf = -__builtin_inf();
    double na[HS];
#pragma unroll
    for (int j = 0; j < HS; j++) {
        na[j] = ninf;
        if (j < S) {
            double c[HS];
            uint32_t mask = 0;
#pragma unroll
            for (int i = 0; i < HS; i++) {
                c[i] = ninf;
                if (i < S && ((m.tmask >> (i * HS + j)) & 1ull)) { c[i] = al[i] + m.ltrans[i * HS + j]; mask |= 1u << i; }
            }
            na[j] = post_lse(c, mask) + hmm_emit(m, j, x);
        }
    }
#pragma unroll
    for (int j = 0; j < HS; j++) al[j] = na[j];
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
