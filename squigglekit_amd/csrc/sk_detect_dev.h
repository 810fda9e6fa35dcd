// sk_detect_dev.h -- the device text of event detection that the one-shot kernels (sk_detect.hip) and the event sessions
// (sk_evstream.hip) share: a detector's window sums and peak state, t_w[i] from the sums, the detector's step and the
// slide of the sums from position i to i + 1.  One text, so that a session's marks are the one-shot call's by
// construction.  The definition: include/squigglekit_hip.h, "event detection".
#pragma once
#include "sk_common.h"

namespace {

constexpr int DET_TILE = 128;                 // samples per row and load round
constexpr int DET_LAG = 64;                   // = the largest window: positions a lane stays behind the newest sample
constexpr int DET_RING = 2 * DET_TILE;        // samples of a row kept in LDS
constexpr int DET_PITCH = DET_RING / 2 + 1;   // dwords per row in LDS (odd: lane l at position j -> bank (l + j / 2) mod 32)

static_assert(DET_LAG <= DET_TILE / 2 && DET_LAG >= 64, "the ring holds [i - 64, i + 64] of every position in flight");

// one detector: its window sums at the lane's position and its peak state
struct det_state {
    int32_t  w, half;
    double   th;
    int32_t  A, B;               // sum x[i-w..i), sum x[i..i+w)   (samples outside the read count as 0)
    int64_t  Q;                  // their sums of squares together
    int32_t  pos, masked_to;
    double   val;
    bool     valid;
};

__device__ __forceinline__ void det_init(det_state &d, int32_t w, double th)
{
    d.w = w; d.half = w / 2; d.th = th;
    d.A = 0; d.B = 0; d.Q = 0;
    d.pos = -1; d.masked_to = -1; d.val = __builtin_inf(); d.valid = false;
}

// t_w[i] from the sums at position i
__device__ __forceinline__ double det_t(const det_state &d, int32_t i, int32_t n)
{
    if (i < d.w || i > n - d.w) return 0.0;
    const int64_t dd = (int64_t)(d.B - d.A);
    int64_t v = (int64_t)d.w * d.Q - (int64_t)d.A * (int64_t)d.A - (int64_t)d.B * (int64_t)d.B;
    if (v < 1) v = 1;
    const int64_t num = dd * dd * (int64_t)d.w;
    return sqrt((double)num / (double)v);
}

// the detector's step at position i with cur = t[i]; `lng`: the long detector a live short peak silences (nullptr for
// the long detector itself); mark(p): what the caller does with a marked position
template <class Mark>
__device__ __forceinline__ void det_step(det_state &d, det_state *lng, double h, int32_t i, double cur, Mark &&mark)
{
    if (d.pos == -1) {
        if (cur < d.val) d.val = cur;
        else if (cur - d.val > h) { d.val = cur; d.pos = i; }
    } else {
        if (cur > d.val) { d.val = cur; d.pos = i; }
        if (lng && d.val > d.th) {
            lng->masked_to = d.pos + d.w;
            lng->pos = -1; lng->val = __builtin_inf(); lng->valid = false;
        }
        if (d.val - cur > h && d.val > d.th) d.valid = true;
        if (d.valid && i - d.pos > d.half) {
            mark(d.pos);
            d.pos = -1; d.val = cur; d.valid = false;
        }
    }
}

// the sums move from position i to i + 1; xrow: the lane's row of the ring, n: the samples known (those at and beyond
// n count as 0)
__device__ __forceinline__ void det_slide(det_state &d, const int16_t *xrow, int32_t i, int32_t n, int32_t xi)
{
    const int32_t jo = i - d.w, jn = i + d.w;
    const int32_t xo = jo >= 0 ? (int32_t)xrow[jo & (DET_RING - 1)] : 0;
    const int32_t xn = jn < n ? (int32_t)xrow[jn & (DET_RING - 1)] : 0;
    d.A += xi - xo;
    d.B += xn - xi;
    d.Q += (int64_t)(xn * xn - xo * xo);
}

} // namespace
