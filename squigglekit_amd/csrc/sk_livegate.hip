// sk_livegate.hip -- the gate of a gated live mapping session: the transcript start an HMM session finds decides which
// events reach the bridge (gfx950).
//
// The definition (include/squigglekit_hip.h, "Gated live sessions"; tests/livegate_ref.py restates it on top of
// hmmstream_ref, evstream_ref and live_ref).  sk_live.hip owns the session and the order of a push; here are the three
// kernels it adds between the inner sessions' own.
//
// k_live_gate_len    one lane per named entry, AHEAD of the HMM push: the chunk length the HMM session sees -- len[k] while
//                    the slot is GATING and has not ended, 0 otherwise (a peek: k_hmms_push then leaves the slot as it
//                    stands and returns its record, the record at the decision).
// k_live_gate        one wavefront per named entry, BEHIND both pushes.  Reads the slot's gate record, the entry's
//                    sk_hmms_rec and the event push's staging rows.  While GATING it takes api.polya_decide's rule on the
//                    record -- one float64 subtract and three compares, as k_live_best does map_decide's -- and then
//                    either appends the push's events to the slot's ring (event number e at e % G; only the last G of a
//                    push are stored, so no two lanes store to one entry) or, on the push that opens the gate, releases:
//                    starts rise strictly, so the released events are a suffix of ring-then-new; every lane looks at the
//                    positions lane, lane + 64, .. for the first start >= t0 and a butterfly takes the minimum.  An OPEN
//                    slot runs the same search over the new events alone (an event cut after the decision can still
//                    straddle t0).  The released rows go to rel[k][0 ..], their count to rcnt[k]: k_live_count and
//                    k_live_fill then read them where an ungated session reads the event push's staging rows.
// k_live_gate_reset  the named slots (or all) back to GATING.
//
// The ring entry that a push overwrites LAST is read by lane 0 before any lane stores to the ring; a barrier stands
// between that load and the stores (k_live_count orders its hold buffer the same way).  The released rows are read from
// the ring as earlier pushes left it: the opening push stores nothing to it.  Plain vector stores throughout.
#include "sk_common.h"

namespace {

static_assert(sizeof(sk_live_gate) == 24 && sizeof(sk_live_gate_info) == 32, "sk_live_gate is 24 bytes, sk_live_gate_info 32");
static_assert(sizeof(sk_gate_slot) == 40 && sizeof(sk_det_event) == 24, "a gate slot is 40 bytes, a ring entry 24");
static_assert(SK_LIVE_MAX_GATE_HOLD + SK_LIVE_MAX_CALIB - 1 < SK_MAP_MAX_CHUNK, "a hold ring and a head fit a mapping chunk");

__device__ __forceinline__ sk_gate_slot gate_first()
{
    sk_gate_slot s;
    s.g.state = SK_LIVE_GATE_GATING; s.g.t0 = -1; s.g.decided_n = -1; s.g.events_cut = 0; s.g.released = 0; s.g.ring = 0;
    s.g.dropped = 0; s.g.flags = 0; s.last_drop = -1; s.pad = 0;
    return s;
}

__global__ void k_live_gate_len(const sk_gate_args a, int32_t *__restrict__ hlen)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    const int32_t slot = a.slots[k];
    int32_t l = 0;
    if (slot >= 0 && slot < a.nslots && a.state[slot].g.state == SK_LIVE_GATE_GATING && a.live[slot].ended == 0) l = a.len[k];
    hlen[k] = l;
}

// api.polya_decide's accept, `state` in place of TRANSCRIPT
// (the record stays in memory: v[state] and enter[state] are loads at a computed address, not a register array indexed
// at run time, which would go to scratch)
__device__ __forceinline__ bool gate_accept(const sk_hmms_rec *r, const sk_live_gate &rule, int32_t &enter_s)
{
    const int s = rule.state;
    double others = -__builtin_inf();
    bool nan = false;
#pragma unroll
    for (int j = 0; j < SK_HMM_STATES; j++) {
        const double v = r->v[j];
        if (j == s) continue;
        if (v != v) nan = true;
        if (v > others) others = v;
    }
    const double margin = r->v[s] - others;                 // (-inf - -inf = NaN: no margin, the test fails)
    enter_s = r->enter[s];
    return r->final_state == s && r->n_used - enter_s >= rule.min_body && !nan && margin >= rule.min_margin;
}

__global__ __launch_bounds__(64)
void k_live_gate(const sk_gate_args a)
{
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (k >= a.m) return;
    const int32_t slot = a.slots[k];
    if (slot < 0 || slot >= a.nslots) {                     // (never: both entry points check the slot numbers)
        if (lane == 0) { a.rcnt[k] = 0; a.ginfo[k] = gate_first().g; }
        return;
    }
    sk_gate_slot st = a.state[slot];
    int64_t n64 = a.eoff[k + 1] - a.eoff[k];
    if (n64 < 0) n64 = 0;
    if (n64 > a.per) n64 = a.per;
    const int32_t n = (int32_t)n64, G = a.G;
    const sk_det_event *mine = a.stage + k * a.per;
    sk_det_event *ring = a.ring + (int64_t)slot * G;
    sk_det_event *out = a.rel + k * ((int64_t)G + a.per);
    const bool was_gating = st.g.state == SK_LIVE_GATE_GATING;
    int32_t count = 0;

    if (was_gating) {
        const sk_hmms_rec *r = a.hrec + k;
        const int32_t n_used = r->n_used;
        int32_t enter_s = -1;
        if (gate_accept(r, a.rule, enter_s)) {
            st.g.state = SK_LIVE_GATE_OPEN; st.g.t0 = enter_s; st.g.decided_n = n_used;
        } else if (a.rule.give_up > 0 && n_used >= a.rule.give_up) {
            st.g.state = SK_LIVE_GATE_REJECTED; st.g.decided_n = n_used;
        } else if (a.end && a.end[k] != 0) {
            st.g.state = SK_LIVE_GATE_REJECTED; st.g.decided_n = n_used; st.g.flags |= SK_LIVE_GATE_ENDED;
        }
    }

    if (st.g.state == SK_LIVE_GATE_OPEN) {
        // ring-then-new (an OPEN slot's ring is empty): position q < held is event number first + q of the slot
        const int32_t held = was_gating ? st.g.ring : 0, first = st.g.events_cut - held, total = held + n, t0 = st.g.t0;
        auto at = [&](int32_t q) -> const sk_det_event & { return q < held ? ring[(first + q) % G] : mine[q - held]; };
        int32_t f = total;
        for (int32_t q = lane; q < total; q += 64)
            if (at(q).start >= t0) { f = q; break; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int32_t v = __shfl_xor(f, o); f = v < f ? v : f; }
        count = total - f;
        for (int32_t j = lane; j < count; j += 64) out[j] = at(f + j);
        if (was_gating && st.g.dropped > 0 && st.last_drop >= t0) st.g.flags |= SK_LIVE_GATE_TRUNCATED;
        st.g.ring = 0;
    } else if (st.g.state == SK_LIVE_GATE_GATING) {
        // event number e -> ring[e % G]; only the last G of the push are stored
        const int64_t all = (int64_t)st.g.events_cut + n;
        if (all > G && n > 0) {
            const int64_t last = all - G - 1;               // the number of the event overwritten last
            int32_t ld = 0;
            if (lane == 0) ld = last >= st.g.events_cut ? mine[last - st.g.events_cut].start : ring[last % G].start;
            st.last_drop = __shfl(ld, 0);
            st.g.dropped = (int32_t)(all - G);
        }
        __syncthreads();                                    // lane 0 has read the ring before any lane stores to it
        const int32_t j0 = n > G ? n - G : 0;
        for (int32_t j = j0 + lane; j < n; j += 64) ring[((int64_t)st.g.events_cut + j) % G] = mine[j];
        st.g.ring = (int32_t)(all < G ? all : G);
    } else {
        st.g.ring = 0;
    }
    st.g.events_cut += n;
    st.g.released += count;
    if (lane == 0) { a.state[slot] = st; a.ginfo[k] = st.g; a.rcnt[k] = count; }
}

__global__ void k_live_gate_reset(sk_gate_slot *state, int32_t nslots, const int32_t *slots, int32_t m)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m) return;
    const int32_t s = slots ? slots[idx] : idx;
    if (s < 0 || s >= nslots) return;
    state[s] = gate_first();
}

} // namespace

int sk_livegate_reset(sk_ctx *c, sk_gate_slot *state, int32_t nslots, const int32_t *d_slots, int32_t m)
{
    if (m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_live_gate_reset, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, state, nslots, d_slots, m);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_livegate_lengths(sk_ctx *c, const sk_gate_args &a, int32_t *d_hlen)
{
    if (a.m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_live_gate_len, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, c->stream, a, d_hlen);
    SK_HIP(hipGetLastError());
    return SK_OK;
}

int sk_livegate_release(sk_ctx *c, const sk_gate_args &a)
{
    if (a.m <= 0) return SK_OK;
    hipLaunchKernelGGL(k_live_gate, dim3((unsigned)a.m), dim3(64), 0, c->stream, a);
    SK_HIP(hipGetLastError());
    return SK_OK;
}
