// sk_select_dev.h -- exact rank selection on one wavefront: np.median's two middle values by a radix select over 64-bit
// keys (device code shared by the read background, sk_bg.hip, and the segment levels, sk_seglev.hip; the scheme is
// described at the head of sk_bg.hip).  Needs sk_prepw_dev.h (wave_incl_scan, bcast_from).
#pragma once

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_min_u64(u64 v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 q = __shfl_xor(v, o); v = q < v ? q : v; }
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 q = __shfl_xor(v, o); v = q > v ? q : v; }
    return v;
}

// The keys of rank k1 and k2 (k1 <= k2 <= k1 + 1, 0-based, ascending) among key(0) .. key(n - 1); keys have bit 63 clear
// unless FULL (any 64-bit key: values of either sign through key_of_double).
// The wavefront is the whole workgroup: __syncthreads orders its LDS traffic.  Every lane returns both keys.
template <bool FULL = false, typename Key>
__device__ __forceinline__ void wave_select2(int n, int k1, int k2, unsigned *hist, int lane, Key key, u64 &ka, u64 &kb)
{
    u64 lo = ~0ull, hi = 0ull;
    for (int j = lane; j < n; j += 64) { const u64 k = key(j); lo = k < lo ? k : lo; hi = k > hi ? k : hi; }
    lo = wave_min_u64(lo); hi = wave_max_u64(hi);
    if (lo == hi) { ka = kb = lo; return; }
    int top = 64 - __clzll((long long)(lo ^ hi));        // the keys agree on the bits [top, 64)
    if (!FULL && top > 63) top = 63;                     // (bit 63 is clear in every key)
    u64 prefix = top > 63 ? 0ull : (hi >> top) << top;   // (top == 64: the keys differ in bit 63, no bit is settled)
    int kk = k1, cnt = n, below = 0;                     // rank inside / size of / keys below the matching set
    while (top > 0 && cnt > 1) {                         // (wave-uniform)
        const int sh = top > 8 ? top - 8 : 0;
        const unsigned dm = (1u << (top - sh)) - 1u;
        *(uint4 *)(hist + 4 * lane) = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (int j = lane; j < n; j += 64) {
            const u64 k = key(j);
            if ((FULL && top > 63) || ((k ^ prefix) >> top) == 0ull) atomicAdd(&hist[(unsigned)(k >> sh) & dm], 1u);
        }
        __syncthreads();
        const uint4 q = *(const uint4 *)(hist + 4 * lane);
        const int c[4] = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
        const int local = c[0] + c[1] + c[2] + c[3];
        const int pre = wave_incl_scan(local) - local;
        const u64 own = __ballot(local > 0 && kk >= pre && kk < pre + local);
        int acc = pre, bin = 4 * lane, cin = 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!found) {
                if (kk < acc + c[i]) { cin = c[i]; found = true; }
                else { acc += c[i]; bin++; }
            }
        }
        const int src = own ? (int)__builtin_ctzll(own) : 0;
        bin = bcast_from(bin, src); acc = bcast_from(acc, src); cin = bcast_from(cin, src);
        prefix |= (u64)(unsigned)bin << sh;
        below += acc; kk -= acc; cnt = cin; top = sh;
        __syncthreads();                                 // the counts are read before the next pass clears them
    }
    // the matching set is one key (top > 0) or cnt equal keys (top == 0: the prefix is the key)
    const bool need_b = k2 != k1 && k2 >= below + cnt;
    u64 fa = prefix, gt = ~0ull;
    if (top > 0 || need_b) {
        const u64 pp = prefix >> top;
        fa = 0ull;
        for (int j = lane; j < n; j += 64) {
            const u64 k = key(j), hp = k >> top;
            if (hp == pp) fa = k;
            else if (hp > pp && k < gt) gt = k;
        }
        fa = wave_max_u64(fa); gt = wave_min_u64(gt);
    }
    ka = fa; kb = need_b ? gt : fa;
}

// A float64 as a key whose unsigned order is the order of the values (either sign; -0.0 sorts below 0.0), and back
__device__ __forceinline__ u64 key_of_double(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double double_of_key(u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k));
}

// np.median's value from the two middle keys: one key for an odd n, np.mean of the two otherwise
__device__ __forceinline__ double median_of(u64 ka, u64 kb, bool even)
{
    const double a = __longlong_as_double((long long)ka), b = __longlong_as_double((long long)kb);
    return even ? (a + b) / 2.0 : a;
}

