"""The definition of the signal HMM's posteriors, stated in numpy (a helper, not a test).

Model, samples, calibration, limit and the emission e_j(x) = max(a_0, a_1) are hmm_ref's.  Every operation below is one
correctly rounded float64 operation in the order written; constants are given by their bit patterns.

sk_exp(d):  0.0 unless d >= -700.0 (this covers -inf); else k = rint(d * LOG2E), r = (d - k * LN2_HI) - k * LN2_LO,
            p = C13, p = p * r + Cq for q = 12 .. 0 (Cq = the double nearest 1 / q!), result = ldexp(p, int(k)).
sk_log(s), 1 <= s < 8:  f = s, k = 0; three times: if f > SQRT2: f = f * 0.5, k = k + 1;  z = (f - 1.0) / (f + 1.0),
            z2 = z * z, p = D23, p = p * z2 + Dq for q = 21, 19, .. 1 (Dq = the double nearest 1 / q),
            result = k * LN2 + (z + z) * p.
lse(c_0 ..): m = the maximum in rising index by `>`; -inf if m == -inf; else s = 0.0, s = s + sk_exp(c_i - m) in rising i;
            result = m + sk_log(s).
Forward:    alpha_j(0) = linit[j] + e_j(x_0); alpha_j(t) = lse_i(alpha_i(t-1) + ltrans[i][j]) + e_j(x_t); L = lse_j alpha_j(n-1)
Backward:   beta_i(n-1) = 0.0; u_ij(t) = ltrans[i][j] + (e_j(x_{t+1}) + beta_j(t+1)); beta_i(t) = lse_j u_ij(t)
Posteriors: gamma_j(t) = sk_exp((alpha_j(t) + beta_j(t)) - L); xi_ij(t) = sk_exp((alpha_i(t) + u_ij(t)) - L), t <= n - 2
Records:    POST_DTYPE (loglik = L, n_used, flags, final_post = gamma(n-1), occ[j] += gamma_j(t) for falling t) and
            COUNTS_DTYPE (for falling t, m = 1 when a_1 > a_0 for state j at x_t: n[j][m] += gamma, sx[j][m] += gamma * x,
            sxx[j][m] += gamma * (x * x); xi[i][j] += xi_ij(t) for falling t; init[j] = gamma_j(0)); every sum from 0.0.
Dense:      gamma[goff[r] + t, j] = gamma_j(t), 0.0 for j >= S, goff = the running sum of n_used.
n = 0: all 0.  L == -inf: loglik -inf, flags IMPOSSIBLE, every probability and count 0.0.

The reads of a batch are advanced together (arrays [R, ..]); every read's arithmetic is the statement above, element by
element.
"""
import numpy as np

from hmm_ref import model_arrays

STATES = 6
IMPOSSIBLE = 1
POST_DTYPE = np.dtype([("loglik", "<f8"), ("n_used", "<i4"), ("flags", "<i4"), ("final_post", "<f8", (STATES,)),
                       ("occ", "<f8", (STATES,))])
COUNTS_DTYPE = np.dtype([("n", "<f8", (STATES, 2)), ("sx", "<f8", (STATES, 2)), ("sxx", "<f8", (STATES, 2)),
                         ("xi", "<f8", (STATES, STATES)), ("init", "<f8", (STATES,))])


def _f64(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


LOG2E, LN2_HI, LN2_LO = _f64(0x3FF71547652B82FE), _f64(0x3FE62E42FEE00000), _f64(0x3DEA39EF35793C76)
EXP_C = [_f64(b) for b in (0x3FF0000000000000, 0x3FF0000000000000, 0x3FE0000000000000, 0x3FC5555555555555,
                           0x3FA5555555555555, 0x3F81111111111111, 0x3F56C16C16C16C17, 0x3F2A01A01A01A01A,
                           0x3EFA01A01A01A01A, 0x3EC71DE3A556C734, 0x3E927E4FB7789F5C, 0x3E5AE64567F544E4,
                           0x3E21EED8EFF8D898, 0x3DE6124613A86D09)]                        # Cq, q = 0 .. 13
SQRT2, LN2 = _f64(0x3FF6A09E667F3BCD), _f64(0x3FE62E42FEFA39EF)
LOG_D = [_f64(b) for b in (0x3FF0000000000000, 0x3FD5555555555555, 0x3FC999999999999A, 0x3FC2492492492492,
                           0x3FBC71C71C71C71C, 0x3FB745D1745D1746, 0x3FB3B13B13B13B14, 0x3FB1111111111111,
                           0x3FAE1E1E1E1E1E1E, 0x3FAAF286BCA1AF28, 0x3FA8618618618618, 0x3FA642C8590B2164)]   # Dq, q = 1, 3 .. 23


def sk_exp(d):
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = d >= -700.0
    dd = np.where(ok, d, 0.0)
    k = np.rint(dd * LOG2E)
    r = (dd - k * LN2_HI) - k * LN2_LO
    p = np.full(d.shape, EXP_C[13])
    for q in range(12, -1, -1):
        p = p * r + EXP_C[q]
    return np.where(ok, np.ldexp(p, k.astype(np.int32)), 0.0)


def sk_log(s):
    s = np.asarray(s, dtype=np.float64)
    f, k = s, np.zeros(s.shape)
    for _ in range(3):
        big = f > SQRT2
        f = np.where(big, f * 0.5, f)
        k = np.where(big, k + 1.0, k)
    z = (f - 1.0) / (f + 1.0)
    z2 = z * z
    p = np.full(s.shape, LOG_D[11])
    for q in range(10, -1, -1):
        p = p * z2 + LOG_D[q]
    return k * LN2 + (z + z) * p


def lse(c, axis):
    """lse over `axis` of c, in rising index along it"""
    c = np.moveaxis(np.asarray(c, dtype=np.float64), axis, 0)
    m = c[0]
    for i in range(1, c.shape[0]):
        m = np.where(c[i] > m, c[i], m)
    s = np.zeros(m.shape)
    with np.errstate(invalid="ignore"):
        for i in range(c.shape[0]):
            s = s + sk_exp(c[i] - m)                    # (m == -inf: NaN -> 0.0, and the sum is dropped below)
        v = m + sk_log(s)
    return np.where(m == -np.inf, -np.inf, v)


def components(c, mu, h, x):
    """(e[.., S], m1[.., S]) of x[..]: the emission and whether component 1 won (a_1 > a_0)"""
    d0 = x[..., None] - mu[:, 0]
    d1 = x[..., None] - mu[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        a0 = c[:, 0] - (d0 * d0) * h[:, 0]
        a1 = c[:, 1] - (d1 * d1) * h[:, 1]
    m1 = a1 > a0
    return np.where(m1, a1, a0), m1


def posterior_rows(model, x, lens, counts=True, dense=True):
    """(post POST_DTYPE [R], counts COUNTS_DTYPE [R] or None, goff int64 [R + 1], gamma float64 [goff[R], 6] or None) of
    the rows x[R, N] (float64, model units), read r = x[r, :lens[r]]"""
    S, linit, ltrans, c, mu, h = model_arrays(model)
    x = np.asarray(x, dtype=np.float64)
    lens = np.asarray(lens, dtype=np.int64)
    R = x.shape[0]
    post = np.zeros(R, dtype=POST_DTYPE)
    post["n_used"] = lens
    cnt = np.zeros(R, dtype=COUNTS_DTYPE)
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    gamma = np.zeros((int(goff[R]), STATES))
    N = int(lens.max(initial=0))
    if N > 0:
        e, m1 = components(c, mu, h, x[:, :N])                       # [R, N, S]
        al = np.full((R, N, S), -np.inf)
        with np.errstate(invalid="ignore"):
            al[:, 0] = linit[None, :] + e[:, 0]
            for t in range(1, N):
                al[:, t] = lse(al[:, t - 1, :, None] + ltrans[None], axis=1) + e[:, t]
        rows = np.arange(R)
        last = np.maximum(lens - 1, 0)
        L = np.where(lens > 0, lse(al[rows, last], axis=1), 0.0)
        live = (L != -np.inf) & (lens > 0)
        Ls = np.where(live, L, 0.0)[:, None]
        post["loglik"] = L
        post["flags"] = np.where(L == -np.inf, IMPOSSIBLE, 0)
        w = np.zeros((R, S))                                         # e_j(x_{t+1}) + beta_j(t+1)
        occ, fpost, ginit = np.zeros((R, S)), np.zeros((R, S)), np.zeros((R, S))
        cn, csx, csxx, cxi = np.zeros((R, S, 2)), np.zeros((R, S, 2)), np.zeros((R, S, 2)), np.zeros((R, S, S))
        for t in range(N - 1, -1, -1):
            act = (lens > t) & live
            end = lens - 1 == t
            with np.errstate(invalid="ignore"):
                u = ltrans[None] + w[:, None, :]                     # [R, from, to]
                be = np.where(end[:, None], 0.0, lse(u, axis=2))
                g = sk_exp((al[:, t] + be) - Ls)
                xi = sk_exp((al[:, t, :, None] + u) - Ls[:, :, None])
            g = np.where(act[:, None], g, 0.0)
            occ = np.where(act[:, None], occ + g, occ)
            fpost = np.where((act & end)[:, None], g, fpost)
            if t == 0:
                ginit = g
            cxi = np.where((act & ~end)[:, None, None], cxi + xi, cxi)
            xt = x[:, t, None]
            for m in (0, 1):
                won = act[:, None] & (m1[:, t] == bool(m))
                cn[:, :, m] = np.where(won, cn[:, :, m] + g, cn[:, :, m])
                csx[:, :, m] = np.where(won, csx[:, :, m] + g * xt, csx[:, :, m])
                csxx[:, :, m] = np.where(won, csxx[:, :, m] + g * (xt * xt), csxx[:, :, m])
            with np.errstate(invalid="ignore"):
                w = np.where((lens > t)[:, None], e[:, t] + be, w)
            on = np.flatnonzero(lens > t)
            gamma[goff[on] + t, :S] = g[on]
        post["final_post"][:, :S], post["occ"][:, :S] = fpost, occ
        cnt["n"][:, :S], cnt["sx"][:, :S], cnt["sxx"][:, :S] = cn, csx, csxx
        cnt["xi"][:, :S, :S], cnt["init"][:, :S] = cxi, ginit
    return post, (cnt if counts else None), goff, (gamma if dense else None)


def _limited(lens, limit):
    return np.minimum(lens, limit) if limit > 0 else lens


def posterior_batch(model, sig, lens, cal2=None, limit=0, counts=True, dense=True):
    """posterior_rows of the int16 rows sig[R, stride] with lengths lens, calibration pairs cal2[R, 2] (or None) and limit"""
    sig = np.asarray(sig)
    lens = _limited(np.clip(np.asarray(lens, dtype=np.int64), 0, sig.shape[1]), limit)
    x = sig.astype(np.float64)
    if cal2 is not None:
        cal2 = np.asarray(cal2, dtype=np.float64).reshape(-1, 2)
        x = (x + cal2[:, :1]) * cal2[:, 1:]
    return posterior_rows(model, x, lens, counts, dense)


def posterior_reads(model, reads, limit=0, counts=True, dense=True):
    """posterior_rows of a list of reads of any lengths (values taken as float64, no calibration)"""
    R = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    x = np.zeros((R, max(1, int(lens.max(initial=0)))), dtype=np.float64)
    for i, r in enumerate(reads):
        x[i, :len(r)] = np.asarray(r, dtype=np.float64)
    return posterior_rows(model, x, _limited(lens, limit), counts, dense)
