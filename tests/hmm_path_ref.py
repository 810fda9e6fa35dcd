"""The definition of the signal HMM's state paths, stated in numpy (a helper, not a test).

Model, samples, emission, recurrence and tie rules are hmm_ref's (the forward arithmetic is imported from it).  Added:

Back pointer: for t >= 1 and j < S, arg_j(t) = the predecessor i that won b_j at t (the lowest i wins ties, also at -inf).
Path:         s(n-1) = f, the record's final_state; s(t-1) = arg_{s(t)}(t).
Segments:     the maximal runs of equal s(t), in rising start; a read with n = 0 has none.
Component:    the winning component of sample t is m = 1 when a_1 > a_0 for state s(t), else 0 -- a_0, a_1 as in the
              emission, on the calibrated x where a calibration is given.
Record:       state, start, length, n1 = samples whose component 1 won, sum[m] / sumsq[m] = the sum / sum of squares of the
              samples component m won: exact integers of the RAW samples for the int16 feed (SEG_DTYPE), float64 for the
              float64 feed (SEGF_DTYPE), there accumulated one sample at a time in rising t from 0.0 as sum += x,
              sumsq += x * x.
Output:       hmm_ref's record per read, off[0..R] (int64), read r's segments at seg[off[r]:off[r+1]].
"""
import numpy as np

import hmm_ref

SEG_DTYPE = np.dtype([("state", "<i4"), ("start", "<i4"), ("length", "<i4"), ("n1", "<i4"), ("sum", "<i8", (2,)),
                      ("sumsq", "<i8", (2,))])
SEGF_DTYPE = np.dtype([("state", "<i4"), ("start", "<i4"), ("length", "<i4"), ("n1", "<i4"), ("sum", "<f8", (2,)),
                       ("sumsq", "<f8", (2,))])


def back_pointers(model, x, lens):
    """(arg int8 [R, N, S], f int64 [R]) of the rows x[R, N] (float64): arg[r, t, j] = arg_j(t) of read r for 1 <= t <
    lens[r], f[r] = the lowest j with the largest v_j(n - 1) (-1 for an empty read)"""
    S, linit, ltrans, c, mu, h = hmm_ref.model_arrays(model)
    x = np.asarray(x, dtype=np.float64)
    lens = np.asarray(lens, dtype=np.int64)
    R, N = x.shape
    arg = np.zeros((R, N, S), dtype=np.int8)
    f = np.full(R, -1, dtype=np.int64)
    if R == 0 or lens.max(initial=0) == 0:
        return arg, f
    v = np.full((R, S), -np.inf)
    for t in range(int(lens.max())):
        act = lens > t
        e = hmm_ref.emission(c, mu, h, x[:, t])
        if t == 0:
            nv = linit[None, :] + e
        else:
            with np.errstate(invalid="ignore"):
                cand = v[:, :, None] + ltrans[None, :, :]           # [R, from, to]
            b = cand[:, 0, :].copy()
            a = np.zeros((R, S), dtype=np.int8)
            for i in range(1, S):
                w = cand[:, i, :] > b
                b = np.where(w, cand[:, i, :], b)
                a = np.where(w, np.int8(i), a)
            arg[act, t] = a[act]
            with np.errstate(invalid="ignore"):
                nv = b + e
        v[act] = nv[act]
    best = v[:, 0].copy()
    fj = np.zeros(R, dtype=np.int64)
    for j in range(1, S):
        w = v[:, j] > best
        best = np.where(w, v[:, j], best)
        fj = np.where(w, j, fj)
    f[lens > 0] = fj[lens > 0]
    return arg, f


def state_paths(arg, f, lens):
    """s[R, N] (int8; -1 past a read's end) by the back-trace"""
    lens = np.asarray(lens, dtype=np.int64)
    R, N, _ = arg.shape
    s = np.full((R, N), -1, dtype=np.int8)
    rows = np.arange(R)
    has = lens > 0
    s[rows[has], lens[has] - 1] = f[has]
    for t in range(int(lens.max(initial=0)) - 1, 0, -1):
        act = rows[lens > t]
        s[act, t - 1] = arg[act, t, s[act, t]]
    return s


def winning_component(model, x, s):
    """m[R, N] (int8): 1 where a_1 > a_0 for state s of sample x (0 past a read's end)"""
    S, _, _, c, mu, h = hmm_ref.model_arrays(model)
    j = np.maximum(s, 0).astype(np.int64)
    d0 = x - mu[j, 0]
    d1 = x - mu[j, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        a0 = c[j, 0] - (d0 * d0) * h[j, 0]
        a1 = c[j, 1] - (d1 * d1) * h[j, 1]
    return ((a1 > a0) & (s >= 0)).astype(np.int8)


def segment_stats(vals, comp, first, length, dtype):
    """n1, sum[.., 2], sumsq[.., 2] of the segments vals[first[k] : first[k] + length[k]] (flat arrays), every segment
    accumulated one sample at a time in rising order from zero"""
    nseg = len(first)
    sums = np.zeros((nseg, 2), dtype=dtype)
    sq = np.zeros((nseg, 2), dtype=dtype)
    n1 = np.zeros(nseg, dtype=np.int32)
    order = np.argsort(-length, kind="stable")
    L, F = length[order], first[order]
    for k in range(int(L.max(initial=0))):
        na = int(np.searchsorted(-L, -k, side="left"))              # the segments longer than k
        idx = F[:na] + k
        v = vals[idx].astype(dtype)
        m = comp[idx].astype(np.int64)
        seg = order[:na]
        sums[seg, m] = sums[seg, m] + v
        sq[seg, m] = sq[seg, m] + v * v
        n1[seg] += m.astype(np.int32)
    return n1, sums, sq


def segments_rows(model, x, lens, raw=None, records=True):
    """(rec, off, seg) of the rows x[R, N] (float64, calibrated): raw = the int rows the statistics are taken of (the int16
    feed, SEG_DTYPE), or None for statistics of x itself (the float64 feed, SEGF_DTYPE).  records=False saves hmm_ref's
    forward pass: rec then holds n_used and final_state only (score 0, enter -1)."""
    x = np.asarray(x, dtype=np.float64)
    lens = np.asarray(lens, dtype=np.int64)
    R, N = x.shape
    arg, f = back_pointers(model, x, lens)
    if records:
        rec = hmm_ref.viterbi_rows(model, x, lens)
        assert (f == rec["final_state"]).all()
    else:
        rec = np.zeros(R, dtype=hmm_ref.DTYPE)
        rec["final_state"], rec["n_used"], rec["enter"] = f, lens, -1
    s = state_paths(arg, f, lens)
    comp = winning_component(model, x, s)
    dtype = SEG_DTYPE if raw is not None else SEGF_DTYPE
    inside = np.arange(N)[None, :] < lens[:, None]
    cut = inside.copy()                                             # a segment starts at t = 0 and wherever the state changes
    cut[:, 1:] &= s[:, 1:] != s[:, :-1]
    r_idx, t_idx = np.nonzero(cut)                                  # (row-major: reads in order, rising start inside a read)
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(r_idx, minlength=R), out=off[1:])
    seg = np.zeros(len(r_idx), dtype=dtype)
    seg["state"] = s[r_idx, t_idx]
    seg["start"] = t_idx
    nxt = np.append(t_idx[1:], 0)
    last = np.zeros(len(r_idx), dtype=bool)
    last[off[1:][np.diff(off) > 0] - 1] = True
    seg["length"] = np.where(last, lens[r_idx], nxt) - t_idx
    vals = (np.asarray(raw).astype(np.int64) if raw is not None else x).reshape(-1)
    acc = np.int64 if raw is not None else np.float64
    seg["n1"], seg["sum"], seg["sumsq"] = segment_stats(vals, comp.reshape(-1), r_idx * N + t_idx,
                                                       seg["length"].astype(np.int64), acc)
    return rec, off, seg


def segments_batch(model, sig, lens, cal2=None, limit=0):
    """the int16 feed: rows sig[R, stride], lengths, calibration pairs cal2[R, 2] (or None), limit"""
    sig = np.asarray(sig)
    lens = np.clip(np.asarray(lens, dtype=np.int64), 0, sig.shape[1])
    if limit > 0:
        lens = np.minimum(lens, limit)
    x = sig.astype(np.float64)
    if cal2 is not None:
        cal2 = np.asarray(cal2, dtype=np.float64).reshape(-1, 2)
        x = (x + cal2[:, :1]) * cal2[:, 1:]
    return segments_rows(model, x, lens, raw=sig)


def segments_reads(model, reads, limit=0, raw=False, records=True):
    """a list of reads of any lengths; raw: integer-valued reads through the int16 feed's records, else the float64 feed's"""
    R = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    x = np.zeros((R, max(1, int(lens.max(initial=0)))), dtype=np.float64)
    for i, r in enumerate(reads):
        x[i, :len(r)] = np.asarray(r, dtype=np.float64)
    if limit > 0:
        lens = np.minimum(lens, limit)
    return segments_rows(model, x, lens, raw=x.astype(np.int64) if raw else None, records=records)


def invariants(model, rec, off, seg):
    """the five invariants the definition implies, asserted"""
    S, _, ltrans, _, _, _ = hmm_ref.model_arrays(model)
    for r in range(len(rec)):
        g = seg[int(off[r]):int(off[r + 1])]
        n = int(rec["n_used"][r])
        if n == 0:
            assert len(g) == 0, r
            continue
        assert len(g) >= 1 and g["start"][0] == 0 and (g["length"] > 0).all(), r
        assert (g["start"][1:] == g["start"][:-1] + g["length"][:-1]).all() and g["start"][-1] + g["length"][-1] == n, r   # tile
        assert (g["state"][1:] != g["state"][:-1]).all(), r
        for k in range(6):
            first = g["start"][g["state"] == k]
            assert int(rec["enter"][r][k]) == (int(first[0]) if first.size else -1), (r, k)
        assert g["state"][-1] == rec["final_state"][r], r
        assert np.isfinite(ltrans[g["state"][:-1], g["state"][1:]]).all(), r
        assert (g["n1"] >= 0).all() and (g["n1"] <= g["length"]).all(), r


def pool(rec, off, seg, S, cal2=None):
    """hmm_pool, stated plainly: per state and component the count, sum and sum of squares in model units (exact Python
    integers for the int16 feed without a calibration, floats otherwise), the transition counts -- length - 1 stays per
    segment plus one step per pair of neighbours -- and the initial counts"""
    exact = seg["sum"].dtype.kind == "i" and cal2 is None
    zero = 0 if exact else 0.0
    n = [[0, 0] for _ in range(S)]
    sm = [[zero, zero] for _ in range(S)]
    sq = [[zero, zero] for _ in range(S)]
    A = [[0] * S for _ in range(S)]
    init = [0] * S
    for r in range(len(rec)):
        g = seg[int(off[r]):int(off[r + 1])]
        for k, e in enumerate(g):
            j = int(e["state"])
            cnt = (int(e["length"]) - int(e["n1"]), int(e["n1"]))
            for m in range(2):
                n[j][m] += cnt[m]
                if exact:
                    sm[j][m] += int(e["sum"][m])
                    sq[j][m] += int(e["sumsq"][m])
                elif cal2 is None:
                    sm[j][m] += float(e["sum"][m])
                    sq[j][m] += float(e["sumsq"][m])
                else:
                    o, u = float(cal2[r][0]), float(cal2[r][1])
                    sm[j][m] += u * (float(e["sum"][m]) + cnt[m] * o)
                    sq[j][m] += (u * u) * (float(e["sumsq"][m]) + 2.0 * o * float(e["sum"][m]) + cnt[m] * (o * o))
            A[j][j] += int(e["length"]) - 1
            if k == 0:
                init[j] += 1
            else:
                A[int(g[k - 1]["state"])][j] += 1
    return {"n": n, "sum": sm, "sumsq": sq, "trans": A, "init": init}
