"""The definition of event detection, stated in numpy and plain Python (a helper, not a test).

Input: one read x[0..n) of int16 raw samples.  Parameters: w_short, w_long, th_short, th_long, peak_height.

t-statistic of window w at position i, for w <= i <= n - w (0.0 elsewhere), with s1, s2 the sums and q1, q2 the sums of
squares of x[i-w..i) and x[i..i+w), all exact integers:
    d = s2 - s1,  v = max(w*(q1+q2) - s1*s1 - s2*s2, 1),  t_w[i] = sqrt(float64(d*d*w) / float64(v))
Two peak detectors (short first) walk i = 0 .. n-1 and mark positions; boundaries are 0, the marks > 0 (sorted, merged),
n; events are the non-empty intervals between consecutive boundaries.  A record is (start, length, sum, sumsq).
"""
import numpy as np

PRESETS = {"dna": (3, 6, 1.4, 9.0, 0.2), "rna": (7, 14, 2.5, 9.0, 1.0)}

DTYPE = np.dtype([("start", "<i4"), ("length", "<i4"), ("sum", "<i8"), ("sumsq", "<i8")])


def tstat(x, w):
    """t_w[0..n) as float64"""
    x = np.asarray(x).astype(np.int64)
    n = x.size
    t = np.zeros(n, dtype=np.float64)
    if n < 2 * w:
        return t
    c1 = np.concatenate(([0], np.cumsum(x)))
    c2 = np.concatenate(([0], np.cumsum(x * x)))
    i = np.arange(w, n - w + 1)
    s1 = c1[i] - c1[i - w]
    s2 = c1[i + w] - c1[i]
    q1 = c2[i] - c2[i - w]
    q2 = c2[i + w] - c2[i]
    d = s2 - s1
    v = np.maximum(w * (q1 + q2) - s1 * s1 - s2 * s2, 1)
    t[i] = np.sqrt((d * d * w).astype(np.float64) / v.astype(np.float64))
    return t


def marks(x, params=PRESETS["dna"]):
    """the marked positions, in the order the detectors mark them"""
    w_short, w_long, th_short, th_long, h = params
    n = len(x)
    ws = (int(w_short), int(w_long))
    th = (float(th_short), float(th_long))
    t = (tstat(x, ws[0]), tstat(x, ws[1]))
    pos = [-1, -1]
    val = [np.inf, np.inf]
    valid = [False, False]
    masked_to = [-1, -1]
    out = []
    for i in range(n):
        for k in (0, 1):
            if i <= masked_to[k]:
                continue
            cur = t[k][i]
            if pos[k] == -1:
                if cur < val[k]:
                    val[k] = cur
                elif cur - val[k] > h:
                    val[k] = cur
                    pos[k] = i
            else:
                if cur > val[k]:
                    val[k] = cur
                    pos[k] = i
                if k == 0 and val[0] > th[0]:
                    masked_to[1] = pos[0] + ws[0]
                    pos[1] = -1
                    val[1] = np.inf
                    valid[1] = False
                if val[k] - cur > h and val[k] > th[k]:
                    valid[k] = True
                if valid[k] and i - pos[k] > ws[k] // 2:
                    out.append(pos[k])
                    pos[k] = -1
                    val[k] = cur
                    valid[k] = False
    return out


def boundaries(x, params=PRESETS["dna"]):
    n = len(x)
    if n == 0:
        return []
    return [0] + sorted({p for p in marks(x, params) if 0 < p < n}) + [n]


def events(x, params=PRESETS["dna"]):
    """the records of one read"""
    x = np.asarray(x).astype(np.int64)
    b = boundaries(x, params)
    rec = np.zeros(max(len(b) - 1, 0), dtype=DTYPE)
    for k in range(len(b) - 1):
        w = x[b[k]:b[k + 1]]
        rec[k] = (b[k], b[k + 1] - b[k], int(w.sum()), int((w * w).sum()))
    return rec


def detect(reads, params=PRESETS["dna"]):
    """(off int64 [R + 1], rec) of a list of reads, as the library returns them"""
    recs = [events(r, params) for r in reads]
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return off, (np.concatenate(recs) if recs else np.zeros(0, dtype=DTYPE))
