"""Inputs for the pile-up tests (tests/test_pileup_host.py, tests/test_gpu_pileup*.py): the hand-worked case, builders
for lists of chosen lengths and DTW-like paths, and the seeded random family (documented in RANDOM_CASES_PILEUP.md).
A case is a dict of pileup_ref's keyword arguments."""
import math

import numpy as np


def case(span_off, spans, value, dwell=None, target=None, shift=None, use=None, tlen=None):
    spans = np.asarray(spans, dtype=np.int32).reshape(-1, 2)
    return dict(span_off=np.asarray(span_off, dtype=np.int64), spans=spans, value=np.asarray(value, dtype=np.float64),
                dwell=None if dwell is None else np.asarray(dwell, dtype=np.int32),
                target=None if target is None else np.asarray(target, dtype=np.int32),
                shift=None if shift is None else np.asarray(shift, dtype=np.int32),
                use=None if use is None else np.asarray(use, dtype=np.uint8), tlen=np.asarray(tlen, dtype=np.int64))


def hand_case():
    """Five pairs, four targets (lengths 6, 0, 5, 3: one empty, the last covered by nobody).
    pair 0 -> target 0, shift 1: rows 0..3 = (0,0) (0,0) (1,3) (-1,-1)   a stay, a shared row, a row without a path
    pair 1 -> target 2, shift 0: rows 4..5 = (0,1) (2,2)
    pair 2 -> target 0, shift 0: rows 6..7 = (1,1) (2,2)
    pair 3 -> target 0, masked by use;  pair 4 -> target -1: both left out
    Lists by flat point (targets at 0, 6, 6, 11):  1: rows 0 1 6;  2: rows 2 7;  3: row 2;  4: row 2;  6: row 4;  7: row 4;
    8: row 5; every other point empty."""
    return case(span_off=[0, 4, 6, 8, 9, 10],
                spans=[(0, 0), (0, 0), (1, 3), (-1, -1), (0, 1), (2, 2), (1, 1), (2, 2), (0, 0), (0, 0)],
                value=[1.0, 2.0, 4.0, 100.0, -1.5, 0.5, 6.0, 8.0, 50.0, 60.0],
                dwell=[3, 5, 10, 7, 2, 4, 4, 2, 9, 9],
                target=[0, 2, 0, 0, -1], shift=[1, 0, 0, 0, 0], use=[1, 1, 1, 0, 1], tlen=[6, 0, 5, 3])


HAND_LISTS = {1: [0, 1, 6], 2: [2, 7], 3: [2], 4: [2], 6: [4], 7: [4], 8: [5]}
# level, level_sd, vmin, vmax, dwell_mean, dwell_sd, depth, n, shared -- worked by hand:
#   point 1: v = 1 2 6: mean 3, deviations -2 -1 3, sd = sqrt(14 / 3); d = 3 5 4: mean 4, sd = sqrt(2 / 3); pairs 0 0 2
#   point 2: v = 4 8: mean 6, sd 2; d = 10 2: mean 6, sd 4; pairs 0 2; row 2 is shared
HAND_RECORDS = {1: (3.0, math.sqrt(14.0 / 3.0), 1.0, 6.0, 4.0, math.sqrt(2.0 / 3.0), 2, 3, 0),
                2: (6.0, 2.0, 4.0, 8.0, 6.0, 4.0, 2, 2, 1),
                3: (4.0, 0.0, 4.0, 4.0, 10.0, 0.0, 1, 1, 1),
                4: (4.0, 0.0, 4.0, 4.0, 10.0, 0.0, 1, 1, 1),
                6: (-1.5, 0.0, -1.5, -1.5, 2.0, 0.0, 1, 1, 1),
                7: (-1.5, 0.0, -1.5, -1.5, 2.0, 0.0, 1, 1, 1),
                8: (0.5, 0.0, 0.5, 0.5, 4.0, 0.0, 1, 1, 0)}


def wide_values(rng, n):
    """values over 12 orders of magnitude and both signs: a wrong order of summation changes bits"""
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 6.0, size=n)


def lists_case(rng, lengths, values=None, tlen_extra=0):
    """One single-row pair per entry: list k (lengths[k] entries) on point k of one target, the pairs of the lists
    interleaved at random so that every list's rows are spread over the whole table."""
    pts = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    E = pts.size
    v = wide_values(rng, E) if values is None else np.asarray(values, dtype=np.float64)
    return case(span_off=np.arange(E + 1), spans=np.stack([pts, pts], axis=1), value=v,
                dwell=rng.integers(1, 200, size=E), tlen=[len(lengths) + tlen_extra])


def path_spans(rng, nrows, tlen, stay=0.3, skip=0.2, start=None):
    """A monotone DTW-like path of nrows rows inside a target of tlen points: a row stays on the last row's point, moves
    on by one, or covers 2 .. 4 points (a skip); clipped at the target's end."""
    a = int(rng.integers(0, max(1, tlen // 4))) if start is None else int(start)
    out = np.zeros((nrows, 2), dtype=np.int32)
    for i in range(nrows):
        u = rng.random()
        if i and u >= stay:
            a = min(out[i - 1, 1] + 1, tlen - 1)
        elif i:
            a = out[i - 1, 1]
        b = a + (int(rng.integers(1, 4)) if rng.random() < skip else 0)
        out[i] = (a, min(b, tlen - 1))
    return out


def paths_case(rng, npairs, nrows, tlens, stay=0.3, skip=0.2):
    """npairs pairs of nrows rows each (an int, or a (lo, hi) range), each a path inside a random target"""
    tlens = np.asarray(tlens, dtype=np.int64)
    roomy = np.flatnonzero(tlens > 0)
    spans, target, lens = [], [], []
    for _ in range(npairs):
        t = int(rng.choice(roomy))
        n = nrows if isinstance(nrows, int) else int(rng.integers(nrows[0], nrows[1] + 1))
        spans.append(path_spans(rng, n, int(tlens[t]), stay, skip))
        target.append(t)
        lens.append(n)
    E = int(np.sum(lens))
    return case(span_off=np.concatenate([[0], np.cumsum(lens)]), spans=np.concatenate(spans), value=rng.normal(size=E),
                dwell=rng.integers(1, 60, size=E), target=target, tlen=tlens)


# ---- the seeded random family (RANDOM_CASES_PILEUP.md) --------------------------------------------------------------------
FAMILY_SEED = 2601
FAMILY_CASES = 200


def random_case(seed):
    rng = np.random.default_rng([FAMILY_SEED, seed])
    T = int(rng.integers(1, 6))
    tlens = rng.integers(0, 400, size=T)
    tlens[rng.integers(0, T)] = int(rng.integers(40, 400))          # at least one target with room
    P = 0 if rng.random() < 0.03 else int(rng.integers(0, 60))
    rowless = rng.random() < 0.04                                   # pairs, but not one row
    stay, skip = rng.uniform(0.0, 0.6), rng.uniform(0.0, 0.4)
    monotone = rng.random() < 0.6
    roomy = np.flatnonzero(tlens >= 8)
    spans, lens, target, shift = [], [], [], []
    for _ in range(P):
        t = int(rng.choice(roomy))
        n = 0 if rowless else int(rng.integers(0, 120))
        sh = int(rng.integers(-50, 200)) if rng.random() < 0.5 else 0
        L = int(tlens[t])
        if monotone:
            sp = path_spans(rng, n, L, stay, skip).astype(np.int64)
        else:                                                       # any span set: the contract does not assume a path
            a = rng.integers(0, L, size=n)
            sp = np.stack([a, np.minimum(a + rng.geometric(0.6, size=n) - 1, L - 1)], axis=1)
        if n and rng.random() < 0.15:                               # a stalled row: it covers a large part of the target
            k = int(rng.integers(0, n))
            sp[k] = (int(rng.integers(0, L // 4 + 1)), int(rng.integers(L // 2, L)))
        if n and rng.random() < 0.2:
            sp[rng.random(n) < 0.2] = -1                            # rows without a path
        if n and rng.random() < 0.1:
            sp[:] = -1                                              # a pair without a path
        sp = np.where(sp >= 0, sp - sh, sp)                         # the table holds the unshifted spans
        spans.append(sp)
        lens.append(n)
        target.append(t if rng.random() >= 0.1 else -1)
        shift.append(sh)
    E = int(np.sum(lens)) if lens else 0
    spans = np.concatenate(spans) if spans else np.zeros((0, 2), dtype=np.int64)
    # a shifted table may hold negative first entries that are real spans only when they stay >= 0: put such rows right
    neg = (spans[:, 0] < 0) & (spans[:, 1] >= 0) if E else np.zeros(0, dtype=bool)
    spans[neg] = -1
    value = rng.normal(size=E) * 10.0 ** rng.integers(-3, 4)
    if E and rng.random() < 0.1:
        value[rng.integers(0, E)] = np.nan
    use = (rng.random(P) >= 0.15).astype(np.uint8) if rng.random() < 0.5 else None
    return case(span_off=np.concatenate([[0], np.cumsum(lens)]) if P else [0], spans=spans, value=value,
                dwell=rng.integers(1, 500, size=E) if rng.random() < 0.8 else None,
                target=target if P else np.zeros(0, dtype=np.int32), shift=shift if P else np.zeros(0, dtype=np.int32),
                use=use, tlen=tlens)
