"""GPU: MotifSeq sessions (sk_stream_*, api.MotifStream) against the numpy statement of tests/stream_ref.py.  Every
comparison is exact: doubles bit for bit, NaN equal to NaN -- the record after any sequence of pushes is the record of the
one-shot search on the samples seen so far."""
import ctypes as C
import os

import numpy as np
import pytest

import stream_ref as ref
from conftest import GOLD

pytestmark = pytest.mark.gpu

LO, HI = 0, 1200
CHUNKS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 200, 1000)
SEAM_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 163, 256, 257, 1024)


def squiggles(R, n, seed, motif=None, spikes=0.02):
    """int16 squiggle-like reads, a few per cent of the samples outside (LO, HI)"""
    from squigglekit_amd import synth
    sig = synth.squiggle_batch(R, n, seed, motif=motif).copy()
    rng = np.random.default_rng(seed + 1)
    hit = rng.random(sig.shape) < spikes
    sig[hit] = rng.choice(np.array([-40, 0, 1200, 3000, 32767], dtype=np.int16), size=int(hit.sum()))
    return sig


def cut(rng, n, sizes=CHUNKS):
    """chunk lengths from `sizes` in a seeded order that add up to n (the last one cut to fit)"""
    out, left = [], n
    while left > 0:
        c = int(rng.choice(sizes))
        c = min(c, left)
        out.append(c)
        left -= c
    return out


class Model:
    """What the statement says a session's slots hold: the raw samples pushed per slot, where the flush came, the pushes."""

    def __init__(self, motifs, nslots, W, mode, lo=LO, hi=HI):
        self.motifs, self.W, self.mode, self.lo, self.hi = motifs, W, mode, lo, hi
        self.raw = [np.zeros(0, dtype=np.int16) for _ in range(nslots)]
        self.flushed = [False] * nslots
        self.given = [None] * nslots
        self.chunks = [0] * nslots
        self.cache = {}

    def push(self, slot, chunk):
        if len(chunk):
            self.raw[slot] = np.concatenate([self.raw[slot], chunk])
            self.chunks[slot] += 1

    def flush(self, slot):
        if self.flushed[slot] is False:
            self.flushed[slot] = len(self.raw[slot])

    def reset(self, slot, given=None):
        self.raw[slot] = np.zeros(0, dtype=np.int16)
        self.flushed[slot], self.given[slot], self.chunks[slot] = False, given, 0

    def want(self, slot, k):
        key = (slot, k, len(self.raw[slot]), self.flushed[slot], self.given[slot], id(self.raw[slot]))
        if key not in self.cache:
            self.cache[key] = ref.record(self.raw[slot], self.motifs[k], self.W, self.mode, self.lo, self.hi,
                                         self.flushed[slot], self.given[slot])
        return self.cache[key]

    def check(self, rec, slots, label=""):
        assert rec.shape == (len(self.motifs), len(slots))
        for k in range(len(self.motifs)):
            for i, s in enumerate(slots):
                got, want = ref.fields(rec[k, i]), self.want(s, k)
                assert ref.same(got, want), "%s motif %d (N=%d) slot %d after %d samples: got %r want %r" % (
                    label, k, len(self.motifs[k]), s, len(self.raw[s]), got, want)
                assert int(rec[k, i]["chunks"]) == self.chunks[s], (label, s, int(rec[k, i]["chunks"]), self.chunks[s])


def seam_motifs():
    from squigglekit_amd import synth
    return [synth.synthetic_motif(N, seed=100 + N) for N in SEAM_LENGTHS]


@pytest.mark.parametrize("nslots", [1, 5])
@pytest.mark.parametrize("no_small", [False, True])
def test_prefix_property_at_the_seams(gpu, monkeypatch, no_small, nslots):
    """After every push every field equals the statement on the prefix -- motif lengths around every lane and row
    boundary, chunk lengths around the lane counts, both lane layouts (SK_DTW_NO_SMALL: four slots per wavefront for
    motifs of up to 256 points)."""
    from squigglekit_amd import api
    if no_small:
        monkeypatch.setenv("SK_DTW_NO_SMALL", "1")
    motifs = seam_motifs()
    rng = np.random.default_rng(11 + nslots + 100 * no_small)
    total = 3000 if nslots == 1 else 1400
    reads = squiggles(nslots, total, 500 + nslots, motif=motifs[10])           # (~half the reads carry the 163-point motif)
    lens = [total] + [int(rng.integers(300, total)) for _ in range(nslots - 1)]
    plans = [cut(rng, n) for n in lens]
    W = 100
    mdl = Model(motifs, nslots, W, "medmad")
    with api.MotifStream(motifs, nslots, "medmad", LO, HI, calib=W) as ms:
        at = [0] * nslots
        step = 0
        while any(plans):
            slots = [s for s in range(nslots) if plans[s]]
            chunks = []
            for s in slots:
                c = plans[s].pop(0)
                chunks.append(reads[s, at[s]:at[s] + c])
                at[s] += c
                mdl.push(s, chunks[-1])
            rec = ms.push(slots, chunks)
            mdl.check(rec, slots, "push %d" % step)
            step += 1


def test_chunking_invariance(gpu):
    """64 reads pushed whole, sample by sample for the first 130 samples, and in random cuts: the same final records,
    and the statement's."""
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(163), synth.synthetic_motif(20, seed=3)]
    R, n, W = 64, 900, 60
    reads = squiggles(R, n, 77, motif=motifs[0])
    rng = np.random.default_rng(5)
    slots = list(range(R))
    finals = []
    with api.MotifStream(motifs, R, "medmad", LO, HI, calib=W) as ms:
        finals.append(ms.push(slots, (reads, np.full(R, n, dtype=np.int32))))
        ms.reset(slots)
        for j in range(130):
            ms.push(slots, (reads[:, j:j + 1].copy(), np.ones(R, dtype=np.int32)))
        finals.append(ms.push(slots, (reads[:, 130:].copy(), np.full(R, n - 130, dtype=np.int32))))
        ms.reset(slots)
        plans, at = [cut(rng, n) for _ in range(R)], [0] * R
        while any(plans):
            live = [s for s in slots if plans[s]]
            chunks = []
            for s in live:
                c = plans[s].pop(0)
                chunks.append(reads[s, at[s]:at[s] + c])
                at[s] += c
            ms.push(live, chunks)
        finals.append(ms.push(slots, [reads[0, :0]] * R))                      # peek
    mdl = Model(motifs, R, W, "medmad")
    for s in slots:
        mdl.push(s, reads[s])
    for f in finals:
        for k in range(2):
            for s in slots:
                assert ref.same(ref.fields(f[k, s]), mdl.want(s, k)), (k, s, ref.fields(f[k, s]), mdl.want(s, k))


def test_lockstep_and_independence(gpu, monkeypatch):
    """130 slots, four to a wavefront: per push a random subset gets chunks of widely different lengths (0 and wholly
    filtered ones included); slots not pushed keep their record; the order of a call's slots only orders its output."""
    from squigglekit_amd import api, synth
    monkeypatch.setenv("SK_DTW_NO_SMALL", "1")
    motifs = [synth.synthetic_motif(40, seed=9)]
    S, W = 130, 50
    reads = squiggles(S, 1500, 31)
    rng = np.random.default_rng(8)
    mdl = Model(motifs, S, W, "zscale")
    at = [0] * S
    with api.MotifStream(motifs, S, "zscale", LO, HI, calib=W) as a, api.MotifStream(motifs, S, "zscale", LO, HI, calib=W) as b:
        for step in range(6):
            slots = sorted(rng.choice(S, size=int(rng.integers(1, S)), replace=False).tolist())
            chunks = []
            for s in slots:
                kind = int(rng.integers(0, 5))
                c = (0, 1, int(rng.integers(2, 40)), int(rng.integers(40, 400)), 37)[kind]
                c = min(c, 1500 - at[s])
                ch = reads[s, at[s]:at[s] + c].copy()
                if kind == 4:
                    ch[:] = 3000                                               # a chunk the filter drops entirely
                    reads[s, at[s]:at[s] + c] = ch
                at[s] += c
                chunks.append(ch)
                mdl.push(s, ch)
            rec = a.push(slots, chunks)
            mdl.check(rec, slots, "step %d" % step)
            perm = rng.permutation(len(slots))
            rec_b = b.push([slots[p] for p in perm], [chunks[p] for p in perm])
            assert rec_b[:, np.argsort(perm)].tobytes() == rec.tobytes()       # the same call in another slot order
            rest = [s for s in range(S) if s not in set(slots)]
            if rest:
                peek = a.push(rest, [reads[0, :0]] * len(rest))                # len 0: the current record, unchanged
                mdl.check(peek, rest, "peek %d" % step)


@pytest.mark.parametrize("mode", ["medmad", "zscale"])
@pytest.mark.parametrize("W", [1, 2, 100, 2000])
def test_calibration_seams(gpu, mode, W):
    """Calibration that completes exactly at a chunk's end, at a chunk's first kept sample, in the middle of a chunk and
    inside a chunk that also holds dropped samples: calibrating records before, the statement from then on."""
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(33, seed=4), synth.synthetic_motif(163)]
    n = W + 700
    base = np.clip(squiggles(4, n + 8, 900 + W, spikes=0.0), 200, 1000)         # every sample inside the limits
    reads, plans = [], []
    # slot 0: the first chunk holds exactly W kept samples; slot 1: W - 1, then a chunk whose first sample completes it
    reads.append(base[0, :n]); plans.append([W, 300, n - W - 300])
    reads.append(base[1, :n]); plans.append([W - 1, 250, n - W - 249] if W > 1 else [0, 250, n - 250])
    # slot 2: in the middle of a chunk; slot 3: the completing chunk also holds dropped samples around the seam
    reads.append(base[2, :n]); plans.append([W // 2, W // 2 + 120, n - 2 * (W // 2) - 120])
    r3 = base[3, :n + 8].copy()
    r3[[max(0, W - 2), W + 1, W + 2]] = 3000
    r3[0] = -5
    reads.append(r3); plans.append([max(0, W - 3), 90, n + 8 - max(0, W - 3) - 90])
    mdl = Model(motifs, 4, W, mode)
    with api.MotifStream(motifs, 4, mode, LO, HI, calib=W) as ms:
        at = [0] * 4
        for step in range(3):
            chunks = []
            for s in range(4):
                c = plans[s][step]
                chunks.append(reads[s][at[s]:at[s] + c])
                at[s] += c
                mdl.push(s, chunks[-1])
            rec = ms.push([0, 1, 2, 3], chunks)
            mdl.check(rec, [0, 1, 2, 3], "W=%d %s step %d" % (W, mode, step))
            if step == 0 and W > 2:
                assert int(rec[0, 1]["flags"]) == ref.CALIBRATING and int(rec[0, 1]["n"]) == W - 1
                assert int(rec[0, 0]["flags"]) == 0 and int(rec[0, 0]["n"]) == W


@pytest.mark.parametrize("mode", ["medmad", "zscale"])
def test_flush_equals_the_one_shot_path(gpu, mode):
    """200 reads shorter than the calibration length, pushed in random chunks and flushed: dist, start, end, n, flags of
    api.motifseq_multi_batch on the whole reads -- a constant read and a read with nothing inside the limits included;
    pushes after the flush go on under the fixed normalisation.

    For the constant read the one-shot call returns dist = +inf (every cell NaN, the running minimum never moves) and
    the flushed slot returns the same; all mismatches are collected and reported together."""
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(163), synth.synthetic_motif(40, seed=2), synth.synthetic_motif(300, seed=5)]
    R, W = 200, 4096
    rng = np.random.default_rng(17)
    lens = rng.integers(50, 3001, R).astype(np.int32)
    sig = squiggles(R, 3000, 41, motif=motifs[0])
    sig[7] = 500                                                               # MAD 0
    sig[11] = 3000                                                             # nothing survives the filter
    slots = list(range(R))
    with api.MotifStream(motifs, R, mode, LO, HI, calib=W) as ms:
        plans = [cut(rng, int(n), (1, 17, 64, 200, 1000)) for n in lens]
        at = [0] * R
        while any(plans):
            live = [s for s in slots if plans[s]]
            chunks = []
            for s in live:
                c = plans[s].pop(0)
                chunks.append(sig[s, at[s]:at[s] + c])
                at[s] += c
            rec = ms.push(live, chunks)
            assert np.all(rec["flags"] == ref.CALIBRATING) and np.all(np.isnan(rec["dist"]))
        got = ms.flush(slots)
        want = api.motifseq_multi_batch(sig, lens, motifs, scale=mode, scale_low=LO, scale_hi=HI)
        failures = []
        for k in range(3):
            for f in ("dist", "start", "end", "n", "flags"):
                a, b = got[k][f], want[k][f]
                print(mode, k, f, "constant read:", a[7], b[7], "empty read:", a[11], b[11])
                bad = np.nonzero(~((a == b) | ((a != a) & (b != b))))[0]
                if bad.size:
                    failures.append((mode, k, f, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist()))
        assert int(got[0, 11]["flags"]) == ref.EMPTY and (mode == "zscale" or int(got[0, 7]["flags"]) == ref.DEGENERATE)
        # more samples after the flush: the statement with the normalisation the flush fixed
        more = squiggles(8, 120, 43)
        mdl = Model(motifs, R, W, mode)
        for s in range(8):
            mdl.push(s, sig[s, :lens[s]])
            mdl.flush(s)
            mdl.push(s, more[s])
        rec = ms.push(list(range(8)), [more[s] for s in range(8)])
        for k in range(3):
            for s in range(8):
                assert ref.same(ref.fields(rec[k, s]), mdl.want(s, k)), (mode, k, s, ref.fields(rec[k, s]), mdl.want(s, k))
        assert not failures, failures


def test_reset_given_scale_two_sessions_and_one_shot_calls_between(gpu):
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(64, seed=6), synth.synthetic_motif(200, seed=8)]
    reads = squiggles(6, 800, 61, motif=motifs[1])
    W = 120
    mdl_a, mdl_b = Model(motifs, 3, W, "medmad"), Model(motifs[:1], 2, 30, "zscale")
    a = api.MotifStream(motifs, 3, "medmad", LO, HI, calib=W)
    b = api.MotifStream(motifs[:1], 2, "zscale", LO, HI, calib=30)
    try:
        for s in range(3):
            mdl_a.push(s, reads[s, :400])
        mdl_a.check(a.push([0, 1, 2], [reads[s, :400] for s in range(3)]), [0, 1, 2], "first read")
        mdl_b.push(1, reads[3, :90])
        mdl_b.check(b.push([1], [reads[3, :90]]), [1], "second session")
        # one-shot calls on the same context between the pushes: neither side moves
        one = api.motifseq_batch(reads, np.full(6, 800, dtype=np.int32), motifs[1])
        segs, nsegs = api.segment_batch(reads, np.full(6, 800, dtype=np.int32))
        for s in range(3):
            mdl_a.push(s, reads[s, 400:650])
        mdl_a.check(a.push([2, 0, 1], [reads[s, 400:650] for s in (2, 0, 1)]), [2, 0, 1], "after one-shot calls")
        assert api.motifseq_batch(reads, np.full(6, 800, dtype=np.int32), motifs[1]).tobytes() == one.tobytes()
        segs2, nsegs2 = api.segment_batch(reads, np.full(6, 800, dtype=np.int32))
        assert segs2.tobytes() == segs.tobytes() and nsegs2.tobytes() == nsegs.tobytes()
        # slot 1 starts a second read: nothing of the first shows; slot 2 restarts under a given normalisation
        a.reset([1])
        mdl_a.reset(1)
        a.reset([2], center=510.5, scale=77.25)
        mdl_a.reset(2, given=(510.5, 77.25))
        rec = a.push([1, 2], [reads[4, :0], reads[5, :0]])
        mdl_a.check(rec, [1, 2], "after reset")
        assert int(rec[0, 1]["flags"]) == 0 and int(rec[0, 0]["flags"]) == ref.CALIBRATING
        for lo, hi in ((0, 1), (1, 130), (130, 500)):
            mdl_a.push(1, reads[4, lo:hi])
            mdl_a.push(2, reads[5, lo:hi])
            rec = a.push([1, 2], [reads[4, lo:hi], reads[5, lo:hi]])
            mdl_a.check(rec, [1, 2], "second read [%d, %d)" % (lo, hi))
            kept = ref.keep(reads[5, :hi], LO, HI)
            for k in range(2 if kept.size else 0):                             # ... which is dtw_subsequence on (kept - c) / s
                d, _, path = api.dtw_subsequence(motifs[k], (kept.astype(np.float64) - 510.5) / 77.25)
                assert (float(rec[k, 1]["dist"]), int(rec[k, 1]["start"]), int(rec[k, 1]["end"])) == \
                       (float(d), int(path[1][0]), int(path[1][-1]))
        mdl_a.check(a.push([0], [reads[0, :0]]), [0], "the slot that was not reset")
        b.close()                                                              # closing one session leaves the other working
        mdl_a.push(0, reads[0, 650:])
        mdl_a.check(a.push([0], [reads[0, 650:]]), [0], "after the other session closed")
        with pytest.raises(ValueError):
            b.push([0], [reads[0, :5]])
    finally:
        a.close()
        b.close()


def test_host_form_errors(gpu):
    from squigglekit_amd import _lib, api, synth
    L = _lib.load()
    with api.MotifStream([synth.synthetic_motif(20)], 4, calib=10) as ms:
        rows = np.full((2, 8), 500, dtype=np.int16)
        out = np.zeros((1, 2), dtype=_lib.STREAM_DTYPE)

        def push(slots, lens, handle=None):
            s, n = np.array(slots, dtype=np.int32), np.array(lens, dtype=np.int32)
            rc = L.sk_stream_push_i16(ms.handle if handle is None else handle, _lib.ptr(s), 2, _lib.ptr(rows), 8, _lib.ptr(n),
                                      _lib.ptr(out))
            return rc, L.sk_last_error().decode()

        for args, word in ((([1, 1], [8, 8]), "twice"), (([0, 4], [8, 8]), "outside"), (([0, 1], [8, 9]), "len["),
                           (([0, 1], [8, 8], 5), "handle")):
            rc, msg = push(*args)
            assert rc == _lib.SK_ERR_INVALID and word in msg, (args, rc, msg)
        s = np.array([0], dtype=np.int32)
        for c, sc in ((0.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0)):
            rc = L.sk_stream_reset(ms.handle, _lib.ptr(s), 1, _lib.ptr(np.array([c])), _lib.ptr(np.array([sc])))
            assert rc == _lib.SK_ERR_INVALID and "scale" in L.sk_last_error().decode()
        assert push([0, 1], [8, 8])[0] == 0 and int(out[0, 0]["seen"]) == 8   # the refused calls changed nothing
    handles = [api.MotifStream([synth.synthetic_motif(20)], 4) for _ in range(8)]
    with pytest.raises(_lib.SquiggleKitError):
        api.MotifStream([synth.synthetic_motif(20)], 4)                        # eight sessions per context
    for h in handles:
        h.close()


def test_device_form_gives_the_host_form_records(gpu):
    from squigglekit_amd import _lib, api, synth
    L = _lib.load()
    motifs = [synth.synthetic_motif(163), synth.synthetic_motif(17, seed=2)]
    S, W, stride = 9, 80, 256
    reads = squiggles(S, 1200, 71, motif=motifs[0])
    rng = np.random.default_rng(3)
    d_rows, d_slots, d_len = L.sk_dev_alloc(S * stride * 2), L.sk_dev_alloc(S * 4), L.sk_dev_alloc(S * 4)
    d_out = L.sk_dev_alloc(2 * S * 40)
    try:
        with api.MotifStream(motifs, S, "medmad", LO, HI, calib=W) as host, \
                api.MotifStream(motifs, S, "medmad", LO, HI, calib=W) as dev:
            at = np.zeros(S, dtype=np.int64)
            for step in range(6):
                slots = rng.permutation(S)[:int(rng.integers(1, S + 1))].astype(np.int32)
                m = slots.size
                lens = rng.integers(0, stride + 1, m).astype(np.int32)
                rows = np.zeros((m, stride), dtype=np.int16)
                for i, s in enumerate(slots):
                    lens[i] = min(int(lens[i]), 1200 - int(at[s]))
                    rows[i, :lens[i]] = reads[s, at[s]:at[s] + lens[i]]
                    at[s] += lens[i]
                want = host.push(slots, (rows, lens))
                _lib.check(L.sk_dev_upload(d_rows, _lib.ptr(rows), rows.nbytes))
                _lib.check(L.sk_dev_upload(d_slots, _lib.ptr(slots), slots.nbytes))
                _lib.check(L.sk_dev_upload(d_len, _lib.ptr(lens), lens.nbytes))
                _lib.check(L.sk_stream_push_dev_i16(dev.handle, d_slots, m, d_rows, stride, d_len, d_out))
                got = np.zeros((2, m), dtype=_lib.STREAM_DTYPE)
                _lib.check(L.sk_dev_download(_lib.ptr(got), d_out, got.nbytes))
                assert got.tobytes() == want.tobytes(), step
    finally:
        for p in (d_rows, d_slots, d_len, d_out):
            L.sk_dev_free(p)


def test_seeded_random_sweep(gpu, monkeypatch):
    """40 random sessions over (K, N, nslots, W, limits, mode, cuts) against the statement."""
    from squigglekit_amd import api, synth
    rng = np.random.default_rng(2026)
    for case in range(40):
        K = int(rng.integers(1, 4))
        Ns = [int(rng.choice([1, 3, 16, 17, 40, 100, 163, 256, 257, 500, 1024])) if rng.random() < 0.5
              else int(rng.integers(1, 400)) for _ in range(K)]
        nslots, W = int(rng.integers(1, 9)), int(rng.choice([1, 2, 10, 64, 300]))
        lo, hi = int(rng.choice([0, 300, -100])), int(rng.choice([1200, 700, 40000]))
        mode = "medmad" if rng.random() < 0.5 else "zscale"
        no_small = bool(rng.random() < 0.5)
        n = int(rng.integers(1, 700))
        desc = dict(case=case, K=K, Ns=Ns, nslots=nslots, W=W, lo=lo, hi=hi, mode=mode, no_small=no_small, n=n)
        if no_small:
            monkeypatch.setenv("SK_DTW_NO_SMALL", "1")
        else:
            monkeypatch.delenv("SK_DTW_NO_SMALL", raising=False)
        motifs = [synth.synthetic_motif(N, seed=case * 7 + i) for i, N in enumerate(Ns)]
        reads = squiggles(nslots, n, 3000 + case, spikes=0.05)
        if case % 4 == 0:
            reads = (reads // 40 * 40).astype(np.int16)                        # few distinct values: ties, MAD 0 at small W
        mdl = Model(motifs, nslots, W, mode, lo, hi)
        plans = [cut(rng, n, (0, 1, 2, 7, 16, 33, 64, 150)) for _ in range(nslots)]
        at = [0] * nslots
        with api.MotifStream(motifs, nslots, mode, lo, hi, calib=W) as ms:
            while any(plans):
                live = [s for s in range(nslots) if plans[s] and rng.random() < 0.8]
                chunks = []
                for s in live:
                    c = plans[s].pop(0)
                    chunks.append(reads[s, at[s]:at[s] + c])
                    at[s] += c
                    mdl.push(s, chunks[-1])
                if live:
                    mdl.check(ms.push(live, chunks), live, str(desc))
            for s in range(nslots):
                mdl.flush(s)
            mdl.check(ms.flush(list(range(nslots))), list(range(nslots)), "flush " + str(desc))


def run_cli(main, argv):
    import contextlib
    import io
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code if isinstance(e.code, int) else 1
    return out.getvalue(), err.getvalue(), code


def test_cli_replay_equals_motifseq_and_decides_on_the_first_accepting_record(gpu, example_read):
    """MotifSeq_stream on the golden BLOW5 read: calibrating on the whole read and never deciding, its twelve columns are
    what MotifSeq.py --blow5 prints for the file (run here, through the existing tool); with a calibration of 2 000
    samples and --accept_Z the line is that of the first record that accepts."""
    from squigglekit_amd import api, fastio, tsvio
    from squigglekit_amd.motifseq_cli import main as motifseq_main
    from squigglekit_amd.stream_cli import main as stream_main
    blow5, model = os.path.join(GOLD, "example_0.blow5"), os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")
    want, err, code = run_cli(motifseq_main, ["--blow5", blow5, "-m", model])
    assert code == 0, err[-300:]
    got, err, code = run_cli(stream_main, ["--blow5", blow5, "-m", model, "--calib", "65536", "--chunk", "4000"])
    assert code == 0, err[-300:]
    wl, gl = want.strip("\n").split("\n"), got.strip("\n").split("\n")
    assert len(wl) == len(gl) >= 2 and gl[0].split("\t")[:12] == wl[0].split("\t")
    for a, b in zip(wl[1:], gl[1:]):
        cols = b.split("\t")
        assert cols[:12] == a.split("\t"), (a, b)
        assert cols[12:] == ["end", "10", str(len(example_read["signal"]))]
    # --accept_Z: replay the pushes through a session of our own and take the Z the third push shows as the threshold
    models, order, lens = tsvio.read_model_auto(model)
    motif = np.asarray(models[order[0]], dtype=np.float64)
    mean = 2.90 * lens[0] + -9.6
    sd = mean * 0.08468
    sig = np.ascontiguousarray(example_read["signal"], dtype=np.int16)
    recs = []
    with api.MotifStream([motif], 1, calib=2000) as ms:
        for lo in range(0, len(sig), 4000):
            recs.append(ms.push([0], [sig[lo:lo + 4000]])[0, 0].copy())
    z = [(float(r["dist"]) - mean) / sd for r in recs]
    thr = z[2]
    first = next(i for i, v in enumerate(z) if v <= thr)
    got, err, code = run_cli(stream_main, ["--blow5", blow5, "-m", model, "--calib", "2000", "--chunk", "4000",
                                           "--accept_Z=" + repr(thr)])
    assert code == 0, err[-300:]
    cols = got.strip("\n").split("\n")[1].split("\t")
    r = recs[first]
    assert cols[12:] == ["accept", str(first + 1), str(int(r["seen"]))] and int(r["seen"]) == min(len(sig), 4000 * (first + 1))
    assert cols[3:7] == [str(int(r["start"])), str(int(r["end"])), str(int(r["end"] - r["start"])), repr(float(r["dist"]))]
    assert cols[9] == "{}".format(z[first]) and cols[10] == "{}".format(fastio.ndtr(z[first]))
