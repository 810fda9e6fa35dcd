"""One op of a session per call (a helper, not a test): for each session kind an object that is given an open session, its
script and the expectations computed from the statement modules beforehand; step() performs the script's next op and
asserts it exactly as the family's play function does (evstream_ref.play_session, hmmstream_ref.iter_session,
mapstream_ref.run_session, live_ref.play, the Model of tests/test_gpu_stream.py), so that a test can put other calls
between two ops of a session.  The expectations never come from the library."""
import numpy as np

import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import mapstream_ref as MR
import pair_hits_ref as PH
import stream_ref


class Steps:
    def __init__(self, name, ops):
        self.name, self.ops, self.at, self.pushes = name, ops, 0, 0

    @property
    def left(self):
        return len(self.ops) - self.at

    def step(self):
        assert self.left > 0, "%s: no op left" % self.name
        op = self.ops[self.at]
        self.do(op, "%s op %d" % (self.name, self.at))
        self.at += 1
        if op[0] == "push":
            self.pushes += 1


class EventSteps(Steps):
    """an api.EventStream under an evstream_ref script; want = evstream_ref.run_session(sess).  finish(api) compares every
    ended read's concatenation with the one-shot call."""

    def __init__(self, es, sess, want, name="event"):
        Steps.__init__(self, name, sess["ops"])
        self.es, self.sess, self.want = es, sess, want
        self.had = [[[], []] for _ in range(sess["nslots"])]
        self.closed = [False] * sess["nslots"]
        self.finished = []

    def do(self, op, label):
        if op[0] == "reset":
            self.es.reset(op[1])
            for s in op[1]:
                self.had[s], self.closed[s] = [[], []], False
            return
        _, slots, chunks, end = op
        off, rec = self.es.push(slots, chunks, end=end)
        w_off, w_rec = self.want[self.pushes]
        assert rec.dtype == ER.DTYPE
        assert np.array_equal(off, w_off) and rec.tobytes() == w_rec.tobytes(), \
            "%s: off %s, want %s\n%s" % (label, off[:12], w_off[:12], ER.describe_session(self.sess))
        for i, (s, c, e) in enumerate(zip(slots, chunks, end)):
            if self.closed[s]:
                continue
            self.had[s][0].append(np.asarray(c, dtype=np.int16))
            self.had[s][1].append(rec[off[i]:off[i + 1]])
            if e:
                self.closed[s] = True
                self.finished.append((np.concatenate(self.had[s][0]), np.concatenate(self.had[s][1])))

    def finish(self, api):
        from squigglekit_amd import _lib
        if self.finished:
            off, rec = api.detect_events([x for x, _ in self.finished], _lib.DetParams(*self.sess["params"]))
            for k, (x, got) in enumerate(self.finished):
                assert got.tobytes() == rec[off[k]:off[k + 1]].tobytes(), \
                    "%s: read %d of %d samples differs from the one-shot call" % (self.name, k, len(x))
        return len(self.finished)


class HmmSteps(Steps):
    """an api.HmmStream under a hmmstream_ref script; want = hmmstream_ref.run_session(model, sess)"""

    def __init__(self, hs, sess, want, name="hmm"):
        Steps.__init__(self, name, sess["ops"])
        self.hs, self.sess, self.want = hs, sess, want

    def do(self, op, label):
        if op[0] == "reset":
            self.hs.reset(op[1], op[2])
            return
        _, slots, chunks, feed = op
        got = self.hs.push(slots, chunks) if feed == "i16" else self.hs.push_values(slots, chunks)
        HR.assert_records(got, self.want[self.pushes], slots, "%s (%s)" % (label, feed), self.sess)


def map_expectations(ora, case):
    """per step of a mapstream_ref case: None for a reset, the records of a push (mapstream_ref.Shadow)"""
    sh = MR.Shadow(ora, case["targets"], case["nslots"])
    want = []
    for st in case["steps"]:
        if st[0] == "reset":
            sh.reset(st[1])
            want.append(None)
        else:
            want.append(sh.push(st[1], st[2]))
    return want


class MapSteps(Steps):
    """an api.MapStream under a mapstream_ref case; want = map_expectations(ora, case).  hits(K) reads the hit lists of
    every slot and compares them with pair_hits_ref.session_hits on what the slots have been given so far."""

    def __init__(self, ms, case, want, name="map"):
        Steps.__init__(self, name, case["steps"])
        self.ms, self.case, self.want = ms, case, want
        self.given = [[] for _ in range(case["nslots"])]

    def do(self, op, label):
        if op[0] == "reset":
            self.ms.reset(op[1])
            for s in op[1]:
                self.given[s] = []
            return
        diff = MR.first_difference(self.ms.push(op[1], op[2]), self.want[self.at])
        assert diff is None, "%s (slots %s, chunks %s): %s" % (label, op[1], [len(c) for c in op[2]], diff)
        for s, c in zip(op[1], op[2]):
            self.given[s].append(c)

    def hits(self, K, label=""):
        every = list(range(self.case["nslots"]))
        hits, count = self.ms.hits(every, K)
        w_hits, w_count = PH.session_hits(self.given, self.case["targets"], K)
        diff = PH.same(hits, w_hits)
        assert diff is None, "%s hits %s after %d ops: %s" % (self.name, label, self.at, diff)
        assert np.array_equal(count, w_count), "%s hits %s: counts %s, want %s" % (self.name, label, count, w_count)
        return hits, count


def motif_expectations(script, W, mode, lo, hi):
    """per push of {"motifs", "nslots", "ops"}: (fields [K][m] as stream_ref.record gives them, chunks [m])"""
    raw = [np.zeros(0, dtype=np.int16) for _ in range(script["nslots"])]
    pushes = [0] * script["nslots"]
    want = []
    for op in script["ops"]:
        if op[0] == "reset":
            for s in op[1]:
                raw[s], pushes[s] = np.zeros(0, dtype=np.int16), 0
            continue
        for s, c in zip(op[1], op[2]):
            if len(c):
                raw[s] = np.concatenate([raw[s], c])
                pushes[s] += 1
        want.append(([[stream_ref.record(raw[s], mo, W, mode, lo, hi, False) for s in op[1]] for mo in script["motifs"]],
                     [pushes[s] for s in op[1]]))
    return want


def check_motif_records(rec, want, slots, label):
    """records STREAM_DTYPE [K, m] of one push against its entry of motif_expectations: doubles bit for bit, NaN == NaN"""
    fields, chunks = want
    assert rec.shape == (len(fields), len(slots)), label
    for k, row in enumerate(fields):
        for i, w in enumerate(row):
            got = stream_ref.fields(rec[k, i])
            assert stream_ref.same(got, w), "%s motif %d slot %d: got %r want %r" % (label, k, int(slots[i]), got, w)
            assert int(rec[k, i]["chunks"]) == chunks[i], (label, k, i, int(rec[k, i]["chunks"]), chunks[i])


class MotifSteps(Steps):
    """an api.MotifStream under {"motifs", "nslots", "ops"}; want = motif_expectations(...)"""

    def __init__(self, ms, script, want, name="motif"):
        Steps.__init__(self, name, script["ops"])
        self.ms, self.want = ms, want

    def do(self, op, label):
        if op[0] == "reset":
            self.ms.reset(op[1])
            return
        check_motif_records(self.ms.push(op[1], op[2]), self.want[self.pushes], op[1], label)


class LiveSteps(Steps):
    """an api.LiveMap under an evstream_ref script; want = live_ref.run_script(..., rule)"""

    def __init__(self, lm, sess, want, rule, name="live"):
        Steps.__init__(self, name, sess["ops"])
        self.lm, self.sess, self.want, self.rule = lm, sess, want, rule

    def do(self, op, label):
        if op[0] == "reset":
            self.lm.reset(op[1])
            return
        res = self.lm.push(op[1], op[2], end=op[3], rule=self.rule)
        d = LR.check_push(res[0], res[1], self.lm.fetch(), res[2], self.want[self.at])
        assert d is None, "%s: %s\n%s" % (label, d, ER.describe_session(self.sess))
