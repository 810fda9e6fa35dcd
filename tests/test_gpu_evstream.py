"""GPU: event sessions (sk_evs_*, api.EventStream) against tests/evstream_ref.py.  Every comparison is == on bytes: the
definition has no tolerance.  After every push the records are the reference's, an ended read's concatenation is the
one-shot api.detect_events output, and guard_hits is 0 after every test."""
import numpy as np
import pytest

import detect_ref
import evstream_ref as ER

pytestmark = pytest.mark.gpu

DNA, RNA = detect_ref.PRESETS["dna"], detect_ref.PRESETS["rna"]
W64 = (64, 64, 2.0, 3.0, 0.1)


@pytest.fixture(autouse=True)
def no_guard_hit(gpu):
    yield
    from squigglekit_amd import api
    assert api.last_event_plan()["guard_hits"] == 0


def i16(a):
    return np.asarray(a, dtype=np.int16)


def script_of_cuts(params, reads, cuts_per_read, end_with_last=True):
    """One slot per read: push j names every slot that still has chunks, slot s getting its j-th chunk; END with a
    slot's last chunk (or as an empty chunk of its own behind it)."""
    plans = []
    for x, cuts in zip(reads, cuts_per_read):
        parts, at = [], 0
        for c in cuts:
            parts.append(x[at:at + c])
            at += c
        assert at == len(x)
        if not end_with_last or not parts:
            parts.append(x[:0])
        plans.append(parts)
    ops = []
    for j in range(max(len(p) for p in plans)):
        slots = [s for s, p in enumerate(plans) if j < len(p)]
        ops.append(("push", np.array(slots, dtype=np.int32), [plans[s][j] for s in slots],
                    np.array([j == len(plans[s]) - 1 for s in slots], dtype=np.int32)))
    return {"params": params, "nslots": len(reads), "ops": ops}


def even_cuts(n, c):
    return [c] * (n // c) + ([n % c] if n % c else [])


@pytest.mark.parametrize("preset", ["dna", "rna"])
def test_cut_grid(gpu, preset):
    """one read of about 3 000 samples under every chunk length of the grid, and whole, each in a slot of one session"""
    from squigglekit_amd import api
    params = detect_ref.PRESETS[preset]
    wl = params[1]
    x = ER.draw_read(np.random.default_rng(3), 3011, "steps")
    grid = [1, wl - 1, wl, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4097, len(x)]
    sess = script_of_cuts(params, [x] * len(grid), [even_cuts(len(x), c) for c in grid])
    assert ER.play_session(api, sess, "cut grid " + preset) == len(grid)
    assert len(detect_ref.events(x, params)) > 50


@pytest.mark.parametrize("S", [1, 64, 65, 130])
def test_wave_mates(gpu, S):
    """pushes that name a shuffled subset: fresh, continuing, ending slots and empty chunks in the same wavefront, chunk
    lengths 0 .. 300"""
    from squigglekit_amd import api
    rng = np.random.default_rng(40 + S)
    for _ in range(2):
        sess = ER.draw_session(rng, nslots=S, budget=12000, maxlen=300)
        ER.play_session(api, sess, "wave mates S=%d" % S)


@pytest.mark.parametrize("params", [DNA, RNA, W64, (1, 1, 0.5, 2.0, 0.0)])
def test_short_reads(gpu, params):
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    lens = [0, 1, 2 * params[0] - 1, 2 * params[1] - 1, 2 * params[1]]
    reads = [ER.draw_read(rng, n, "clean") for n in lens]
    ER.play_session(api, script_of_cuts(params, reads, [[n] if n else [] for n in lens]), "short, at once")
    ER.play_session(api, script_of_cuts(params, reads, [[1] * n for n in lens]), "short, sample by sample")
    ER.play_session(api, script_of_cuts(params, reads, [[1] * n for n in lens], end_with_last=False), "short, END alone")


def test_value_corners(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(6)
    const = np.full(700, -123, dtype=np.int16)                          # v clamps to 1 everywhere
    hi = np.tile(i16([32767, 0]), 200)
    lo = np.tile(i16([-32768, 0]), 200)
    both = np.tile(i16([32767, -32768]), 200)
    extremes = np.concatenate([hi, lo, both, np.full(150, 32767, dtype=np.int16), np.full(150, -32768, dtype=np.int16), hi])
    ties = [ER.draw_read(rng, 900, "ties") for _ in range(3)]
    for params in (DNA, W64, (1, 64, 1.0, 2.0, 0.0)):
        reads = [const, extremes] + ties
        cuts = [even_cuts(len(r), c) for r, c in zip(reads, (130, 97, 1000, 64, 129))]
        ER.play_session(api, script_of_cuts(params, reads, cuts), "value corners %r" % (params,))


def test_long_event(gpu):
    """one event far longer than any staging row or tile: nothing depends on keeping an event's samples"""
    from squigglekit_amd import api
    rng = np.random.default_rng(7)
    x = np.concatenate([np.full(20000, 411, dtype=np.int16), ER.draw_read(rng, 2500, "steps")])
    ev = detect_ref.events(x, DNA)
    assert ev["length"][0] >= 20000 - 6
    ER.play_session(api, script_of_cuts(DNA, [x, x], [even_cuts(len(x), 1000), even_cuts(len(x), 4097)]), "long event")


def test_reset_mid_read_and_a_push_to_an_ended_slot(gpu):
    from squigglekit_amd import _lib, api
    rng = np.random.default_rng(8)
    a, b, c = (ER.draw_read(rng, n, k) for n, k in ((700, "steps"), (900, "walk"), (500, "steps")))
    e0, e1 = np.zeros(2, dtype=np.int32), np.array([1, 0], dtype=np.int32)
    two = np.array([0, 1], dtype=np.int32)
    sess = {"params": DNA, "nslots": 2, "ops": [
        ("push", two, [a[:300], c[:100]], e0),
        ("reset", np.array([0], dtype=np.int32)),                      # mid-read: slot 0 starts a different read
        ("push", two, [b[:450], c[100:101]], e0),
        ("push", two, [b[450:], c[101:330]], e1),                      # slot 0 ends
        ("push", two, [b[:0], c[330:]], np.array([1, 1], dtype=np.int32)),   # an empty chunk for an ended slot does nothing
    ]}
    ER.play_session(api, sess, "reset mid-read")
    # samples for an ended slot: refused, and nothing changes -- not for the other slot of the push either
    with api.EventStream(_lib.DetParams(*DNA), 2) as es:
        off0, rec0 = es.push([0, 1], [a[:200], c[:200]], end=[1, 0])
        assert rec0[off0[0]:off0[1]].tobytes() == detect_ref.events(a[:200], DNA).tobytes()
        with pytest.raises(_lib.SquiggleKitError) as ei:
            es.push([1, 0], [c[200:300], a[200:210]])
        assert ei.value.code == _lib.SK_ERR_INVALID and "slot 0 has ended" in str(ei.value), str(ei.value)
        off, rec1 = es.push([1], [c[200:]], end=[1])
        got = np.concatenate([rec0[off0[1]:off0[2]], rec1])
        assert got.tobytes() == detect_ref.events(c, DNA).tobytes()
        es.reset([0])
        off, rec = es.push([0], [a], end=[1])
        assert rec.tobytes() == detect_ref.events(a, DNA).tobytes()


def test_refusals_that_need_the_session(gpu):
    """Through the C entries, by return code: push (both forms), fetch, reset and close on a handle inside [0, 8) that was
    never opened and on one that has been closed; push and reset with slot == nslots -- and off, rec and the session are
    as they were.  (Samples for an ended slot: the test above.  The one refusal left, a slot whose total would pass
    2^31 - 1 samples, needs 4 GiB of pushes and is out of a test's reach: it is not tested.)"""
    import ctypes as C
    from squigglekit_amd import _lib, api
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    x, y = (ER.draw_read(np.random.default_rng(12 + k), 900, "steps") for k in range(2))
    params = _lib.DetParams(*DNA)
    off = np.full(3, -5, dtype=np.int64)
    rec = np.full(600, 0xAB, dtype=np.uint8)
    cap = rec.size // 24

    def push(fn, handle, slots, chunks, end=None):
        rows, lens = api.pack_i16(chunks)
        return getattr(L, fn)(handle, _lib.ptr(slots), len(slots), _lib.ptr(rows), rows.shape[1], _lib.ptr(lens),
                              None if end is None else _lib.ptr(end), _lib.ptr(off), _lib.ptr(rec), cap)

    def refused(rc, words):
        msg = L.sk_last_error().decode()
        assert rc == INV and words in msg, (rc, msg)
        assert np.all(off == -5) and np.all(rec == 0xAB)                # nothing was written

    def unknown(handle):
        words = "unknown event session handle %d" % handle
        refused(push("sk_evs_push_i16", handle, i32(0), [x[:10]]), words)
        refused(push("sk_evs_push_dev_i16", handle, i32(0), [x[:10]]), words)   # (refused before a pointer is followed)
        refused(L.sk_evs_fetch(handle, _lib.ptr(rec), cap), words)
        refused(L.sk_evs_reset(handle, _lib.ptr(i32(0)), 1), words)
        refused(L.sk_evs_close(handle), words)

    h = C.c_int32(-1)
    _lib.check(L.sk_evs_open(C.byref(params), 2, C.byref(h)))
    handle = h.value
    try:
        never = 7 if handle != 7 else 6                                 # (sessions take the lowest free handle)
        unknown(never)
        first = np.zeros(3, dtype=np.int64)
        got = np.zeros(400, dtype=api.DET_EVENT_DTYPE)
        rows, lens = api.pack_i16([x[:500], y[:300]])
        _lib.check(L.sk_evs_push_i16(handle, _lib.ptr(i32(0, 1)), 2, _lib.ptr(rows), rows.shape[1], _lib.ptr(lens), None,
                                     _lib.ptr(first), _lib.ptr(got), got.size))
        parts = [[got[first[0]:first[1]].copy()], [got[first[1]:first[2]].copy()]]
        # slot == nslots: push and reset are refused, whatever else they name
        refused(push("sk_evs_push_i16", handle, i32(1, 2), [y[300:400], x[:50]]), "entry 1: slot 2 is outside [0, 2)")
        refused(L.sk_evs_reset(handle, _lib.ptr(i32(0, 2)), 2), "entry 1: slot 2 is outside [0, 2)")
        # ... and the session is as it was: the last push's records are still there, both reads go on and end as ever
        again = np.zeros(int(first[2]), dtype=api.DET_EVENT_DTYPE)
        _lib.check(L.sk_evs_fetch(handle, _lib.ptr(again), again.size))
        assert again.tobytes() == got[:int(first[2])].tobytes()
        o, r = np.zeros(3, dtype=np.int64), np.zeros(600, dtype=api.DET_EVENT_DTYPE)
        rows, lens = api.pack_i16([y[300:], x[500:]])
        _lib.check(L.sk_evs_push_i16(handle, _lib.ptr(i32(1, 0)), 2, _lib.ptr(rows), rows.shape[1], _lib.ptr(lens),
                                     _lib.ptr(i32(1, 1)), _lib.ptr(o), _lib.ptr(r), r.size))
        parts[1].append(r[o[0]:o[1]])
        parts[0].append(r[o[1]:o[2]])
        assert np.concatenate(parts[0]).tobytes() == detect_ref.events(x, DNA).tobytes()
        assert np.concatenate(parts[1]).tobytes() == detect_ref.events(y, DNA).tobytes()
    finally:
        assert L.sk_evs_close(handle) == 0
    unknown(handle)                                                     # closed: as if never opened


def test_overflow_keeps_the_records_for_fetch(gpu):
    from squigglekit_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(9)
    xs = [ER.draw_read(rng, 1500, "steps") for _ in range(3)]
    sess = script_of_cuts(DNA, xs, [[600, 500, 400]] * 3)
    want = ER.run_session(sess)
    params = _lib.DetParams(*DNA)
    slots = np.arange(3, dtype=np.int32)
    with api.EventStream(params, 3) as es:
        for j, op in enumerate(sess["ops"]):
            rows, lens = api.pack_i16(op[2])
            off = np.full(4, -1, dtype=np.int64)
            w_off, w_rec = want[j]
            if j == 1:                                                  # too little room: off complete, rec untouched
                small = np.full(3 * 24, 0xAB, dtype=np.uint8)
                rc = L.sk_evs_push_i16(es.handle, _lib.ptr(slots), 3, _lib.ptr(rows), rows.shape[1], _lib.ptr(lens),
                                       _lib.ptr(op[3]), _lib.ptr(off), _lib.ptr(small), 3)
                assert rc == _lib.SK_ERR_OVERFLOW and np.array_equal(off, w_off) and np.all(small == 0xAB)
                assert int(off[3]) > 3
                assert L.sk_evs_fetch(es.handle, _lib.ptr(small), 3) == _lib.SK_ERR_OVERFLOW and np.all(small == 0xAB)
                rec = np.zeros(int(off[3]) + 2, dtype=api.DET_EVENT_DTYPE)
                _lib.check(L.sk_evs_fetch(es.handle, _lib.ptr(rec), rec.size))
                assert rec[:int(off[3])].tobytes() == w_rec.tobytes()
                _lib.check(L.sk_evs_fetch(es.handle, _lib.ptr(rec), rec.size))       # as often as asked
                assert rec[:int(off[3])].tobytes() == w_rec.tobytes()
                continue
            o, rec = es.push(slots, op[2], end=op[3])                   # the pushes around it are as ever
            assert np.array_equal(o, w_off) and rec.tobytes() == w_rec.tobytes(), j


def test_device_entry_gives_the_bytes_of_the_host_entry(gpu):
    from squigglekit_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(10)
    S, stride, cap = 70, 304, 70 * 200
    params = _lib.DetParams(*RNA)
    sess = ER.draw_session(rng, nslots=S, budget=9000, maxlen=300)
    sess["params"] = RNA
    want = ER.run_session(sess)
    d_rows, d_slots, d_len, d_end = (L.sk_dev_alloc(n) for n in (S * stride * 2, S * 4, S * 4, S * 4))
    d_off, d_rec = L.sk_dev_alloc((S + 1) * 8), L.sk_dev_alloc(cap * 24)
    try:
        with api.EventStream(params, S) as dev, api.EventStream(params, S) as host:
            j = 0
            for op in sess["ops"]:
                if op[0] == "reset":
                    dev.reset(op[1])
                    host.reset(op[1])
                    continue
                _, slots, chunks, end = op
                m = len(slots)
                rows = np.zeros((m, stride), dtype=np.int16)
                lens = np.array([len(c) for c in chunks], dtype=np.int32)
                for i, c in enumerate(chunks):
                    rows[i, :len(c)] = c
                for d, a in ((d_rows, rows), (d_slots, slots), (d_len, lens), (d_end, np.ascontiguousarray(end, dtype=np.int32))):
                    _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))
                _lib.check(L.sk_evs_push_dev_i16(dev.handle, d_slots, m, d_rows, stride, d_len, d_end, d_off, d_rec, cap))
                off = np.zeros(m + 1, dtype=np.int64)
                _lib.check(L.sk_dev_download(_lib.ptr(off), d_off, off.nbytes))
                w_off, w_rec = want[j]
                j += 1
                assert np.array_equal(off, w_off), (j, ER.describe_session(sess))
                rec = np.zeros(max(int(off[m]), 1), dtype=api.DET_EVENT_DTYPE)
                _lib.check(L.sk_dev_download(_lib.ptr(rec), d_rec, int(off[m]) * 24 or 8))
                assert rec[:int(off[m])].tobytes() == w_rec.tobytes(), (j, ER.describe_session(sess))
                h_off, h_rec = host.push(slots, chunks, end=end)        # the host entry: the same bytes
                assert h_off.tobytes() == off.tobytes() and h_rec.tobytes() == rec[:int(off[m])].tobytes(), j
            # the host form after device-form pushes: it knows which slots have ended
            with pytest.raises(_lib.SquiggleKitError) as ei:
                dev.push([0], [np.ones(5, dtype=np.int16)])             # (the script's last op ended every slot)
            assert "has ended" in str(ei.value)
    finally:
        for p in (d_rows, d_slots, d_len, d_end, d_off, d_rec):
            L.sk_dev_free(p)


def test_plan_reports_state_and_staging(gpu):
    from squigglekit_amd import _lib, api
    with api.EventStream(_lib.DetParams(*DNA), 3000) as es:
        es.push([5, 7], [np.zeros(100, dtype=np.int16), np.zeros(40, dtype=np.int16)])
        plan = api.last_event_plan()
    assert plan["state_bytes"] == 3000 * 416 and plan["state_bytes"] / 3000 < 512
    assert plan["staged_records"] == 2 * ((100 + 6) // 2 + 3) and plan["guard_hits"] == 0


# ---- command line ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_chunk", [2000, 777])
def test_cli_live_ends_on_the_lines_of_the_event_space_replay(gpu, tmp_path, sample_chunk):
    """--live with thresholds that can neither accept nor give up: every read prints `end`, and its first ten columns and
    events_seen are the non-live run's with the same --calib (MapStream's record does not depend on the cuts)"""
    from squigglekit_amd.mapstream_cli import HEADER, main
    from test_gpu_mapstream import run_cli, synthetic_input
    path, model, reads, _ = synthetic_input(tmp_path)
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", str(reads.shape[1]), "--calib", "40", "--channels", "3",
            "--min_events", "1000000", "--give_up", "1000000"]
    so, se, code = run_cli(main, base + ["--chunk", "37"])
    assert code == 0, se
    want = {ln.split("\t")[0]: ln.split("\t") for ln in so.split("\n")[1:-1]}
    so, se, code = run_cli(main, base + ["--live", "--sample_chunk", str(sample_chunk)])
    assert code == 0, se
    lines = so.split("\n")
    assert lines[0] == "\t".join(HEADER) and lines[-1] == ""
    got = {ln.split("\t")[0]: ln.split("\t") for ln in lines[1:-1]}
    assert sorted(got) == sorted(want) and len(got) == 8
    for rid, cols in got.items():
        assert cols[:10] == want[rid][:10] and cols[12] == want[rid][12], (rid, cols, want[rid])
        assert cols[10] == want[rid][10] == ("." if rid == "6" else "end"), (rid, cols)
    assert int(got["7"][12]) > 1024
