"""GPU: filtered HMM sessions (sk_hmms_open_ex with SK_HMMS_FILTER, sk_hmms_filter*, api.HmmStream(filter=True)) against
tests/hmmfilter_ref.py.  Every comparison is == on bytes, every double by its bits, after every push: the definition has
no tolerance.  Reads have at most 400 samples so that the numpy statement stays fast."""
import ctypes as C

import numpy as np
import pytest

import hmmfilter_ref as FR
import hmmstream_ref as HR

pytestmark = pytest.mark.gpu

NINF = -np.inf
N = 300                                                                  # samples of the cut grid's read
# chunk lengths of the cut grid, each a cycle: peeks between chunks, 1, 2, the seams of the int16 tile (128 samples) and of
# the float64 tile (32 values), and the whole read
CUTS = ((1,), (2,), (0, 3, 0, 0, 40), (127,), (128,), (129,), (31,), (32,), (33,), (N,))
LAYOUTS = ((64, 0), (63, 2), (63, 0), (64, 2), (64, 8), (61, 6))          # device rows: (stride in samples, byte shift of the base)
MODELS = ("S1", "loop", "synth_raw", "rna_pa", "dead_end")


@pytest.fixture(autouse=True)
def no_guard_hit(gpu):
    yield
    from squigglekit_amd import api
    assert api.last_hmm_stream_plan()["guard_hits"] == 0


def levels(rng, n):
    return rng.integers(380, 620, n).astype(np.int16)


def small_ints(rng, n):
    return rng.integers(0, 4, n).astype(np.int16)


def model_case(which):
    """(model, int16 read of N samples, calibration pair or None)"""
    from squigglekit_amd import api
    rng = np.random.default_rng(20261021 + MODELS.index(which))
    if which == "S1":
        m = HR.tie_model(rng, 1)
        m["linit"][0] = -1.0
        m["ltrans"][0, 0] = -2.0                                         # the one state can stay: the read is possible
        return m, small_ints(rng, N), None
    if which == "loop":
        return FR.loop_model(), small_ints(rng, N), None
    if which == "dead_end":
        return FR.dead_end_model(), small_ints(rng, N), None
    if which == "synth_raw":
        return api.polya_model("synth_raw"), HR.small_drna_read(rng, N), None
    raw = np.rint(HR.small_drna_read(rng, N).astype(np.float64) / 5.3 / 0.1825 - 3.0).astype(np.int16)
    return api.polya_model("rna_pa"), raw, (3.0, 0.1825)


_tables = {}


def prefix_table(which):
    """the statement's (records, filters) after each prefix of the model's read: table[n], computed once per model (one
    slot, one sample per push -- by the definition a slot's filter depends on nothing but its own samples)"""
    if which not in _tables:
        model, x, cal = model_case(which)
        ref = FR.Session(model, 1)
        if cal is not None:
            ref.reset([0], [cal])
        rec, filt = [ref.records([0])[0]], [ref.filter([0])[0]]
        for t in range(len(x)):
            rec.append(ref.push([0], [x[t:t + 1]], "i16")[0])
            filt.append(ref.filter([0])[0])
        _tables[which] = (np.array(rec, dtype=HR.DTYPE), np.array(filt, dtype=FR.FILT_DTYPE))
    return _tables[which]


@pytest.mark.parametrize("which", MODELS)
def test_cut_grid(gpu, which):
    """one read under every chunk cycle of CUTS, through the int16 feed (slots [0, G)) and, fed the same values, the
    float64 feed (slots [G, 2 G)) of one filtered session; a plain session takes the same pushes.  After every push the
    filter is the statement's, the records are the statement's and the plain session's; at the end the filter is the
    one-shot call's loglik and final_post of the whole read."""
    from squigglekit_amd import api
    model, x, cal = model_case(which)
    trec, tfilt = prefix_table(which)
    lm = HR.lib_model(model)
    G = len(CUTS)
    xv = x.astype(np.float64) if cal is None else (x.astype(np.float64) + cal[0]) * cal[1]
    if which == "dead_end":
        assert (tfilt["flags"][4:] == FR.IMPOSSIBLE).all() and (tfilt["flags"][1:3] == 0).all()
    else:
        assert (tfilt["flags"] == 0).all() and (abs(tfilt["post"][1:].sum(axis=1) - 1.0) < 1e-9).all()
    with api.HmmStream(lm, 2 * G, filter=True) as hs, api.HmmStream(lm, 2 * G) as plain:
        if cal is not None:
            for h in (hs, plain):
                h.reset(np.arange(G), np.tile(np.array(cal), (G, 1)))
        assert hs.filter(np.arange(2 * G)).tobytes() == FR.empty_filters(2 * G).tobytes()
        at = np.zeros(G, dtype=np.int64)
        turn, pushes = 0, np.zeros(G, dtype=np.int64)
        while (at < N).any():
            live = np.flatnonzero(at < N)
            cut = [CUTS[g][turn % len(CUTS[g])] for g in live]
            chunks = [x[at[g]:at[g] + c] for g, c in zip(live, cut)]
            at[live] += [len(c) for c in chunks]
            pushes[live] += [len(c) > 0 for c in chunks]
            turn += 1
            want = trec[at[live]].copy()
            want["pushes"] = pushes[live]
            got = hs.push(live, chunks)
            HR.assert_records(got, want, live, "%s int16 feed, push %d" % (which, turn))
            assert plain.push(live, chunks).tobytes() == got.tobytes()
            FR.assert_filters(hs.filter(live), tfilt[at[live]], live, "%s int16 feed, push %d" % (which, turn))
            values = [xv[a - len(c):a] for a, c in zip(at[live], chunks)]
            got = hs.push_values(live + G, values)
            HR.assert_records(got, want, live + G, "%s float64 feed, push %d" % (which, turn))
            assert plain.push_values(live + G, values).tobytes() == got.tobytes()
            FR.assert_filters(hs.filter(live + G), tfilt[at[live]], live + G, "%s float64 feed, push %d" % (which, turn))
        last = hs.filter(np.arange(2 * G))
        assert hs.peek(np.arange(2 * G)).tobytes() == plain.peek(np.arange(2 * G)).tobytes()
    post = api.hmm_posterior_batch(x[None, :], None, lm, None if cal is None else np.array([cal]))[0][0]
    fpost = api.hmm_posterior_ragged_f64(xv, [0, N], lm)[0][0]
    for one in (post, fpost):
        assert one["n_used"] == N and one["flags"] == tfilt[N]["flags"]
        assert all(f["loglik"].tobytes() == one["loglik"].tobytes() and f["post"].tobytes() == one["final_post"].tobytes()
                   and f["n_used"] == N and f["flags"] == one["flags"] for f in last), (one, last[0])


def can_stay(m):
    """every state of a drawn tie model can stay: the reads do not all turn impossible"""
    d = np.arange(m["nstates"])
    m["ltrans"][d, d] = np.where(np.isfinite(m["ltrans"][d, d]), m["ltrans"][d, d], -1.0)
    return m


def premises(sess, want, pushes):
    """what the drawn script must hold for the test to mean something, from the statement alone"""
    resets = [op for op in sess["ops"] if op[0] == "reset"]
    assert any(op[2] is not None for op in resets) and any(op[2] is None for op in resets)
    assert {op[3] for op in sess["ops"] if op[0] == "push"} == {"i16", "f64"}
    assert len(want) >= pushes and max(int(w[1]["n_used"].max()) for w in want) <= 400


@pytest.mark.parametrize("S, seed", [(1, 161), (63, 224), (64, 227), (65, 233), (130, 297)])
def test_wave_mates(gpu, S, seed):
    """pushes that name a shuffled subset: fresh, continuing and peeked slots in one wavefront, chunk lengths 0 .. 60,
    both feeds, resets in mid-read, calibrated slots next to uncalibrated ones; a plain session beside the filtered one"""
    from squigglekit_amd import api
    rng = np.random.default_rng(seed)
    model, draw = {1: (FR.loop_model(), small_ints), 63: (api.polya_model("synth_raw"), levels), 64: (FR.loop_model(), small_ints),
                   65: (can_stay(HR.tie_model(rng, 6)), small_ints), 130: (api.polya_model("synth_raw"), levels)}[S]
    sess = HR.draw_session(rng, nslots=S, budget=200 + 200 * S, maxlen=60, draw_chunk=draw)
    want = FR.run_session(model, sess)
    premises(sess, want, 10)
    assert sum(int((w[1]["flags"] == 0).sum()) for w in want) > 10
    assert FR.play_session(api, model, sess, "wave mates S=%d" % S, want) == len(want)


@pytest.mark.parametrize("kind, seed", [("tie", 20261040), ("rna_pa", 20261034), ("dead_end", 20261041)])
def test_random_sessions(gpu, kind, seed):
    """three seeded sessions drawn with hmmstream_ref.draw_session; the slot count and the longest chunk are drawn too.  A
    drawn tie model, the pA preset (levels of a raw read under drawn calibration pairs), and the model whose reads turn
    impossible after three samples"""
    from squigglekit_amd import api
    rng = np.random.default_rng(seed)
    model, draw = {"tie": (can_stay(HR.tie_model(rng)), small_ints), "rna_pa": (api.polya_model("rna_pa"), levels),
                   "dead_end": (FR.dead_end_model(), small_ints)}[kind]
    nslots = int(rng.integers(2, 90))
    sess = HR.draw_session(rng, nslots=nslots, budget=200 * nslots, maxlen=int(rng.integers(1, 90)), draw_chunk=draw)
    want = FR.run_session(model, sess)
    premises(sess, want, 8)
    impossible = sum(int((w[1]["flags"] != 0).sum()) for w in want)
    assert impossible > 10 if kind == "dead_end" else impossible == 0
    assert FR.play_session(api, model, sess, "random session (%s)" % kind, want) == len(want)


def test_device_forms_and_row_layouts(gpu):
    """push_dev_* and sk_hmms_filter_dev on device buffers.  The int16 rows take LAYOUTS in turn: the aligned one (16-byte
    loads) and odd strides and bases shifted by 2, 6 and 8 bytes (2-byte loads).  Every push and every filter call carries
    two entries that name no slot of the session: their records are empty / all zero and nobody else is touched; the
    filter call names one slot twice."""
    from squigglekit_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(10)
    S, M = 70, 73
    ran = []
    model = api.polya_model("synth_raw")
    sess = HR.draw_session(rng, nslots=S, budget=14000, maxlen=60, draw_chunk=levels)
    want = FR.run_session(model, sess)
    d_rows, d_vals = L.sk_dev_alloc(M * 64 * 2 + 16), L.sk_dev_alloc(M * 60 * 8 + 8)
    d_slots, d_len, d_off, d_out, d_filt = (L.sk_dev_alloc(n) for n in (M * 4, M * 4, (M + 1) * 8, M * 96, M * 64))
    up = lambda d, a: _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))   # noqa: E731
    try:
        with api.HmmStream(model, S, filter=True) as dev:
            j = 0
            for op in sess["ops"]:
                if op[0] == "reset":
                    dev.reset(op[1], op[2])
                    continue
                _, slots, chunks, feed = op
                m = len(slots) + 2
                named = np.concatenate([slots[:1], [S], slots[1:], [-1]]).astype(np.int32)   # entries 1 and m - 1 name no slot
                parts = chunks[:1] + [levels(rng, 9).astype(chunks[0].dtype)] + chunks[1:] + [levels(rng, 5).astype(chunks[0].dtype)]
                lens = np.array([len(c) for c in parts], dtype=np.int32)
                up(d_slots, named)
                if feed == "i16":
                    stride, shift = LAYOUTS[len(ran) % len(LAYOUTS)]
                    ran.append((stride, shift))
                    rows = np.full((m, stride), -12345, dtype=np.int16)
                    for i, c in enumerate(parts):
                        rows[i, :len(c)] = c
                    up(d_rows + shift, rows)
                    up(d_len, lens)
                    _lib.check(L.sk_hmms_push_dev_i16(dev.handle, d_slots, m, d_rows + shift, stride, d_len, d_out))
                else:
                    off = np.zeros(m + 1, dtype=np.int64)
                    off[1:] = np.cumsum(lens)
                    up(d_vals, np.concatenate(parts + [np.zeros(1)]))
                    up(d_off, off)
                    _lib.check(L.sk_hmms_push_dev_f64(dev.handle, d_slots, m, d_vals, d_off, d_out))
                got = np.zeros(m, dtype=api.HMMS_DTYPE)
                _lib.check(L.sk_dev_download(_lib.ptr(got), d_out, got.nbytes))
                assert got[[1, m - 1]].tobytes() == HR.empty_records(2).tobytes(), j
                HR.assert_records(np.delete(got, [1, m - 1]), want[j][0], slots, "device form, push %d (%s)" % (j, feed), sess)
                # the filter of the same entries, and entry 0's slot once more at the end
                again = np.concatenate([named, named[:1]]).astype(np.int32)
                up(d_slots, again)
                filt = np.full(m + 1, 0xAB, dtype=np.uint8).repeat(64).view(api.HMMS_FILT_DTYPE)
                up(d_filt, filt)
                _lib.check(L.sk_hmms_filter_dev(dev.handle, d_slots, m + 1, d_filt))
                _lib.check(L.sk_dev_download(_lib.ptr(filt), d_filt, filt.nbytes))
                assert filt[[1, m - 1]].tobytes() == FR.empty_filters(2).tobytes(), (j, filt[[1, m - 1]])
                FR.assert_filters(np.delete(filt[:m], [1, m - 1]), want[j][1], slots, "device form, filter %d (%s)" % (j, feed))
                assert filt[m].tobytes() == filt[0].tobytes()
                assert dev.filter(slots).tobytes() == want[j][1].tobytes()      # the host form reads what the device forms wrote
                j += 1
            feeds = [op[3] for op in sess["ops"] if op[0] == "push"]
            assert {"f64"} < set(feeds) and set(ran) == set(LAYOUTS)     # both feeds and every layout ran
    finally:
        for p in (d_rows, d_vals, d_slots, d_len, d_off, d_out, d_filt):
            L.sk_dev_free(p)


def test_reset_in_mid_read_and_a_slot_twice(gpu):
    from squigglekit_amd import api
    model, x, _ = model_case("synth_raw")
    _, tfilt = prefix_table("synth_raw")
    with api.HmmStream(model, 3, filter=True) as hs:
        hs.push([0, 1, 2], [x[:100], x[:200], x[:0]])
        assert hs.filter([1, 0, 1, 2]).tobytes() == tfilt[[200, 100, 200, 0]].tobytes()
        hs.reset([1])
        assert hs.filter([1, 0]).tobytes() == tfilt[[0, 100]].tobytes()
        hs.push([1, 2], [x[:150], x[:1]])                                # a fresh slot beside one that goes on elsewhere
        hs.push_values([0], [x[100:129].astype(np.float64)])
        assert hs.filter([0, 1, 2]).tobytes() == tfilt[[129, 150, 1]].tobytes()
        assert hs.filter([]).shape == (0,)


def test_plans_report_272_bytes_per_slot_filtered_and_224_plain(gpu):
    from squigglekit_amd import api
    model = api.polya_model("rna_pa")
    chunk = [np.full(10, 500, dtype=np.int16)]
    with api.HmmStream(model, 3000, filter=True) as hf, api.HmmStream(model, 3000) as hp:
        hf.push([5], chunk)
        assert api.last_hmm_stream_plan() == {"state_bytes": 3000 * 272, "guard_hits": 0}
        hp.push([5], chunk)
        assert api.last_hmm_stream_plan() == {"state_bytes": 3000 * 224, "guard_hits": 0}
        hf.push_values([7], [np.zeros(0)])
        assert api.last_hmm_stream_plan()["state_bytes"] == 3000 * 272
        assert hf.filter([5, 7, 2999])["n_used"].tolist() == [10, 0, 0]


def test_session_side_refusals_leave_out_untouched(gpu):
    """Through the C entries, by return code: a handle opened without SK_HMMS_FILTER, a handle that was closed, a slot at
    or above nslots -- in that order where two apply -- and out is as it was.  flags == 0 is sk_hmms_open."""
    from squigglekit_amd import _lib, api
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    model = api.polya_model("synth_raw")
    out = np.full(64 * 2, 0xAB, dtype=np.uint8)
    d_slots, d_out = L.sk_dev_alloc(8), L.sk_dev_alloc(128)
    _lib.check(L.sk_dev_upload(d_slots, _lib.ptr(i32(0, 1)), 8))
    _lib.check(L.sk_dev_upload(d_out, _lib.ptr(out), 128))

    def refused(rc, words):
        msg = L.sk_last_error().decode()
        assert rc == INV and words in msg, (rc, msg)
        assert np.all(out == 0xAB)
        back = np.zeros(128, dtype=np.uint8)
        _lib.check(L.sk_dev_download(_lib.ptr(back), d_out, 128))
        assert np.all(back == 0xAB)

    try:
        h = C.c_int32(-1)
        _lib.check(L.sk_hmms_open_ex(C.byref(model), 2, 0, C.byref(h)))     # flags == 0: a plain session
        plain = h.value
        with api.HmmStream(model, 2, filter=True) as hf:
            assert hf.handle != plain
            x = levels(np.random.default_rng(3), 20)
            rec = np.zeros(1, dtype=api.HMMS_DTYPE)
            _lib.check(L.sk_hmms_push_i16(plain, _lib.ptr(i32(1)), 1, _lib.ptr(x), 20, _lib.ptr(i32(20)), _lib.ptr(rec)))
            assert rec.tobytes() == hf.push([0], [x]).tobytes()
            assert api.last_hmm_stream_plan()["state_bytes"] == 2 * 272
            refused(L.sk_hmms_filter(plain, _lib.ptr(i32(0, 1)), 2, _lib.ptr(out)), "opened without SK_HMMS_FILTER")
            refused(L.sk_hmms_filter_dev(plain, d_slots, 2, d_out), "opened without SK_HMMS_FILTER")
            refused(L.sk_hmms_filter(plain, _lib.ptr(i32(0, 2)), 2, _lib.ptr(out)), "entry 1: slot 2 is outside [0, 2)")
            refused(L.sk_hmms_filter(hf.handle, _lib.ptr(i32(2, 0)), 2, _lib.ptr(out)), "entry 0: slot 2 is outside [0, 2)")
            before = hf.filter([0, 1])
            assert before["n_used"].tolist() == [20, 0]
            gone = hf.handle
        for handle in (gone, 7):                                         # closed, and never opened
            refused(L.sk_hmms_filter(handle, _lib.ptr(i32(0, 1)), 2, _lib.ptr(out)), "unknown HMM session handle %d" % handle)
            refused(L.sk_hmms_filter_dev(handle, d_slots, 2, d_out), "unknown HMM session handle %d" % handle)
        with pytest.raises(ValueError):
            hf.filter([0])
        _lib.check(L.sk_hmms_close(plain))
    finally:
        L.sk_dev_free(d_slots)
        L.sk_dev_free(d_out)
