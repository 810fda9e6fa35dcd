"""GPU: the reference pile-up (sk_pileup, sk_pileup.hip) against tests/pileup_ref.py, which states the contract in numpy.
Every comparison is on bytes: pile.tobytes(), ent_off, ent_row.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import pileup_cases as pc
import pileup_ref as pr

pytestmark = pytest.mark.gpu


def both(kw, ref=None):
    """the case through the library (with the inverted index) and through the reference; asserts they agree"""
    from squigglekit_amd import api
    pile, ent_off, ent_row = api.pileup(entries=True, **kw)
    wpile, woff, wrow = ref if ref is not None else pr.pileup_ref(**kw)
    assert pile.dtype == api.PILE_DTYPE and pile.dtype == pr.PILE_DTYPE
    assert np.array_equal(ent_off, woff), np.flatnonzero(ent_off != woff)[:5]
    assert np.array_equal(ent_row, wrow), np.flatnonzero(ent_row != wrow)[:5]
    if pile.tobytes() != wpile.tobytes():
        bad = [m for m in range(len(pile)) if pile[m].tobytes() != wpile[m].tobytes()][:3]
        raise AssertionError("points %s: got %s, want %s" % (bad, [pile[m] for m in bad], [wpile[m] for m in bad]))
    assert api.pileup(**kw).tobytes() == wpile.tobytes()            # and without the index
    return pile, ent_off, ent_row


def test_hand_case(gpu):
    from squigglekit_amd import api
    kw = pc.hand_case()
    pile, ent_off, ent_row = both(kw)
    for m in range(14):
        assert ent_row[ent_off[m]:ent_off[m + 1]].tolist() == pc.HAND_LISTS.get(m, []), m
    for m, want in pc.HAND_RECORDS.items():
        assert pile[m].tolist()[:9] == want, m
    parts = api.pile_split(pile, kw["tlen"])
    assert [len(p) for p in parts] == [6, 0, 5, 3] and (parts[3]["n"] == 0).all() and np.isnan(parts[3]["level"]).all()
    plan = api.last_pileup_plan()
    assert plan["entries"] == 10 and plan["longest_list"] == 3 and plan["lists_in_long_tier"] == 0 and plan["scratch_bytes"] > 0


def test_numpys_summation_tiers(gpu):
    """list lengths on both sides of every boundary of numpy's summation: the serial loop below 8, one leaf up to 128, the
    pairwise tree, the 8 192-term buffers"""
    rng = np.random.default_rng(11)
    lengths = [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193]
    kw = pc.lists_case(rng, lengths)
    ref = pr.pileup_ref(**kw)
    differ = 0
    for k in range(len(lengths)):
        v = kw["value"][ref[2][ref[1][k]:ref[1][k + 1]]]
        assert v.size == lengths[k]
        differ += pr.naive_sum(v) != np.sum(v)
    assert differ >= 1, "a left-to-right sum gives numpy's bits on every list: the case proves nothing"
    both(kw, ref)


def test_ordering_under_contention(gpu):
    """2 000 pairs of 50 rows inside one 64-point target: every list is fed by many workgroups at once"""
    from squigglekit_amd import api
    rng = np.random.default_rng(12)
    kw = pc.paths_case(rng, 2000, 50, [64], stay=0.35, skip=0.25)
    ref = pr.pileup_ref(**kw)
    a = both(kw, ref)
    b = api.pileup(entries=True, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_every_ordering_tier(gpu, monkeypatch):
    """the LDS tier shrunk to 64 entries: lists of 63 and 64 stay in it, 65 and 5 000 take the merge tier"""
    from squigglekit_amd import api
    rng = np.random.default_rng(13)
    kw = pc.lists_case(rng, [63, 64, 65, 5000, 2, 0, 1])
    ref = pr.pileup_ref(**kw)
    monkeypatch.setenv("SK_PILE_LDS_ENTRIES", "64")
    small = both(kw, ref)
    plan = api.last_pileup_plan()
    assert plan["lists_in_long_tier"] == 2 and plan["longest_list"] == 5000 and plan["entries"] == 5195
    monkeypatch.setenv("SK_PILE_LDS_ENTRIES", "2")                  # the smallest tier: many merge passes
    tiny = both(kw, ref)
    assert api.last_pileup_plan()["lists_in_long_tier"] == 4              # 63, 64, 65 and 5 000
    monkeypatch.delenv("SK_PILE_LDS_ENTRIES")
    plain = both(kw, ref)
    assert api.last_pileup_plan()["lists_in_long_tier"] == 1        # 5 000 > 4 096
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(small, tiny, plain))


def test_the_long_tier_as_built(gpu, monkeypatch):
    """70 000 single-row pairs on one point, no tuning variable"""
    from squigglekit_amd import api
    monkeypatch.delenv("SK_PILE_LDS_ENTRIES", raising=False)
    rng = np.random.default_rng(14)
    kw = pc.lists_case(rng, [70000, 3], tlen_extra=2)
    both(kw)
    plan = api.last_pileup_plan()
    assert plan["lists_in_long_tier"] == 1 and plan["longest_list"] == 70000 and plan["entries"] == 70003


def test_long_spans(gpu):
    """a row that covers 5 000 points of a 6 000-point target beside ordinary rows; rows of exactly 64 and 65 points"""
    rng = np.random.default_rng(15)
    kw = pc.paths_case(rng, 30, (20, 80), [6000, 300])
    sp = kw["spans"]
    first = kw["span_off"][:-1]
    on0 = np.flatnonzero(kw["target"] == 0)
    sp[first[on0[0]] + 3] = (700, 5699)
    sp[first[on0[1]] + 1] = (100, 163)                              # 64 points: the lane walks it
    sp[first[on0[1]] + 2] = (164, 228)                              # 65: the wavefront takes it
    sp[first[on0[2]]] = (0, 5999)
    both(kw)


def test_nan_and_inf(gpu):
    """a list holding a NaN, one holding +inf and -inf, one holding +inf alone, one of equal values"""
    rng = np.random.default_rng(16)
    lengths = [9, 200, 5, 40, 1]
    kw = pc.lists_case(rng, lengths, values=rng.normal(size=sum(lengths)))
    pts = kw["spans"][:, 0]
    v = kw["value"]
    v[np.flatnonzero(pts == 0)[4]] = np.nan
    v[np.flatnonzero(pts == 1)[[17, 150]]] = (np.inf, -np.inf)
    v[np.flatnonzero(pts == 2)[0]] = np.inf
    v[pts == 3] = 0.5
    pile, _, _ = both(kw)
    assert np.isnan(pile["level"][:2]).all() and np.isnan(pile["vmin"][0]) and np.isnan(pile["vmax"][0])
    assert pile["vmin"][1] == -np.inf and pile["vmax"][1] == np.inf and np.isnan(pile["level_sd"][1])
    assert pile["level"][2] == np.inf and np.isnan(pile["level_sd"][2])
    assert pile["level_sd"][3] == 0.0 and pile["level"][3] == 0.5 and pile["level_sd"][4] == 0.0


# ---- refusals ----------------------------------------------------------------------------------------------------------
def raw_call(gpu, kw, out, ent_off, ent_row, cap):
    L = gpu.load()
    P, E = kw["span_off"].size - 1, len(kw["spans"])

    def p(a):
        return None if a is None else gpu.ptr(a if a.size else np.zeros(2, dtype=a.dtype))
    rc = L.sk_pileup(p(kw["span_off"]), p(kw["spans"]), p(kw["value"]), p(kw["dwell"]), p(kw["target"]), p(kw["shift"]),
                     p(kw["use"]), P, E, p(kw["tlen"]), kw["tlen"].size, p(out), p(ent_off), p(ent_row), cap)
    return rc, L.sk_last_error().decode()


def refused(gpu, kw, words, cap=None):
    mtot = int(np.maximum(kw["tlen"], 0).sum())
    out = np.full(mtot * 64, 0xAB, dtype=np.uint8)
    ent_off = np.full((mtot + 1) * 8, 0xAB, dtype=np.uint8)
    ent_row = np.full(4096 * 4, 0xAB, dtype=np.uint8)
    rc, msg = raw_call(gpu, kw, out, ent_off, ent_row, 4096 if cap is None else cap)
    assert rc == gpu.SK_ERR_INVALID and all(w in msg for w in words), (rc, msg)
    assert np.all(out == 0xAB) and np.all(ent_off == 0xAB) and np.all(ent_row == 0xAB), "a refused call wrote something"
    if cap is None:
        with pytest.raises(pr.Refused):
            pr.check(**kw)


def test_refusals_write_nothing_and_name_the_lowest_pair(gpu):
    base = pc.paths_case(np.random.default_rng(17), 12, 20, [80, 50])
    base["shift"], base["use"] = np.zeros(12, dtype=np.int32), np.ones(12, dtype=np.uint8)
    both(base)
    first = base["span_off"][:-1]

    def variant(**changes):
        kw = {k: (None if v is None else v.copy()) for k, v in base.items()}
        for k, f in changes.items():
            if f is None:
                kw[k] = None
            else:
                f(kw[k])
        return kw

    def set_rows(rows):
        def f(sp):
            for e, ab in rows.items():
                sp[e] = ab
        return f
    tl = base["tlen"]
    t5, t9 = int(base["target"][5]), int(base["target"][9])
    refused(gpu, variant(spans=set_rows({first[5] + 2: (30, 29)})), ("pair 5 ", "ends before"))
    refused(gpu, variant(spans=set_rows({first[5] + 2: (10, tl[t5])})), ("pair 5 ", "leaves its target"))
    refused(gpu, variant(spans=set_rows({first[9]: (0, 3)}), shift=lambda s: s.__setitem__(9, -1)), ("pair 9 ", "leaves"))
    refused(gpu, variant(shift=lambda s: s.__setitem__(9, int(tl[t9]))), ("pair 9 ", "leaves"))
    refused(gpu, variant(target=lambda t: t.__setitem__(7, 2)), ("pair 7 ", "target"))
    refused(gpu, variant(target=lambda t: t.__setitem__(7, 2), use=None), ("pair 7 ",))
    # two bad pairs: the lower index is named, whatever the kind of fault
    refused(gpu, variant(spans=set_rows({first[8] + 1: (5, 4), first[3] + 4: (0, 200)})), ("pair 3 ", "leaves"))
    refused(gpu, variant(spans=set_rows({first[8] + 1: (5, 4)}), target=lambda t: t.__setitem__(10, 9)), ("pair 8 ", "ends before"))
    # a masked pair, a pair without a target and a row without a path may hold anything
    ok = variant(spans=set_rows({first[2]: (9, 3), first[4]: (0, 10 ** 6), first[6] + 1: (-1, -7)}),
                 target=lambda t: t.__setitem__(2, -1))
    ok["use"][4] = 0
    both(ok)
    # span_off: a decrease, a wrong end, a wrong beginning
    def bump(i, d):
        return lambda so: so.__setitem__(i, so[i] + d)
    refused(gpu, variant(span_off=bump(4, 25)), ("span_off", "pair 4"))
    refused(gpu, variant(span_off=bump(12, 1)), ("span_off", "pair 11"))
    refused(gpu, variant(span_off=bump(12, -1)), ("span_off", "pair 11"))
    refused(gpu, variant(span_off=bump(0, 1)), ("span_off", "pair 0"))
    refused(gpu, variant(tlen=lambda t: t.__setitem__(1, -50), target=lambda t: t.__setitem__(slice(None), 0)), ("target 1", "negative"))
    total = int(pr.pileup_ref(**base)[1][-1])
    refused(gpu, base, ("ent_cap", str(total)), cap=total - 1)
    both(base)                                                      # a valid call after the refused ones


def test_nothing_to_do_is_ok(gpu):
    from squigglekit_amd import api
    for kw in (pc.case([0], np.zeros((0, 2)), [], tlen=[5, 0, 2]),                      # no pairs
               pc.case([0, 0, 0], np.zeros((0, 2)), [], target=[0, 2], tlen=[5, 0, 2]),  # pairs without rows
               pc.case([0, 2], [(-1, -1), (-1, -1)], [1.0, 2.0], tlen=[4]),              # rows without a path
               pc.case([0], np.zeros((0, 2)), [], tlen=[]),                              # no targets
               pc.case([0, 1], [(-1, -1)], [1.0], target=[-1], tlen=[])):
        pile, ent_off, ent_row = both(kw)
        assert (pile["n"] == 0).all() and np.isnan(pile["dwell_sd"]).all() and ent_row.size == 0 and not ent_off.any()
    assert api.last_pileup_plan()["entries"] == 0


def test_device_form_gives_the_host_forms_bytes(gpu):
    """sk_pileup_dev on uploaded arrays; use, dwell, target and shift also as NULL"""
    from squigglekit_amd import api
    L = gpu.load()
    rng = np.random.default_rng(18)
    for full in (True, False):
        kw = pc.paths_case(rng, 300, (5, 60), [500, 0, 90] if full else [500])
        if full:
            kw["shift"] = rng.integers(0, 3, size=300).astype(np.int32)
            kw["use"] = (rng.random(300) > 0.1).astype(np.uint8)
            kw["spans"][:, 1] = np.minimum(kw["spans"][:, 1], kw["tlen"][kw["target"]].repeat(np.diff(kw["span_off"])) - 3)
            kw["spans"][kw["spans"][:, 1] < kw["spans"][:, 0]] = -1
        else:
            kw["dwell"] = kw["target"] = None
        pile, ent_off, ent_row = both(kw)
        dev = {}
        try:
            for k in ("span_off", "spans", "value", "dwell", "target", "shift", "use"):
                if kw[k] is not None:
                    a = np.ascontiguousarray(kw[k])
                    dev[k] = L.sk_dev_alloc(max(a.nbytes, 8))
                    gpu.check(L.sk_dev_upload(dev[k], gpu.ptr(a), a.nbytes))
            for k, nbytes in (("out", pile.nbytes), ("ent_off", ent_off.nbytes), ("ent_row", max(ent_row.nbytes, 8))):
                dev[k] = L.sk_dev_alloc(nbytes)
            gpu.check(L.sk_pileup_dev(dev["span_off"], dev["spans"], dev["value"], dev.get("dwell"), dev.get("target"),
                                      dev.get("shift"), dev.get("use"), 300, len(kw["spans"]), gpu.ptr(kw["tlen"]),
                                      kw["tlen"].size, dev["out"], dev["ent_off"], dev["ent_row"], ent_row.size))
            gpu.check(L.sk_sync())
            got = [np.zeros_like(pile), np.zeros_like(ent_off), np.zeros_like(ent_row)]
            for a, k in zip(got, ("out", "ent_off", "ent_row")):
                if a.nbytes:
                    gpu.check(L.sk_dev_download(gpu.ptr(a), dev[k], a.nbytes))
            assert got[0].tobytes() == pile.tobytes() and np.array_equal(got[1], ent_off) and np.array_equal(got[2], ent_row)
            a, b, c, d = (C.c_int64() for _ in range(4))
            gpu.check(L.sk_last_pileup_plan(C.byref(a), C.byref(b), None, C.byref(d)))
            assert a.value == ent_row.size and b.value == int(np.diff(ent_off).max()) and d.value > 0
            # the records alone: no index is asked for
            gpu.check(L.sk_pileup_dev(dev["span_off"], dev["spans"], dev["value"], dev.get("dwell"), dev.get("target"),
                                      dev.get("shift"), dev.get("use"), 300, len(kw["spans"]), gpu.ptr(kw["tlen"]),
                                      kw["tlen"].size, dev["out"], None, None, 0))
            gpu.check(L.sk_sync())
            gpu.check(L.sk_dev_download(gpu.ptr(got[0]), dev["out"], pile.nbytes))
            assert got[0].tobytes() == pile.tobytes()
        finally:
            for d_ptr in dev.values():
                L.sk_dev_free(d_ptr)


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def event_reads(gpu):
    """a few hundred synthetic reads cut into events: (z-scored levels per read, dwells per read), shared and left unchanged"""
    from squigglekit_amd import api, synth
    sig = synth.squiggle_batch(240, 3000, 77)
    off, rec = api.detect_events([sig[r, :2000 + 4 * r] for r in range(240)])
    values, _ = api.event_levels(off, rec)
    zs, dw = [], []
    for r in range(240):
        v = values[off[r]:off[r + 1]][:1024]
        if v.size >= 8 and v.std() > 0:
            zs.append((v - v.mean()) / v.std())
            dw.append(rec["length"][off[r]:off[r + 1]][:1024].astype(np.int32))
    assert len(zs) >= 200
    return zs, dw


def test_end_to_end_subsequence_paths(gpu, event_reads):
    """detect_events -> event_levels -> z-score -> map_queries against two targets and their reversals -> map_paths ->
    pileup_of_map, against the reference on the same spans"""
    from squigglekit_amd import api
    zs, dw = event_reads
    rng = np.random.default_rng(19)
    fwd = [np.concatenate([zs[3][:150], rng.normal(size=500), zs[40][20:220]]), rng.normal(size=900)]
    targets = fwd + [t[::-1].copy() for t in fwd]
    rec, best = api.map_queries(zs, targets)
    which = best.copy()
    which[[1, 17]] = -1                                             # two queries without a path
    span_off, spans = api.map_paths(zs, targets, rec, which)
    assert api.last_path_mismatches() == 0
    pile = api.pileup_of_map(zs, dw, targets, rec, span_off, spans, which)
    has = np.diff(span_off) > 0
    want = pr.pileup_ref(span_off, spans, np.concatenate([z for z, h in zip(zs, has) if h]),
                         np.concatenate([d for d, h in zip(dw, has) if h]), target=np.where(has, which, -1),
                         tlen=[len(t) for t in targets])[0]
    assert pile.tobytes() == want.tobytes()
    assert int(pile["depth"].max()) >= 2 and int(pile["n"].sum()) == api.last_pileup_plan()["entries"]
    assert api.pileup_of_map(zs, None, targets, rec, span_off, spans, which)["level"].tobytes() == want["level"].tobytes()
    # one DBA step: covered points move to the pile's level, the others stay
    new = api.refine_targets(targets, pile, min_depth=2)
    for t, part, y in zip(targets, api.pile_split(pile, [len(t) for t in targets]), new):
        deep = part["depth"] >= 2
        assert np.array_equal(y[deep], part["level"][deep]) and np.array_equal(y[~deep], t[~deep])


def test_end_to_end_banded_paths(gpu, event_reads):
    """align_reads on sub-targets: the spans are relative to target[start : start + span], the pile-up takes shift = start"""
    from squigglekit_amd import api
    zs, dw = event_reads
    zs, dw = zs[:60], dw[:60]
    rng = np.random.default_rng(20)
    refs = [rng.normal(size=5000), rng.normal(size=3000)]
    tgt = rng.integers(0, 2, size=60).astype(np.int32)
    start = np.array([int(rng.integers(1, len(refs[t]) - 2 * len(z))) for t, z in zip(tgt, zs)], dtype=np.int32)
    subs = [refs[t][s:s + int(1.5 * len(z))] for t, s, z in zip(tgt, start, zs)]
    rec, span_off, spans = api.align_reads(zs, subs, band=128, end="free")
    assert (spans[:, 0] >= 0).any()
    kw = dict(span_off=span_off, spans=spans, value=np.concatenate(zs), dwell=np.concatenate(dw), target=tgt, shift=start,
              tlen=[len(r) for r in refs])
    pile, _, _ = both(kw)
    assert int(pile["n"].sum()) > 0 and (pile["n"][:1] == 0).all()      # point 0 lies before every start
