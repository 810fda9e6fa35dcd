"""GPU: segment levels (sk_seglev.hip) against plain numpy on the segments the oracle finds.

Every record of every read is compared, field by field and by bit pattern (the doubles as uint64, NaN slots included).
Expected values: with a the read after the [:Num] cut in its own dtype (int64 for integer input, float64 for pA),
kept = np.flatnonzero((a > lo) & (a < hi)), y = a[kept] and [s, e] a segment the oracle reports on y:
w = y[s:e] -> np.mean, np.std, np.median, np.median(np.abs(w - median)), min, max, kept[s], kept[e - 1] + 1, e - s.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOUBLES = ("mean", "std", "median", "mad", "min", "max")
INTS = ("raw_start", "raw_end", "n", "pad")
LENGTH_CLASSES = (1, 2, 7, 8, 9, 127, 128, 129, 1000)


def expected_record(api, w, kept, s):
    rec = api.no_levels(1)[0]
    if len(w) == 0:
        return rec
    med = np.median(w)
    rec["mean"], rec["std"], rec["median"] = np.mean(w), np.std(w), med
    rec["mad"] = np.median(np.abs(w - med))
    rec["min"], rec["max"] = float(w.min()), float(w.max())
    rec["raw_start"], rec["raw_end"], rec["n"] = kept[s], kept[s + len(w) - 1] + 1, len(w)
    return rec


def expected_levels(api, reads, seg_lists, lo, hi, max_segs):
    """reads: arrays in the dtype numpy is to work in; seg_lists: per read the oracle's [[s, e], ..] (or False)"""
    R = len(reads)
    levels = api.no_levels((R, max_segs))
    read_level = api.no_levels(R)
    for r, a in enumerate(reads):
        kept = np.flatnonzero((a > lo) & (a < hi))
        y = a[kept]
        read_level[r] = expected_record(api, y, kept, 0)
        for k, (s, e) in enumerate(seg_lists[r] or []):
            levels[r, k] = expected_record(api, y[s:e], kept, s)
    return levels, read_level


def assert_same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in DOUBLES:
        g = np.ascontiguousarray(got[f]).view(np.uint64)
        w = np.ascontiguousarray(want[f]).view(np.uint64)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (
            what, f, bad[0].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    for f in INTS:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (
            what, f, bad[0].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def seg_lists_of(segs, nsegs):
    return [segs[r, :nsegs[r]].tolist() for r in range(len(nsegs))]


def opar(ora, p):
    """the oracle's own parameter structure (it takes the limits apart)"""
    return ora.SegParams(p.error, p.corrector, p.window, p.seg_dist, p.std_scale, p.stall_len)


def plateau(n, phase=0):
    """n in-band samples, 498 .. 502 with many ties"""
    return (500 + ((np.arange(n) + phase) * 7) % 5 - 2).astype(np.int16)


def noise(n, phase=0):
    """n out-of-band samples, alternating around the plateaus"""
    return np.where((np.arange(n) + phase) % 2 == 0, 200, 800).astype(np.int16)


def hand_reads():
    """Alternations around plateaus (as the KAT table's reads).  Read 0 holds every length class; 0 and 1 000 are
    dropped by scale_outliers' limits (0, 900)."""
    z, k = np.array([0], dtype=np.int16), np.array([1000], dtype=np.int16)
    big = [z, k, noise(11)]                                    # dropped samples at the first sample of the read
    for i, n in enumerate(LENGTH_CLASSES):
        big += [plateau(n, i), noise(5 + i, i)]
    big += [z, z, k, noise(6)]                                 # dropped before a segment ...
    big += [plateau(40), k, z, plateau(33, 2), z, plateau(7, 1)]   # ... and inside it (one segment of 80 for the walk)
    big += [k, noise(9)]                                       # right after a segment's last sample
    big += [plateau(9000, 3), noise(8)]                        # above 8 192: numpy's second reduction buffer
    big += [plateau(4097, 1), z, noise(4), plateau(4096), noise(3)]   # both sides of the staging threshold
    reads = [np.concatenate(big)]
    reads.append(noise(700))                                   # no segment (nothing lies in the band)
    reads.append(np.tile(np.array([0, 1000, 1000, 0], dtype=np.int16), 50))    # no surviving sample
    reads.append(np.full(300, 500, dtype=np.int16))            # constant: std 0, empty band
    many = []
    for i in range(90):                                        # 90 segments: more than max_segs
        many += [plateau(2 + i % 5, i), noise(3 + i % 2, i)]
    reads.append(np.concatenate(many + [plateau(400)]))
    reads.append(np.concatenate([plateau(64), z, plateau(64), noise(2), plateau(63), k, noise(3)]))   # entry boundaries
    reads.append(np.concatenate([noise(4), plateau(5)]))       # the read ends inside a run
    reads.append(np.zeros(0, dtype=np.int16))                  # empty read
    return reads


def hand_params(_lib):
    return _lib.SegParams(error=0, corrector=50, window=1, seg_dist=0, std_scale=0.3, stall_len=1.0, lim_low=0, lim_hi=900)


@pytest.fixture(scope="module")
def hand(gpu, ora):
    """the hand-built batch, the oracle's segments on it and numpy's records -- computed once"""
    from squigglekit_amd import api
    reads = hand_reads()
    buf, lens = api.pack_i16(reads)
    p = hand_params(gpu)
    osegs, onsegs = ora.segment_batch_i16(buf, lens, opar(ora, p), lo=0, hi=900, max_segs=128)
    lists = seg_lists_of(osegs, onsegs)
    want = expected_levels(api, [r.astype(np.int64) for r in reads], lists, 0, 900, 128)
    return {"reads": reads, "buf": buf, "lens": lens, "p": p, "lists": lists, "want": want, "nsegs": onsegs}


def test_hand_built_reads_every_length_class(gpu, hand):
    from squigglekit_amd import api
    # the oracle's output must hold what this test is about, before the GPU is looked at
    lengths = {e - s for s, e in hand["lists"][0]}
    for n in LENGTH_CLASSES + (9000, 4097, 4096, 80):
        assert n in lengths, "no segment of length %d in the oracle's output: %s" % (n, sorted(lengths))
    assert max(lengths) > 8192 and hand["lens"][0] > 8192
    assert not hand["lists"][1] and not hand["lists"][2] and not hand["lists"][3]
    assert hand["nsegs"][4] > 64
    wl, wr = hand["want"]
    assert wr["n"][2] == 0 and wr["std"][3] == 0.0 and wr["n"][3] == 300
    segs_in = wl[wl["n"] > 0]
    assert np.any(segs_in["raw_end"] - segs_in["raw_start"] > segs_in["n"])      # a drop inside a segment
    assert wr["raw_start"][0] == 2                                                # drops at the first sample
    odd = segs_in[(segs_in["n"] % 2 == 1) & (segs_in["n"] > 2)]
    even = segs_in[(segs_in["n"] % 2 == 0) & (segs_in["n"] > 2)]
    assert len(odd) and len(even) and np.any(even["median"] == np.floor(even["median"]))   # tied middle values

    segs, nsegs, levels, read_level = api.segment_levels_batch(hand["buf"], hand["lens"], hand["p"], max_segs=8)
    assert segs.shape[1] >= 91                                                    # overflowed, grown, retried
    assert np.array_equal(nsegs, hand["nsegs"])
    assert seg_lists_of(segs, nsegs) == [x or [] for x in hand["lists"]]
    ms = segs.shape[1]
    assert_same_records(levels, wl[:, :ms], "levels")
    assert not np.any(wl[:, ms:]["n"])
    assert_same_records(read_level, wr, "read_level")
    # segs / nsegs are segment_batch's on the same input
    s2, n2 = api.segment_batch(hand["buf"], hand["lens"], hand["p"], max_segs=ms)
    assert np.array_equal(s2, segs) and np.array_equal(n2, nsegs)
    top, bot = api.thresholds_of(read_level, hand["p"])
    assert top[3] == 500.0 and bot[3] == 500.0


def test_overflow_status_and_null_outputs(gpu, hand):
    """the C ABI itself: SK_ERR_OVERFLOW with the true counts, truncated records like truncated segs; NULL is invalid"""
    from squigglekit_amd import api
    L = gpu.load()
    buf, lens, p = hand["buf"], hand["lens"], hand["p"]
    R, ms = buf.shape[0], 16
    segs = np.zeros((R, ms, 2), dtype=np.int32)
    nsegs = np.zeros(R, dtype=np.int32)
    lv, rl = api.no_levels((R, ms)), api.no_levels(R)
    rc = L.sk_segment_levels_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, C.byref(p), gpu.ptr(segs), gpu.ptr(nsegs), ms,
                                 gpu.ptr(lv), gpu.ptr(rl))
    assert rc == gpu.SK_ERR_OVERFLOW
    assert np.array_equal(nsegs, hand["nsegs"])
    assert_same_records(lv, hand["want"][0][:, :ms], "truncated levels")
    assert_same_records(rl, hand["want"][1], "read_level")
    for a, b in ((None, gpu.ptr(rl)), (gpu.ptr(lv), None)):
        assert L.sk_segment_levels_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, C.byref(p), gpu.ptr(segs),
                                       gpu.ptr(nsegs), ms, a, b) == gpu.SK_ERR_INVALID


def test_device_resident_form_and_two_shards(gpu, hand):
    from squigglekit_amd import api
    L = gpu.load()
    buf, lens, p = hand["buf"], hand["lens"], hand["p"]
    R, ms = buf.shape[0], 128
    host = api.segment_levels_batch(buf, lens, p, max_segs=ms)
    two = api.segment_levels_batch(buf, lens, p, max_segs=ms, devices=[0, 0])
    for a, b, what in zip(host, two, ("segs", "nsegs", "levels", "read_level")):
        if a.dtype == api.LEVEL_DTYPE:
            assert_same_records(b, a, "devices=[0, 0] " + what)
        else:
            assert np.array_equal(a, b), what
    gpu.init(0)
    sizes = (buf.nbytes, lens.nbytes, R * ms * 8, R * 4, R * ms * 64, R * 64)
    d = [L.sk_dev_alloc(n) for n in sizes]
    try:
        assert all(d)
        gpu.check(L.sk_dev_upload(d[0], gpu.ptr(buf), buf.nbytes))
        gpu.check(L.sk_dev_upload(d[1], gpu.ptr(lens), lens.nbytes))
        gpu.check(L.sk_segment_levels_dev_i16(d[0], buf.shape[1], d[1], R, C.byref(p), d[2], d[3], ms, d[4], d[5]))
        gpu.check(L.sk_sync())
        out = (np.zeros((R, ms, 2), np.int32), np.zeros(R, np.int32), api.no_levels((R, ms)), api.no_levels(R))
        for arr, dp in zip(out, d[2:]):
            gpu.check(L.sk_dev_download(gpu.ptr(arr), dp, arr.nbytes))
    finally:
        for x in d:
            if x:
                L.sk_dev_free(x)
    assert np.array_equal(out[0], host[0]) and np.array_equal(out[1], host[1])
    assert_same_records(out[2], host[2], "device-resident levels")
    assert_same_records(out[3], host[3], "device-resident read_level")
    assert_same_records(host[2], hand["want"][0], "levels")


def test_hand_built_reads_float64_and_mixed(gpu, ora, hand):
    """the same reads as float64 with a fractional part (the float64 body: selection on values of either sign is
    covered by the negative limits), and the mixed-input form"""
    from squigglekit_amd import api
    p = gpu.SegParams(error=0, corrector=50, window=1, seg_dist=0, std_scale=0.3, stall_len=1.0, lim_low=-600, lim_hi=400)
    reads = [r.astype(np.float64) * 0.5 - 500.25 for r in hand["reads"][:7]]      # 0 -> -500.25 kept; 1000 -> -0.25 kept
    reads = [np.where(r == -500.25, -700.0, np.where(r == -0.25, 450.0, r)) for r in reads]   # ... so: dropped again
    lists = [ora.get_segs(ora.scale_outliers(r, -600, 400), opar(ora, p)) for r in reads]
    assert {1, 2, 7, 8, 9, 127, 128, 129, 1000, 9000} <= {e - s for s, e in lists[0]}
    ms = max(len(x or []) for x in lists)
    wl, wr = expected_levels(api, reads, lists, -600, 400, ms)
    assert np.any(wl["median"] < 0)
    flat, off = api.pack_f64(reads)
    segs, nsegs, levels, read_level = api.segment_levels_ragged_f64(flat, off, None, p, max_segs=ms)
    assert seg_lists_of(segs, nsegs) == [x or [] for x in lists]
    assert_same_records(levels, wl, "float64 levels")
    assert_same_records(read_level, wr, "float64 read_level")
    # mixed input: integer reads through the int16 route, the rest through the float64 one, input order kept
    p0 = hand["p"]
    mixed = [hand["reads"][5], hand["reads"][5].astype(np.float64) + 0.5, hand["reads"][1], hand["reads"][6]]
    segs, nsegs, levels, read_level = api.segment_levels(mixed, p0)
    mlists = [ora.get_segs(ora.scale_outliers(np.asarray(m, dtype=np.float64), 0, 900), opar(ora, p0)) for m in mixed]
    assert seg_lists_of(segs, nsegs) == [x or [] for x in mlists]
    typed = [np.asarray(m).astype(np.int64) if np.asarray(m).dtype.kind == "i" else np.asarray(m) for m in mixed]
    wl, wr = expected_levels(api, typed, mlists, 0, 900, segs.shape[1])
    assert_same_records(levels, wl, "mixed levels")
    assert_same_records(read_level, wr, "mixed read_level")


def test_real_read_every_route(gpu, ora, example_read):
    """tests/golden/example_0.blow5: 36 978 samples, the long-row route -- raw, float64 pA, centi-units, the pA rows"""
    from squigglekit_amd import api
    from squigglekit_amd.blow5 import to_pA
    raw = example_read["signal"]
    assert raw.size > 8192
    p = gpu.SegParams()
    buf, lens = api.pack_i16([raw, raw[:-1], raw[:3000]])
    osegs, onsegs = ora.segment_batch_i16(buf, lens, opar(ora, p), lo=0, hi=900, max_segs=64)
    lists = seg_lists_of(osegs, onsegs)
    assert lists[0]
    segs, nsegs, levels, read_level = api.segment_levels_batch(buf, lens, p)
    assert seg_lists_of(segs, nsegs) == lists
    wl, wr = expected_levels(api, [buf[r, :lens[r]].astype(np.int64) for r in range(3)], lists, 0, 900, 64)
    assert_same_records(levels, wl, "raw levels")
    assert_same_records(read_level, wr, "raw read_level")
    top, bot = api.thresholds_of(read_level, p)
    for r in range(3):
        a = buf[r, :lens[r]]
        _, otop, obot = ora.get_segs(ora.scale_outliers(a, 0, 900), opar(ora, p), return_thresholds=True)
        assert np.float64(otop).view(np.uint64) == top[r].view(np.uint64)
        assert np.float64(obot).view(np.uint64) == bot[r].view(np.uint64)

    pa = to_pA(raw, example_read["digitisation"], example_read["offset"], example_read["range"])
    reads = [pa, pa[:20000]]
    plists = []
    for a in reads:
        sg, otop, obot = ora.get_segs(ora.scale_outliers(a, 0, 900), opar(ora, p), return_thresholds=True)
        plists.append((sg, otop, obot))
    wl, wr = expected_levels(api, reads, [x[0] for x in plists], 0, 900, 64)
    flat, off = api.pack_f64(reads)
    centi = np.rint(flat * 100.0).astype(np.int32)
    assert np.array_equal(centi / 100.0, flat)
    calib = np.array([[example_read["digitisation"], example_read["offset"], example_read["range"]]] * 2)
    rbuf, rlens = api.pack_i16([raw, raw[:20000]])
    assert all(np.array_equal(a, b) for a, b in zip(api.pa_values(rbuf, rlens, calib), reads))
    for what, res in (("float64", api.segment_levels_ragged_f64(flat, off, None, p)),
                      ("centi", api.segment_levels_ragged_f64(centi, off, None, p)),
                      ("pA rows", api.segment_levels_batch_pa(rbuf, rlens, calib, p)),
                      ("cut", api.segment_levels_ragged_f64(np.concatenate([pa, pa]), np.array([0, pa.size, 2 * pa.size]),
                                                            np.array([pa.size, 20000], dtype=np.int32), p))):
        segs, nsegs, levels, read_level = res
        assert seg_lists_of(segs, nsegs) == [x[0] or [] for x in plists], what
        assert_same_records(levels, wl, what + " levels")
        assert_same_records(read_level, wr, what + " read_level")
        top, bot = api.thresholds_of(read_level, p)
        for r in range(2):
            assert np.float64(plists[r][1]).view(np.uint64) == top[r].view(np.uint64), what
            assert np.float64(plists[r][2]).view(np.uint64) == bot[r].view(np.uint64), what


def test_wide_limits_take_the_float64_body(gpu, ora, hand):
    from squigglekit_amd import api
    p = gpu.SegParams(error=0, corrector=50, window=1, seg_dist=0, std_scale=0.3, stall_len=1.0, lim_low=-30000, lim_hi=30000)
    assert api._too_wide_for_i16(p.lim_low, p.lim_hi)
    reads = hand["reads"][4:7]
    buf, lens = api.pack_i16(reads)
    lists = [ora.get_segs(ora.scale_outliers(r.astype(np.float64), -30000, 30000), opar(ora, p)) for r in reads]
    ms = max(len(x or []) for x in lists)
    segs, nsegs, levels, read_level = api.segment_levels_batch(buf, lens, p, max_segs=ms)
    assert seg_lists_of(segs, nsegs) == [x or [] for x in lists]
    wl, wr = expected_levels(api, [r.astype(np.float64) for r in reads], lists, -30000, 30000, ms)
    assert_same_records(levels, wl, "wide-limit levels")
    assert_same_records(read_level, wr, "wide-limit read_level")
