"""CPU: MotifSeq sessions without a GPU -- the numpy statement against its own column-by-column resume (the state a
session keeps), argument validation through api.MotifStream and the C ABI, stream_decide, the CLI's flag checks and the
record layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import stream_ref as ref
from conftest import GOLD


def _resume_vs_statement(ora, x, y, cuts):
    """dtw_subsequence(x, y[:c]) for every cut c against the resume that was fed y in those pieces"""
    rs, at = ref.Resume(x), 0
    for c in cuts:
        rs.push(y[at:c])
        at = c
        if c == 0:
            assert ref.same(rs.record(), (ref.NAN, ref.NAN, -1, -1))
            continue
        dist, start, end, cost = ora.dtw_subsequence(x, y[:c], want_cost=True)
        assert ref.same(rs.record(), (float(dist), float(cost[-1, -1]), int(start), int(end))), (len(x), c, cuts)


def test_resume_equals_the_statement_on_random_cuts(ora):
    rng = np.random.default_rng(20260)
    for case in range(40):
        N = int(rng.integers(1, 40))
        n = int(rng.integers(1, 120))
        ties = case % 2 == 0                                       # integer-valued motif and samples: ties everywhere
        x = rng.integers(-3, 4, N).astype(np.float64) if ties else rng.normal(size=N)
        y = rng.integers(-3, 4, n).astype(np.float64) if ties else rng.normal(size=n)
        cuts = sorted(set(rng.integers(0, n + 1, int(rng.integers(1, 6))).tolist()) | {n})
        if case % 5 == 0:
            cuts = [0] + cuts                                      # a first chunk of length 0
        _resume_vs_statement(ora, x, y, cuts)


def test_resume_single_point_motif_and_every_cut_of_a_short_read(ora):
    rng = np.random.default_rng(7)
    y = rng.integers(-2, 3, 23).astype(np.float64)
    _resume_vs_statement(ora, np.array([1.0]), y, list(range(0, 24)))          # N = 1
    for N in (2, 5, 17):
        x = rng.integers(-2, 3, N).astype(np.float64)
        _resume_vs_statement(ora, x, y, list(range(0, 24)))                    # a cut at every position
        for c in range(1, 23):
            _resume_vs_statement(ora, x, y, [c, 23])


def test_statement_calibration_and_flags(ora):
    motif = np.array([0.0, 1.0, -1.0])
    raw = np.array([500, 3000, 510, 490, -5, 505, 520], dtype=np.int16)        # two samples outside (0, 1200)
    r = ref.record(raw[:3], motif, 3, "medmad", 0, 1200, False)
    assert ref.same(r, (ref.NAN, ref.NAN, -1, -1, 2, 3, ref.CALIBRATING))
    r = ref.record(raw[:4], motif, 3, "medmad", 0, 1200, False)                # calibration complete: 500, 510, 490
    assert r[4:] == (3, 4, 0) and r[0] == r[0]
    c, s, _ = ref.statistics(np.array([500, 510, 490]), "medmad")
    assert (c, s) == (500.0, 10.0 * 1.4826)
    full = ref.record(raw, motif, 3, "medmad", 0, 1200, False)                 # later samples do not move the statistics
    y = (ref.keep(raw, 0, 1200).astype(np.float64) - c) / s
    assert ref.same(full[:4], ref.Resume(motif).push(y).record())
    assert ref.record(raw[:3], motif, 3, "medmad", 0, 1200, True)[6] == 0      # a flush ends the calibration with n >= 1
    assert ref.record(raw[1:2], motif, 3, "medmad", 0, 1200, True)[4:] == (0, 1, ref.EMPTY)
    assert ref.record(np.full(9, 500, dtype=np.int16), motif, 3, "medmad", 0, 1200, False)[6] == ref.DEGENERATE
    assert ref.record(np.full(9, 500, dtype=np.int16), motif, 3, "zscale", 0, 1200, False)[6] == 0    # std 0 -> 1
    deg = ref.record(np.full(9, 500, dtype=np.int16), motif, 3, "medmad", 0, 1200, False)
    assert ref.same(deg, (ref.NAN, ref.NAN, -1, -1, 9, 9, ref.DEGENERATE))     # MAD 0 at W samples: NaN
    deg = ref.record(np.full(2, 500, dtype=np.int16), motif, 3, "medmad", 0, 1200, True)
    assert ref.same(deg, (float("inf"), ref.NAN, -1, -1, 2, 2, ref.DEGENERATE))    # MAD 0 at a flush: the one-shot +inf
    early = ref.record(raw, motif, 5, "medmad", 0, 1200, 3)                    # flushed after three raw samples: 500, 510
    c2, s2, _ = ref.statistics(np.array([500, 510]), "medmad")
    assert ref.same(early[:4], ref.Resume(motif).push((ref.keep(raw, 0, 1200).astype(np.float64) - c2) / s2).record())


def test_record_layouts_match_the_header():
    from squigglekit_amd import _lib
    assert C.sizeof(_lib.StreamRec) == 40 and _lib.STREAM_DTYPE.itemsize == 40
    assert C.sizeof(_lib.StreamParams) == 32
    for name, _ in _lib.StreamRec._fields_:
        assert _lib.STREAM_DTYPE.fields[name][1] == getattr(_lib.StreamRec, name).offset, name
    assert _lib.SK_FLAG_CALIBRATING == 8 == ref.CALIBRATING
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "squigglekit_hip.h")).read()
    assert "#define SK_STREAM_MAX_CALIB 65536" in hdr and "SK_FLAG_CALIBRATING = 8" in hdr
    for sym in ("sk_stream_open", "sk_stream_push_i16", "sk_stream_push_dev_i16", "sk_stream_flush", "sk_stream_reset",
                "sk_stream_close"):
        assert sym in _lib.ABI


def test_python_validation_needs_no_device():
    from squigglekit_amd import api
    motif = np.zeros(10)
    for kw in ({"calib": 0}, {"calib": 65537}, {"nslots": 0}, {"nslots": 65537}, {"scale": "minmax"}):
        args = {"nslots": 4}
        args.update(kw)
        with pytest.raises(ValueError):
            api.MotifStream([motif], **args)
    with pytest.raises(ValueError):
        api.MotifStream([np.zeros(1025)], 4)
    with pytest.raises(ValueError):
        api.MotifStream([], 4)
    with pytest.raises(ValueError):
        api.stream_slots([0, 3, 0], 4)                                         # a slot twice in one call
    with pytest.raises(ValueError):
        api.stream_slots([4], 4)
    assert api.stream_slots([3, 1], 4).dtype == np.int32


def test_abi_validation_and_no_cpu_fallback():
    """The C entry point checks its arguments before it looks at the device; with valid arguments and no GPU it fails
    loudly."""
    from squigglekit_amd import _lib, api
    L = _lib.load()
    h = C.c_int32(-1)

    def open_(npoints=10, **kw):
        m = np.zeros(npoints)
        off = np.array([0, npoints], dtype=np.int32)
        p = _lib.StreamParams(0, 0, 1200, 2000, 4)
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[1] = v
            else:
                setattr(p, k, v)
        rc = L.sk_stream_open(_lib.ptr(m), _lib.ptr(off), 1, C.byref(p), C.byref(h))
        return rc, L.sk_last_error().decode()

    for kw, word in (({"calib": 0}, "calib"), ({"calib": 65537}, "calib"), ({"nslots": 0}, "nslots"),
                     ({"nslots": 65537}, "nslots"), ({"reserved": 1}, "reserved"), ({"scale_mode": 2}, "scale mode")):
        rc, msg = open_(**kw)
        assert rc == _lib.SK_ERR_INVALID and word in msg, (kw, rc, msg)
    rc, msg = open_(npoints=1025)
    assert rc == _lib.SK_ERR_UNSUPPORTED and "1024" in msg
    if L.sk_device_count() > 0:
        return                                                                 # (the GPU suite opens sessions for real)
    rc, msg = open_()
    assert rc == _lib.SK_ERR_NO_DEVICE and ("no CPU fallback" in msg or "no HIP device" in msg)
    with pytest.raises(_lib.SquiggleKitError) as ei:
        api.MotifStream([np.zeros(10)], nslots=4)
    assert "no CPU fallback" in str(ei.value) or "no HIP device" in str(ei.value)
    assert L.sk_stream_close(0) == _lib.SK_ERR_NO_DEVICE


def test_stream_decide_truth_table():
    from squigglekit_amd import _lib, api
    rec = np.zeros((2, 5), dtype=_lib.STREAM_DTYPE)
    #            accept    wait     give up   NaN, few   NaN, many
    rec["dist"] = [[10.0, 30.0, 30.0, np.nan, np.nan], [50.0, 20.0, 100.0, np.nan, np.nan]]
    rec["n"] = [[100, 100, 5000, 10, 9000]] * 2
    got = api.stream_decide(rec, means=[20.0, 40.0], sds=[5.0, 10.0], accept_z=-1.0, give_up_after=4000)
    assert got.dtype == np.int8 and got.shape == (2, 5)
    # motif 0: Z = -2, 2, 2; motif 1: Z = 1, -2, 6
    assert got.tolist() == [[1, 0, -1, 0, 0], [0, 1, -1, 0, 0]]
    edge = np.zeros((1, 2), dtype=_lib.STREAM_DTYPE)
    edge["dist"], edge["n"] = [[15.0, 15.0 + 1e-9]], [[4000, 4000]]           # Z == accept_z accepts; n == give_up_after gives up
    assert api.stream_decide(edge, [20.0], [5.0], -1.0, 4000).tolist() == [[1, -1]]


def test_cli_refuses_what_a_session_cannot_take(tmp_path, capsys):
    from squigglekit_amd import stream_cli
    fa = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.fa")
    pa = tmp_path / "pa.tsv"
    pa.write_text("f.fast5\tread1\t" + "\t".join(["."] * 6) + "\t" + "\t".join("%.2f" % (80 + 0.25 * i) for i in range(50)) + "\n")
    with pytest.raises(SystemExit) as ei:
        stream_cli.main(["-s", str(pa), "-i", fa])
    assert ei.value.code not in (0, None)
    assert "raw" in capsys.readouterr().err                                    # float pA values: says what it takes instead
    raw = tmp_path / "raw.tsv"
    raw.write_text("f.fast5\tread1\t" + "\t".join(["."] * 6) + "\t" + "\t".join(str(400 + i % 90) for i in range(50)) + "\n")
    for bad in (["--chunk", "0"], ["--channels", "0"], ["--calib", "0"], ["--calib", "65537"]):
        with pytest.raises(SystemExit) as ei:
            stream_cli.main(["-s", str(raw), "-i", fa] + bad)
        assert ei.value.code not in (0, None), bad
        assert bad[0] in capsys.readouterr().err
