"""GPU: the segmenter parameter sweep (api.segment_sweep, sk_segment_sweep_*) against the existing single-set routes --
every set's records equal what segment_batch / segment_reads_f64 report for that set alone, the summaries equal the
counts recomputed from the records, a sample against the oracle -- plus the forced redo, a real read, scale, the
multi-GPU dry run and the command line against segmenter_cli."""
import contextlib
import io
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu


def _expected_rec(segs, n):
    """The sweep record of one read from a segment_batch result row."""
    return (int(n), int(segs[0][0]) if n else -1, int(segs[0][1]) if n else -1,
            int(segs[1][0]) if n > 1 else -1, int(segs[1][1]) if n > 1 else -1, 0)


def _sums_from_recs(sets, recs):
    from squigglekit_amd import _lib
    out = np.zeros(len(sets), dtype=_lib.SWEEP_SUM_DTYPE)
    for k, s in enumerate(sets):
        r = recs[k]
        n = r["nsegs"].astype(np.int64)
        anyseg = n >= 1
        stall = anyseg & (r["s0_start"] <= s.stall_start)
        gap = anyseg & ((n == 1) | (r["s1_start"].astype(np.int64) <= r["s0_end"].astype(np.int64) + s.gap_dist))
        out[k] = (len(n), anyseg.sum(), n.sum(), stall.sum(), gap.sum(), (stall & gap).sum(),
                  r["s0_end"][anyseg].astype(np.int64).sum(), 0)
    return out


def _check_against_batch(sig, lens, sets, sums, recs):
    from squigglekit_amd import api
    for k, s in enumerate(sets):
        segs, nsegs = api.segment_batch(sig, lens, s.seg)
        want = [_expected_rec(segs[r], nsegs[r]) for r in range(sig.shape[0])]
        got = [tuple(int(x) for x in v) for v in recs[k].tolist()]
        assert got == want, (k, api.sweep_values(s))
    assert np.array_equal(sums, _sums_from_recs(sets, recs))


def _edge_batch():
    from squigglekit_amd import api, synth
    base = synth.squiggle_batch(64, 4000, 4242)
    rng = np.random.default_rng(11)
    reads = [r for r in base]
    for n in (0, 1, 63, 64, 65, 4000, 4001, 20000, 70000):
        x = rng.integers(300, 700, size=n).astype(np.int16)
        if n >= 1000:                          # a stall and a step in there, so segments appear
            x[200:700] = rng.integers(560, 580, size=500)
            x[n // 2:n // 2 + 900] = rng.integers(420, 430, size=900)
        reads.append(x)
    return api.pack_i16(reads)


def _corner_grid():
    from squigglekit_amd import api
    sets = []
    # a group of 64+ sets: the defaults' limits and std_scale, both walk kinds
    sets += api.sweep_grid(error=[0, 5, 60], corrector=[0, 50], window=[0, 1, 126, 150], seg_dist=[0, 50, 10 ** 9],
                           stall_len=[0, 0.25])[:72]
    # groups of 7 and of 1
    sets += api.sweep_grid(std_scale=3.0, window=[1, 50, 100, 150, 200, 300, 400])
    sets += api.sweep_grid(std_scale=0.0, stall_len=5.0)
    # three (lim_low, lim_hi) pairs
    sets += api.sweep_grid(lim_low=[0, 200], lim_hi=[900, 2500], stall_start=[50, 300], gap_dist=[10, 3000])
    sets += api.sweep_grid(lim_low=-40000, lim_hi=40000, window=[100, 150])      # too wide for int16: float64 route
    return sets


def test_sweep_equals_segment_batch_per_set(gpu, ora):
    from squigglekit_amd import _lib, api
    sig, lens = _edge_batch()
    sets = _corner_grid()
    assert len(sets) >= 96
    sums, recs = api.segment_sweep(sig, sets, lens, records=True)
    assert recs.shape == (len(sets), sig.shape[0])
    _check_against_batch(sig, lens, sets, sums, recs)
    sums2, none = api.segment_sweep(sig, sets, lens)
    assert none is None and np.array_equal(sums, sums2)
    # a sample of (set, read) pairs against the oracle
    rng = np.random.default_rng(5)
    for k in rng.choice(len(sets), 12, replace=False):
        s = sets[int(k)]
        g = s.seg
        op = ora.SegParams(g.error, g.corrector, g.window, g.seg_dist, g.std_scale, g.stall_len)
        for r in rng.choice(sig.shape[0], 6, replace=False):
            segs = ora.get_segs(ora.scale_outliers(sig[r, :lens[r]].astype(float), g.lim_low, g.lim_hi), op) or []
            assert tuple(int(x) for x in recs[int(k), int(r)].tolist()) == _expected_rec(segs, len(segs)), (k, r)
    assert _lib.SWEEP_SUM_DTYPE.itemsize == 64


def test_negative_error_with_corrector_zero_takes_the_general_walk(gpu, ora):
    """Found by tests/test_gpu_random.py (sweep seeds 16 and 60): error = -1 < corrector = 0 passed the run-hopping
    walks' test, but there the first run of a read has c == w, the corrector test of segmenter.py:439 fires at every
    sample past `window`, err falls below `error` and out-of-band samples are tolerated from then on -- the reference
    reports other segments (often none, the run reaching the end of the read) than a walk without the corrector.
    Both planners (sk_sweep_plan, walk_params) now ask for corrector >= 1; the sweep and segment_batch against the oracle."""
    from squigglekit_amd import api, synth
    sig = synth.squiggle_batch(64, 4000, 16)
    lens = np.full(64, 4000, dtype=np.int32)
    lens[::7] = 1000
    sets = api.sweep_grid(error=[-1, -3], corrector=0, window=[20, 127], stall_len=[0.05, 1.2], lim_low=300, lim_hi=800,
                          std_scale=[1.5, 3.0])
    sums, recs = api.segment_sweep(sig, sets, lens, records=True)
    differs = 0
    for k, s in enumerate(sets):
        g = s.seg
        op = ora.SegParams(g.error, g.corrector, g.window, g.seg_dist, g.std_scale, g.stall_len)
        plain = ora.SegParams(g.error, 50, g.window, g.seg_dist, g.std_scale, g.stall_len)      # the corrector test dead
        segs, nsegs = api.segment_batch(sig, lens, g)
        for r in range(sig.shape[0]):
            f = ora.scale_outliers(sig[r, :lens[r]].astype(float), g.lim_low, g.lim_hi)
            want = ora.get_segs(f, op, max_segs=f.size) or []
            assert tuple(int(x) for x in recs[k, r].tolist()) == _expected_rec(want, len(want)), (k, r)
            assert segs[r, :nsegs[r]].tolist() == want, (k, r)
            differs += want != (ora.get_segs(f, plain, max_segs=f.size) or [])
    assert differs > 0                                       # the inputs are ones where the corrector test matters
    assert np.array_equal(sums, _sums_from_recs(sets, recs))


def test_sweep_small_group_packs_reads(gpu):
    """8 sets in one group (several reads per wavefront) and 3 sets (lanes left idle) give the per-set results."""
    from squigglekit_amd import api, synth
    sig = synth.squiggle_batch(1001, 4000, 777)
    lens = np.full(sig.shape[0], 3999, dtype=np.int32)
    for sets in (api.sweep_grid(window=[100, 150], seg_dist=[0, 50], error=[3, 5]), api.sweep_grid(window=[90, 150, 300])):
        sums, recs = api.segment_sweep(sig, sets, lens, records=True)
        _check_against_batch(sig, lens, sets, sums, recs)


def test_sweep_f64_route(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(3)
    reads = []
    for n in (0, 5, 64, 1000, 4096, 9000, 36977, 50000):
        x = np.round(rng.normal(90.0, 15.0, size=n), 2)
        if n >= 1000:
            x[100:600] = np.round(rng.normal(120.0, 1.0, size=500), 2)
        reads.append(x)
    sets = api.sweep_grid(window=[50, 150], error=[5, 60], std_scale=[0.75, 1.5], lim_low=[0, 40], lim_hi=[200])
    sums, recs = api.segment_sweep(reads, sets, records=True)
    for k, s in enumerate(sets):
        for r, res in enumerate(api.segment_reads_f64(reads, s.seg)):
            segs = res or []
            assert tuple(int(x) for x in recs[k, r].tolist()) == _expected_rec(segs, len(segs)), (k, r)
    assert np.array_equal(sums, _sums_from_recs(sets, recs))


def test_sweep_forced_redo(gpu, monkeypatch):
    """Every read through the numpy-order redo: the results do not move."""
    from squigglekit_amd import api, synth
    sig = synth.squiggle_batch(300, 4000, 99)
    lens = np.full(300, 4000, dtype=np.int32)
    sets = api.sweep_grid(std_scale=[0.5, 0.75], window=[100, 150], error=[5, 70])
    base_sums, base_recs = api.segment_sweep(sig, sets, lens, records=True)
    monkeypatch.setenv("SK_SEG_DELTA_SCALE", "1e13")
    sums, recs = api.segment_sweep(sig, sets, lens, records=True)
    assert np.array_equal(sums, base_sums) and np.array_equal(recs, base_recs)
    _check_against_batch(sig, lens, sets, sums, recs)


def test_sweep_real_read(gpu, example_read):
    from squigglekit_amd import api
    from squigglekit_amd.blow5 import to_pA
    raw = example_read["signal"][:-1]                  # segmenter.py's default cut, sig[:-1]: 36 977 samples
    assert raw.size == 36977
    pa = to_pA(raw, example_read["digitisation"], example_read["offset"], example_read["range"])
    sets = api.sweep_grid(error=[3, 5], window=[100, 150], std_scale=[0.75, 1.0])
    for read in (raw, pa):
        sums, recs = api.segment_sweep([read], sets, records=True)
        for k, s in enumerate(sets):
            segs = api.segment_any([read], s.seg)[0] or []
            assert tuple(int(x) for x in recs[k, 0].tolist()) == _expected_rec(segs, len(segs)), k


def test_sweep_scale_and_dev_entry(gpu):
    """200 000 x 4 000 reads x 64 sets: the summaries equal the per-set loop; the device entry point agrees."""
    import ctypes
    from squigglekit_amd import _lib, api, synth
    R, M = 200000, 4000
    sig = synth.squiggle_batch(R, M, 2024)
    lens = np.full(R, M, dtype=np.int32)
    sets = api.sweep_grid(std_scale=[0.5, 0.625, 0.75, 0.875, 1.0, 1.125, 1.25, 1.5], window=[100, 150],
                          seg_dist=[0, 50], error=[3, 5])
    assert len(sets) == 64
    sums, recs = api.segment_sweep(sig, sets, lens, records=True)
    assert np.array_equal(sums, _sums_from_recs(sets, recs))
    sums_only, _ = api.segment_sweep(sig, sets, lens)
    assert np.array_equal(sums_only, sums)
    for k, s in enumerate(sets):
        segs, nsegs = api.segment_batch(sig, lens, s.seg)
        n = nsegs.astype(np.int64)
        assert int(n.sum()) == int(sums[k]["segs"]) and int((n > 0).sum()) == int(sums[k]["with_segs"]), k
        assert np.array_equal(recs[k]["nsegs"], nsegs), k
        assert np.array_equal(recs[k]["s0_end"][n > 0], segs[n > 0, 0, 1]), k
    # the device-resident entry over the same rows
    L = _lib.load()
    nb = sig.nbytes
    d_sig, d_len = L.sk_dev_alloc(nb), L.sk_dev_alloc(lens.nbytes)
    d_sums = L.sk_dev_alloc(64 * len(sets))
    try:
        _lib.check(L.sk_dev_upload(d_sig, _lib.ptr(sig), nb))
        _lib.check(L.sk_dev_upload(d_len, _lib.ptr(lens), lens.nbytes))
        arr = (_lib.SweepSet * len(sets))(*sets)
        _lib.check(L.sk_segment_sweep_dev_i16(d_sig, M, d_len, R, arr, len(sets), d_sums, None))
        got = np.zeros(len(sets), dtype=_lib.SWEEP_SUM_DTYPE)
        _lib.check(L.sk_dev_download(_lib.ptr(got), d_sums, got.nbytes))
        assert np.array_equal(got, sums)
    finally:
        for p in (d_sig, d_len, d_sums):
            L.sk_dev_free(ctypes.c_void_p(p))


def test_sweep_two_ranks_on_one_device(gpu, monkeypatch):
    from squigglekit_amd import api, synth
    monkeypatch.setenv("SK_OVERSUBSCRIBE", "1")
    sig = synth.squiggle_batch(501, 3000, 13579)
    lens = np.full(501, 2999, dtype=np.int32)
    sets = api.sweep_grid(window=[100, 150], error=[5, 60])
    one = api.segment_sweep(sig, sets, lens, records=True)
    two = api.segment_sweep(sig, sets, lens, records=True, devices=[0, 0])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


def _run(main, argv):
    so, se = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
        try:
            main(argv)
        except SystemExit:
            pass
    return so.getvalue()


def test_sweep_cli_end_to_end(gpu):
    """segmenter_sweep.py on a BLOW5 fixture: each set's columns equal the line counts segmenter_cli prints with that
    set's flags (plain, -k -u, -k -g -u)."""
    from squigglekit_amd import segmenter_cli, sweep_cli
    f = os.path.join(GOLD, "example_0.blow5")
    out = _run(sweep_cli.main, ["--blow5", f, "--raw_signal", "-w", "100,150", "-e", "5", "-j", "100", "-b", "100",
                                "-t", "0.75"])
    out += "".join(_run(sweep_cli.main, ["--blow5", f, "-w", "150", "-j", "100", "-b", "100"]).splitlines(True)[1:])
    lines = out.strip().split("\n")
    head = lines[0].split("\t")
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]
    assert len(rows) == 3
    for i, row in enumerate(rows):
        flags = ["--blow5", f, "-w", row["window"], "-e", row["error"], "-j", "100", "-b", "100"]
        if i < 2:
            flags.append("--raw_signal")
        for cols, extra in (("with_segs", []), ("stall_ok", ["-k", "-u"]), ("stall_gap_ok", ["-k", "-g", "-u"])):
            printed = _run(segmenter_cli.main, flags + extra)
            assert int(row[cols]) == len(printed.splitlines()), (row, cols)
