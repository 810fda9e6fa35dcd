"""GPU: event detection (sk_detect.hip) against the numpy statement of its definition (tests/detect_ref.py).

Every read's off and every field of every record is compared exactly; all four fields are integers, so there is no
tolerance anywhere.  The kernel's seams: k_detect_mark loads tiles of TILE = 128 samples per read and runs 64 positions
behind them, a mark word holds 64 samples, k_detect_fill takes FILL = 4 096 samples a round, 64 reads share a wavefront.
"""
import ctypes as C

import numpy as np
import pytest

import detect_ref

pytestmark = pytest.mark.gpu

TILE, FILL = 128, 4096
DNA, RNA = detect_ref.PRESETS["dna"], detect_ref.PRESETS["rna"]
ODD = (1, 1, 1.4, 9.0, 0.0)
WIDE = (32, 64, 1.4, 9.0, 0.2)
RAGGED_LENGTHS = (0, 1, 2, 5, 6, 11, 12, 13, 63, 64, 65, 127, 128, 129, 1000, 4000)


def squiggle(rng, n):
    """levels N(500, 80), dwell 1 + Poisson(8), noise N(0, 8), as int16"""
    out = np.zeros(0)
    while out.size < n:
        out = np.concatenate([out, np.full(1 + rng.poisson(8), rng.normal(500, 80))])
    return np.rint(out[:n] + rng.normal(0, 8, n)).astype(np.int16)


def steps(n, at, lo=400, hi=520):
    """a noiseless read of n samples that steps between lo and hi at every position of `at`"""
    x = np.full(n, lo, dtype=np.int16)
    for k, p in enumerate(sorted(at)):
        x[p:] = hi if k % 2 == 0 else lo
    return x


def par(api, p):
    return api.det_params(w_short=p[0], w_long=p[1], th_short=p[2], th_long=p[3], peak_height=p[4])


def rows(reads, stride=None):
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    stride = stride or max(8, (int(lens.max()) + 7) // 8 * 8)
    buf = np.full((len(reads), stride), -12345, dtype=np.int16)          # (nothing past a read's end may matter)
    for i, r in enumerate(reads):
        buf[i, :len(r)] = r
    return buf, lens


def assert_same(got, want, what):
    goff, grec = got
    woff, wrec = want
    assert np.array_equal(goff, woff), "%s: off differs at read %s" % (what, np.flatnonzero(goff != woff)[:4] - 1)
    assert grec.shape == wrec.shape, what
    for f in ("start", "length", "sum", "sumsq"):
        bad = np.flatnonzero(grec[f] != wrec[f])
        assert bad.size == 0, "%s: %s differs at record %d: got %r, want %r" % (what, f, bad[0], grec[bad[0]], wrec[bad[0]])


def check(api, reads, p, what, stride=None):
    buf, lens = rows(reads, stride)
    assert_same(api.detect_events_batch(buf, lens, par(api, p)), detect_ref.detect(reads, p), what)


@pytest.fixture(scope="module")
def pool():
    """130 noisy reads whose lengths differ widely inside every group of 64 (lanes finish at different tiles)"""
    rng = np.random.default_rng(20261018)
    lengths = rng.choice([0, 3, 40, 100, 130, 260, 300, 520, 700, 900], size=130)
    lengths[[0, 63, 64, 129]] = (900, 1, 700, 520)
    reads = [squiggle(rng, int(n)) for n in lengths]
    return reads, {name: detect_ref.detect(reads, p) for name, p in (("dna", DNA), ("rna", RNA), ("odd", ODD))}


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(7)
    return [squiggle(rng, n) for n in RAGGED_LENGTHS]


@pytest.mark.parametrize("name, p", [("dna", DNA), ("rna", RNA), ("odd", ODD)])
def test_ragged_lengths(gpu, ragged, name, p):
    from squigglekit_amd import api
    check(api, ragged, p, "ragged " + name)
    check(api, ragged, p, "ragged, stride 4003 " + name, stride=4003)     # rows that are not 16-byte aligned


@pytest.mark.parametrize("name, p", [("dna", DNA), ("rna", RNA), ("odd", ODD)])
def test_read_counts(gpu, pool, name, p):
    from squigglekit_amd import api
    reads, want = pool
    woff, wrec = want[name]
    for R in (1, 63, 64, 65, 130):
        buf, lens = rows(reads[:R], stride=904)
        assert_same(api.detect_events_batch(buf, lens, par(api, p)), (woff[:R + 1], wrec[:woff[R]]), "%d reads %s" % (R, name))


def test_steps_at_the_seams(gpu):
    from squigglekit_amd import api
    reads = []
    for T in (64, TILE, 2 * TILE, TILE - 64, 2 * TILE - 64):
        for p in (T - 1, T, T + 1):
            reads.append(steps(3 * TILE + 17, [p]))
            reads.append(steps(3 * TILE + 17, [p, p + 9, p + 64, p + 65]))
    n = 3 * TILE
    for p in list(range(1, 15)) + list(range(n - 14, n)):                 # within w_long of either end (both presets)
        reads.append(steps(n, [p]))
    reads.append(steps(n, list(range(10, n - 10, 10))))
    for name, p in (("dna", DNA), ("rna", RNA), ("odd", ODD)):
        check(api, reads, p, "seams " + name)
    # the planted steps are found where they are
    off, rec = api.detect_events_batch(*rows([steps(3 * TILE + 17, [T]) for T in (63, 64, 65, 127, 128, 129, 255, 256, 257)]))
    assert np.diff(off).tolist() == [2] * 9
    assert rec["start"][1::2].tolist() == [63, 64, 65, 127, 128, 129, 255, 256, 257]


def test_steps_at_the_fill_round(gpu):
    from squigglekit_amd import api
    reads = [steps(FILL + 200, [p, FILL + 100]) for p in (FILL - 1, FILL, FILL + 1)]
    reads.append(steps(2 * FILL + 5, [70, FILL - 64, 2 * FILL, 2 * FILL + 1]))
    reads.append(steps(FILL + 200, []))                                   # one event over two rounds
    check(api, reads, DNA, "fill round")


def test_int16_extremes_and_flat_reads(gpu):
    from squigglekit_amd import api
    alt = np.where(np.arange(1000) % 2 == 0, -32768, 32767).astype(np.int16)
    blocks = np.repeat(np.where(np.arange(10) % 2 == 0, -32768, 32767), 100).astype(np.int16)
    reads = [alt, alt[:300], alt[1:130], blocks, np.full(500, 32767, np.int16), np.full(129, -32768, np.int16),
             np.zeros(64, np.int16), np.full(4000, 500, np.int16), np.full(1, 7, np.int16)]
    for name, p in (("wide", WIDE), ("dna", DNA), ("rna", RNA), ("w64", (64, 64, 0.0, 0.0, 0.0))):
        check(api, reads, p, "extremes " + name)
    off, rec = api.detect_events_batch(*rows(reads[4:]))
    assert np.diff(off).tolist() == [1] * 5                               # flat: v clamps to 1, t = 0, one event


@pytest.fixture(scope="module")
def noisy():
    rng = np.random.default_rng(99)
    return np.stack([squiggle(rng, 1000) for _ in range(256)])


@pytest.mark.parametrize("name, p", [("dna", DNA), ("rna", RNA)])
def test_noisy_batch(gpu, noisy, name, p):
    from squigglekit_amd import api
    got = api.detect_events_batch(noisy, None, par(api, p))
    assert_same(got, detect_ref.detect(list(noisy), p), "noisy " + name)
    assert got[0][-1] > 256 * 20


def test_device_form_equals_host_form_and_respects_cap(gpu, pool):
    from squigglekit_amd import api
    L = gpu.load()
    reads, want = pool
    woff, wrec = want["dna"]
    buf, lens = rows(reads, stride=904)
    R, total = len(reads), int(woff[-1])
    p = api.det_params()
    off, rec = api.detect_events_batch(buf, lens, p)
    assert_same((off, rec), (woff, wrec), "host form")
    pad = 16
    sizes = (buf.nbytes, lens.nbytes, (R + 1) * 8, (total + pad) * 24)
    d = [L.sk_dev_alloc(n) for n in sizes]
    try:
        assert all(d)
        gpu.check(L.sk_dev_upload(d[0], gpu.ptr(buf), buf.nbytes))
        gpu.check(L.sk_dev_upload(d[1], gpu.ptr(lens), lens.nbytes))
        canary = np.full((total + pad) * 24, 0xA5, dtype=np.uint8)
        for cap in (total - 1, 0, total):
            gpu.check(L.sk_dev_upload(d[3], gpu.ptr(canary), canary.nbytes))
            doff = np.full(R + 1, -1, dtype=np.int64)
            gpu.check(L.sk_dev_upload(d[2], gpu.ptr(doff), doff.nbytes))
            gpu.check(L.sk_detect_events_dev_i16(d[0], buf.shape[1], d[1], R, C.byref(p), d[2], d[3] if cap else None, cap))
            gpu.check(L.sk_sync())
            back = np.zeros_like(canary)
            gpu.check(L.sk_dev_download(gpu.ptr(doff), d[2], doff.nbytes))
            gpu.check(L.sk_dev_download(gpu.ptr(back), d[3], back.nbytes))
            assert doff.tobytes() == off.tobytes(), cap                   # off is always filled
            if cap < total:
                assert np.array_equal(back, canary), cap                  # too small: nothing is written at all
            else:
                assert back[:total * 24].tobytes() == rec.tobytes()       # byte for byte the host form's
                assert np.array_equal(back[total * 24:], canary[total * 24:])
    finally:
        for q in d:
            if q:
                L.sk_dev_free(q)


def test_host_cap_too_small(gpu, pool):
    from squigglekit_amd import api
    L = gpu.load()
    reads, want = pool
    woff, wrec = want["dna"]
    buf, lens = rows(reads, stride=904)
    R, total = len(reads), int(woff[-1])
    p = api.det_params()
    pad = 16
    for cap in (total - 1, 1):
        rec = np.zeros(total + pad, dtype=api.DET_EVENT_DTYPE)
        rec.view(np.uint8)[:] = 0xA5
        off = np.full(R + 1, -1, dtype=np.int64)
        rc = L.sk_detect_events_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, C.byref(p), gpu.ptr(off), gpu.ptr(rec), cap)
        assert rc == gpu.SK_ERR_OVERFLOW
        assert np.array_equal(off, woff)
        assert np.all(rec.view(np.uint8) == 0xA5)                         # nothing written, before or after rec[cap]
    # the counting call, then the retry with the count
    off = np.full(R + 1, -1, dtype=np.int64)
    assert L.sk_detect_events_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, C.byref(p), gpu.ptr(off), None, 0) == gpu.SK_ERR_OVERFLOW
    cap = int(off[R])
    assert cap == total
    rec = np.zeros(cap + pad, dtype=api.DET_EVENT_DTYPE)
    rec.view(np.uint8)[:] = 0xA5
    gpu.check(L.sk_detect_events_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, C.byref(p), gpu.ptr(off), gpu.ptr(rec), cap))
    assert rec[:cap].tobytes() == wrec.tobytes() and np.all(rec[cap:].view(np.uint8) == 0xA5)
    # lengths outside [0, stride] are clamped into it
    wild = lens.copy()
    wild[0], wild[1] = 10 ** 6, -5
    got = api.detect_events_batch(buf[:2], wild[:2], p)
    assert_same(got, detect_ref.detect([buf[0], buf[1, :0]], DNA), "clamped lengths")
    # no reads
    off0 = np.full(1, -1, dtype=np.int64)
    gpu.check(L.sk_detect_events_i16(None, 8, None, 0, C.byref(p), gpu.ptr(off0), None, 0))
    assert off0[0] == 0


def test_three_sub_batches_equal_one_call(gpu, pool, monkeypatch):
    """9 000 reads x stride 128 with SK_INGEST_MB=1: three sub-batches of 3 000 reads"""
    from squigglekit_amd import api
    reads, want = pool
    rng = np.random.default_rng(5)
    base = np.stack([squiggle(rng, 128) for _ in range(90)])
    sig = np.tile(base, (100, 1))
    lens = (np.arange(9000) * 37 % 129).astype(np.int32)
    one = api.detect_events_batch(sig, lens)
    monkeypatch.setenv("SK_INGEST_MB", "1")
    three = api.detect_events_batch(sig, lens)
    monkeypatch.delenv("SK_INGEST_MB")
    assert_same(three, one, "sub-batches")
    pick = [0, 1, 2999, 3000, 3001, 5999, 6000, 8999]                     # ... and both are the definition's
    for r in pick:
        woff, wrec = detect_ref.detect([sig[r, :lens[r]]], DNA)
        assert np.array_equal(one[1][one[0][r]:one[0][r + 1]], wrec), r
