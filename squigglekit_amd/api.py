"""Host-side mirror of the reference's two in-process boundaries, over the HIP C ABI.

    get_segs(sig, args)            <->  segmenter.get_segs      (segmenter.py:399)
    dtw_subsequence(x, y)          <->  mlpy.dtw_subsequence    (MotifSeq.py:437)

plus the batch forms the GPU actually wants (many reads per call).  All arithmetic
on samples happens in the HIP kernels; this module only marshals numpy buffers.
Same names, argument meaning and "no segments -> False" behaviour as the
reference so the parity tests read like calls into the reference.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BG_DTYPE, DET_EVENT_DTYPE, DetParams, EVENT_DTYPE, GATE_DTYPE, LiveGate, HIT_DTYPE, HMM_COUNTS_DTYPE, HMM_DTYPE, HMM_POST_DTYPE, HMM_SEG_DTYPE, HMM_SEGF_DTYPE, HMMS_DTYPE, HMMS_FILT_DTYPE, HmmModel, LEVEL_DTYPE, LIVEBEST_DTYPE, LIVEINFO_DTYPE, LiveRule, MAPREC_DTYPE, PANEL_DTYPE, PILE_DTYPE, POOL_DTYPE, STREAM_DTYPE, SWEEP_REC_DTYPE, SWEEP_SUM_DTYPE, SegParams, SquiggleKitError, SweepSet,  # noqa: F401
                   check, ptr)


# ----------------------------------------------------------------------------
# device selection
# ----------------------------------------------------------------------------
_default_devices = None


def set_devices(devices):
    """GPUs the batch calls shard their reads over when no `devices=` is passed (None / one entry: the
    calling thread's bound GPU, as before).  The CLIs' --gpus N sets range(N)."""
    global _default_devices
    devices = None if devices is None else [int(d) for d in devices]
    if devices is not None:
        n = _lib.load().sk_device_count()
        if not devices or len(set(devices)) != len(devices) or min(devices) < 0 or max(devices) >= max(n, 1):
            raise ValueError("devices %s: need distinct indices below the %d visible GPU(s)" % (devices, n))
    _default_devices = devices


def _devs(devices):
    return _default_devices if devices is None else devices


# ----------------------------------------------------------------------------
# pinned host buffers
# ----------------------------------------------------------------------------
def pinned_empty(shape, dtype=np.int16):
    """A numpy array in page-locked host memory (sk_host_alloc): the batch calls copy from it by DMA at PCIe
    speed, under the kernels of the previous sub-batch.  Freed when the array (and every view of it) is gone."""
    import weakref
    L = _lib.ensure_init()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = L.sk_host_alloc(max(1, n))
    if not p:
        check(-4)
    raw = (C.c_char * max(1, n)).from_address(p)
    arr = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(raw, L.sk_host_free, C.c_void_p(p))
    return arr


# ----------------------------------------------------------------------------
# packing helpers
# ----------------------------------------------------------------------------
def pack_i16(reads):
    """list of 1-D integer arrays -> (int16 [R, stride] zero padded, int32 lens).
    stride is a multiple of 8 so rows are 16-byte aligned (vector loads)."""
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    stride = int(max(8, (int(lens.max()) + 7) // 8 * 8)) if len(reads) else 8
    buf = np.zeros((len(reads), stride), dtype=np.int16)
    for i, r in enumerate(reads):
        buf[i, :len(r)] = r
    return buf, lens


def as_int16_exact(a):
    """The read as an int16 array if every value is an integer that fits int16, else None.
    (One cast and one comparison: a wrapped, rounded or NaN value fails the comparison.)"""
    a = np.asarray(a)
    if a.dtype == np.int16:
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        b = a.astype(np.int16)
    return b if (a.size == 0 or np.array_equal(b, a)) else None


def _split_int16(reads):
    """indices + int16 arrays of the integer-valued reads, indices of the rest"""
    ints, arrs, flts = [], [], []
    for i, r in enumerate(reads):
        b = as_int16_exact(r)
        if b is None:
            flts.append(i)
        else:
            ints.append(i)
            arrs.append(b)
    return ints, arrs, flts


def is_int16_exact(a):
    """True if every value of the float/int array is an integer that fits int16."""
    a = np.asarray(a)
    if a.size == 0:
        return True
    if a.dtype.kind in "iu":
        return bool(a.min() >= -32768 and a.max() <= 32767)
    return bool(np.all(np.isfinite(a)) and np.all(a == np.rint(a))
                and a.min() >= -32768 and a.max() <= 32767)


def _too_wide_for_i16(lo, hi):
    """The int16 kernels keep a histogram of the values between the outlier limits in LDS (up to
    ~38 900 values); wider limits go through the float64 kernels (radix select, same results)."""
    return min(int(hi), 32768) - max(int(lo), -32769) - 1 > 38000


# ----------------------------------------------------------------------------
# segmenter path
# ----------------------------------------------------------------------------
def segment_batch(sig, lens=None, params=None, max_segs=64, devices=None):
    """scale_outliers + get_segs for every row of an int16 [R, stride] batch.

    Returns (segs int32 [R, max_segs, 2], nsegs int32 [R]); grows max_segs and
    retries on overflow.  Coordinates are in the FILTERED signal, like the
    reference's (segmenter.py:209-211).  devices=[d0, d1, ...]: the reads are block-sharded over those
    GPUs, one host thread each (multigpu.py); results land in the same arrays, in input order."""
    devices = _devs(devices)
    L = _lib.load() if devices else _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None
            else np.ascontiguousarray(lens, dtype=np.int32))
    params = params or SegParams()
    if _too_wide_for_i16(params.lim_low, params.lim_hi):
        per_read = segment_reads_f64([sig[r, :lens[r]].astype(np.float64) for r in range(R)], params)
        nsegs = np.array([len(x) if x else 0 for x in per_read], dtype=np.int32)
        segs = np.zeros((R, max(max_segs, int(nsegs.max()) if R else 0), 2), dtype=np.int32)
        for r, x in enumerate(per_read):
            if x:
                segs[r, :len(x)] = x
        return segs, nsegs
    sharded = devices is not None and len(devices) > 1 and R >= len(devices)
    while True:
        segs = np.zeros((R, max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(R, dtype=np.int32)
        if sharded:
            from . import multigpu
            rcs = []

            def shard(lo, hi, comm, ms=max_segs):
                if hi > lo:
                    rc = L.sk_segment_batch_i16(ptr(sig[lo:hi]), stride, ptr(lens[lo:hi]), hi - lo, C.byref(params),
                                                ptr(segs[lo:hi]), ptr(nsegs[lo:hi]), ms)
                    if rc != _lib.SK_ERR_OVERFLOW:
                        check(rc)
                    rcs.append(rc)
            multigpu.run_sharded(devices, R, shard)
            rc = _lib.SK_ERR_OVERFLOW if _lib.SK_ERR_OVERFLOW in rcs else 0
        else:
            if devices:
                _lib.init(devices[0])
            rc = L.sk_segment_batch_i16(ptr(sig), stride, ptr(lens), R, C.byref(params),
                                        ptr(segs), ptr(nsegs), max_segs)
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        check(rc)
        return segs, nsegs


# ----------------------------------------------------------------------------
# segmenter parameter sweep
# ----------------------------------------------------------------------------
SWEEP_KEYS = ("error", "corrector", "window", "seg_dist", "std_scale", "stall_len", "lim_low", "lim_hi",
              "stall_start", "gap_dist")
SWEEP_DEFAULTS = dict(error=5, corrector=50, window=150, seg_dist=50, std_scale=0.75, stall_len=0.25, lim_low=0,
                      lim_hi=900, stall_start=300, gap_dist=3000)        # segmenter.py's argparse defaults
_SWEEP_FLOAT = ("std_scale", "stall_len")


def sweep_set(**kw):
    """One sweep set (sk_seg_sweep_set) from keyword values of SWEEP_KEYS; the others take segmenter.py's defaults."""
    bad = set(kw) - set(SWEEP_KEYS)
    if bad:
        raise TypeError("unknown sweep parameter(s): %s" % ", ".join(sorted(bad)))
    v = dict(SWEEP_DEFAULTS, **kw)
    seg = SegParams(int(v["error"]), int(v["corrector"]), int(v["window"]), int(v["seg_dist"]), float(v["std_scale"]),
                    float(v["stall_len"]), int(v["lim_low"]), int(v["lim_hi"]))
    return SweepSet(seg, int(v["stall_start"]), int(v["gap_dist"]))


def sweep_values(s):
    """The ten parameters of a sweep set, in SWEEP_KEYS order."""
    g = s.seg
    return (g.error, g.corrector, g.window, g.seg_dist, g.std_scale, g.stall_len, g.lim_low, g.lim_hi, s.stall_start,
            s.gap_dist)


def sweep_grid(**kw):
    """The Cartesian product of the given values as a list of sweep sets.  Each argument (any of SWEEP_KEYS) is a scalar
    or a sequence; the others take segmenter.py's defaults.  Order: error, corrector, window, seg_dist, std_scale,
    stall_len, lim_low, lim_hi, stall_start, gap_dist -- the last one varying fastest."""
    import itertools
    bad = set(kw) - set(SWEEP_KEYS)
    if bad:
        raise TypeError("unknown sweep parameter(s): %s" % ", ".join(sorted(bad)))
    axes = []
    for k in SWEEP_KEYS:
        v = kw.get(k, SWEEP_DEFAULTS[k])
        axes.append(list(v) if isinstance(v, (list, tuple, range, np.ndarray)) else [v])
    return [sweep_set(**dict(zip(SWEEP_KEYS, combo))) for combo in itertools.product(*axes)]


def _check_sweep_sets(sets):
    for k, s in enumerate(sets):
        if s.seg.corrector < 0:
            raise ValueError("sweep set %d: corrector must be >= 0 (the reference divides by zero otherwise)" % k)


def _sweep_route(entry, R, args_of, sets, records, devices):
    """One sweep entry point over R reads, block-sharded over `devices`: (sums, recs) with the shards' counts added and
    their records in input order."""
    import threading
    ns = len(sets)
    arr = (SweepSet * max(ns, 1))(*sets)
    sums = np.zeros(ns, dtype=SWEEP_SUM_DTYPE)
    recs = np.zeros((ns, R), dtype=SWEEP_REC_DTYPE) if records else None
    lock = threading.Lock()

    def call(lo, hi):
        part = np.zeros(max(ns, 1), dtype=SWEEP_SUM_DTYPE)
        rp = np.zeros((ns, hi - lo), dtype=SWEEP_REC_DTYPE) if records else None
        rc = entry(*args_of(lo, hi), arr, ns, ptr(part), None if rp is None or rp.size == 0 else ptr(rp))
        if rc == 0:
            with lock:
                sums.view(np.int64).reshape(ns, 8)[:] += part[:ns].view(np.int64).reshape(ns, 8)
                if rp is not None:
                    recs[:, lo:hi] = rp
        return rc
    if ns:
        _over_devices(devices, R, call)
    return sums, recs


def _add_sweep(a, b):
    out = a.copy()
    out.view(np.int64).reshape(len(a), 8)[:] += b.view(np.int64).reshape(len(b), 8)
    return out


def segment_sweep(reads, sets, lens=None, records=False, devices=None):
    """segmenter.py's scale_outliers + get_segs + test_segs for every set of a grid over the same reads, in one pass per
    distinct (lim_low, lim_hi, std_scale) (sk_segment_sweep_i16 / _f64).

    reads: an int16 [R, stride] batch (with `lens`), or a list of reads routed like segment_any -- integer-valued reads
    that fit int16 go to the int16 entry, the others to the float64 one; sets whose limits are too wide for the int16
    kernels take the float64 route too, as in segment_batch.  sets: sweep sets (sweep_grid / sweep_set).
    Returns (sums, recs): sums a SWEEP_SUM_DTYPE array [nsets], recs a SWEEP_REC_DTYPE array [nsets, R] (records=True)
    or None.  For set k and read r the record holds what segment_batch reports with set k's params: the segment count
    and the first two segments (-1 where there is none).  devices: the reads are block-sharded over those GPUs."""
    sets = list(sets)
    _check_sweep_sets(sets)
    L = _lib.load()
    ns = len(sets)
    if isinstance(reads, np.ndarray) and reads.ndim == 2:
        sig = np.ascontiguousarray(reads, dtype=np.int16)
        R, stride = sig.shape
        ln = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
        ints, arrs, flts = list(range(R)), None, []
    else:
        if lens is not None:
            raise ValueError("lens goes with an int16 [R, stride] batch")
        R = len(reads)
        ints, arrs, flts = _split_int16(reads)
        sig = ln = None
        if ints:
            sig, ln = pack_i16(arrs)
    wide = [k for k, s in enumerate(sets) if _too_wide_for_i16(s.seg.lim_low, s.seg.lim_hi)]
    narrow = [k for k in range(ns) if k not in set(wide)]
    sums = np.zeros(ns, dtype=SWEEP_SUM_DTYPE)
    recs = np.zeros((ns, R), dtype=SWEEP_REC_DTYPE) if records else None

    def put(idx_sets, idx_reads, part):
        ps, pr = part
        sums[idx_sets] = _add_sweep(sums[idx_sets], ps)
        if records:
            recs[np.ix_(idx_sets, idx_reads)] = pr

    def f64_route(rows, idx_reads, idx_sets):
        flat, off = pack_f64(rows)
        sub = [sets[k] for k in idx_sets]
        put(idx_sets, idx_reads, _sweep_route(L.sk_segment_sweep_f64, len(rows),
                                              lambda lo, hi: (ptr(flat), ptr(off[lo:hi + 1]), None, hi - lo),
                                              sub, records, devices))
    if ints:
        stride = sig.shape[1]
        if narrow:
            sub = [sets[k] for k in narrow]
            put(narrow, ints, _sweep_route(L.sk_segment_sweep_i16, len(ints),
                                           lambda lo, hi: (ptr(sig[lo:hi]), stride, ptr(ln[lo:hi]), hi - lo),
                                           sub, records, devices))
        if wide:
            f64_route([sig[i, :ln[i]].astype(np.float64) for i in range(len(ints))], ints, wide)
    if flts:
        f64_route([np.asarray(reads[i], dtype=np.float64) for i in flts], flts, list(range(ns)))
    return sums, recs


def segment_reads(reads, params=None):
    """Fused scale_outliers + get_segs on a list of raw integer reads.
    Returns, per read, a list of [start, end] or False (the reference's value)."""
    if not len(reads):
        return []
    buf, lens = pack_i16(reads)
    segs, nsegs = segment_batch(buf, lens, params)
    return [segs[i, :nsegs[i]].tolist() if nsegs[i] else False for i in range(len(reads))]


def pack_f64(reads):
    """list of 1-D float arrays -> (flat float64, int64 offsets[R+1])."""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    for i, r in enumerate(reads):
        off[i + 1] = off[i] + len(r)
    flat = (np.concatenate([np.asarray(r, dtype=np.float64) for r in reads])
            if len(reads) else np.zeros(0))
    return np.ascontiguousarray(flat, dtype=np.float64), off


def segment_reads_f64(reads, params=None, max_segs=64):
    """Fused scale_outliers + get_segs on float64 (pA) reads (segmenter.py:198-199)."""
    if not len(reads):
        return []
    L = _lib.ensure_init()
    flat, off = pack_f64(reads)
    params = params or SegParams()
    R = len(reads)
    while True:
        segs = np.zeros((R, max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(R, dtype=np.int32)
        rc = L.sk_segment_batch_f64(ptr(flat), ptr(off), R, C.byref(params), ptr(segs), ptr(nsegs), max_segs)
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        check(rc)
        return [segs[i, :nsegs[i]].tolist() if nsegs[i] else False for i in range(R)]


def _flat_motifs(motifs):
    """A list of motifs as the multi-motif entry points take it: (the float64 arrays, all points in one array, int32
    offsets [len + 1])."""
    ms = [np.ascontiguousarray(m, dtype=np.float64) for m in motifs]
    flat = np.ascontiguousarray(np.concatenate(ms)) if ms else np.zeros(0)
    moff = np.concatenate([[0], np.cumsum([m.size for m in ms])]).astype(np.int32)
    return ms, flat, moff


def _over_devices(devices, R, call):
    """call(lo, hi) -> status on the calling thread's GPU, or -- with several devices -- on one host thread per GPU
    over the block split of the R reads (multigpu.run_sharded; every shard writes its slice of the caller's arrays).
    Returns SK_ERR_OVERFLOW if any shard overflowed, else 0; any other failure raises."""
    devices = _devs(devices)
    if devices is not None and len(devices) > 1 and R >= len(devices):
        from . import multigpu
        rcs = []

        def shard(lo, hi, comm):
            if hi > lo:
                rc = call(lo, hi)
                if rc != _lib.SK_ERR_OVERFLOW:
                    check(rc)
                rcs.append(rc)
        multigpu.run_sharded(devices, R, shard)
        return _lib.SK_ERR_OVERFLOW if _lib.SK_ERR_OVERFLOW in rcs else 0
    if devices:
        _lib.init(devices[0])
    else:
        _lib.ensure_init()
    rc = call(0, R)
    if rc != _lib.SK_ERR_OVERFLOW:
        check(rc)
    return rc


def segment_batch_pa(sig, lens, calib, params=None, max_segs=64, devices=None):
    """Raw int16 rows through the pA route (segmenter.py:345-349: fast5 / slow5 input without --raw_signal): the
    conversion np.round((raw + offset) * (float("%.2f" % range) / digitisation), 2) is a monotone map of the sample, so
    since round 6 the rows stay int16 on the GPU and limits, median, std and thresholds are found in the raw domain
    (k_seg_stats<.., PA>; reads it cannot certify are redone from their float64 values in numpy's order).
    calib: float64 [R, 3] = digitisation, offset, range per read.  Returns (segs, nsegs).
    devices (or api.set_devices / --gpus): the reads are block-sharded like segment_batch's."""
    L = _lib.load()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    R = sig.shape[0]
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    calib = np.ascontiguousarray(calib, dtype=np.float64).reshape(R, 3)
    params = params or SegParams()
    while True:
        segs = np.zeros((max(R, 1), max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(max(R, 1), dtype=np.int32)
        rc = _over_devices(devices, R, lambda lo, hi, ms=max_segs: L.sk_segment_batch_i16_pa(
            ptr(sig[lo:hi]), sig.shape[1], ptr(lens[lo:hi]), hi - lo, ptr(calib[lo:hi]), C.byref(params),
            ptr(segs[lo:hi]), ptr(nsegs[lo:hi]), ms))
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        return segs[:R], nsegs[:R]


def pack_prefixes(prefixes):
    """A list of bytes -> (blob, int64 offsets [n + 1]) for pull_text; a (blob, offsets) pair passes through."""
    if isinstance(prefixes, tuple):
        blob, off = prefixes
        return blob, np.ascontiguousarray(off, dtype=np.int64)
    off = np.zeros(len(prefixes) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in prefixes], out=off[1:])
    return b"".join(prefixes), off


def pull_text(rows, lens, prefixes, calib=None, raw=False, out=None):
    """SquigglePull's lines for int16 rows, made on the GPU (sk_pull_text; SquigglePull.py:178-189, 211-222, 238-253):
    read r's line is prefixes[r] + the first lens[r] samples of rows[r], tab-separated, + "\n" -- str(int(x)) with
    raw=True, else str(np.round((x + offset) * (float("%.2f" % range) / digitisation), 2)) with calib[r] = digitisation,
    offset, range (float64 [n, 3], as Blow5Block.calib holds them; the range is cut to two decimals on the host).
    prefixes: a list of bytes (file name, read id, -i columns, trailing tab), or a (blob, offsets) pair.
    Returns bytes; with `out` (a uint8 array, e.g. pinned) the text goes there and a memoryview of it comes back
    (a larger array is made when `out` is too small)."""
    L = _lib.ensure_init()
    rows = np.ascontiguousarray(rows, dtype=np.int16)
    R = rows.shape[0] if rows.ndim == 2 else 0
    stride = max(1, rows.shape[1] if rows.ndim == 2 else 1)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    blob, poff = pack_prefixes(prefixes)
    if len(lens) != R or len(poff) != R + 1:
        raise ValueError("rows, lens and prefixes disagree on the number of reads")
    mode = _lib.SK_PULL_RAW if raw else _lib.SK_PULL_PA
    cal = None
    if not raw and R:
        cal = np.ascontiguousarray(calib, dtype=np.float64).reshape(R, 3)
    pbuf = np.frombuffer(blob, dtype=np.uint8) if len(blob) else np.zeros(1, dtype=np.uint8)
    # most tokens take at most 7 characters + separator ("-123.45\t", "-32768\t"): a retry with the exact size otherwise
    cap = int(poff[-1] - poff[0]) + 8 * int(lens.sum()) + R + 1
    total = C.c_int64(0)
    while True:
        buf = out if out is not None and out.nbytes >= cap else np.empty(cap, dtype=np.uint8)
        rc = L.sk_pull_text(ptr(rows), stride, ptr(lens), R, None if cal is None else ptr(cal), mode, ptr(pbuf), ptr(poff),
                            ptr(buf), buf.nbytes, C.byref(total), None)
        if rc == _lib.SK_ERR_OVERFLOW and total.value > buf.nbytes:
            cap = total.value
            continue
        check(rc)
        break
    if out is not None:
        return memoryview(buf)[:total.value]
    return buf[:total.value].tobytes()


def last_pa_retries():
    """Reads of the most recent segment_batch_pa call on this thread's device (all its sub-batches) that took the
    numpy-order redo; -1 when the call expanded its rows to float64 instead of staying in the raw domain, or when a
    MotifSeq / segmenter call of another route came after it."""
    return int(_lib.load().sk_last_pa_retries())


def segment_ragged_f64(values, off, lens=None, params=None, max_segs=64, devices=None):
    """scale_outliers + get_segs for a ragged float64 batch as a tokenizer leaves it: read r is the first lens[r]
    (default: all) of values[off[r]:off[r+1]].  Returns (segs int32 [R, max_segs, 2], nsegs int32 [R]).
    devices (or api.set_devices / --gpus): block-sharded over the GPUs (a shard is a run of offsets into the same
    `values`: nothing is repacked)."""
    L = _lib.load()
    # int32 values are centi-units (tsvio.FloatBlock.centi: tokens with at most two decimals): sample = c / 100.0 on the GPU
    centi = isinstance(values, np.ndarray) and values.dtype == np.int32
    values = np.ascontiguousarray(values, dtype=np.int32 if centi else np.float64)
    entry = L.sk_segment_batch_centi_len if centi else L.sk_segment_batch_f64_len
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = off.size - 1
    params = params or SegParams()
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    while True:
        segs = np.zeros((max(R, 1), max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(max(R, 1), dtype=np.int32)
        rc = _over_devices(devices, R, lambda lo, hi, ms=max_segs: entry(
            ptr(values), ptr(off[lo:hi + 1]), None if ln is None else ptr(ln[lo:hi]), hi - lo, C.byref(params),
            ptr(segs[lo:hi]), ptr(nsegs[lo:hi]), ms))
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        return segs[:R], nsegs[:R]


# ----------------------------------------------------------------------------
# segment levels: per-segment and per-read signal statistics, raw coordinates
# ----------------------------------------------------------------------------
def no_levels(shape):
    """LEVEL_DTYPE records of slots that hold no span: six NaNs, raw_start = raw_end = -1, n = 0."""
    a = np.zeros(shape, dtype=LEVEL_DTYPE)
    for f in ("mean", "std", "median", "mad", "min", "max"):
        a[f] = np.nan
    a["raw_start"] = a["raw_end"] = -1
    return a


def _levels_call(R, max_segs, devices, call):
    """The shared tail of the levels calls: call(lo, hi, segs, nsegs, levels, read_level, max_segs) -> status over the
    reads [lo, hi) (sharded over `devices` like segment_batch), max_segs grown until no read overflows."""
    while True:
        segs = np.zeros((max(R, 1), max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(max(R, 1), dtype=np.int32)
        levels = no_levels((max(R, 1), max_segs))
        read_level = no_levels(max(R, 1))
        rc = _over_devices(devices, R, lambda lo, hi, ms=max_segs: call(lo, hi, segs, nsegs, levels, read_level, ms))
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        return segs[:R], nsegs[:R], levels[:R], read_level[:R]


def segment_levels_ragged_f64(values, off, lens=None, params=None, max_segs=64, devices=None):
    """segment_ragged_f64, and what every segment is: (segs, nsegs, levels, read_level).  levels[r, k] (LEVEL_DTYPE) is the
    record of segs[r, k] = [s, e] over w = y[s:e], y the read after the cut and scale_outliers: np.mean, np.std, np.median,
    np.median(np.abs(w - median)), min, max -- numpy's bits -- and raw_start, raw_end, the slice of the RAW read that,
    filtered, is w.  read_level[r] is the same over all of y.  float64 values, or int32 centi-units."""
    L = _lib.load()
    centi = isinstance(values, np.ndarray) and values.dtype == np.int32
    values = np.ascontiguousarray(values, dtype=np.int32 if centi else np.float64)
    entry = L.sk_segment_levels_centi_len if centi else L.sk_segment_levels_f64_len
    off = np.ascontiguousarray(off, dtype=np.int64)
    params = params or SegParams()
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    return _levels_call(off.size - 1, max_segs, devices, lambda lo, hi, segs, nsegs, lv, rl, ms: entry(
        ptr(values), ptr(off[lo:hi + 1]), None if ln is None else ptr(ln[lo:hi]), hi - lo, C.byref(params),
        ptr(segs[lo:hi]), ptr(nsegs[lo:hi]), ms, ptr(lv[lo:hi]), ptr(rl[lo:hi])))


def segment_levels_batch(sig, lens=None, params=None, max_segs=64, devices=None):
    """segment_batch, and what every segment is: (segs, nsegs, levels, read_level) for the rows of an int16 [R, stride]
    batch (see segment_levels_ragged_f64; w is int64 here, as segmenter.py:200-201 makes it).  Limits too wide for the
    int16 kernels go through the float64 ones, like segment_batch's."""
    L = _lib.load()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    params = params or SegParams()
    if _too_wide_for_i16(params.lim_low, params.lim_hi):
        off = np.arange(R + 1, dtype=np.int64) * stride
        return segment_levels_ragged_f64(sig.astype(np.float64).reshape(-1), off, lens, params, max_segs, devices)
    return _levels_call(R, max_segs, devices, lambda lo, hi, segs, nsegs, lv, rl, ms: L.sk_segment_levels_i16(
        ptr(sig[lo:hi]), stride, ptr(lens[lo:hi]), hi - lo, C.byref(params), ptr(segs[lo:hi]), ptr(nsegs[lo:hi]), ms,
        ptr(lv[lo:hi]), ptr(rl[lo:hi])))


def pa_values(sig, lens, calib):
    """The float64 pA reads segmenter.py makes of raw rows (convert_to_pA_numpy + np.round(.., 2), segmenter.py:345-349,
    515-520; range cut to two decimals first, :385): a list of arrays."""
    calib = np.asarray(calib, dtype=np.float64).reshape(-1, 3)
    out = []
    for r in range(len(lens)):
        dig, ofs, rng = calib[r]
        unit = float("{0:.2f}".format(rng)) / dig
        out.append(np.round((np.asarray(sig[r][:lens[r]], dtype=np.float64) + ofs) * unit, 2))
    return out


def segment_levels_batch_pa(sig, lens, calib, params=None, max_segs=64, devices=None):
    """segment_batch_pa's reads with their levels: the float64 pA values are formed first (pa_values) and go through the
    float64 route, so that every record is numpy's on the pA array."""
    flat, off = pack_f64(pa_values(sig, lens, calib))
    return segment_levels_ragged_f64(flat, off, None, params, max_segs, devices)


def segment_levels(reads, params=None):
    """Mixed input, as segment_any: integer-valued reads that fit int16 through the int16 route, the rest through the
    float64 one.  Returns (segs, nsegs, levels, read_level) in input order, max_segs the widest any route needed."""
    ints, arrs, flts = _split_int16(reads)
    parts = []
    if ints:
        buf, lens = pack_i16(arrs)
        parts.append((ints, segment_levels_batch(buf, lens, params)))
    if flts:
        flat, off = pack_f64([reads[i] for i in flts])
        parts.append((flts, segment_levels_ragged_f64(flat, off, None, params)))
    R = len(reads)
    ms = max([p[1][0].shape[1] for p in parts] or [1])
    segs = np.zeros((R, ms, 2), dtype=np.int32)
    nsegs = np.zeros(R, dtype=np.int32)
    levels = no_levels((R, ms))
    read_level = no_levels(R)
    for idx, (sg, ns, lv, rl) in parts:
        segs[idx, :sg.shape[1]] = sg
        nsegs[idx] = ns
        levels[idx, :lv.shape[1]] = lv
        read_level[idx] = rl
    return segs, nsegs, levels, read_level


def thresholds_of(read_level, params=None):
    """(top, bot) of get_segs from the whole-read records: median + std * std_scale and median - std * std_scale, two
    float64 operations each in the order of segmenter.py:413-414."""
    params = params or SegParams()
    rl = np.asarray(read_level)
    d = rl["std"].astype(np.float64) * np.float64(params.std_scale)
    return rl["median"] + d, rl["median"] - d


LEVELS_HEADER = ("fast5", "seg", "start", "end", "raw_start", "raw_end", "length", "mean", "stdev", "median", "mad", "min",
                 "max", "read_median", "read_stdev", "top", "bot")


def levels_lines(name, segs, levels, read_level, params=None):
    """The rows `segmenter.py --levels FILE` writes for one printed read: one tab-separated line per segment, columns
    LEVELS_HEADER, floats as Python's "{}" writes them.  segs: the [start, end] pairs printed for the read."""
    top, bot = thresholds_of(read_level, params)
    out = []
    for k, (s, e) in enumerate(segs):
        v = levels[k]
        cols = [name, k, int(s), int(e), int(v["raw_start"]), int(v["raw_end"]), int(v["n"])]
        cols += [float(v[f]) for f in ("mean", "std", "median", "mad", "min", "max")]
        cols += [float(read_level["median"]), float(read_level["std"]), float(top), float(bot)]
        out.append("\t".join("{}".format(c) for c in cols) + "\n")
    return out


def motifseq_multi_ragged_f64(values, off, motifs, scale="medmad", scale_low=0, scale_hi=1200, devices=None):
    """Every motif against a ragged float64 batch (read r = values[off[r]:off[r+1]]): one record array per motif.
    devices (or api.set_devices / --gpus): block-sharded over the GPUs."""
    L = _lib.load()
    centi = isinstance(values, np.ndarray) and values.dtype == np.int32      # centi-units, see segment_ragged_f64
    values = np.ascontiguousarray(values, dtype=np.int32 if centi else np.float64)
    entry = L.sk_motifseq_multi_batch_centi if centi else L.sk_motifseq_multi_batch_f64
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = off.size - 1
    # a shard is staged and filtered ONCE, every motif runs against it on the device (sk_motifseq_multi_batch_f64)
    return _multi_over(devices, R, motifs, scale, scale_low, scale_hi,
                       lambda lo, hi, *tail: entry(ptr(values), ptr(off[lo:hi + 1]), hi - lo, *tail))


def _multi_over(devices, R, motifs, scale, scale_low, scale_hi, entry_call):
    """Runs entry_call(lo, hi, motifs, motif_off, nmotifs, scale_mode, scale_low, scale_hi, out) -- the tail of every
    multi-motif first-match entry point -- over the devices (_over_devices: every shard writes its reads); returns one
    HIT_DTYPE array [R] per motif."""
    ms, flat, moff = _flat_motifs(motifs)
    out = np.zeros((len(ms), R), dtype=HIT_DTYPE)

    def call(lo, hi):
        part = np.zeros((len(ms), hi - lo), dtype=HIT_DTYPE)
        rc = entry_call(lo, hi, ptr(flat), ptr(moff), len(ms), _lib.SK_SCALE[scale], int(scale_low), int(scale_hi), ptr(part))
        if rc == 0:
            out[:, lo:hi] = part
        return rc
    if R and ms:
        _over_devices(devices, R, call)
    return list(out)


def drna_segment_batch(sig, lens, params=None, max_segs=32):
    """dRNA_segmenter.py's slow5 branch for every row of an int16 [R, stride] batch: (segs int32 [R, max_segs, 2], nsegs)."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    params = params or _lib.DrnaParams()
    R = sig.shape[0]
    while True:
        segs = np.zeros((max(R, 1), max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(max(R, 1), dtype=np.int32)
        rc = L.sk_drna_segment_batch_i16(ptr(sig), sig.shape[1], ptr(lens), R, C.byref(params), ptr(segs), ptr(nsegs), max_segs)
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        check(rc)
        return segs[:R], nsegs[:R]


def drna_segment_reads(reads, params=None, max_segs=32):
    """dRNA_segmenter.py's slow5-branch per-read work (scale_outliers, window statistics, scan)
    for a list of raw integer reads: per read the list of [start, end] collected before the scan
    stopped (the script prints only the first, dRNA_segmenter.py:173-176)."""
    if not len(reads):
        return []
    L = _lib.ensure_init()
    buf, lens = pack_i16(reads)
    params = params or _lib.DrnaParams()
    R = len(reads)
    while True:
        segs = np.zeros((R, max_segs, 2), dtype=np.int32)
        nsegs = np.zeros(R, dtype=np.int32)
        rc = L.sk_drna_segment_batch_i16(ptr(buf), buf.shape[1], ptr(lens), R, C.byref(params),
                                         ptr(segs), ptr(nsegs), max_segs)
        if rc == _lib.SK_ERR_OVERFLOW:
            max_segs = int(nsegs.max()) + 8
            continue
        check(rc)
        return [segs[i, :nsegs[i]].tolist() for i in range(R)]


def segment_any(reads, params=None):
    """Route each read to the int16 kernels when it is integer valued and fits,
    else to the float64 kernels; results come back in input order."""
    ints, arrs, flts = _split_int16(reads)
    out = [None] * len(reads)
    if ints:
        for i, res in zip(ints, segment_reads(arrs, params)):
            out[i] = res
    if flts:
        for i, res in zip(flts, segment_reads_f64([reads[i] for i in flts], params)):
            out[i] = res
    return out


def get_segs(sig, args):
    """Drop-in for segmenter.get_segs(sig, args): `sig` is already filtered
    (segmenter.py:209), args carries error/corrector/window/seg_dist/std_scale/
    stall_len.  Returns [[start, end], ...] or False."""
    sig = np.asarray(sig)
    if sig.size == 0:
        return False
    # limits that keep every sample: the caller has already run scale_outliers
    lo = int(np.floor(float(sig.min()))) - 1
    hi = int(np.ceil(float(sig.max()))) + 1
    p = SegParams(args.error, args.corrector, args.window, args.seg_dist, args.std_scale,
                  args.stall_len, lo, hi)
    return segment_any([sig], p)[0]


def test_segs(segs, args, err=None):
    """segmenter.test_segs (segmenter.py:473-494): host-side acceptance filter.
    Messages go to `err` (a file object) exactly as the reference writes them."""
    import sys
    import traceback
    err = err or sys.stderr
    try:
        if args.stall:
            if segs[0][0] > args.stall_start:
                err.write("start seg too late!")
                return False
        if args.gap:
            if segs[1][0] > segs[0][1] + args.gap_dist:
                err.write("second seg too far!")
                return False
    except Exception:                                   # reference: bare except, read passes
        err.write("something went wrong test_segs()")
        traceback.print_exc(file=err)
    return segs


def drna_roll_reads(reads, params=None):
    """dRNA_segmenter.py's --signal branch (:272-326) on raw integer reads: per read (x, y) -- the first
    low rolling-mean segment of acceptable length, both ends shifted as the script prints them -- or None."""
    if not len(reads):
        return []
    from ._lib import RollParams
    L = _lib.ensure_init()
    params = params or RollParams()
    buf, lens = pack_i16(reads)
    R = len(reads)
    xy = np.zeros((R, 2), dtype=np.int32)
    found = np.zeros(R, dtype=np.int32)
    check(L.sk_drna_roll_batch_i16(ptr(buf), buf.shape[1], ptr(lens), R, C.byref(params), ptr(xy), ptr(found)))
    return [(int(xy[i, 0]), int(xy[i, 1])) if found[i] else None for i in range(R)]


# ----------------------------------------------------------------------------
# MotifSeq path
# ----------------------------------------------------------------------------
def motifseq_batch(sig, lens, motif, scale="medmad", scale_low=0, scale_hi=1200, devices=None, gather="host"):
    """scale_outliers + medmad/zscale + dtw_subsequence for every row of an
    int16 [R, stride] batch.  Returns a HIT_DTYPE record array (dist, start,
    end, n, flags); start/end index the FILTERED signal (MotifSeq.py:438-439).
    devices=[d0, d1, ...]: reads block-sharded over those GPUs, one host thread each; gather="host" writes
    every shard's records straight into the result, gather="rccl" all-gathers them GPU to GPU first (RCCL) and
    downloads the complete result from the first device (multigpu.motifseq_sharded)."""
    devices = _devs(devices)
    L = _lib.load()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None
            else np.ascontiguousarray(lens, dtype=np.int32))
    motif = np.ascontiguousarray(motif, dtype=np.float64)
    if _too_wide_for_i16(scale_low, scale_hi):
        return motifseq_reads_f64([sig[r, :lens[r]].astype(np.float64) for r in range(R)], motif, scale,
                                  scale_low, scale_hi)
    if gather == "rccl" and devices is not None and len(devices) > 1 and R >= len(devices):
        from . import multigpu
        return multigpu.motifseq_sharded(sig, lens, motif, _lib.SK_SCALE[scale], scale_low, scale_hi,
                                         devices, gather="rccl")[0]
    out = np.zeros(R, dtype=HIT_DTYPE)
    _over_devices(devices, R, lambda lo, hi: L.sk_motifseq_batch_i16(
        ptr(sig[lo:hi]), stride, ptr(lens[lo:hi]), hi - lo, ptr(motif), motif.size, _lib.SK_SCALE[scale], int(scale_low),
        int(scale_hi), ptr(out[lo:hi])))
    return out


GUARD_FIELDS = ("premise_violations", "audited", "audit_mismatches", "image_rejects", "alarm", "exact_fallback",
                "second_windows")


def last_dtw_guard():
    """Run-time guard counters of the most recent DTW call on this thread's device (sk_last_dtw_guard): premise
    violations the window pass found, reads audited by the exact pass and how many of them differed, reads kept from
    the screening because their sample image could not be bounded, the alarm count, and whether the whole call was
    redone by the exact pass.  A healthy build reports 0 violations / 0 mismatches, always."""
    g = (C.c_int32 * 8)()
    check(_lib.load().sk_last_dtw_guard(g))
    return dict(zip(GUARD_FIELDS, (int(v) for v in g)))


def motifseq_reads_f64(reads, motif, scale="medmad", scale_low=0, scale_hi=1200):
    """Same as motifseq_batch for float64 (pA) reads given as a list (MotifSeq.py:270)."""
    L = _lib.ensure_init()
    flat, off = pack_f64(reads)
    motif = np.ascontiguousarray(motif, dtype=np.float64)
    out = np.zeros(len(reads), dtype=HIT_DTYPE)
    check(L.sk_motifseq_batch_f64(ptr(flat), ptr(off), len(reads), ptr(motif), motif.size,
                                  _lib.SK_SCALE[scale], int(scale_low), int(scale_hi), ptr(out)))
    return out


def motifseq_any(reads, motif, scale="medmad", scale_low=0, scale_hi=1200):
    """Integer-valued reads go through the int16 kernels, the rest through the
    float64 kernels (bit-identical results either way); input order is kept."""
    out = np.zeros(len(reads), dtype=HIT_DTYPE)
    ints, arrs, flts = _split_int16(reads)
    if ints:
        buf, lens = pack_i16(arrs)
        out[ints] = motifseq_batch(buf, lens, motif, scale, scale_low, scale_hi)
    if flts:
        out[flts] = motifseq_reads_f64([reads[i] for i in flts], motif, scale, scale_low, scale_hi)
    return out


def stall_cuts(reads, seg_params=None):
    """[extension -- the author's TODO "integration with MotifSeq", segmenter.py:35]  Per read, the raw
    index right after the first segment the segmenter finds (the stall at the start of a read), 0 when it
    finds none: the filtered coordinate get_segs reports is mapped back through scale_outliers' mask."""
    params = seg_params or SegParams()
    cuts = np.zeros(len(reads), dtype=np.int64)
    for i, (r, s) in enumerate(zip(reads, segment_any(reads, params))):
        if s:
            a = np.asarray(r)
            kept = np.flatnonzero((a > params.lim_low) & (a < params.lim_hi))      # segmenter.py:311-318
            e = s[0][1]
            cuts[i] = int(kept[e]) if e < kept.size else int(a.size)
    return cuts


def motifseq_after_stall(reads, motif, scale="medmad", scale_low=0, scale_hi=1200, seg_params=None):
    """[extension]  MotifSeq on what follows the stall: reads[i][cut:] goes through the usual filter,
    normalisation and subsequence DTW.  Returns (hits, cuts); hit coordinates index the filtered slice."""
    cuts = stall_cuts(reads, seg_params)
    return motifseq_any([np.asarray(r)[c:] for r, c in zip(reads, cuts)], motif, scale, scale_low, scale_hi), cuts


def _multi_rows(buf, lens, motifs, scale, scale_low, scale_hi):
    """Every motif against the rows of a packed int16 batch (limits the int16 kernels take): one array per motif."""
    L = _lib.load()
    return _multi_over(None, buf.shape[0], motifs, scale, scale_low, scale_hi,
                       lambda lo, hi, *tail: L.sk_motifseq_multi_batch_i16(ptr(buf[lo:hi]), buf.shape[1], ptr(lens[lo:hi]),
                                                                           hi - lo, *tail))


def motifseq_multi_batch(sig, lens, motifs, scale="medmad", scale_low=0, scale_hi=1200):
    """Every motif of `motifs` against every row of an int16 [R, stride] batch (one filter / statistics pass):
    list (one per motif) of HIT_DTYPE arrays in read order.  The block form of motifseq_multi."""
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    R = sig.shape[0]
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    if _too_wide_for_i16(scale_low, scale_hi):
        return motifseq_multi([sig[r, :lens[r]] for r in range(R)], motifs, scale, scale_low, scale_hi)
    return _multi_rows(sig, lens, motifs, scale, scale_low, scale_hi)


def motifseq_multi(reads, motifs, scale="medmad", scale_low=0, scale_hi=1200):
    """Every motif of `motifs` (list of float vectors) against every read: list (one per motif,
    in order) of HIT_DTYPE arrays in read order -- the double loop of MotifSeq.py:261-298,436.
    The reads share one filter/statistics pass across motifs: the integer-valued ones as int16 rows, the rest as one
    ragged float64 batch."""
    motifs = list(motifs)
    outs = [np.zeros(len(reads), dtype=HIT_DTYPE) for _ in motifs]
    ints, arrs, flts = _split_int16(reads)
    if ints and motifs:
        for k, part in enumerate(_multi_rows(*pack_i16(arrs), motifs, scale, scale_low, scale_hi)):
            outs[k][ints] = part
    if flts and motifs:
        flat, off = pack_f64([reads[i] for i in flts])
        for k, part in enumerate(motifseq_multi_ragged_f64(flat, off, motifs, scale, scale_low, scale_hi)):
            outs[k][flts] = part
    return outs


# ----------------------------------------------------------------------------
# MotifSeq hit lists: up to K non-overlapping matches per read and motif -- and the three families that return the
# hit lists plus one more array (read background, alignment paths, events).  The four share everything below but
# their names and docstrings.
# ----------------------------------------------------------------------------
def _hits_args(motifs, max_hits, max_dist):
    max_hits, max_dist = int(max_hits), float(max_dist)
    if not 1 <= max_hits <= 64:
        raise ValueError("max_hits must be in 1..64, got %d" % max_hits)
    if max_dist != max_dist:
        raise ValueError("max_dist is NaN")
    return _flat_motifs(motifs) + (max_hits, max_dist)


class _Family:
    """What the calls of one family return per motif besides (hits[R, K], count[R]) -- `per`: "" nothing, "read" one
    record per read (in C [motif][read]), "point" `width` values per motif point (in C the blocks of _unpack_blocks) --
    with the array's dtype and the fill of a read no call reaches, and whether its calls make paths (the self-check
    counter of last_path_mismatches)."""

    def __init__(self, name, dtype=None, per="", width=1, fill=None, counts_paths=False):
        self.name, self.dtype, self.per, self.width = name, dtype, per, width
        self.fill, self.counts_paths = fill, counts_paths

    def shape(self, R, K, N):
        """of one motif's array: [R], [R, K, N] or [R, K, N, width]"""
        return (R,) if self.per == "read" else (R, K, N) + ((self.width,) if self.width > 1 else ())

    def flat(self, nmotifs, n, K, total):
        """elements of the C buffer of a shard of n reads (total: the motifs' points in all)"""
        return nmotifs * n if self.per == "read" else self.width * K * n * total


_HITS = _Family("hits")
_BACKGROUND = _Family("background", BG_DTYPE, "read", fill=lambda shape: np.zeros(shape, dtype=BG_DTYPE))
_PATHS = _Family("paths", np.int32, "point", 2, lambda shape: np.full(shape, -1, dtype=np.int32), True)
_EVENTS = _Family("events", EVENT_DTYPE, "point", 1, lambda shape: no_events(shape), True)
_path_lock = __import__("threading").Lock()
_path_mismatches = [-1]


def _unpack_blocks(buf, moff, K, n, width):
    """The per-motif arrays of the flat spans (width 2) or events (width 1) buffer of a call over n reads
    (include/squigglekit_hip.h): motif k's block begins at width * K * n * moff[k], inside it [read][hit][N_k][width]
    ([read][hit][N_k] for width 1)."""
    out = []
    for k in range(len(moff) - 1):
        N, b = int(moff[k + 1] - moff[k]), width * K * n * int(moff[k])
        out.append(buf[b:b + width * K * n * N].reshape((n, K, N) + ((width,) if width > 1 else ())))
    return out


def _hits_over(fam, devices, R, ms, moff, K, entry_call):
    """Runs entry_call(lo, hi, hits_part, count_part[, third_part]) over the devices (_over_devices: every shard writes
    its reads); returns per motif (hits[R, K], count[R]) plus the family's third array.  A family that makes paths
    resets the self-check counter and adds up its shards' (last_path_mismatches)."""
    L = _lib.load()
    hits = np.zeros((len(ms), R, K), dtype=HIT_DTYPE)
    count = np.zeros((len(ms), R), dtype=np.int32)
    third = [fam.fill(fam.shape(R, K, m.size)) for m in ms] if fam.per else None
    if fam.counts_paths:
        with _path_lock:
            _path_mismatches[0] = 0

    def call(lo, hi):
        n = hi - lo
        bufs = [np.zeros((len(ms), n, K), dtype=HIT_DTYPE), np.zeros((len(ms), n), dtype=np.int32)]
        if fam.per:
            bufs.append(np.zeros(fam.flat(len(ms), n, K, int(moff[-1])), dtype=fam.dtype))
        rc = entry_call(lo, hi, *bufs)
        if rc == 0:
            hits[:, lo:hi], count[:, lo:hi] = bufs[0], bufs[1]
            if fam.per:
                parts = bufs[2].reshape(len(ms), n) if fam.per == "read" else _unpack_blocks(bufs[2], moff, K, n, fam.width)
                for k in range(len(ms)):
                    third[k][lo:hi] = parts[k]
            if fam.counts_paths:
                bad = L.sk_last_path_mismatches()
                with _path_lock:
                    _path_mismatches[0] += max(bad, 0)
        return rc
    if R and ms:
        _over_devices(devices, R, call)
    return [(hits[k], count[k]) + ((third[k],) if fam.per else ()) for k in range(len(ms))]


def _hits_batch(fam, sig, lens, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices):
    """The packed int16 form of a family: rows of an int16 [R, stride] batch."""
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    R = sig.shape[0]
    if _too_wide_for_i16(scale_low, scale_hi):
        # limits wider than the int16 kernels' histogram: the float64 kernels (the same filter, the same statistics)
        flat, off = pack_f64([sig[r, :lens[r]] for r in range(R)])
        return globals()["motifseq_%s_ragged_f64" % fam.name](flat, off, motifs, max_hits, max_dist, scale, scale_low,
                                                              scale_hi, devices)
    entry = getattr(_lib.load(), "sk_motifseq_%s_i16" % fam.name)
    ms, flat, moff, K, md = _hits_args(motifs, max_hits, max_dist)

    def call(lo, hi, *bufs):
        return entry(ptr(sig[lo:hi]), sig.shape[1], ptr(lens[lo:hi]), hi - lo, ptr(flat), ptr(moff), len(ms),
                     _lib.SK_SCALE[scale], int(scale_low), int(scale_hi), K, md, *map(ptr, bufs))
    return _hits_over(fam, devices, R, ms, moff, K, call)


def _hits_ragged(fam, values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices):
    """The ragged form of a family: read r = values[off[r]:off[r+1]], float64 or int32 centi-units."""
    centi = isinstance(values, np.ndarray) and values.dtype == np.int32      # converted on the device (value / 100)
    values = np.ascontiguousarray(values, dtype=np.int32 if centi else np.float64)
    entry = getattr(_lib.load(), "sk_motifseq_%s_%s" % (fam.name, "centi" if centi else "f64"))
    off = np.ascontiguousarray(off, dtype=np.int64)
    ms, flat, moff, K, md = _hits_args(motifs, max_hits, max_dist)

    def call(lo, hi, *bufs):
        return entry(ptr(values), ptr(off[lo:hi + 1]), hi - lo, ptr(flat), ptr(moff), len(ms), _lib.SK_SCALE[scale],
                     int(scale_low), int(scale_hi), K, md, *map(ptr, bufs))
    return _hits_over(fam, devices, off.size - 1, ms, moff, K, call)


def _hits_mixed(fam, reads, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices):
    """The per-read form of a family: integer-valued reads through its packed int16 form, the rest through its ragged
    form (both looked up by name when called), merged in read order; the self-check counters of the two add up."""
    ms = _hits_args(motifs, max_hits, max_dist)[0]            # (argument errors before any GPU work)
    ints, arrs, flts = _split_int16(reads)
    R, K = len(reads), int(max_hits)
    res = [(np.zeros((R, K), dtype=HIT_DTYPE), np.zeros(R, dtype=np.int32))
           + ((fam.fill(fam.shape(R, K, m.size)),) if fam.per else ()) for m in ms]
    bad = 0
    for idx, route, pack in ((ints, "_batch", lambda: pack_i16(arrs)),
                             (flts, "_ragged_f64", lambda: pack_f64([reads[i] for i in flts]))):
        if idx and ms:
            got = globals()["motifseq_" + fam.name + route](*pack(), ms, K, max_dist, scale, scale_low, scale_hi, devices)
            for whole, part in zip(res, got):
                for a, b in zip(whole, part):
                    a[idx] = b
            bad += _path_mismatches[0]
    if fam.counts_paths:
        with _path_lock:
            _path_mismatches[0] = bad
    return res


def motifseq_hits_batch(sig, lens, motifs, max_hits=8, max_dist=float("inf"), scale="medmad", scale_low=0,
                        scale_hi=1200, devices=None):
    """Hit lists of every motif against every row of an int16 [R, stride] batch (one filter / statistics pass):
    a list, per motif, of (hits[R, max_hits] HIT_DTYPE, count[R]).  The block form of motifseq_hits."""
    return _hits_batch(_HITS, sig, lens, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_hits_ragged_f64(values, off, motifs, max_hits=8, max_dist=float("inf"), scale="medmad", scale_low=0,
                             scale_hi=1200, devices=None):
    """Hit lists of every motif against a ragged float64 batch (read r = values[off[r]:off[r+1]]; int32 values are
    centi-units, value / 100): per motif (hits[R, max_hits], count[R]).  The pA TSV / BLOW5-pA route."""
    return _hits_ragged(_HITS, values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_hits(reads, motifs, max_hits=8, max_dist=float("inf"), scale="medmad", scale_low=0, scale_hi=1200,
                  devices=None):
    """Up to max_hits non-overlapping matches of every motif in every read: a list, per motif, of
    (hits[nreads, max_hits] HIT_DTYPE, count[nreads]).  Rank 1 is motifseq_multi's record; the ranks after it take
    the next smallest distance whose [start, end] overlaps no earlier hit, up to max_dist.  Unused slots: dist NaN,
    start = end = -1.  Integer-valued reads go through the int16 kernels, the rest through the float64 ones."""
    return _hits_mixed(_HITS, reads, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


# ----------------------------------------------------------------------------
# MotifSeq read background: the hit list plus the statistics of each read's whole last row
# ----------------------------------------------------------------------------
MAD_SCALE = 1.4826                     # medmad's constant (MotifSeq.py:192-200)


def motifseq_background_batch(sig, lens, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                              scale_hi=1200, devices=None):
    """motifseq_hits_batch plus each read's own background: a list, per motif, of (hits[R, max_hits], count[R], bg[R]).
    bg (BG_DTYPE) describes d = cost[-1, :], the whole last DTW row of the motif against the read -- the row view_region
    draws a hit against (MotifSeq.py:507-513) -- bit for bit as numpy would: mean = np.mean(d), std = np.std(d),
    median = np.median(d), mad = np.median(np.abs(d - median)), below = the columns with d < mean - std, n = columns.
    Reads flagged empty or degenerate: NaN, below -1.  local_scores turns a hit's distance into scores against it."""
    return _hits_batch(_BACKGROUND, sig, lens, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_background_ragged_f64(values, off, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                                   scale_hi=1200, devices=None):
    """motifseq_hits_ragged_f64 plus the background records (see motifseq_background_batch); int32 values are
    centi-units."""
    return _hits_ragged(_BACKGROUND, values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_background(reads, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0, scale_hi=1200,
                        devices=None):
    """motifseq_hits plus each read's own background: a list, per motif, of
    (hits[nreads, max_hits], count[nreads], bg[nreads]) -- see motifseq_background_batch.  The same read kinds as
    motifseq_hits: integer-valued reads through the int16 kernels, the rest through the float64 ones."""
    return _hits_mixed(_BACKGROUND, reads, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def local_scores(dist, bg):
    """(local_Z, robust_Z) of hit distances against their reads' background records (arrays that broadcast against each
    other, e.g. hits["dist"] [R, K] and bg[:, None]): local_Z = (dist - mean) / std and robust_Z = (dist - median) /
    (mad * 1.4826), in numpy float64 on the host like MotifSeq's own scores.  std == 0 or mad == 0 give the IEEE result
    (inf or NaN)."""
    dist = np.asarray(dist, dtype=np.float64)
    with np.errstate(all="ignore"):
        local_z = (dist - bg["mean"]) / bg["std"]
        robust_z = (dist - bg["median"]) / (bg["mad"] * MAD_SCALE)
    return local_z, robust_z


# ----------------------------------------------------------------------------
# MotifSeq alignment paths: per hit, the samples each motif point covers
# ----------------------------------------------------------------------------
def motifseq_paths_batch(sig, lens, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                         scale_hi=1200, devices=None):
    """motifseq_hits_batch plus, per hit, the spans of its warping path: a list, per motif, of
    (hits[R, max_hits], count[R], spans[R, max_hits, N, 2]).  spans[r, h, i] = (a_i, b_i): the filtered samples motif
    point i covers in hit h of read r (expand_path turns them into mlpy's (px, py)); -1 where there is no path."""
    return _hits_batch(_PATHS, sig, lens, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_paths_ragged_f64(values, off, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                              scale_hi=1200, devices=None):
    """motifseq_hits_ragged_f64 plus the spans (see motifseq_paths_batch); int32 values are centi-units."""
    return _hits_ragged(_PATHS, values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_paths(reads, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0, scale_hi=1200,
                   devices=None):
    """motifseq_hits plus the alignment path of every hit: a list, per motif, of
    (hits[nreads, max_hits], count[nreads], spans[nreads, max_hits, N, 2])."""
    return _hits_mixed(_PATHS, reads, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def spans_of_path(px, py, n_points):
    """(a_i, b_i) per motif point of a warping path (px, py): the inverse of expand_path."""
    px, py = np.asarray(px), np.asarray(py)
    spans = np.full((int(n_points), 2), -1, dtype=np.int32)
    if px.size:
        first = np.flatnonzero(np.r_[True, px[1:] != px[:-1]])
        last = np.r_[first[1:] - 1, px.size - 1]
        spans[px[first], 0] = py[first]
        spans[px[first], 1] = py[last]
    return spans


def expand_path(spans):
    """mlpy's path (px, py) from the spans [N, 2] of one hit: (i, j) for j = a_i .. b_i, i ascending.
    A hit without a path (spans -1) gives two empty arrays."""
    spans = np.asarray(spans).reshape(-1, 2)
    if spans.size == 0 or spans[0, 0] < 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cnt = (spans[:, 1] - spans[:, 0] + 1).astype(np.int64)
    px = np.repeat(np.arange(spans.shape[0], dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    py = np.arange(cnt.sum(), dtype=np.int64) - np.repeat(first, cnt) + np.repeat(spans[:, 0].astype(np.int64), cnt)
    return px, py


def last_path_mismatches():
    """Hits of the last paths call of this module whose path failed the kernel's self-check (they carry spans -1);
    a healthy build reports 0.  -1: no paths call yet."""
    return _path_mismatches[0]


# ----------------------------------------------------------------------------
# MotifSeq events: per hit and motif point what the signal did; pooled models
# ----------------------------------------------------------------------------
def no_events(shape):
    """An EVENT_DTYPE array of hits without a path: sum = std = cost = NaN, start -1, dwell 0."""
    ev = np.zeros(shape, dtype=EVENT_DTYPE)
    ev["sum"] = ev["std"] = ev["cost"] = np.nan
    ev["start"] = -1
    return ev


def motifseq_events_batch(sig, lens, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                          scale_hi=1200, devices=None):
    """motifseq_hits_batch plus, per hit and motif point, what the signal did in the samples the path gives that point:
    a list, per motif, of (hits[R, max_hits], count[R], events[R, max_hits, N]).  With y the read's filtered, normalised
    samples and w = y[a_i : b_i + 1] (the span motifseq_paths_batch returns), events[r, h, i] (EVENT_DTYPE) holds
    sum = np.sum(w), std = np.std(w), cost = np.sum(np.abs(motif[i] - w)), start = a_i and dwell = b_i - a_i + 1, bit
    for bit as numpy would; sum / dwell is np.mean(w).  No path: NaN, start -1, dwell 0."""
    return _hits_batch(_EVENTS, sig, lens, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_events_ragged_f64(values, off, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0,
                               scale_hi=1200, devices=None):
    """motifseq_hits_ragged_f64 plus the events (see motifseq_events_batch); int32 values are centi-units."""
    return _hits_ragged(_EVENTS, values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def motifseq_events(reads, motifs, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0, scale_hi=1200,
                    devices=None):
    """motifseq_hits plus the events of every hit: a list, per motif, of
    (hits[nreads, max_hits], count[nreads], events[nreads, max_hits, N]) -- see motifseq_events_batch.  The same read
    kinds as motifseq_paths; spans_of_events gives the spans a paths call would have returned."""
    return _hits_mixed(_EVENTS, reads, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices)


def spans_of_events(events):
    """The spans [..., N, 2] int32 a paths call returns for the hits of `events` [..., N]: (start, start + dwell - 1),
    -1 where there is no path."""
    events = np.asarray(events)
    spans = np.empty(events.shape + (2,), dtype=np.int32)
    spans[..., 0] = events["start"]
    spans[..., 1] = events["start"] + events["dwell"] - 1
    spans[events["dwell"] <= 0] = -1
    return spans


def pool_events(events, use=None):
    """The model the hits of `events` show: POOL_DTYPE[N], one record per motif point, from events [..., N] (every
    leading axis is flattened into the hit order) and an optional boolean mask over the hits.  A hit without a path
    (dwell 0) is never used.  Over the selected records of point i: level = np.sum(sum) / total dwell (sample weighted:
    one update of DTW barycentre averaging), level_sd = np.std(sum / dwell), sd_mean = np.mean(std), dwell_mean, dwell_sd
    = np.std(dwell), cost_mean = np.mean(cost), hits -- bit for bit as numpy would; no hit: NaN.  Always one device (the
    calling thread's), so the reduction order does not depend on how the events call was sharded."""
    events = np.asarray(events)
    if events.dtype != EVENT_DTYPE or events.ndim < 1 or events.shape[-1] < 1:
        raise ValueError("events must be an EVENT_DTYPE array [..., N] with N >= 1")
    N = events.shape[-1]
    ev = np.ascontiguousarray(events).reshape(-1, N)
    H = ev.shape[0]
    mask = None
    if use is not None:
        mask = np.ascontiguousarray(np.asarray(use).reshape(-1) != 0).view(np.uint8)
        if mask.size != H:
            raise ValueError("use has %d entries for %d hits" % (mask.size, H))
    L = _lib.ensure_init()
    out = np.zeros(N, dtype=POOL_DTYPE)
    check(L.sk_events_pool(ptr(ev), None if mask is None else ptr(mask), H, N, ptr(out)))
    return out


def refine_motif(reads, motif, rounds=1, max_hits=1, max_dist=float("inf"), scale="medmad", scale_low=0, scale_hi=1200,
                 devices=None):
    """Corrects a motif from the data: `rounds` times -- motifseq_events of the current motif, pool_events of the hits
    with dist <= max_dist, then x_i = level_i (a point no hit covers keeps its value).  One round is one step of DTW
    barycentre averaging.  Returns the list of (motif_t, pool_t) per round: the motif after round t and the pool it was
    made from."""
    x = np.ascontiguousarray(motif, dtype=np.float64).copy()
    max_dist = float(max_dist)
    out = []
    for _ in range(int(rounds)):
        hits, _, events = motifseq_events(reads, [x], max_hits, float("inf"), scale, scale_low, scale_hi, devices)[0]
        pool = pool_events(events, hits["dist"] <= max_dist)
        x = np.where(pool["hits"] > 0, pool["level"], x)
        out.append((x.copy(), pool))
    return out


def normalise(sig, scale="medmad", scale_low=0, scale_hi=1200):
    """Filtered + normalised signal of one read, as MotifSeq hands it to
    dtw_subsequence (MotifSeq.py:274-289)."""
    L = _lib.ensure_init()
    n = C.c_int32(0)
    if is_int16_exact(sig):
        s = np.ascontiguousarray(np.asarray(sig).astype(np.int16))
        out = np.empty(max(1, s.size), dtype=np.float64)
        check(L.sk_normalise_i16(ptr(s), s.size, _lib.SK_SCALE[scale], int(scale_low), int(scale_hi),
                                 ptr(out), C.byref(n)))
    else:
        s = np.ascontiguousarray(sig, dtype=np.float64)
        out = np.empty(max(1, s.size), dtype=np.float64)
        check(L.sk_normalise_f64(ptr(s), s.size, _lib.SK_SCALE[scale], int(scale_low), int(scale_hi),
                                 ptr(out), C.byref(n)))
    return out[:n.value].copy()


class LastRowCost:
    """What MotifSeq reads from mlpy's cost matrix: only `cost[-1, :]`
    (MotifSeq.py:507-509).  The N x n matrix itself is never materialised."""

    def __init__(self, last_row, nrows):
        self._last = last_row
        self.shape = (nrows, last_row.size)

    def __getitem__(self, key):
        if isinstance(key, tuple):
            row = key[0]
            rest = key[1] if len(key) > 1 else slice(None)
        else:
            row, rest = key, slice(None)
        if row in (-1, self.shape[0] - 1):
            return self._last[rest]
        raise IndexError("only the last row of the DTW cost matrix is kept on this path")


def dtw_subsequence(x, y, last_row=False, full_path=False):
    """Drop-in for mlpy.dtw_subsequence(x, y) as MotifSeq.py:437-439 consumes it:
    returns (dist, cost, path) with path[1][0] == start and path[1][-1] == end.
    `cost` supports cost[-1, :] when last_row=True, else it is None.  full_path=True: `path` is mlpy's whole warping
    path (px, py), rebuilt from the spans the path kernel returns; the default keeps its two ends only."""
    L = _lib.ensure_init()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    dist, s, e = C.c_double(), C.c_int32(), C.c_int32()
    row = np.empty(y.size, dtype=np.float64) if last_row else None
    check(L.sk_dtw_subsequence(ptr(x), x.size, ptr(y), y.size, C.byref(dist), C.byref(s),
                               C.byref(e), ptr(row) if last_row else None))
    path = (np.array([0, x.size - 1]), np.array([s.value, e.value]))
    if full_path:
        spans = np.empty((x.size, 2), dtype=np.int32)
        d2, s2, e2 = C.c_double(), C.c_int32(), C.c_int32()
        check(L.sk_dtw_subsequence_path(ptr(x), x.size, ptr(y), y.size, C.byref(d2), C.byref(s2), C.byref(e2), ptr(spans)))
        with _path_lock:
            _path_mismatches[0] = max(L.sk_last_path_mismatches(), 0)
        path = expand_path(spans)
    return dist.value, (LastRowCost(row, x.size) if last_row else None), path


def dtw_subsequence_cref(x, y):
    """mlpy.dtw_subsequence(x, y) -> (dist, start, end) in the reference's own C arithmetic for inputs that hold inf / nan
    (medmad of a read whose MAD is 0): one GPU lane, full cost matrix (sk_dtw_subsequence_cref)."""
    L = _lib.ensure_init()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    dist, s, e = C.c_double(), C.c_int32(), C.c_int32()
    check(L.sk_dtw_subsequence_cref(ptr(x), x.size, ptr(y), y.size, C.byref(dist), C.byref(s), C.byref(e)))
    return dist.value, s.value, e.value


def dtw_subsequence_batch(x, ys):
    """dtw_subsequence(x, y) for a list of already-normalised float64 signals."""
    L = _lib.ensure_init()
    x = np.ascontiguousarray(x, dtype=np.float64)
    off = np.zeros(len(ys) + 1, dtype=np.int64)
    for i, y in enumerate(ys):
        off[i + 1] = off[i] + len(y)
    flat = (np.concatenate([np.asarray(y, dtype=np.float64) for y in ys])
            if len(ys) else np.zeros(0))
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    out = np.zeros(len(ys), dtype=HIT_DTYPE)
    check(L.sk_dtw_subsequence_batch(ptr(x), x.size, ptr(flat), ptr(off), len(ys), ptr(out)))
    return out


# ----------------------------------------------------------------------------
# DTW over a pair list: a query of its own per pair, shared targets, global mode ("DTW over a pair list" in
# include/squigglekit_hip.h and DESIGN.md 4.15)
# ----------------------------------------------------------------------------
PAIRS_MODES = {"subsequence": _lib.SK_PAIRS_SUBSEQUENCE, "global": _lib.SK_PAIRS_GLOBAL}
PAIR_DTYPE = np.dtype([("query", "<i4"), ("target", "<i4")])


def _as_pool(seqs):
    """(values float64, off int64 [nseq + 1]) of a list of arrays; a (values, off) tuple passes through."""
    if isinstance(seqs, tuple) and len(seqs) == 2:
        values = np.ascontiguousarray(seqs[0], dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(seqs[1], dtype=np.int64).reshape(-1)
        if off.size < 1 or np.any(np.diff(off) < 0) or off[0] < 0 or off[-1] > values.size:
            raise ValueError("off must hold nseq + 1 non-decreasing offsets into values")
        return values, off
    arrs = [np.asarray(s, dtype=np.float64).reshape(-1) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        off[1:] = np.cumsum([a.size for a in arrs])
    values = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0), dtype=np.float64)
    return values, off


def _as_pairs(pairs):
    if isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE:
        return np.ascontiguousarray(pairs).reshape(-1)
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("pair indices must fit int32")
    out = np.zeros(len(a), dtype=PAIR_DTYPE)
    out["query"], out["target"] = a[:, 0], a[:, 1]
    return out


def dtw_pairs(seqs, pairs, mode="subsequence"):
    """DTW of every (query, target) pair of a pool of already-normalised float64 sequences in one call: seqs a list of
    arrays or a (values, off) tuple, pairs [npairs, 2] indices into it.  Returns HIT_DTYPE [npairs] in the order of the
    list.  mode "subsequence": the record dtw_subsequence(seqs[q], seqs[t]) gives (n = the target's length); "global":
    both ends pinned (mlpy's dtw_std(x, y, dist_only=True)): dist = D[N-1][M-1], start = 0, end = M - 1.  A query holds
    1 .. 1 024 points; an empty target gives a NaN record flagged SK_FLAG_EMPTY.  Single device."""
    if mode not in PAIRS_MODES:
        raise ValueError("mode %r: need one of %s" % (mode, sorted(PAIRS_MODES)))
    L = _lib.ensure_init()
    values, off = _as_pool(seqs)
    pr = _as_pairs(pairs)
    out = np.zeros(len(pr), dtype=HIT_DTYPE)
    keep = values if values.size else np.zeros(1)
    check(L.sk_dtw_pairs(ptr(keep), ptr(off), off.size - 1, ptr(pr), len(pr), PAIRS_MODES[mode], ptr(out)))
    return out


def dtw_matrix(seqs, mode="global"):
    """All pairs of a pool: the float64 [nseq, nseq] distances.  mode "global": only i < j is computed, with the shorter
    of the two as the query (so the 1 024-point limit applies to the shorter one), then mirrored, diagonal 0.0 -- the
    global distance is symmetric bit for bit, the transposed path adds the same cells in the same order.  mode
    "subsequence": the full matrix, dists[i][j] = seqs[i] searched in seqs[j]."""
    values, off = _as_pool(seqs)
    n = off.size - 1
    lens = np.diff(off)
    if mode == "global":
        i, j = np.triu_indices(n, 1)
        swap = lens[j] < lens[i]
        pr = np.stack([np.where(swap, j, i), np.where(swap, i, j)], axis=1)
        rec = dtw_pairs((values, off), pr, "global")
        d = np.zeros((n, n), dtype=np.float64)
        d[i, j] = rec["dist"]
        d[j, i] = rec["dist"]
        return d
    i, j = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return dtw_pairs((values, off), np.stack([i, j], axis=1), mode)["dist"].reshape(n, n)


def map_queries(queries, targets, mode="subsequence"):
    """Every query against every target in one call.  Returns (records HIT_DTYPE [T, Q], best int64 [Q]): best[q] is the
    target with the smallest dist, ties to the smallest target index (-1 when no target gave a distance)."""
    qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in queries]
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in targets]
    Q, T = len(qs), len(ts)
    t, q = np.divmod(np.arange(T * Q, dtype=np.int64), max(Q, 1))
    rec = dtw_pairs(qs + ts, np.stack([q, Q + t], axis=1), mode).reshape(T, Q)
    return rec, best_targets(rec)


def best_targets(records):
    """best [Q] of records [T, Q]: the smallest dist, ties to the smallest target index; -1 where every dist is NaN."""
    nan = np.isnan(records["dist"])
    if nan.shape[0] == 0:
        return np.full(nan.shape[1], -1, dtype=np.int64)
    best = np.argmin(np.where(nan, np.inf, records["dist"]), axis=0).astype(np.int64)
    best[nan.all(axis=0)] = -1
    return best


def pair_span_off(off, pairs):
    """span_off int64 [npairs + 1] of a pair list: the spans of pair p are rows span_off[p] .. span_off[p + 1] -- the query
    lengths of the pairs before it, summed in list order (a query used by several pairs counts once per pair)."""
    off = np.asarray(off, dtype=np.int64)
    pr = _as_pairs(pairs)
    out = np.zeros(len(pr) + 1, dtype=np.int64)
    if len(pr):
        q = pr["query"].astype(np.int64)
        out[1:] = np.cumsum(off[q + 1] - off[q])
    return out


def dtw_pairs_paths(seqs, pairs, mode="subsequence", records=None):
    """dtw_pairs plus the warping path of every pair: (records HIT_DTYPE [npairs], span_off int64 [npairs + 1], spans int32
    [sum N, 2]).  Rows span_off[p] .. span_off[p + 1] are pair p's spans: query point i covers the target points
    spans[.., 0] .. spans[.., 1] (target coordinates; expand_path turns them into mlpy's (px, py)).  mode "subsequence":
    mlpy's subsequence_path; "global": mlpy's path() of dtw_std, row 0 covering [0, b_0].  records=None: the records are
    computed first (dtw_pairs' bytes) and returned; otherwise they are input and name the window [start, end] of each
    target to trace (merged records of a tiled search against the whole targets).  A pair without a distance has spans
    -1; so has a pair whose path fails the kernel's self-check, and last_path_mismatches() counts those."""
    if mode not in PAIRS_MODES:
        raise ValueError("mode %r: need one of %s" % (mode, sorted(PAIRS_MODES)))
    L = _lib.ensure_init()
    values, off = _as_pool(seqs)
    pr = _as_pairs(pairs)
    if len(pr) and (pr["query"].min() < 0 or pr["query"].max() >= off.size - 1):
        span_off = np.zeros(len(pr) + 1, dtype=np.int64)           # (the library names the pair and refuses)
    else:
        span_off = pair_span_off(off, pr)
    have = records is not None
    if have:
        rec = np.ascontiguousarray(records, dtype=HIT_DTYPE).reshape(-1).copy()
        if len(rec) != len(pr):
            raise ValueError("records: need one per pair")
    else:
        rec = np.zeros(len(pr), dtype=HIT_DTYPE)
    spans = np.full((int(span_off[-1]), 2), -1, dtype=np.int32)
    keep = values if values.size else np.zeros(1)
    keep_spans = spans if spans.size else np.zeros((1, 2), dtype=np.int32)
    check(L.sk_dtw_pairs_paths(ptr(keep), ptr(off), off.size - 1, ptr(pr), len(pr), PAIRS_MODES[mode],
                               ptr(rec if len(rec) else np.zeros(1, dtype=HIT_DTYPE)), int(have), ptr(keep_spans)))
    with _path_lock:
        _path_mismatches[0] = max(L.sk_last_path_mismatches(), 0) if len(pr) else 0
    return rec, span_off, spans


def last_pair_paths_tiers():
    """(listed, slab_bytes, waves) of the last dtw_pairs_paths / map_paths call of this thread's device: the pairs that
    did not fit the kernel's LDS tier, the bytes of one scratch slab (sized from those pairs), the wavefronts that
    shared them."""
    L = _lib.ensure_init()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    check(L.sk_last_pair_paths_tiers(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


# ----------------------------------------------------------------------------
# Adaptive-band DTW over a pair list: whole reads, records and paths in one pass ("Adaptive-band DTW over a pair list"
# in include/squigglekit_hip.h and DESIGN.md 4.17)
# ----------------------------------------------------------------------------
BAND_ENDS = {"pinned": _lib.SK_BAND_PINNED, "free": _lib.SK_BAND_FREE}
BAND_WIDTHS = (64, 128, 256)


def dtw_band(seqs, pairs, band=128, end="pinned", paths=True):
    """DTW of every (query, target) pair of a pool inside an adaptive band of `band` cells (64, 128 or 256) per
    anti-diagonal: the start pinned to (0, 0), the end pinned to (N-1, M-1) or, end="free", free along the last row.
    Returns (records HIT_DTYPE [npairs], span_off int64 [npairs + 1], spans int32 [sum N, 2]) with the layout of
    dtw_pairs_paths, or the records alone when paths=False.  Sequences hold up to 2^20 points.  While N and M are at most
    band / 2 the record is dtw_pairs(mode="global")'s bit for bit; beyond that dist is >= the full matrix's.  A pair whose
    band lost the end cell has dist +inf, start = end = -1, SK_FLAG_BAND_LOST and spans -1 and is counted by
    last_path_mismatches(); an empty target gives a NaN record flagged SK_FLAG_EMPTY.  Single device."""
    if end not in BAND_ENDS:
        raise ValueError("end %r: need one of %s" % (end, sorted(BAND_ENDS)))
    if band not in BAND_WIDTHS:
        raise ValueError("band %r: need one of %s" % (band, list(BAND_WIDTHS)))
    L = _lib.ensure_init()
    values, off = _as_pool(seqs)
    pr = _as_pairs(pairs)
    rec = np.zeros(len(pr), dtype=HIT_DTYPE)
    keep = values if values.size else np.zeros(1)
    keep_rec = rec if len(rec) else np.zeros(1, dtype=HIT_DTYPE)
    if not paths:
        check(L.sk_dtw_band(ptr(keep), ptr(off), off.size - 1, ptr(pr), len(pr), int(band), BAND_ENDS[end], ptr(keep_rec), None))
        return rec
    if len(pr) and (pr["query"].min() < 0 or pr["query"].max() >= off.size - 1):
        span_off = np.zeros(len(pr) + 1, dtype=np.int64)           # (the library names the pair and refuses)
    else:
        span_off = pair_span_off(off, pr)
    spans = np.full((int(span_off[-1]), 2), -1, dtype=np.int32)
    keep_spans = spans if spans.size else np.zeros((1, 2), dtype=np.int32)
    check(L.sk_dtw_band(ptr(keep), ptr(off), off.size - 1, ptr(pr), len(pr), int(band), BAND_ENDS[end], ptr(keep_rec),
                        ptr(keep_spans)))
    with _path_lock:
        _path_mismatches[0] = max(L.sk_last_path_mismatches(), 0) if len(pr) else 0
    return rec, span_off, spans


def align_reads(queries, targets, band=128, end="pinned"):
    """dtw_band of query i against target i: (records, span_off, spans)."""
    qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in queries]
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in targets]
    if len(qs) != len(ts):
        raise ValueError("align_reads: need one target per query")
    idx = np.arange(len(qs), dtype=np.int64)
    return dtw_band(qs + ts, np.stack([idx, len(qs) + idx], axis=1), band, end)


def last_band_plan():
    """(slab_bytes, waves, steps_max) of the last dtw_band / align_reads call of this thread's device: the bytes of one
    wavefront's slab of direction words and move bits (0 for a records-only call), the wavefronts of the launch, N + M - 1
    of the longest listed pair."""
    L = _lib.ensure_init()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    check(L.sk_last_band_plan(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def map_paths(queries, targets, records, which=None):
    """The warping path of every query in ONE of its targets: (span_off int64 [Q + 1], spans int32 [sum, 2]).  records
    [T, Q] come from map_queries, or from merge_tiles with the whole targets passed here; which [Q] names the target per
    query (default best_targets(records)).  A query whose target is -1 has no path: a zero-length entry in span_off."""
    qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in queries]
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in targets]
    records = np.asarray(records)
    Q = len(qs)
    if records.shape != (len(ts), Q):
        raise ValueError("records: need shape [T, Q] = (%d, %d)" % (len(ts), Q))
    which = best_targets(records) if which is None else np.asarray(which, dtype=np.int64).reshape(-1)
    if which.size != Q or np.any(which >= len(ts)):
        raise ValueError("which: need one target index per query")
    use = np.flatnonzero(which >= 0)
    span_off = np.zeros(Q + 1, dtype=np.int64)
    if use.size == 0:
        return span_off, np.zeros((0, 2), dtype=np.int32)
    pr = np.stack([use, Q + which[use]], axis=1)
    _, off_p, spans = dtw_pairs_paths(qs + ts, pr, "subsequence", records=records[which[use], use])
    span_off[use + 1] = np.diff(off_p)
    return np.cumsum(span_off), spans


def dtw_std(x, y, dist_only=True):
    """Drop-in for mlpy.dtw_std(x, y, dist_only): the global DTW of two already-normalised float64 sequences.  Returns
    dist, or with dist_only=False (dist, None, (px, py)): the cost matrix is never materialised, the path is mlpy's
    path() rebuilt from the spans of the pair-list path kernel.  x holds 1 .. 1 024 points."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if dist_only:
        return float(dtw_pairs([x, y], [(0, 1)], "global")["dist"][0])
    rec, _, spans = dtw_pairs_paths([x, y], [(0, 1)], "global")
    return float(rec["dist"][0]), None, expand_path(spans)


def tile_targets(targets, piece, overlap):
    """Long targets cut into pieces of `piece` points that step by piece - overlap, for map_queries: returns (pieces,
    tiling) with tiling = {"target": int64 [P], "origin": int64 [P], "length": int64 [T]} -- piece p is
    targets[target[p]][origin[p] : origin[p] + piece].  The last piece of a target ends at its end; a target of at most
    `piece` points is one piece.  merge_tiles puts the records back in whole-target coordinates."""
    piece, overlap = int(piece), int(overlap)
    if not 0 <= overlap < piece:
        raise ValueError("need 0 <= overlap < piece")
    step = piece - overlap
    pieces, tgt, org, length = [], [], [], []
    for t, y in enumerate(targets):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        length.append(y.size)
        s = 0
        while True:
            pieces.append(y[s:s + piece])
            tgt.append(t)
            org.append(s)
            if s + piece >= y.size:
                break
            s += step
    return pieces, {"target": np.array(tgt, dtype=np.int64), "origin": np.array(org, dtype=np.int64),
                    "length": np.array(length, dtype=np.int64)}


def merge_tiles(records, tiling):
    """records [P, Q] of the pieces of tile_targets (subsequence mode) -> records [T, Q] of the whole targets: start and
    end shifted by the piece's origin, n the whole target's length, per (query, target) the smallest dist, ties to the
    smallest end.  Guarantee: dist equals the whole-target dist whenever the whole-target match spans at most `overlap`
    points (some piece then holds the whole match, and no piece can do better than the whole target)."""
    records = np.asarray(records)
    tgt, org, length = tiling["target"], tiling["origin"], tiling["length"]
    T, Q = len(length), records.shape[1]
    out = np.zeros((T, Q), dtype=HIT_DTYPE)
    seen = np.zeros(T, dtype=bool)
    for p in range(records.shape[0]):
        t = int(tgt[p])
        r = records[p].copy()
        has = r["start"] >= 0
        r["start"][has] += int(org[p])
        r["end"][has] += int(org[p])
        r["n"] = int(length[t])
        if not seen[t]:
            out[t], seen[t] = r, True
            continue
        cur = out[t]
        better = (r["dist"] < cur["dist"]) | ((r["dist"] == cur["dist"]) & (r["end"] < cur["end"])) | \
                 (np.isnan(cur["dist"]) & ~np.isnan(r["dist"]))
        cur[better] = r[better]
    return out


# ----------------------------------------------------------------------------
# Hit lists over a pair list: up to K non-overlapping loci per pair ("Hit lists over a pair list" in
# include/squigglekit_hip.h and DESIGN.md 4.21)
# ----------------------------------------------------------------------------
def _hit_limits(max_hits, max_dist):
    K, md = int(max_hits), float(max_dist)
    if not 1 <= K <= 64:
        raise ValueError("max_hits must be in 1 .. 64, got %d" % K)
    if md != md:
        raise ValueError("max_dist is NaN")
    return K, md


def dtw_pairs_hits(seqs, pairs, max_hits=8, max_dist=np.inf):
    """Up to max_hits non-overlapping loci of every (query, target) pair of a pool (subsequence mode): (hits HIT_DTYPE
    [npairs, K], count int32 [npairs]).  From the last row d_j = D[N-1][j] and the back-trace starts s_j, K rounds take the
    smallest admissible d_j (ties: the smallest j); a column is admissible if d_j <= max_dist and [s_j, j] is disjoint
    from every interval taken before.  hits[p, k] for k < count[p] is (dist, start = s_j, end = j, n = M, flags); the
    rest hold dist NaN, start = end = -1.  With max_dist = inf hits[:, 0] is dtw_pairs' record byte for byte.  Single
    device."""
    K, md = _hit_limits(max_hits, max_dist)
    L = _lib.ensure_init()
    values, off = _as_pool(seqs)
    pr = _as_pairs(pairs)
    hits = np.zeros((len(pr), K), dtype=HIT_DTYPE)
    count = np.zeros(len(pr), dtype=np.int32)
    keep = values if values.size else np.zeros(1)
    keep_hits = hits if hits.size else np.zeros(1, dtype=HIT_DTYPE)
    keep_count = count if count.size else np.zeros(1, dtype=np.int32)
    check(L.sk_dtw_pairs_hits(ptr(keep), ptr(off), off.size - 1, ptr(pr), len(pr), K, md, ptr(keep_hits), ptr(keep_count)))
    return hits, count


def map_queries_hits(queries, targets, max_hits=8, max_dist=np.inf):
    """Every query against every target, up to max_hits loci each: (hits HIT_DTYPE [T, Q, K], count int32 [T, Q]);
    hits[:, :, 0] are map_queries' records when max_dist is inf."""
    qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in queries]
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in targets]
    Q, T = len(qs), len(ts)
    t, q = np.divmod(np.arange(T * Q, dtype=np.int64), max(Q, 1))
    hits, count = dtw_pairs_hits(qs + ts, np.stack([q, Q + t], axis=1), max_hits, max_dist)
    return hits.reshape(T, Q, -1), count.reshape(T, Q)


def last_pair_hits_plan():
    """The last dtw_pairs_hits / map_queries_hits / MapStream.hits call of this thread's device: {"row_bytes": bytes of
    last rows selected from at a time, "slices": slices of the pair list (1 for a session), "long_rows": rows of more than
    4 096 columns (a workgroup each; the others take a wavefront each)}."""
    L = _lib.ensure_init()
    v = [C.c_int64(0) for _ in range(3)]
    check(L.sk_last_pair_hits_plan(*[C.byref(x) for x in v]))
    return {"row_bytes": v[0].value, "slices": v[1].value, "long_rows": v[2].value}


def merge_tile_hits(hits, count, tiling, max_hits):
    """Hit lists [P, Q, K] / counts [P, Q] of the pieces of tile_targets -> (hits [T, Q, max_hits], count [T, Q]) in
    whole-target coordinates.  Per (target, query): the pieces' hits are pooled, shifted by their piece's origin, ordered
    by (dist, end, start) and taken greedily while disjoint from those taken -- a locus two overlapping pieces both
    report is kept once.  Hit 1 equals merge_tiles' record.  Host only."""
    hits, count = np.asarray(hits), np.asarray(count)
    K = _hit_limits(max_hits, 0.0)[0]
    tgt, org, length = tiling["target"], tiling["origin"], tiling["length"]
    T, Q = len(length), hits.shape[1]
    out = np.zeros((T, Q, K), dtype=HIT_DTYPE)
    out["dist"], out["start"], out["end"] = np.nan, -1, -1
    cnt = np.zeros((T, Q), dtype=np.int32)
    for t in range(T):
        ps = np.flatnonzero(tgt == t)
        out["n"][t] = int(length[t])
        for q in range(Q):
            if ps.size:
                out["flags"][t, q] = hits["flags"][ps[0], q, 0]
            pool = []
            for p in ps:
                for k in range(int(count[p, q])):
                    h = hits[p, q, k]
                    pool.append((float(h["dist"]), int(h["end"]) + int(org[p]), int(h["start"]) + int(org[p]), int(h["flags"])))
            pool.sort(key=lambda c: c[:3])
            taken = []
            for d, e, s, fl in pool:
                if len(taken) == K:
                    break
                if all(e < s0 or s > e0 for s0, e0 in taken):
                    out[t, q, len(taken)] = (d, s, e, int(length[t]), fl)
                    taken.append((s, e))
            cnt[t, q] = len(taken)
    return out, cnt


def locus_margin(hits, count):
    """Over ALL listed loci of all targets (hits [T, Q, K], count [T, Q]): (best_target int64 [Q], best_hit HIT_DTYPE [Q],
    second_dist float64 [Q]).  The best locus has the smallest dist, ties to the smallest target, then to the smallest
    end; second_dist is the smallest dist of any OTHER listed locus -- hit 2 of the best target or any hit of another
    target -- and +inf when there is none.  A query without a locus: best_target -1, a NaN record.  Host only."""
    hits, count = np.asarray(hits), np.asarray(count)
    T, Q = count.shape
    best = np.full(Q, -1, dtype=np.int64)
    rec = np.zeros(Q, dtype=HIT_DTYPE)
    rec["dist"], rec["start"], rec["end"] = np.nan, -1, -1
    second = np.full(Q, np.inf)
    if T == 0 or Q == 0:
        return best, rec, second
    K = hits.shape[2]
    first = np.where(count > 0, hits["dist"][:, :, 0], np.inf)          # a list is ordered by (dist, end): its hit 1 leads
    bt = np.argmin(first, axis=0)
    col = np.arange(Q)
    has = count[bt, col] > 0
    best[has] = bt[has]
    rec[has] = hits[bt, col, 0][has]
    rest = first.copy()
    rest[bt, col] = np.inf
    if K > 1:
        rest[bt, col] = np.where(count[bt, col] > 1, hits["dist"][bt, col, 1], np.inf)
    second[has] = rest.min(axis=0)[has]
    return best, rec, second


# ----------------------------------------------------------------------------
# MotifSeq panel: many motifs ranked per read, inside a search region
# ----------------------------------------------------------------------------
INT32_MAX = 2 ** 31 - 1


def resolve_region(lens, begin, end):
    """Per read the (start, stop) that slice(begin, end).indices(len) gives (pure numpy; end None: to the end of the
    read): negative values count from the end, everything is cut to the read, stop < start is an empty slice."""
    n = np.asarray(lens, dtype=np.int64)

    def side(v):
        if v is None:
            return n.copy()
        v = int(v)
        return np.clip(n + v, 0, None) if v < 0 else np.minimum(n, v)
    lo = np.zeros_like(n) if begin is None else side(begin)
    return np.stack([lo, side(end)], axis=-1)


def _region_pair(region):
    begin, end = (0, None) if region is None else region
    begin = 0 if begin is None else int(begin)
    end = INT32_MAX if end is None else int(end)
    if not (-2 ** 31 <= begin <= INT32_MAX and -2 ** 31 <= end <= INT32_MAX):
        raise ValueError("region bounds must fit int32")
    return begin, end


def _panel_args(motifs, means, sds, win, R):
    ms = [np.ascontiguousarray(m, dtype=np.float64) for m in motifs]
    if not 1 <= len(ms) <= 256:
        raise ValueError("a panel takes 1..256 motifs, got %d" % len(ms))
    flat = np.ascontiguousarray(np.concatenate(ms))
    moff = np.concatenate([[0], np.cumsum([m.size for m in ms])]).astype(np.int32)
    means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1)
    sds = np.ascontiguousarray(sds, dtype=np.float64).reshape(-1)
    if means.size != len(ms) or sds.size != len(ms):
        raise ValueError("means / sds need one entry per motif")
    if win is not None:
        win = np.ascontiguousarray(win, dtype=np.int32)
        if win.shape != (R, 2):
            raise ValueError("win must be [reads, 2]")
    return ms, flat, moff, means, sds, win


def _panel_result(out, frm, allrec, records):
    return (out, frm, [allrec[k] for k in range(allrec.shape[0])]) if records else (out, frm)


def motifseq_panel_batch(sig, lens, motifs, means, sds, region=(0, None), win=None, scale="medmad", scale_low=0,
                         scale_hi=1200, records=False, devices=None):
    """The panel over an int16 [R, stride] batch: per read the slice raw[begin:end] (region; or the read's own win row)
    is cut before scale_outliers, every motif is searched in it, and score[k] = (dist_k - means[k]) / sds[k] is
    ranked on the GPU.  Returns (panel[R] PANEL_DTYPE, from[R]) -- from: the raw index the slice starts at -- and with
    records=True also the list, per motif, of HIT_DTYPE records (what motifseq_multi_batch gives for the sliced rows)."""
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    begin, end = _region_pair(region)
    ms, flat, moff, means, sds, win = _panel_args(motifs, means, sds, win, R)
    if _too_wide_for_i16(scale_low, scale_hi):
        vals, off = pack_f64([sig[r, :lens[r]] for r in range(R)])
        return motifseq_panel_ragged_f64(vals, off, motifs, means, sds, region, win, scale, scale_low, scale_hi, records,
                                         devices)
    L = _lib.load()
    out = np.zeros(R, dtype=PANEL_DTYPE)
    frm = np.zeros(R, dtype=np.int32)
    allrec = np.zeros((len(ms), R), dtype=HIT_DTYPE)

    def call(lo, hi):
        part = np.zeros((len(ms), hi - lo), dtype=HIT_DTYPE)
        rc = L.sk_motifseq_panel_i16(ptr(sig[lo:hi]), stride, ptr(lens[lo:hi]), hi - lo, begin, end,
                                     None if win is None else ptr(win[lo:hi]), ptr(flat), ptr(moff), len(ms), ptr(means),
                                     ptr(sds), _lib.SK_SCALE[scale], int(scale_low), int(scale_hi), ptr(out[lo:hi]),
                                     ptr(frm[lo:hi]), ptr(part) if records else None)
        if rc == 0:
            allrec[:, lo:hi] = part
        return rc
    if R:
        _over_devices(devices, R, call)
    return _panel_result(out, frm, allrec, records)


def motifseq_panel_ragged_f64(values, off, motifs, means, sds, region=(0, None), win=None, scale="medmad", scale_low=0,
                              scale_hi=1200, records=False, devices=None):
    """motifseq_panel_batch for a ragged float64 batch (read r = values[off[r]:off[r+1]]): the pA route."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = off.size - 1
    begin, end = _region_pair(region)
    ms, flat, moff, means, sds, win = _panel_args(motifs, means, sds, win, R)
    L = _lib.load()
    out = np.zeros(R, dtype=PANEL_DTYPE)
    frm = np.zeros(R, dtype=np.int32)
    allrec = np.zeros((len(ms), R), dtype=HIT_DTYPE)

    def call(lo, hi):
        part = np.zeros((len(ms), hi - lo), dtype=HIT_DTYPE)
        rc = L.sk_motifseq_panel_f64(ptr(values), ptr(off[lo:hi + 1]), hi - lo, begin, end,
                                     None if win is None else ptr(win[lo:hi]), ptr(flat), ptr(moff), len(ms), ptr(means),
                                     ptr(sds), _lib.SK_SCALE[scale], int(scale_low), int(scale_hi), ptr(out[lo:hi]),
                                     ptr(frm[lo:hi]), ptr(part) if records else None)
        if rc == 0:
            allrec[:, lo:hi] = part
        return rc
    if R:
        _over_devices(devices, R, call)
    return _panel_result(out, frm, allrec, records)


def motifseq_panel(reads, motifs, means, sds, region=(0, None), win=None, scale="medmad", scale_low=0, scale_hi=1200,
                   records=False, devices=None):
    """The panel over a list of reads: integer-valued reads go through the int16 kernels, the rest through the float64
    ones (the same records either way); input order is kept.  See motifseq_panel_batch."""
    R = len(reads)
    ms, _, _, means, sds, win = _panel_args(motifs, means, sds, win, R)
    out = np.zeros(R, dtype=PANEL_DTYPE)
    frm = np.zeros(R, dtype=np.int32)
    allrec = np.zeros((len(ms), R), dtype=HIT_DTYPE)
    ints, arrs, flts = _split_int16(reads)
    for idx, run in ((ints, lambda w: motifseq_panel_batch(*pack_i16(arrs), ms, means, sds, region, w, scale, scale_low,
                                                           scale_hi, True, devices)),
                     (flts, lambda w: motifseq_panel_ragged_f64(*pack_f64([reads[i] for i in flts]), ms, means, sds, region,
                                                                w, scale, scale_low, scale_hi, True, devices))):
        if idx:
            o, f, a = run(None if win is None else win[idx])
            out[idx], frm[idx] = o, f
            for k in range(len(ms)):
                allrec[k][idx] = a[k]
    return _panel_result(out, frm, allrec, records)


def region_rows(sig, lens, region=(0, None), win=None):
    """The window rows alone (k_region_rows): (rows int16 [R, wstride] zero padded, wlen[R], from[R]) of an int16
    [R, stride] batch -- what the hit-list and path calls take when they search a region."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    begin, end = _region_pair(region)
    if win is not None:
        win = np.ascontiguousarray(win, dtype=np.int32)
        se = np.stack([np.array(slice(int(a), int(b)).indices(int(n))[:2]) for (a, b), n in zip(win, lens)]) if R else \
            np.zeros((0, 2), dtype=np.int64)
    else:
        se = resolve_region(lens, begin, None if end == INT32_MAX else end)
    longest = int(np.clip(se[:, 1] - se[:, 0], 0, None).max()) if R else 0
    wstride = max(8, (longest + 7) // 8 * 8)
    rows = np.zeros((R, wstride), dtype=np.int16)
    wlen = np.zeros(R, dtype=np.int32)
    frm = np.zeros(R, dtype=np.int32)
    if R:
        check(L.sk_region_rows_i16(ptr(sig), stride, ptr(lens), R, begin, end, None if win is None else ptr(win), wstride,
                                   ptr(rows), ptr(wlen), ptr(frm)))
    return rows, wlen, frm


# ----------------------------------------------------------------------------
# event detection: a read cut into its own sequence of levels (the definition: "event detection" in
# include/squigglekit_hip.h and DESIGN.md)
# ----------------------------------------------------------------------------
DET_PRESETS = {"dna": dict(w_short=3, w_long=6, th_short=1.4, th_long=9.0, peak_height=0.2),
               "rna": dict(w_short=7, w_long=14, th_short=2.5, th_long=9.0, peak_height=1.0)}


def det_params(preset="dna", **overrides):
    """The sk_det_params of a named preset ("dna" or "rna") with single fields replaced: det_params("rna", th_long=8.0)."""
    if preset not in DET_PRESETS:
        raise ValueError("preset %r: need one of %s" % (preset, sorted(DET_PRESETS)))
    kw = dict(DET_PRESETS[preset])
    for k, v in overrides.items():
        if k not in kw:
            raise TypeError("det_params: no field %r (fields: %s)" % (k, ", ".join(kw)))
        kw[k] = v
    return DetParams(int(kw["w_short"]), int(kw["w_long"]), float(kw["th_short"]), float(kw["th_long"]),
                     float(kw["peak_height"]))


def detect_events_batch(sig, lens=None, params=None):
    """Event detection for every row of an int16 [R, stride] batch of RAW samples (no outlier filter, no cut; raw
    coordinates).  Returns (off int64 [R + 1], rec DET_EVENT_DTYPE [off[R]]): read r's events are rec[off[r]:off[r + 1]],
    each with start, length and the exact sum and sum of squares of its samples.  The room for the records is a first
    guess (one event per eight samples); a batch that needs more is counted by that call and runs again with the count.
    Single device (the calling thread's): the ragged output is not sharded over `devices`."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    if lens.shape != (R,):
        raise ValueError("lens must hold one length per row")
    params = params or det_params()
    off = np.zeros(R + 1, dtype=np.int64)
    if R == 0 or stride == 0:
        return off, np.zeros(0, dtype=DET_EVENT_DTYPE)
    cap = int(np.clip(lens, 0, stride).sum()) // 8 + R
    while True:
        rec = np.zeros(cap, dtype=DET_EVENT_DTYPE)
        rc = L.sk_detect_events_i16(ptr(sig), stride, ptr(lens), R, C.byref(params), ptr(off), ptr(rec), cap)
        if rc == _lib.SK_ERR_OVERFLOW and int(off[R]) > cap:
            cap = int(off[R])
            continue
        check(rc)
        return off, rec[:int(off[R])]


def detect_events(reads, params=None):
    """detect_events_batch for a list of reads of any lengths.  Every read must hold int16-exact values: the detector runs
    on the raw samples, and as its statistic does not change under the affine pA calibration, pA users detect on the raw
    samples too (event_levels maps the levels to pA).  A float read that is not int16-exact raises ValueError."""
    arrs = []
    for i, r in enumerate(reads):
        b = as_int16_exact(r)
        if b is None:
            raise ValueError("read %d is not int16-exact: event detection takes raw samples (detect on the raw read; "
                             "event_levels(off, rec, calib) gives the levels in pA)" % i)
        arrs.append(np.asarray(b).reshape(-1))
    buf, lens = pack_i16(arrs)
    return detect_events_batch(buf, lens, params)


def event_levels(off, rec, calib=None):
    """(values float64, off): the level of every event, sum / length, as the ragged rows motifseq_multi_ragged_f64,
    motifseq_hits_ragged_f64 and dtw_subsequence_batch (after a split at off) take.  calib [R, 3] = digitisation, offset,
    range per read: the levels in pA, by pa_values' expression."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    rec = np.asarray(rec)
    values = rec["sum"].astype(np.float64) / rec["length"].astype(np.float64)
    if calib is not None:
        calib = np.asarray(calib, dtype=np.float64).reshape(-1, 3)
        if len(calib) != off.size - 1:
            raise ValueError("calib must hold one (digitisation, offset, range) per read")
        unit = np.array([float("{0:.2f}".format(rng)) / dig for dig, _, rng in calib], dtype=np.float64)
        per = np.diff(off)
        values = np.round((values + np.repeat(calib[:, 1], per)) * np.repeat(unit, per), 2)
    return values, off


def event_stdv(rec):
    """The standard deviation of every event's samples (ddof 0) from its exact integers:
    sqrt(max(length * sumsq - sum * sum, 0)) / length in float64."""
    rec = np.asarray(rec)
    n = rec["length"].astype(np.int64)
    var = np.maximum(n * rec["sumsq"] - rec["sum"] * rec["sum"], 0)
    return np.sqrt(var.astype(np.float64)) / n.astype(np.float64)


# ----------------------------------------------------------------------------
# signal HMM: every sample of a read assigned to a named stretch by the best path through a small model (the
# definition: "signal HMM" in include/squigglekit_hip.h and DESIGN.md 4.12)
# ----------------------------------------------------------------------------
def _log0(p):
    """log(p), -inf for p == 0"""
    p = float(p)
    if not p >= 0.0:
        raise ValueError("a probability or weight must be >= 0, got %r" % p)
    return float(np.log(p)) if p > 0.0 else float("-inf")


def hmm_model(init, trans, emissions):
    """The sk_hmm_model of probabilities: init [S], trans [S][S] (from, to) -- a zero becomes -inf -- and per state one
    or two emission components, each (weight, mean, sigma) for a Gaussian, c = log(weight) - log(sigma * sqrt(2 pi)),
    h = 1 / (2 sigma^2), or (weight, None, range) for a flat one, c = log(weight / range), h = 0.  An absent second
    component has c = -inf.  Nothing is normalised: the numbers are used as given."""
    S = len(init)
    if not 1 <= S <= _lib.SK_HMM_STATES or len(trans) != S or any(len(row) != S for row in trans) or len(emissions) != S:
        raise ValueError("need 1 <= S <= %d states, trans [S][S] and S emission lists" % _lib.SK_HMM_STATES)
    c = np.full((S, 2), -np.inf)
    mu = np.zeros((S, 2))
    h = np.zeros((S, 2))
    for j, comps in enumerate(emissions):
        if not 1 <= len(comps) <= 2:
            raise ValueError("state %d: one or two emission components" % j)
        for q, (weight, mean, width) in enumerate(comps):
            width = float(width)
            if not (width > 0.0 and np.isfinite(width)):
                raise ValueError("state %d: sigma / range must be positive and finite" % j)
            if mean is None:
                c[j, q] = _log0(float(weight) / width)
            else:
                c[j, q] = _log0(weight) - float(np.log(width * np.sqrt(2.0 * np.pi)))
                mu[j, q] = float(mean)
                h[j, q] = 1.0 / (2.0 * width * width)
    return HmmModel.from_arrays(S, [_log0(p) for p in init], [[_log0(p) for p in row] for row in trans], c, mu, h)


def _hmm_cal(cal2, R):
    if cal2 is None:
        return None
    cal2 = np.ascontiguousarray(cal2, dtype=np.float64)
    if cal2.shape != (R, 2):
        raise ValueError("cal2 must hold one (offset, unit) pair per read")
    return cal2


def hmm_viterbi_batch(sig, lens, model, cal2=None, limit=0):
    """The Viterbi record (HMM_DTYPE: score, final_state, n_used, enter[6]) of every row of an int16 [R, stride] batch of
    raw samples.  cal2 [R, 2] = (offset, unit) per read: the model sees (raw + offset) * unit, i.e. pA with unit =
    range / digitisation; None: it sees the raw values.  limit > 0: only the first min(len, limit) samples of a read.
    Single device (the calling thread's)."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    if lens.shape != (R,):
        raise ValueError("lens must hold one length per row")
    cal2 = _hmm_cal(cal2, R)
    rec = np.zeros(R, dtype=HMM_DTYPE)
    if R == 0 or stride == 0:                            # no samples at all: the record of an empty read
        rec["final_state"], rec["enter"] = -1, -1
        return rec
    check(L.sk_hmm_viterbi_i16(ptr(sig), stride, ptr(lens), R, None if cal2 is None else ptr(cal2), C.byref(model), int(limit),
                               ptr(rec)))
    return rec


def hmm_viterbi_ragged_f64(values, off, model, limit=0):
    """hmm_viterbi_batch for ragged float64 reads (pA values as a SquigglePull TSV holds them): read r is
    values[off[r]:off[r + 1]] and the model sees the values as they are."""
    L = _lib.ensure_init()
    values = np.ascontiguousarray(values, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = off.size - 1
    rec = np.zeros(max(R, 0), dtype=HMM_DTYPE)
    if values.size == 0:
        values = np.zeros(1)
    check(L.sk_hmm_viterbi_f64_len(ptr(values), ptr(off), R, C.byref(model), int(limit), ptr(rec)))
    return rec


def hmm_viterbi(reads, model, limit=0):
    """The records of a list of reads of any lengths: integer-valued reads go through the int16 feed, the rest through the
    float64 one (the same records either way); input order is kept."""
    rec = np.zeros(len(reads), dtype=HMM_DTYPE)
    ints, arrs, flts = _split_int16(reads)
    if ints:
        rec[ints] = hmm_viterbi_batch(*pack_i16([np.asarray(a).reshape(-1) for a in arrs]), model, None, limit)
    if flts:
        rec[flts] = hmm_viterbi_ragged_f64(*pack_f64([reads[i] for i in flts]), model, limit)
    return rec


# the poly(A) layer: a left-to-right model of a direct-RNA read
POLYA_STATES = ("START", "LEADER", "ADAPTER", "POLYA", "CLIFF", "TRANSCRIPT")
START, LEADER, ADAPTER, POLYA, CLIFF, TRANSCRIPT = range(6)
# Per preset: the emission components of the six states, (weight, mean, sigma) or (weight, None, range).
#   synth_raw  raw units, what synth.drna_reads plants: adapter N(430, 25), poly(A) N(560, 8), a body of event levels
#              N(530, 80) with plateaus near 535; the flat components take the spikes and the excursions it adds.
#   rna_pa     pA.  These numbers are this project's own choice, read off published direct-RNA (SQK-RNA002) traces -- open
#              pore well above 150 pA, leader near 105 pA, adapter near 80 pA, a tight poly(A) plateau near 108 pA, a
#              body spread around 95 pA -- and not fitted to data: treat them as a starting point and check them against
#              the reads at hand.
POLYA_PRESETS = {
    "synth_raw": {
        "emissions": [[(1.0, 900.0, 120.0)],
                      [(1.0, 500.0, 150.0)],
                      [(0.98, 430.0, 25.0), (0.02, None, 2400.0)],
                      [(0.98, 560.0, 8.0), (0.02, None, 2400.0)],
                      [(1.0, 480.0, 40.0)],
                      [(0.3, 535.0, 15.0), (0.7, 530.0, 90.0)]],
        "stay": (0.9, 0.9, 0.9995, 0.999, 0.3, 1.0), "cliff": 0.0001},
    "rna_pa": {
        "emissions": [[(1.0, 220.0, 40.0)],
                      [(1.0, 105.0, 12.0)],
                      [(0.98, 80.0, 6.0), (0.02, None, 300.0)],
                      [(0.98, 108.0, 2.5), (0.02, None, 300.0)],
                      [(1.0, 85.0, 8.0)],
                      [(0.4, 100.0, 8.0), (0.6, 95.0, 18.0)]],
        "stay": (0.9, 0.99, 0.9995, 0.999, 0.3, 1.0), "cliff": 0.0001},
}


def polya_spec(preset="rna_pa"):
    """The description (init, trans, emissions) of polya_model(preset), as hmm_model takes it and hmm_refit changes it:
    polya_model(preset) is hmm_model(*polya_spec(preset))."""
    if preset not in POLYA_PRESETS:
        raise ValueError("preset %r: need one of %s" % (preset, sorted(POLYA_PRESETS)))
    p = POLYA_PRESETS[preset]
    stay, cliff = p["stay"], p["cliff"]
    T = [[0.0] * 6 for _ in range(6)]
    T[START][START], T[START][LEADER] = stay[START], 1.0 - stay[START]
    T[LEADER][LEADER], T[LEADER][ADAPTER] = stay[LEADER], 1.0 - stay[LEADER]
    T[ADAPTER][ADAPTER], T[ADAPTER][POLYA] = stay[ADAPTER], 1.0 - stay[ADAPTER]
    T[POLYA][POLYA], T[POLYA][CLIFF], T[POLYA][TRANSCRIPT] = stay[POLYA], cliff, 1.0 - stay[POLYA] - cliff
    T[CLIFF][CLIFF], T[CLIFF][POLYA] = stay[CLIFF], 1.0 - stay[CLIFF]
    T[TRANSCRIPT][TRANSCRIPT] = 1.0
    return [0.5, 0.5, 0.0, 0.0, 0.0, 0.0], T, [[tuple(comp) for comp in comps] for comps in p["emissions"]]


def polya_model(preset="rna_pa"):
    """The six-state model START, LEADER, ADAPTER, POLYA, CLIFF, TRANSCRIPT of a direct-RNA read.  Transitions: S -> S, L;
    L -> L, A; A -> A, P; P -> P, C, T; C -> C, P; T -> T; every other one is impossible, and a read starts in START or
    LEADER.  POLYA is one tight Gaussian plus a flat component, TRANSCRIPT a mixture of two Gaussians.  Presets:
    "rna_pa" (pA; the values are this project's own choice, see POLYA_PRESETS) and "synth_raw" (raw units, matching
    synth.drna_reads)."""
    return hmm_model(*polya_spec(preset))


POLYA_DTYPE = np.dtype([("adapter_start", "<i4"), ("adapter_end", "<i4"), ("polya_start", "<i4"), ("polya_end", "<i4"),
                        ("polya_samples", "<i4"), ("found", "?")])


def polya_segments(records):
    """Where the adapter and the poly(A) tail lie, from the records of a polya_model (POLYA_DTYPE per read): adapter =
    [adapter_start, adapter_end], poly(A) = [polya_start, polya_end] in samples, both ends included: adapter_start =
    enter[ADAPTER], adapter_end = enter[POLYA] - 1, polya_start = enter[POLYA], polya_end = enter[TRANSCRIPT] - 1,
    polya_samples = polya_end - polya_start + 1 (cliffs inside the tail count).  found: the best path ends in TRANSCRIPT
    and went through POLYA; every coordinate of a read that is not found is -1 and polya_samples 0."""
    records = np.asarray(records)
    en = records["enter"].reshape(-1, 6)
    out = np.zeros(en.shape[0], dtype=POLYA_DTYPE)
    found = (records["final_state"].reshape(-1) == TRANSCRIPT) & (en[:, POLYA] >= 0) & (en[:, TRANSCRIPT] >= 0)
    out["found"] = found
    out["adapter_start"] = np.where(found, en[:, ADAPTER], -1)
    out["adapter_end"] = np.where(found, en[:, POLYA] - 1, -1)
    out["polya_start"] = np.where(found, en[:, POLYA], -1)
    out["polya_end"] = np.where(found, en[:, TRANSCRIPT] - 1, -1)
    out["polya_samples"] = np.where(found, en[:, TRANSCRIPT] - en[:, POLYA], 0)
    return out


# ----------------------------------------------------------------------------
# signal HMM state paths: the best path as run-length segments with exact statistics, pooled counts, and one-call
# re-estimation of a model from them (the definition: "signal HMM: state paths" in include/squigglekit_hip.h)
# ----------------------------------------------------------------------------
def _segments_call(call, R, dtype, cap):
    """rec, off, seg of one C call; the room for the segments is a first guess, a batch that needs more is counted by
    that call and runs again with the count"""
    rec = np.zeros(R, dtype=HMM_DTYPE)
    off = np.zeros(R + 1, dtype=np.int64)
    while True:
        seg = np.zeros(cap, dtype=dtype)
        rc = call(rec, off, seg, cap)
        if rc == _lib.SK_ERR_OVERFLOW and int(off[R]) > cap:
            cap = int(off[R])
            continue
        check(rc)
        return rec, off, seg[:int(off[R])]


def hmm_segments_batch(sig, lens, model, cal2=None, limit=0):
    """hmm_viterbi_batch with the best path itself: (rec HMM_DTYPE [R], off int64 [R + 1], seg HMM_SEG_DTYPE [off[R]]).
    Read r's segments -- the maximal runs of one state, in rising start -- are seg[off[r]:off[r + 1]]; each holds state,
    start, length, n1 (samples whose second emission component won) and per winning component the exact sum and sum of
    squares of its RAW samples, with or without cal2 (hmm_segment_levels converts).  rec is hmm_viterbi_batch's."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    if lens.shape != (R,):
        raise ValueError("lens must hold one length per row")
    cal2 = _hmm_cal(cal2, R)
    if R == 0 or stride == 0:
        rec = np.zeros(R, dtype=HMM_DTYPE)
        rec["final_state"], rec["enter"] = -1, -1
        return rec, np.zeros(R + 1, dtype=np.int64), np.zeros(0, dtype=HMM_SEG_DTYPE)
    cap = 16 * R + int(np.clip(lens, 0, stride).sum()) // 512

    def call(rec, off, seg, cap):
        return L.sk_hmm_segments_i16(ptr(sig), stride, ptr(lens), R, None if cal2 is None else ptr(cal2), C.byref(model),
                                     int(limit), ptr(rec), ptr(off), ptr(seg) if cap else None, cap)
    return _segments_call(call, R, HMM_SEG_DTYPE, cap)


def hmm_segments_ragged_f64(values, off, model, limit=0):
    """hmm_segments_batch for ragged float64 reads, read r = values[off[r]:off[r + 1]]: (rec, seg_off, seg HMM_SEGF_DTYPE)
    -- the sums are float64, accumulated sample by sample in rising order."""
    L = _lib.ensure_init()
    values = np.ascontiguousarray(values, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = max(off.size - 1, 0)
    if R == 0:
        return np.zeros(0, dtype=HMM_DTYPE), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=HMM_SEGF_DTYPE)
    if values.size == 0:
        values = np.zeros(1)
    cap = 16 * R + int(off[R] - off[0]) // 512

    def call(rec, soff, seg, cap):
        return L.sk_hmm_segments_f64_len(ptr(values), ptr(off), R, C.byref(model), int(limit), ptr(rec), ptr(soff),
                                         ptr(seg) if cap else None, cap)
    return _segments_call(call, R, HMM_SEGF_DTYPE, cap)


def _segments_parts(reads, model, limit=0):
    """the reads of a list through both feeds: [(indices into reads, rec, off, seg)], integer-valued reads first"""
    ints, arrs, flts = _split_int16(reads)
    parts = []
    if ints:
        parts.append((ints,) + hmm_segments_batch(*pack_i16([np.asarray(a).reshape(-1) for a in arrs]), model, None, limit))
    if flts:
        parts.append((flts,) + hmm_segments_ragged_f64(*pack_f64([reads[i] for i in flts]), model, limit))
    return parts


def hmm_segments(reads, model, limit=0):
    """The records and segments of a list of reads of any lengths: (rec HMM_DTYPE [R], segs) with segs[r] the segments of
    read r -- HMM_SEG_DTYPE for an integer-valued read (int16 feed), HMM_SEGF_DTYPE otherwise.  Input order is kept."""
    rec = np.zeros(len(reads), dtype=HMM_DTYPE)
    segs = [None] * len(reads)
    for idx, prec, off, seg in _segments_parts(reads, model, limit):
        rec[idx] = prec
        for k, i in enumerate(idx):
            segs[i] = seg[int(off[k]):int(off[k + 1])]
    return rec, segs


def hmm_state_path(seg_of_read, n=None):
    """The state of every sample of one read from its segments (int32 [n]); n, when given, is checked against them."""
    seg = np.asarray(seg_of_read)
    path = np.repeat(seg["state"].astype(np.int32), seg["length"])
    if n is not None and path.size != int(n):
        raise ValueError("the segments hold %d samples, not %d" % (path.size, int(n)))
    return path


def _seg_moments(seg):
    """length, sum and sum of squares of every segment (both components together) as long doubles"""
    seg = np.asarray(seg)
    return (seg["length"].astype(np.longdouble), seg["sum"].astype(np.longdouble).sum(axis=1),
            seg["sumsq"].astype(np.longdouble).sum(axis=1))


def hmm_segment_levels(seg, cal=None):
    """(mean, stdv) of every segment's samples (ddof 0) in the model's units, float64.  cal: None, one (offset, unit) pair,
    or one pair per segment ([len(seg), 2], e.g. np.repeat(cal2, np.diff(off), axis=0)) -- the affine conversion of the raw
    sums of the int16 feed: mean = (mean_raw + offset) * unit, stdv = stdv_raw * |unit|."""
    n, s, q = _seg_moments(seg)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / n
        stdv = np.sqrt(np.maximum(q / n - mean * mean, 0))
    if cal is not None:
        cal = np.asarray(cal, dtype=np.float64).reshape(-1, 2)
        if len(cal) not in (1, len(mean)):
            raise ValueError("cal must hold one (offset, unit) pair, or one per segment")
        mean = (mean + cal[:, 0]) * cal[:, 1]
        stdv = stdv * np.abs(cal[:, 1])
    return mean.astype(np.float64), stdv.astype(np.float64)


def hmm_pool(rec, off, seg, S, cal2=None):
    """What the paths of a batch say about its model, as a dict: "n", "sum", "sumsq" [S, 2] -- per state and emission
    component the samples it won, their sum and sum of squares in the model's units (int64 and exact for the int16 feed
    without cal2; float64 under cal2 [R, 2] = (offset, unit) per read: x = (raw + offset) * unit, expanded on the sums) --
    "trans" [S, S] int64: length - 1 stays per segment plus one step per pair of neighbours, "init" [S] int64: the first
    state of every read with samples, and "reads": those reads."""
    off = np.asarray(off, dtype=np.int64)
    seg = np.asarray(seg)
    R = off.size - 1
    if len(np.asarray(rec)) != R:
        raise ValueError("rec and off must describe the same reads")
    st = seg["state"].astype(np.int64)
    ln = seg["length"].astype(np.int64)
    n1 = seg["n1"].astype(np.int64)
    per = np.diff(off)
    exact = seg["sum"].dtype.kind == "i" and cal2 is None
    sm, sq = seg["sum"], seg["sumsq"]
    cnt = np.stack([ln - n1, n1], axis=1)
    if cal2 is not None:
        cal2 = np.asarray(cal2, dtype=np.float64).reshape(-1, 2)
        if len(cal2) != R:
            raise ValueError("cal2 must hold one (offset, unit) pair per read")
        o, u = np.repeat(cal2[:, 0], per)[:, None], np.repeat(cal2[:, 1], per)[:, None]
        smf, sqf, cf = sm.astype(np.float64), sq.astype(np.float64), cnt.astype(np.float64)
        sq = (u * u) * (sqf + 2.0 * o * smf + cf * (o * o))
        sm = u * (smf + cf * o)
    dt = np.int64 if exact else np.float64
    out = {"n": np.zeros((S, 2), dtype=np.int64), "sum": np.zeros((S, 2), dtype=dt), "sumsq": np.zeros((S, 2), dtype=dt),
           "trans": np.zeros((S, S), dtype=np.int64), "init": np.zeros(S, dtype=np.int64), "reads": int((per > 0).sum())}
    np.add.at(out["n"], st, cnt)
    np.add.at(out["sum"], st, sm.astype(dt))
    np.add.at(out["sumsq"], st, sq.astype(dt))
    np.add.at(out["trans"], (st, st), ln - 1)
    if st.size:
        first = np.zeros(st.size, dtype=bool)
        first[off[:-1][per > 0]] = True
        np.add.at(out["init"], st[first], 1)
        nb = ~first[1:]                                      # pairs of neighbours inside one read
        np.add.at(out["trans"], (st[:-1][nb], st[1:][nb]), 1)
    return out


def hmm_pool_add(a, b):
    """the pooled counts of two batches together (a may be None)"""
    if a is None:
        return b
    out = {}
    for k in a:
        if k == "reads":
            out[k] = a[k] + b[k]
        elif a[k].dtype == b[k].dtype:
            out[k] = a[k] + b[k]
        else:
            out[k] = a[k].astype(np.float64) + b[k].astype(np.float64)
    return out


def hmm_spec_to_json(spec):
    """The description (init, trans, emissions) of a model as JSON text -- settings only; a flat component's mean is null.
    hmm_spec_from_json gives the same numbers back."""
    import json
    init, trans, emissions = spec
    return json.dumps({"init": [float(p) for p in init], "trans": [[float(p) for p in row] for row in trans],
                       "emissions": [[[float(w), None if m is None else float(m), float(s)] for w, m, s in comps]
                                     for comps in emissions]}, indent=1) + "\n"


def hmm_spec_from_json(text):
    import json
    d = json.loads(text)
    try:
        spec = ([float(p) for p in d["init"]], [[float(p) for p in row] for row in d["trans"]],
                [[(float(w), None if m is None else float(m), float(s)) for w, m, s in comps] for comps in d["emissions"]])
    except (KeyError, TypeError, ValueError):
        raise ValueError("not a model description: need init [S], trans [S][S] and emissions [S][1 or 2][3]") from None
    hmm_model(*spec)                                         # (its checks)
    return spec


HMM_REFIT_FIELDS = ("mean", "sigma", "weight", "trans")


def hmm_refit(spec, pooled, states, update=("mean", "sigma"), sigma_floor=1.0, min_count=16, pseudo=1.0):
    """One round of Viterbi training: a new description from `spec` and the pooled counts of its paths (hmm_pool).  Only
    the states named in `states` and only the fields named in `update` change:
      "mean", "sigma"  a Gaussian component that won N >= min_count samples: mean = sum / N,
                       sigma = sqrt(max(sumsq / N - (sum / N)^2, sigma_floor^2)); a flat component keeps its range.
      "weight"         a state of two components, N = N_0 + N_1 >= min_count: weight_m = W * (N_m + pseudo * old_m / W) /
                       (N + pseudo) with W = old_0 + old_1 -- smoothed toward the old weights by `pseudo` samples.
      "trans"          the state's row, N = its steps >= min_count: over the allowed (non-zero) transitions only,
                       p_j = (A_j + pseudo * old_j / sum(old)) / (N + pseudo): the row sums to 1, a forbidden transition
                       stays forbidden and an allowed one stays above zero.
    The default leaves weights and transitions alone on purpose: with everything free, wide states take samples from their
    neighbours round after round."""
    init, trans, emissions = spec
    bad = [f for f in update if f not in HMM_REFIT_FIELDS]
    if bad:
        raise ValueError("update: no field %r (fields: %s)" % (bad[0], ", ".join(HMM_REFIT_FIELDS)))
    if not (sigma_floor > 0 and pseudo > 0):
        raise ValueError("sigma_floor and pseudo must be positive")
    S = len(init)
    init = [float(p) for p in init]
    trans = [[float(p) for p in row] for row in trans]
    emissions = [[tuple(comp) for comp in comps] for comps in emissions]
    for k in states:
        k = int(k)
        if not 0 <= k < S:
            raise ValueError("state %d: the model has %d states" % (k, S))
        n = [float(v) for v in pooled["n"][k]]
        comps = list(emissions[k])
        for m, (w, mean, width) in enumerate(comps):
            if mean is None or n[m] < max(min_count, 1):
                continue
            mu = float(pooled["sum"][k][m]) / n[m]
            if "sigma" in update:
                width = float(np.sqrt(max(float(pooled["sumsq"][k][m]) / n[m] - mu * mu, sigma_floor * sigma_floor)))
            if "mean" in update:
                mean = mu
            comps[m] = (w, mean, width)
        if "weight" in update and len(comps) == 2 and n[0] + n[1] >= max(min_count, 1):
            W = comps[0][0] + comps[1][0]
            comps = [(W * (n[m] + pseudo * comps[m][0] / W) / (n[0] + n[1] + pseudo),) + comps[m][1:] for m in range(2)]
        emissions[k] = comps
        if "trans" in update:
            A = [float(v) for v in pooled["trans"][k]]
            allowed = [j for j in range(S) if trans[k][j] > 0.0]
            N, old = sum(A[j] for j in allowed), sum(trans[k][j] for j in allowed)
            if allowed and N >= max(min_count, 1):
                for j in allowed:
                    trans[k][j] = (A[j] + pseudo * trans[k][j] / old) / (N + pseudo)
    return init, trans, emissions


def hmm_fit(batches, spec, states, rounds, update=("mean", "sigma"), sigma_floor=1.0, min_count=16, pseudo=1.0, limit=0,
            decode=None):
    """Viterbi training: `rounds` times decode every batch under the current model, pool the paths, refit (hmm_refit).
    batches: a list of reads (one batch), or a callable that returns an iterable of batches -- each a list of reads or a
    tuple (sig int16 [R, stride], lens, cal2 or None) -- and is called once per round (a file streamed again).  decode:
    None for the GPU (hmm_segments_batch / hmm_segments_ragged_f64), or decode(batch, model, limit) -> an iterable of
    (rec, off, seg, cal2).  Returns (spec, history): history[i] = {"round", "reads", "segments", "max_segments", "pooled",
    "spec"} of round i -- its counts and the description they led to."""
    def gpu_decode(batch, model, limit):
        if isinstance(batch, tuple):
            sig, lens, cal2 = (tuple(batch) + (None,))[:3]
            yield hmm_segments_batch(sig, lens, model, cal2, limit) + (cal2,)
        else:
            for _idx, rec, off, seg in _segments_parts(batch, model, limit):
                yield rec, off, seg, None
    decode = decode or gpu_decode
    S = len(spec[0])
    history = []
    for rnd in range(int(rounds)):
        model = hmm_model(*spec)
        pooled, nseg, most = None, 0, 0
        for batch in (batches() if callable(batches) else [batches]):
            for rec, off, seg, cal2 in decode(batch, model, limit):
                pooled = hmm_pool_add(pooled, hmm_pool(rec, off, seg, S, cal2))
                nseg += int(off[-1])
                most = max(most, int(np.diff(off).max(initial=0)))
        if pooled is None:
            raise ValueError("hmm_fit: no reads")
        spec = hmm_refit(spec, pooled, states, update, sigma_floor, min_count, pseudo)
        history.append({"round": rnd, "reads": pooled["reads"], "segments": nseg, "max_segments": most, "pooled": pooled,
                        "spec": spec})
    return spec, history


# ----------------------------------------------------------------------------
# signal HMM posteriors: forward-backward per read, soft counts, Baum-Welch (the definition: "signal HMM: posteriors" in
# include/squigglekit_hip.h)
# ----------------------------------------------------------------------------
def _posterior_out(R, n_used, counts, dense):
    """post, counts, goff, gamma and the pointers the C call takes for them"""
    post = np.zeros(R, dtype=HMM_POST_DTYPE)
    cnt = np.zeros(R, dtype=HMM_COUNTS_DTYPE) if counts else None
    goff = gamma = None
    if dense:
        goff = np.concatenate([[0], np.cumsum(n_used, dtype=np.int64)]).astype(np.int64)
        gamma = np.zeros((int(goff[R]), _lib.SK_HMM_STATES), dtype=np.float64)
    args = (ptr(post), ptr(cnt) if counts else None, ptr(goff) if dense else None,
            ptr(gamma if gamma is not None and gamma.size else np.zeros(1)) if dense else None)
    return post, cnt, goff, gamma, args


def _n_used(lens, limit):
    lens = np.minimum(np.asarray(lens, dtype=np.int64), 0x7fffff00)
    return np.minimum(lens, int(limit)) if limit > 0 else lens


def hmm_posterior_batch(sig, lens, model, cal2=None, limit=0, counts=False, dense=False):
    """Forward-backward over every row of an int16 [R, stride] batch (cal2, limit: hmm_viterbi_batch's): (post, counts,
    goff, gamma).  post HMM_POST_DTYPE [R]: loglik, n_used, flags (SK_HMM_POST_IMPOSSIBLE: the model gives the read
    probability 0), final_post[6] = P(state at the last sample), occ[6] = the expected samples per state.  counts
    HMM_COUNTS_DTYPE [R] or None: the soft counts of Baum-Welch in the model's units (hmm_soft_pool pools them).  dense:
    gamma float64 [goff[R], 6], read r's posteriors are gamma[goff[r]:goff[r + 1]]; else goff and gamma are None."""
    L = _lib.ensure_init()
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    if sig.ndim != 2:
        raise ValueError("sig must be [reads, samples]")
    R, stride = sig.shape
    lens = (np.full(R, stride, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32))
    if lens.shape != (R,):
        raise ValueError("lens must hold one length per row")
    cal2 = _hmm_cal(cal2, R)
    post, cnt, goff, gamma, args = _posterior_out(R, _n_used(np.clip(lens, 0, stride), limit), counts, dense)
    if R and stride:
        check(L.sk_hmm_posterior_i16(ptr(sig), stride, ptr(lens), R, None if cal2 is None else ptr(cal2), C.byref(model),
                                     int(limit), *args))
    return post, cnt, goff, gamma


def hmm_posterior_ragged_f64(values, off, model, limit=0, counts=False, dense=False):
    """hmm_posterior_batch for ragged float64 reads: read r is values[off[r]:off[r + 1]], seen as it is."""
    L = _lib.ensure_init()
    values = np.ascontiguousarray(values, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    R = max(off.size - 1, 0)
    post, cnt, goff, gamma, args = _posterior_out(R, _n_used(np.diff(off), limit), counts, dense)
    if values.size == 0:
        values = np.zeros(1)
    if R:
        check(L.sk_hmm_posterior_f64_len(ptr(values), ptr(off), R, C.byref(model), int(limit), *args))
    return post, cnt, goff, gamma


def hmm_posterior(reads, model, limit=0, counts=False, dense=False):
    """The posteriors of a list of reads of any lengths: (post [R], counts [R] or None, gammas or None) with gammas[r] the
    float64 [n_used, 6] posteriors of read r.  Integer-valued reads go through the int16 feed, the rest through the
    float64 one (the same bytes either way); input order is kept."""
    R = len(reads)
    post = np.zeros(R, dtype=HMM_POST_DTYPE)
    cnt = np.zeros(R, dtype=HMM_COUNTS_DTYPE) if counts else None
    gammas = [None] * R if dense else None
    ints, arrs, flts = _split_int16(reads)
    parts = []
    if ints:
        parts.append((ints, hmm_posterior_batch(*pack_i16([np.asarray(a).reshape(-1) for a in arrs]), model, None, limit,
                                                counts, dense)))
    if flts:
        parts.append((flts, hmm_posterior_ragged_f64(*pack_f64([reads[i] for i in flts]), model, limit, counts, dense)))
    for idx, (p, c, goff, gamma) in parts:
        post[idx] = p
        if counts:
            cnt[idx] = c
        if dense:
            for k, i in enumerate(idx):
                gammas[i] = gamma[int(goff[k]):int(goff[k + 1])]
    return post, cnt, gammas


def hmm_soft_pool(post, counts, S):
    """The soft counts of a batch pooled into hmm_pool's dict, for hmm_refit and hmm_pool_add: "n", "sum", "sumsq" [S, 2]
    and "trans" [S, S], "init" [S] as float64 -- expected counts in the model's units, summed over the reads in rising
    order -- and "reads": the reads with samples and a probability above 0 (an integer)."""
    post, counts = np.asarray(post), np.asarray(counts)
    if post.shape != counts.shape:
        raise ValueError("post and counts must describe the same reads")
    ok = (post["n_used"] > 0) & (post["flags"] == 0)
    return {"n": counts["n"][:, :S].sum(axis=0), "sum": counts["sx"][:, :S].sum(axis=0),
            "sumsq": counts["sxx"][:, :S].sum(axis=0), "trans": counts["xi"][:, :S, :S].sum(axis=0),
            "init": counts["init"][:, :S].sum(axis=0), "reads": int(ok.sum())}


def hmm_fit_em(batches, spec, states, rounds, update=("mean", "sigma"), sigma_floor=1.0, min_count=16, pseudo=1.0, limit=0,
               decode=None):
    """Baum-Welch: hmm_fit's loop with posteriors in place of paths -- `rounds` times take the soft counts of every batch
    under the current model, pool them (hmm_soft_pool), refit (hmm_refit).  batches: as hmm_fit takes them.  decode: None
    for the GPU (hmm_posterior_batch / hmm_posterior_ragged_f64), or decode(batch, model, limit) -> an iterable of (post,
    counts).  Returns (spec, history): history[i] = {"round", "reads", "loglik", "pooled", "spec"} of round i -- loglik is
    the total over the reads the model gives a probability above 0, under the model the round STARTED with."""
    def gpu_decode(batch, model, limit):
        if isinstance(batch, tuple):
            sig, lens, cal2 = (tuple(batch) + (None,))[:3]
            yield hmm_posterior_batch(sig, lens, model, cal2, limit, counts=True)[:2]
        else:
            ints, arrs, flts = _split_int16(batch)
            if ints:
                yield hmm_posterior_batch(*pack_i16([np.asarray(a).reshape(-1) for a in arrs]), model, None, limit,
                                          counts=True)[:2]
            if flts:
                yield hmm_posterior_ragged_f64(*pack_f64([batch[i] for i in flts]), model, limit, counts=True)[:2]
    decode = decode or gpu_decode
    S = len(spec[0])
    history = []
    for rnd in range(int(rounds)):
        model = hmm_model(*spec)
        pooled, loglik = None, 0.0
        for batch in (batches() if callable(batches) else [batches]):
            for post, counts in decode(batch, model, limit):
                pooled = hmm_pool_add(pooled, hmm_soft_pool(post, counts, S))
                loglik += float(post["loglik"][post["flags"] == 0].sum())
        if pooled is None:
            raise ValueError("hmm_fit_em: no reads")
        spec = hmm_refit(spec, pooled, states, update, sigma_floor, min_count, pseudo)
        history.append({"round": rnd, "reads": pooled["reads"], "loglik": loglik, "pooled": pooled, "spec": spec})
    return spec, history


def hmm_boundary_interval(gamma_of_read, states, lo=0.05, hi=0.95):
    """Where the read enters a set of states, as an interval (host numpy): with c(t) = the sum over j in `states` of
    gamma_j(t), (the first t at which c(t) > lo, the first t at which c(t) > hi); -1 where there is none."""
    g = np.asarray(gamma_of_read, dtype=np.float64).reshape(-1, _lib.SK_HMM_STATES)
    c = np.zeros(len(g))
    for j in states:
        c = c + g[:, int(j)]
    first = lambda mask: int(np.argmax(mask)) if mask.any() else -1   # noqa: E731
    return first(c > lo), first(c > hi)


# ----------------------------------------------------------------------------
# MotifSeq sessions: search reads chunk by chunk as they arrive
# ----------------------------------------------------------------------------
def stream_slots(slots, nslots):
    """The slots of one session call as an int32 array: every one inside [0, nslots), none twice."""
    a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= nslots):
        raise ValueError("slot outside [0, %d)" % nslots)
    if np.unique(a).size != a.size:
        raise ValueError("a slot may appear once per call")
    return a


class MotifStream:
    """A MotifSeq session (sk_stream_*): `nslots` reads in progress, searched for every motif of `motifs` chunk by chunk.
    A slot calibrates on its first `calib` kept samples (medmad or zscale, fixed from then on) -- or takes the
    (center, scale) a reset hands it -- and from then on every push returns, per motif, the record dtw_subsequence would
    give on all the samples the slot has seen: STREAM_DTYPE [K, m] (dist, tail, start, end, n, seen, flags, chunks).

        with MotifStream([motif], nslots=512) as ms:
            rec = ms.push(slots, chunks)          # chunks: a list of int16 arrays, or (rows [m, stride], lens [m])
            rec = ms.flush(slots)                 # end of read: calibrate on what there is
            ms.reset(slots)                       # the slots start a new read
    """

    def __init__(self, motifs, nslots, scale="medmad", scale_low=0, scale_hi=1200, calib=2000):
        self._h = None
        self._ms, flat, moff = _flat_motifs(motifs)
        if not self._ms or any(m.size == 0 for m in self._ms):
            raise ValueError("a session needs at least one motif, none of them empty")
        if max(m.size for m in self._ms) > _lib.SK_STREAM_MAX_POINTS:
            raise ValueError("a session takes motifs of at most %d points" % _lib.SK_STREAM_MAX_POINTS)
        if scale not in _lib.SK_SCALE:
            raise ValueError("scale must be one of %s" % sorted(_lib.SK_SCALE))
        if not 1 <= int(calib) <= _lib.SK_STREAM_MAX_CALIB:
            raise ValueError("calib must be in 1 .. %d, got %d" % (_lib.SK_STREAM_MAX_CALIB, int(calib)))
        if not 1 <= int(nslots) <= _lib.SK_STREAM_MAX_SLOTS:
            raise ValueError("nslots must be in 1 .. %d, got %d" % (_lib.SK_STREAM_MAX_SLOTS, int(nslots)))
        self.nslots, self.K, self.calib = int(nslots), len(self._ms), int(calib)
        L = _lib.ensure_init()
        p = _lib.StreamParams(_lib.SK_SCALE[scale], int(scale_low), int(scale_hi), self.calib, self.nslots)
        h = C.c_int32(-1)
        check(L.sk_stream_open(ptr(flat), ptr(moff), self.K, C.byref(p), C.byref(h)))
        self._h = h.value

    handle = property(lambda self: self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001 -- interpreter shutdown
            pass

    def _open(self):
        if self._h is None:
            raise ValueError("the session is closed")
        return _lib.load()

    def push(self, slots, chunks):
        """Append chunk i to slot slots[i]; a chunk of length 0 is a peek.  Records [K, m]."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if isinstance(chunks, tuple):
            rows, lens = chunks
            rows = np.ascontiguousarray(rows, dtype=np.int16)
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if rows.ndim != 2:
                raise ValueError("rows must be [m, stride]")
        else:
            chunks = [np.asarray(c) for c in chunks]
            if any(c.dtype != np.int16 for c in chunks):
                raise ValueError("a session takes int16 chunks (raw samples)")
            rows, lens = pack_i16(chunks)
        if rows.shape[0] != slots.size or lens.size != slots.size:
            raise ValueError("one chunk per slot")
        out = np.zeros((self.K, slots.size), dtype=STREAM_DTYPE)
        if slots.size:
            check(L.sk_stream_push_i16(self._h, ptr(slots), slots.size, ptr(rows), rows.shape[1], ptr(lens), ptr(out)))
        return out

    def flush(self, slots):
        """End the calibration of the slots with what they hold (end of read).  Records [K, m]."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        out = np.zeros((self.K, slots.size), dtype=STREAM_DTYPE)
        if slots.size:
            check(L.sk_stream_flush(self._h, ptr(slots), slots.size, ptr(out)))
        return out

    def reset(self, slots, center=None, scale=None):
        """The slots start a new read: calibrating, or under the given normalisation (scalars or one value per slot)."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if (center is None) != (scale is None):
            raise ValueError("center and scale: both or neither")
        if center is None:
            check(L.sk_stream_reset(self._h, ptr(slots), slots.size, None, None))
            return
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(center, dtype=np.float64), slots.shape))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), slots.shape))
        check(L.sk_stream_reset(self._h, ptr(slots), slots.size, ptr(c), ptr(s)))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L = _lib.load()
            if L.sk_stream_close(h) not in (0, _lib.SK_ERR_NO_DEVICE):   # (after sk_shutdown the session is gone already)
                check(-1)


def stream_decide(rec, means, sds, accept_z, give_up_after):
    """What a selective-sequencing client does with the records [K, m] of a push: int8 [K, m], 1 = accept
    (Z = (dist - mean[k]) / sd[k] <= accept_z, the scoring motifseq_panel takes), -1 = give up (not accepted and
    n >= give_up_after), 0 = wait.  A NaN distance (calibrating, empty, degenerate) waits.  Host only."""
    rec = np.asarray(rec)
    means = np.asarray(means, dtype=np.float64).reshape(-1, *([1] * (rec.ndim - 1)))
    sds = np.asarray(sds, dtype=np.float64).reshape(-1, *([1] * (rec.ndim - 1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (rec["dist"] - means) / sds
        accept = z <= float(accept_z)                                 # (NaN compares false)
    out = np.zeros(rec.shape, dtype=np.int8)
    out[~accept & ~np.isnan(rec["dist"]) & (rec["n"] >= int(give_up_after))] = -1
    out[accept] = 1
    return out


# ----------------------------------------------------------------------------
# Mapping sessions: the pair-list DTW continued as a read's events arrive
# ----------------------------------------------------------------------------
class MapStream:
    """A mapping session (sk_map_*): `nslots` queries in progress, each searched in every target of `targets` as its
    points arrive.  A push appends a chunk of already-normalised float64 points to every named slot and returns
    MAPREC_DTYPE [T, m]: (dist, start, end, n, flags) of record [t, i] are dtw_subsequence(all points slot slots[i] has
    had since its reset, targets[t]) bit for bit, whatever the cuts and the total; rows / pushes count them.

        with MapStream(targets, nslots=512) as ms:
            rec = ms.push(slots, chunks)          # chunks: a list of float64 arrays, or a (values, off) tuple
            rec = ms.peek(slots)                  # the last records again, nothing swept
            ms.reset(slots)                       # the slots start a new read

    Long targets: open the session on the pieces of tile_targets and hand map_hits(rec) to merge_tiles."""

    def __init__(self, targets, nslots):
        self._h = None
        flat, toff = _as_pool(targets)
        self.T = toff.size - 1
        lens = np.diff(toff)
        if self.T < 1 or self.T > _lib.SK_MAP_MAX_TARGETS:
            raise ValueError("a mapping session takes 1 .. %d targets" % _lib.SK_MAP_MAX_TARGETS)
        if np.any(lens == 0):
            raise ValueError("target %d is empty" % int(np.flatnonzero(lens == 0)[0]))
        if not 1 <= int(nslots) <= _lib.SK_MAP_MAX_SLOTS:
            raise ValueError("nslots must be in 1 .. %d, got %d" % (_lib.SK_MAP_MAX_SLOTS, int(nslots)))
        self.nslots = int(nslots)
        self.state_bytes = self.nslots * int(toff[-1] - toff[0]) * 12
        if self.state_bytes > _lib.SK_MAP_MAX_STATE_BYTES:
            raise ValueError("row state of %d bytes above the cap of %d" % (self.state_bytes, _lib.SK_MAP_MAX_STATE_BYTES))
        L = _lib.ensure_init()
        h = C.c_int32(-1)
        check(L.sk_map_open(ptr(flat), ptr(toff), self.T, self.nslots, C.byref(h)))
        self._h = h.value

    handle = property(lambda self: self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001 -- interpreter shutdown
            pass

    def _open(self):
        if self._h is None:
            raise ValueError("the session is closed")
        return _lib.load()

    def push(self, slots, chunks):
        """Append chunk i to slot slots[i]; a chunk of length 0 is a peek.  Records [T, m]."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        values, off = _as_pool(chunks)
        if off.size - 1 != slots.size:
            raise ValueError("one chunk per slot")
        if off.size > 1 and int(np.diff(off).max()) > _lib.SK_MAP_MAX_CHUNK:
            raise ValueError("a chunk holds at most %d points" % _lib.SK_MAP_MAX_CHUNK)
        out = np.zeros((self.T, slots.size), dtype=MAPREC_DTYPE)
        if slots.size:
            keep = values if values.size else np.zeros(1)
            check(L.sk_map_push(self._h, ptr(slots), slots.size, ptr(keep), ptr(off), ptr(out)))
        return out

    def peek(self, slots):
        """The named slots' last records [T, m]; nothing is swept."""
        slots = stream_slots(slots, self.nslots)
        return self.push(slots, (np.zeros(0), np.zeros(slots.size + 1, dtype=np.int64)))

    def hits(self, slots, max_hits=2, max_dist=np.inf):
        """Up to max_hits non-overlapping loci of the named slots in every target, selected from the rows the pushes
        stored (dtw_pairs_hits' rule): (hits HIT_DTYPE [T, m, K], count int32 [T, m]).  Nothing is swept and nothing of
        the session changes; hits[:, :, 0] are the HIT fields of the slots' last push records; a slot without points
        has count 0."""
        L = self._open()
        K, md = _hit_limits(max_hits, max_dist)
        slots = stream_slots(slots, self.nslots)
        hits = np.zeros((self.T, slots.size, K), dtype=HIT_DTYPE)
        count = np.zeros((self.T, slots.size), dtype=np.int32)
        if slots.size:
            check(L.sk_map_hits(self._h, ptr(slots), slots.size, K, md, ptr(hits), ptr(count)))
        return hits, count

    def reset(self, slots):
        """The slots start a new read: rows = pushes = 0."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if slots.size:
            check(L.sk_map_reset(self._h, ptr(slots), slots.size))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L = _lib.load()
            if L.sk_map_close(h) not in (0, _lib.SK_ERR_NO_DEVICE):      # (after sk_shutdown the session is gone already)
                check(-1)


def map_hits(rec):
    """The HIT_DTYPE fields of mapping-session records (a copy, same shape): what merge_tiles and best_targets take."""
    rec = np.asarray(rec)
    out = np.zeros(rec.shape, dtype=HIT_DTYPE)
    for f in HIT_DTYPE.names:
        out[f] = rec[f]
    return out


def last_map_plan():
    """The last push of a mapping session: {"state_bytes", "entries", "launches"} (sk_last_map_plan)."""
    L = _lib.ensure_init()
    v = [C.c_int64(0) for _ in range(3)]
    check(L.sk_last_map_plan(*[C.byref(x) for x in v]))
    return {"state_bytes": v[0].value, "entries": v[1].value, "launches": v[2].value}


def map_decide(rec, min_rows, max_dist_per_row, min_margin, give_up_rows):
    """What a selective-sequencing client does with the records [T, m] of a mapping session's push.  Returns (best int64
    [m], decision int8 [m]): best is best_targets' rule (the smallest dist, ties to the smallest target index, -1 where
    every dist is NaN); decision 1 = accept, when rows >= min_rows, dist / rows <= max_dist_per_row and (second-best dist
    - best dist) / rows >= min_margin (no margin test with one target); -1 = give up: not accepted and rows >=
    give_up_rows; 0 = wait.  An entry without a distance waits.  Host only."""
    rec = np.asarray(rec)
    T, m = rec.shape
    best = best_targets(rec)
    dec = np.zeros(m, dtype=np.int8)
    if T == 0 or m == 0:
        return best, dec
    has = best >= 0
    d = np.where(np.isnan(rec["dist"]), np.inf, rec["dist"])
    col = np.arange(m)
    bt = np.where(has, best, 0)
    dbest = d[bt, col]
    rows = rec["rows"][bt, col].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        accept = has & (rows >= int(min_rows)) & (dbest / rows <= float(max_dist_per_row))
        if T > 1:
            rest = d.copy()
            rest[bt, col] = np.inf
            accept &= (rest.min(axis=0) - dbest) / rows >= float(min_margin)
    dec[has & ~accept & (rows >= int(give_up_rows))] = -1
    dec[accept] = 1
    return best, dec


def map_decide_loci(hits, count, rows, min_rows, max_dist_per_row, min_margin, give_up_rows):
    """map_decide's rule over hit lists (hits [T, m, K], count [T, m] of MapStream.hits; rows [m], or [T, m] as the push
    records hold them): the margin is (second_dist - best dist) / rows with locus_margin's second_dist -- the next locus
    on ANY target, the best one included -- and a +inf margin (no other locus) passes.  Returns (best int64 [m],
    decision int8 [m]) as map_decide does; with K = 1 and two or more targets it returns what map_decide returns.  Host
    only."""
    hits, count = np.asarray(hits), np.asarray(count)
    T, m = count.shape
    best, rec, second = locus_margin(hits, count)
    dec = np.zeros(m, dtype=np.int8)
    if T == 0 or m == 0:
        return best, dec
    has = best >= 0
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[np.where(has, best, 0), np.arange(m)]
    rows = rows.astype(np.float64)
    dbest = np.where(has, rec["dist"], np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        accept = has & (rows >= int(min_rows)) & (dbest / rows <= float(max_dist_per_row))
        accept &= (second - dbest) / rows >= float(min_margin)
    dec[has & ~accept & (rows >= int(give_up_rows))] = -1
    dec[accept] = 1
    return best, dec


# ----------------------------------------------------------------------------
# Event sessions: a read cut into events as its samples arrive
# ----------------------------------------------------------------------------
class EventStream:
    """An event session (sk_evs_*): `nslots` reads in progress under one sk_det_params, each cut into events as its
    samples arrive.  A push appends a chunk of int16 raw samples to every named slot and returns (off int64 [m + 1],
    rec DET_EVENT_DTYPE [off[m]]): entry i's NEW events are rec[off[i]:off[i + 1]], in read coordinates.  Everything a
    slot returns from its reset to its END is detect_events' array of all its samples, byte for byte, whatever the cuts.

        with EventStream(det_params("dna"), nslots=512) as es:
            off, rec = es.push(slots, chunks)             # chunks: a list of int16 arrays, or (rows [m, stride], lens [m])
            off, rec = es.push(slots, chunks, end=flags)  # flags[i] true: slot slots[i]'s read ends with this chunk
            off, rec = es.finish(slots)                   # END with empty chunks
            es.reset(slots)                               # the slots start a new read

    The records come in detect_events' dtype: event_levels(off, rec) and event_stdv(rec) take them as they are."""

    def __init__(self, params=None, nslots=1):
        self._h = None
        if not 1 <= int(nslots) <= _lib.SK_EVS_MAX_SLOTS:
            raise ValueError("nslots must be in 1 .. %d, got %d" % (_lib.SK_EVS_MAX_SLOTS, int(nslots)))
        self.nslots = int(nslots)
        self.params = params or det_params()
        L = _lib.ensure_init()
        h = C.c_int32(-1)
        check(L.sk_evs_open(C.byref(self.params), self.nslots, C.byref(h)))
        self._h = h.value

    handle = property(lambda self: self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001 -- interpreter shutdown
            pass

    def _open(self):
        if self._h is None:
            raise ValueError("the session is closed")
        return _lib.load()

    def push(self, slots, chunks, end=None):
        """Append chunk i to slot slots[i] (a chunk may be empty); end: None, or one flag per slot -- true says the read
        ends with this chunk.  Returns (off [m + 1], rec): the new events of every entry."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if isinstance(chunks, tuple):
            rows, lens = chunks
            rows = np.ascontiguousarray(rows, dtype=np.int16)
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if rows.ndim != 2:
                raise ValueError("rows must be [m, stride]")
        else:
            chunks = [np.asarray(c) for c in chunks]
            if any(c.dtype != np.int16 for c in chunks):
                raise ValueError("a session takes int16 chunks (raw samples)")
            rows, lens = pack_i16(chunks) if chunks else (np.zeros((0, 0), dtype=np.int16), np.zeros(0, dtype=np.int32))
        m = slots.size
        if rows.shape[0] != m or lens.size != m:
            raise ValueError("one chunk per slot")
        flags = None
        if end is not None:
            flags = np.ascontiguousarray(np.broadcast_to(np.asarray(end), (m,)) != 0, dtype=np.int32)
        off = np.zeros(m + 1, dtype=np.int64)
        if m == 0:
            return off, np.zeros(0, dtype=DET_EVENT_DTYPE)
        keep = rows if rows.size else np.zeros((m, 1), dtype=np.int16)
        stride = rows.shape[1]
        cap = int(np.clip(lens, 0, stride).sum()) // 8 + 2 * m
        rec = np.zeros(cap, dtype=DET_EVENT_DTYPE)
        rc = L.sk_evs_push_i16(self._h, ptr(slots), m, ptr(keep), stride, ptr(lens), None if flags is None else ptr(flags),
                               ptr(off), ptr(rec), cap)
        if rc == _lib.SK_ERR_OVERFLOW and int(off[m]) > cap:          # the session kept them: fetch with room for all
            rec = np.zeros(int(off[m]), dtype=DET_EVENT_DTYPE)
            rc = L.sk_evs_fetch(self._h, ptr(rec), rec.size)
        check(rc)
        return off, rec[:int(off[m])]

    def finish(self, slots):
        """The named slots' reads end here (END with empty chunks): (off, rec) of their last events."""
        slots = stream_slots(slots, self.nslots)
        m = slots.size
        return self.push(slots, (np.zeros((m, 0), dtype=np.int16), np.zeros(m, dtype=np.int32)), end=np.ones(m, dtype=np.int32))

    def reset(self, slots):
        """The slots start a new read."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if slots.size:
            check(L.sk_evs_reset(self._h, ptr(slots), slots.size))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L = _lib.load()
            if L.sk_evs_close(h) not in (0, _lib.SK_ERR_NO_DEVICE):      # (after sk_shutdown the session is gone already)
                check(-1)


def last_event_plan():
    """{"state_bytes", "staged_records"} of the last push of an event session, and "guard_hits": the slots any push of
    any event session of this thread's context has stopped at a guard so far -- it only counts up, so one look after a
    run covers every push of it (sk_last_evs_plan)."""
    L = _lib.ensure_init()
    v = [C.c_int64(0) for _ in range(3)]
    check(L.sk_last_evs_plan(*[C.byref(x) for x in v]))
    return {"state_bytes": v[0].value, "staged_records": v[1].value, "guard_hits": v[2].value}


# ----------------------------------------------------------------------------
# Live mapping sessions: samples in, mapping records and decisions out
# ----------------------------------------------------------------------------
def live_rule(min_rows, max_dist_per_row, min_margin, give_up_rows):
    """map_decide's thresholds, in its argument order, as the sk_live_rule a LiveMap push takes."""
    return LiveRule(int(min_rows), int(give_up_rows), float(max_dist_per_row), float(min_margin))


def live_gate(model, min_body, min_margin, give_up=0, hold=1024, state=TRANSCRIPT):
    """The gate of a gated LiveMap: (model, sk_live_gate).  polya_decide's thresholds in its argument order -- a slot's
    gate opens at enter[state] when the HMM record ends in `state` (TRANSCRIPT = 5 for a polya_model), the body is at
    least min_body samples long and `state` leads every other state by min_margin; give_up <= 0: never -- and `hold`,
    the events a slot keeps while it is gating (1 .. 4096)."""
    if not isinstance(model, HmmModel):
        raise TypeError("model must be an HmmModel (hmm_model / polya_model)")
    return model, LiveGate(int(state), int(min_body), int(give_up), int(hold), float(min_margin))


class LiveMap:
    """A live mapping session (sk_live_*): `nslots` channels in progress under one sk_det_params, one calibration length
    `calib` and one set of targets.  A push appends a chunk of int16 raw samples to every named slot; on the device the
    events are cut (EventStream's kernel), their levels held back until the slot has `calib` of them (or ends), then
    normalised with the mean and standard deviation of those and swept over every target (MapStream's kernel).  Returns
    (rec MAPREC_DTYPE [T, m], info LIVEINFO_DTYPE [m]) -- rec as MapStream.push would return it for the normalised levels
    the slot has been handed, info the slot's state -- and with a rule also best LIVEBEST_DTYPE [m]: map_decide's choice
    and decision per entry.

        with LiveMap(det_params("dna"), 200, targets, nslots=512) as lm:
            rec, info = lm.push(slots, chunks, end=flags)         # chunks: a list of int16 arrays, or (rows, lens)
            rec, info, best = lm.push(slots, chunks, rule=live_rule(100, 0.5, 0.05, 400))
            off, z = lm.fetch()                                   # the normalised chunks of the last push
            hits, count = lm.hits(slots, 2)                       # MapStream.hits on the inner session
            lm.reset(slots)                                       # the slots start a new read

    A live session holds one event-session and one mapping-session handle of the context while it is open.

    gate=live_gate(polya_model("rna_pa"), min_body=2000, min_margin=50.0) makes it a GATED session (it then holds an
    HMM-session handle too): every slot also runs HmmStream's Viterbi pass on its samples and holds the last `hold` events
    back; once polya_decide's rule accepts, only the events that start at or after the transcript start enter[state]
    reach the calibration head and the mapping side -- events, held, mapped and new_events count those.

            lm.reset(slots, cal2)                                 # cal2 [m, 2] = (offset, unit) for the HMM's int16 feed
            gate, hrec = lm.gate()                                # GATE_DTYPE [m], HMMS_DTYPE [m] of the last push"""

    def __init__(self, params, calib, targets, nslots, gate=None):
        self._h = None
        flat, toff = _as_pool(targets)
        self.T = toff.size - 1
        lens = np.diff(toff)
        if self.T < 1 or self.T > _lib.SK_MAP_MAX_TARGETS:
            raise ValueError("a live session takes 1 .. %d targets" % _lib.SK_MAP_MAX_TARGETS)
        if np.any(lens == 0):
            raise ValueError("target %d is empty" % int(np.flatnonzero(lens == 0)[0]))
        if not 1 <= int(nslots) <= _lib.SK_MAP_MAX_SLOTS:
            raise ValueError("nslots must be in 1 .. %d, got %d" % (_lib.SK_MAP_MAX_SLOTS, int(nslots)))
        if not 2 <= int(calib) <= _lib.SK_LIVE_MAX_CALIB:
            raise ValueError("calib must be in 2 .. %d, got %d" % (_lib.SK_LIVE_MAX_CALIB, int(calib)))
        self.nslots, self.calib = int(nslots), int(calib)
        self.params = params or det_params()
        self._last_m = 0
        L = _lib.ensure_init()
        h = C.c_int32(-1)
        self.gated = gate is not None
        if gate is None:
            check(L.sk_live_open(C.byref(self.params), self.calib, ptr(flat), ptr(toff), self.T, self.nslots, C.byref(h)))
        else:
            model, rule = gate
            if not 1 <= rule.hold <= _lib.SK_LIVE_MAX_GATE_HOLD:
                raise ValueError("hold must be in 1 .. %d, got %d" % (_lib.SK_LIVE_MAX_GATE_HOLD, rule.hold))
            check(L.sk_live_open_gated(C.byref(self.params), self.calib, ptr(flat), ptr(toff), self.T, self.nslots,
                                       C.byref(model), C.byref(rule), C.byref(h)))
        self._h = h.value

    handle = property(lambda self: self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001 -- interpreter shutdown
            pass

    def _open(self):
        if self._h is None:
            raise ValueError("the session is closed")
        return _lib.load()

    def push(self, slots, chunks, end=None, rule=None):
        """Append chunk i to slot slots[i] (a chunk may be empty); end: None, or one flag per slot -- true says the read
        ends with this chunk; rule: None, or a live_rule / (min_rows, max_dist_per_row, min_margin, give_up_rows).
        Returns (rec [T, m], info [m]) or, with a rule, (rec, info, best [m])."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if isinstance(chunks, tuple):
            rows, lens = chunks
            rows = np.ascontiguousarray(rows, dtype=np.int16)
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if rows.ndim != 2:
                raise ValueError("rows must be [m, stride]")
        else:
            chunks = [np.asarray(c) for c in chunks]
            if any(c.dtype != np.int16 for c in chunks):
                raise ValueError("a session takes int16 chunks (raw samples)")
            rows, lens = pack_i16(chunks) if chunks else (np.zeros((0, 0), dtype=np.int16), np.zeros(0, dtype=np.int32))
        m = slots.size
        if rows.shape[0] != m or lens.size != m:
            raise ValueError("one chunk per slot")
        flags = None
        if end is not None:
            flags = np.ascontiguousarray(np.broadcast_to(np.asarray(end), (m,)) != 0, dtype=np.int32)
        if rule is not None and not isinstance(rule, LiveRule):
            rule = live_rule(*rule)
        rec = np.zeros((self.T, m), dtype=MAPREC_DTYPE)
        info = np.zeros(m, dtype=LIVEINFO_DTYPE)
        best = np.zeros(m, dtype=LIVEBEST_DTYPE) if rule is not None else None
        if m:
            keep = rows if rows.size else np.zeros((m, 1), dtype=np.int16)
            check(L.sk_live_push_i16(self._h, ptr(slots), m, ptr(keep), rows.shape[1], ptr(lens),
                                     None if flags is None else ptr(flags), None if rule is None else C.byref(rule),
                                     ptr(rec), ptr(info), None if best is None else ptr(best)))
            self._last_m = m
        return (rec, info) if rule is None else (rec, info, best)

    def finish(self, slots, rule=None):
        """The named slots' reads end here (END with empty chunks): what push returns."""
        slots = stream_slots(slots, self.nslots)
        m = slots.size
        return self.push(slots, (np.zeros((m, 0), dtype=np.int16), np.zeros(m, dtype=np.int32)), end=np.ones(m, dtype=np.int32),
                         rule=rule)

    def fetch(self):
        """(off int64 [m + 1], values float64 [off[m]]): the normalised chunks the last push handed to the mapping side,
        entry i's at values[off[i]:off[i + 1]]."""
        L = self._open()
        m = self._last_m
        off = np.zeros(m + 1, dtype=np.int64)
        if m == 0:
            return off, np.zeros(0)
        rc = L.sk_live_fetch(self._h, ptr(off), None, 0)
        if rc == _lib.SK_ERR_OVERFLOW:
            values = np.zeros(int(off[m]), dtype=np.float64)
            rc = L.sk_live_fetch(self._h, ptr(off), ptr(values), values.size)
        else:
            values = np.zeros(0)
        check(rc)
        return off, values

    def hits(self, slots, max_hits=2, max_dist=np.inf):
        """MapStream.hits of the named slots on the inner mapping session: (hits HIT_DTYPE [T, m, K], count int32 [T, m])."""
        L = self._open()
        K, md = _hit_limits(max_hits, max_dist)
        slots = stream_slots(slots, self.nslots)
        hits = np.zeros((self.T, slots.size, K), dtype=HIT_DTYPE)
        count = np.zeros((self.T, slots.size), dtype=np.int32)
        if slots.size:
            check(L.sk_live_hits(self._h, ptr(slots), slots.size, K, md, ptr(hits), ptr(count)))
        return hits, count

    def reset(self, slots, cal2=None):
        """The slots start a new read: CALIBRATING, no events, nothing mapped; in a gated session GATING, with cal2 [m, 2] =
        (offset, unit) per slot for the HMM's int16 feed (None: the raw values)."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        cal2 = _hmm_cal(cal2, slots.size)
        if cal2 is not None and not self.gated:
            raise ValueError("only a gated session takes calibration pairs")
        if slots.size and cal2 is None:
            check(L.sk_live_reset(self._h, ptr(slots), slots.size))
        elif slots.size:
            check(L.sk_live_reset_cal(self._h, ptr(slots), slots.size, ptr(cal2)))

    def gate(self):
        """(gate GATE_DTYPE [m], rec HMMS_DTYPE [m]) of the entries of the last push of a gated session: the slots' gate
        records and the HMM records the decisions were taken on."""
        L = self._open()
        if not self.gated:
            raise ValueError("the session has no gate")
        gate = np.zeros(self._last_m, dtype=GATE_DTYPE)
        rec = np.zeros(self._last_m, dtype=HMMS_DTYPE)
        if self._last_m:
            check(L.sk_live_gate_fetch(self._h, ptr(gate), ptr(rec)))
        return gate, rec

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L = _lib.load()
            if L.sk_live_close(h) not in (0, _lib.SK_ERR_NO_DEVICE):     # (after sk_shutdown the session is gone already)
                check(-1)


def last_live_plan():
    """The last push of a live session: {"state_bytes", "bridged_levels", "launches"} (sk_last_live_plan)."""
    L = _lib.ensure_init()
    v = [C.c_int64(0) for _ in range(3)]
    check(L.sk_last_live_plan(*[C.byref(x) for x in v]))
    return {"state_bytes": v[0].value, "bridged_levels": v[1].value, "launches": v[2].value}


# ----------------------------------------------------------------------------
# HMM sessions: the signal HMM's Viterbi pass continued as a read's samples arrive
# ----------------------------------------------------------------------------
def no_hmm_stream_records(m):
    """m records of slots that have had no sample: sk_hmm_rec's empty record, every v -inf, no push"""
    rec = np.zeros(m, dtype=HMMS_DTYPE)
    rec["final_state"], rec["enter"], rec["v"] = -1, -1, -np.inf
    return rec


class HmmStream:
    """An HMM session (sk_hmms_*): `nslots` reads in progress under one model, each taken through the Viterbi pass as its
    samples arrive.  A push appends a chunk to every named slot and returns HMMS_DTYPE [m]: per entry the record
    hmm_viterbi_batch / hmm_viterbi_ragged_f64 would give on ALL the samples the slot has had since its reset (score,
    final_state, n_used, enter -- bit for bit, whatever the cuts), then v[6], the six scores behind it, and pushes.  An
    empty chunk is a peek.  There is no END: the record after the last push is the finished read's.

        with HmmStream(polya_model("rna_pa"), nslots=512) as hs:
            hs.reset(slots, cal2)                   # a new read per slot; cal2 [m, 2] = (offset, unit) or None
            rec = hs.push(slots, chunks)            # chunks: a list of int16 arrays, or (rows [m, stride], lens [m])
            rec = hs.push_values(slots, chunks)     # chunks: a list of float64 arrays (pA, event levels)
            seg = polya_segments(rec)               # the records are read as hmm_viterbi's are
            dec = polya_decide(rec, min_body=2000, min_margin=50.0, give_up=60000)

    filter=True opens a filtered session (SK_HMMS_FILTER): every slot also carries the forward recursion of the
    posteriors (hmm_posterior_*), 48 bytes more per slot, and filter(slots) returns HMMS_FILT_DTYPE [m]: loglik of the
    samples so far and post[j] = P(state j at the newest sample | the samples so far) -- hmm_posterior_*'s loglik and
    final_post of the same prefix, bit for bit.  The records of push are those of a plain session, byte for byte.

        with HmmStream(polya_model("rna_pa"), nslots=512, filter=True) as hs:
            rec = hs.push(slots, chunks)
            dec = polya_decide_post(rec, hs.filter(slots), min_body=2000, min_post=0.99, give_up=60000)
    """

    def __init__(self, model, nslots=1, filter=False):                   # noqa: A002 -- the ABI's word
        self._h = None
        if not 1 <= int(nslots) <= _lib.SK_HMMS_MAX_SLOTS:
            raise ValueError("nslots must be in 1 .. %d, got %d" % (_lib.SK_HMMS_MAX_SLOTS, int(nslots)))
        self.nslots = int(nslots)
        self.model = model
        L = _lib.ensure_init()
        h = C.c_int32(-1)
        self.filtered = bool(filter)
        if self.filtered:
            check(L.sk_hmms_open_ex(C.byref(model), self.nslots, _lib.SK_HMMS_FILTER, C.byref(h)))
        else:
            check(L.sk_hmms_open(C.byref(model), self.nslots, C.byref(h)))
        self._h = h.value

    handle = property(lambda self: self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001 -- interpreter shutdown
            pass

    def _open(self):
        if self._h is None:
            raise ValueError("the session is closed")
        return _lib.load()

    def push(self, slots, chunks):
        """Append int16 chunk i to slot slots[i] (a chunk may be empty: a peek); the model sees (raw + offset) * unit with
        the slot's calibration pair.  Returns HMMS_DTYPE [m]."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        if isinstance(chunks, tuple):
            rows, lens = chunks
            rows = np.ascontiguousarray(rows, dtype=np.int16)
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if rows.ndim != 2:
                raise ValueError("rows must be [m, stride]")
        else:
            chunks = [np.asarray(c) for c in chunks]
            if any(c.dtype != np.int16 for c in chunks):
                raise ValueError("push takes int16 chunks (raw samples); float64 values go through push_values")
            rows, lens = pack_i16(chunks) if chunks else (np.zeros((0, 0), dtype=np.int16), np.zeros(0, dtype=np.int32))
        m = slots.size
        if rows.shape[0] != m or lens.size != m:
            raise ValueError("one chunk per slot")
        rec = np.zeros(m, dtype=HMMS_DTYPE)
        if m == 0:
            return rec
        keep = rows if rows.size else np.zeros((m, 1), dtype=np.int16)
        check(L.sk_hmms_push_i16(self._h, ptr(slots), m, ptr(keep), rows.shape[1], ptr(lens), ptr(rec)))
        return rec

    def push_values(self, slots, chunks):
        """Append float64 chunk i to slot slots[i]; the model sees the values as they are.  Returns HMMS_DTYPE [m]."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        chunks = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in chunks]
        m = slots.size
        if len(chunks) != m:
            raise ValueError("one chunk per slot")
        rec = np.zeros(m, dtype=HMMS_DTYPE)
        if m == 0:
            return rec
        off = np.zeros(m + 1, dtype=np.int64)
        off[1:] = np.cumsum([c.size for c in chunks])
        values = np.concatenate(chunks) if off[m] else np.zeros(1)
        check(L.sk_hmms_push_f64(self._h, ptr(slots), m, ptr(values), ptr(off), ptr(rec)))
        return rec

    def peek(self, slots):
        """The records of the named slots as they stand; nothing changes."""
        slots = stream_slots(slots, self.nslots)
        return self.push(slots, (np.zeros((slots.size, 0), dtype=np.int16), np.zeros(slots.size, dtype=np.int32)))

    def filter(self, slots):
        """HMMS_FILT_DTYPE [m] of the named slots as they stand (a slot may appear twice); nothing changes.  The session
        must have been opened with filter=True."""
        L = self._open()
        slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        out = np.zeros(slots.size, dtype=HMMS_FILT_DTYPE)
        if slots.size:
            check(L.sk_hmms_filter(self._h, ptr(slots), slots.size, ptr(out)))
        return out

    def reset(self, slots, cal2=None):
        """The slots start a new read; cal2 [m, 2] = (offset, unit) per slot for the int16 feed, None: the raw values."""
        L = self._open()
        slots = stream_slots(slots, self.nslots)
        cal2 = _hmm_cal(cal2, slots.size)
        if slots.size:
            check(L.sk_hmms_reset(self._h, ptr(slots), slots.size, None if cal2 is None else ptr(cal2)))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L = _lib.load()
            if L.sk_hmms_close(h) not in (0, _lib.SK_ERR_NO_DEVICE):     # (after sk_shutdown the session is gone already)
                check(-1)


def last_hmm_stream_plan():
    """{"state_bytes"} of the last push of an HMM session, and "guard_hits": the entries of device-form pushes of any HMM
    session of this thread's context that brought samples beyond their slot's cap so far -- it only counts up, so one
    look after a run covers every push of it (sk_last_hmms_plan)."""
    L = _lib.ensure_init()
    v = [C.c_int64(0) for _ in range(2)]
    check(L.sk_last_hmms_plan(*[C.byref(x) for x in v]))
    return {"state_bytes": v[0].value, "guard_hits": v[1].value}


def polya_decide(rec, min_body, min_margin, give_up):
    """What a live direct-RNA client does with the records of an HMM session under a polya_model.  Returns int8 per
    record: 1 = accept (the transcript has begun: map from enter[TRANSCRIPT]) when final_state == TRANSCRIPT, the body
    is at least min_body samples long (n_used - enter[TRANSCRIPT] >= min_body) and TRANSCRIPT leads every other state by
    at least min_margin (v[TRANSCRIPT] - max(v[j], j != TRANSCRIPT) >= min_margin); -1 = give up: not accepted and
    n_used >= give_up (give_up <= 0: never); 0 = wait.  Host only.

    A heuristic, not a proof: the best path into TRANSCRIPT can still move its entry point while POLYA stays
    competitive, so no record of a prefix is provably final -- which is why the margin is the caller's to set."""
    rec = np.asarray(rec)
    flat = rec.reshape(-1)
    v = flat["v"].reshape(-1, 6)
    n = flat["n_used"].astype(np.int64)
    body = n - flat["enter"].reshape(-1, 6)[:, TRANSCRIPT]
    others = np.delete(v, TRANSCRIPT, axis=1).max(axis=1) if flat.size else np.zeros(0)
    with np.errstate(invalid="ignore"):
        margin = v[:, TRANSCRIPT] - others                           # (-inf - -inf = NaN: no margin, the test fails)
        accept = (flat["final_state"] == TRANSCRIPT) & (body >= int(min_body)) & (margin >= float(min_margin))
    dec = np.zeros(flat.size, dtype=np.int8)
    if int(give_up) > 0:
        dec[~accept & (n >= int(give_up))] = -1
    dec[accept] = 1
    return dec.reshape(rec.shape)


def polya_decide_post(rec, filt, min_body, min_post, give_up, min_rate=None):
    """polya_decide with a probability in the margin's place: rec HMMS_DTYPE and filt HMMS_FILT_DTYPE of the same slots
    after the same push of a filtered HmmStream under a polya_model.  Returns int8 per record: 1 = accept when
    final_state == TRANSCRIPT, n_used - enter[TRANSCRIPT] >= min_body and filt.post[TRANSCRIPT] >= min_post; -1 = reject
    when not accepted and any of: the model gives the samples probability 0 (flags & IMPOSSIBLE); give_up > 0 and
    n_used >= give_up; min_rate is given, n_used >= min_body and loglik / n_used < min_rate (a read the model fits badly:
    junk); 0 = wait.  Host only.

    What is probabilistic: THAT the transcript has begun -- under the left-to-right polya_model post[TRANSCRIPT] is the
    probability, given every sample so far, that the newest sample lies in the transcript.  What is not: WHERE it began
    -- the entry point still comes from the Viterbi record's enter[TRANSCRIPT], the best single path, and can still move
    while the read goes on (hmm_posterior_* with dense=True and hmm_boundary_interval bound it on a finished read)."""
    rec, filt = np.asarray(rec), np.asarray(filt)
    if rec.shape != filt.shape:
        raise ValueError("one filter per record: %s records, %s filters" % (rec.shape, filt.shape))
    flat, ff = rec.reshape(-1), filt.reshape(-1)
    n = flat["n_used"].astype(np.int64)
    body = n - flat["enter"].reshape(-1, 6)[:, TRANSCRIPT]
    post = ff["post"].reshape(-1, 6)[:, TRANSCRIPT]
    accept = (flat["final_state"] == TRANSCRIPT) & (body >= int(min_body)) & (post >= float(min_post))
    reject = (ff["flags"] & _lib.SK_HMM_POST_IMPOSSIBLE) != 0
    if int(give_up) > 0:
        reject |= n >= int(give_up)
    if min_rate is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            rate = ff["loglik"] / np.maximum(n, 1)
            reject |= (n > 0) & (n >= int(min_body)) & (rate < float(min_rate))
    dec = np.zeros(flat.size, dtype=np.int8)
    dec[reject & ~accept] = -1
    dec[accept] = 1
    return dec.reshape(rec.shape)


# ----------------------------------------------------------------------------
# Reference pile-up: per-point event statistics over aligned reads ("Reference pile-up" in include/squigglekit_hip.h and
# DESIGN.md 4.26; tests/pileup_ref.py states it in numpy)
# ----------------------------------------------------------------------------
PILE_CMP_DTYPE = np.dtype([("depth_a", "<i4"), ("depth_b", "<i4"), ("level_a", "<f8"), ("level_b", "<f8"), ("diff", "<f8"),
                           ("t", "<f8"), ("df", "<f8"), ("d", "<f8")])


def _pile_vec(x, n, dtype, name, fill):
    if x is None:
        return np.full(n, fill, dtype=dtype)
    a = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if a.size != n:
        raise ValueError("%s: need %d entries, got %d" % (name, n, a.size))
    return a


def pileup(span_off, spans, value, dwell=None, target=None, shift=None, use=None, tlen=None, entries=False):
    """The alignment table turned round: for every point of every target the rows (events) that cover it, and their
    statistics.  span_off int64 [P + 1] and spans int32 [E, 2] in the layout of dtw_pairs_paths / dtw_band / map_paths (a
    row with a negative first entry has no path); value float64 [E] the query point of each row, dwell int32 [E] its
    samples (default ones); target int32 [P] the target each pair was aligned to (default 0; negative leaves the pair
    out), shift int32 [P] added to both ends of the pair's spans (default 0), use [P] a mask (0 leaves the pair out); tlen
    the targets' lengths.  Returns pile PILE_DTYPE [sum(tlen)], target after target (pile_split cuts it up): level,
    level_sd, vmin, vmax, dwell_mean and dwell_sd are np.mean / np.std / np.min / np.max / np.sum(int64) / n / np.std over
    the point's rows in ascending row order, bit for bit; depth the distinct pairs, n the rows, shared the rows that cover
    more than one point; a point nobody covers has NaN and zeros.  entries=True: (pile, ent_off int64 [sum(tlen) + 1],
    ent_row int32) as well, the rows of flat point m being ent_row[ent_off[m]:ent_off[m + 1]], ascending.  The library
    refuses (SquiggleKitError, code -1, the lowest offending pair named) a span that ends before it begins or leaves its
    target, a target index beyond tlen, and a span_off that is no non-decreasing cover of the rows.  Single device."""
    if tlen is None:
        raise ValueError("pileup: tlen (the targets' lengths) is required")
    span_off = np.ascontiguousarray(span_off, dtype=np.int64).reshape(-1)
    if span_off.size < 1:
        raise ValueError("span_off: need npairs + 1 entries")
    P = span_off.size - 1
    spans = np.ascontiguousarray(spans, dtype=np.int32).reshape(-1, 2)
    E = len(spans)
    value = _pile_vec(value, E, np.float64, "value", 0.0)
    dwell = _pile_vec(dwell, E, np.int32, "dwell", 1)
    target = _pile_vec(target, P, np.int32, "target", 0)
    shift = _pile_vec(shift, P, np.int32, "shift", 0)
    use = None if use is None else _pile_vec(np.asarray(use) != 0, P, np.uint8, "use", 1)
    tlen = np.ascontiguousarray(tlen, dtype=np.int64).reshape(-1)
    mtot = int(tlen.sum()) if tlen.size and tlen.min() >= 0 else 0
    pile = np.zeros(mtot, dtype=PILE_DTYPE)
    ent_off = ent_row = None
    cap = 0
    if entries:
        # the entries, to size ent_row (a span_off the library will refuse leaves it empty)
        if P and E and span_off[0] == 0 and span_off[-1] == E and not np.any(np.diff(span_off) < 0):
            rp = np.repeat(np.arange(P), np.diff(span_off))
            on = (target[rp] >= 0) & (spans[:, 0] >= 0)
            if use is not None:
                on &= use[rp] != 0
            cap = int(np.maximum(spans[on, 1].astype(np.int64) - spans[on, 0] + 1, 0).sum())
        ent_off = np.zeros(mtot + 1, dtype=np.int64)
        ent_row = np.zeros(cap, dtype=np.int32)

    def p(a, empty):
        return ptr(a if a.size else empty)
    z8, z4 = np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.int32)
    L = _lib.ensure_init()                                          # (after the checks that need no device)
    check(L.sk_pileup(ptr(span_off), p(spans, z4), p(value, np.zeros(1)), p(dwell, z4), p(target, z4), p(shift, z4),
                      None if use is None else p(use, np.zeros(1, dtype=np.uint8)), P, E, p(tlen, z8), tlen.size,
                      p(pile, np.zeros(1, dtype=PILE_DTYPE)), None if ent_off is None else ptr(ent_off),
                      None if ent_row is None else p(ent_row, z4), cap))
    return (pile, ent_off, ent_row) if entries else pile


def last_pileup_plan():
    """The last pileup call of this thread's device: {"entries", "longest_list", "lists_in_long_tier", "scratch_bytes"} --
    the entries of the inverted index, the longest point's list, the lists that were put in order by the merge tier
    instead of inside one wavefront's LDS, the bytes of device scratch."""
    L = _lib.ensure_init()
    v = [C.c_int64() for _ in range(4)]
    check(L.sk_last_pileup_plan(*[C.byref(x) for x in v]))
    return dict(zip(("entries", "longest_list", "lists_in_long_tier", "scratch_bytes"), (x.value for x in v)))


def pileup_of_map(queries, dwells, targets, records, span_off, spans, which=None):
    """pileup over what map_queries / map_paths returned: queries the (normalised) query sequences, dwells one int array
    per query (or None: ones), records [T, Q], (span_off, spans) from map_paths(queries, targets, records, which).  The
    target of query q is which[q] (default best_targets(records)); a query without a path is left out.  Returns the pile
    over the targets, in their order."""
    qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in queries]
    Q = len(qs)
    which = best_targets(np.asarray(records)) if which is None else np.asarray(which, dtype=np.int64).reshape(-1)
    if which.size != Q:
        raise ValueError("which: need one target index per query")
    span_off = np.asarray(span_off, dtype=np.int64).reshape(-1)
    if span_off.size != Q + 1:
        raise ValueError("span_off: need one entry per query and one more (map_paths' layout)")
    has = np.diff(span_off) > 0
    if any(has[q] and span_off[q + 1] - span_off[q] != qs[q].size for q in range(Q)):
        raise ValueError("span_off does not match the queries' lengths")
    value = np.concatenate([qs[q] for q in range(Q) if has[q]]) if has.any() else np.zeros(0)
    dwell = None
    if dwells is not None:
        ds = [np.asarray(d, dtype=np.int32).reshape(-1) for d in dwells]
        if len(ds) != Q or any(ds[q].size != qs[q].size for q in range(Q)):
            raise ValueError("dwells: need one entry per query point")
        dwell = np.concatenate([ds[q] for q in range(Q) if has[q]]) if has.any() else np.zeros(0, dtype=np.int32)
    tlen = [np.asarray(t).size for t in targets]
    return pileup(span_off, spans, value, dwell=dwell, target=np.where(has, which, -1), tlen=tlen)


def pile_split(pile, tlen):
    """The per-target views of a flat pile (or of any per-point array): a list, target after target."""
    tlen = np.asarray(tlen, dtype=np.int64).reshape(-1)
    if tlen.size and tlen.min() < 0 or int(tlen.sum()) != len(pile):
        raise ValueError("pile_split: the lengths do not add up to the pile's %d points" % len(pile))
    toff = np.concatenate([[0], np.cumsum(tlen)])
    return [pile[toff[t]:toff[t + 1]] for t in range(tlen.size)]


def refine_targets(targets, pile, min_depth=1):
    """One step of DTW barycentre averaging for whole references, the counterpart of refine_motif: point j of a target
    becomes the pile's level there when depth >= min_depth and the level is a number, and stays as it is otherwise.
    Returns new arrays, one per target.  Host numpy."""
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in targets]
    out = []
    for t, part in zip(ts, pile_split(pile, [t.size for t in ts])):
        ok = (part["depth"] >= int(min_depth)) & ~np.isnan(part["level"])
        out.append(np.where(ok, part["level"], t))
    return out


def pileup_compare(a, b, min_depth=2):
    """Two piles of the same targets (two samples), point by point: PILE_CMP_DTYPE per point.  With n the rows of a point
    (the pile's n), sd its level_sd and v = sd**2 * n / (n - 1) the unbiased variance:
        diff = level_a - level_b
        t    = diff / sqrt(v_a / n_a + v_b / n_b)                                          (Welch)
        df   = (v_a / n_a + v_b / n_b)**2 / ((v_a / n_a)**2 / (n_a - 1) + (v_b / n_b)**2 / (n_b - 1))   (Welch-Satterthwaite)
        d    = diff / sqrt((sd_a**2 + sd_b**2) / 2)
    t, df and d are NaN where either side has n < min_depth (min_depth >= 2) or both variances are zero.  No p-value: a
    normal approximation would mislead at low depth.  Host numpy."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("pileup_compare: need two piles of the same points")
    if int(min_depth) < 2:
        raise ValueError("pileup_compare: min_depth must be at least 2")
    out = np.zeros(len(a), dtype=PILE_CMP_DTYPE)
    out["depth_a"], out["depth_b"] = a["depth"], b["depth"]
    out["level_a"], out["level_b"] = a["level"], b["level"]
    na, nb = a["n"].astype(np.float64), b["n"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["diff"] = a["level"] - b["level"]
        va = a["level_sd"] ** 2 * na / (na - 1)
        vb = b["level_sd"] ** 2 * nb / (nb - 1)
        sa, sb = va / na, vb / nb
        t = out["diff"] / np.sqrt(sa + sb)
        df = (sa + sb) ** 2 / (sa ** 2 / (na - 1) + sb ** 2 / (nb - 1))
        d = out["diff"] / np.sqrt((a["level_sd"] ** 2 + b["level_sd"] ** 2) / 2)
    bad = (a["n"] < int(min_depth)) | (b["n"] < int(min_depth)) | ((va == 0) & (vb == 0))
    for name, v in (("t", t), ("df", df), ("d", d)):
        out[name] = np.where(bad, np.nan, v)
    return out
