"""MotifSeq events and pooled models, host side: a numpy statement of the contract (include/squigglekit_hip.h, sk_event
and sk_pool_rec) with checks of its own, the inputs the GPU tests reuse and what they must contain, the header and
the binding, the DBA property of one pooled round, the CLI's flag checks.

An event: with y the read's filtered, normalised samples, x the motif and [a_i, b_i] the span of motif point i in the
warping path of a hit, w = y[a_i : b_i + 1] and the record is (np.sum(w), np.std(w), np.sum(np.abs(x[i] - w)), a_i,
b_i - a_i + 1).  A pool: per motif point, numpy reductions over the selected hits' records in hit order.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from test_hits_host import normalised
from test_paths_host import reference_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "squigglekit_amd", "libsquigglekit_hip.so")
HEADER = os.path.join(ROOT, "include", "squigglekit_hip.h")
NEW_SYMBOLS = ("sk_motifseq_events_i16", "sk_motifseq_events_f64", "sk_motifseq_events_centi",
               "sk_motifseq_events_dev_i16", "sk_events_pool", "sk_events_pool_dev")
EVENT = np.dtype([("sum", "<f8"), ("std", "<f8"), ("cost", "<f8"), ("start", "<i4"), ("dwell", "<i4")])
POOL = np.dtype({"names": ["level", "level_sd", "sd_mean", "dwell_mean", "dwell_sd", "cost_mean", "hits"],
                 "formats": ["<f8"] * 6 + ["<i4"], "offsets": [0, 8, 16, 24, 32, 40, 48], "itemsize": 56})


# ---- the reference -----------------------------------------------------------------------------------------------
def no_events(N):
    ev = np.zeros(N, dtype=EVENT)
    ev["sum"] = ev["std"] = ev["cost"] = np.nan
    ev["start"] = -1
    return ev


def reference_events(x, y, spans):
    """EVENT[N] of one hit from the definitions; spans [N, 2] (-1: no path)."""
    x = np.asarray(x, dtype=np.float64)
    ev = no_events(x.size)
    if spans[0, 0] < 0:
        return ev
    for i, (a, b) in enumerate(spans):
        w = np.ascontiguousarray(y[a:b + 1], dtype=np.float64)
        ev[i] = (np.sum(w), np.std(w), np.sum(np.abs(x[i] - w)), a, b - a + 1)
    return ev


def reference_pool(events, use=None):
    """POOL[N] from events [H, N] and an optional mask [H], from the definitions."""
    N = events.shape[-1]
    ev = events.reshape(-1, N)
    sel = ev["dwell"][:, 0] > 0
    if use is not None:
        sel &= np.asarray(use).reshape(-1) != 0
    out = np.zeros(N, dtype=POOL)
    for i in range(N):
        col = ev[sel, i]
        hits = col.size
        out[i]["hits"] = hits
        if hits == 0:
            for f in POOL.names[:6]:
                out[i][f] = np.nan
            continue
        sum_col, std_col, cost_col = (np.ascontiguousarray(col[f]) for f in ("sum", "std", "cost"))
        dwell_col = np.ascontiguousarray(col["dwell"])
        total_dwell = int(dwell_col.astype(np.int64).sum())
        out[i]["level"] = np.sum(sum_col) / total_dwell
        out[i]["level_sd"] = np.std(sum_col / dwell_col)
        out[i]["sd_mean"] = np.mean(std_col)
        out[i]["dwell_mean"] = total_dwell / hits
        out[i]["dwell_sd"] = np.std(dwell_col.astype(np.float64))
        out[i]["cost_mean"] = np.mean(cost_col)
    return out


def reference_batch(ora, reads, motif, K, scale="medmad", lo=0, hi=1200):
    """(paths, events): reference_paths' list per read (None: flagged) and events [R, K, N] of the same hits."""
    paths = reference_paths(ora, reads, motif, K, scale=scale, lo=lo, hi=hi)
    events = np.stack([np.stack([no_events(len(motif))] * K)] * len(reads))
    for r, (raw, w) in enumerate(zip(reads, paths)):
        if w is None:
            continue
        y = normalised(ora, raw, scale, lo, hi)
        for k, (_, sp) in enumerate(w):
            events[r, k] = reference_events(motif, y, sp)
    return paths, events


# ---- inputs the GPU tests share ----------------------------------------------------------------------------------------
def event_reads(N, seed, nreads=20):
    """A motif and int16 reads of every kind the contract names.  `nreads` squiggles of up to 4 000 samples carry the
    motif (levels placed with the read's own median and MAD) stretched by random dwells (1 .. 3 samples a point, three
    points of 8 .. 40), the first of them noiseless and with one point held for 300 samples (a stalled point: a plateau
    its level matches); then a read nothing of which survives the filter, a constant read (MAD = 0) and two tie-heavy reads of small integers."""
    from squigglekit_amd import synth
    motif = synth.synthetic_motif(N, seed=seed)
    base = synth.squiggle_batch(nreads, 4000, 1000 + seed)
    rng = np.random.default_rng(seed)
    reads = []
    for r in range(nreads):
        keep = base[r][(base[r] > 0) & (base[r] < 1200)].astype(np.float64)
        med = np.median(keep)
        mot = np.rint(motif * (np.median(np.abs(keep - med)) * 1.4826) + med)    # the normalised read shows the motif
        dw = rng.integers(1, 4, size=N)
        if N >= 8:
            dw[rng.integers(0, N, size=3)] = rng.integers(8, 41, size=3)
        noise = np.rint(rng.normal(0.0, 3.0, size=int(dw.sum() + 300)))
        if r == 0 and N >= 8:
            i = N // 2
            dw[i] = 300
            noise[:] = 0                                 # (noiseless: 300 samples more must not cost more than a hit elsewhere)
        sig = np.repeat(mot, dw) + noise[:int(dw.sum())]
        row = base[r].copy()
        n = 4000 if r % 3 else 4000 - 37 * r
        if sig.size + 100 < n:
            at = int(rng.integers(50, n - sig.size - 50))
            row[at:at + sig.size] = sig
        reads.append(row[:n])
    reads += [np.full(40, 2000, dtype=np.int16), np.full(500, 512, dtype=np.int16),
              (500 + rng.integers(0, 3, size=700)).astype(np.int16),
              (480 + 10 * rng.integers(0, 4, size=4000)).astype(np.int16)]
    return motif, reads


def check_input_conditions(paths, events):
    """What a batch must contain for a comparison on it to mean something -- from the reference alone."""
    dw = events["dwell"]
    N = dw.shape[-1]
    if N >= 8:                                           # (a 1-point motif has one cell: a_0 = b_0 = start)
        assert np.any((dw > 0) & (dw < 8)) and np.any((dw >= 8) & (dw <= 128)) and np.any(dw >= 129), \
            (dw[dw > 0].min(), dw.max())
        st = events["start"]
        shared = (dw[..., :-1] > 0) & (st[..., 1:] == st[..., :-1] + dw[..., :-1] - 1)
        assert np.any(shared)
    good = sum(1 for w in paths if w)
    assert good >= 0.9 * len(paths), (good, len(paths))


@functools.lru_cache(maxsize=None)
def cached_batch(N, seed, K, scale, kind):
    """(motif, reads, paths, events) of event_reads through the reference, once per process.  kind: "i16", or "pa" --
    the same reads as float64 pA values with two decimals."""
    from oracle import oracle as ora
    ora.build()
    motif, reads = event_reads(N, seed)
    if kind == "pa":
        reads = [np.round((r.astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for r in reads]
    paths, events = reference_batch(ora, reads, motif, K, scale=scale)
    check_input_conditions(paths, events)
    for a in (motif, events):
        a.setflags(write=False)
    return motif, reads, paths, events


# ---- the reference's own checks ----------------------------------------------------------------------------------------
def test_reference_events_on_a_mixed_batch(ora):
    from squigglekit_amd import api
    motif, reads, paths, events = cached_batch(200, 3, 3, "medmad", "i16")
    seen = 0
    for r, w in enumerate(paths):
        if w is None:
            assert np.all(events[r]["dwell"] == 0) and np.all(events[r]["start"] == -1)
            assert np.all(np.isnan(events[r]["sum"]) & np.isnan(events[r]["std"]) & np.isnan(events[r]["cost"]))
            continue
        y = normalised(ora, reads[r])
        for k, ((dist, start, end), sp) in enumerate(w):
            ev = events[r, k]
            if k == 0:                                   # hit 1: the oracle's own path through api.spans_of_path
                px, py = ora.dtw_subsequence_path(motif, y)
                assert np.array_equal(api.spans_of_path(px, py, motif.size), sp)
            px, py = api.expand_path(sp)
            assert int(ev["dwell"].sum()) == px.size                                 # sum of dwells = path length
            for i in range(motif.size):
                w_i = y[sp[i, 0]:sp[i, 1] + 1]
                assert np.float64(ev[i]["sum"] / ev[i]["dwell"]).tobytes() == np.mean(w_i).tobytes()
                if w_i.size == 1:
                    assert ev[i]["std"] == 0.0
            # the shares add up to the distance, in another order than the DTW's own sums: close, not bit-equal
            assert np.isclose(ev["cost"].sum(), dist, rtol=1e-9, atol=1e-9), (r, k)
            assert np.array_equal(api.spans_of_events(ev), sp) and api.spans_of_events(ev).dtype == np.int32
            seen += 1
        assert np.all(api.spans_of_events(events[r, len(w):]) == -1)
    assert seen > 40


def test_spans_of_events_of_no_path():
    from squigglekit_amd import api
    sp = api.spans_of_events(np.stack([no_events(7)] * 3))
    assert sp.shape == (3, 7, 2) and np.all(sp == -1)


def synthetic_events(H, N, seed, dead_every=5):
    """Event arrays that need no DTW: signed sums, dwells of 1 .. 300, every dead_every-th hit without a path."""
    rng = np.random.default_rng(seed)
    ev = np.zeros((H, N), dtype=EVENT)
    ev["dwell"] = rng.integers(1, 300, size=(H, N))
    ev["sum"] = rng.normal(0.3, 1.5, size=(H, N)) * ev["dwell"]
    ev["std"] = np.abs(rng.normal(0.1, 0.05, size=(H, N)))
    ev["cost"] = np.abs(rng.normal(0.4, 0.3, size=(H, N))) * ev["dwell"]
    ev["start"] = rng.integers(0, 4000, size=(H, N))
    if dead_every:
        ev[dead_every - 1::dead_every] = no_events(N)
    return ev


def test_reference_pool_properties():
    ev = synthetic_events(50, 4, 1)
    live = ev["dwell"][:, 0] > 0
    p = reference_pool(ev)
    assert np.all(p["hits"] == live.sum()) and live.sum() == 40
    for i in range(4):
        col = ev[live, i]
        assert p[i]["level"] == col["sum"].sum() / col["dwell"].sum()              # the sample-weighted mean
        assert p[i]["dwell_mean"] == col["dwell"].mean()
    third = np.arange(50) % 3 == 0
    assert np.all(reference_pool(ev, third)["hits"] == (live & third).sum())
    none = reference_pool(ev, np.zeros(50, bool))
    assert np.all(none["hits"] == 0) and all(np.all(np.isnan(none[f])) for f in POOL.names[:6])
    one = reference_pool(ev[:1])
    assert np.all(one["level_sd"] == 0.0) and np.all(one["dwell_sd"] == 0.0)


# ---- header and binding ---------------------------------------------------------------------------------------------------
def test_new_symbols_and_structs():
    head = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, head), name
    assert re.search(r"typedef struct sk_event \{\s*/\* 32 bytes \*/", head)
    assert re.search(r"typedef struct sk_pool_rec \{\s*/\* 56 bytes \*/", head)
    syms = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    from squigglekit_amd import _lib, api
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None
    assert ctypes.sizeof(_lib.Event) == 32 and _lib.EVENT_DTYPE.itemsize == 32 and _lib.EVENT_DTYPE == EVENT
    assert ctypes.sizeof(_lib.PoolRec) == 56 and _lib.POOL_DTYPE.itemsize == 56 and _lib.POOL_DTYPE == POOL
    assert api.EVENT_DTYPE is _lib.EVENT_DTYPE and api.POOL_DTYPE is _lib.POOL_DTYPE


def test_shutdown_frees_every_scratch_buffer_of_a_context():
    """sk_shutdown frees a hand-kept list of the context's sk_buf members and then resets the context: a member that is
    missing from the list leaks its device memory (the events of one big call are gigabytes) at every init / shutdown."""
    csrc = os.path.join(ROOT, "squigglekit_amd", "csrc")
    common = open(os.path.join(csrc, "sk_common.h")).read()
    ctx = common[common.index("struct sk_ctx {"):common.index("// ---- tuning switches")]
    members = re.findall(r"^\s*sk_buf\s+(\w+);", ctx, re.M)
    assert {"events", "poolev", "pool", "pathspans", "bgrec"} <= set(members) and len(members) >= 50
    runtime = open(os.path.join(csrc, "sk_runtime.hip")).read()
    body = runtime[runtime.index("int sk_shutdown(void)"):runtime.index("int sk_sync(void)")]
    assert [m for m in members if "&c->%s" % m not in body] == []


def test_api_rejects_bad_arguments():
    from squigglekit_amd import api
    for K in (0, 65):
        with pytest.raises(ValueError):
            api.motifseq_events([np.arange(10)], [np.zeros(3)], max_hits=K)
    with pytest.raises(ValueError):
        api.motifseq_events([np.arange(10)], [np.zeros(3)], max_dist=float("nan"))
    with pytest.raises(ValueError):
        api.pool_events(np.zeros((3, 4)))                                           # not EVENT_DTYPE
    with pytest.raises(ValueError):
        api.pool_events(synthetic_events(6, 2, 0), use=np.ones(5, bool))


# ---- one round of DTW barycentre averaging --------------------------------------------------------------------------------
def dba_input():
    """24 reads x 1 500 samples that carry a 40-point true motif (levels placed with each background's own median and
    MAD, so that the normalised read shows the truth), and the search motif: the truth with five points moved by 1.5."""
    from squigglekit_amd import synth
    rng = np.random.default_rng(77)
    truth = np.repeat(rng.normal(0.0, 1.1, size=10), 4)
    base = synth.squiggle_batch(24, 1500, 4242)
    reads = []
    for r in range(24):
        row = base[r].astype(np.float64)
        keep = row[(row > 0) & (row < 1200)]
        med = np.median(keep)
        mad = np.median(np.abs(keep - med)) * 1.4826
        dw = rng.integers(2, 6, size=truth.size)
        sig = np.repeat(truth * mad + med, dw) + rng.normal(0.0, 2.0, size=int(dw.sum()))
        at = int(rng.integers(650, 1300 - sig.size))
        row[at:at + sig.size] = sig
        reads.append(np.rint(row).astype(np.int16))
    search = truth.copy()
    search[[3, 11, 18, 26, 35]] += 1.5
    return truth, search, reads


def reference_round(ora, reads, x):
    """(x', pool): events of the best hit per read, pooled, x_i = level_i (a point without hits keeps its value)."""
    _, events = reference_batch(ora, reads, x, 1)
    pool = reference_pool(events[:, 0])
    return np.where(pool["hits"] > 0, pool["level"], x), pool


def test_one_reference_round_moves_the_motif_towards_the_truth(ora):
    truth, search, reads = dba_input()
    assert len(reads) == 24 and all(r.size == 1500 for r in reads) and truth.size == 40
    x1, pool = reference_round(ora, reads, search)
    assert np.all(pool["hits"] == 24)
    before, after = np.mean(np.abs(search - truth)), np.mean(np.abs(x1 - truth))
    assert after < before, (before, after)


# ---- CLI flags -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--pool", "p.tsv", "--panel"], ["--pool", "p.tsv", "--after_stall"],
                                  ["--pool", "p.tsv", "--hits", "3", "--after_stall"]])
def test_cli_refuses_pool_with_panel_and_after_stall(argv, tmp_path, capsys):
    from squigglekit_amd import motifseq_cli
    sig = tmp_path / "s.tsv"
    sig.write_text("f.fast5\tid0\t1\t2\t3\n")
    model = tmp_path / "m.model"
    model.write_text("pos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.0\t0.1\t8\n")
    argv = [str(tmp_path / a) if a == "p.tsv" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        motifseq_cli.main(["-s", str(sig), "-m", str(model)] + argv)
    assert e.value.code == 2
    out = capsys.readouterr()
    assert "readID\t" not in out.out and "--pool" in out.err
    assert not (tmp_path / "p.tsv").exists()
