"""GPU: the tools' hit-list flags.  squiggle_map --hits K --secondary FILE leaves stdout as it is and writes the table of
api.map_queries_hits (whole targets, and pieces merged by api.merge_tile_hits); squiggle_map_stream --locus_margin decides
by api.map_decide_loci on MapStream.hits, so a read from a stretch the reference holds twice is not accepted on the
margin between the strands."""
import numpy as np
import pytest

from test_gpu_mapstream import run_cli, synthetic_input

pytestmark = pytest.mark.gpu


def queries_of(api, reads, prefix):
    """the z-scored event levels per read, or None, as squiggle_map makes them"""
    from squigglekit_amd.map_cli import zscore
    off, rec = api.detect_events([r[:prefix] for r in reads], api.det_params("dna"))
    values, _ = api.event_levels(off, rec)
    out = []
    for k in range(len(reads)):
        v = values[int(off[k]):int(off[k + 1])]
        out.append(zscore(v) if v.size <= 1024 else None)
    return out


def table(read_ids, queries, hits, count, targets):
    """the --secondary lines: per read its listed loci by (dist, target, end), rank from 1, margin to the first"""
    lines, q = [], 0
    for rid, z in zip(read_ids, queries):
        if z is None:
            continue
        loci = []
        for t in range(hits.shape[0]):
            for k in range(count[t, q]):
                h = hits[t, q, k]
                loci.append((float(h["dist"]), t, int(h["end"]), int(h["start"])))
        q += 1
        loci.sort()
        for rank, (d, t, e, a) in enumerate(loci, 1):
            lines.append("\t".join(str(v) for v in (rid, rank, targets[t][0], targets[t][1], a, e, d, d / len(z), d - loci[0][0])))
    return lines


def test_squiggle_map_secondary_table(gpu, tmp_path):
    from squigglekit_amd import api
    from squigglekit_amd.map_cli import SECONDARY_HEADER, main
    path, model, reads, targets = synthetic_input(tmp_path)
    W = reads.shape[1]
    ys = [t[2] for t in targets]
    queries = queries_of(api, reads, W)
    assert queries[6] is None and queries[7] is None and queries[0] is not None
    qs = [z for z in queries if z is not None]
    ids = [str(r) for r in range(len(reads))]
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", str(W)]
    for extra, pieces in (([], None), (["--piece", "64", "--overlap", "40"], (64, 40))):
        plain, se, code = run_cli(main, base + extra)
        assert code == 0, se
        sec = tmp_path / ("sec%d.tsv" % len(extra))
        so, se, code = run_cli(main, base + extra + ["--hits", "3", "--secondary", str(sec)])
        assert code == 0, se
        assert so == plain                                              # stdout: byte for byte the run without the flags
        if pieces:
            cut, tiling = api.tile_targets(ys, *pieces)
            hits, count = api.merge_tile_hits(*api.map_queries_hits(qs, cut, 3), tiling, 3)
        else:
            hits, count = api.map_queries_hits(qs, ys, 3)
        got = open(sec).read().split("\n")
        assert got[0] == "\t".join(SECONDARY_HEADER) and got[-1] == ""
        want = table(ids, queries, hits, count, targets)
        assert got[1:-1] == want
        assert len(want) > len(qs) and {ln.split("\t")[1] for ln in want} >= {"1", "2", "3"}
        # rank 1 is the line on stdout
        first = {ln.split("\t")[0]: ln.split("\t") for ln in want if ln.split("\t")[1] == "1"}
        for ln in plain.split("\n")[1:-1]:
            c = ln.split("\t")
            if c[1] != ".":
                assert first[c[0]][2:7] == c[1:5] + [c[6]], (c, first[c[0]])
    # a cut on dist per event lists fewer loci, the same ones
    sec = tmp_path / "cut.tsv"
    plain = run_cli(main, base)[0]
    so, se, code = run_cli(main, base + ["--hits", "3", "--secondary", str(sec), "--max_dist_per_event", "0.3"])
    assert code == 0 and so == plain
    hits, count = api.map_queries_hits(qs, ys, 3)
    kept = [ln for ln in table(ids, queries, hits, count, targets) if float(ln.split("\t")[7]) <= 0.3]
    ranked = {}
    for ln in kept:
        c = ln.split("\t")
        ranked.setdefault(c[0], []).append(c[2:8])
    got = {}
    for ln in open(sec).read().split("\n")[1:-1]:
        c = ln.split("\t")
        got.setdefault(c[0], []).append(c[2:8])
    assert got == ranked and 0 < len(kept)
    for argv in (["--hits", "3"], ["--secondary", str(sec)], ["--hits", "65", "--secondary", str(sec)],
                 ["--max_dist_per_event", "1"]):
        assert run_cli(main, base + argv)[2] == 2


def test_stream_locus_margin_on_a_repeat(gpu, tmp_path):
    """the reference holds one stretch twice; a read from it is accepted at once on the margin between the strands, and
    waits to its end under --locus_margin, where the second copy is the second locus"""
    from squigglekit_amd import api
    from squigglekit_amd.mapstream_cli import main, normalise
    rng = np.random.default_rng(15)
    lev = lambda n: np.array([float("%.3f" % v) for v in rng.uniform(60, 130, size=n)])      # noqa: E731
    X = lev(60)
    record = np.concatenate([lev(70), X, lev(40), X, lev(50)])
    model = tmp_path / "rep.model"
    with open(model, "w") as fh:
        fh.write("#rep\npos\tbase\tcurrent\tsd\tdwell\n")
        for i, v in enumerate(record):
            fh.write("%d\tA\t%.3f\t1.5\t8.0\n" % (i, v))
    sig = np.repeat(X * 5.0, rng.integers(18, 32, size=60))
    reads = np.zeros((1, 2500), dtype=np.int16)
    reads[0, :len(sig)] = np.round(sig + rng.normal(scale=2.0, size=len(sig)))
    reads[0, len(sig):] = reads[0, len(sig) - 1]
    path = tmp_path / "one.npy"
    np.save(path, reads)
    rule = (30, 1e9, 0.05, 1000000)
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", "2500", "--calib", "0", "--chunk", "30", "--channels", "2",
            "--min_events", "30", "--max_dist_per_event", "1e9", "--min_margin", "0.05", "--give_up", "1000000"]
    so, se, code = run_cli(main, base)
    assert code == 0, se
    plain = so.split("\n")[1].split("\t")
    assert plain[10] == "accept" and plain[11] == "1" and plain[1:3] == ["rep", "+"]
    so, se, code = run_cli(main, base + ["--locus_margin"])
    assert code == 0, se
    cols = so.split("\n")[1].split("\t")
    assert cols[10] == "end" and len(cols) == 13                        # it waited: never accepted, the give-up is out of reach
    # the decisions are map_decide_loci's on MapStream.hits, push after push
    z = normalise(queries_levels(api, reads[0]), 0)
    zrec = (record - record.mean()) / record.std()
    ys = [zrec, zrec[::-1].copy()]
    pushes, seen, words = 0, 0, []
    with api.MapStream(ys, 2) as ms:
        while seen < len(z):
            rec = ms.push([0], [z[seen:seen + 30]])
            seen, pushes = min(len(z), seen + 30), pushes + 1
            hits, count = ms.hits([0], 2)
            best, dec = api.map_decide_loci(hits, count, rec["rows"][0], *rule)
            assert best[0] == 0 and count[0, 0] == 2
            assert abs(int(hits["start"][0, 0, 0]) - int(hits["start"][0, 0, 1])) >= 90      # the two copies, 100 apart
            words.append(int(dec[0]))
            assert api.map_decide(rec, *rule)[1][0] == 1                 # the margin between the strands accepts every time
    assert words == [0] * pushes and cols[11:] == [str(pushes), str(len(z))]
    assert cols[1:5] == [plain[1], plain[2]] + [str(int(rec["start"][0, 0])), str(int(rec["end"][0, 0]))]


def queries_levels(api, row):
    off, rec = api.detect_events([row], api.det_params("dna"))
    return api.event_levels(off, rec)[0]
