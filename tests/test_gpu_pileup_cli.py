"""GPU: squiggle_map.py --pileup on a small synthetic read set and model.  The spans, z and sample lengths are rebuilt by
parsing the alignment table the same run wrote (--align, or --whole with --pileup_of whole), fed to tests/pileup_ref.py
and formatted: the pile-up file equals that text byte for byte, and stdout and the tables equal a run without --pileup."""
import numpy as np
import pytest

import pileup_ref as pr
from test_cli import run_cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a model of two records and 40 reads made of stretches of them (both strands), two reads that cannot be mapped"""
    d = tmp_path_factory.mktemp("pileup_cli")
    rng = np.random.default_rng(31)
    levels = {}
    with open(d / "ref.model", "w") as fh:
        for name, n in (("recA", 140), ("recB", 80)):
            levels[name] = np.array([float("%.3f" % v) for v in rng.uniform(60, 130, size=n)])
            fh.write("#%s\npos\tbase\tcurrent\tsd\tdwell\n" % name)
            for i, v in enumerate(levels[name]):
                fh.write("%d\tA\t%.3f\t1.5\t8.0\n" % (i, v))
    reads = np.zeros((40, 1600), dtype=np.int16)
    for r in range(38):
        src = levels[("recA", "recB")[r % 2]]
        src = src[::-1] if r % 3 == 0 else src
        a = int(rng.integers(0, len(src) - 66))
        lev = np.repeat(src[a:a + 66] * 5.0, rng.integers(16, 30, size=66))[:1600]
        reads[r, :len(lev)] = np.round(lev + rng.normal(scale=2.0, size=len(lev)))
        reads[r, len(lev):] = reads[r, len(lev) - 1]
    reads[38] = 7
    reads[39, :] = np.repeat([300, 500], 800)
    np.save(d / "reads.npy", reads)
    return d, str(d / "reads.npy"), str(d / "ref.model")


def table_rows(path, targets):
    """(span_off, spans, z, lengths, target per read) of an alignment table: the rows of a read are consecutive"""
    index = {(name, strand): t for t, (name, strand, _) in enumerate(targets)}
    spans, z, lengths, target, counts, last = [], [], [], [], [], None
    for ln in open(path).read().split("\n")[1:-1]:
        f = ln.split("\t")
        if f[0] != last:
            last = f[0]
            target.append(index[(f[1], f[2])])
            counts.append(0)
        counts[-1] += 1
        lengths.append(int(f[5]))
        z.append(float(f[7]))
        spans.append((int(f[8]), int(f[9])))
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.array(spans, dtype=np.int32).reshape(-1, 2),
            np.array(z), np.array(lengths, dtype=np.int32), np.array(target, dtype=np.int32))


def expected_text(path, targets):
    span_off, spans, z, lengths, target = table_rows(path, targets)
    tlen = [len(t[2]) for t in targets]
    pile = pr.pileup_ref(span_off, spans, z, lengths, target=target, tlen=tlen)[0]
    return pr.format_table([t[0] for t in targets], [t[1] for t in targets], [t[2] for t in targets], pile, tlen), pile


def test_pileup_of_the_align_table(gpu, inputs):
    from squigglekit_amd.map_cli import load_targets, main
    d, reads, model = inputs
    argv = ["--i16", reads, "-m", model, "--both", "--prefix", "700", "--batch", "16"]
    plain, se, code = run_cli(main, argv)
    assert code == 0, se
    a0, a1, p1, p2 = (str(d / n) for n in ("a0.tsv", "a1.tsv", "p1.tsv", "p2.tsv"))
    so0, se0, code = run_cli(main, argv + ["--align", a0])
    assert code == 0, se0
    so1, se1, code = run_cli(main, argv + ["--align", a1, "--pileup", p1])
    assert code == 0, se1
    assert so0 == plain and so1 == plain and se1 == se0 and open(a1).read() == open(a0).read()
    targets = load_targets(model, True)
    want, pile = expected_text(a1, targets)
    assert open(p1).read() == want
    assert int(pile["depth"].max()) >= 3 and (pile["n"] == 0).any() and (pile["n"] > pile["depth"]).any()
    # without --align the paths are still traced: the same file
    so2, se2, code = run_cli(main, argv + ["--pileup", p2])
    assert code == 0 and so2 == plain and se2 == se0 and open(p2).read() == want
    # the columns: one line per point of every target, `.` where nobody is
    lines = want.split("\n")[1:-1]
    assert len(lines) == 2 * (140 + 80) and any(ln.endswith("\t.\t.\t.\t.\t.\t.") for ln in lines)
    assert lines[0].split("\t")[:4] == ["recA", "+", "0", "{}".format(float(targets[0][2][0]))]


def test_pileup_of_the_whole_read_table(gpu, inputs):
    from squigglekit_amd.map_cli import load_targets, main
    d, reads, model = inputs
    argv = ["--i16", reads, "-m", model, "--both", "--prefix", "700"]
    w0, w1, a0, a1, p = (str(d / n) for n in ("w0.tsv", "w1.tsv", "wa0.tsv", "wa1.tsv", "pw.tsv"))
    so0, se0, code = run_cli(main, argv + ["--align", a0, "--whole", w0])
    assert code == 0, se0
    so1, se1, code = run_cli(main, argv + ["--align", a1, "--whole", w1, "--pileup", p, "--pileup_of", "whole"])
    assert code == 0, se1
    assert so1 == so0 and se1 == se0 and open(w1).read() == open(w0).read() and open(a1).read() == open(a0).read()
    targets = load_targets(model, True)
    want, pile = expected_text(w1, targets)
    assert open(p).read() == want and int(pile["n"].sum()) > 0
    assert want != expected_text(a1, targets)[0]                    # the whole reads, not their prefixes
