"""CPU: the host side of the reference pile-up -- the numpy statement (tests/pileup_ref.py) on a hand-worked example, the
numpy helpers of the API (pile_split, refine_targets, pileup_compare), the command lines' argument errors and
squiggle_compare.py on two tables written here."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as pc
import pileup_ref as pr
from conftest import GOLD, ROOT
from test_cli import run_cli

MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")


def test_the_numpy_statement_on_the_hand_case():
    """every list and every double of the example is written out in pileup_cases"""
    kw = pc.hand_case()
    pile, ent_off, ent_row = pr.pileup_ref(**kw)
    assert pile.dtype.itemsize == 64 and len(pile) == 14 and ent_off.tolist()[-1] == 10 == ent_row.size
    for m in range(14):
        assert ent_row[ent_off[m]:ent_off[m + 1]].tolist() == pc.HAND_LISTS.get(m, []), m
    for m in range(14):
        if m in pc.HAND_RECORDS:
            assert pile[m].tolist() == pc.HAND_RECORDS[m] + (0,), m
        else:
            assert pile[m].tolist()[6:] == (0, 0, 0, 0) and all(x != x for x in pile[m].tolist()[:6]), m
    # the sums are in table order: swapping two values of a list changes nothing here, but the rows are where they say
    assert kw["value"][ent_row[ent_off[1]:ent_off[2]]].tolist() == [1.0, 2.0, 6.0]


def test_the_numpy_statement_refuses_what_the_library_refuses():
    kw = pc.hand_case()
    for change, pair in ((("spans", 6, (3, 2)), 2), (("spans", 2, (1, 5)), 0), (("target", 1, 4), 1), (("shift", 2, -2), 2),
                         (("span_off", 2, 3), 1), (("span_off", 5, 11), 4), (("span_off", 0, 1), 0)):
        bad = {k: (None if v is None else v.copy()) for k, v in kw.items()}
        bad[change[0]][change[1]] = change[2]
        with pytest.raises(pr.Refused) as ei:
            pr.pileup_ref(**bad)
        assert ei.value.pair == pair, (change, ei.value)
    bad = dict(kw, tlen=np.array([6, -1, 5, 3]))
    with pytest.raises(pr.Refused):
        pr.pileup_ref(**bad)
    masked = {k: (None if v is None else v.copy()) for k, v in kw.items()}
    masked["spans"][8], masked["spans"][9] = (5, 1), (0, 99)        # pairs 3 and 4 are left out: anything goes
    assert pr.pileup_ref(**masked)[0].tobytes() == pr.pileup_ref(**kw)[0].tobytes()


def test_naive_and_numpy_sums_differ_on_wide_values():
    rng = np.random.default_rng(1)
    v = pc.wide_values(rng, 1000)
    assert pr.naive_sum(v) != np.sum(v)


def test_pile_split_and_refine_targets():
    from squigglekit_amd import api
    assert api.PILE_DTYPE == pr.PILE_DTYPE
    kw = pc.hand_case()
    pile = pr.pileup_ref(**kw)[0]
    parts = api.pile_split(pile, kw["tlen"])
    assert [len(p) for p in parts] == [6, 0, 5, 3]
    assert parts[2][0].tobytes() == pile[6].tobytes() and parts[0].base is not None      # views, not copies
    with pytest.raises(ValueError):
        api.pile_split(pile, [6, 5, 2])
    targets = [np.arange(6.0) * 10, np.zeros(0), np.arange(5.0) - 7, np.ones(3)]
    new = api.refine_targets(targets, pile)
    assert new[0].tolist() == [0.0, 3.0, 6.0, 4.0, 4.0, 50.0] and new[1].size == 0
    assert new[2].tolist() == [-1.5, -1.5, 0.5, -4.0, -3.0] and new[3].tolist() == [1.0, 1.0, 1.0]
    deep = api.refine_targets(targets, pile, min_depth=2)
    assert deep[0].tolist() == [0.0, 3.0, 6.0, 30.0, 40.0, 50.0] and deep[2].tolist() == targets[2].tolist()
    assert targets[0][1] == 10.0                                    # the input is left alone


def test_pileup_compare_against_its_formulas():
    from squigglekit_amd import api
    rng = np.random.default_rng(2)
    M = 40
    a, b = np.zeros(M, dtype=api.PILE_DTYPE), np.zeros(M, dtype=api.PILE_DTYPE)
    for p in (a, b):
        p["n"] = rng.integers(0, 30, size=M)
        p["depth"] = np.minimum(p["n"], rng.integers(0, 30, size=M))
        p["level"] = rng.normal(size=M)
        p["level_sd"] = rng.uniform(0.1, 2.0, size=M)
        p["level"][p["n"] == 0] = np.nan
        p["level_sd"][p["n"] == 0] = np.nan
    a["n"][:4], b["n"][:4] = (1, 5, 2, 3), (5, 1, 2, 3)
    a["level_sd"][3] = b["level_sd"][3] = 0.0                       # both variances zero
    a["level_sd"][2] = 0.0                                          # one of them: still tested
    for min_depth in (2, 5):
        got = api.pileup_compare(a, b, min_depth)
        assert got.dtype == api.PILE_CMP_DTYPE and len(got) == M
        for m in range(M):
            na, nb, sa, sb = int(a["n"][m]), int(b["n"][m]), float(a["level_sd"][m]), float(b["level_sd"][m])
            r = got[m]
            assert (r["depth_a"], r["depth_b"]) == (a["depth"][m], b["depth"][m])
            if na and nb:
                assert r["diff"] == a["level"][m] - b["level"][m]
            else:
                assert np.isnan(r["diff"])
            if na < min_depth or nb < min_depth or (sa == 0 and sb == 0):
                assert np.isnan(r["t"]) and np.isnan(r["df"]) and np.isnan(r["d"]), m
                continue
            va, vb = sa * sa * na / (na - 1), sb * sb * nb / (nb - 1)
            diff = float(a["level"][m]) - float(b["level"][m])
            t = diff / math.sqrt(va / na + vb / nb)
            df = (va / na + vb / nb) ** 2 / ((va / na) ** 2 / (na - 1) + (vb / nb) ** 2 / (nb - 1))
            d = diff / math.sqrt((sa * sa + sb * sb) / 2)
            assert r["t"] == pytest.approx(t, rel=1e-12) and r["df"] == pytest.approx(df, rel=1e-12)
            assert r["d"] == pytest.approx(d, rel=1e-12), m
    assert not np.isnan(api.pileup_compare(a, b)["t"][2])
    with pytest.raises(ValueError):
        api.pileup_compare(a, b[:-1])
    with pytest.raises(ValueError):
        api.pileup_compare(a, b, min_depth=1)


def test_pileup_needs_tlen_and_matching_lengths():
    from squigglekit_amd import api
    kw = pc.hand_case()
    with pytest.raises(ValueError):
        api.pileup(kw["span_off"], kw["spans"], kw["value"])
    with pytest.raises(ValueError):
        api.pileup(kw["span_off"], kw["spans"], kw["value"][:-1], tlen=kw["tlen"])
    with pytest.raises(ValueError):
        api.pileup(kw["span_off"], kw["spans"], kw["value"], target=[0, 1], tlen=kw["tlen"])


def test_squiggle_map_pileup_argument_errors(tmp_path):
    from squigglekit_amd.map_cli import build_parser, main
    base = ["--i16", "x.npy", "-m", MODEL]
    for argv, msg in ((base + ["--pileup", "p.tsv", "--pileup_of", "whole"], "--pileup_of whole needs --whole"),
                      (base + ["--pileup_of", "whole", "--whole", "w.tsv"], "--pileup_of needs --pileup"),
                      (base + ["--pileup", "p.tsv", "--pileup_of", "both"], "invalid choice"),
                      (base + ["--pileup"], "expected one argument")):
        so, se, code = run_cli(main, argv)
        assert code == 2 and msg in se and (so == "" or so.startswith("usage")), (argv, se)
    args = build_parser().parse_args(base + ["--pileup", "p.tsv"])
    assert args.pileup == "p.tsv" and args.pileup_of == "align" and args.align is None
    # a file that cannot be written fails before the run: no header on stdout, nothing read
    so, se, code = run_cli(main, base + ["--pileup", str(tmp_path / "no" / "such" / "dir" / "p.tsv")])
    assert code == 2 and so == "" and "p.tsv" in se


def write_table(path, names, strands, targets, pile):
    with open(path, "w") as fh:
        fh.write(pr.format_table(names, strands, targets, pile, [len(t) for t in targets]))


def test_squiggle_compare_on_two_tables(tmp_path):
    from squigglekit_amd import api
    from squigglekit_amd.compare_cli import HEADER, main
    from squigglekit_amd.map_cli import PILEUP_HEADER, pileup_text
    rng = np.random.default_rng(3)
    targets = [rng.normal(size=30), rng.normal(size=12)]
    names, strands = ["chrA", "chrA"], ["+", "-"]
    piles = []
    for s in (4, 5):
        kw = pc.paths_case(np.random.default_rng(s), 25, (5, 20), [30, 12])
        piles.append(pr.pileup_ref(**kw)[0])
    a, b, c = (str(tmp_path / n) for n in ("a.tsv", "b.tsv", "c.tsv"))
    write_table(a, names, strands, targets, piles[0])
    write_table(b, names, strands, targets, piles[1])
    # the tool's own writer gives the text of the reference's
    assert pileup_text(list(zip(names, strands, targets)), piles[0]) == open(a).read()
    assert open(a).readline().rstrip("\n").split("\t") == list(PILEUP_HEADER)
    so, se, code = run_cli(main, [a, b])
    assert code == 0 and se == "", se
    lines = so.split("\n")
    assert lines[0].split("\t") == list(HEADER) and lines[-1] == "" and len(lines) == 42 + 2
    want = api.pileup_compare(piles[0], piles[1], 2)
    assert np.isnan(want["t"]).any() and not np.isnan(want["t"]).all()
    pos = list(range(30)) + list(range(12))
    for m, ln in enumerate(lines[1:-1]):
        f = ln.split("\t")
        assert f[:5] == ["chrA", "+" if m < 30 else "-", str(pos[m]), str(want["depth_a"][m]), str(want["depth_b"][m])]
        for x, name in zip(f[5:], ("level_a", "level_b", "diff", "t", "df", "d")):
            assert x == ("." if np.isnan(want[name][m]) else "{}".format(float(want[name][m]))), (m, name)
    so5, _, code = run_cli(main, [a, b, "--min_depth", "5"])
    assert code == 0 and so5 != so and so5.count(".\t.\t.\n") > so.count(".\t.\t.\n")
    # the launcher in the repository's root runs the same tool, without a GPU
    r = subprocess.run([sys.executable, os.path.join(ROOT, "squiggle_compare.py"), a, b], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == so
    # refusals: other points, not a table, a missing file, a bad --min_depth
    write_table(c, names, ["+", "+"], targets, piles[1])
    so, se, code = run_cli(main, [a, c])
    assert code == 2 and so == "" and "same points" in se and "line 32" in se
    write_table(c, names[:1], strands[:1], targets[:1], piles[1][:30])
    so, se, code = run_cli(main, [a, c])
    assert code == 2 and so == "" and "same points" in se
    open(c, "w").write("readID\ttarget\n")
    assert run_cli(main, [a, c])[2] == 2 and run_cli(main, [a, str(tmp_path / "none.tsv")])[2] == 2
    so, se, code = run_cli(main, [a, b, "--min_depth", "1"])
    assert code == 2 and "--min_depth must be at least 2" in se
