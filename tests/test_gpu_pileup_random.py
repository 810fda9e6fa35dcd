"""The seeded random family of the reference pile-up (tests/pileup_cases.py: random_case; tests/RANDOM_CASES_PILEUP.md):
200 drawn calls through sk_pileup against tests/pileup_ref.py, bytes for bytes.  A third of the cases runs with the LDS
tier of the ordering step shrunk to 64 entries and a third with 2, so that drawn lists reach the merge tier."""
import numpy as np
import pytest

import pileup_cases as pc
import pileup_ref as pr

GROUP = 20
TIERS = (None, "64", "2")


def tier_of(seed):
    return TIERS[seed % 3]


def test_the_family_reaches_what_it_is_for():
    """CPU, from the cases and the numpy statement alone"""
    seen = dict(no_pairs=0, no_rows=0, nan=0, stalled=0, masked=0, no_target=0, empty_target=0, uncovered_target=0, shifted=0,
                no_path_rows=0, non_monotone=0, past_lds64=0, no_dwell=0, stay=0, shared=0)
    for seed in range(pc.FAMILY_CASES):
        kw = pc.random_case(seed)
        pile, ent_off, ent_row = pr.pileup_ref(**kw)                # no drawn case is a refusal
        P, E = kw["span_off"].size - 1, len(kw["spans"])
        seen["no_pairs"] += P == 0
        seen["no_rows"] += P > 0 and E == 0
        seen["nan"] += bool(np.isnan(pile["level"][pile["n"] > 0]).any())
        seen["stalled"] += bool(E and (kw["spans"][:, 1] - kw["spans"][:, 0] >= 64).any())
        seen["masked"] += kw["use"] is not None and not kw["use"].all()
        seen["no_target"] += bool(P and (kw["target"] < 0).any())
        seen["empty_target"] += bool((kw["tlen"] == 0).any())
        toff = np.concatenate([[0], np.cumsum(kw["tlen"])])
        seen["uncovered_target"] += any(kw["tlen"][t] > 0 and not pile["n"][toff[t]:toff[t + 1]].any() for t in range(kw["tlen"].size))
        seen["shifted"] += bool(P and (kw["shift"] != 0).any())
        seen["no_path_rows"] += bool(E and (kw["spans"][:, 0] < 0).any())
        seen["non_monotone"] += bool(E > 1 and (np.diff(kw["spans"][:, 0]) < -1).any())
        seen["past_lds64"] += tier_of(seed) == "64" and bool((pile["n"] > 64).any())
        seen["no_dwell"] += kw["dwell"] is None
        seen["stay"] += bool((pile["n"] > pile["depth"]).any())
        seen["shared"] += bool(pile["shared"].any())
    assert all(v >= 3 for v in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, pc.FAMILY_CASES, GROUP))
def test_drawn_cases(gpu, monkeypatch, first):
    from squigglekit_amd import api
    for seed in range(first, first + GROUP):
        kw = pc.random_case(seed)
        want = pr.pileup_ref(**kw)
        monkeypatch.delenv("SK_PILE_LDS_ENTRIES", raising=False)
        if tier_of(seed):
            monkeypatch.setenv("SK_PILE_LDS_ENTRIES", tier_of(seed))
        pile, ent_off, ent_row = api.pileup(entries=True, **kw)
        assert np.array_equal(ent_off, want[1]) and np.array_equal(ent_row, want[2]), seed
        bad = [m for m in range(len(pile)) if pile[m].tobytes() != want[0][m].tobytes()][:3]
        assert not bad, (seed, bad, [pile[m] for m in bad], [want[0][m] for m in bad])
        plan = api.last_pileup_plan()
        tier = int(tier_of(seed) or 4096)
        n = np.diff(want[1])
        assert plan["entries"] == ent_row.size and plan["longest_list"] == (int(n.max()) if n.size else 0), seed
        assert plan["lists_in_long_tier"] == int((n > tier).sum()), seed
