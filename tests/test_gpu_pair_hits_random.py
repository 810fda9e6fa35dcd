"""GPU: seeded random hit lists -- a drawn pair list (tests/pair_hits_ref.draw_pairs_case: K, max_dist and the row budget
drawn with it) and a drawn session script (draw_session_case) per seed, against the statement.  A failure names the seed
and the first record that differs."""
import numpy as np
import pytest

import pair_hits_ref as ref

SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)


def cases_of(seed):
    rng = np.random.default_rng([91, seed])
    return ref.draw_pairs_case(rng), ref.draw_session_case(rng)


def test_the_draws_reach_what_they_are_for(ora):
    """(no GPU work) from the reference alone, over the committed seeds: a list with count == K, one with 0 < count < K,
    one with count 0, a row above 4 096 columns, a round decided by a tie on dist"""
    seen = set()
    for seed in SEEDS:
        case, sess = cases_of(seed)
        _, count, tie = ref.pair_hits(ora, case["seqs"], case["pairs"], case["K"], ref.max_dist_of(ora, case))
        for c in count:
            seen.add("full" if c == case["K"] else "none" if c == 0 else "some")
        if tie:
            seen.add("tie")
        if max(len(case["seqs"][t]) for _, t in case["pairs"]) > 4096 or max(len(t) for t in sess["targets"]) > 4096:
            seen.add("long")
    assert seen >= {"full", "some", "none", "long", "tie"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_pair_list(gpu, ora, seed):
    import os
    from squigglekit_amd import api
    case, _ = cases_of(seed)
    msg = ref.run_pairs_case(api, ora, case, os.environ)
    assert msg is None, "seed %d: %s" % (seed, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_session_script(gpu, ora, seed):
    from squigglekit_amd import api
    _, sess = cases_of(seed)
    msg = ref.run_session_case(api, sess)
    assert msg is None, "seed %d: %s" % (seed, msg)
