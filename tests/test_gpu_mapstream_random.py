"""GPU: seeded random mapping sessions -- drawn targets, slot counts, cuts, subsets, resets and peeks
(tests/mapstream_ref.draw_session) against the oracle on every slot's concatenation, after every push.  A failure names
the seed, the session and the first record that differs."""
import numpy as np
import pytest

import mapstream_ref as ref

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5, 8, 13, 21, 34, 58, 88)


def test_the_draws_reach_what_they_are_for():
    """(no GPU work) over the committed seeds: a reset, a peek, a chunk above 1 024 points, one-point chunks, a slot that
    continues, tie-heavy and normal data, targets of 1 point and above 1 024"""
    seen = set()
    for seed in SEEDS:
        case = ref.draw_session(np.random.default_rng([77, seed]))
        given = {}
        for st in case["steps"]:
            if st[0] == "reset":
                seen.add("reset")
                for s in st[1]:
                    given[s] = 0
                continue
            for s, c in zip(st[1], st[2]):
                seen.add("peek" if len(c) == 0 else "long" if len(c) > 1024 else "one" if len(c) == 1 else "chunk")
                if len(c) and given.get(s, 0):
                    seen.add("continuing")
                given[s] = given.get(s, 0) + len(c)
        for t in case["targets"]:
            seen.add("M=1" if len(t) == 1 else "M>1024" if len(t) > 1024 else "M")
    assert seen >= {"reset", "peek", "long", "one", "chunk", "continuing", "M=1", "M>1024"}, seen


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_session(gpu, ora, seed):
    from squigglekit_amd import api
    case = ref.draw_session(np.random.default_rng([77, seed]))
    msg = ref.run_session(api, ora, case)
    assert msg is None, "seed %d: %s\n  %s" % (seed, msg, ref.describe_session(case))
