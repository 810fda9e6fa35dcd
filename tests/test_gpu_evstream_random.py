"""GPU: seeded random event sessions -- drawn parameters, slot counts, reads of the four kinds, cuts, shuffled subsets,
ENDs and resets (tests/evstream_ref.draw_session) against the reference after every push, byte for byte, and against the
one-shot call on every ended read.  A failure names the seed and the session."""
import numpy as np
import pytest

import evstream_ref as ER

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89)


def test_the_draws_reach_what_they_are_for():
    """(no GPU work) over the committed seeds: a reset, an END with samples and an empty one, empty and one-sample chunks,
    a chunk above a tile, a continuing slot, more than one wavefront, both presets and a window of 64"""
    seen = set()
    for seed in SEEDS:
        sess = ER.draw_session(np.random.default_rng([91, seed]))
        seen.add("w%d" % sess["params"][1] if sess["params"][1] in (6, 14, 64) else "w")
        seen.add("S>64" if sess["nslots"] > 64 else "S")
        given = {}
        for op in sess["ops"]:
            if op[0] == "reset":
                seen.add("reset")
                for s in op[1]:
                    given[int(s)] = 0
                continue
            for s, c, e in zip(op[1], op[2], op[3]):
                seen.add("empty" if len(c) == 0 else "one" if len(c) == 1 else "tile+" if len(c) > 128 else "chunk")
                if e:
                    seen.add("END+" if len(c) else "END0")
                if len(c) and given.get(int(s), 0):
                    seen.add("continuing")
                given[int(s)] = given.get(int(s), 0) + len(c)
    assert seen >= {"reset", "empty", "one", "tile+", "chunk", "END+", "END0", "continuing", "S>64", "S", "w6", "w14",
                    "w64"}, seen


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_session(gpu, seed):
    from squigglekit_amd import api
    sess = ER.draw_session(np.random.default_rng([91, seed]))
    try:
        ER.play_session(api, sess, "seed %d" % seed)
    except AssertionError as e:
        raise AssertionError("seed %d: %s\n%s" % (seed, str(e)[:2000], ER.describe_session(sess))) from None
