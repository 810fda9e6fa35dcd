"""GPU: seeded random HMM sessions -- drawn models (1 .. 6 states, real-valued or tie-heavy integer ones, -inf transitions
and absent components), slot counts, cuts, shuffled subsets, both feeds, peeks, resets with and without calibration pairs
(tests/hmmstream_ref.draw_session) against the reference after every push, byte for byte.  A failure names the seed and
the session."""
import numpy as np
import pytest

import hmmstream_ref as HR

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5, 8, 13, 21, 34, 89, 144)


def draw(seed):
    """(model, session) of a seed"""
    from test_gpu_hmm import random_model
    rng = np.random.default_rng([77, seed])
    integer = bool(rng.random() < 0.5)
    if integer:
        model = HR.tie_model(rng)
        chunk = lambda r, n: r.integers(0, 4, n).astype(np.int16)       # noqa: E731
    else:
        model = random_model(rng, int(rng.integers(1, 7)))
        chunk = lambda r, n: r.integers(380, 620, n).astype(np.int16)   # noqa: E731
    nslots = int(rng.choice([1, 3, 63, 64, 65, 129, 200]))
    sess = HR.draw_session(rng, nslots=nslots, budget=3000 + 1200 * nslots, maxlen=int(rng.choice([40, 130, 300])),
                           draw_chunk=chunk, cal_prob=0.0 if integer else 0.5)
    return model, sess, integer


def test_the_draws_reach_what_they_are_for():
    """(no GPU work) over the committed seeds: both kinds of model, two states and six, 64 and 65 slots, fewer and more, a
    reset with and without pairs, both feeds, a peek, a one-sample chunk, a chunk above either tile, a continuing slot
    and a fresh slot beside a continuing one in the same push"""
    seen = set()
    for seed in SEEDS:
        model, sess, integer = draw(seed)
        S = model["nstates"] if isinstance(model, dict) else model.nstates
        seen |= {"integer" if integer else "real", "S%d" % S, "slots>64" if sess["nslots"] > 64 else "slots", "n%d" % sess["nslots"]}
        given = {}
        for op in sess["ops"]:
            if op[0] == "reset":
                seen.add("reset" if op[2] is None else "reset+cal")
                for s in op[1]:
                    given[int(s)] = 0
                continue
            kinds = set()
            for s, c in zip(op[1], op[2]):
                seen.add("peek" if len(c) == 0 else "one" if len(c) == 1 else "tile+" if len(c) > 128 else "chunk")
                if len(c):
                    kinds.add("continuing" if given.get(int(s), 0) else "fresh")
                given[int(s)] = given.get(int(s), 0) + len(c)
            seen |= kinds | {op[3]}
            if len(kinds) == 2:
                seen.add("mixed")
    assert seen >= {"integer", "real", "S2", "S6", "n64", "n65", "slots>64", "slots", "reset", "reset+cal", "i16", "f64",
                    "peek", "one", "tile+", "chunk", "continuing", "fresh", "mixed"}, seen


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_session(gpu, seed):
    from squigglekit_amd import api
    model, sess, _ = draw(seed)
    try:
        HR.play_session(api, model, sess, "seed %d" % seed)
    except AssertionError as e:
        raise AssertionError("seed %d: %s" % (seed, str(e)[:3000])) from None
    assert api.last_hmm_stream_plan()["guard_hits"] == 0
