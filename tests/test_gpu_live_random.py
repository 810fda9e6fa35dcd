"""GPU: seeded random live mapping sessions -- drawn detection parameters, calibration lengths, targets, slot counts,
reads of the four kinds, cuts, shuffled subsets, ENDs and resets -- against tests/live_ref.py after every op, byte for
byte.  Self-contained: the generator is below.  A failure names the seed and the session."""
import numpy as np
import pytest

import evstream_ref as ER
import live_ref as LR

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233)


def draw_live(rng):
    """{"params", "C", "targets", "nslots", "rule", "ops"}: ops as evstream_ref scripts, about 5 000 samples in all"""
    params = ER.draw_params(rng)
    C = int(rng.choice([2, 3, 8, 9, int(rng.integers(2, 151)), int(rng.integers(2, 151))]))
    targets = [rng.integers(-2, 3, size=n).astype(np.float64) if rng.random() < 0.3 else rng.normal(size=n)
               for n in rng.integers(20, 701, size=int(rng.integers(1, 5)))]
    S = int(rng.choice([1, 2, 5, 33, 64, 65, 90, int(rng.integers(1, 91))]))
    rule = (int(rng.integers(0, 40)), float(rng.uniform(0.3, 3.0)), float(rng.uniform(-0.2, 0.2)), int(rng.integers(1, 120)))
    kinds = [ER.KINDS[int(rng.integers(0, 4))] for _ in range(S)]
    maxlen = int(rng.choice([40, 300, 900] if S <= 8 else [20, 80, 200]))
    ended = [False] * S
    ops, used, budget = [], 0, 5000
    while used < budget:
        k = int(rng.integers(1, S + 1)) if rng.random() < 0.6 else int(rng.integers(1, min(S, 6) + 1))
        slots = rng.permutation(S)[:k].astype(np.int32)
        if rng.random() < 0.1:
            ops.append(("reset", slots))
            for s in slots:
                ended[s], kinds[s] = False, ER.KINDS[int(rng.integers(0, 4))]
            continue
        chunks, end = [], []
        for s in slots:
            u = rng.random()
            n = 0 if (ended[s] or u < 0.12) else (1 if u < 0.2 else int(rng.integers(0, maxlen + 1)))
            chunks.append(ER.draw_read(rng, n, kinds[s]))
            used += n + 1
            e = bool(rng.random() < 0.12)
            end.append(e)
            ended[s] = ended[s] or e
        ops.append(("push", slots, chunks, np.array(end, dtype=np.int32)))
    ops.append(("push", np.arange(S, dtype=np.int32), [np.zeros(0, dtype=np.int16)] * S, np.ones(S, dtype=np.int32)))
    return {"params": params, "C": C, "targets": targets, "nslots": S, "rule": rule, "ops": ops}


def describe_session(case):
    return "C = %d, targets %s, rule %r\n%s" % (case["C"], [len(t) for t in case["targets"]], case["rule"],
                                                 ER.describe_session(case))


def test_the_draws_reach_what_they_are_for(ora):
    """(no GPU work) over the committed seeds: all three states, a slot reset while mapping and one while calibrating, a
    read that ends before C levels, every decision, one target and several, more than one wavefront"""
    seen = set()
    for seed in SEEDS:
        case = draw_live(np.random.default_rng([93, seed]))
        seen.add("T1" if len(case["targets"]) == 1 else "T+")
        seen.add("S>64" if case["nslots"] > 64 else "S")
        want = LR.run_script(ora, case["params"], case["C"], case["targets"], case["ops"], case["nslots"], case["rule"])
        state = {}
        for op, w in zip(case["ops"], want):
            if op[0] == "reset":
                for s in op[1]:
                    seen.add("reset in state %d" % state.get(int(s), 0))
                    state[int(s)] = 0
                continue
            for i, s in enumerate(op[1]):
                nf = w["info"][i]
                state[int(s)] = int(nf["state"])
                seen.add("state %d" % nf["state"])
                seen.add("decision %d" % w["best"]["decision"][i])
                if nf["state"] == LR.MAPPING and nf["ended"] and nf["events"] < case["C"]:
                    seen.add("short head")
    assert seen >= {"T1", "T+", "S>64", "S", "state 0", "state 1", "state 2", "reset in state 0", "reset in state 1",
                    "decision 0", "decision 1", "decision -1", "short head"}, seen


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_random_live_session(gpu, ora, seed):
    from squigglekit_amd import api
    case = draw_live(np.random.default_rng([93, seed]))
    try:
        LR.play(api, ora, case["params"], case["C"], case["targets"], case["ops"], case["nslots"], rule=case["rule"],
                label="seed %d" % seed)
        assert api.last_event_plan()["guard_hits"] == 0, "guard_hits"
    except AssertionError as e:
        raise AssertionError("seed %d: %s\n%s" % (seed, str(e)[:2000], describe_session(case))) from None
