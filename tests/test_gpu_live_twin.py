"""GPU: a live mapping session against its unfused twin on the same device -- api.EventStream, api.event_levels, the
normalisation rule in numpy, api.MapStream, api.map_decide, which is what squiggle_map_stream --live does per push --
driven by the same scripts: the same record bytes after every push, the same decisions."""
import numpy as np
import pytest

import detect_ref
import evstream_ref as ER
import live_ref as LR

pytestmark = pytest.mark.gpu

S, CAL = 130, 5
RULE = (5, 5.0, -1.0, 60)                            # accepts easily: both signs of the decision are seen
_rng = np.random.default_rng(77)
TARGETS = [_rng.normal(size=n) for n in (150, 400, 1100)]


@pytest.mark.parametrize("k", range(3))
def test_the_unfused_route_gives_the_same_bytes(gpu, k):
    from squigglekit_amd import _lib, api
    sess = ER.draw_session(np.random.default_rng(300 + k), nslots=S, budget=12000, maxlen=300)
    if k < 2:
        sess["params"] = detect_ref.PRESETS[("dna", "rna")[k]]
    params = _lib.DetParams(*sess["params"])
    slot = [LR.Slot() for _ in range(S)]
    mapped = decided = 0
    with api.LiveMap(params, CAL, TARGETS, S) as lm, api.EventStream(params, S) as es, api.MapStream(TARGETS, S) as ms:
        for j, op in enumerate(sess["ops"]):
            if op[0] == "reset":
                lm.reset(op[1])
                es.reset(op[1])
                ms.reset(op[1])
                for s in op[1]:
                    slot[int(s)] = LR.Slot()
                continue
            _, slots, chunks, end = op
            rec, info, best = lm.push(slots, chunks, end=end, rule=RULE)
            off, erec = es.push(slots, chunks, end=end)
            values, _ = api.event_levels(off, erec)
            zs = [slot[int(s)].take(values[int(off[i]):int(off[i + 1])], end[i], CAL) for i, s in enumerate(slots)]
            twin = ms.push(slots, zs)
            assert rec.tobytes() == twin.tobytes(), "script %d op %d\n%s" % (k, j, ER.describe_session(sess))
            want_info = np.array([slot[int(s)].info(int(off[i + 1] - off[i])) for i, s in enumerate(slots)], dtype=LR.INFO)
            d = LR.same_bytes(info, want_info)
            assert d is None, "script %d op %d: info %s" % (k, j, d)
            foff, fz = lm.fetch()
            assert fz.tobytes() == (np.concatenate(zs) if zs else np.zeros(0)).tobytes() and foff[-1] == len(fz)
            b, dec = api.map_decide(twin, *RULE)
            assert np.array_equal(best["target"], b) and np.array_equal(best["decision"], dec), (k, j)
            mapped += int(sum(len(z) for z in zs))
            decided += int(np.count_nonzero(dec))
        assert api.last_event_plan()["guard_hits"] == 0
    assert mapped > 0 and (k == 2 or decided > 0)
