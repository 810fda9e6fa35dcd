"""GPU: the gated live session against its unfused twin on the same device -- api.HmmStream -> api.polya_decide ->
api.EventStream -> the filter start >= t0 behind a ring -> numpy hold-back and normalisation -> api.MapStream ->
api.map_decide.  The same gate states, t0, HMM records, info, mapping records and decisions after every push."""
from collections import deque

import numpy as np
import pytest

import detect_ref
import hmmstream_ref as HR
import livegate_ref as GR
from test_gpu_livegate import script

pytestmark = pytest.mark.gpu

RNA = detect_ref.PRESETS["rna"]
_rng = np.random.default_rng(808)
TARGETS = [_rng.normal(size=n) for n in (300, 450, 600)]
RULE = (40, 1.5, 0.01, 60)


class Twin:
    def __init__(self, G):
        self.state, self.t0, self.ring = GR.GATING, -1, deque(maxlen=G)
        self.lev, self.mean, self.sd, self.mapped, self.ended, self.undecidable = np.zeros(0), np.nan, np.nan, 0, False, False


@pytest.mark.parametrize("hold,give_up,calib", [(64, 0, 8), (4, 1000, 20)])
def test_the_unfused_route_gives_the_same_on_every_push(gpu, hold, give_up, calib):
    from squigglekit_amd import api, _lib
    S = 8
    reads = [HR.small_drna_read(np.random.default_rng(seed), 1500 if seed % 2 else 2200) for seed in range(S)]
    reads[3] = reads[3][:800]                                           # ends while gating
    ops = script(reads, [200, 130, 64, 300, 150, 777, 250, 90])
    model = api.polya_model("synth_raw")
    params = _lib.DetParams(*RNA)
    min_body, margin = 200, 20.0
    tw = [Twin(hold) for _ in range(S)]
    seen = set()
    with api.LiveMap(params, calib, TARGETS, S, gate=api.live_gate(model, min_body, margin, give_up, hold)) as lm, \
            api.HmmStream(model, S) as hs, api.EventStream(params, S) as es, api.MapStream(TARGETS, S) as ms:
        for j, (_, slots, chunks, end) in enumerate(ops):
            rec, info, best = lm.push(slots, chunks, end=end, rule=RULE)
            gate, ghrec = lm.gate()
            # ---- the twin
            gating = [i for i, s in enumerate(slots) if tw[s].state == GR.GATING]
            hrec = hs.push([slots[i] for i in gating], [chunks[i] for i in gating])
            dec = api.polya_decide(hrec, min_body, margin, give_up)
            off, ev = es.push(slots, chunks, end=end)
            mslots, mchunks, at = [], [], []
            for i, s in enumerate(slots):
                t = tw[s]
                was = t.state
                if i in gating:
                    k = gating.index(i)
                    assert ghrec[i].tobytes() == hrec[k].tobytes(), (j, i)
                    if dec[k] == 1:
                        t.state, t.t0 = GR.OPEN, int(hrec["enter"][k][api.TRANSCRIPT])
                    elif dec[k] == -1 or end[i]:
                        t.state = GR.REJECTED
                new = ev[int(off[i]):int(off[i + 1])]
                released = []
                if t.state == GR.OPEN:
                    released = [e for e in (list(t.ring) if was == GR.GATING else []) + list(new) if e["start"] >= t.t0]
                    t.ring.clear()
                elif t.state == GR.GATING:
                    t.ring.extend(new)
                assert (gate["state"][i], gate["t0"][i]) == (t.state, t.t0), (j, i, gate[i])
                lev = np.array([float(e["sum"]) / float(e["length"]) for e in released])
                had = len(t.lev)
                t.lev = np.concatenate([t.lev, lev])
                t.ended = t.ended or bool(end[i])
                z = np.zeros(0)
                if np.isnan(t.sd) and not t.undecidable and (len(t.lev) >= calib or t.ended):
                    head = t.lev[:calib]
                    sd = head.std() if head.size >= 2 else 0.0
                    if sd > 0:
                        t.mean, t.sd, had = head.mean(), sd, 0
                    else:
                        t.undecidable = True
                if not np.isnan(t.sd):
                    z = (t.lev[had:] - t.mean) / t.sd
                t.mapped += len(z)
                state = _lib.SK_LIVE_UNDECIDABLE if t.undecidable else _lib.SK_LIVE_MAPPING if not np.isnan(t.sd) else _lib.SK_LIVE_CALIBRATING
                assert (info["events"][i], info["mapped"][i], info["state"][i], info["new_events"][i], info["ended"][i]) == \
                    (len(t.lev), t.mapped, state, len(lev), int(t.ended)), (j, i, info[i])
                assert info["mean"][i:i + 1].tobytes() == np.array([t.mean]).tobytes(), (j, i)
                assert info["sd"][i:i + 1].tobytes() == np.array([t.sd]).tobytes(), (j, i)
                mslots.append(s)
                mchunks.append(z)
                seen.add((t.state, state))
            mrec = ms.push(mslots, mchunks)
            assert mrec.tobytes() == rec.tobytes(), j
            b, d = api.map_decide(mrec, *RULE)
            assert np.array_equal(best["target"], b) and np.array_equal(best["decision"], d), j
    assert (GR.OPEN, _lib.SK_LIVE_MAPPING) in seen and (GR.REJECTED, _lib.SK_LIVE_UNDECIDABLE) in seen
    assert (GR.GATING, _lib.SK_LIVE_CALIBRATING) in seen and ((GR.REJECTED, _lib.SK_LIVE_CALIBRATING) in seen) == (give_up > 0)
