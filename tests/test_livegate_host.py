"""CPU: self-checks of tests/livegate_ref.py -- the reference of the gated live sessions -- against first principles (they
use nothing of the library but the existing api.polya_decide and api.polya_model), and the argument errors of
squiggle_map_stream --polya_gate.  The released levels
of a finished read are the one-shot events of all its samples with start >= t0, whatever the cuts; with a small ring what
is missing is exactly what the ring had overwritten before the gate opened, and TRUNCATED says so; the decision is
api.polya_decide's on every prefix."""
import numpy as np
import pytest

import detect_ref
import hmmstream_ref as HR
import live_ref as LR
import livegate_ref as GR

RNA = detect_ref.PRESETS["rna"]
_rng = np.random.default_rng(77)
TARGETS = [_rng.normal(size=n) for n in (40, 55)]
ONE = np.array([0], dtype=np.int32)


def cut_ops(x, cuts, end=True):
    ops, a = [], 0
    for i, n in enumerate(cuts):
        last = i == len(cuts) - 1
        ops.append(("push", ONE, [x[a:a + n]], np.array([int(end and last)], dtype=np.int32)))
        a += n
    assert a == len(x)
    return ops


def random_cuts(rng, n):
    cuts = []
    while n:
        c = min(n, int(rng.choice([1, 7, 64, 200, 333, 900])))
        cuts.append(c)
        n -= c
    return cuts


def polya():
    from squigglekit_amd import api
    return api.polya_model("synth_raw")


@pytest.mark.parametrize("seed", range(4))
def test_an_unbounded_ring_releases_the_one_shot_events_from_t0(ora, seed):
    rng = np.random.default_rng(seed)
    x = HR.small_drna_read(rng, 1500)
    rule = GR.rule_of(5, 200, 20.0, 0, 4096)
    for cuts in ([200] * 7 + [100], [len(x)], random_cuts(rng, len(x)), random_cuts(rng, len(x))):
        want = GR.run_script(ora, RNA, 8, TARGETS, polya(), rule, cut_ops(x, cuts), 1)
        g = want[-1]["gate"][0]
        assert g["state"] == GR.OPEN and g["flags"] == 0 and g["dropped"] == 0 and g["ring"] == 0
        ev = detect_ref.events(x, RNA)
        assert g["events_cut"] == len(ev)
        keep = ev[ev["start"] >= g["t0"]]
        got = np.concatenate([w["released"][0] for w in want])
        assert got.tobytes() == keep.tobytes() and g["released"] == len(keep) >= 8
        # the live side saw exactly those levels: the mapping side's points are their normalisation under the head of 8
        lev = LR.levels_of(keep)
        z = (lev - lev[:8].mean()) / lev[:8].std()
        assert np.concatenate([w["z"] for w in want]).tobytes() == z.tobytes()
        assert want[-1]["info"][0]["events"] == len(keep) == want[-1]["info"][0]["mapped"]
        # t0 is the whole read's answer only once the decision is final; at the decision it is the prefix's enter[state]
        at = next(j for j, w in enumerate(want) if w["gate"][0]["state"] == GR.OPEN)
        assert want[at]["gate"][0]["t0"] == want[at]["hrec"][0]["enter"][5] == g["t0"]
        assert want[at]["gate"][0]["decided_n"] == want[at]["hrec"][0]["n_used"] == sum(cuts[:at + 1])
        assert want[-1]["hrec"][0]["n_used"] == g["decided_n"]          # the HMM slot stands still after the decision
        assert abs(int(g["t0"]) - 841) <= 35                            # the planted body start of a 1 500-sample read


@pytest.mark.parametrize("hold", [1, 4, 16])
@pytest.mark.parametrize("seed", range(3))
def test_a_small_ring_loses_what_it_overwrote_and_says_so(ora, seed, hold):
    rng = np.random.default_rng(100 + seed)
    x = HR.small_drna_read(rng, 1500)
    rule = GR.rule_of(5, 200, 20.0, 0, hold)
    ev = detect_ref.events(x, RNA)
    seen_truncated = False
    for cuts in ([200] * 7 + [100], [50] * 30, random_cuts(rng, len(x))):
        want = GR.run_script(ora, RNA, 8, TARGETS, polya(), rule, cut_ops(x, cuts), 1)
        at = next(j for j, w in enumerate(want) if w["gate"][0]["state"] == GR.OPEN)
        g = want[-1]["gate"][0]
        before = int(want[at - 1]["gate"][0]["events_cut"]) if at else 0     # the events cut before the opening push
        lost = ev[:max(0, before - hold)]                               # what the ring had overwritten when the gate opened
        assert g["dropped"] == len(lost)
        truncated = bool((lost["start"] >= g["t0"]).any())
        assert bool(g["flags"] & GR.TRUNCATED) == truncated
        keep = ev[max(0, before - hold):]
        keep = keep[keep["start"] >= g["t0"]]
        assert np.concatenate([w["released"][0] for w in want]).tobytes() == keep.tobytes()
        seen_truncated |= truncated
    assert seen_truncated or hold == 16


def test_end_while_gating_and_give_up(ora):
    x = HR.small_drna_read(np.random.default_rng(9), 1500)
    # END before the body is long enough: REJECTED | ENDED, and the live side has nothing: UNDECIDABLE
    want = GR.run_script(ora, RNA, 8, TARGETS, polya(), GR.rule_of(5, 200, 20.0, 0, 64), cut_ops(x[:900], [300] * 3), 1)
    g, i = want[-1]["gate"][0], want[-1]["info"][0]
    assert (g["state"], g["flags"], g["t0"], g["released"], g["ring"]) == (GR.REJECTED, GR.ENDED, -1, 0, 0)
    assert (i["state"], i["events"], i["ended"]) == (LR.UNDECIDABLE, 0, 1) and g["decided_n"] == 900
    # give up at 600 samples: REJECTED with no flag, the live side stays CALIBRATING with 0 events until the read ends
    want = GR.run_script(ora, RNA, 8, TARGETS, polya(), GR.rule_of(5, 200, 20.0, 600, 64), cut_ops(x, [300] * 5), 1)
    assert [int(w["gate"][0]["state"]) for w in want] == [GR.GATING] + [GR.REJECTED] * 4
    assert all(int(w["gate"][0]["decided_n"]) == 600 and int(w["hrec"][0]["n_used"]) == 600 for w in want[1:])
    assert [int(w["info"][0]["state"]) for w in want] == [LR.CALIBRATING] * 4 + [LR.UNDECIDABLE]
    assert want[-1]["gate"][0]["flags"] == 0 and want[-1]["gate"][0]["events_cut"] == len(detect_ref.events(x, RNA))


def test_cli_argument_errors():
    """squiggle_map_stream --polya_gate: what the parser refuses, before a file is opened or a device looked for"""
    from squigglekit_amd.mapstream_cli import build_parser, main
    from test_cli import run_cli
    base = ["--i16", "x.npy", "-m", "ref.model", "--calib", "8"]
    gate = ["--live", "--polya_gate"]
    for argv, msg in ((base + gate + ["--gate_hold", "0"], "--gate_hold must be in 1 .. 4096"),
                      (base + gate + ["--gate_hold", "4097"], "--gate_hold must be in 1 .. 4096"),
                      (base + gate + ["--min_body", "0"], "--min_body must be at least 1"),
                      (base + gate + ["--gate_margin", "nan"], "--gate_margin must be a number"),
                      (base + gate + ["--gate_hold", "4096", "--sample_chunk", "61433"], "--calib + --gate_hold + --sample_chunk"),
                      (base + gate + ["--gate_preset", "dna"], "invalid choice"),
                      (base + ["--polya_gate"], "--polya_gate needs --live"),
                      (base + ["--polya_gate", "--fused"], "--fused needs --live")):
        so, se, code = run_cli(main, argv)
        assert code == 2 and msg in se and (so == "" or so.startswith("usage")), (argv, se)
    a = build_parser().parse_args(base + gate)
    assert (a.gate_preset, a.gate_model, a.min_body, a.gate_margin, a.gate_give_up, a.gate_hold) == ("rna_pa", None, 2000, 20.0, 0, 1024)
    assert (a.min_margin, a.give_up) == (0.05, 400)                     # the mapping rule's flags keep their names


def test_the_decision_is_polya_decides_on_every_prefix():
    """200 tie-heavy models with integer samples: every score is an exact integer, margins land on the threshold"""
    from squigglekit_amd import api
    seen = {1: 0, 0: 0, -1: 0}
    equal_margin = 0
    for case in range(200):
        rng = np.random.default_rng(5000 + case)
        model = HR.tie_model(rng)
        S = model["nstates"]
        s = int(rng.integers(0, S))
        rule = GR.rule_of(s, int(rng.integers(1, 6)), float(rng.integers(-2, 4)), int(rng.choice([0, 0, 9, 20])), 4)
        n = int(rng.integers(5, 40))
        x = rng.integers(-1, 5, n).astype(np.int16)
        sess = HR.Session(model, 1)
        gate = GR.Gate(4)
        none = np.zeros(0, dtype=detect_ref.DTYPE)
        state = GR.GATING
        for t in range(n):
            rec = sess.push([0], [x[t:t + 1]], "i16")
            # api.polya_decide reads TRANSCRIPT = 5: hand it the record with states s and 5 exchanged
            r2 = rec.copy()
            r2["v"][:, [s, 5]] = rec["v"][:, [5, s]]
            r2["enter"][:, [s, 5]] = rec["enter"][:, [5, s]]
            f = int(rec["final_state"][0])
            r2["final_state"][0] = 5 if f == s else (s if f == 5 else f)
            dec = int(api.polya_decide(r2, rule["min_body"], rule["min_margin"], rule["give_up"])[0])
            assert GR.accept(rec[0], rule) == (dec == 1), (case, t)
            with np.errstate(invalid="ignore"):
                equal_margin += int(rec["v"][0][s] - np.delete(rec["v"][0], s).max() == rule["min_margin"])
            if state == GR.GATING:
                state = {1: GR.OPEN, -1: GR.REJECTED, 0: GR.GATING}[dec]
                seen[dec] += 1
                t0 = int(rec["enter"][0][s]) if dec == 1 else -1
                decided = t + 1 if dec else -1
            gate.take(rec[0], none, False, rule)
            assert (gate.state, gate.t0, gate.decided_n) == (state, t0, decided), (case, t)
            if state != GR.GATING:
                break
    assert seen[1] >= 30 and seen[-1] >= 10 and seen[0] >= 500 and equal_margin >= 20, (seen, equal_margin)
