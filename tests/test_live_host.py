"""CPU: the live-session statement of tests/live_ref.py against the two things it must agree with -- the normalisation
squiggle_map_stream applies to a whole read (mapstream_cli.normalise: whatever the cuts, an ended read is handed exactly
those values, or is undecidable exactly when that returns None) and api.map_decide (the decision summary) -- and the
parser errors of --fused.  Nothing here needs a device."""
import numpy as np
import pytest

import detect_ref
import evstream_ref as ER
import live_ref as LR

TARGETS = [np.sin(np.arange(n) * 0.37) * 1.3 for n in (23, 41)]


@pytest.mark.parametrize("seed", range(20))
def test_an_ended_read_is_handed_the_normalised_levels_of_the_whole_read(ora, seed):
    from squigglekit_amd.mapstream_cli import normalise
    rng = np.random.default_rng(9000 + seed)
    sess = ER.draw_session(rng, nslots=int(rng.choice([1, 3, 7])), budget=2500, maxlen=int(rng.choice([40, 150, 300])))
    C = int(rng.choice([2, 3, 5, 9, 40]))
    params, S, ops = sess["params"], sess["nslots"], sess["ops"]
    rule = (int(rng.integers(0, 30)), float(rng.uniform(0.2, 3.0)), float(rng.uniform(-0.1, 0.3)), int(rng.integers(1, 60)))
    want = LR.run_script(ora, params, C, TARGETS, ops, S, rule)
    from squigglekit_amd import api
    had = [[[], [], False] for _ in range(S)]                           # per slot: sample chunks, z chunks, closed
    checked = undecidable = 0
    for op, w in zip(ops, want):
        if op[0] == "reset":
            for s in op[1]:
                had[s] = [[], [], False]
            continue
        _, slots, chunks, end = op
        # the decision summary is api.map_decide on the same records
        best, dec = api.map_decide(w["rec"], *rule)
        assert np.array_equal(w["best"]["target"], best) and np.array_equal(w["best"]["decision"], dec)
        for i, (s, c, e) in enumerate(zip(slots, chunks, end)):
            z = w["z"][w["off"][i]:w["off"][i + 1]]
            if had[s][2]:
                assert len(z) == 0 and w["info"]["new_events"][i] == 0
                continue
            had[s][0].append(np.asarray(c, dtype=np.int16))
            had[s][1].append(z)
            if not e:
                continue
            had[s][2] = True
            x = np.concatenate(had[s][0])
            ev = detect_ref.events(x, params)
            whole = normalise(LR.levels_of(ev), C)
            got = np.concatenate(had[s][1])
            state = int(w["info"]["state"][i])
            if whole is None:
                assert state == LR.UNDECIDABLE and len(got) == 0 and np.isnan(w["info"]["mean"][i])
                undecidable += 1
            else:
                assert state == LR.MAPPING and got.tobytes() == whole.tobytes(), (seed, int(s), len(got), len(whole))
                assert w["info"]["mapped"][i] == w["info"]["events"][i] == len(ev) and w["rec"]["rows"][0, i] == len(ev)
            checked += 1
    assert checked >= S                                                # (the closing push ends every slot)


def test_best_of_second_target_follows_map_lines():
    """second_target is np.argmin of the column with the best set to +inf -- 0 when nothing else has a distance, the best
    itself included -- and -1 with one target; an entry without a distance waits"""
    rec = np.zeros((3, 4), dtype=LR.MR.MAPREC)
    rec["dist"] = [[5.0, np.nan, 2.0, np.nan], [1.0, np.nan, 2.0, 7.0], [1.0, np.nan, 9.0, np.nan]]
    rec["rows"] = [[10, 0, 10, 10]] * 3
    b = LR.best_of(rec, (0, 10.0, 0.0, 1))
    assert b["target"].tolist() == [1, -1, 0, 1] and b["second_target"].tolist() == [2, 0, 1, 0]
    assert b["decision"].tolist() == [1, 0, 1, 1] and np.isnan(b["dist"][1]) and np.isnan(b["second_dist"][3])
    one = LR.best_of(rec[:1], (0, 0.1, 0.0, 5))
    assert one["second_target"].tolist() == [-1] * 4 and one["decision"].tolist() == [-1, 0, -1, 0]


def test_fused_parser_errors(capsys):
    """--fused without --live and --fused with a --calib above SK_LIVE_MAX_CALIB: parser errors, before any input or device
    is looked at"""
    from squigglekit_amd import _lib
    from squigglekit_amd.mapstream_cli import main
    base = ["--i16", "no-such.npy", "-m", "no-such.model"]
    for extra, word in ((["--fused"], "--fused needs --live"),
                        (["--fused", "--calib", "40"], "--fused needs --live"),
                        (["--live", "--fused", "--calib", str(_lib.SK_LIVE_MAX_CALIB + 1)], "--calib must be at most 8192"),
                        (["--live", "--fused", "--calib", "1"], "--live needs --calib >= 2")):
        with pytest.raises(SystemExit) as ei:
            main(base + extra)
        first = capsys.readouterr().err.split("\n")[0]
        assert ei.value.code == 2 and first.startswith("error: ") and word in first, (extra, first)
