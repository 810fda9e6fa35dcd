"""CPU: the two facts the event sessions rest on, and the reference session itself (tests/evstream_ref.py).

Fact 1: detect_ref.marks() returns strictly rising positions across both detectors together -- an event is final the
        moment its end is marked, nothing is buffered or sorted.
Fact 2: consecutive marks lie at least w_short // 2 + 1 apart -- k walked positions emit at most
        k // (w_short // 2 + 1) + 2 events, which sizes the staging rows of a push.
Then: the reference session's concatenation equals detect_ref.events for random cuts (lengths 0 and 1 and one cut per
sample among them), what a slot has emitted is a prefix of it after every push, and run_session's one walk per read
gives emitted()'s arrays.
"""
import numpy as np
import pytest

import detect_ref
import evstream_ref as ER

CORNERS = [detect_ref.PRESETS["dna"], detect_ref.PRESETS["rna"], (1, 1, 0.5, 2.0, 0.0), (1, 6, 1.0, 4.0, 0.0),
           (64, 64, 2.0, 3.0, 0.1), (64, 64, 1.0, 1.5, 0.0), (3, 6, 1.4, 9.0, 0.0), (19, 39, 2.0, 5.0, 1.0)]


def reads_and_params(seed, count, nmax):
    rng = np.random.default_rng(seed)
    for j in range(count):
        params = CORNERS[j % len(CORNERS)] if j < 2 * len(CORNERS) else ER.draw_params(rng)
        kind = ER.KINDS[j % 4]
        n = int(rng.integers(0, nmax)) if j % 7 else int(rng.choice([0, 1, 2 * params[0] - 1, 2 * params[1] - 1, 2 * params[1]]))
        yield params, kind, ER.draw_read(rng, n, kind)


def test_marks_with_steps_is_detect_refs_walk():
    for params, kind, x in reads_and_params(11, 40, 700):
        ms = ER.marks_with_steps(x, params)
        assert [p for p, _ in ms] == detect_ref.marks(x, params), (params, kind, len(x))
        assert all(st > p for p, st in ms)


def test_fact_1_marks_rise_strictly_across_both_detectors():
    total = 0
    for params, kind, x in reads_and_params(12, 120, 900):
        m = detect_ref.marks(x, params)
        total += len(m)
        assert all(b > a for a, b in zip(m, m[1:])), (params, kind, len(x), m[:20])
        assert all(0 < p < len(x) for p in m), (params, kind, len(x))
    assert total > 1500                                                # (the cases do mark)


def test_fact_2_marks_lie_a_half_window_apart_and_bound_a_push():
    for params, kind, x in reads_and_params(13, 120, 900):
        ms = ER.marks_with_steps(x, params)
        gap = params[0] // 2 + 1
        pos = [p for p, _ in ms]
        assert all(b - a >= gap for a, b in zip(pos, pos[1:])), (params, kind, len(x))
        # any stretch of k walked positions emits at most k // gap + 2 events
        steps = np.array([st for _, st in ms], dtype=np.int64)
        rng = np.random.default_rng(len(x))
        for _ in range(20):
            a = int(rng.integers(0, len(x) + 1))
            b = int(rng.integers(a, len(x) + 1))
            made = int(np.count_nonzero((steps >= a) & (steps < b)))
            assert made <= (b - a) // gap + 2, (params, kind, len(x), a, b, made)


def random_cuts(rng, n, style):
    if style == "each":
        return [1] * n
    cuts, left = [], n
    while left > 0:
        c = int(rng.choice([0, 1, int(rng.integers(0, 90)), int(rng.integers(0, 400))]))
        c = min(c, left)
        cuts.append(c)
        left -= c
    return cuts + [0]


@pytest.mark.parametrize("style", ["random", "each"])
def test_reference_session_concatenates_to_the_one_shot_events(style):
    for j, (params, kind, x) in enumerate(reads_and_params(14 if style == "random" else 15, 24, 260 if style == "each" else 900)):
        rng = np.random.default_rng(100 + j)
        cuts = random_cuts(rng, len(x), style)
        full = detect_ref.events(x, params)
        n, have = 0, 0
        for c in cuts:
            n += c
            got = ER.emitted(x[:n], params)
            assert len(got) >= have and got.tobytes() == full[:len(got)].tobytes(), (params, kind, len(x), n)
            have = len(got)
        assert n == len(x)
        assert ER.emitted(x, params, ended=True).tobytes() == full.tobytes()
        assert have <= len(full)


def test_short_reads_emit_only_at_the_end():
    for params in CORNERS:
        for n in (0, 1, 2 * params[0] - 1, 2 * params[1] - 1, 2 * params[1]):
            x = ER.draw_read(np.random.default_rng(n), n, "steps")
            assert len(ER.emitted(x[:min(n, params[1] - 1)], params)) == 0
            assert ER.emitted(x, params, ended=True).tobytes() == detect_ref.events(x, params).tobytes()


def test_cli_live_refuses_what_is_not_knowable_live(capsys):
    """--live needs --calib >= 2 and a positive --sample_chunk: parser errors, before any input or device is looked at"""
    from squigglekit_amd.mapstream_cli import main
    base = ["--i16", "no-such.npy", "-m", "no-such.model", "--live"]
    for extra, word in (([], "--calib"), (["--calib", "0"], "--calib"), (["--calib", "1"], "--calib"),
                        (["--calib", "10", "--sample_chunk", "0"], "--sample_chunk"),
                        (["--calib", "60000", "--sample_chunk", "6000"], "--calib + --sample_chunk")):
        with pytest.raises(SystemExit) as ei:
            main(base + extra)
        first = capsys.readouterr().err.split("\n")[0]
        assert ei.value.code == 2 and first.startswith("error: ") and word in first, (extra, first)


def test_run_session_is_emitted_on_every_prefix():
    for seed in range(6):
        rng = np.random.default_rng(500 + seed)
        sess = ER.draw_session(rng, nslots=int(rng.choice([1, 3, 5])), budget=2500)
        want = ER.run_session(sess)
        params = sess["params"]
        have = {s: (np.zeros(0, dtype=np.int16), False, 0) for s in range(sess["nslots"])}
        j = 0
        for op in sess["ops"]:
            if op[0] == "reset":
                for s in op[1]:
                    have[int(s)] = (np.zeros(0, dtype=np.int16), False, 0)
                continue
            off, rec = want[j]
            j += 1
            for i, (s, c, e) in enumerate(zip(op[1], op[2], op[3])):
                x, ended, out = have[int(s)]
                new = rec[off[i]:off[i + 1]]
                if ended:
                    assert len(new) == 0 and len(c) == 0
                    continue
                x = np.concatenate([x, c])
                all_now = ER.emitted(x, params, ended=bool(e))
                assert new.tobytes() == all_now[out:].tobytes(), (seed, j, int(s), ER.describe_session(sess))
                have[int(s)] = (x, bool(e), len(all_now))
        assert j == len(want)
