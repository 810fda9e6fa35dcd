"""GPU: ten seeded random gated live sessions against tests/livegate_ref.py after every push -- drawn slot counts, cuts,
ENDs, resets with and without calibration pairs, ring lengths, calibration lengths and gate rules; tie-heavy integer
models and synth_raw direct-RNA reads.  On failure the script is printed.  Over the ten sessions at least half of the
reads open their gate; that count comes from the reference alone, not from what the library returns."""
import numpy as np
import pytest

import detect_ref
import hmmstream_ref as HR
import livegate_ref as GR

pytestmark = pytest.mark.gpu

# 1, 3, 8 and 66 slots; three tie models (one never opens, one gives up); rings of 1 .. 64; calib 2 .. 129.  By the reference
# 547 of the 672 reads of these ten scripts open their gate.
SEEDS = (9100, 9101, 9103, 9104, 9107, 9109, 9112, 9115, 9120, 9123)
_rng = np.random.default_rng(99)
TARGETS = [_rng.normal(size=n) for n in (300, 520)]
LIVE_RULE = (30, 1.5, 0.01, 90)
EMPTY = np.zeros(0, dtype=np.int16)
_opened = {}


def draw_session(seed):
    """{"params", "calib", "model", "rule", "nslots", "ops", "reads"}: reads counts the reads that were given a sample"""
    rng = np.random.default_rng(seed)
    tie = rng.random() < 0.3
    S = int(rng.choice([1, 3, 8, 66]))
    hold = int(rng.choice([1, 4, 16, 64]))
    calib = int(rng.choice([2, 8, 20, 129]))
    if tie:
        model = HR.tie_model(rng, S=int(rng.integers(3, 7)))
        rule = GR.rule_of(int(rng.integers(0, model["nstates"])), int(rng.choice([1, 5, 17])), float(rng.choice([0, 1, 2])),
                          int(rng.choice([0, 200])), hold)
        params = detect_ref.PRESETS["dna"]
    else:
        from squigglekit_amd import api
        model = api.polya_model("synth_raw")
        rule = GR.rule_of(5, int(rng.choice([50, 200, 300])), 20.0, int(rng.choice([0, 0, 1400])), hold)
        params = detect_ref.PRESETS[str(rng.choice(["rna", "rna", "dna"]))]

    def new_read(with_pair):
        """(samples, pair): with a pair the samples are in other units and the pair takes them back, exactly"""
        if tie:
            x = rng.integers(-1, 5, int(rng.integers(200, 500))).astype(np.int16)
            return (x - 1).astype(np.int16) if with_pair else x, (1.0, 1.0) if with_pair else None
        x = HR.small_drna_read(rng, int(rng.choice([1200, 1500, 2000])))
        return (2 * x.astype(np.int32) + 6).astype(np.int16) if with_pair else x, (-6.0, 0.5) if with_pair else None

    budget = 16000 if S < 66 else 130000
    cur = [list(new_read(False)) + [0, False] for _ in range(S)]       # per slot: samples, pair, position, ended
    ops, used, nreads = [], 0, S
    sizes = [0, 1, 64, 150, 200, 400, 400] if not tie else [0, 1, 7, 37, 64, 100]
    while used < budget:
        k = int(rng.integers(1, S + 1)) if rng.random() < 0.5 else S
        slots = rng.permutation(S)[:k].astype(np.int32)
        if rng.random() < 0.04:
            slots = slots[:3]
            k = len(slots)
            pairs = rng.random() < 0.5
            for s in slots:
                cur[s] = list(new_read(pairs)) + [0, False]
            nreads += k
            ops.append(("reset", slots, np.array([cur[s][1] for s in slots], dtype=np.float64) if pairs else None))
            continue
        chunks, end = [], []
        for s in slots:
            x, _, at, ended = cur[s]
            n = 0 if ended else min(int(rng.choice(sizes)), len(x) - at)
            chunks.append(x[at:at + n])
            cur[s][2] = at + n
            e = not ended and (at + n >= len(x) or rng.random() < 0.004)
            end.append(int(e))
            cur[s][3] = ended or e
            used += n
        ops.append(("push", slots, chunks, np.array(end, dtype=np.int32)))
        used += 1
        if all(c[3] for c in cur) and used < budget:                    # every read has ended: new ones all round
            every = np.arange(S, dtype=np.int32)
            for s in every:
                cur[s] = list(new_read(False)) + [0, False]
            nreads += S
            ops.append(("reset", every, None))
    while not all(c[3] for c in cur):                                   # the reads in progress run to their ends
        slots = np.array([s for s in range(S) if not cur[s][3]], dtype=np.int32)
        chunks = [cur[s][0][cur[s][2]:cur[s][2] + sizes[-1]] for s in slots]
        for s, c in zip(slots, chunks):
            cur[s][2] += len(c)
            cur[s][3] = cur[s][2] >= len(cur[s][0])
        ops.append(("push", slots, chunks, np.array([int(cur[s][3]) for s in slots], dtype=np.int32)))
    ops.append(("push", np.arange(S, dtype=np.int32), [EMPTY] * S, np.ones(S, dtype=np.int32)))
    return {"params": params, "calib": calib, "model": model, "rule": rule, "nslots": S, "ops": ops, "reads": nreads}


def reads_opened(sess, want):
    """how many reads of the script reached OPEN, by the reference's gate records"""
    state = {}
    count = 0
    for op, w in zip(sess["ops"], want):
        if op[0] == "reset":
            for s in op[1]:
                count += state.pop(int(s), 0)
            continue
        for i, s in enumerate(op[1]):
            state[int(s)] = int(w["gate"]["state"][i] == GR.OPEN)
    return count + sum(state.values())


@pytest.mark.parametrize("seed", SEEDS)
def test_random_session(gpu, ora, seed):
    from squigglekit_amd import api
    sess = draw_session(seed)
    want = GR.run_script(ora, sess["params"], sess["calib"], TARGETS, sess["model"], sess["rule"], sess["ops"], sess["nslots"], LIVE_RULE)
    _opened[seed] = (reads_opened(sess, want), sess["reads"])
    GR.play(api, ora, sess["params"], sess["calib"], TARGETS, sess["model"], sess["rule"], sess["ops"], sess["nslots"], LIVE_RULE,
            label="seed %d" % seed, want=want)
    assert api.last_event_plan()["guard_hits"] == 0 and api.last_hmm_stream_plan()["guard_hits"] == 0


def test_half_of_the_reads_open_their_gate(gpu, ora):
    """(after the sessions above when the file runs in order; it computes what is missing itself)"""
    for seed in SEEDS:
        if seed not in _opened:
            sess = draw_session(seed)
            want = GR.run_script(ora, sess["params"], sess["calib"], TARGETS, sess["model"], sess["rule"], sess["ops"], sess["nslots"])
            _opened[seed] = (reads_opened(sess, want), sess["reads"])
    opened, reads = sum(v[0] for v in _opened.values()), sum(v[1] for v in _opened.values())
    assert 2 * opened >= reads, _opened
