"""GPU: dRNA_polya_stream.py --min_post (squigglekit_amd/polya_stream_cli.py), the replay of a file through a filtered HMM
session, against dRNA_polya.py --posterior on the same input; and without the new flags, against what the tool printed
before it had them."""
import numpy as np
import pytest

import hmmstream_ref as HR
from test_gpu_hmmstream_cli import table
from test_gpu_mapstream import run_cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """(reads.npy, reads int16 [5, 1200]): shrunk direct-RNA reads in the synth_raw preset's units"""
    rng = np.random.default_rng(20261022)
    reads = np.stack([HR.small_drna_read(rng, 1200) for _ in range(5)])
    path = tmp_path_factory.mktemp("hmmfilter") / "reads.npy"
    np.save(path, reads)
    return str(path), reads


@pytest.mark.parametrize("chunk", [2000, 333])
def test_reads_that_run_to_their_end_print_the_posterior_columns_of_the_one_shot_tool(gpu, synthetic, chunk):
    """a --min_body above any read length: every read prints `end`; its first seven columns are dRNA_polya.py's, the two
    new ones are dRNA_polya.py --posterior's loglik_per_sample and p_transcript, text for text.  Without --min_post the
    lines are the first ten columns, as before."""
    from squigglekit_amd.polya_cli import main as polya_main
    from squigglekit_amd.polya_stream_cli import main as stream_main
    base = ["--i16", synthetic[0], "--preset", "synth_raw"]
    want, err, code = run_cli(polya_main, base + ["--posterior"])
    assert code == 0, err[-300:]
    live = ["--sample_chunk", str(chunk), "--channels", "3", "--give_up", "0", "--min_body", "1000000000"]
    got, err, code = run_cli(stream_main, base + live + ["--min_post", "0.99"])
    assert code == 0, err[-300:]
    plain, err, code = run_cli(stream_main, base + live)
    assert code == 0, err[-300:]
    want, got, plain = table(want), table(got), table(plain)
    assert sorted(got) == sorted(want) == sorted(plain) == sorted(str(r) for r in range(5))
    for rid, cols in got.items():
        w = want[rid]
        assert len(w) == 10 and len(cols) == 12, (cols, w)
        assert cols[:7] == w[:7] and cols[7] == "end" and int(cols[9]) == 1200, (cols, w)
        assert cols[10:] == [w[7], w[9]], (cols, w)                      # loglik_per_sample, p_transcript (w[8]: polya_expected)
        assert float(cols[11]) > 0.5 and cols[10] != "."
        assert plain[rid] == cols[:10]


def test_accepts_by_probability_where_the_statement_does(gpu, synthetic):
    """a small --min_body: the numpy replay (tests/hmmfilter_ref.py with api.polya_decide_post) accepts every read, at least
    one before its samples run out, and the tool prints the replay's lines; --min_margin changes nothing"""
    import hmmfilter_ref as FR
    from squigglekit_amd import api
    from squigglekit_amd.polya_cli import polya_lines
    from squigglekit_amd.polya_stream_cli import filter_columns, main as stream_main
    path, reads = synthetic
    chunk, body, min_post = 150, 100, 0.99
    model = api.polya_model("synth_raw")
    want = {}
    for r, x in enumerate(reads):
        ref = FR.Session(model, 1)
        for at in range(0, len(x), chunk):
            rec = ref.push([0], [x[at:at + chunk]], "i16")
            filt = ref.filter([0])
            if api.polya_decide_post(rec, filt, body, min_post, 0)[0] == 1:
                break
        assert api.polya_decide_post(rec, filt, body, min_post, 0)[0] == 1, (r, rec, filt)
        want[str(r)] = (polya_lines([str(r)], rec)[0].rstrip("\n").split("\t")
                        + ["accept", str(int(rec["pushes"][0])), str(int(rec["n_used"][0]))] + filter_columns(filt))
    assert any(int(w[9]) < reads.shape[1] for w in want.values())
    for margin in ("20", "1e9"):
        got, err, code = run_cli(stream_main, ["--i16", path, "--preset", "synth_raw", "--sample_chunk", str(chunk), "--channels", "4",
                                               "--min_body", str(body), "--min_post", str(min_post), "--min_margin", margin])
        assert code == 0, err[-300:]
        assert table(got) == want
