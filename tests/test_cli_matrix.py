"""The MotifSeq command line over input routes x flag sets (tools/gen_cli_matrix.py): stdout, stderr, the exit code and
every side file of each case against the recording in tests/golden/motifseq_cli_matrix.json.gz.

GPU leg: the whole matrix.  CPU leg: the cases the oracle stand-ins of test_cli.py can answer -- first match over the
TSV routes -- against the same recording, so the harness (routing, ordering, scoring, formatting, messages) is held
without a GPU."""
import pytest

from conftest import load_golden
from test_cli import oracle_backend      # noqa: F401  (fixture)
from tools import gen_cli_matrix as matrix


def check(tmp_path, which):
    from squigglekit_amd.motifseq_cli import main
    gold = load_golden("motifseq_cli_matrix.json.gz")["runs"]
    got = matrix.run_matrix(main, str(tmp_path), which)
    assert which is not None or sorted(got) == sorted(gold)
    for name, run in got.items():
        want = gold[name]
        for part in ("argv", "exit", "stdout", "stderr", "files"):
            assert run[part] == want[part], (name, part)
    return got


def test_matrix_is_the_recorded_one():
    """every case of the matrix has its recording, and nothing else is recorded"""
    gold = load_golden("motifseq_cli_matrix.json.gz")["runs"]
    assert [c[0] for c in matrix.cases()] == list(gold)
    assert len(gold) >= 130


def test_cli_matrix_cpu(oracle_backend, tmp_path):      # noqa: F811
    which = matrix.cpu_cases()
    assert len(which) == 5 * 5 + 2                       # six flag sets x five routes, -x on two of them
    check(tmp_path, which)


@pytest.mark.gpu
def test_cli_matrix_gpu(gpu, tmp_path):
    check(tmp_path, None)
