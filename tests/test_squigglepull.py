"""SquigglePull drop-in (SquigglePull.py:70-253): squigglekit_amd/squigglepull_cli.py over csrc/sk_pull.hip.

CPU: the reference's runs (goldens: tools/gen_golden_pull.py) replayed through squigglepull_cli.main with the GPU
formatter replaced by numpy_pull_text below -- the reference's own formula, str(np.round((d + offset) * raw_unit, 2))
-- so the file walk, auto-detection, messages and partial lines are checked without a GPU; argument parsing; --blow5.
GPU: the same replay through HIP, and the kernel against numpy_pull_text byte for byte (ties, negative zeros, the
int16 range, odd lengths, a 1.2 M-sample read, 200 000 reads), the host and device entry points, overflow."""
import contextlib
import ctypes as C
import hashlib
import io
import os
import re
import shutil
import traceback

import numpy as np
import pytest

from conftest import GOLD, load_golden


def numpy_pull_text(rows, lens, prefixes, calib=None, raw=False, out=None):
    """What SquigglePull prints for these reads (SquigglePull.py:185-189, 238-253), evaluated by numpy."""
    from squigglekit_amd import api
    blob, off = api.pack_prefixes(prefixes)
    lines = []
    for r in range(len(lens)):
        d = np.asarray(rows[r, :lens[r]], dtype=int)
        if raw:
            toks = map(str, d.tolist())
        else:
            dig, ofs, rng = (float(v) for v in calib[r])
            rng = float("{0:.2f}".format(rng))
            toks = map(str, np.round((d + ofs) * (rng / dig), 2))
        lines.append(bytes(blob[off[r]:off[r + 1]]) + "\t".join(toks).encode() + b"\n")
    return b"".join(lines)


@pytest.fixture
def numpy_formatter(monkeypatch):
    from squigglekit_amd import api
    monkeypatch.setattr(api, "pull_text", numpy_pull_text)


def run(argv):
    """squigglepull_cli.main(argv): (stdout, stderr, exit code); an uncaught exception is reported as Python would."""
    from squigglekit_amd.squigglepull_cli import main
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code if isinstance(e.code, int) else 1
        except Exception:                                   # noqa: BLE001
            traceback.print_exc()
            code = 1
    return out.getvalue(), err.getvalue(), code


def _layout(tmp, gold):
    for dst, src in gold["layout"].items():
        os.makedirs(os.path.dirname(os.path.join(tmp, dst)), exist_ok=True)
        shutil.copyfile(os.path.join(GOLD, src), os.path.join(tmp, dst))
    os.makedirs(os.path.join(tmp, "bad"))
    with open(os.path.join(tmp, "bad", "broken.fast5"), "wb") as fh:
        fh.write(b"this is not an HDF5 file\n" * 40)
    with open(os.path.join(tmp, "bad", "notes.txt"), "w") as fh:
        fh.write("not a fast5\n")


_TB = re.compile(r"Traceback \(most recent call last\):\n(?:  .*\n)*(\S.*\n)")


def _stderr_norm(s, keep_exc):
    """Tracebacks name the files and lines of whoever raised (the reference's there, ours here): each is cut down to
    its last line (the exception; dropped too when h5py, not the built-in reader, raised it); the timer is masked."""
    s = _TB.sub(lambda m: "<traceback>" + (m.group(1) if keep_exc else "\n"), s)
    return re.sub(r"Time taken: \S+\n", "Time taken: <t>\n", s)


def _same_stdout(got, want):
    if "text" in want:
        return got == want["text"]
    b = got.encode("utf-8", "surrogateescape")
    return (len(b) == want["bytes"] and hashlib.sha256(b).hexdigest() == want["sha256"]
            and b[:len(want["head"])].decode() == want["head"] and b[-len(want["tail"]):].decode() == want["tail"])


def _replay(tmp_path):
    from squigglekit_amd import tsvio
    gold = load_golden("squigglepull_cli.json.gz")
    tmp = str(tmp_path)
    _layout(tmp, gold)
    keep_exc = not tsvio.have_h5py()
    for r in gold["runs"]:
        so, se, code = run([a.replace("<TMP>", tmp) for a in r["argv"]])
        so, se = so.replace(tmp, "<TMP>"), se.replace(tmp, "<TMP>")
        assert code == r["exit"], (r["argv"], code, se[-300:])
        assert _same_stdout(so, r["stdout"]), (r["argv"], so[:200], so[-200:])
        assert _stderr_norm(se, keep_exc) == _stderr_norm(r["stderr"], keep_exc), (r["argv"], se[-400:], r["stderr"][-400:])
    return len(gold["runs"])


# ------------------------------------------------------------------------------------------------ CPU
def test_golden_replay_cpu(numpy_formatter, tmp_path):
    assert _replay(tmp_path) >= 14


def test_arguments_and_help():
    from squigglekit_amd.squigglepull_cli import build_parser
    p = build_parser()
    a = p.parse_args(["-p", "d"])
    assert (a.path, a.type, a.verbose, a.raw_signal, a.extra_info, a.blow5) == ("d", "auto", False, False, False, None)
    a = p.parse_args(["--path", "d", "--type", "multi", "--verbose", "--raw_signal", "--extra_info"])
    assert (a.type, a.verbose, a.raw_signal, a.extra_info) == ("multi", True, True, True)
    assert p.parse_args(["--blow5", "x.blow5"]).blow5 == "x.blow5"
    h = p.format_help()
    assert h.startswith("usage: SquigglePull.py [-h] [-p PATH] [-t {auto,single,multi}] [-v] [-r] [-i]\n")
    assert "blow5" not in h                                   # (hidden: the help text stays the reference's)
    gold = {tuple(r["argv"]): r for r in load_golden("squigglepull_cli.json.gz")["runs"]}
    assert gold[()]["stderr"] == h and gold[()]["exit"] == 1
    assert gold[("--bogus",)]["stdout"]["text"] == h and gold[("--bogus",)]["exit"] == 2


def _blow5_vs_fast5(tmp_path, flags):
    d = tmp_path / ("f5" + "".join(flags))
    d.mkdir()
    shutil.copyfile(os.path.join(GOLD, "example_test.fast5"), d / "example_test.fast5")
    so5, se5, c5 = run(["-p", str(d)] + flags)
    sob, seb, cb = run(["--blow5", os.path.join(GOLD, "example_0.blow5")] + flags)
    assert c5 == cb == 0 and se5 == seb == "", (se5, seb)
    assert so5.count("\n") == sob.count("\n") == 1
    assert sob.startswith("example_0.blow5\t")
    assert so5.split("\t", 1)[1] == sob.split("\t", 1)[1]
    return sob


def test_blow5_route_cpu(numpy_formatter, tmp_path):
    line = _blow5_vs_fast5(tmp_path, [])
    want = [r for r in load_golden("squigglepull_cli.json.gz")["runs"] if r["argv"] == ["-p", "<TMP>/single", "-t", "single"]][0]
    assert _same_stdout(line.replace("example_0.blow5\t", "example_test.fast5\t", 1), want["stdout"])
    for flags in (["-r"], ["-i"], ["-r", "-i"]):
        _blow5_vs_fast5(tmp_path, flags)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_golden_replay_gpu(gpu, tmp_path):
    assert _replay(tmp_path) >= 14


@pytest.mark.gpu
def test_blow5_route_gpu(gpu, tmp_path):
    for flags in ([], ["-r"], ["-i"], ["-r", "-i"]):
        _blow5_vs_fast5(tmp_path, flags)


def _prefixes(n, tag="r"):
    return [("file.fast5\t%s%d\t" % (tag, i)).encode() for i in range(n)]


def _check(rows, lens, calib=None, raw=False, prefixes=None):
    from squigglekit_amd import api
    prefixes = prefixes or _prefixes(len(lens))
    got = api.pull_text(rows, lens, prefixes, calib=calib, raw=raw)
    want = numpy_pull_text(rows, lens, prefixes, calib=calib, raw=raw)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = next(i for i in range(min(len(g), len(w))) if g[i] != w[i]) if len(g) == len(w) else -1
        pytest.fail("text differs (%d vs %d bytes), first differing line %d: %r / %r" % (
            len(got), len(want), bad, g[bad][:200] if bad >= 0 else b"", w[bad][:200] if bad >= 0 else b""))
    return got


@pytest.mark.gpu
def test_kernel_matches_numpy_seeded_reads(gpu):
    rng = np.random.default_rng(20261016)
    R, N = 2000, 4000
    rows = rng.integers(-2000, 3000, size=(R, N)).astype(np.int16)
    lens = np.full(R, N, dtype=np.int32)
    calib = np.stack([np.full(R, 8192.0), rng.uniform(-40, 40, R), rng.uniform(20, 2000, R)], axis=1)
    calib[::7, 1] = 16.0                                       # integer offsets too
    calib[::5, 2] = rng.uniform(0.004, 0.02, R)[::5]           # tiny ranges: many values round to 0 and to -0.0
    calib[::11, 0] = 2048.0
    text = _check(rows, lens, calib)
    assert b"\t-0.0\t" in text and b"\t0.0\t" in text


@pytest.mark.gpu
def test_kernel_ties_and_negative_zero(gpu):
    d = np.arange(-200, 200, dtype=np.int16)
    rows = np.tile(d, (4, 1))
    lens = np.full(4, len(d), dtype=np.int32)
    calib = np.array([[8192.0, 16.0, 1024.0], [8192.0, 0.5, 1024.0], [8192.0, -16.0, 1.0], [4096.0, 0.25, 0.5]])
    text = _check(rows, lens, calib)
    line0 = text.split(b"\n")[0].split(b"\t")[2:]
    assert [line0[int(i) + 200] for i in (-17, -15, 3)] == [b"-0.12", b"0.12", b"2.38"]   # ties to even
    assert b"-0.0" in text


@pytest.mark.gpu
def test_kernel_raw_full_int16_range(gpu):
    d = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    rows = d.reshape(16, 4096)
    text = _check(rows, np.full(16, 4096, dtype=np.int32), raw=True)
    assert b"\t-32768\t" in text and b"\t32767\n" in text
    calib = np.tile([8192.0, 7.25, 1467.61], (16, 1))
    _check(rows, np.full(16, 4096, dtype=np.int32), calib)


@pytest.mark.gpu
def test_kernel_odd_lengths_and_a_long_read(gpu):
    rng = np.random.default_rng(7)
    lens = np.array([0, 1, 63, 64, 65, 4097, 0, 255, 256, 257, 511, 513], dtype=np.int32)
    rows = rng.integers(-32768, 32768, size=(len(lens), 4100)).astype(np.int16)
    calib = np.stack([np.full(len(lens), 8192.0), rng.uniform(-20, 20, len(lens)), rng.uniform(10, 3000, len(lens))], axis=1)
    for raw in (False, True):
        text = _check(rows, lens, calib, raw=raw)
        assert text.startswith(b"file.fast5\tr0\t\nfile.fast5\tr1\t")
    long_n = 1200001
    R = 9
    rows = rng.integers(0, 1200, size=(R, long_n)).astype(np.int16)
    lens = rng.integers(0, 300, size=R).astype(np.int32)
    lens[4] = long_n
    calib = np.tile([8192.0, 16.0, 1493.94], (R, 1))
    _check(rows, lens, calib)
    _check(rows, lens, raw=True)


@pytest.mark.gpu
def test_many_reads_cross_workgroups(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(11)
    R = 200003
    rows = rng.integers(-1000, 1000, size=(R, 40)).astype(np.int16)
    lens = rng.integers(0, 41, size=R).astype(np.int32)
    calib = np.stack([np.full(R, 8192.0), rng.uniform(-30, 30, R), rng.uniform(100, 2000, R)], axis=1)
    prefixes = _prefixes(R)
    for raw in (False, True):
        text = api.pull_text(rows, lens, prefixes, calib=calib, raw=raw)
        starts = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == ord("\n")) + 1
        assert len(starts) == R and starts[-1] == len(text)
        off = np.concatenate([[0], starts])
        for r in list(range(0, R, 997)) + [R - 1]:
            want = numpy_pull_text(rows[r:r + 1], lens[r:r + 1], [prefixes[r]], calib=calib[r:r + 1], raw=raw)
            assert text[off[r]:off[r + 1]] == want, r


@pytest.mark.gpu
def test_host_and_dev_entry_points_and_overflow(gpu):
    from squigglekit_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(3)
    R, S = 300, 700
    rows = rng.integers(-500, 900, size=(R, S)).astype(np.int16)
    lens = rng.integers(0, S + 1, size=R).astype(np.int32)
    calib = np.stack([np.full(R, 8192.0), rng.uniform(-20, 20, R), rng.uniform(100, 2000, R)], axis=1)
    blob, poff = api.pack_prefixes(_prefixes(R, "dev"))
    pbuf = np.frombuffer(blob, dtype=np.uint8)
    ptr = _lib.ptr
    for mode in (_lib.SK_PULL_PA, _lib.SK_PULL_RAW):
        want = numpy_pull_text(rows, lens, (blob, poff), calib=calib, raw=mode == _lib.SK_PULL_RAW)
        n = len(want)
        total = C.c_int64(-1)
        # host form, capacity one byte short: the needed size comes back, nothing is written
        buf = np.full(n + 64, 0xA5, dtype=np.uint8)
        rc = L.sk_pull_text(ptr(rows), S, ptr(lens), R, ptr(calib), mode, ptr(pbuf), ptr(poff), ptr(buf), n - 1,
                            C.byref(total), None)
        assert rc == _lib.SK_ERR_OVERFLOW and total.value == n
        assert np.all(buf == 0xA5)
        line_off = np.zeros(R + 1, dtype=np.int64)
        rc = L.sk_pull_text(ptr(rows), S, ptr(lens), R, ptr(calib), mode, ptr(pbuf), ptr(poff), ptr(buf), n,
                            C.byref(total), ptr(line_off))
        assert rc == 0 and total.value == n and buf[:n].tobytes() == want and np.all(buf[n:] == 0xA5)
        assert line_off[-1] == n and np.all(np.diff(line_off) > 0)
        # device form
        cal2 = np.zeros((R, 2))
        assert L.sk_pa_calib(ptr(calib), R, ptr(cal2)) == 0
        d = {k: L.sk_dev_alloc(a.nbytes) for k, a in (("rows", rows), ("lens", lens), ("cal", cal2), ("pre", pbuf),
                                                        ("poff", poff), ("off", line_off))}
        d_text = L.sk_dev_alloc(n + 64)
        try:
            for k, a in (("rows", rows), ("lens", lens), ("cal", cal2), ("pre", pbuf), ("poff", poff)):
                assert L.sk_dev_upload(d[k], ptr(a), a.nbytes) == 0
            fill = np.full(n + 64, 0x5A, dtype=np.uint8)
            assert L.sk_dev_upload(d_text, ptr(fill), fill.nbytes) == 0
            dcal = d["cal"] if mode == _lib.SK_PULL_PA else None
            rc = L.sk_pull_text_dev(d["rows"], S, d["lens"], R, dcal, mode, d["pre"], d["poff"], d_text, n - 1,
                                    C.byref(total), d["off"])
            assert rc == _lib.SK_ERR_OVERFLOW and total.value == n
            back = np.zeros(n + 64, dtype=np.uint8)
            assert L.sk_dev_download(ptr(back), d_text, back.nbytes) == 0 and np.all(back == 0x5A)
            rc = L.sk_pull_text_dev(d["rows"], S, d["lens"], R, dcal, mode, d["pre"], d["poff"], d_text, n,
                                    C.byref(total), d["off"])
            assert rc == 0 and L.sk_sync() == 0 and total.value == n
            assert L.sk_dev_download(ptr(back), d_text, back.nbytes) == 0
            assert back[:n].tobytes() == want and np.all(back[n:] == 0x5A)
            off2 = np.zeros(R + 1, dtype=np.int64)
            assert L.sk_dev_download(ptr(off2), d["off"], off2.nbytes) == 0 and np.array_equal(off2, line_off)
        finally:
            for p in list(d.values()) + [d_text]:
                L.sk_dev_free(p)
    # bad arguments
    assert L.sk_pull_text(ptr(rows), S, ptr(lens), R, ptr(calib), 7, ptr(pbuf), ptr(poff), ptr(buf), n,
                          C.byref(total), None) == _lib.SK_ERR_INVALID
    assert L.sk_pull_text(ptr(rows), S, ptr(lens), R, None, _lib.SK_PULL_PA, ptr(pbuf), ptr(poff), ptr(buf), n,
                          C.byref(total), None) == _lib.SK_ERR_INVALID
    bad = calib.copy()
    bad[int(np.argmax(lens)), 0] = 0.0                                            # digitisation 0: raw_unit = inf, numpy would print inf
    assert L.sk_pull_text(ptr(rows), S, ptr(lens), R, ptr(bad), _lib.SK_PULL_PA, ptr(pbuf), ptr(poff), ptr(buf),
                          buf.nbytes, C.byref(total), None) == _lib.SK_ERR_UNSUPPORTED
