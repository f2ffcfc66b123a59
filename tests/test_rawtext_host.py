"""mapx/rawtext.py without a GPU: the Python restatement (tests/rawtext_ref.py) against the reference's own
read_feat() on the committed raw files (tests/golden/rawtext_*.npz, from gen_rawtext_golden.py), the bucket threshold
table against the expression it replaces, the hash-string code, the chunker, the line parser of csrc/rawtext_line.h
compiled for the CPU (tools/rawtext_host_check.cpp), and the refusals."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import rawtext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}


def _fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"rawtext_{name}.npz"))
    with open(os.path.join(golden_dir, RAW[name]), "rb") as f:
        return z, f.read()


def _as_fixture(col, want):
    """A parsed int64 column in the form read_feat() saved it: hash codes back to strings."""
    if want.dtype.kind == "U":
        return np.array([R.decode_hex(int(v)) for v in col])
    return col


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_restatement_equals_the_reference_fixture(golden_dir, name):
    """Licenses rawtext_ref as the expected value for synthetic inputs: on the committed raw files it gives exactly
    what the reference's read_feat() saved — labels, date parts, buckets, -1 for empty fields, hash strings."""
    from mapx import rawtext
    z, data = _fixture(golden_dir, name)
    schema = rawtext.SCHEMAS[name]
    labels, cols = R.parse(data, schema)
    assert [str(n) for n in z["names"]] == [schema.label] + list(cols) == schema.columns
    assert np.array_equal(labels, z["col/click"].astype(np.int64))
    for n, c in cols.items():
        want = z[f"col/{n}"]
        assert (want.dtype.kind == "U") == (n in schema.string_columns), n
        assert np.array_equal(_as_fixture(c, want), want), n
    if name == "criteo":
        assert len(R.lines(data)) == len(labels) == data.count(b"\n") - 1          # the blank line is skipped
        assert (cols["I1"] == -1).any() and (cols["C26"] == -1).any()


def test_dates_the_reference_cannot_read_follow_strptime():
    """00010100 is not in the fixture (pandas drops the leading zeros and the reference's to_datetime raises): the
    restatement's dates are Python's strptime, checked here at %y's pivot and on leap days."""
    from mapx import rawtext
    a = rawtext.AVAZU
    want = {b"00010100": (5, 1, 0, 1), b"99123123": (4, 31, 23, 0), b"16022912": (0, 29, 12, 0),
            b"68123100": (0, 31, 0, 0), b"69010100": (2, 1, 0, 0), b"00022923": (1, 29, 23, 0)}
    for tok, parts in want.items():
        row = R.parse_line(R.with_field(R.AVAZU_LINE, a, "hour", tok), a)
        assert tuple(row[1:5]) == parts, tok
    for tok in (b"14022900", b"00000100", b"14100024"[:7] + b"a"):
        with pytest.raises(R._Bad):
            R.parse_line(R.with_field(R.AVAZU_LINE, a, "hour", tok), a)


def test_threshold_table_equals_the_expression():
    from mapx import rawtext
    t = rawtext.bucket_thresholds()
    assert t.dtype == np.int64 and len(t) == 1906 and t[0] == 3 and bool((np.diff(t) > 0).all())
    v = np.arange(3, 200_001, dtype=np.int64)
    direct = np.floor(np.log(v) ** 2).astype(np.int64)                  # proc_criteo.py:30 over the whole range
    assert np.array_equal(np.searchsorted(t, v, side="right"), direct)
    for b, tb in enumerate(t.tolist(), start=1):                        # t - 1, t, t + 1 of every threshold
        for x in (tb - 1, tb, tb + 1):
            if x > 2:
                assert int(np.searchsorted(t, x, side="right")) == int(np.floor(np.log(int(x)) ** 2)) == rawtext.bucket_of(x), x
        assert rawtext.bucket_of(tb) == b and (tb == 3 or rawtext.bucket_of(tb - 1) == b - 1)
    assert [rawtext.bucket_of(x) for x in (-3, 0, 1, 2)] == [-3, 0, 1, 2]
    assert np.array_equal(R.bucket_array(v), direct)


def test_hex_code_is_a_bijection():
    from mapx import rawtext
    rng = np.random.RandomState(5)
    seen = {}
    for w in range(1, 15):
        toks = {"0" * w, "f" * w, "a" + "0" * (w - 1), "0" * (w - 1) + "a"}
        toks |= {"".join("0123456789abcdef"[d] for d in rng.randint(0, 16, w)) for _ in range(50)}
        for s in toks:
            code = rawtext.encode_hex(s)
            assert 0 < code < 2 ** 60 and code == R.hex_code(s.encode())
            assert rawtext.decode_hex(code) == s == R.decode_hex(code)
            assert seen.setdefault(code, s) == s                       # no two strings share a code
    assert rawtext.encode_hex("0a") != rawtext.encode_hex("a")
    assert rawtext.encode_hex("") == -1 and rawtext.decode_hex(-1) == "-1"
    for bad in ("A0", "g", "0" * 15, " 1", "+1", "1_0"):
        with pytest.raises(ValueError):
            rawtext.encode_hex(bad)
    assert rawtext.AVAZU.decoder("C20")(-1) == "-1" and rawtext.AVAZU.decoder("site_id")(rawtext.encode_hex("00ff")) == "00ff"


@pytest.mark.parametrize("final_newline", [True, False])
def test_chunker_keeps_lines_and_line_numbers(final_newline):
    from mapx import rawtext
    rng = np.random.RandomState(9)
    pieces = []
    for i in range(400):
        if i in (0, 1, 57, 58, 399) or rng.rand() < 0.05:
            pieces.append(b"" if i % 2 else b"\r")                     # blank lines, some with a carriage return
        else:
            pieces.append(b"%d,%s" % (i, b"x" * rng.randint(0, 50)))
    data = b"\n".join(pieces) + (b"\n" if final_newline else b"")
    whole = R.lines(data)
    for chunk_bytes in (64, 700, 4096, None):
        got, total = [], b""
        for chunk, line0 in rawtext.iter_chunks(io.BytesIO(data), chunk_bytes):
            assert chunk_bytes is None or len(chunk) <= chunk_bytes
            assert total.count(b"\n") == line0 and (chunk.endswith(b"\n") or total + chunk == data)
            got += [(line0 + no, line) for no, line in R.lines(chunk)]
            total += chunk
        assert total == data and got == whole, chunk_bytes
    with pytest.raises(ValueError, match="line 3 is longer"):
        list(rawtext.iter_chunks(io.BytesIO(b"a\nb\n" + b"x" * 100 + b"\nc\n"), 64))
    assert list(rawtext.iter_chunks(io.BytesIO(b""), 64)) == []
    assert rawtext.first_line(b"\n\r\n\nab\r\ncd\n") == b"ab" and rawtext.first_line(b"\n\r\n") is None


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path_factory.mktemp("rawtext_host") / "rawtext_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rawtext_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_host_harness_reproduces_the_fixture(golden_dir, host_check, name):
    """The very text of csrc/rawtext_line.h, compiled as plain C++: the columns of the reference's read_feat()."""
    from mapx import rawtext
    z, _ = _fixture(golden_dir, name)
    schema = rawtext.SCHEMAS[name]
    run = subprocess.run([host_check, name, os.path.join(golden_dir, RAW[name])], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-300:] + run.stderr[-300:]
    table = np.array([[int(x) for x in line.split()] for line in run.stdout.splitlines()], dtype=np.int64)
    assert table.shape == (len(z["index"]), len(schema.columns))
    for j, n in enumerate(schema.columns):
        want = z[f"col/{n}"]
        if n in schema.string_columns:
            assert np.array_equal(_as_fixture(table[:, j], want), want), n
        else:                                          # (Criteo's click was read with dtype=object: '0' / '1')
            assert np.array_equal(table[:, j], want.astype(np.int64)), n


def test_host_harness_reports_what_the_restatement_reports(host_check, tmp_path):
    from mapx import rawtext
    cases = [(cid, sname, [R.GOOD_LINE[sname]] * 3 + [bad] + [R.GOOD_LINE[sname]], col, reason)
             for cid, sname, bad, col, reason in R.error_cases(rawtext.SCHEMAS)]
    a = rawtext.AVAZU
    cases.append(("two_bad_lines", "avazu", [R.AVAZU_LINE, R.with_field(R.AVAZU_LINE, a, "C14", b"x"),
                                            R.with_field(R.AVAZU_LINE, a, "C1", b"")], "C14", R.E_INT))
    for cid, sname, lines, col, reason in cases:
        schema = rawtext.SCHEMAS[sname]
        for final_newline in (True, False):
            data = R.document(schema, lines, blank_at=(0, 2), final_newline=final_newline, eol=b"\r\n")
            with pytest.raises(R.RefError) as ref:
                R.parse(data, schema)
            assert (ref.value.column, ref.value.reason) == (col, reason), cid
            path = tmp_path / f"{cid}.txt"
            path.write_bytes(data)
            run = subprocess.run([host_check, sname, str(path)], capture_output=True, text=True)
            assert run.returncode == 1, cid
            assert run.stdout.split() == ["error", "line", str(ref.value.line), "column",
                                          str(schema.source_names.index(col)), "reason", str(reason)], (cid, run.stdout)
    # valid oddities: date edges, a last line that ends in a delimiter, no final newline, negative and huge integers
    lines = [R.with_field(R.AVAZU_LINE, a, "hour", t) for t in (b"00010100", b"99123123", b"16022912", b"69010100")]
    lines.append(R.with_field(R.AVAZU_LINE, a, "C21", b"-999999999999999999"))
    lines.append(R.with_field(R.AVAZU_LINE, a, "site_id", b""))
    for schema, doc in ((a, R.document(a, lines, blank_at=(1, len(lines)), final_newline=False)),
                        (rawtext.CRITEO, R.document(rawtext.CRITEO, [R.with_field(R.CRITEO_LINE, rawtext.CRITEO, "C26", b""),
                                                                     R.with_field(R.CRITEO_LINE, rawtext.CRITEO, "I5", b"999999999999999999")],
                                                    final_newline=False))):
        labels, cols = R.parse(doc, schema)
        path = tmp_path / f"ok_{schema.name}.txt"
        path.write_bytes(doc)
        run = subprocess.run([host_check, schema.name, str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout
        table = np.array([[int(x) for x in line.split()] for line in run.stdout.splitlines()], dtype=np.int64)
        assert np.array_equal(table[:, 0], labels)
        for j, n in enumerate(schema.columns[1:], start=1):
            assert np.array_equal(table[:, j], cols[n]), n


def test_there_is_no_cpu_parsing_path(golden_dir):
    import torch
    from mapx import rawtext
    from mapx.native import MapxError
    path = os.path.join(golden_dir, RAW["criteo"])
    with pytest.raises(MapxError):
        rawtext.read_columns(path, rawtext.CRITEO, device="cpu")
    with pytest.raises(MapxError):
        rawtext.parse_bytes(b"0\t1\n", rawtext.CRITEO, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(MapxError):
            rawtext.read_columns(path, rawtext.CRITEO)
    buf = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(MapxError):                                    # CPU pointers never reach the library
        rawtext.index_lines(buf, 10, 4)
    i32 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(MapxError):
        rawtext.parse_lines(buf, 10, i32, i32, rawtext.CRITEO, torch.zeros(40, 1, dtype=torch.int64))


@pytest.mark.parametrize("argv", [
    [],
    ["--dataset", "avazu", "--n_core", "2", "--out", "x"],                                        # no --raw
    ["--dataset", "kdd12", "--raw", "RAW", "--n_core", "2", "--out", "x"],
    ["--dataset", "avazu", "--raw", "RAW", "--n_core", "0", "--out", "x"],
    ["--dataset", "avazu", "--raw", "RAW", "--n_core", "two", "--out", "x"],
    ["--dataset", "avazu", "--raw", "RAW", "--n_core", "2", "--out", "x", "--split", "0.5,0.5"],
    ["--dataset", "avazu", "--raw", "RAW", "--n_core", "2", "--out", "x", "--split", "0.8,0.3,0.1"],
    ["--dataset", "avazu", "--raw", "RAW", "--n_core", "2", "--out", "x", "--chunk_mb", "2048"],
    ["--dataset", "avazu", "--raw", "MISSING", "--n_core", "2", "--out", "x"],
])
def test_command_line_rejects_bad_arguments(golden_dir, tmp_path, argv, capsys):
    from mapx import preprocess
    argv = [os.path.join(golden_dir, RAW["avazu"]) if a == "RAW" else str(tmp_path / "nothing.gz") if a == "MISSING"
            else str(tmp_path / "out") if a == "x" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        preprocess.main(argv)
    assert e.value.code == 2 and "error" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
