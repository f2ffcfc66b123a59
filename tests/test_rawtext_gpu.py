"""Raw text -> device columns on the GPU (mapx/rawtext.py over csrc/rawtext.hip): against the reference's own
read_feat() / generate_dataset() on the committed raw files (tests/golden/rawtext_*.npz), and against the Python
restatement (tests/rawtext_ref.py, pinned to those fixtures by test_rawtext_host.py) on synthetic inputs: extents
around the 64-line wave, both parse paths, pad bytes, guard bands, every error of the grammar.  Integer work: bit-exact."""
import gzip
import os

import numpy as np
import pytest
import torch

import rawtext_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAW = {"avazu": "raw_avazu.csv", "criteo": "raw_criteo.tsv"}


def _fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"rawtext_{name}.npz"))
    return z, os.path.join(golden_dir, RAW[name])


def _equals_fixture(result, z, schema):
    labels, cols, decode, strings = result
    assert list(cols) == [str(n) for n in z["names"]][1:] and strings == schema.string_columns
    assert labels.dtype == torch.int64 and labels.is_cuda
    assert np.array_equal(labels.cpu().numpy(), z["col/click"].astype(np.int64))
    for n, c in cols.items():
        want, got = z[f"col/{n}"], c.cpu().numpy()
        assert c.dtype == torch.int64 and c.is_cuda and c.is_contiguous()
        if n in strings:
            got = np.array([decode[n](v) for v in got.tolist()])
        assert np.array_equal(got, want), n


def _equals_restatement(result, data, schema):
    labels, cols = R.parse(data, schema)
    assert np.array_equal(result[0].cpu().numpy(), labels)
    assert list(result[1]) == list(cols)
    for n, c in cols.items():
        assert np.array_equal(result[1][n].cpu().numpy(), c), n
    return len(labels)


def _same(a, b):
    assert torch.equal(a[0], b[0]) and list(a[1]) == list(b[1])
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("chunk_bytes", [None, 4096, 700])
@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_fixture_columns(golden_dir, name, chunk_bytes, mode):
    from mapx import rawtext
    z, path = _fixture(golden_dir, name)
    schema = rawtext.SCHEMAS[name]
    first = rawtext.read_columns(path, schema, device=DEV, chunk_bytes=chunk_bytes, mode=mode)
    _equals_fixture(first, z, schema)
    _same(first, rawtext.read_columns(path, schema, device=DEV, chunk_bytes=chunk_bytes, mode=mode))   # bitwise again


def test_gzip_and_crlf_copies(golden_dir, tmp_path):
    from mapx import rawtext
    for name in ("avazu", "criteo"):
        z, path = _fixture(golden_dir, name)
        schema = rawtext.SCHEMAS[name]
        with open(path, "rb") as f:
            data = f.read()
        assert b"\r" not in data
        crlf = tmp_path / f"{name}_crlf.txt"
        crlf.write_bytes(data.replace(b"\n", b"\r\n"))
        for chunk_bytes in (None, 700):
            _equals_fixture(rawtext.read_columns(str(crlf), schema, device=DEV, chunk_bytes=chunk_bytes), z, schema)
        if name == "avazu":
            gz = tmp_path / "train.gz"
            with gzip.open(gz, "wb") as f:
                f.write(data)
            for chunk_bytes in (256 << 20, 4096):
                _equals_fixture(rawtext.read_columns(str(gz), schema, device=DEV, chunk_bytes=chunk_bytes), z, schema)


@pytest.mark.parametrize("name", ["avazu", "criteo"])
def test_command_line_end_to_end(golden_dir, tmp_path, name):
    """Raw file -> python -m mapx.preprocess -> the dataset directory: the reference's feat_map (keys in order, ids),
    feat_ids, row permutation and labels; the type ids by the reference's rule; read back by mapx.dataset."""
    import json
    from mapx import preprocess, rawtext
    from mapx.dataset import BaseDataset
    z, path = _fixture(golden_dir, name)
    schema = rawtext.SCHEMAS[name]
    out = str(tmp_path / "data")
    assert preprocess.main(["--dataset", name, "--raw", path, "--n_core", str(int(z["n_core"])), "--out", out,
                            "--chunk_mb", "1", "--split", "0.8,0.1,0.1"]) == 0
    with open(os.path.join(out, f"{name}-meta.json")) as f:
        meta = json.load(f)
    assert list(meta["feat_map"].keys()) == [str(k) for k in z["feat_map_keys"]]
    assert list(meta["feat_map"].values()) == z["feat_map_ids"].tolist()
    index = z["index"]
    assert meta["index"] == index.tolist() and meta["field_names"] == ["<rsv>"] + schema.columns[1:]
    tab = np.load(os.path.join(out, f"{name}.npz"))
    assert np.array_equal(tab["feat_ids"], z["feat_ids"])
    labels = z["col/click"].astype(np.int64)[index]
    assert np.array_equal(tab["labels"], labels) and meta["num_pos"] == int(labels.sum())
    oov = meta["feat_type_map"]["<oov>"]
    for j, n in enumerate(schema.columns[1:]):
        col = z[f"col/{n}"][index]
        plain = meta["feat_type_map"][schema.feat_types[n]]
        want = np.full(len(col), plain) if n in schema.string_columns else np.where(col == -1, oov, plain)
        assert np.array_equal(tab["type_ids"][:, j], want), n
    if name == "criteo":
        assert (tab["type_ids"] == oov).any() and meta["feat_type_map"] == {"<rsv>": 0, "<num>": 1, "<cat>": 2, "<oov>": 3}

    class Args:
        data_dir, dataset_name, pretrain, pt_type, RFD_replace = out, name, True, "MFP", "Unigram"
    ds = BaseDataset(Args())
    N = len(index)
    assert ds.get_splited_dataset("train").X.shape == (int(N * 0.8), len(schema.columns) - 1)
    assert ds.feat_map == meta["feat_map"]


def _fixture_lines(golden_dir, name):
    with open(os.path.join(golden_dir, RAW[name]), "rb") as f:
        lines = [line for _, line in R.lines(f.read())]
    return lines[1:] if name == "avazu" else lines


@pytest.mark.parametrize("n_lines", [1, 63, 64, 65, 255, 257])
def test_extents_around_the_wave(golden_dir, n_lines):
    from mapx import rawtext
    for name in ("avazu", "criteo"):
        schema = rawtext.SCHEMAS[name]
        lines = _fixture_lines(golden_dir, name)[:n_lines]
        for final_newline in (True, False):
            for blank_at in ((), (0, n_lines // 2, n_lines)):
                data = R.document(schema, lines, blank_at=blank_at, final_newline=final_newline)
                for mode in (0, 1):
                    got = rawtext.parse_bytes(data, schema, device=DEV, mode=mode)
                    assert _equals_restatement(got, data, schema) == n_lines
    empty = rawtext.parse_bytes(b"\n\r\n", rawtext.CRITEO, device=DEV)
    assert empty[0].numel() == 0 and all(c.numel() == 0 for c in empty[1].values())


def test_spans_beyond_the_lds_window_take_the_direct_path():
    from mapx import rawtext
    from mapx.native import lib
    c = rawtext.CRITEO
    window = lib.mapx_rawtext_window_bytes()
    rng = np.random.RandomState(3)

    def wide(i):                                       # every field at its maximum width
        toks = [b"-" + b"%018d" % (i + 1)] + [b"-" + b"%018d" % rng.randint(1, 10 ** 9) for _ in range(13)]
        toks[3] = b"%018d" % (10 ** 17 + i)            # a bucket far up the table
        toks += [b"%014x" % ((i * 2654435761 + j) % (1 << 56)) for j in range(26)]
        return b"\t".join(toks)
    long_lines = [wide(i) for i in range(130)]
    assert 64 * len(long_lines[0]) > window >= 4096
    short = [R.CRITEO_LINE] * 100
    for lines in (long_lines, short + long_lines + short, long_lines[:3] + short + long_lines[3:70]):
        data = R.document(c, lines, final_newline=False)
        auto = rawtext.parse_bytes(data, c, device=DEV, mode=0)
        _equals_restatement(auto, data, c)
        _same(auto, rawtext.parse_bytes(data, c, device=DEV, mode=1))
        _same(auto, rawtext.parse_bytes(data, c, device=DEV, mode=0, chunk_bytes=50_000))


def _parse_raw(buf, n, schema, out=None, row0=0, mode=0, max_lines=None):
    """index + parse of one device buffer through the library, nothing else: -> (line_start, line_no, out, bad)."""
    from mapx import rawtext
    ls, ln, n_lines, n_nl = rawtext.index_lines(buf, n, n if max_lines is None else max_lines)
    if schema.header:                                  # (the header line is the host's to check and skip)
        ls, ln, n_lines = ls[1:], ln[1:], n_lines - 1
    if out is None:
        out = torch.full((len(schema.columns), row0 + n_lines), -77, dtype=torch.int64, device=DEV)
    bad = rawtext.parse_lines(buf, n, ls, ln, schema, out, row0=row0, mode=mode)
    return ls, ln, out, bad, n_nl


def test_pad_bytes_change_nothing():
    """The kernels may load the 0-15 bytes between n_bytes and the next multiple of 16: whatever they hold — line
    ends, delimiters, digits that would lengthen the last field — the index and the columns are the same."""
    from mapx import rawtext
    for schema, line in ((rawtext.CRITEO, R.CRITEO_LINE), (rawtext.AVAZU, R.AVAZU_LINE)):
        seen = set()
        for extra in range(16):                        # every remainder of n_bytes modulo 16
            if schema is rawtext.AVAZU:                # the file ends in a digit / in a hexadecimal digit
                last = R.with_field(line, schema, "C21", b"1" * (extra + 1))
            else:
                last = R.with_field(R.with_field(line, schema, "C25", b"b" * (8 + max(extra - 14, 0))), schema, "C26",
                                    b"a" * min(extra, 14))
            data = R.document(schema, [line] * 70 + [last], final_newline=False)
            n = len(data)
            seen.add(n % 16)
            labels, cols = R.parse(data, schema)
            results = []
            for pad in (b"\n", schema.delimiter.encode(), b"7", b"\r", b'"'):
                buf = torch.frombuffer(bytearray(data + pad * 32), dtype=torch.uint8)[:(n + 15) // 16 * 16].to(DEV)
                for mode in (0, 1):
                    ls, ln, out, bad, n_nl = _parse_raw(buf, n, schema, mode=mode)
                    assert bad is None and n_nl == data.count(b"\n")
                    results.append((ls, ln, out))
            for ls, ln, out in results[1:]:
                assert torch.equal(ls, results[0][0]) and torch.equal(ln, results[0][1]) and torch.equal(out, results[0][2])
            out = results[0][2].cpu().numpy()
            assert np.array_equal(out[0], labels)
            for j, name in enumerate(schema.columns[1:], start=1):
                assert np.array_equal(out[j], cols[name]), name
        assert len(seen) == 16


@pytest.mark.parametrize("malformed", [False, True])
def test_guard_bands_stay_intact(golden_dir, malformed):
    """Index and columns inside guarded buffers, a column pitch larger than the rows and a row offset: nothing outside
    the extent changes, also when some lines are malformed (they stop at their first bad field)."""
    from guarded import guarded
    from mapx import rawtext
    from mapx.native import check, lib, ptr, stream
    c = rawtext.CRITEO
    lines = _fixture_lines(golden_dir, "criteo")[:200]
    if malformed:
        lines[5] = R.with_field(lines[5], c, "C3", b"XYZ")
        lines[70] = lines[70] + b"\t1"
        lines[131] = lines[131][:40]
        lines[199] = R.with_field(lines[199], c, "click", b"")
    data = R.document(c, lines, blank_at=(0, 64, 200), final_newline=False)
    n, N = len(data), len(lines)
    buf = torch.frombuffer(bytearray(data + b"0" * 16), dtype=torch.uint8)[:(n + 15) // 16 * 16].to(DEV)
    ls_view, ls_chk = guarded(1, N, torch.int32, ld=N + 5, col0=3)
    ln_view, ln_chk = guarded(1, N, torch.int32, ld=N + 5, col0=1)
    ws = torch.empty(lib.mapx_rawtext_index_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    counts = torch.empty(2, dtype=torch.int32, device=DEV)
    for max_lines in (N, N - 7):                       # an index cut short writes only what fits
        check(lib.mapx_rawtext_index(ptr(buf), n, ptr(ws), ws.numel(), ls_view.data_ptr(), ln_view.data_ptr(), max_lines,
                                     ptr(counts), stream()))
        assert counts.tolist() == [N, data.count(b"\n")]
        ls_chk()
        ln_chk()
    want = R.lines(data)
    assert ln_view[0, :N - 7].tolist() == [no for no, _ in want][:N - 7]
    check(lib.mapx_rawtext_index(ptr(buf), n, ptr(ws), ws.numel(), ls_view.data_ptr(), ln_view.data_ptr(), N,
                                 ptr(counts), stream()))
    assert [data[s:s + 3] for s in ls_view[0].tolist()] == [line[:3] for _, line in want]
    ls2, ln2, n2, _ = rawtext.index_lines(buf, n, 3)                   # a guess too small: the host builds it again
    assert n2 == N and torch.equal(ls2, ls_view[0]) and torch.equal(ln2, ln_view[0])
    row0, ld = 11, N + 11 + 37
    for mode in (0, 1):
        view, chk = guarded(len(c.columns), N, torch.int64, ld=ld, col0=row0)
        bad = rawtext.parse_lines(buf, n, ls_view[0], ln_view[0], c, chk.rows, row0=row0, mode=mode)
        chk()
        good = np.ones(N, dtype=bool)
        if malformed:
            assert bad == (want[5][0], c.source_names.index("C3"), R.E_HEX)
            good[[5, 70, 131, 199]] = False
        else:
            assert bad is None
        labels, cols = R.parse(R.document(c, [l for l, g in zip(lines, good) if g]), c)
        got = view.cpu().numpy()
        assert np.array_equal(got[0][good], labels)
        for j, name in enumerate(c.columns[1:], start=1):
            assert np.array_equal(got[j][good], cols[name]), name


def _error_cases():
    from mapx import rawtext
    return R.error_cases(rawtext.SCHEMAS)


@pytest.mark.parametrize("case", range(12))
def test_errors_name_line_and_column(case):
    from mapx import rawtext
    cid, sname, bad_line, column, reason = _error_cases()[case]
    schema = rawtext.SCHEMAS[sname]
    good = R.GOOD_LINE[sname]
    later = R.with_field(good, schema, "click", b"x")                       # a second, later bad line
    lines = [good] * 9 + [bad_line] + [good] * 3 + [later, good]
    data = R.document(schema, lines, blank_at=(0, 4, 9), final_newline=case % 2 == 0, eol=b"\r\n" if case % 3 == 0 else b"\n")
    with pytest.raises(R.RefError) as ref:
        R.parse(data, schema)
    assert (ref.value.column, ref.value.reason) == (column, reason)
    line = ref.value.line
    assert line == 9 + 3 + (1 if schema.header else 0) + 1                  # header and blank lines counted
    messages = []
    for chunk_bytes in (None, 700, 700):                                    # across a chunk cut; and once more
        for mode in (0, 1):
            with pytest.raises(ValueError) as e:
                rawtext.parse_bytes(data, schema, device=DEV, chunk_bytes=chunk_bytes, mode=mode, where="train.txt")
            messages.append(str(e.value))
    assert len(set(messages)) == 1
    assert messages[0] == f"train.txt: line {line}, column {column!r}: {rawtext.REASONS[reason]}"


def test_header_must_match():
    from mapx import rawtext
    a = rawtext.AVAZU
    with pytest.raises(ValueError, match="line 2: the header names"):
        rawtext.parse_bytes(b"\n" + R.AVAZU_HEADER.replace(b"C21", b"C22") + b"\n" + R.AVAZU_LINE + b"\n", a, device=DEV)
    with pytest.raises(ValueError, match="line 1: the header names"):
        rawtext.parse_bytes(R.AVAZU_LINE + b"\n", a, device=DEV)
    with pytest.raises(ValueError, match="no header"):
        rawtext.parse_bytes(b"\n\n", a, device=DEV)
    only_header = rawtext.parse_bytes(R.AVAZU_HEADER + b"\r\n", a, device=DEV)
    assert only_header[0].numel() == 0 and list(only_header[1]) == a.columns[1:]


def test_fifty_thousand_criteo_lines():
    """About 14 MB in 1 MiB chunks; the expected values are the seeded columns themselves: the integers through the
    vectorised expression of proc_criteo.py:30, the hash strings through their code."""
    from mapx import rawtext
    c = rawtext.CRITEO
    N = 50_000
    rng = np.random.RandomState(17)
    click = (rng.rand(N) < 0.25).astype(np.int64)
    ints = np.where(rng.rand(N, 13) < 0.5, rng.randint(-3, 40, (N, 13)),
                    np.minimum(rng.pareto(0.5, (N, 13)) * 50, 1e17).astype(np.int64)).astype(np.int64)
    ints[rng.rand(N, 13) < 0.02] = 2 ** 31
    int_empty = rng.rand(N, 13) < 0.15
    hashes = rng.randint(0, 1 << 32, (N, 26), dtype=np.int64) % np.array([7, 1000, 10 ** 6, 1 << 32] * 6 + [50, 1 << 32])
    hash_empty = rng.rand(N, 26) < 0.15
    cells = [click.astype(str)]
    cells += [np.where(int_empty[:, j], "", ints[:, j].astype(str)) for j in range(13)]
    cells += [np.where(hash_empty[:, j], "", np.array([format(v, "08x") for v in hashes[:, j].tolist()])) for j in range(26)]
    data = ("\n".join("\t".join(row) for row in zip(*cells)) + "\n").encode()
    assert 10 << 20 < len(data) < 20 << 20
    got = rawtext.parse_bytes(data, c, device=DEV, chunk_bytes=1 << 20)
    assert np.array_equal(got[0].cpu().numpy(), click)
    for j in range(13):
        want = np.where(int_empty[:, j], -1, R.bucket_array(ints[:, j]))
        assert np.array_equal(got[1][f"I{j + 1}"].cpu().numpy(), want), j
    for j in range(26):
        want = np.where(hash_empty[:, j], -1, (hashes[:, j] << 4) | 8)
        assert np.array_equal(got[1][f"C{j + 1}"].cpu().numpy(), want), j
    _same(got, rawtext.parse_bytes(data, c, device=DEV, chunk_bytes=1 << 20, mode=1))
