#!/usr/bin/env python3
"""Fixtures of the raw-text reader (mapx/rawtext.py) from the REAL reference preprocessing: read_feat() and then
generate_dataset(n_core) of data_preprocess/proc_avazu.py and proc_criteo.py, run on two small seeded raw files.

Runs only where /root/reference exists (the build container).  What is stored:
  raw_avazu.csv, raw_criteo.tsv    the synthetic raw files (LF only) — input data the reference's programs read;
  rawtext_<name>.npz               every column as read_feat() saved it (int64, or fixed-width unicode), the row
                                   permutation `index`, feat_map keys and ids, and feat_ids — outputs, no source.

Import notes (as in gen_vocab_golden.py): an EMPTY module stands in for h5py, so generate_dataset() writes its JSON
and then stops at `h5py.File`; DataFrame.describe is wrapped to drop the `datetime_is_numeric` keyword that pandas 2
removed (proc_avazu.py:40).  Avazu's read_feat() opens train.gz: a gzipped temporary copy of the CSV is made.

    python tests/golden/gen_rawtext_golden.py
"""
import gzip
import json
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/data_preprocess"
N_ROWS = 500

AVAZU_HEADER = ["id", "click", "hour", "C1", "banner_pos", "site_id", "site_domain", "site_category", "app_id",
                "app_domain", "app_category", "device_id", "device_ip", "device_model", "device_type",
                "device_conn_type", "C14", "C15", "C16", "C17", "C18", "C19", "C20", "C21"]
AVAZU_HASH = AVAZU_HEADER[5:14]


def _zipf_pick(rng, vocab, n):
    ranks = np.minimum((rng.pareto(0.9, n) * 2).astype(np.int64), len(vocab) - 1)
    return [vocab[r] for r in ranks]


def _hash_vocab(rng, size):
    return [format(int(x), "08x") for x in rng.randint(0, 1 << 32, size=size, dtype=np.int64)]


def write_avazu(path, seed=101):
    rng = np.random.RandomState(seed)
    n = N_ROWS
    cols = {"id": [str(int(x)) + str(int(y)) for x, y in zip(rng.randint(10 ** 9, 10 ** 10, n, dtype=np.int64),
                                                          rng.randint(10 ** 9, 10 ** 10, n, dtype=np.int64))],
            "click": [str(int(x)) for x in (rng.rand(n) < 0.17)]}
    hours = ["1410%02d%02d" % (d, h) for d, h in zip(rng.randint(21, 31, n), rng.randint(0, 24, n))]
    # a leap day, and %y's 19YY side.  (Not 00010100: pandas reads the column as integers, the leading zeros are
    # gone and the reference's own to_datetime raises on "10100"; tests/test_rawtext_*.py check that date against
    # Python's strptime instead.)
    hours[7], hours[33] = "16022912", "99123123"
    cols["hour"] = hours
    cols["C1"] = [str(x) for x in _zipf_pick(rng, [1005, 1002, 1010, 1012, 1007, 1001, 1008], n)]
    cols["banner_pos"] = [str(x) for x in _zipf_pick(rng, [0, 1, 7, 2, 4, 5, 3], n)]
    for j, name in enumerate(AVAZU_HASH):
        vocab = _hash_vocab(rng, [5, 30, 200][j % 3])
        vocab[0] = "a" + vocab[0][1:]                                      # a letter: pandas must keep strings
        cols[name] = _zipf_pick(rng, vocab, n)
    cols["device_type"] = [str(x) for x in _zipf_pick(rng, [1, 0, 4, 5, 2], n)]
    cols["device_conn_type"] = [str(x) for x in _zipf_pick(rng, [0, 2, 3, 5], n)]
    for name, lo, hi, k in (("C14", 375, 24052, 150), ("C15", 120, 1024, 6), ("C16", 20, 1024, 7), ("C17", 112, 2758, 60),
                            ("C18", 0, 4, 4), ("C19", 33, 1959, 30), ("C21", 1, 255, 25)):
        cols[name] = [str(x) for x in _zipf_pick(rng, sorted(set(rng.randint(lo, hi, k).tolist())), n)]
    c20 = _zipf_pick(rng, [-1] + sorted(set(rng.randint(100000, 100250, 40).tolist())), n)
    cols["C20"] = [str(x) for x in c20]
    with open(path, "w", newline="") as f:
        f.write(",".join(AVAZU_HEADER) + "\n")
        for i in range(n):
            f.write(",".join(cols[h][i] for h in AVAZU_HEADER) + "\n")


def _bucket(v):
    return int(math.floor(math.log(v) ** 2)) if v > 2 else v


def _threshold(b):
    lo, hi = 3, 1 << 40
    if _bucket(lo) >= b:
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _bucket(mid) >= b:
            hi = mid
        else:
            lo = mid
    return hi


def write_criteo(path, seed=202):
    rng = np.random.RandomState(seed)
    n = N_ROWS
    edge = []
    for b in (2, 3, 4, 7, 19, 50, 101, 250, 399, 461):                     # t - 1, t, t + 1 of several thresholds
        t = _threshold(b)
        edge += [t - 1, t, t + 1]
    edge += list(range(-3, 9)) + [2 ** 31, 2 ** 31 - 1, 2 ** 31 - 7, 65535, 10 ** 6]
    rows = []
    for i in range(n):
        toks = [str(int(rng.rand() < 0.25))]
        for j in range(13):
            r = rng.rand()
            if r < 0.15:
                toks.append("")
            elif r < 0.45:
                toks.append(str(edge[rng.randint(len(edge))]))
            else:
                toks.append(str(int(rng.pareto(0.7) * 3)))
        for j in range(26):
            if rng.rand() < 0.15:
                toks.append("")
            else:
                size = [4, 40, 400][j % 3]
                r = min(int(rng.pareto(0.9) * 2), size - 1)
                toks.append(format((r * 2654435761 + j * 97 + 0xa0000000) & 0xffffffff, "08x"))
        if i % 9 == 4:
            toks[1] = ""                                                   # an empty I1
        if i % 7 == 3:
            toks[39] = ""                                                  # an empty C26: the line ends in a tab
        rows.append("\t".join(toks))
    with open(path, "w", newline="") as f:
        for i, r in enumerate(rows):
            if i == 211:
                f.write("\n")                                              # one blank line
            f.write(r + "\n")


def _load_reference(module_name):
    import pandas as pd
    if "h5py" not in sys.modules:
        sys.modules["h5py"] = types.ModuleType("h5py")
    if not getattr(pd.DataFrame.describe, "_drops_keyword", False):
        plain = pd.DataFrame.describe

        def describe(self, *a, datetime_is_numeric=None, **k):
            return plain(self, *a, **k)
        describe._drops_keyword = True
        pd.DataFrame.describe = describe
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return __import__(module_name)


def run_reference(module_name, subdir, raw_path, n_core):
    mod = _load_reference(module_name)
    with tempfile.TemporaryDirectory() as tmp:
        if subdir == "avazu":
            data_dir = os.path.join(tmp, "data", "avazu") + os.sep
            os.makedirs(os.path.join(data_dir, "avazu_x4"))
            with open(raw_path, "rb") as src, gzip.open(os.path.join(data_dir, "train.gz"), "wb") as dst:
                dst.write(src.read())
        else:
            data_dir = os.path.join(tmp, "data", "criteo", "criteo_x4") + os.sep
            os.makedirs(os.path.join(data_dir, "dac"))
            with open(raw_path, "rb") as src, open(os.path.join(data_dir, "dac", "train.txt"), "wb") as dst:
                dst.write(src.read())
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        mod.data_dir = data_dir
        cwd = os.getcwd()
        os.chdir(work)                       # generate_dataset's output paths are '../data/<subdir>/<subdir>_x4/...'
        try:
            mod.read_feat()
            try:
                mod.generate_dataset(n_core=n_core)
            except AttributeError as e:      # h5py.File on the empty module: the JSON is on disk by now
                assert "File" in str(e), e
        finally:
            os.chdir(cwd)
        names = list(mod.valid_fields)
        cols = {n: np.load(os.path.join(data_dir, f"{n}.npy"), allow_pickle=True) for n in names}
        meta = json.load(open(os.path.join(tmp, "data", subdir, f"{subdir}_x4", f"{subdir}_x4_{n_core}-core.json")))
    index = np.array(meta["index"], dtype=np.int64)
    feat_map = meta["feat_map"]
    fields = [n for n in names if n != "click"]
    ids = np.stack([np.array([feat_map.get(f"{n}-{v}", feat_map[f"{n}-<oov>"]) for v in cols[n][index]], dtype=np.int64)
                    for n in fields], axis=1)
    out = {"n_core": np.int64(n_core), "names": np.array(names), "index": index, "feat_ids": ids,
           "feat_map_keys": np.array(list(feat_map.keys())),
           "feat_map_ids": np.array(list(feat_map.values()), dtype=np.int64)}
    for n in names:
        c = cols[n]
        if c.dtype.kind == "O":
            assert all(isinstance(x, str) for x in c.tolist()), n
            c = c.astype(str)
        else:
            c = c.astype(np.int64)
        out[f"col/{n}"] = c
    return out


if __name__ == "__main__":
    avazu, criteo = os.path.join(HERE, "raw_avazu.csv"), os.path.join(HERE, "raw_criteo.tsv")
    write_avazu(avazu)
    write_criteo(criteo)
    for module_name, subdir, raw, n_core in (("proc_avazu", "avazu", avazu, 2), ("proc_criteo", "criteo", criteo, 2)):
        out = run_reference(module_name, subdir, raw, n_core)
        if subdir == "avazu":
            for n in AVAZU_HASH:             # pandas kept them as strings (a token with a letter in every column)
                assert out[f"col/{n}"].dtype.kind == "U", n
            assert out["col/C20"].dtype.kind == "i" and (out["col/C20"] == -1).any()
        path = os.path.join(HERE, f"rawtext_{subdir}.npz")
        np.savez_compressed(path, **out)
        print(path, "rows", out["feat_ids"].shape[0], "fields", out["feat_ids"].shape[1], "input_size",
              len(out["feat_map_keys"]), os.path.getsize(path) // 1024, "KiB;", os.path.basename(raw),
              os.path.getsize(raw) // 1024, "KiB")
