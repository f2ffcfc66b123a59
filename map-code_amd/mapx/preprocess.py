"""Raw Avazu / Criteo file -> the dataset directory mapx/dataset.py reads, on the GPU:

    python -m mapx.preprocess --dataset avazu|criteo --raw PATH --n_core K --out DIR [--name NAME] [--chunk_mb M]
                              [--split a,b,c]
    python -m mapx.preprocess --dataset avazu|criteo --raw PATH --vocab META.json --out DIR [...]
    python -m mapx.preprocess --dataset avazu|criteo --raw PATH --vocab META.json --grow K --out DIR [...]

read_feat (mapx/rawtext.py over csrc/rawtext.hip) and generate_dataset (mapx/vocab.py over csrc/vocab.hip) of the
reference's data_preprocess/proc_avazu.py / proc_criteo.py in one pass: `<name>-meta.json`, `<name>.npz` and, with
--split, a seeded random `split.pkl` (the reference's own split files come from split_criteo_x4.py and are used as
they are when present).  With --vocab instead of --n_core nothing is fitted: the file is translated through the
feat_map saved in META.json by an earlier run (mapx/vocab.py Vocabulary over csrc/vocab_apply.hip), values that map
does not hold take their field's <oov> id, and the rows stay in file order.  With --grow K the saved feat_map is
extended first: per field the file's values it lacks and that occur at least K times are appended behind the field's
keys in Counter.most_common() order (mapx/vocab.py Vocabulary.grow over csrc/vocab_grow.hip); every old key keeps its
place among its field's keys, and `python -m mapx.grow` carries a checkpoint or a dataset over to the grown ids."""
import argparse
import os
import sys


def _split(text):
    try:
        parts = tuple(float(x) for x in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: three fractions a,b,c")
    if len(parts) != 3 or min(parts) < 0 or abs(sum(parts) - 1.0) > 1e-6:
        raise argparse.ArgumentTypeError(f"{text!r}: three non-negative fractions that sum to 1")
    return parts


def _positive(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: an integer")
    if v < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: must be at least 1")
    return v


def parser():
    p = argparse.ArgumentParser(prog="python -m mapx.preprocess", description=__doc__.split("\n\n")[0])
    p.add_argument("--dataset", required=True, choices=("avazu", "criteo"))
    p.add_argument("--raw", required=True, help="train.gz / train.txt (a .gz path is streamed through gzip)")
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--n_core", type=_positive, help="fit a vocabulary: keep values seen at least this often")
    how.add_argument("--vocab", metavar="META.json", help="encode with the feat_map of an earlier run's <name>-meta.json")
    p.add_argument("--grow", type=_positive, metavar="K", default=None,
                   help="with --vocab: append the file's values the feat_map lacks and that occur at least K times")
    p.add_argument("--out", required=True, help="dataset directory")
    p.add_argument("--name", default=None, help="file prefix inside --out (default: the dataset's name)")
    p.add_argument("--chunk_mb", type=_positive, default=256, help="bytes of the file on the device at a time (<= 1024)")
    p.add_argument("--split", type=_split, default=None, help="train,valid,test fractions of a seeded random split.pkl")
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.chunk_mb > 1024:
        p.error("--chunk_mb: at most 1024")
    if not os.path.isfile(args.raw):
        p.error(f"--raw: {args.raw} is not a file")
    if args.vocab is not None and not os.path.isfile(args.vocab):
        p.error(f"--vocab: {args.vocab} is not a file")
    if args.grow is not None and args.vocab is None:
        p.error("--grow extends a saved vocabulary: it goes with --vocab META.json")
    from . import rawtext, vocab
    if args.grow is not None:
        meta, input_size = vocab.grow_dataset_from_text(args.raw, rawtext.SCHEMAS[args.dataset], args.vocab, args.grow,
                                                        args.out, args.name or args.dataset,
                                                        chunk_bytes=args.chunk_mb << 20, split=args.split)
        N, total = len(meta["index"]), sum(meta["grown"].values())
        most = sorted(meta["grown"].items(), key=lambda x: -x[1])[:3]
        print(f"{args.out}: {N} rows, {len(meta['field_names']) - 1} fields, input_size {input_size - total} -> "
              f"{input_size} ({total} keys added; " + ", ".join(f"{n} +{a}" for n, a in most) + f"), "
              f"avg_ctr {meta['avg_ctr']:.6f}; <oov> cells left {sum(meta['oov_rows'].values())}")
        return 0
    if args.vocab is not None:
        meta, input_size = vocab.encode_dataset_from_text(args.raw, rawtext.SCHEMAS[args.dataset], args.vocab, args.out,
                                                          args.name or args.dataset, chunk_bytes=args.chunk_mb << 20,
                                                          split=args.split)
        N = len(meta["index"])
        share = sorted(((c / N if N else 0.0, n) for n, c in meta["oov_rows"].items()), key=lambda x: -x[0])[:3]
        print(f"{args.out}: {N} rows, {len(meta['field_names']) - 1} fields, input_size {input_size}, "
              f"avg_ctr {meta['avg_ctr']:.6f}; <oov> share " + ", ".join(f"{n} {s:.4f}" for s, n in share))
        return 0
    meta, input_size = vocab.generate_dataset_from_text(args.raw, rawtext.SCHEMAS[args.dataset], args.n_core, args.out,
                                                        args.name or args.dataset, chunk_bytes=args.chunk_mb << 20,
                                                        split=args.split)
    print(f"{args.out}: {len(meta['index'])} rows, {len(meta['field_names']) - 1} fields, input_size {input_size}, "
          f"avg_ctr {meta['avg_ctr']:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
