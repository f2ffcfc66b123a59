#!/usr/bin/env python3
"""Generate the Transformer backbone's fixtures by running the REAL reference `Transformer` class (CPU, fp32, train
mode, dropout 0), as gen_golden.py does for the other backbones.

Parameters and inputs come from trans_params.py / paramgen.py (rebuilt bit-identically by the tests); the fixtures
hold outputs only: loss, logits, every encoder layer's output (first MID_ROWS samples), every gradient (paramgen.digest) and the state-dict
manifest (names and shapes) of every variant.

    python tests/golden/gen_trans_golden.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import paramgen as pg  # noqa: E402
import trans_params as tp  # noqa: E402


MID_ROWS = 8            # samples of which every encoder layer's output is kept


def ref_config(arguments, cfg, mode, feat_count, data_dir, variant):
    d = dict(
        model_name="trans", data_dir=data_dir, input_size=cfg["V"], num_fields=cfg["F"], embed_size=cfg["E"],
        embed_dropout_rate=0.0, embed_norm=False, num_cross_layers=cfg["NC"], pt_neg_num=cfg["K"], proj_size=cfg["P"],
        pretrain=(mode != "CTR"), pt_type=("RFD" if mode == "RFD" else "MFP"), RFD_replace="Unigram",
        feat_count=torch.from_numpy(feat_count), device=torch.device("cpu"), n_gpu=0, idx_low=None, idx_high=None,
        feat_num_per_field=None)
    d.update(tp.extras_of(variant))
    return arguments.Config.from_dict(d)


def encoder_layers(model, x):
    outs = []
    for layer in model.encoder.layers:
        x = layer(x)
        outs.append(x.detach().numpy().copy())
    return outs


def run_case(arguments, models, mode, variant, outdir):
    case, cfg = tp.CASE, pg.CASES[tp.CASE]
    torch.manual_seed(0)
    inp = pg.make_inputs(case, cfg)
    params = tp.make_params(cfg, mode, variant)
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        model = models.BaseModel.from_config(ref_config(arguments, cfg, mode, inp["feat_count"], tmp, variant))
    manifest = {k: list(v.shape) for k, v in model.state_dict().items()}
    trainable = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert set(params) == set(trainable), sorted(set(params) ^ set(trainable))
    with torch.no_grad():
        for k, p in trainable.items():
            p.copy_(torch.from_numpy(params[k]))
    model.train()
    ids = torch.from_numpy(inp["input_ids"])
    mi = torch.from_numpy(inp["masked_index"])
    if mode == "MFP":
        labels = torch.gather(ids, 1, mi)
        ids_in = torch.scatter(ids, 1, mi, torch.full_like(mi, pg.MASK_ID))
        noise = torch.from_numpy(inp["noise"])
        model.mfp_criterion.get_noise = lambda b, l: noise
        cap = {}
        orig_forward = model.mfp_criterion.forward

        def fwd(target, *a, **k):
            out = orig_forward(target, *a, **k)
            cap["logits"] = out[1].detach()
            return out
        model.mfp_criterion.forward = fwd
        loss, count, total_acc = model(input_ids=ids_in, labels=labels, masked_index=mi)
        store["out/count"] = np.int64(count)
        store["out/total_acc"] = np.int64(total_acc)
        store["out/logits"] = cap["logits"].numpy()
    elif mode == "RFD":
        ids_in = torch.scatter(ids, 1, mi, torch.from_numpy(inp["replace_feat"]))
        labels = (ids != ids_in).float()
        loss, count, acc, pos_ratio = model(input_ids=ids_in, labels=labels, masked_index=None)
        store["out/count"] = np.int64(count)
        store["out/acc"] = acc.detach().numpy()
        store["out/pos_ratio"] = pos_ratio.detach().numpy()
        with torch.no_grad():
            store["out/logits"] = model.pred_rfd(model.encoder(model.embed(ids_in)).flatten(1)).numpy()
    else:
        ids_in = ids
        loss, logits = model(input_ids=ids, labels=torch.from_numpy(inp["y"]))
        store["out/logits"] = logits.detach().numpy()
    with torch.no_grad():
        for li, out in enumerate(encoder_layers(model, model.embed(ids_in))):
            store[f"mid/enc{li}"] = out[:MID_ROWS]
    loss.backward()
    store["out/loss"] = loss.detach().numpy()
    for k, p in trainable.items():
        G.put(store, "grad", k, p.grad.numpy())
    np.savez_compressed(os.path.join(outdir, f"{case}_{mode}_{variant}.npz"), **store)
    return manifest


def main():
    arguments, models = G.import_reference()
    torch.set_num_threads(1)
    manifests = {}
    for variant in tp.VARIANTS:
        for mode in tp.modes_of(variant):
            manifests[f"{tp.CASE}_{mode}_{variant}"] = run_case(arguments, models, mode, variant, HERE)
            print("wrote", tp.CASE, mode, variant)
    with open(os.path.join(HERE, "trans_manifest.json"), "w") as f:
        json.dump(manifests, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
