#!/usr/bin/env python3
"""Generate the FiGNN backbone's fixtures by running the REAL reference `FiGNN` class (CPU, fp32, train mode), as
gen_fgcnn_golden.py does for FGCNN.

Parameters and inputs come from fignn_params.py / paramgen.py (rebuilt bit-identically by the tests); the fixtures
hold outputs only: loss, logits and counts, every gradient (paramgen.digest), the attention graph and the trunk's
output of the first MID_ROWS samples, and the state-dict manifest (names, shapes, dtypes) of every variant.

The Leaky-ReLU of the graph has a slope that jumps by 100x at zero: the generator asserts, in float64, that no
off-diagonal pre-activation of the fixture lies within 1e-6 of it (fignn_params.SALT re-draws the parameters if one
does).

    python tests/golden/gen_fignn_golden.py
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
import fignn_params as fp  # noqa: E402


def ref_config(arguments, cfg, mode, feat_count, data_dir, variant):
    d = dict(
        model_name="fignn", data_dir=data_dir, input_size=cfg["V"], num_fields=cfg["F"], embed_size=cfg["E"],
        embed_dropout_rate=0.0, embed_norm=False, layer_norm_eps=1e-12, hidden_size=cfg["H"],
        num_hidden_layers=cfg["NL"], num_cross_layers=cfg["NC"], pt_neg_num=cfg["K"], proj_size=cfg["P"],
        pretrain=(mode != "CTR"), pt_type=("RFD" if mode == "RFD" else "MFP"), RFD_replace="Unigram",
        feat_count=torch.from_numpy(feat_count), device=torch.device("cpu"), n_gpu=0, idx_low=None, idx_high=None,
        feat_num_per_field=None)
    d.update(fp.extras_of(variant))
    return arguments.Config.from_dict(d)


def run_case(arguments, models, mode, variant, outdir):
    case, cfg = fp.CASE, pg.CASES[fp.CASE]
    torch.manual_seed(0)
    inp = pg.make_inputs(case, cfg)
    params = fp.make_params(cfg, mode, variant)
    store, cap = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        model = models.BaseModel.from_config(ref_config(arguments, cfg, mode, inp["feat_count"], tmp, variant))
    assert type(model).__name__ == "FiGNN"
    sd = model.state_dict()
    manifest = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()}
    trainable = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert set(params) == set(trainable), sorted(set(params) ^ set(trainable))
    with torch.no_grad():
        for k, p in trainable.items():
            p.copy_(torch.from_numpy(params[k]))
    model.train()
    block = model.fignn
    orig_graph = block.build_graph_with_attention

    def graph(feat_embed):
        cap["x"] = feat_embed.detach()
        cap["graph"] = orig_graph(feat_embed)
        return cap["graph"]
    block.build_graph_with_attention = graph
    block.register_forward_hook(lambda m, i, o: cap.__setitem__("h", o.detach().clone()))
    ids = torch.from_numpy(inp["input_ids"])
    mi = torch.from_numpy(inp["masked_index"])
    if mode == "MFP":
        labels = torch.gather(ids, 1, mi)
        ids_in = torch.scatter(ids, 1, mi, torch.full_like(mi, pg.MASK_ID))
        noise = torch.from_numpy(inp["noise"])
        model.mfp_criterion.get_noise = lambda b, l: noise
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
        hook = model.pred_rfd.register_forward_hook(lambda m, i, o: cap.__setitem__("logits", o.detach()))
        loss, count, acc, pos_ratio = model(input_ids=ids_in, labels=labels, masked_index=None)
        hook.remove()
        store["out/count"] = np.int64(count)
        store["out/acc"] = acc.detach().numpy()
        store["out/pos_ratio"] = pos_ratio.detach().numpy()
        store["out/logits"] = cap["logits"].numpy()
    else:
        loss, logits = model(input_ids=ids, labels=torch.from_numpy(inp["y"]))
        store["out/logits"] = logits.detach().numpy()
    smallest = fp.smallest_pre(cap["x"].numpy(), params["fignn.W_attn.weight"])
    assert smallest > fp.PRE_MARGIN, (f"{mode}/{variant}: an off-diagonal pre-activation of the graph is {smallest:.3e} "
                                      "from the Leaky-ReLU's kink: salt the parameter seed (fignn_params.SALT)")
    store["mid/graph"] = cap["graph"].detach()[:fp.MID_ROWS].numpy().copy()
    store["mid/h"] = cap["h"][:fp.MID_ROWS].numpy().copy()
    loss.backward()
    store["out/loss"] = loss.detach().numpy()
    for k, p in trainable.items():
        G.put(store, "grad", k, p.grad.numpy())
    np.savez_compressed(os.path.join(outdir, f"{case}_{mode}_{variant}.npz"), **store)
    return manifest, smallest


def main():
    arguments, models = G.import_reference()
    torch.set_num_threads(1)
    manifests = {}
    for variant in fp.VARIANTS:
        for mode in fp.modes_of(variant):
            manifests[f"{fp.CASE}_{mode}_{variant}"], smallest = run_case(arguments, models, mode, variant, HERE)
            print("wrote", fp.CASE, mode, variant, f"smallest |pre| {smallest:.3e}")
    with open(os.path.join(HERE, "fignn_manifest.json"), "w") as f:
        json.dump(manifests, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
