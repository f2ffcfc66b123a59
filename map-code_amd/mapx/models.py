"""BaseModel + DCNV2 (host mirror of reference code/models.py:21-127, 282-322): same factory,
same forward signature and output tuples, same state_dict key layout; every arithmetic step
is a gfx950 kernel.  The other backbones the factory builds: DNN, DeepFM, xDeepFM, AutoInt, trans, fgcnn
(from_config still refuses fignn, and trans / xDeepFM / fgcnn with compute_dtype=bf16; build_backbone builds them)."""
import logging

import torch
from torch import nn

from . import ops
from .arguments import Config
from .layers import (_JoinColumns, AttentionalPrediction, CIN, CrossNetV2, Embeddings, FGCNNBlock, FiGNNBlock,
                     HipLinear, MLPBlock, MultiHeadSelfAttention, RowTable, TableWeight, TransformerEncoder, TransformerEncoderLayer,
                     bce_with_logits, field_pool, fm_product_sum, inner_product, to_bf16)
from .nce import IndexLinear

logger = logging.getLogger(__name__)
WIDE_CROSS_TOWER = 512        # columns: from here on the cross tower's stream is the longer one (Criteo-shaped inputs)


def layout_on_main(D):
    """The grouped encoder's slot layout ahead of the deep tower (main stream, True) or on the cross tower's stream:
    on the main stream when the cross tower is at least 512 columns wide (Criteo-shaped: its stream is the longer
    one of the forward pass, 1.0026 -> 0.9924 ms with the layout off it), on the cross tower's stream otherwise
    (Avazu-shaped: equal either way, 0.7064 vs 0.7070)."""
    return D >= WIDE_CROSS_TOWER


def plan_after_main(pretrain, f32_trunk, D):
    """RFD / finetune steps (one table, one sort chain): the sort goes behind what the main stream (the deep tower's
    forward GEMMs, True) or the tower stream (the cross tower's, False) holds.  Forked from the ids alone the graph
    runtime ran it LAST, 127 us of sort + reduction + row update exposed behind the backward pass; behind the deep
    tower's forward GEMMs it runs beside the head: RFD 0.946 -> 0.845 ms, finetune 0.765 -> 0.664.  Behind the CROSS
    tower's (the head is short then and the deep tower's backward would wait for the sort on its queue): finetune
    0.636 -> 0.619 ms, RFD 0.768 -> 0.786 — so by the head.  After the join's capture order changed the finetune step
    with the fp32 trunk at Avazu's width also prefers the main stream (0.515 / 0.513 -> 0.493 / 0.492 ms); its
    Criteo-shaped (0.623 vs 0.641) and bf16 (0.345 vs 0.376) forms keep the tower stream.  (The single-stream
    backbones measured neutral (RFD / CTR) or worse (DNN + MFP): left as they were.)"""
    return pretrain or (f32_trunk and D < WIDE_CROSS_TOWER)


_OTHER_BACKBONES = ("fignn",)


def _refuse_bf16_mlp_options(config, act_flag, drop_flag):
    """DeepFM / AutoInt in compute_dtype=bf16: what MLPBlock.forward refuses for a bf16 input (a non-ReLU activation,
    dropout between the layers) is refused when the model is built, with MLPBlock's messages and the flag's name."""
    from .layers import compute_dtype_of
    if compute_dtype_of(config) == torch.float32:
        return
    act = str(getattr(config, act_flag)).lower()
    if act != "relu":
        raise NotImplementedError(f"{act_flag}: hidden_act={act!r} is built for compute_dtype=fp32")
    if float(getattr(config, drop_flag) or 0.0) > 0:
        raise NotImplementedError(f"{drop_flag}: hidden_dropout_rate > 0 is built for compute_dtype=fp32")


class _RfdPredictor(nn.ModuleDict):
    """Linear -> ReLU -> Linear with the reference nn.Sequential's keys "0" and "2"
    (models.py:119-123); the ReLU is fused into the first GEMM's epilogue."""

    def __init__(self, input_dim, hidden, out):
        super().__init__({"0": HipLinear(input_dim, hidden, relu=True), "2": HipLinear(hidden, out, out_fp32=True)})

    def forward(self, x, link_in=None):
        return self["2"](self["0"](x, link_in=link_in))


class BaseModel(nn.Module):
    used_params = []

    def __init__(self, model_name="BaseModel", config: Config = None):
        super().__init__()
        self.model_name = model_name
        self.config = config

    @classmethod
    def from_config(cls, config: Config):
        name = config.model_name.lower()
        from .layers import compute_dtype_of
        if compute_dtype_of(config) != torch.float32 and name not in ("dcnv2", "dnn", "deepfm", "autoint"):
            raise NotImplementedError("compute_dtype=bf16 is built for DCNv2, DNN, DeepFM and AutoInt, "
                                      f"not {config.model_name}")
        if name == "dcnv2":
            return DCNV2(config)
        if name == "dnn":
            return DNN(config)
        if name == "deepfm":
            return DeepFM(config)
        if name == "autoint":
            return AutoInt(config)
        if name == "xdeepfm":
            return xDeepFM(config)
        if name == "trans":
            return Transformer(config)
        if name == "fgcnn":
            return FGCNN(config)
        if name in _OTHER_BACKBONES:
            raise NotImplementedError(
                f"{config.model_name}: mapx builds the DCNv2 hot path and, of the other backbones "
                "(SURVEY §8 f4), DNN, DeepFM, xDeepFM, AutoInt, the Transformer and FGCNN")
        raise NotImplementedError(config.model_name)

    def validate_model_config(self):
        logger.info(f"  model_name = {self.model_name}")
        for key in self.used_params:
            logger.info(f"  {key} = {getattr(self.config, key)}")

    # ------------------------------------------------------------------ heads
    def _sample_early(self, labels, masked_index, noise_samples):
        """MFP over a single-stream trunk (DNN, DeepFM, xDeepFM, AutoInt, trans, FGCNN): the NCE head's sampling and the lazy
        catch-up of the sampled rows need only the targets — they run on the tower stream beside the trunk instead of
        between the trunk and the loss (as DCNV2.forward does by hand).  -> (ids | None, the open fork | None)."""
        if not (self.config.pretrain and self.config.pt_type == "MFP" and masked_index is not None
                and labels is not None and labels.is_cuda):
            return None, None
        with ops.Fork(ops.aux_stream("tower", labels.device), torch.cuda.current_stream()) as fork:
            idx = self.mfp_criterion.sample_ids(labels, noise_samples)
        fork.reads(labels)
        return idx, fork

    def _plans_and_join(self, idx, fork):
        """Behind the trunk: the tables' segment plans from ONE chain of launches per two tables (behind what the main
        stream holds), then the main stream takes the sampled ids over.  The trunk's tables: `embed`, and FGCNN's second
        embedding `fg_embed`."""
        trunk = [self.embed.table]
        if getattr(self, "fg_embed", None) is not None:
            trunk.append(self.fg_embed.table)
        if fork is None:
            for tb in trunk:
                tb.start_plan()
            return
        from .layers import PlanSlot
        if self.mfp_criterion.table.plan is not None and all(tb.plan is not None for tb in trunk):
            PlanSlot.start_many([tb.plan for tb in trunk] + [self.mfp_criterion.table.plan], after=fork.origin)
        else:
            for tb in trunk:
                tb.start_plan()
        fork.join()
        fork.produces(idx)

    def get_outputs(self, inputs, labels=None, masked_index=None, is_pretrain=None, noise_samples=None,
                    groups=None, nce_idx=None, join=None):
        """MFP -> (loss, #signals, #targets ranked first)            (models.py:71-78)
        RFD -> (loss, #signals, accuracy, positive ratio)            (models.py:79-85)
        CTR -> (loss, logits) or (logits,)                           (models.py:88-93)
        `#targets ranked first` is a device scalar (no host sync per step); the reference
        returns a Python int after `.item()`.  `join`: the layers._JoinLink of a two-tower trunk whose output
        `inputs` is (the head's first layer then does both towers' first backward step in its dX epilogue)."""
        cfg = self.config
        if (is_pretrain is None and cfg.pretrain) or is_pretrain:
            if cfg.pt_type == "MFP":
                crit = self.mfp_criterion
                if (crit.supports_grouped_encoder() and inputs.shape[1] % 8 == 0
                        and inputs.dtype == torch.float32):
                    # only the L masked fields' blocks of feat_encoder are computed (26 %)
                    loss, _logits, _idx = crit.forward_with_encoder(labels, inputs, self.feat_encoder,
                                                                    masked_index, noise_samples=noise_samples,
                                                                    groups=groups, idx=nce_idx, join=join)
                else:
                    # (bf16 mode: the dense encoder GEMM — 16x the MFMA rate makes computing all F blocks
                    # cheaper than the grouped GEMM's gathers; its output and the whole NCE head stay fp32)
                    enc = self.feat_encoder(inputs, link_in=join)
                    loss, _logits, _idx = crit(labels, enc, masked_index=masked_index,
                                               noise_samples=noise_samples, idx=nce_idx)
                return (loss, labels.shape[0] * labels.shape[1], self.mfp_criterion.last_acc)
            if cfg.pt_type == "RFD":
                logits = self.pred_rfd(inputs, link_in=join)
                loss, stats = bce_with_logits(logits, labels)
                return (loss, labels.shape[0] * labels.shape[1], stats[1], stats[2])
            raise NotImplementedError(cfg.pt_type)
        outputs = (inputs,)
        if labels is not None:
            loss, _ = bce_with_logits(inputs.view(-1), labels.float())
            outputs = (loss,) + outputs
        return outputs

    def create_pretraining_predictor(self, input_dim):
        cfg = self.config
        if cfg.pt_type == "MFP":
            self.feat_encoder = HipLinear(input_dim, cfg.num_fields * cfg.proj_size, out_fp32=True)
            self.mfp_criterion = IndexLinear(cfg)
        elif cfg.pt_type == "RFD":
            self.pred_rfd = _RfdPredictor(input_dim, cfg.num_fields * cfg.proj_size, cfg.num_fields)
        else:
            raise NotImplementedError(cfg.pt_type)

    # ------------------------------------------------------------------ checkpoints
    def load_from_target_model(self, target_model_dict):
        """Copy every tensor whose NAME and SHAPE match; report the rest (models.py:97-107)."""
        own = self.state_dict()
        skipped = []
        for k, v in target_model_dict.items():
            if k in own and own[k].shape == v.shape:
                own[k] = v
                logger.info(f"Load tensor: {k}, {tuple(v.shape)}")
            else:
                skipped.append(k)
                logger.info(f"Unmatched tensor in the target model: {k}, {tuple(v.shape)}")
        self.load_state_dict(own)
        return skipped

    def load_for_finetune(self, model_path):
        return self.load_from_target_model(torch.load(model_path, map_location="cpu"))

    def row_tables(self):
        """The [V,*] tables with row-sparse gradients (optimised by mapx.optim.TableAdam)."""
        return [m.table for m in self.modules() if hasattr(m, "table")]

    def table_parameter_ids(self):
        ids = set()
        for t in self.row_tables():
            ids.add(id(t.p0))
            if t.p1 is not None:
                ids.add(id(t.p1))
        return ids


class DCNV2(BaseModel):
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act",
                   "num_cross_layers"]

    def __init__(self, config: Config):
        super().__init__(model_name="DCNV2", config=config)
        self.embed = Embeddings(config)
        self.embed.defer_plan = True                 # forward() picks the fork point of the sort
        self.embed.table.mark_dense_ready = True     # the gather's backward node is this model's last one
        input_dim = config.num_fields * config.embed_size
        self.cross_net = CrossNetV2(input_dim, config.num_cross_layers)
        final_dim = input_dim
        if config.num_hidden_layers > 0:
            self.parallel_dnn = MLPBlock(input_dim=input_dim, hidden_size=config.hidden_size,
                                         num_hidden_layers=config.num_hidden_layers,
                                         hidden_dropout_rate=config.hidden_dropout_rate,
                                         hidden_act=config.hidden_act)
            final_dim += config.hidden_size
        if config.pretrain:
            self.create_pretraining_predictor(final_dim)
        else:
            self.fc_out = HipLinear(final_dim, 1, out_fp32=True)

    def _mfp_head(self, masked_index):
        return self.config.pretrain and self.config.pt_type == "MFP" and masked_index is not None

    def _grouped_head(self, masked_index):
        return (self._mfp_head(masked_index) and self.embed.compute_dtype == torch.float32
                and self.mfp_criterion.supports_grouped_encoder()
                and self.feat_encoder.in_features % 8 == 0)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        groups, nce_idx, join = None, None, None
        feat_embed = ops.flat_rows(self.embed(input_ids))
        if self.config.num_hidden_layers > 0:
            # Three independent chains leave the gather: the cross tower (small D x D GEMMs on a
            # second stream that fill the tails of the deep tower's big ones; autograd replays the
            # same stream assignment in backward), the deep tower (main stream) and the sort for
            # the embedding gradient's segment plan.  The sort is enqueued LAST but forks from the
            # event where its keys were final: a captured hipGraph keeps the first-captured
            # successor of a node on the node's queue, and a chain of tiny kernels there starves
            # the other queues (measured: the trunk's first GEMM started 150 us late).
            main = torch.cuda.current_stream()
            tower = ops.aux_stream("tower", feat_embed.device)
            fork = ops.Fork(tower, main)

            # both towers write their last layer straight into the concatenated buffer
            D, H = feat_embed.shape[1], self.config.hidden_size
            direct = self.config.num_cross_layers > 0
            if (direct and torch.is_grad_enabled() and feat_embed.dtype == torch.float32
                    and self.parallel_dnn.act == "relu"
                    and not (self.parallel_dnn.p_drop > 0 and self.training)):
                from .layers import _JoinLink
                join = _JoinLink(D)            # towers -> the head's first layer (fused backward epilogue)
            x0_link = None
            if (direct and torch.is_grad_enabled() and self.embed.table.plan is not None
                    and not self.embed.embed_norm and not (self.embed.dropout.p > 0 and self.training)):
                from .layers import _X0Link
                x0_link = _X0Link(main)        # cross tower -> the gather's backward (no elementwise add, no wait)
            self.embed.table.x0_link = x0_link
            final_buf = torch.empty(feat_embed.shape[0], D + H, dtype=feat_embed.dtype, device=feat_embed.device)
            if feat_embed.dtype == torch.float32:
                # ONE magnitude record for the concatenated output: both towers' last kernels raise it (ops.out_record)
                ops.tag(final_buf, ops.amax_record(final_buf.device))
            if layout_on_main(D) and self._grouped_head(masked_index):
                # the grouped encoder's slot layout (one 15-us launch) ahead of the deep tower, which by now
                # has ~45 us of slack against the cross tower's stream (round 1 had it the other way round)
                groups = ops.EncGroups(masked_index, self.config.num_fields)
            with fork:
                if self._grouped_head(masked_index) and groups is None:
                    # the cross tower has ~70 us of slack against the deep one: the slot layout of
                    # the grouped encoder (one single-workgroup launch) rides on its stream
                    groups = ops.EncGroups(masked_index, self.config.num_fields)
                if self._mfp_head(masked_index) and labels is not None \
                        and (groups is not None or self.embed.compute_dtype != torch.float32):
                    # the NCE head's sampling and the lazy catch-up of the sampled rows need only
                    # the targets: HBM-bound kernels that run beside the deep tower's first GEMMs
                    # instead of alone between the towers and the loss (same branch, no new one)
                    nce_idx = self.mfp_criterion.sample_ids(labels, noise_samples)
                cross_output = self.cross_net(feat_embed, out=ops.alias_cols(final_buf, 0, D) if direct else None,
                                              link=join, x0_link=x0_link)
            dnn_output = self.parallel_dnn(feat_embed, out=ops.alias_cols(final_buf, D, H) if direct else None,
                                           link_last=join.relu if join is not None else None)
            # Both tables' segment plans from ONE chain of launches (8 instead of 8 + 8, 0.112 instead of 0.19 ms of
            # sorting per step), when the sampled ids exist already (drawn early on the tower stream).  The chain
            # waits for the deep tower's GEMMs to be on their way: captured as a branch of its own the graph runtime
            # ran it ahead of them on the queue the two share.
            if nce_idx is not None:
                from .layers import PlanSlot
                # (the tower stream forked from the main one behind the gather: the sampled ids' event
                # implies that the embedding's keys are final)
                PlanSlot.start_many([self.embed.table.plan, self.mfp_criterion.table.plan],
                                    implied=[self.embed.table.plan], after=main)
            else:
                # (RFD / finetune steps: one table, one chain)
                f32_trunk = self.embed.compute_dtype == torch.float32
                self.embed.table.start_plan(after=main if plan_after_main(self.config.pretrain, f32_trunk, D) else tower)
            fork.join()
            fork.reads(feat_embed, final_buf)
            if groups is not None:
                fork.reads(masked_index)
                fork.produces(*groups.tensors())
            if nce_idx is not None:
                fork.reads(labels)
                fork.produces(nce_idx)
            final_output = ops.carry(_JoinColumns.apply(cross_output, dnn_output, final_buf, join), final_buf) if direct \
                else torch.cat([cross_output, dnn_output], dim=-1)
            if self._mfp_head(masked_index):
                # the towers' join node and the cross tower's node run behind the head's backward: it may leave them
                # a stream join and the table's gradient (nce._NceLoss.backward)
                self.mfp_criterion.towers_follow = direct and torch.is_grad_enabled()
        else:
            self.embed.table.x0_link = None
            final_output = self.cross_net(feat_embed)
            self.embed.table.start_plan()
        if self.config.pretrain:
            return self.get_outputs(final_output, labels, masked_index, noise_samples=noise_samples, groups=groups,
                                    nce_idx=nce_idx, join=join)
        return self.get_outputs(self.fc_out(final_output, link_in=join), labels)


class DNN(BaseModel):
    """Embeddings -> MLP -> head (reference models.py:164-193).  Same heads, tables and optimizer
    path as DCNV2; only the trunk differs."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act"]

    def __init__(self, config: Config):
        super().__init__(model_name="DNN", config=config)
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        self.dnn = MLPBlock(input_dim=config.embed_size * config.num_fields, hidden_size=config.hidden_size,
                            num_hidden_layers=config.num_hidden_layers,
                            hidden_dropout_rate=config.hidden_dropout_rate, hidden_act=config.hidden_act)
        if config.pretrain:
            self.create_pretraining_predictor(config.hidden_size)
        else:
            self.fc_out = HipLinear(config.hidden_size, 1, out_fp32=True)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        feat_embed = ops.flat_rows(self.embed(input_ids))
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        nn_output = self.dnn(feat_embed)
        self._plans_and_join(nce_idx, early)     # the sort(s) fork from the ids, enqueued behind the trunk
        if self.config.pretrain:
            return self.get_outputs(nn_output, labels, masked_index, noise_samples=noise_samples, nce_idx=nce_idx)
        return self.get_outputs(self.fc_out(nn_output), labels)


class LR(nn.Module):
    """First-order term (reference models.py:129-143): `embed_w` [V,1] + `bias` [1].  In DeepFM the
    weight is the secondary parameter of the embedding's RowTable (same ids, one gradient plan);
    the reference initialises it like any nn.Embedding, N(0, 1)."""

    def __init__(self, config: Config):
        super().__init__()
        self.embed_w = TableWeight(config.input_size, 1)
        with torch.no_grad():
            self.embed_w.weight.normal_(0.0, 1.0)
        self.bias = nn.Parameter(torch.zeros(1))


class _InnerProductBuffers(nn.Module):
    """The reference's InnerProductLayer keeps three index tensors as frozen Parameters
    (layers.py:116-121); they appear in its state_dict, so they do here (as buffers)."""

    def __init__(self, num_fields):
        super().__init__()
        iu = torch.triu_indices(num_fields, num_fields, offset=1)
        self.register_buffer("field_p", iu[0].clone())
        self.register_buffer("field_q", iu[1].clone())
        self.register_buffer("upper_triangle_mask",
                             torch.triu(torch.ones(num_fields, num_fields), 1).bool())


class DeepFM(BaseModel):
    """LR + FM(product_sum) + MLP (reference models.py:196-233).  Pretraining feeds
    cat([dnn_vec, lr + fm]) [B, H+1] to the MFP / RFD heads; CTR sums the three logits.
    compute_dtype=bf16: the gathered rows and the MLP are bf16; the LR sum, the FM term and lr + bias + fm [B,1] stay
    fp32 — rounded once where that column joins the heads' bf16 input, added in fp32 to the CTR logit."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act"]
    FM_EMBED_SIZES = (4, 8, 16, 32, 64)

    def __init__(self, config: Config):
        super().__init__(model_name="DeepFM", config=config)
        _refuse_bf16_mlp_options(config, "hidden_act", "hidden_dropout_rate")
        if config.embed_size not in self.FM_EMBED_SIZES:      # (csrc/fm.hip refuses the others inside the first forward)
            raise NotImplementedError(f"DeepFM: the FM kernels take embed_size in {self.FM_EMBED_SIZES} "
                                      f"(embed_size={config.embed_size})")
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        self.lr_layer = LR(config)
        # one row table for both [V,*] parameters read with input_ids
        self.embed.table = RowTable("embed.embedding", self.embed.embedding.weight, self.lr_layer.embed_w.weight)
        self.dnn = MLPBlock(input_dim=config.num_fields * config.embed_size, hidden_size=config.hidden_size,
                            num_hidden_layers=config.num_hidden_layers,
                            hidden_dropout_rate=config.hidden_dropout_rate, hidden_act=config.hidden_act)
        self.ip_layer = _InnerProductBuffers(config.num_fields)
        if config.pretrain:
            self.create_pretraining_predictor(config.hidden_size + 1)
        else:
            self.dnn_fc_out = HipLinear(config.hidden_size, 1, out_fp32=True)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        x3, lr = self.embed.forward_with_linear(input_ids, self.lr_layer.embed_w.weight)
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        dnn_vec = self.dnn(ops.flat_rows(x3))
        self._plans_and_join(nce_idx, early)
        lr_fm = lr.view(-1, 1) + self.lr_layer.bias + fm_product_sum(x3)
        if self.config.pretrain:
            final_vec = torch.cat([dnn_vec, to_bf16(lr_fm) if ops.is_bf16(dnn_vec) else lr_fm], dim=1)
            return self.get_outputs(final_vec, labels, masked_index, noise_samples=noise_samples, nce_idx=nce_idx)
        return self.get_outputs(self.dnn_fc_out(dnn_vec) + lr_fm, labels)


class AutoInt(BaseModel):
    """Stacked multi-head self-attention over the field embeddings (reference models.py:440-488);
    the flattened [B, F*heads*attn_size] output feeds the MFP / RFD heads or `attn_out`; the finetune model adds
    the LR term (use_lr: its weight is the secondary parameter of the embedding's RowTable, as in DeepFM) and an MLP
    tower over the flattened embeddings (num_dnn_layers > 0: `dnn` + `dnn_out`), models.py:464-471, 482-486.
    attn_probs_dropout_rate > 0: two dropouts per attention layer, drawn inside csrc/attn.hip.
    compute_dtype=bf16: the gathered rows, q, k, v, the attention output and every layer's output are bf16 (the bf16
    I/O forms of csrc/attn.hip, bf16 GEMMs on the weights' shadows); the probabilities, the LR term and the logits of
    attn_out / dnn_out stay fp32; attn_probs_dropout_rate > 0 works as in fp32 mode."""
    used_params = ["embed_size", "num_attn_layers", "attn_size", "num_attn_heads", "attn_probs_dropout_rate",
                   "use_lr", "res_conn", "attn_scale", "dnn_size", "num_dnn_layers", "dnn_act", "dnn_drop"]

    def __init__(self, config: Config):
        super().__init__(model_name="AutoInt", config=config)
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        HA = config.num_attn_heads * config.attn_size
        self.self_attention = nn.Sequential(*[
            MultiHeadSelfAttention(config.embed_size if i == 0 else HA, attention_dim=config.attn_size,
                                   num_heads=config.num_attn_heads, dropout_rate=config.attn_probs_dropout_rate,
                                   use_residual=config.res_conn, use_scale=config.attn_scale)
            for i in range(config.num_attn_layers)])
        final_dim = config.num_fields * HA
        if config.pretrain:
            self.create_pretraining_predictor(final_dim)
        else:
            self.attn_out = HipLinear(final_dim, 1, out_fp32=True)       # (bf16 mode: the logits stay fp32)
            # (the reference creates these for the finetune model only: models.py:463-471)
            self.lr_layer = LR(config) if config.use_lr else None
            if self.lr_layer is not None:       # one row table for both [V, *] parameters read with input_ids
                self.embed.table = RowTable("embed.embedding", self.embed.embedding.weight, self.lr_layer.embed_w.weight)
            # The reference sizes the tower's input as final_dim (fields x heads x attn_size, models.py:466) and feeds
            # it the flattened EMBEDDINGS (fields x embed_size, models.py:486): the option runs only when the two
            # agree; the same shapes and the same error otherwise.
            if config.num_dnn_layers:
                _refuse_bf16_mlp_options(config, "dnn_act", "dnn_drop")
            if config.num_dnn_layers and final_dim != config.num_fields * config.embed_size:
                raise ValueError("AutoInt with num_dnn_layers > 0 needs embed_size == num_attn_heads * attn_size "
                                 "(reference models.py:466, 486: the tower is sized for the attention output and fed "
                                 "the embeddings)")
            self.dnn = MLPBlock(input_dim=final_dim, hidden_size=config.dnn_size,
                                num_hidden_layers=config.num_dnn_layers, hidden_dropout_rate=config.dnn_drop,
                                hidden_act=config.dnn_act) if config.num_dnn_layers else None
            self.dnn_out = HipLinear(config.dnn_size, 1, out_fp32=True) if config.num_dnn_layers else None

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        lr = None
        if not self.config.pretrain and self.lr_layer is not None:
            x, lr = self.embed.forward_with_linear(input_ids, self.lr_layer.embed_w.weight)
        else:
            x = self.embed(input_ids)
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        attention_out = self.self_attention(x).flatten(start_dim=1)
        self._plans_and_join(nce_idx, early)
        if self.config.pretrain:
            return self.get_outputs(attention_out, labels, masked_index, noise_samples=noise_samples, nce_idx=nce_idx)
        logits = self.attn_out(attention_out)
        if lr is not None:
            logits = logits + (lr.view(-1, 1) + self.lr_layer.bias)         # models.py:483-484
        if self.dnn is not None:
            logits = logits + self.dnn_out(self.dnn(ops.flat_rows(x)))      # models.py:485-486
        return self.get_outputs(logits, labels)


class xDeepFM(BaseModel):
    """CIN + MLP (reference models.py:235-279): cat([CIN(embed), MLP(embed.flatten)]) — or the CIN alone when
    num_hidden_layers = 0 — feeds the MFP / RFD heads or `fc` (+ the LR term when use_lr).  The LR weight, when present, is the
    secondary parameter of the embedding's RowTable as in DeepFM.
    compute_dtype=bf16 (through build_backbone): the gathered rows, every CIN layer's output, the pooled CIN vector and
    the MLP are bf16 — the fused kernels of csrc/cin_fused.hip, which never write the Hadamard matrix, and bf16 GEMMs on
    the weights' shadows; the LR term and every logit stay fp32.  The fused kernels take 2 <= num_fields <= 64 and
    cin_layer_units in 1..128."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act",
                   "cin_layer_units", "use_lr"]

    def __init__(self, config: Config):
        super().__init__(model_name="xDeepFM", config=config)
        from .layers import compute_dtype_of
        half = compute_dtype_of(config) != torch.float32
        units = [int(c) for c in str(config.cin_layer_units).split(",")]
        if half:
            if config.num_hidden_layers > 0:
                _refuse_bf16_mlp_options(config, "hidden_act", "hidden_dropout_rate")
            if min(units) < 1 or max(units) > ops.CIN_MAX_UNITS:
                raise NotImplementedError(f"cin_layer_units={config.cin_layer_units!r}: the fused CIN kernels of "
                                          f"compute_dtype=bf16 take 1..{ops.CIN_MAX_UNITS} units per layer")
            if not 2 <= int(config.num_fields) <= ops.CIN_MAX_FIELDS:
                raise NotImplementedError(f"num_fields={config.num_fields}: the fused CIN kernels of compute_dtype=bf16 "
                                          f"take 2..{ops.CIN_MAX_FIELDS} fields")
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        self.cin = CIN(config.num_fields, units)
        if config.num_hidden_layers > 0:
            self.dnn = MLPBlock(input_dim=config.num_fields * config.embed_size, hidden_size=config.hidden_size,
                                num_hidden_layers=config.num_hidden_layers,
                                hidden_dropout_rate=config.hidden_dropout_rate, hidden_act=config.hidden_act)
            final_dim = sum(units) + config.hidden_size
        else:                                   # models.py:253-255: the CIN alone feeds the heads
            self.dnn = None
            final_dim = sum(units)
        if config.pretrain:
            self.create_pretraining_predictor(final_dim)
        else:
            self.lr_layer = LR(config) if config.use_lr else None
            if self.lr_layer is not None:
                self.embed.table = RowTable("embed.embedding", self.embed.embedding.weight,
                                            self.lr_layer.embed_w.weight)
            self.fc = HipLinear(final_dim, 1, out_fp32=half)          # (bf16 mode: the logits stay fp32)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        lr = None
        if not self.config.pretrain and self.lr_layer is not None:
            x3, lr = self.embed.forward_with_linear(input_ids, self.lr_layer.embed_w.weight)
        else:
            x3 = self.embed(input_ids)
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        final_vec = self.cin(x3)
        if self.dnn is not None:
            final_vec = torch.cat([final_vec, self.dnn(ops.flat_rows(x3))], dim=1)
        self._plans_and_join(nce_idx, early)
        if self.config.pretrain:
            return self.get_outputs(final_vec, labels, masked_index, noise_samples=noise_samples, nce_idx=nce_idx)
        logits = self.fc(final_vec)
        if lr is not None:
            logits = logits + lr.view(-1, 1) + self.lr_layer.bias
        return self.get_outputs(logits, labels)


class Transformer(BaseModel):
    """nn.TransformerEncoder over the field embeddings (reference models.py:491-568): d_model = hidden_size (which
    must equal embed_size), no final norm.  Pretraining feeds the flattened [B, F*E] encoder output to the MFP / RFD
    heads; finetuning reduces it by `output_reduction` ("fc": trans_out over F*E; "mean,fc" / "sum,fc": over fields,
    then trans_out over E; "attn,fc": softmax-weighted field sum with the weights from field_reduction_attn =
    Linear(E,E), ReLU, Linear(E,1)) and adds the LR term (use_lr: its weight is the secondary parameter of the
    embedding's RowTable, as in DeepFM) and an MLP tower over the flattened embeddings (num_dnn_layers > 0: `mlp` +
    `mlp_out`).  The attention core is csrc/mha.hip: F <= 64 fields, head size hidden_size / num_attn_heads a
    multiple of 4 and <= 64; LayerNorm over hidden_size <= 64.
    compute_dtype=bf16 (through build_backbone): the gathered rows, qkv, the attention output, every projection's and
    LayerNorm's output, the saved gelu pre-activation and the pooled vectors are bf16 — the bf16 I/O forms of
    csrc/mha.hip, the residual add + LayerNorm pair and the bf16 gelu / dropout of csrc/extras.hip, bf16 GEMMs on the
    weights' shadows; the attention probabilities, LayerNorm statistics, pooling weights, the scores of
    field_reduction_attn, the LR term and every logit stay fp32.  hidden_dropout_rate > 0 works as in fp32 mode."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act",
                   "num_attn_heads", "intermediate_size", "output_reduction",
                   "norm_first", "layer_norm_eps", "use_lr",
                   "dnn_size", "num_dnn_layers", "dnn_act", "dnn_drop"]
    REDUCTIONS = ("fc", "mean,fc", "sum,fc", "attn,fc")

    def __init__(self, config: Config):
        super().__init__(model_name="trans", config=config)
        E, H, F = int(config.hidden_size), int(config.num_attn_heads), int(config.num_fields)
        if H < 1 or E % H or (E // H) % 4 or E // H > 64:
            raise NotImplementedError(f"trans: the attention kernel takes a head size hidden_size / num_attn_heads that "
                                      f"is a multiple of 4 and <= 64 (hidden_size={E}, num_attn_heads={H})")
        if F > 64:
            raise NotImplementedError(f"trans: the attention kernel takes at most 64 fields (num_fields={F})")
        if E > 64:
            raise NotImplementedError(f"trans: LayerNorm is built for hidden_size <= 64 (hidden_size={E})")
        if not config.pretrain and config.output_reduction not in self.REDUCTIONS:
            raise NotImplementedError(f"trans: output_reduction={config.output_reduction!r} (models.py:527-545 builds "
                                      f"{', '.join(self.REDUCTIONS)})")
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        layer = TransformerEncoderLayer(E, H, config.intermediate_size, dropout=config.hidden_dropout_rate,
                                        activation=config.hidden_act, layer_norm_eps=config.layer_norm_eps,
                                        norm_first=config.norm_first)
        self.encoder = TransformerEncoder(layer, config.num_hidden_layers)
        Ee = config.embed_size
        if config.pretrain:
            self.create_pretraining_predictor(config.num_fields * Ee)
            return
        red = config.output_reduction
        if red == "attn,fc":
            self.field_reduction_attn = nn.ModuleDict({"0": HipLinear(Ee, Ee, relu=True),
                                                       "2": HipLinear(Ee, 1, out_fp32=True)})
        self.trans_out = HipLinear(config.num_fields * Ee if red == "fc" else Ee, 1, out_fp32=True)   # (bf16 mode: fp32 logits)
        self.lr_layer = LR(config) if config.use_lr else None
        if self.lr_layer is not None:          # one row table for both [V, *] parameters read with input_ids
            self.embed.table = RowTable("embed.embedding", self.embed.embedding.weight, self.lr_layer.embed_w.weight)
        if config.num_dnn_layers > 0:
            _refuse_bf16_mlp_options(config, "dnn_act", "dnn_drop")
            self.mlp = MLPBlock(input_dim=config.num_fields * Ee, hidden_size=config.dnn_size,
                                num_hidden_layers=config.num_dnn_layers, hidden_dropout_rate=config.dnn_drop,
                                hidden_act=config.dnn_act)
            self.mlp_out = HipLinear(config.dnn_size, 1, out_fp32=True)
        else:
            self.mlp = None

    def validate_model_config(self):
        assert self.config.embed_size == self.config.hidden_size, \
            f"model {self.model_name} requires embed_size == hidden_size"
        super().validate_model_config()

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        lr = None
        if not self.config.pretrain and self.lr_layer is not None:
            x, lr = self.embed.forward_with_linear(input_ids, self.lr_layer.embed_w.weight)
        else:
            x = self.embed(input_ids)
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        enc = self.encoder(x)
        self._plans_and_join(nce_idx, early)
        if self.config.pretrain:
            return self.get_outputs(enc.flatten(start_dim=1), labels, masked_index, noise_samples=noise_samples,
                                    nce_idx=nce_idx)
        red = self.config.output_reduction
        if red == "fc":
            logits = self.trans_out(enc.flatten(start_dim=1))
        elif red == "attn,fc":
            B, F, E = enc.shape
            fra = self.field_reduction_attn
            scores = fra["2"](fra["0"](enc.reshape(B * F, E))).view(B, F)
            logits = self.trans_out(field_pool(enc, "attn", scores))
        else:
            logits = self.trans_out(field_pool(enc, red.split(",")[0]))
        if lr is not None:
            logits = logits + (lr.view(-1, 1) + self.lr_layer.bias)          # models.py:562-563
        if self.mlp is not None:
            logits = logits + self.mlp_out(self.mlp(ops.flat_rows(x)))      # models.py:564-565
        return self.get_outputs(logits, labels)


def _int_list(config, key):
    try:
        return [int(c) for c in str(getattr(config, key)).split(",")]
    except ValueError:
        raise ValueError(f"{key}={getattr(config, key)!r}: a comma list of integers") from None


class FGCNN(BaseModel):
    """Feature generation by convolution (reference models.py:325-407): a second embedding `fg_embed` of the same ids
    (or `embed` itself with share_embedding) goes through FGCNNBlock (Conv2d (kh,1) -> BatchNorm2d -> conv_act ->
    MaxPool2d (ps,1) -> recombine Linear -> conv_act per stage); the new feature rows are concatenated behind the
    embeddings to `combined` [B,T,E], and cat([combined.flatten(1), upper triangle of combined combined^T]) feeds the
    MFP / RFD heads, or `dnn` + `fc_out` (fc_out alone when num_hidden_layers = 0).  Conv, batch norm, pooling and the
    inner products are csrc/fgcnn.hip: at most 32 channels, odd kernel heights <= 15, T <= 192 rows, conv_act tanh |
    relu.  Batch norm keeps per-replica buffers that the reference's DistributedDataParallel re-broadcasts from
    rank 0 at every forward; that is not built, so the model trains on one replica only (`single_replica_only`).
    compute_dtype=bf16 (through build_backbone): the gathered rows, every stage's input, the saved conv
    output z, the pooled output, the recombine layers' outputs, `combined`, the inner products, dense_input and the MLP
    activations are bf16 (the bf16 I/O forms of csrc/fgcnn.hip, bf16 GEMMs on the weights' shadows); the conv weights,
    the batch-norm parameters, statistics and buffers, g = dL/du inside a stage's backward, every parameter gradient and
    the heads' logits stay fp32.  hidden_act != relu and hidden_dropout_rate > 0 are refused at construction."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act",
                   "share_embedding", "channels", "kernel_heights", "pooling_sizes", "recombined_channels",
                   "conv_act"]
    MAX_ROWS = 192        # csrc/fgcnn.hip kIpMaxT
    MAX_LDS = 128 * 1024  # csrc/fgcnn.hip kFgLdsLimit: weights + one sample's input and gradient slabs
    single_replica_only = ("model_name=fgcnn trains on one replica: its BatchNorm buffers (running_mean, running_var, "
                           "num_batches_tracked) would have to be broadcast from rank 0 at every forward, as the "
                           "reference's DistributedDataParallel does, and that is not built")

    def __init__(self, config: Config):
        super().__init__(model_name="fgcnn", config=config)
        from .layers import compute_dtype_of
        half = compute_dtype_of(config) != torch.float32
        if not config.pretrain and config.num_hidden_layers > 0:
            _refuse_bf16_mlp_options(config, "hidden_act", "hidden_dropout_rate")
        lists = {k: _int_list(config, k) for k in ("channels", "kernel_heights", "pooling_sizes", "recombined_channels")}
        if len({len(v) for v in lists.values()}) != 1:
            raise ValueError("channels, kernel_heights, pooling_sizes and recombined_channels must list one value per "
                             "stage each, got " + ", ".join(f"{k}={getattr(config, k)!r}" for k in lists))
        if any(kh < 1 or kh % 2 == 0 for kh in lists["kernel_heights"]):
            raise NotImplementedError(f"kernel_heights={config.kernel_heights!r}: odd heights only (an even height "
                                      "changes the stage's height, which the reference's own bookkeeping of the "
                                      "recombine layers' widths does not follow)")
        if max(lists["kernel_heights"]) > 15 or max(lists["channels"]) > 32:
            raise NotImplementedError(f"channels={config.channels!r}, kernel_heights={config.kernel_heights!r}: the "
                                      "convolution kernels take at most 32 channels and kernel heights up to 15")
        if min(lists["channels"] + lists["pooling_sizes"] + lists["recombined_channels"]) < 1:
            raise ValueError("channels, pooling_sizes and recombined_channels must be positive")
        c_in, height = 1, config.num_fields
        for c, kh, ps in zip(lists["channels"], lists["kernel_heights"], lists["pooling_sizes"]):
            lds = 4 * (c * c_in * kh + (c_in + c) * height * config.embed_size)
            if lds > self.MAX_LDS:
                raise NotImplementedError(
                    f"fgcnn: a stage of {c_in} -> {c} channels over {height} rows of embed_size={config.embed_size} "
                    f"needs {lds} bytes of LDS in the convolution's backward kernel, above {self.MAX_LDS}: lower "
                    f"embed_size or channels={config.channels!r}")
            c_in, height = c, -(-height // ps)
        self.share_embedding = bool(config.share_embedding)
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        if not self.share_embedding:
            # a second table over the same ids, with its own optimizer state and fingerprint entries
            self.fg_embed = Embeddings(config)
            self.fg_embed.defer_plan = True
            self.fg_embed.table = RowTable("fg_embed.embedding", self.fg_embed.embedding.weight)
        else:
            self.fg_embed = None
        self.fgcnn_layer = FGCNNBlock(config.num_fields, config.embed_size, lists["channels"], lists["kernel_heights"],
                                      lists["pooling_sizes"], lists["recombined_channels"], activation=config.conv_act)
        final_dim, total = self.compute_input_dim(config.embed_size, config.num_fields, lists["channels"],
                                                  lists["pooling_sizes"], lists["recombined_channels"])
        if total > self.MAX_ROWS or config.embed_size > 64:
            raise NotImplementedError(f"fgcnn: the inner-product kernel takes at most {self.MAX_ROWS} feature rows of "
                                      f"embed_size <= 64 (num_fields, pooling_sizes and recombined_channels give "
                                      f"{total} rows, embed_size={config.embed_size})")
        self.final_dim, self.total_features = final_dim, total
        self.ip_layer = _InnerProductBuffers(total)
        if config.pretrain:
            self.create_pretraining_predictor(final_dim)
        elif config.num_hidden_layers > 0:
            self.dnn = MLPBlock(input_dim=final_dim, hidden_size=config.hidden_size,
                                num_hidden_layers=config.num_hidden_layers,
                                hidden_dropout_rate=config.hidden_dropout_rate, hidden_act=config.hidden_act)
            self.fc_out = HipLinear(config.hidden_size, 1, out_fp32=half)          # (bf16 mode: the logits stay fp32)
        else:
            self.dnn = None
            self.fc_out = HipLinear(final_dim, 1, out_fp32=half)

    @staticmethod
    def compute_input_dim(embedding_dim, num_fields, channels, pooling_sizes, recombined_channels):
        """-> (width of the heads' input, T = rows of `combined`)   (models.py:369-382)."""
        total = height = num_fields
        for i in range(len(channels)):
            height = -(-height // pooling_sizes[i])
            total += height * recombined_channels[i]
        return total * (total - 1) // 2 + total * embedding_dim, total

    def combined_features(self, input_ids, between=None):
        """cat([embed(ids), FGCNNBlock(fg_embed(ids))], dim=1) [B,T,E]; `between`: called behind the gathers."""
        feat_embed = self.embed(input_ids)
        feat_embed2 = feat_embed if self.fg_embed is None else self.fg_embed(input_ids)
        if between is not None:
            between()
        return torch.cat([feat_embed, self.fgcnn_layer(feat_embed2.unsqueeze(1))], dim=1)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        early = [None, None]

        def sample():           # (as the other single-stream trunks: behind the gathers, beside the trunk)
            early[0], early[1] = self._sample_early(labels, masked_index, noise_samples)
        combined = self.combined_features(input_ids, between=sample)
        nce_idx, early = early
        dense_input = torch.cat([combined.flatten(start_dim=1), inner_product(combined)], dim=1)
        self._plans_and_join(nce_idx, early)
        if self.config.pretrain:
            return self.get_outputs(dense_input, labels, masked_index, noise_samples=noise_samples, nce_idx=nce_idx)
        if self.dnn is not None:
            dense_input = self.dnn(dense_input)
        return self.get_outputs(self.fc_out(dense_input), labels)


class FiGNN(BaseModel):
    """Field interactions on a per-sample attention graph (reference models.py:410-438): Embeddings -> FiGNNBlock
    (the graph from W_attn once, then num_hidden_layers steps of GraphLayer + one shared GRUCell, optional residual to
    the embeddings, optionally ONE GraphLayer for all steps) -> the flattened [B, F*E] state feeds the MFP / RFD heads,
    or `fc` = AttentionalPrediction.  Only embed_size is used (the reference warns that hidden_size should equal it
    and goes on).  The trunk is csrc/fignn.hip: fp32, embed_size % 4 == 0 and <= 32, 2 <= num_fields <= 64."""
    used_params = ["embed_size", "hidden_size", "num_hidden_layers", "hidden_dropout_rate", "hidden_act",
                   "res_conn", "reuse_graph_layer"]
    MAX_FIELDS, MAX_EMBED = ops.FIGNN_MAX_FIELDS, ops.FIGNN_MAX_EMBED

    def __init__(self, config: Config):
        super().__init__(model_name="FiGNN", config=config)
        from .layers import compute_dtype_of
        if compute_dtype_of(config) != torch.float32:
            raise NotImplementedError("compute_dtype=bf16 is not built for fignn: its graph / GRU kernels are fp32")
        E, F, L = int(config.embed_size), int(config.num_fields), int(config.num_hidden_layers)
        if E % 4 or E < 4 or E > self.MAX_EMBED:
            raise NotImplementedError(f"fignn: the graph / GRU kernels take embed_size % 4 == 0 and <= {self.MAX_EMBED} "
                                      f"(embed_size={E})")
        if F < 2 or F > self.MAX_FIELDS:
            raise NotImplementedError(f"fignn: the graph kernels take 2 <= num_fields <= {self.MAX_FIELDS} "
                                      f"(num_fields={F}; with one field the reference's masked softmax is NaN)")
        if L < 1:
            raise NotImplementedError(f"fignn: num_hidden_layers >= 1 graph steps (num_hidden_layers={L})")
        if int(config.hidden_size) != E:
            logger.warning("this model requires embed_size == hidden_size, only uses embed_size")
        self.embed = Embeddings(config)
        self.embed.defer_plan = True
        self.fignn = FiGNNBlock(config)
        if config.pretrain:
            self.create_pretraining_predictor(F * E)
        else:
            self.fc = AttentionalPrediction(config)

    def forward(self, input_ids, labels=None, masked_index=None, noise_samples=None):
        x = self.embed(input_ids)
        nce_idx, early = self._sample_early(labels, masked_index, noise_samples)
        h = self.fignn(x)
        self._plans_and_join(nce_idx, early)
        if self.config.pretrain:
            return self.get_outputs(h.flatten(start_dim=1), labels, masked_index, noise_samples=noise_samples,
                                    nce_idx=nce_idx)
        return self.get_outputs(self.fc(h), labels)


def build_backbone(config: Config):
    """Every model name the reference's factory reaches: FiGNN, and the Transformer, xDeepFM and FGCNN in
    compute_dtype=bf16 here, the rest through BaseModel.from_config (which still refuses fignn, and trans / xDeepFM /
    fgcnn with bf16, as existing tests pin; making it delegate is a one-line follow-up)."""
    from .layers import compute_dtype_of
    name = str(config.model_name).lower()
    if name == "trans" and compute_dtype_of(config) != torch.float32:
        return Transformer(config)
    if name == "xdeepfm" and compute_dtype_of(config) != torch.float32:
        return xDeepFM(config)
    if name == "fgcnn" and compute_dtype_of(config) != torch.float32:
        return FGCNN(config)
    if name == "fignn":
        if compute_dtype_of(config) != torch.float32:
            raise NotImplementedError("compute_dtype=bf16 is built for DCNv2, DNN, DeepFM and AutoInt, "
                                      f"not {config.model_name}")
        return FiGNN(config)
    return BaseModel.from_config(config)
