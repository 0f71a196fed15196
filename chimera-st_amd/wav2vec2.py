"""wav2vec2 feature path (features_only) — mirror of fairseq/models/wav2vec/wav2vec2.py on the Chimera
path: ConvFeatureExtractionModel (:685-763), Wav2Vec2Model.forward features_only branch (:527-586) and
extract_features (:650-652), TransformerEncoder (:766-861), TransformerSentenceEncoderLayer (:864-959).

The pre-training forward (:527-641, forward_pretrain below: quantizer, negatives, the operands of the fused InfoNCE loss) runs on the
kernels of csrc/w2v_pretrain.hip; padded batches, --quantize-input, --target-glu, --negatives-from-everywhere and
--codebook-negatives are refused.  The parameters of the pre-training heads that exist in every checkpoint (mask_emb, project_q, final_proj) are kept so
state dicts round-trip.  Fine-tuning's time / channel masking (apply_mask :414-452 over
data_utils.compute_mask_indices) is built for wav2vec2_asr.py: forward(mask=True).

MI355X layout: the whole CNN runs channels-last [B, L, C] so every conv after layer 0 is an implicit GEMM on
MFMA tiles with the GELU in the epilogue, and `features.transpose(1, 2)` (:539) is free."""
import math
import os
from argparse import Namespace

import numpy as np
import torch
import torch.nn as nn

from . import functional as CF
from . import kernels as K
from .distributed import notify_unused_parameters
from .modules import LayerNorm, Linear, MultiheadAttention, to_batch_major, to_time_major_view
from .registry import register_model, register_model_architecture


class _Slot(nn.Module):
    """Parameter holder that keeps the reference's nn.Sequential index in state-dict keys (conv_layers.N.0.weight ...)."""


class ConvFeatureExtractionModel(nn.Module):
    """wav2vec2.py:685-763.  mode "default": layer 0 = Conv1d+GroupNorm(C,C)+GELU, layers 1.. = Conv1d+GELU;
    mode "layer_norm" (the published large models): every layer = Conv1d+LayerNorm over channels (fp32 statistics)+GELU.
    conv_bias adds a bias to every conv.  State-dict keys are the reference's: conv_layers.N.0.{weight,bias} for the conv,
    conv_layers.N.2.{weight,bias} for layer 0's GroupNorm, conv_layers.N.2.1.{weight,bias} for a layer's LayerNorm."""

    def __init__(self, conv_layers, dropout=0.0, mode="default", conv_bias=False):
        super().__init__()
        assert mode in {"default", "layer_norm"}, "extractor_mode must be default or layer_norm, not %r" % (mode,)
        assert dropout == 0.0
        if mode == "default" and conv_bias:
            # layer 0's GroupNorm kernel derives its statistics from lag moments of the audio (csrc/conv0.hip), which a bias would
            # have to enter as extra terms; no published checkpoint uses this combination
            raise NotImplementedError("extractor_mode=default with conv_bias=True is not built (no published wav2vec2 model uses it); "
                                      "extractor_mode=layer_norm takes conv_bias")
        self.mode, self.conv_bias = mode, bool(conv_bias)
        self.conv_spec = [tuple(c) for c in conv_layers]
        self.conv_layers = nn.ModuleList()
        in_d = 1
        for i, (dim, k, stride) in enumerate(self.conv_spec):
            blk = nn.Module()
            conv = nn.Module()
            conv.weight = nn.Parameter(torch.empty(dim, in_d, k))
            nn.init.kaiming_normal_(conv.weight)
            if conv_bias:  # nn.Conv1d's default bias init: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                bound = 1.0 / math.sqrt(in_d * k)
                conv.bias = nn.Parameter(torch.empty(dim).uniform_(-bound, bound))
            blk.add_module("0", conv)
            if mode == "layer_norm":  # nn.Sequential(TransposeLast(), Fp32LayerNorm(dim), TransposeLast()) at index 2
                seq = nn.Module()
                ln = nn.Module()
                ln.weight = nn.Parameter(torch.ones(dim))
                ln.bias = nn.Parameter(torch.zeros(dim))
                seq.add_module("1", ln)
                blk.add_module("2", seq)
            elif i == 0:
                gn = nn.Module()
                gn.weight = nn.Parameter(torch.ones(dim))
                gn.bias = nn.Parameter(torch.zeros(dim))
                blk.add_module("2", gn)
            self.conv_layers.append(blk)
            in_d = dim

    def forward(self, x, nz_last=None):
        """x [B,S] raw samples -> channels-last features [B, T1, C] (the reference returns [B,C,T1]).
        nz_last (int32 [B], optional): the caller guarantees that the gradient of the returned features is exactly zero at frames
        t >= nz_last[b] (wav2vec2 zeroes the padded frames, wav2vec2.py:820-821).  The bound is carried down the stack — a
        frame t of layer i+1 reads rows [s t, s t + k) of layer i, so layer i's gradient is zero from (nz - 1) s + k on — and the
        weight-gradient GEMMs of each layer stop their reduction over frames there (cst_gemm_desc.k_len): exact."""
        nz = [None] * len(self.conv_spec)
        res = [None] * len(self.conv_spec)
        lim = None
        if nz_last is not None:
            # nz[i][b]: frames of layer i that anything reads; res[i][r][b]: live rows of residue class r of layer i's input gradient
            lim = K.conv_row_limits(nz_last.to(torch.int32).contiguous(), self.conv_spec, x.shape[1])
            for i, (_, _, st_) in enumerate(self.conv_spec):
                nz[i] = lim[i, 0]
                res[i] = lim[i, 1:1 + st_]
        if self.mode == "layer_norm":
            return self._forward_layer_norm(x, lim, nz, res)
        l0 = self.conv_layers[0]
        dim, k, stride = self.conv_spec[0]
        # layer 0 writes only the frames layer 1's live tiles read, its backward reads only the frames that carry gradient
        y = CF.conv0_gn_gelu(x, getattr(l0, "0").weight, getattr(l0, "2").weight, getattr(l0, "2").bias, stride,
                             write_limit=lim[0, 1] if lim is not None and len(self.conv_spec) > 1 else None,
                             grad_limit=nz[0])
        z = None
        n = len(self.conv_spec)
        for i in range(1, n):
            dim, k, stride = self.conv_spec[i]
            w = getattr(self.conv_layers[i], "0").weight
            # fold GELU' of layer i-1 into layer i's col2im pass; layer i then receives d/dz directly
            # rows t >= nz[i][b] of layer i are frames nobody reads (the stack's output is zeroed behind the utterance's end,
            # wav2vec2.py:820-821) and whose gradient is exactly zero: their GEMM tiles skip the K loop (cst_gemm_desc.m_len / k_len)
            y, z = CF.conv1d_cl(y, w, None, stride, pad=0, act="gelu", prev_z=z, grad_is_dz=(i < n - 1), nz_out=nz[i], nz_in=res[i])
        return y

    def _forward_layer_norm(self, x, lim, nz, res):
        """Conv (+ bias) -> LayerNorm over channels -> GELU in every layer.  Layer 0 is one fused pass from the samples
        (cst_conv0_ln_gelu); layers 1.. are the implicit-GEMM conv with the bias in its epilogue followed by cst_ln_gelu.  The trick
        of the default mode — GELU' of layer i-1 folded into layer i's dX epilogue — does not apply: a LayerNorm sits between them.
        The frame limits carry over unchanged: no statistic crosses frames, a frame's gradient is zero where its dy is zero."""
        n = len(self.conv_spec)
        zero_bias = None

        def params(i):
            nonlocal zero_bias
            conv, ln = getattr(self.conv_layers[i], "0"), getattr(getattr(self.conv_layers[i], "2"), "1")
            bias = getattr(conv, "bias", None)
            if bias is None:
                if zero_bias is None or zero_bias.numel() != conv.weight.shape[0]:
                    zero_bias = torch.zeros(conv.weight.shape[0], dtype=conv.weight.dtype, device=conv.weight.device)
                bias = zero_bias
            return conv.weight, bias, ln.weight, ln.bias

        w, b, g, be = params(0)
        y = CF.conv0_ln_gelu(x, w, b, g, be, self.conv_spec[0][2],
                             write_limit=lim[0, 1] if lim is not None and n > 1 else None, grad_limit=nz[0])
        for i in range(1, n):
            w, b, g, be = params(i)
            # the conv bias takes its gradient from cst_ln_gelu_bwd (the column sums of du): the GEMM sees a detached copy.
            # unread_ok: rows of skipped tiles hold the bias instead of a conv output — behind nz[i] nobody reads them (ln_gelu skips them too)
            u, _ = CF.conv1d_cl(y, w, b.detach(), self.conv_spec[i][2], pad=0, act=None, nz_out=nz[i], nz_in=res[i], unread_ok=True)
            y = CF.ln_gelu(u, g, be, conv_bias=b if b.requires_grad else None, row_limit=nz[i])
        return y

    def output_length(self, s):
        for (_, k, st) in self.conv_spec:
            s = (s - k) // st + 1
        return s


class TransformerSentenceEncoderLayer(nn.Module):
    """wav2vec2.py:864-959: the post-norm branch (layer_norm_first=False, :936-957) and the pre-norm one (True, :917-934)."""

    def __init__(self, embedding_dim=768, ffn_embedding_dim=3072, num_attention_heads=8, dropout=0.1,
                 attention_dropout=0.1, activation_dropout=0.1, activation_fn="relu", layer_norm_first=False):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.dropout, self.activation_dropout = dropout, activation_dropout
        self.activation_fn = activation_fn
        self.self_attn = MultiheadAttention(embedding_dim, num_attention_heads, dropout=attention_dropout, self_attention=True)
        self.layer_norm_first = layer_norm_first
        self.self_attn_layer_norm = LayerNorm(embedding_dim)
        self.fc1 = Linear(embedding_dim, ffn_embedding_dim)
        self.fc2 = Linear(ffn_embedding_dim, embedding_dim)
        self.final_layer_norm = LayerNorm(embedding_dim)

    def forward(self, x, self_attn_mask=None, self_attn_padding_mask=None, need_weights=False, att_args=None, seq=None):
        p_drop = float(self.dropout) if self.training else 0.0             # dropout1 / dropout3 (wav2vec2.py:940-955)
        p_act = float(self.activation_dropout) if self.training else 0.0   # dropout2
        if self.layer_norm_first:
            # x = x + dropout1(attn(LN(x)));  x = x + dropout3(fc2(dropout2(act(fc1(LN(x))))))  — the residual adds and dropouts ride in
            # the out_proj / fc2 epilogues as in the post-norm branch; the LayerNorm hands its input back as the residual so both
            # gradient branches meet inside cst_layernorm_bwd (LayerNorm.forward_residual)
            h, residual = self.self_attn_layer_norm.forward_residual(x)
            x, _ = self.self_attn(query=h, key=h, value=h, key_padding_mask=self_attn_padding_mask, need_weights=False,
                                  resid=residual, out_dropout_p=p_drop, seq=seq)
            h, residual = self.final_layer_norm.forward_residual(x)
            x = to_time_major_view(CF.ffn(to_batch_major(h), self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                                          self.activation_fn, resid=to_batch_major(residual), activation_dropout_p=p_act,
                                          dropout_p=p_drop))
            return x, None
        residual = x
        x, _ = self.self_attn(query=x, key=x, value=x, key_padding_mask=self_attn_padding_mask, need_weights=False,
                              resid=residual, out_dropout_p=p_drop, seq=seq)  # x = residual + dropout1(attn) (out_proj epilogue)
        x = self.self_attn_layer_norm(x)
        residual = x
        x = to_time_major_view(CF.ffn(to_batch_major(x), self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                                      self.activation_fn, resid=to_batch_major(residual), activation_dropout_p=p_act,
                                      dropout_p=p_drop))
        x = self.final_layer_norm(x)
        return x, None


def init_bert_params(module):
    """modules/transformer_sentence_encoder.py:22-50 — normal(0, 0.02) for Linear / attention projections."""
    if isinstance(module, Linear):
        module.weight.data.normal_(mean=0.0, std=0.02)
        if module.bias is not None:
            module.bias.data.zero_()
    if isinstance(module, MultiheadAttention):
        for p in (module.q_proj, module.k_proj, module.v_proj):
            p.weight.data.normal_(mean=0.0, std=0.02)


class TransformerEncoder(nn.Module):
    """wav2vec2.py:766-861: weight-normed grouped pos_conv + SamePad + GELU, LayerNorm, N layers, layerdrop.  Post-norm stacks
    normalise in front of the layers, pre-norm ones (layer_norm_first, the large models) behind the last layer."""

    def __init__(self, args):
        super().__init__()
        self.dropout = args.dropout
        self.embedding_dim = args.encoder_embed_dim
        self.conv_pos, self.conv_pos_groups = args.conv_pos, args.conv_pos_groups
        cg = self.embedding_dim // args.conv_pos_groups
        std = math.sqrt(4 / (args.conv_pos * self.embedding_dim))
        pc = nn.Module()  # nn.utils.weight_norm(conv, name="weight", dim=2): weight_g [1,1,k], weight_v [C, C/g, k]
        v = torch.empty(self.embedding_dim, cg, args.conv_pos).normal_(0, std)
        pc.bias = nn.Parameter(torch.zeros(self.embedding_dim))
        pc.weight_g = nn.Parameter(v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
        pc.weight_v = nn.Parameter(v)
        self.pos_conv = nn.Module()
        self.pos_conv.add_module("0", pc)
        self.layers = nn.ModuleList([
            TransformerSentenceEncoderLayer(
                embedding_dim=self.embedding_dim, ffn_embedding_dim=args.encoder_ffn_embed_dim,
                num_attention_heads=args.encoder_attention_heads, dropout=self.dropout,
                attention_dropout=args.attention_dropout, activation_dropout=args.activation_dropout,
                activation_fn=args.activation_fn, layer_norm_first=args.layer_norm_first)
            for _ in range(args.encoder_layers)])
        self.layer_norm_first = args.layer_norm_first
        self.layer_norm = LayerNorm(self.embedding_dim)
        self.layerdrop = args.encoder_layerdrop
        self.apply(init_bert_params)

    def pos_conv_weight(self):
        pc = getattr(self.pos_conv, "0")
        v = pc.weight_v
        if v.is_cuda and v.shape[-1] % 8 == 0 and v.shape[-1] <= 256 and 256 % (v.shape[-1] // 8) == 0:
            return CF.weight_norm_last_dim(v, pc.weight_g)  # cst_weight_norm_fwd/bwd
        norm = v.float().pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
        return (v.float() * (pc.weight_g.float() / norm)).to(v.dtype)

    def forward(self, x, padding_mask=None, plan=None):
        x, padding_mask = self.extract_features(x, padding_mask, plan)
        return x, padding_mask

    # Padding-free layer stack.  Rows of the 12 post-norm layers are independent of each other except through attention, whose
    # keys are the real frames only.  A padding frame t >= len + conv_pos/2 of an utterance sees nothing but zeros through the
    # positional convolution (the frames were zeroed at :820-821), so ALL such frames of an utterance enter the stack with one and
    # the same vector and leave every layer with one and the same vector: the stack runs on len + conv_pos/2 + 1 rows per
    # utterance and the last row is copied to the frames behind it (functional.pack_rows / unpack_rows).  With every dropout
    # inactive this reproduces the padded computation bit for bit, padding frames included.  With dropout active the copies
    # share one mask instead of drawing their own: allowed only where nobody reads those frames (`padding_rows_consumed = False`,
    # set by the s2t_transformer_w2v2 encoder: its subsampler reads a handful of frames past the end, all inside the margin, and
    # every later layer masks the padding); the Chimera memory attends every padded frame (quirk Q1), so there the padded stack
    # stays whenever a dropout is active.
    padding_rows_consumed = True
    # how many frames past an utterance's end the consumer reads when it does not consume the padding rows (s2t encoder: the reach of
    # its Conv1dSubsampler, 6 frames for two k = 5 / stride 2 layers).  None = unknown: keep the positional convolution's reach.
    padding_rows_read = None

    def packing_margin(self):
        """Padding frames kept per utterance in front of the one representative row.  Bit-identity with the padded stack on EVERY
        frame needs the positional convolution's reach (conv_pos // 2: behind it all padding frames are one and the same vector);
        a consumer that reads only `padding_rows_read` frames past the end needs only those computed exactly — the frames behind
        them are then copies of a row nobody reads (forward bits of every frame that IS read, and every gradient, are unchanged:
        rows do not interact except through attention, whose keys are the real frames).  6 % fewer rows at the bench's lengths."""
        reach = self.conv_pos // 2
        # (CST_NO_PACK_S2T=1 — the consumer's own layer stack runs padded and then computes, and returns, its padding frames from
        #  ours: that debugging mode reproduces the reference on every frame, so it keeps the full reach)
        if not self.padding_rows_consumed and self.padding_rows_read is not None and not os.environ.get("CST_NO_PACK_S2T"):
            reach = min(reach, int(self.padding_rows_read))
        return reach

    def wants_packing(self, padding_mask):
        if padding_mask is None or os.environ.get("CST_NO_PACK"):
            return False
        noisy = self.training and (self.dropout > 0 or any(l.self_attn.dropout_module.p > 0 or l.activation_dropout > 0 for l in self.layers))
        return (not noisy) or (not self.padding_rows_consumed)

    def extract_features(self, x, padding_mask=None, plan=None):
        """x [B,T,C] batch-major."""
        if padding_mask is not None:
            x = CF.mask_rows(x, padding_mask)  # x[padding_mask] = 0 (:820-821)
        pc = getattr(self.pos_conv, "0")
        if plan is None and self.wants_packing(padding_mask):
            plan = CF.plan_packed_rows(padding_mask, self.packing_margin())
        if plan is not None and plan.rows >= plan.B * plan.T:
            plan = None  # nothing to drop (no padding beyond the margin)
        # frame limits of the positional convolution (functional.pos_conv_gelu_residual): the input is zero from each utterance's end on (the
        # lines above), so the output tiles whose windows lie in the padding skip their products — exact on every frame — and with a
        # packing plan the gradient of the output is zero behind the rows the plan keeps, which bounds the dX GEMM the same way
        lens = grad_rows = grad_rows_host = None
        if padding_mask is not None and not os.environ.get("CST_NO_POSCONV_LIMITS") and not CF.no_mlen():
            lens = plan.kv_len if plan is not None else (~padding_mask).sum(dim=1).to(torch.int32)
            if plan is not None:
                grad_rows = plan.offsets[1:] - plan.offsets[:-1]
                if plan.host_lens is not None and plan.kept_host is not None:
                    grad_rows_host = plan.kept_host
        x = CF.pos_conv_gelu_residual(x, self.pos_conv_weight(), pc.bias, self.conv_pos_groups, lens, grad_rows, grad_rows_host)  # x += GELU(SamePad(conv(x)))
        if plan is not None:
            x = CF.pack_rows(x, plan)  # [1, rows, C]
        if not self.layer_norm_first:
            x = self.layer_norm(x)  # (:827-828; a pre-norm stack normalises behind its last layer instead)
        if self.training and self.dropout > 0:
            x = CF.dropout(x, self.dropout)  # F.dropout(x, p=self.dropout) (:830)
        x = to_time_major_view(x)
        for layer in self.layers:
            dropout_probability = np.random.random()  # same RNG call order as the reference (:836-840)
            if not self.training or (dropout_probability > self.layerdrop):
                x, _ = layer(x, self_attn_padding_mask=None if plan is not None else padding_mask, need_weights=False, seq=plan)
            else:
                notify_unused_parameters(layer.parameters())  # keeps the overlapped bucket order moving (distributed.py)
        x = to_batch_major(x)
        if self.layer_norm_first:
            x = self.layer_norm(x)  # (:813-814, applied by forward() behind extract_features: a row-wise op, so before the unpacking)
        if plan is not None:
            # [B, T, C]; frames behind the kept rows repeat the last kept row — unless the consumer declared how far past an utterance's
            # end it reads and the plan keeps exactly those frames (packing_margin): then nobody reads the frames behind them, they come
            # back as zeros and the backward pass does not walk their (exactly zero) gradients to add them into the last kept row
            # (one wave per utterance summing up to a thousand rows: 4 x 52 us per update)
            unread = (not self.padding_rows_consumed and self.padding_rows_read is not None and not os.environ.get("CST_NO_PACK_S2T")
                      and not os.environ.get("CST_UNPACK_BROADCAST"))
            x = CF.unpack_rows(x, plan, broadcast=not unread)
        return x, padding_mask


@register_model("wav2vec2")
class Wav2Vec2Model(nn.Module):
    """wav2vec2.py:33-680: the feature path (features_only: fine-tuning, ST) and the pre-training forward on cropped batches."""

    @staticmethod
    def add_args(parser):
        """wav2vec2.py:36-300: the architecture and pre-training flags.  No defaults here (base_architecture fills what is absent)."""
        import argparse
        S = argparse.SUPPRESS
        for flag, typ in (("--extractor-mode", str), ("--encoder-layers", int), ("--encoder-embed-dim", int), ("--encoder-ffn-embed-dim", int),
                          ("--encoder-attention-heads", int), ("--activation-fn", str), ("--dropout", float), ("--attention-dropout", float),
                          ("--activation-dropout", float), ("--encoder-layerdrop", float), ("--dropout-input", float),
                          ("--dropout-features", float), ("--final-dim", int), ("--conv-feature-layers", str), ("--logit-temp", float),
                          ("--feature-grad-mult", float), ("--latent-vars", int), ("--latent-groups", int), ("--latent-dim", int),
                          ("--latent-temp", str), ("--mask-length", int), ("--mask-prob", float), ("--mask-selection", str),
                          ("--mask-other", float), ("--mask-min-space", int), ("--mask-channel-length", int), ("--mask-channel-prob", float),
                          ("--mask-channel-selection", str), ("--mask-channel-other", float), ("--mask-channel-min-space", int),
                          ("--num-negatives", int), ("--cross-sample-negatives", int), ("--codebook-negatives", int), ("--conv-pos", int),
                          ("--conv-pos-groups", int)):
            parser.add_argument(flag, type=typ, default=S)
        for flag in ("--layer-norm-first", "--quantize-targets", "--quantize-input", "--same-quantizer", "--target-glu", "--conv-bias",
                     "--no-mask-overlap", "--no-mask-channel-overlap", "--negatives-from-everywhere"):
            parser.add_argument(flag, action="store_true", default=S)

    def __init__(self, args, pretraining_heads=True):
        """pretraining_heads=False: built as the reference leaves the model after remove_pretraining_modules() (wav2vec2.py:678-682) —
        no quantizer / project_q / target_glu / final_proj, the key set of `w2v_encoder.w2v_model.*` in a wav2vec_ctc checkpoint."""
        super().__init__()
        self.args = args
        feature_enc_layers = eval(args.conv_feature_layers)
        self.embed = feature_enc_layers[-1][0]
        self.feature_extractor = ConvFeatureExtractionModel(conv_layers=feature_enc_layers, dropout=0.0,
                                                            mode=args.extractor_mode, conv_bias=args.conv_bias)
        self.post_extract_proj = (Linear(self.embed, args.encoder_embed_dim)
                                  if self.embed != args.encoder_embed_dim and not args.quantize_input else None)
        self.feature_grad_mult = args.feature_grad_mult
        self.dropout_input_p = getattr(args, "dropout_input", 0)
        self.dropout_features_p = getattr(args, "dropout_features", 0)
        self.logit_temp = getattr(args, "logit_temp", 0.1)
        self.n_negatives = getattr(args, "num_negatives", 100)
        self.cross_sample_negatives = getattr(args, "cross_sample_negatives", 0)
        # variants of the pre-training head that are in no published recipe: refused by name, here, not in the middle of an update
        if getattr(args, "negatives_from_everywhere", False):
            raise NotImplementedError("--negatives-from-everywhere (negatives sampled from unmasked frames too) is not built")
        if getattr(args, "codebook_negatives", 0) > 0:
            raise NotImplementedError("--codebook-negatives > 0 (negatives drawn from the codebook) is not built")
        if getattr(args, "target_glu", False) and pretraining_heads and getattr(args, "criterion", None) == "wav2vec":
            raise NotImplementedError("--target-glu (a GLU over the targets and negatives) is not built for pre-training")
        final_dim = args.final_dim if args.final_dim > 0 else args.encoder_embed_dim
        # registration ORDER follows wav2vec2.py:306-420 (post_extract_proj, quantizer, project_q, [input_quantizer, project_inp],
        # mask_emb, encoder, layer_norm, [target_glu], final_proj): model.parameters() order is the index space of the
        # reference's optimizer state and state_dict() its key set (checkpoint interop).  The pre-training heads
        # (quantizer, project_q, final_proj, ...) are never on the ST path; they are instantiated as inert parameters with the
        # reference's shapes so that real checkpoints (wav2vec_small: quantize_targets=True) load with strict=True through
        # ANY enclosing module, are re-emitted by state_dict(), and keep every later optimizer-state index where the
        # reference has it.
        self.quantizer = self.input_quantizer = self.project_inp = self.target_glu = None
        if getattr(args, "quantize_targets", False):
            vq_dim = args.latent_dim if getattr(args, "latent_dim", 0) > 0 else final_dim
            self.quantizer = GumbelVectorQuantizer(self.embed, args.latent_vars, args.latent_groups, vq_dim, _latent_temp(args))
            self.project_q = Linear(vq_dim, final_dim)
        else:
            self.project_q = Linear(self.embed, final_dim)
        if getattr(args, "quantize_input", False):
            if getattr(args, "same_quantizer", False) and self.quantizer is not None:
                vq_dim = final_dim
                self.input_quantizer = self.quantizer
            else:
                vq_dim = args.latent_dim if getattr(args, "latent_dim", 0) > 0 else args.encoder_embed_dim
                self.input_quantizer = GumbelVectorQuantizer(self.embed, args.latent_vars, args.latent_groups, vq_dim, _latent_temp(args))
            self.project_inp = Linear(vq_dim, args.encoder_embed_dim)
            raise NotImplementedError("--quantize-input (the quantised features feed the encoder) is not built, for pre-training or the ST path")
        self.mask_emb = nn.Parameter(torch.FloatTensor(args.encoder_embed_dim).uniform_())
        self.encoder = TransformerEncoder(args)
        self.layer_norm = LayerNorm(self.embed)
        if getattr(args, "target_glu", False):
            self.target_glu = nn.Sequential(Linear(final_dim, final_dim * 2), nn.GLU())
        self.final_proj = Linear(args.encoder_embed_dim, final_dim)
        # fine-tuning's time / channel masking (wav2vec2.py:341-353); read with the reference's defaults so that no Namespace grows
        self.mask_prob, self.mask_length = getattr(args, "mask_prob", 0.65), getattr(args, "mask_length", 10)
        self.mask_selection, self.mask_other = getattr(args, "mask_selection", "static"), getattr(args, "mask_other", 0)
        self.no_mask_overlap, self.mask_min_space = getattr(args, "no_mask_overlap", False), getattr(args, "mask_min_space", 1)
        self.mask_channel_prob, self.mask_channel_length = getattr(args, "mask_channel_prob", 0), getattr(args, "mask_channel_length", 10)
        self.mask_channel_selection = getattr(args, "mask_channel_selection", "static")
        self.mask_channel_other = getattr(args, "mask_channel_other", 0)
        self.no_mask_channel_overlap = getattr(args, "no_mask_channel_overlap", False)
        self.mask_channel_min_space = getattr(args, "mask_channel_min_space", 1)
        if not pretraining_heads:
            self.remove_pretraining_modules()

    def remove_pretraining_modules(self):
        """wav2vec2.py:678-682."""
        self.quantizer = self.project_q = self.target_glu = self.final_proj = None

    def draw_masks_host(self, B, T, host_lens):
        """The draws of apply_mask (wav2vec2.py:414-452) from numpy's global generator, in its order: the time mask [B, T] over each
        utterance's real frames (host_lens: host integers, None without a padding mask), then the channel mask [B, C] — numpy bool
        arrays on the host (None where the probability is 0)."""
        tmask = cmask = None
        if self.mask_prob > 0:
            tmask = compute_mask_indices((B, T), host_lens, self.mask_prob, self.mask_length, self.mask_selection, self.mask_other,
                                         min_masks=2, no_overlap=self.no_mask_overlap, min_space=self.mask_min_space)
        if self.mask_channel_prob > 0:
            cmask = compute_mask_indices((B, self.mask_emb.numel()), None, self.mask_channel_prob, self.mask_channel_length,
                                         self.mask_channel_selection, self.mask_channel_other, no_overlap=self.no_mask_channel_overlap,
                                         min_space=self.mask_channel_min_space)
        return tmask, cmask

    def draw_masks(self, B, T, host_lens):
        """draw_masks_host as device bool tensors; nothing here waits for the device."""
        dev = self.mask_emb.device
        return tuple(None if m is None else torch.from_numpy(m).to(dev, non_blocking=True) for m in self.draw_masks_host(B, T, host_lens))

    def apply_mask(self, x, tmask, cmask):
        """x[tmask] = mask_emb; x[:, :, cmask] = 0 (wav2vec2.py:429, :450) as where-compositions: a boolean index_put would wait for
        the device.  Autograd gives mask_emb the sum of the incoming gradient over the masked frames (channel-masked columns excluded)
        and passes nothing back through a masked position."""
        if tmask is not None:
            x = torch.where(tmask.unsqueeze(-1), self.mask_emb.to(x.dtype), x)
        if cmask is not None:
            x = x.masked_fill(cmask.unsqueeze(1), 0.0)
        return x

    @classmethod
    def build_model(cls, args, task=None):
        base_architecture(args)
        return cls(args)

    def set_num_updates(self, num_updates):
        """The quantizers' Gumbel temperature follows the update count (the reference's walk over the children, fairseq_model.py)."""
        for m in (self.quantizer, self.input_quantizer):
            if m is not None:
                m.set_num_updates(num_updates)

    def forward(self, source, padding_mask=None, mask=True, features_only=False, mask_indices=None, neg_idxs=None, noise=None):
        """features_only: the feature path (fine-tuning, ST).  Otherwise the pre-training forward (wav2vec2.py:527-641), see
        forward_pretrain; mask_indices / neg_idxs / noise replay recorded draws (tests, fixtures)."""
        if not features_only:
            return self.forward_pretrain(source, padding_mask, mask_indices, neg_idxs, noise)
        if mask_indices is not None or neg_idxs is not None or noise is not None:
            raise ValueError("mask_indices / neg_idxs / noise replay the draws of the pre-training forward; the feature path takes none")
        if self.training:
            # pre-training-only parameters never receive a gradient on this path: without this the gradient bucket that holds
            # final_proj (the FIRST wav2vec2 bucket in backward order) would wait for finish() and un-overlap every later one
            heads = [] if (mask and self.mask_prob > 0) else [self.mask_emb]
            for m in (self.final_proj, self.project_q, self.quantizer, self.target_glu):
                if m is not None:
                    heads += list(m.parameters())
            notify_unused_parameters(heads)
        # the frame-level padding mask of :543-548 is a function of the sample-level one and the CNN's output length: computed ONCE,
        # before the CNN is queued (it serves the packing plan, the conv frame limits and the encoder's key mask)
        frame_mask, plan, nz_last = None, None, None
        if padding_mask is not None:
            t1 = self.feature_extractor.output_length(source.shape[1])
            pm = padding_mask
            extra = pm.size(1) % t1
            if extra > 0:
                pm = pm[:, :-extra]
            frame_mask = pm.view(pm.size(0), t1, -1).all(-1)
            if self.encoder.wants_packing(padding_mask):
                # the packing plan needs a few integers on the host (rows in total, longest sequence, lengths): read them HERE — the
                # stream is empty at this point of an update, later the read would drain 20 ms of queued convolutions
                plan = CF.plan_packed_rows(frame_mask, self.encoder.packing_margin())
            # frames past the last real one get a zero gradient (they are overwritten with zeros at the encoder input), which bounds
            # every conv layer's weight-gradient reduction and the frames the CNN has to compute at all
            pos = torch.arange(1, t1 + 1, device=frame_mask.device, dtype=torch.int32)
            nz_last = (pos * (~frame_mask)).amax(dim=1).to(torch.int32)
        masks = None
        if mask:
            # fine-tuning's masks are drawn HERE, on host integers, before anything is queued: the per-utterance frame counts are the
            # packing plan's host lengths (the reference reads them with an .item() per row in the middle of the forward pass)
            host_lens = None
            if padding_mask is not None:
                host_lens = plan.host_lens if plan is not None else (~frame_mask).sum(dim=1).tolist()
            masks = self.draw_masks(source.shape[0], self.feature_extractor.output_length(source.shape[1]), host_lens)
        self.last_plan = plan  # (the caller's own layer stack derives its packing plan from this one's host lengths)
        feats = self.feature_extractor(source, nz_last)  # [B, T1, C] channels-last
        if self.feature_grad_mult <= 0:
            feats = feats.detach()
        elif self.feature_grad_mult != 1.0:
            feats = _GradMultiply.apply(feats, self.feature_grad_mult)
        feats = self.layer_norm(feats)  # transpose(1,2) is free in channels-last (:539-540)
        if padding_mask is not None:
            assert feats.size(1) == frame_mask.size(1)
            padding_mask = frame_mask
        if self.post_extract_proj is not None:
            feats = self.post_extract_proj(feats)
        if self.training and self.dropout_input_p > 0:
            feats = CF.dropout(feats, self.dropout_input_p)  # self.dropout_input (:553)
        if masks is not None:
            feats = self.apply_mask(feats, *masks)  # (:561-562)
        x, padding_mask = self.encoder(feats, padding_mask=padding_mask, plan=plan)
        return {"x": x, "padding_mask": padding_mask}

    def extract_features(self, source, padding_mask, mask=False):
        res = self.forward(source, padding_mask, mask=mask, features_only=True)
        return res["x"], res["padding_mask"]

    def forward_pretrain(self, source, padding_mask=None, mask_indices=None, neg_idxs=None, noise=None):
        """wav2vec2.py:527-641 on cropped batches (no padding mask).  The masked positions are known on the host (the masks are drawn
        there, the same number per utterance), so x and y are gathered by index without a device read.  Returns the operands of the
        fused contrastive loss instead of logits — x = final_proj(encoder output) and y = project_q(quantised targets) at the masked
        positions, both [B, M, final_dim], and neg_idx int32 [B * M, K'] — plus features_pen, and with a quantizer num_vars /
        code_perplexity / prob_perplexity / temp.  get_logits builds the reference's [B * M, K' + 1] logits from them on request."""
        if padding_mask is not None:
            raise NotImplementedError("wav2vec2 pre-training on padded batches (--enable-padding) is not built: batches are cropped")
        if self.final_proj is None or self.project_q is None:
            raise RuntimeError("this wav2vec2 model was built without its pre-training heads")
        B, T = source.shape[0], self.feature_extractor.output_length(source.shape[1])
        dev = source.device
        cmask = None
        if mask_indices is None:
            assert self.mask_prob > 0, "pre-training needs --mask-prob > 0"
            host, cmask = self.draw_masks_host(B, T, None)
            tmask = torch.from_numpy(host).to(dev, non_blocking=True)
            cmask = None if cmask is None else torch.from_numpy(cmask).to(dev, non_blocking=True)
        else:
            host = np.asarray(mask_indices.cpu() if torch.is_tensor(mask_indices) else mask_indices, dtype=bool)
            tmask = torch.from_numpy(host).to(dev, non_blocking=True)
        per_row = host.sum(1)
        M = int(per_row[0])
        assert (per_row == M).all() and M > 0, "the time masks must cover the same number of frames in every utterance"
        pos = torch.from_numpy(np.flatnonzero(host.reshape(-1))).to(dev, non_blocking=True)
        self.last_plan = None
        feats = self.feature_extractor(source, None)
        if self.feature_grad_mult <= 0:
            feats = feats.detach()
        elif self.feature_grad_mult != 1.0:
            feats = _GradMultiply.apply(feats, self.feature_grad_mult)
        features_pen = CF.mean_square(feats)  # (:537, on the CNN's output)
        feats = self.layer_norm(feats)
        unmasked = feats
        if self.post_extract_proj is not None:
            feats = self.post_extract_proj(feats)
        if self.training and self.dropout_input_p > 0:
            feats = CF.dropout(feats, self.dropout_input_p)
        if self.training and self.dropout_features_p > 0:
            unmasked = CF.dropout(unmasked, self.dropout_features_p)
        x = self.apply_mask(feats, tmask, cmask)
        y = unmasked.reshape(B * T, -1).index_select(0, pos)
        x, _ = self.encoder(x, padding_mask=None, plan=None)
        x = x.reshape(B * T, -1).index_select(0, pos)
        result = {"padding_mask": None, "features_pen": features_pen, "mask_indices": tmask}
        if self.quantizer is not None:
            q = self.quantizer(y.view(B, M, -1), produce_targets=True, noise=noise)
            y = q["x"].reshape(B * M, -1)
            result.update(num_vars=q["num_vars"], code_perplexity=q["code_perplexity"], prob_perplexity=q["prob_perplexity"], temp=q["temp"],
                          quantizer_targets=q["targets"])
        y = self.project_q(y)
        x = self.final_proj(x)
        if neg_idxs is None:
            neg_idxs = CF.sample_negatives(B, M, self.n_negatives, self.cross_sample_negatives, device=dev)
        else:
            neg_idxs = torch.as_tensor(neg_idxs).to(dev).to(torch.int32).reshape(B * M, -1)
        result.update(x=x.view(B, M, -1), y=y.view(B, M, -1), neg_idx=neg_idxs)
        return result

    def get_logits(self, net_output):
        """The reference's logits [B * M, K' + 1] (positive first, -inf where a negative equals it) in fp32: built on request only —
        the training path (criterion wav2vec) goes through functional.infonce_loss and never has them."""
        x, y = net_output["x"], net_output["y"]
        D = x.shape[-1]
        return K.infonce_fwd(x.reshape(-1, D).detach(), y.reshape(-1, D).detach(), net_output["neg_idx"], 1.0 / self.logit_temp,
                             want_logits=True)[4]

    def get_targets(self, sample, net_output, expand_steps=True):
        x = net_output["x"]
        return x.new_zeros(x.shape[0] * x.shape[1], dtype=torch.long)

    def get_extra_losses(self, net_output):
        """(:665-676) the diversity loss where there is a quantizer, then the feature penalty."""
        pen = []
        if "prob_perplexity" in net_output:
            pen.append((net_output["num_vars"] - net_output["prob_perplexity"]) / net_output["num_vars"])
        if "features_pen" in net_output:
            pen.append(net_output["features_pen"])
        return pen


def compute_mask_indices(shape, lengths, mask_prob, mask_length, mask_type="static", mask_other=0.0, min_masks=0, no_overlap=False,
                         min_space=0):
    """Span masks [bsz, all_sz] (numpy bool) with the draws of data/data_utils.py:354-478 from numpy's GLOBAL generator, in the same
    order, so that a seed reproduces the reference's masks.  `lengths`: the real elements per row as host integers where the reference
    is given a padding mask (it then draws one rounding number per row), None where it is given none."""
    bsz, all_sz = shape
    mask = np.zeros((bsz, all_sz), dtype=bool)
    all_num_mask = max(min_masks, int(mask_prob * all_sz / float(mask_length) + np.random.rand()))
    rows = []
    for i in range(bsz):
        if lengths is not None:
            sz = int(lengths[i])
            num_mask = max(min_masks, int(mask_prob * sz / float(mask_length) + np.random.rand()))
        else:
            sz, num_mask = all_sz, all_num_mask
        if mask_type == "static":
            spans = np.full(num_mask, mask_length)
        elif mask_type == "uniform":
            spans = np.random.randint(mask_other, mask_length * 2 + 1, size=num_mask)
        elif mask_type == "normal":
            spans = [max(1, int(round(v))) for v in np.random.normal(mask_length, mask_other, size=num_mask)]
        elif mask_type == "poisson":
            spans = [int(round(v)) for v in np.random.poisson(mask_length, size=num_mask)]
        else:
            raise ValueError("unknown mask selection " + mask_type)
        if sum(spans) == 0:
            spans[0] = min(mask_length, sz - 1)
        if no_overlap:
            idc = []
            parts = [(0, sz)]
            shortest = min(spans)
            for span in sorted(spans, reverse=True):
                room = np.array([e - s if e - s >= span + min_space else 0 for s, e in parts], dtype=np.int64)
                if room.sum() == 0:
                    break
                s, e = parts.pop(np.random.choice(len(parts), p=room / room.sum()))
                start = np.random.randint(s, e - span)
                idc.extend(range(start, start + span))
                if start - s - min_space >= shortest:
                    parts.append((s, start - min_space + 1))
                if e - start - shortest - min_space > shortest:
                    parts.append((start + span + min_space, e))
            idc = np.asarray(idc, dtype=np.int64)
        else:
            shortest = min(spans)
            if sz - shortest <= num_mask:
                shortest = sz - num_mask - 1
            starts = np.random.choice(sz - shortest, num_mask, replace=False)
            idc = np.asarray([starts[j] + o for j in range(len(starts)) for o in range(spans[j])], dtype=np.int64)
        rows.append(np.unique(idc[idc < sz]))
    keep = min(len(r) for r in rows)
    for i, r in enumerate(rows):
        if len(r) > keep:
            r = np.random.choice(r, keep, replace=False)
        mask[i, r] = True
    return mask


class GumbelVectorQuantizer(nn.Module):
    """modules/gumbel_vector_quantizer.py (combine_groups=False, weight_proj_depth=1, time_first): `vars` [1, groups * num_vars,
    vq_dim / groups] and `weight_proj` Linear(dim, groups * num_vars) — the reference's names, shapes, init and registration order, so
    its checkpoints load strictly.  forward: the projection is this library's GEMM, everything after it ONE fused call
    (functional.gumbel_vector_quantize over csrc/w2v_pretrain.hip): the hard choice of l + Gumbel noise (training) or of l (eval), the
    codebook rows, both perplexities, and in backward the straight-through and diversity gradients.  The noise comes from the
    dropout counter hash (one site key per call), `noise` (fp32 [B * T, groups, num_vars]) replaces it where a recorded draw is replayed.
    Pre-training only: nothing on the ST or CTC paths calls it."""

    def __init__(self, dim, num_vars, groups, vq_dim, temp=(2.0, 0.5, 0.999995)):
        super().__init__()
        assert vq_dim % groups == 0
        self.groups, self.num_vars, self.input_dim = groups, num_vars, dim
        self.vars = nn.Parameter(torch.FloatTensor(1, groups * num_vars, vq_dim // groups).uniform_())
        self.weight_proj = nn.Linear(dim, groups * num_vars)
        nn.init.normal_(self.weight_proj.weight, mean=0, std=1)
        nn.init.zeros_(self.weight_proj.bias)
        assert len(temp) == 3, temp
        self.max_temp, self.min_temp, self.temp_decay = (float(t) for t in temp)
        self.curr_temp = self.max_temp

    def set_num_updates(self, num_updates):
        self.curr_temp = max(self.max_temp * self.temp_decay ** num_updates, self.min_temp)

    def forward(self, x, produce_targets=False, noise=None):
        """x [B, T, dim] -> dict(x = the quantised features [B, T, vq_dim], num_vars, code_perplexity, prob_perplexity (device scalars;
        prob_perplexity carries the diversity gradient), temp, and under produce_targets `targets` int64 [B, T, groups])."""
        B, T, C = x.shape
        logits = CF.linear(x.reshape(B * T, C), self.weight_proj.weight, self.weight_proj.bias)
        q, ppl, cpl, idx, _ = CF.gumbel_vector_quantize(logits, self.vars.view(self.groups * self.num_vars, -1), self.groups, self.curr_temp,
                                                        training=self.training, noise=noise)
        result = {"num_vars": self.num_vars * self.groups, "code_perplexity": cpl, "prob_perplexity": ppl, "temp": self.curr_temp,
                  "x": q.view(B, T, -1)}
        if produce_targets:
            result["targets"] = idx.view(B, T, self.groups).long()
        return result

    def forward_idx(self, x):
        res = self.forward(x, produce_targets=True)
        return res["x"], res["targets"]

    def quantize(self, x):
        """The quantised features alone (the hard choice's codebook rows)."""
        return self.forward(x)["x"]


def _latent_temp(args):
    """--latent-temp '(start, stop, decay)' as the reference passes it around: a string or a tuple."""
    t = getattr(args, "latent_temp", None) or (2.0, 0.5, 0.999995)
    if isinstance(t, str):
        import ast
        t = ast.literal_eval(t)
    return tuple(t)


class _GradMultiply(torch.autograd.Function):
    """modules/grad_multiply.py."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return grad * ctx.scale, None


@register_model_architecture("wav2vec2", "wav2vec2")
def base_architecture(args):
    """wav2vec2.py:962-1029 defaults (only the ones the feature path reads, plus checkpoint-visible ones)."""
    d = dict(
        extractor_mode="default", encoder_layers=12, encoder_embed_dim=768, encoder_ffn_embed_dim=3072,
        encoder_attention_heads=12, activation_fn="gelu", dropout=0.1, attention_dropout=0.1, activation_dropout=0.0,
        final_dim=0, layer_norm_first=False, encoder_layerdrop=0.0,
        conv_feature_layers="[(512, 10, 5)] + [(512, 8, 4)] + [(512, 4, 2)] * 3 + [(512, 1, 1)]",
        logit_temp=0.1, quantize_targets=False, quantize_input=False, same_quantizer=False, feature_grad_mult=1.0,
        latent_vars=320, latent_groups=2, latent_dim=0, dropout_input=0, dropout_features=0, conv_pos=128,
        conv_pos_groups=16, conv_bias=False, target_glu=False,
        num_negatives=100, cross_sample_negatives=0, codebook_negatives=0, negatives_from_everywhere=False,
        latent_temp="(2,0.5,0.999995)", mask_length=10, mask_prob=0.65, mask_selection="static", mask_other=0, no_mask_overlap=False,
        mask_min_space=1, mask_channel_length=10, mask_channel_prob=0, mask_channel_selection="static", mask_channel_other=0,
        no_mask_channel_overlap=False, mask_channel_min_space=1,
    )
    for k, v in d.items():
        if not hasattr(args, k):
            setattr(args, k, v)


def wav2vec_small_args(**over):
    """The published wav2vec_small.pt hyper-parameters (SURVEY §8 caveat): 7-layer stride-320 CNN, 12x768 encoder,
    feature_grad_mult 0.1, layerdrop 0.05."""
    ns = Namespace(
        conv_feature_layers="[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2", encoder_layers=12, encoder_embed_dim=768,
        encoder_ffn_embed_dim=3072, encoder_attention_heads=12, activation_fn="gelu", dropout=0.1, attention_dropout=0.1,
        activation_dropout=0.0, encoder_layerdrop=0.05, feature_grad_mult=0.1, final_dim=256, quantize_targets=True,
        conv_pos=128, conv_pos_groups=16, layer_norm_first=False, extractor_mode="default", conv_bias=False,
        dropout_input=0.1, dropout_features=0.1)
    for k, v in over.items():
        setattr(ns, k, v)
    base_architecture(ns)
    return ns
