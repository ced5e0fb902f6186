"""Encoders with the reference's names and forward signatures (reference: modules/module_cross.py:47-108
CrossConfig, :110-149 temporal blocks, :152-237 VisualEncoder, :240-305 TextEncoder, :308-357 MLM head)."""
from __future__ import annotations

import copy
import json
import logging
import math
import os
from collections import OrderedDict

import torch
from torch import nn

from . import functional as Fn
from . import ops
from .module_clip import CLIP, build_model, build_visual
from .until_module import LayerNorm

logger = logging.getLogger(__name__)

CONFIG_NAME = "cross_config.json"


class CrossConfig(object):
    """Holds cross-base/cross_config.json (reference modules/module_cross.py:47-108, until_config.py:41-99)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @classmethod
    def from_json_file(cls, path):
        with open(path, "r", encoding="utf-8") as fh:
            return cls(**json.load(fh))

    @classmethod
    def get_config(cls, pretrained_model_name, cache_dir=None, type_vocab_size=2, state_dict=None, task_config=None):
        here = os.path.dirname(os.path.abspath(__file__))
        cand = os.path.join(here, pretrained_model_name)
        path = cand if os.path.exists(cand) else pretrained_model_name
        cfg_file = os.path.join(path, CONFIG_NAME) if os.path.isdir(path) else path
        if not os.path.exists(cfg_file):
            if task_config is None or getattr(task_config, "local_rank", 0) == 0:
                logger.error("Model name '%s' was not found (looked for %s)", pretrained_model_name, cfg_file)
            return None
        config = cls.from_json_file(cfg_file)
        config.type_vocab_size = type_vocab_size
        return config, state_dict

    def to_dict(self):
        return copy.deepcopy(self.__dict__)

    def __repr__(self):
        return json.dumps(self.to_dict(), indent=2, sort_keys=True)


class QuickGELU(nn.Module):
    def forward(self, x):
        raise RuntimeError("QuickGELU is fused into hmmc_gemm_f32's epilogue; call the enclosing Transformer")


class ResidualAttentionBlock(nn.Module):
    """fp32 temporal block container, TF-style LN eps 1e-12 (reference modules/module_cross.py:114-139)."""

    def __init__(self, d_model, n_head):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.n_head = n_head


class Transformer(nn.Module):
    """Temporal transformer container (reference modules/module_cross.py:141-149); executed inside
    functional.TemporalFn together with the position add, the residual and the pooling."""

    def __init__(self, width, layers, heads):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads) for _ in range(layers)])

    def flat_params(self):
        out = []
        for blk in self.resblocks:
            out += Fn.block_params(blk)
        return out


def _clip_for(task_config, cross_config):
    name = getattr(task_config, "pretrained_clip_name", None) or cross_config.pretrained_clip_name
    sd = getattr(cross_config, "_clip_state_dict", None)
    if sd is None:
        sd = CLIP.get_config(pretrained_clip_name=name)
    return sd, build_model(sd, local_rank=getattr(task_config, "local_rank", 0))


class VisualEncoder(nn.Module):
    """video [b,F,3,H,W] -> (video_emb [b,512], frame_output [b,F,512]) fp32
    (reference modules/module_cross.py:152-237)."""

    def __init__(self, task_config, cross_config):
        super().__init__()
        self.use_temp = task_config.use_temp
        self.is_vit = True
        sd = getattr(cross_config, "_clip_state_dict", None)
        if sd is not None and "token_embedding.weight" not in sd:
            self.visual = build_visual(sd)          # a checkpoint of the Chinese branch: it holds no CLIP text tower
        else:
            _, clip = _clip_for(task_config, cross_config)
            self.visual = copy.deepcopy(clip.visual)
        if self.use_temp:
            self.temporal_transformer = Transformer(width=cross_config.temporal_hidden_size,
                                                    layers=cross_config.temporal_hidden_layers,
                                                    heads=cross_config.temporal_attention_heads)
            self.frame_position_embeddings = nn.Embedding(cross_config.max_position_embeddings,
                                                          cross_config.temporal_hidden_size)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def forward(self, video, video_frames=None, frame_index=None):
        """frame_index (int32 [bs, frames] from hmmc_amd.sampling.batch_frame_index): `video` then holds every STORED frame,
        uint8 [bs, stored, 3, H, W], and the sampled ones are read in place by the patch kernel."""
        bs, frames, channel, h, w = video.shape
        video = video.reshape(bs * frames, channel, h, w)
        if frame_index is not None:
            frames = frame_index.shape[1]
            frame_index = frame_index.reshape(-1).contiguous()
        frame_output = self.encode_image(video, video_frame=frames, frame_index=frame_index).view(bs, frames, -1)
        if self.use_temp:
            if frames > self.frame_position_embeddings.weight.shape[0]:
                raise ValueError("more frames than max_position_embeddings")
            visual_output = Fn.temporal(frame_output, self.temporal_transformer.heads,
                                                self.frame_position_embeddings.weight,
                                                *self.temporal_transformer.flat_params())
        else:
            visual_output = Fn.temporal(frame_output, 0, None)
        return visual_output, frame_output

    def encode_image(self, image, return_hidden=False, video_frame=-1, frame_index=None):
        """ln_post(hidden) @ proj, CLS row, .float() (reference modules/module_cross.py:222-237).  Only the CLS
        rows are normalised and projected unless return_hidden asks for all tokens."""
        n = image.shape[0] if frame_index is None else frame_index.numel()
        L = self.visual.tokens
        # without return_hidden only the class-token row of the last block is consumed: its per-token half runs on that row alone
        tokens = self.visual.hidden_tokens(image, lead_only=not return_hidden, frame_index=frame_index)
        v = self.visual
        if return_hidden:
            hidden = Fn.LnProjFn.apply(tokens, None, v.ln_post.weight, v.ln_post.bias, v.proj).view(n, L, -1)
            return hidden[:, 0, :], hidden
        idx = torch.arange(n, device=tokens.device, dtype=torch.int32) * L
        # the fp16 tower ran lead_only: its backward reads the gradient of `tokens` at the class rows alone
        return Fn.LnProjFn.apply(tokens, idx, v.ln_post.weight, v.ln_post.bias, v.proj, tokens.dtype == torch.float16)


class _Holder(nn.Module):
    """Parameter container: a node of the HuggingFace BertModel's module tree (names only; nothing runs here)."""


class BertLayerParams(nn.Module):
    """encoder.layer.N of a HuggingFace BertModel: parameters under the reference's names."""

    def __init__(self, width, inter):
        super().__init__()
        self.attention = _Holder()
        self.attention.self = _Holder()
        for n in ("query", "key", "value"):
            setattr(self.attention.self, n, nn.Linear(width, width))
        self.attention.output = _Holder()
        self.attention.output.dense = nn.Linear(width, width)
        self.attention.output.LayerNorm = nn.LayerNorm(width)
        self.intermediate = _Holder()
        self.intermediate.dense = nn.Linear(width, inter)
        self.output = _Holder()
        self.output.dense = nn.Linear(inter, width)
        self.output.LayerNorm = nn.LayerNorm(width)

    def flat_params(self):
        a, o = self.attention, self.output
        mods = (a.self.query, a.self.key, a.self.value, a.output.dense, a.output.LayerNorm, self.intermediate.dense, o.dense,
                o.LayerNorm)
        return [t for m in mods for t in (m.weight, m.bias)]


class ChineseBert(nn.Module):
    """Parameter container with the state_dict of the HuggingFace BertModel the reference loads with AutoModel.from_pretrained
    (modules/module_cross.py:257-265); executed by functional.BertFn (hmmc_bert_fwd / hmmc_bert_bwd).  `config` is the
    dict of <pretrained_text>/config.json."""

    def __init__(self, config):
        super().__init__()
        w, inter = config["hidden_size"], config["intermediate_size"]
        self.embeddings = _Holder()
        self.embeddings.word_embeddings = nn.Embedding(config["vocab_size"], w)
        self.embeddings.position_embeddings = nn.Embedding(config["max_position_embeddings"], w)
        self.embeddings.token_type_embeddings = nn.Embedding(config.get("type_vocab_size", 2), w)
        self.embeddings.LayerNorm = nn.LayerNorm(w)
        self.encoder = _Holder()
        self.encoder.layer = nn.ModuleList([BertLayerParams(w, inter) for _ in range(config["num_hidden_layers"])])
        self.pooler = _Holder()
        self.pooler.dense = nn.Linear(w, w)

    def flat_params(self):
        e = self.embeddings
        out = [e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight, e.LayerNorm.weight,
               e.LayerNorm.bias]
        for layer in self.encoder.layer:
            out += layer.flat_params()
        return out


def _bert_config(path):
    """<pretrained_text>/config.json, checked against what the HIP tower implements."""
    cfg_file = os.path.join(path, "config.json") if path and os.path.isdir(path) else path
    if not cfg_file or not os.path.exists(cfg_file):
        raise FileNotFoundError(f"task_config.pretrained_text: no config.json of the Chinese BERT encoder at {path!r}")
    with open(cfg_file, "r", encoding="utf-8") as fh:
        cfg = json.load(fh)
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError(f"position_embedding_type {cfg['position_embedding_type']!r}: only absolute positions are implemented")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"hidden_act {cfg['hidden_act']!r}: only the erf-GELU (\"gelu\") is implemented")
    if cfg["hidden_size"] != 64 * cfg["num_attention_heads"]:
        raise NotImplementedError("the attention kernels take a head dimension of 64 "
                                  f"(hidden_size {cfg['hidden_size']}, {cfg['num_attention_heads']} heads)")
    return cfg


def bert_tokenizer_constants(path):
    """<pretrained_text>/vocab.txt as BertTokenizer indexes it (one token per line, id = line number, the trailing newline
    stripped) -> {"vocab_size", "pad_id", "cls_id", "mask_id"}: what the pre-training model takes from its tokenizer
    (reference modules/modeling.py:104-120,164,185-194).  The size is checked against the word-embedding table of config.json."""
    vocab_file = os.path.join(path, "vocab.txt") if path and os.path.isdir(path) else None
    if not vocab_file or not os.path.exists(vocab_file):
        raise NotImplementedError("pre-training with language = \"chinese\" takes the BertTokenizer vocabulary (its size and the "
                                  f"[MASK] / [PAD] / [CLS] ids) from <pretrained_text>/vocab.txt: no such file at {path!r}")
    with open(vocab_file, "r", encoding="utf-8") as fh:
        tokens = [line.rstrip("\n") for line in fh.readlines()]
    index = {tok: i for i, tok in enumerate(tokens)}
    out = {"vocab_size": len(tokens)}
    for key, tok in (("pad_id", "[PAD]"), ("cls_id", "[CLS]"), ("mask_id", "[MASK]")):
        if tok not in index:
            raise ValueError(f"{vocab_file}: the special token {tok} is missing")
        out[key] = index[tok]
    embedding_rows = _bert_config(path)["vocab_size"]
    if out["vocab_size"] > embedding_rows:
        raise ValueError(f"{vocab_file}: vocab_size {out['vocab_size']} is larger than the encoder's word-embedding table "
                         f"({embedding_rows} rows)")
    return out


def _bert_linears(text_encoder):
    """(name, module) of every nn.Linear of the Chinese branch: all of chinese_encoder.* and text_proj."""
    out = [("chinese_encoder." + n, m) for n, m in text_encoder.chinese_encoder.named_modules() if isinstance(m, nn.Linear)]
    return out + [("text_proj", text_encoder.text_proj)]


def convert_bert_weights(text_encoder):
    """Select the fp16 regime of the Chinese text encoder (csrc/bert_f16.hip), as clip.convert_weights selects the fp16 CLIP
    towers: weight AND bias of every nn.Linear under chinese_encoder.* and of text_proj become fp16; the three embedding
    tables and every LayerNorm weight / bias stay fp32.  In place; returns the encoder."""
    if getattr(text_encoder, "language", None) != "chinese":
        raise ValueError("convert_bert_weights takes a TextEncoder with language = \"chinese\"")
    for _, m in _bert_linears(text_encoder):
        m.weight.data = m.weight.data.half()
        m.bias.data = m.bias.data.half()
    return text_encoder


def bert_regime(text_encoder):
    """torch.float32 for the untouched layout, torch.float16 for exactly the layout convert_bert_weights produces.  Any other
    mix of dtypes (a plain .half(), which also halves LayerNorms and embeddings; one Linear left behind) raises a TypeError
    that names convert_bert_weights.  The decision is functional.bert_layout_regime's, the one every tower call makes."""
    enc = text_encoder.chinese_encoder
    return Fn.bert_layout_regime(enc.pooler.dense.weight, enc.pooler.dense.bias, text_encoder.text_proj.weight,
                                 text_encoder.text_proj.bias, enc.flat_params())


def _bert_max_tokens(text_encoder, L):
    """The attention kernels' sequence limit of the encoder's regime."""
    if L > 256:
        raise ValueError("the masked attention kernels take at most 256 tokens")
    if L > 64 and bert_regime(text_encoder) == torch.float16:
        raise ValueError("the masked attention kernels take at most 64 tokens in the fp16 regime (256 in fp32)")


class TextEncoder(nn.Module):
    """CLIP text transformer (english) or a BERT encoder + text_proj (chinese); reference modules/module_cross.py:240-305."""

    def __init__(self, task_config, cross_config):
        super().__init__()
        self.language = task_config.language
        if self.language == "chinese":
            clip_sd = getattr(cross_config, "_clip_state_dict", None)
            if clip_sd is None:
                clip_sd = CLIP.get_config(pretrained_clip_name=getattr(task_config, "pretrained_clip_name", None)
                                          or cross_config.pretrained_clip_name)
            self.logit_scale = copy.deepcopy(clip_sd["logit_scale"]).float()
            self.bert_config = _bert_config(getattr(task_config, "pretrained_text", None))
            self.chinese_encoder = ChineseBert(self.bert_config)
            self.text_proj = nn.Linear(cross_config.chinese_hidden_size, cross_config.temporal_hidden_size)
            if cross_config.chinese_hidden_size != self.bert_config["hidden_size"]:
                raise ValueError(f"cross_config.chinese_hidden_size ({cross_config.chinese_hidden_size}) is not the encoder's "
                                 f"hidden_size ({self.bert_config['hidden_size']})")
            self.dtype = torch.float32
            # the id encode_many pads shorter inputs with (those positions carry mask 0 and are never read): config.json's
            # pad_token_id here; a model that owns the tokenizer's constants (BirdPreTrainedModel) assigns its [PAD] id
            self.pad_id = int(self.bert_config.get("pad_token_id", 0) or 0)
            return
        if self.language != "english":
            raise NotImplementedError(f"language {self.language!r}: the text encoder is the CLIP transformer (\"english\") or a "
                                      "BERT encoder (\"chinese\")")
        clip_state_dict, clip = _clip_for(task_config, cross_config)
        self.logit_scale = copy.deepcopy(clip_state_dict["logit_scale"]).float()    # plain tensor attribute, ln(100)
        self.token_embedding = copy.deepcopy(clip.token_embedding)
        self.positional_embedding = copy.deepcopy(clip.positional_embedding)
        self.transformer = copy.deepcopy(clip.transformer)
        self.ln_final = copy.deepcopy(clip.ln_final)
        self.text_projection = copy.deepcopy(clip.text_projection)
        self.dtype = clip.visual.conv1.weight.dtype

    def _forward_chinese(self, input_ids, attention_mask, return_hidden):
        """BertModel(input_ids, attention_mask) -> text_proj of the pooler output, or of every hidden row (reference
        modules/module_cross.py:273-277).  Dropout follows self.training, under torch.no_grad() too, as in HuggingFace; the
        seed of a call comes from torch's default host generator."""
        cfg = self.bert_config
        if not input_ids.is_cuda:
            raise TypeError(f"input_ids: expected a cuda tensor, got {input_ids.device}")
        b, L = input_ids.shape
        if L > cfg["max_position_embeddings"]:
            raise ValueError("sequence longer than the position embedding table")
        _bert_max_tokens(self, L)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if not attention_mask.is_cuda:
            raise TypeError(f"attention_mask: expected a cuda tensor, got {attention_mask.device}")
        mask = attention_mask.reshape(b, L).to(torch.int64).contiguous()
        ph = float(cfg.get("hidden_dropout_prob", 0.0)) if self.training else 0.0
        pa = float(cfg.get("attention_probs_dropout_prob", 0.0)) if self.training else 0.0
        seed = Fn.bert_seed() if (ph > 0 or pa > 0) else 0
        enc = self.chinese_encoder
        call_cfg = (cfg["num_attention_heads"], cfg["intermediate_size"], float(cfg.get("layer_norm_eps", 1e-12)), ph, pa, seed)
        return Fn.bert_text(input_ids.to(torch.int64).contiguous(), mask, call_cfg, "hidden" if return_hidden else "feat",
                            enc.pooler.dense.weight, enc.pooler.dense.bias, self.text_proj.weight, self.text_proj.bias,
                            *enc.flat_params())

    def forward(self, input_ids, attention_mask=None, return_hidden=False):
        bs_pair = input_ids.size(0)
        if self.language == "chinese":
            return self._forward_chinese(input_ids.view(bs_pair, -1), attention_mask, return_hidden)
        text_output, hidden = self.encode_text(input_ids, return_hidden=True, _want=("hidden" if return_hidden else "feat"))
        if return_hidden:
            return hidden.view(bs_pair, -1, hidden.size(-1))
        return text_output.view(bs_pair, text_output.size(-1))

    def encode_text(self, text, return_hidden=False, _want="both"):
        b, L = text.shape
        if L > self.positional_embedding.shape[0]:
            raise ValueError("sequence longer than the positional embedding table")
        # activations in self.dtype, a STORED attribute as in the reference (module_cross.py:256,288): model.float() alone leaves
        # it at fp16 and the text path then fails on mixed dtypes; the fp32 regime sets text_encoder.dtype = torch.float32 too
        x = Fn.TextEmbedFn.apply(text, self.token_embedding.weight, self.positional_embedding, self.dtype)
        x = self.transformer(x, b, L)
        feat = hidden = None
        if _want in ("both", "hidden"):
            hidden = Fn.LnProjFn.apply(x, None, self.ln_final.weight, self.ln_final.bias, self.text_projection).view(b, L, -1)
        if _want in ("both", "feat"):
            idx = ops.eot_index(text.contiguous())                                                  # EOT = largest id
            feat = Fn.LnProjFn.apply(x, idx, self.ln_final.weight, self.ln_final.bias, self.text_projection)
        if return_hidden:
            return feat, hidden
        return feat


def _encode_many(self, texts, wants, masks=None):
    """Several id tensors [b_i, L_i] through ONE pass of the text tower (padded with id 0 to the longest; the tower is
    causal and its rows independent, so every sequence's feature / hidden states are those of its own pass): one set of
    ~600 small launches instead of one per input, and ONE gradient per parameter where separate passes make autograd
    add two (the pre-training step runs the online title pass and the MLM pass of the masked titles on the same
    weights, modules/modeling.py:347-352,160-169, and two momentum passes, :369-373).
    wants[i]: "feat" -> [b_i, 512] (EOT row), "hidden" -> [b_i, L_i, 512].
    masks[i]: the attention mask of texts[i] (None: every token is real).  The Chinese tower needs them (shorter inputs are
    padded with [PAD] and mask 0); the CLIP tower is causal and reads its EOT row, so it ignores them."""
    if self.language == "chinese":
        return _encode_many_chinese(self, texts, wants, masks)
    Lmax = max(t.shape[1] for t in texts)
    if Lmax > self.positional_embedding.shape[0]:
        raise ValueError("sequence longer than the positional embedding table")
    ids = torch.cat([t if t.shape[1] == Lmax else torch.nn.functional.pad(t, (0, Lmax - t.shape[1])) for t in texts], dim=0)
    x = Fn.TextEmbedFn.apply(ids, self.token_embedding.weight, self.positional_embedding, self.dtype)
    x = self.transformer(x, ids.shape[0], Lmax)
    outs, row0 = [], 0
    for t, want in zip(texts, wants):
        b, L = t.shape
        if want == "feat":
            idx = ops.eot_index(t.contiguous(), base=row0 * Lmax, stride=Lmax)   # EOT = largest id
            outs.append(Fn.LnProjFn.apply(x, idx, self.ln_final.weight, self.ln_final.bias, self.text_projection))
        elif L == Lmax:
            rows = x[row0 * Lmax:(row0 + b) * Lmax]
            outs.append(Fn.LnProjFn.apply(rows, None, self.ln_final.weight, self.ln_final.bias, self.text_projection).view(b, L, -1))
        else:
            seq = torch.arange(row0, row0 + b, device=t.device)
            idx = (seq[:, None] * Lmax + torch.arange(L, device=t.device)[None, :]).reshape(-1).to(torch.int32)
            outs.append(Fn.LnProjFn.apply(x, idx, self.ln_final.weight, self.ln_final.bias, self.text_projection).view(b, L, -1))
        row0 += b
    return outs


def _encode_many_chinese(self, texts, wants, masks):
    """ONE hmmc_bert_fwd over all rows (and one hmmc_bert_bwd: one gradient per parameter); a "feat" segment's pooler reads
    its class rows in place, a "hidden" segment's text_proj runs over its rows (functional.BertManyFn).  One dropout seed per
    call, as for every tower call."""
    cfg = self.bert_config
    if masks is None:
        masks = [None] * len(texts)
    Lmax = max(t.shape[1] for t in texts)
    if Lmax > cfg["max_position_embeddings"]:
        raise ValueError("sequence longer than the position embedding table")
    _bert_max_tokens(self, Lmax)
    pad = int(self.pad_id)
    ids, ms, segs, row0 = [], [], [], 0
    for t, m, want in zip(texts, masks, wants):
        if not t.is_cuda:
            raise TypeError(f"input_ids: expected a cuda tensor, got {t.device}")
        b, L = t.shape
        m = torch.ones_like(t) if m is None else m.reshape(b, L)
        if not m.is_cuda:
            raise TypeError(f"attention_mask: expected a cuda tensor, got {m.device}")
        t, m = t.to(torch.int64), m.to(torch.int64)
        if L < Lmax:
            t = torch.nn.functional.pad(t, (0, Lmax - L), value=pad)
            m = torch.nn.functional.pad(m, (0, Lmax - L), value=0)
        ids.append(t)
        ms.append(m)
        segs.append((row0, b, want))
        row0 += b
    ph = float(cfg.get("hidden_dropout_prob", 0.0)) if self.training else 0.0
    pa = float(cfg.get("attention_probs_dropout_prob", 0.0)) if self.training else 0.0
    seed = Fn.bert_seed() if (ph > 0 or pa > 0) else 0
    enc = self.chinese_encoder
    call_cfg = (cfg["num_attention_heads"], cfg["intermediate_size"], float(cfg.get("layer_norm_eps", 1e-12)), ph, pa, seed)
    outs = Fn.bert_text_many(torch.cat(ids, dim=0).contiguous(), torch.cat(ms, dim=0).contiguous(), call_cfg, segs,
                             enc.pooler.dense.weight, enc.pooler.dense.bias, self.text_proj.weight, self.text_proj.bias,
                             *enc.flat_params())
    # a shorter input's padded positions are sliced off OUTSIDE the node: their gradient is exactly zero
    return [o if want == "feat" or t.shape[1] == Lmax else o[:, :t.shape[1]] for o, t, want in zip(outs, texts, wants)]


TextEncoder.encode_many = _encode_many


class BertLayerNorm(LayerNorm):
    pass


class BertPredictionHeadTransform(nn.Module):
    def __init__(self, hidden_size, hidden_act="gelu"):
        super().__init__()
        self.dense = nn.Linear(hidden_size, hidden_size)
        self.hidden_act = hidden_act
        self.LayerNorm = BertLayerNorm(hidden_size, eps=1e-12)


class BertLMPredictionHead(nn.Module):
    """MLM head container (reference modules/module_cross.py:308-357): dense, erf-GELU, LN(1e-12), decoder to vocab."""

    def __init__(self, hidden_size, vocab_size, hidden_act="gelu"):
        super().__init__()
        self.transform = BertPredictionHeadTransform(hidden_size, hidden_act)
        self.decoder = nn.Linear(hidden_size, vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(vocab_size))
        self.decoder.bias = self.bias

    def forward(self, hidden_states):
        """[..., hidden] -> [..., vocab] fp32 logits, differentiable (reference modules/module_cross.py:319-322).  The
        pre-training loss does not call this: calculate_mlm_loss evaluates head + cross-entropy on the labelled rows only."""
        t = self.transform
        return Fn.LmLogitsFn.apply(hidden_states.float(), t.dense.weight, t.dense.bias, t.LayerNorm.weight, t.LayerNorm.bias,
                                   self.decoder.weight, self.bias)
