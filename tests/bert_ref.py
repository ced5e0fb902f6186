"""Plain-torch CPU restatement of the Chinese text branch (reference modules/module_cross.py:257-265,273-277: a HuggingFace
BertModel - post-LN, erf-GELU, an additive finfo.min key mask, a tanh pooler - followed by text_proj).  Same role as
tests/heads_ref.py: the definition the HIP kernels are held to, in any dtype (fp64 for the kernel tests), differentiable by
autograd.  Every dropout site takes an explicit optional keep mask (1 = kept), applied as x * keep / (1 - p)."""
import math

import torch
import torch.nn.functional as F


def dropout(x, keep, p):
    if keep is None or p == 0:
        return x
    return x * keep.to(x.dtype) / (1.0 - p)


def embed_ln(ids, word, pos, typ, gamma, beta, eps=1e-12):
    """LN(word[ids] + pos[:L] + type[0]); ids [b, L] -> [b, L, D]."""
    L = ids.shape[1]
    e = word[ids] + pos[:L][None] + typ[0][None, None]
    return F.layer_norm(e, (e.shape[-1],), gamma, beta, eps)


def masked_attention(qkv, mask, heads, keep=None, p=0.0):
    """qkv [b, L, 3D] (Q | K | V), mask [b, L] (nonzero = valid key) -> (out [b, L, D], probs after dropout [b, H, L, L],
    the softmax itself)."""
    b, L, D3 = qkv.shape
    D = D3 // 3
    q, k, v = [t.reshape(b, L, heads, 64).transpose(1, 2) for t in qkv.split(D, dim=-1)]
    scores = q @ k.transpose(-1, -2) / math.sqrt(64)
    add = torch.zeros(b, 1, 1, L, dtype=qkv.dtype)
    add.masked_fill_((mask == 0)[:, None, None, :], torch.finfo(qkv.dtype).min)
    raw = torch.softmax(scores + add, dim=-1)
    probs = dropout(raw, keep, p)
    out = (probs @ v).transpose(1, 2).reshape(b, L, D)
    return out, probs, raw


def pooler(x, w, bias):
    """tanh(x[:, 0] W^T + b)."""
    return torch.tanh(x[:, 0] @ w.T + bias)


def layer(x, mask, W, heads, eps=1e-12, p_hidden=0.0, p_attn=0.0, keeps=(None, None, None)):
    """One BertLayer.  W: the 16 tensors in hmmc_bert_fwd's order; keeps: (probabilities, after attention.output.dense,
    after output.dense)."""
    qw, qb, kw, kb, vw, vb, aow, aob, l1w, l1b, iw, ib, ow, ob, l2w, l2b = W
    qkv = torch.cat([x @ qw.T + qb, x @ kw.T + kb, x @ vw.T + vb], dim=-1)
    att, _, _ = masked_attention(qkv, mask, heads, keeps[0], p_attn)
    x1 = F.layer_norm(dropout(att @ aow.T + aob, keeps[1], p_hidden) + x, (x.shape[-1],), l1w, l1b, eps)
    g = F.gelu(x1 @ iw.T + ib)
    return F.layer_norm(dropout(g @ ow.T + ob, keeps[2], p_hidden) + x1, (x.shape[-1],), l2w, l2b, eps)


LAYER_KEYS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
              "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")


def layer_params(sd, prefix, i):
    p = f"{prefix}chinese_encoder.encoder.layer.{i}."
    return [sd[p + k + s] for k in LAYER_KEYS for s in (".weight", ".bias")]


def text_encoder(sd, ids, mask, cfg, prefix="text_encoder.", want="feat", keeps=None):
    """TextEncoder(language="chinese").forward: sd holds chinese_encoder.* / text_proj.* (any float dtype); cfg: the config
    dict (num_hidden_layers, num_attention_heads, layer_norm_eps, the two dropout probabilities).  keeps: None, or a dict
    site -> keep mask with the sites numbered as hmmc_bert_fwd numbers them."""
    e = prefix + "chinese_encoder.embeddings."
    eps = cfg.get("layer_norm_eps", 1e-12)
    ph, pa = cfg.get("hidden_dropout_prob", 0.0), cfg.get("attention_probs_dropout_prob", 0.0)
    keeps = keeps or {}
    x = embed_ln(ids, sd[e + "word_embeddings.weight"], sd[e + "position_embeddings.weight"], sd[e + "token_type_embeddings.weight"],
                 sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], eps)
    x = dropout(x, keeps.get(0), ph)
    for i in range(cfg["num_hidden_layers"]):
        x = layer(x, mask, layer_params(sd, prefix, i), cfg["num_attention_heads"], eps, ph, pa,
                  (keeps.get(1 + 3 * i), keeps.get(2 + 3 * i), keeps.get(3 + 3 * i)))
    pw, pb = sd[prefix + "text_proj.weight"], sd[prefix + "text_proj.bias"]
    if want == "hidden":
        return x @ pw.T + pb
    pooled = pooler(x, sd[prefix + "chinese_encoder.pooler.dense.weight"], sd[prefix + "chinese_encoder.pooler.dense.bias"])
    return pooled @ pw.T + pb
