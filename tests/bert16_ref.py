"""Plain-torch CPU restatement of the fp16 regime of the Chinese text branch (hmmc_amd/csrc/bert_f16.hip): fp32 arithmetic
with .half() exactly at the rounding points that file's header names, forward AND backward (the backward is written out by
hand, as the kernels run it, because its intermediate gradients are rounded too).  tests/hotpath_ref.py's role for the CLIP
towers.  tests/bert_ref.py in fp64 remains the definition; this file only says how much error the regime itself carries.
Every dropout site takes an explicit keep mask (1 = kept)."""
import math

import torch

import bert_ref


def r(x):
    """one fp16 rounding"""
    return x.half().float()


def _drop(x, keep, p):
    return x if keep is None or p == 0 else x * keep.float() / (1.0 - p)


def linear(x, w, b, resid=None):
    y = r(x @ w.T + b)
    return y if resid is None else r(resid + y)


def dgrad(dy, w, resid=None):
    y = r(dy @ w)
    return y if resid is None else r(resid + y)


def wgrad(dy, x):
    return r(dy.T @ x)


def colsum(dy):
    return r(dy.sum(0))


def gelu_fwd(h):
    return r(h * 0.5 * (1.0 + torch.erf(h * 0.7071067811865476)))


def gelu_bwd(h, dg):
    cdf = 0.5 * (1.0 + torch.erf(h * 0.7071067811865476))
    return r(dg * (cdf + h * 0.3989422804014327 * torch.exp(-0.5 * h * h)))


def dropout_fwd(x, keep, p, resid=None):
    y = _drop(x, keep, p)
    return r(y if resid is None else y + resid)


def dropout_bwd(dy, keep, p):
    return r(_drop(dy, keep, p))


def ln_fwd(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rs
    return r(xh * g + b), (xh, rs)


def ln_bwd(dy, saved, g):
    xh, rs = saved
    dxh = dy * g
    dx = rs * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    return r(dx), (dy * xh).sum(0), dy.sum(0)


def _heads(t, b, L, H):
    return t.reshape(b, L, H, 64).transpose(1, 2)


def attention_fwd(qkv, mask, H, keep=None, p=0.0):
    """qkv [b, L, 3D] (fp16 values) -> (out [b, L, D], lse [b, H, L]); keep [b, H, L, L]."""
    b, L, D3 = qkv.shape
    D = D3 // 3
    q, k, v = [_heads(t, b, L, H) for t in qkv.split(D, dim=-1)]
    dead = (mask == 0)[:, None, None, :]
    s = (q @ k.transpose(-1, -2) * 0.125).masked_fill(dead, -math.inf)
    P = torch.softmax(s, dim=-1)
    Pd = r(_drop(P, keep, p))
    out = r(Pd @ v.masked_fill(dead.transpose(-1, -2), 0.0))
    return out.transpose(1, 2).reshape(b, L, D), torch.logsumexp(s, dim=-1)


def attention_bwd(qkv, mask, H, dout, keep=None, p=0.0):
    b, L, D3 = qkv.shape
    D = D3 // 3
    q, k, v = [_heads(t, b, L, H) for t in qkv.split(D, dim=-1)]
    dead = (mask == 0)[:, None, None, :]
    k, v = k.masked_fill(dead.transpose(-1, -2), 0.0), v.masked_fill(dead.transpose(-1, -2), 0.0)
    dO = _heads(dout, b, L, H)
    P = torch.softmax((q @ k.transpose(-1, -2) * 0.125).masked_fill(dead, -math.inf), dim=-1)
    dP = _drop(dO @ v.transpose(-1, -2), keep, p)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = r(P * (dP - delta) * 0.125)
    Pd = r(_drop(P, keep, p))
    dq, dk, dv = r(dS @ k), r(dS.transpose(-1, -2) @ q), r(Pd.transpose(-1, -2) @ dO)
    return torch.cat([t.transpose(1, 2).reshape(b, L, D) for t in (dq, dk, dv)], dim=-1)


def pooler_fwd(x, w, bias):
    """x [b, L, D] -> fp16(tanh(fp16(x[:, 0] W^T + b)))"""
    return r(torch.tanh(r(x[:, 0] @ w.T + bias)))


def pooler_bwd(dy, y, x, w):
    """-> (dx of the class rows [b, D], dW, db)"""
    dz = r(dy * (1.0 - y * y))
    return r(dz @ w), r(dz.T @ x[:, 0]), r(dz.sum(0))


def convert_state(sd, prefix="text_encoder."):
    """The values convert_bert_weights leaves, as fp32 tensors: dense weights / biases rounded to fp16, the rest untouched."""
    out = {}
    for k, v in sd.items():
        fixed = "embeddings." in k or "LayerNorm." in k or not k.startswith(prefix)
        out[k] = v.detach().clone().float() if fixed else r(v.detach().float())
    return out


def text_encoder(sd, ids, mask, cfg, dout, prefix="text_encoder.", want="feat", keeps=None):
    """Forward and backward of TextEncoder(language="chinese") in the fp16 regime.  sd: convert_state's values; dout: the
    gradient of the returned features.  -> (features fp32, {state_dict name: gradient})."""
    eps = cfg.get("layer_norm_eps", 1e-12)
    ph, pa = cfg.get("hidden_dropout_prob", 0.0), cfg.get("attention_probs_dropout_prob", 0.0)
    H, nl = cfg["num_attention_heads"], cfg["num_hidden_layers"]
    keeps = keeps or {}
    b, L = ids.shape
    e = prefix + "chinese_encoder.embeddings."
    emb_names = [e + n for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                                 "LayerNorm.weight", "LayerNorm.bias")]
    emb = [sd[n].detach().clone().requires_grad_() for n in emb_names]
    x0_32 = bert_ref.dropout(bert_ref.embed_ln(ids, *emb, eps), keeps.get(0), ph)          # fp32, by autograd
    x = r(x0_32.detach()).reshape(b * L, -1)
    D = x.shape[1]
    saved = []
    for i in range(nl):
        W = bert_ref.layer_params(sd, prefix, i)
        kp = (keeps.get(1 + 3 * i), keeps.get(2 + 3 * i), keeps.get(3 + 3 * i))
        kp = (kp[0], None if kp[1] is None else kp[1].reshape(b * L, D), None if kp[2] is None else kp[2].reshape(b * L, D))
        qkv = torch.cat([linear(x, W[2 * j], W[2 * j + 1]) for j in range(3)], dim=-1)
        att, _ = attention_fwd(qkv.reshape(b, L, 3 * D), mask, H, kp[0], pa)
        att = att.reshape(b * L, D)
        pre1 = dropout_fwd(linear(att, W[6], W[7]), kp[1], ph, x) if ph > 0 else linear(att, W[6], W[7], x)
        x1, s1 = ln_fwd(pre1, W[8], W[9], eps)
        h = linear(x1, W[10], W[11])
        g = gelu_fwd(h)
        pre2 = dropout_fwd(linear(g, W[12], W[13]), kp[2], ph, x1) if ph > 0 else linear(g, W[12], W[13], x1)
        y, s2 = ln_fwd(pre2, W[14], W[15], eps)
        saved.append((x, qkv, att, s1, x1, h, g, s2, kp))
        x = y
    pw, pb = sd[prefix + "chinese_encoder.pooler.dense.weight"], sd[prefix + "chinese_encoder.pooler.dense.bias"]
    tw, tb = sd[prefix + "text_proj.weight"], sd[prefix + "text_proj.bias"]
    G = {}
    d = r(dout.float().reshape(-1, dout.shape[-1]))
    G[prefix + "text_proj.bias"] = colsum(d)
    if want == "hidden":
        out = linear(x, tw, tb).reshape(b, L, -1)
        G[prefix + "text_proj.weight"] = wgrad(d, x)
        gin = dgrad(d, tw)
    else:
        x3 = x.reshape(b, L, D)
        pooled = pooler_fwd(x3, pw, pb)
        out = linear(pooled, tw, tb)
        G[prefix + "text_proj.weight"] = wgrad(d, pooled)
        dcls, G[prefix + "chinese_encoder.pooler.dense.weight"], G[prefix + "chinese_encoder.pooler.dense.bias"] = \
            pooler_bwd(dgrad(d, tw), pooled, x3, pw)
        gin = torch.zeros(b, L, D)
        gin[:, 0] = dcls
        gin = gin.reshape(b * L, D)
    for i in reversed(range(nl)):
        W = bert_ref.layer_params(sd, prefix, i)
        names = [f"{prefix}chinese_encoder.encoder.layer.{i}.{k}{s}" for k in bert_ref.LAYER_KEYS for s in (".weight", ".bias")]
        xi, qkv, att, s1, x1, h, g, s2, kp = saved[i]
        g_ = [None] * 16
        dA, g_[14], g_[15] = ln_bwd(gin, s2, W[14])
        da2 = dropout_bwd(dA, kp[2], ph) if ph > 0 else dA
        g_[13] = colsum(da2)
        g_[12] = wgrad(da2, g)
        dh = gelu_bwd(h, dgrad(da2, W[12]))
        g_[11], g_[10] = colsum(dh), wgrad(dh, x1)
        dC = dgrad(dh, W[10], dA)
        dD, g_[8], g_[9] = ln_bwd(dC, s1, W[8])
        da1 = dropout_bwd(dD, kp[1], ph) if ph > 0 else dD
        g_[7], g_[6] = colsum(da1), wgrad(da1, att)
        dqkv = attention_bwd(qkv.reshape(b, L, 3 * D), mask, H, dgrad(da1, W[6]).reshape(b, L, D), kp[0], pa).reshape(b * L, 3 * D)
        acc = dD
        for j in range(3):
            dj = dqkv[:, j * D:(j + 1) * D]
            g_[2 * j + 1], g_[2 * j] = colsum(dj), wgrad(dj, xi)
            acc = dgrad(dj, W[2 * j], acc)
        gin = acc
        G.update(zip(names, g_))
    x0_32.backward(gin.reshape(b, L, D))
    G.update({n: t.grad for n, t in zip(emb_names, emb)})
    return out, G
