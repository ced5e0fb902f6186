"""Plain fp64 statements of the fp32 head, pre-training (MoCo / BatchNorm) and optimizer ops, and the fp32 rounding bounds the
GPU tests hold the HIP kernels to (tests/test_gpu_heads.py).  tests/test_heads_reference.py pins each statement to the oracle
where the oracle states the op, so the kernels are compared with the reference's semantics, not with a second restatement.

Error model of the bounds: every fp32 operation rounds with relative error at most U = 2^-24; a sum evaluated as chains of at
most `c` dependent additions (per-lane loops, then a fixed tree) has absolute error at most c * U * sum|terms|; __expf(t) is
v_exp_f32(t * log2 e) (the product's rounding moves the result by |t| U relative, v_exp_f32 by at most 2 ulp) and __logf(s) is
v_log_f32(s) * ln 2.  The bounds are first-order in U; the tests allow twice the first-order value (SLACK) for the second-order
terms and the reference's own rounding.  Plain functions, no fixtures: this is not a conftest."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SLACK = 2.0
TINY = 2.0 ** -126            # results in fp32's denormal range may be flushed


def f64(t):
    return t.detach().to(torch.float64)


def exp_rel(t):
    """relative error bound of __expf at an argument t formed by one subtraction or product (its rounding: |t| U) and scaled by
    log2 e (|t| U), v_exp_f32 2 ulp, 2 U for the scalar factors around it"""
    return (2.0 * t.abs() + 4.0) * U


# ----------------------------------------------------------------------------- fine-tune head

def l2norm(x, eps=0.0):
    """F.normalize(x, dim=1, eps): x / max(||x||, eps) row-wise (eps = 0: the plain x / ||x|| of modules/modeling.py:210-214)."""
    n = x.norm(dim=1, keepdim=True)
    return x / (n.clamp_min(eps) if eps > 0 else n)


def infonce_cols(B, F_, device=None):
    """cols[i][blk]: the column of S_all holding (text i, block blk): video i for blk 0, frame blk-1 of video i after it."""
    b = torch.arange(B, device=device).unsqueeze(1)
    f = torch.arange(F_, device=device).unsqueeze(0)
    return torch.cat([b, B + b * F_ + f], dim=1)


def infonce_blocks(S, B, F_):
    """[1+F, B, B]: block 0 = the video-text logits, block 1+f = frame f of every video."""
    video = S[:, :B].unsqueeze(0)
    return torch.cat([video, S[:, B:].reshape(B, B, F_).permute(2, 0, 1)], dim=0) if F_ else video


def infonce(S, B, F_, w_video, w_frame):
    """Hierarchical InfoNCE on S_all [B, B(1+F)] (column c < B: video c; column B + b F + f: frame f of video b):
    loss = sum_blk w_blk (CrossEn(S_blk) + CrossEn(S_blk^T)), w_0 = w_video, w_f = w_frame (modules/modeling.py:665-672,702-709,
    until_module.py:196-205).  -> (loss, lse_row [B, 1+F], lse_col [B(1+F)])."""
    cols = infonce_cols(B, F_, S.device)
    lse_col = torch.logsumexp(S, dim=0)
    lse_row = torch.logsumexp(infonce_blocks(S, B, F_), dim=2).t()
    d = S.gather(1, cols)
    w = torch.tensor([w_video] + [w_frame] * F_, dtype=S.dtype, device=S.device)
    loss = (((lse_row - d) + (lse_col[cols] - d)) * w).sum() / B
    return loss, lse_row, lse_col


def lse_bound(x, dim, chain):
    """bound on |lse_kernel - lse| for x.logsumexp(dim) formed as max, sum of __expf(x - max) over `chain`-long chains, __logf:
    sum_j p_j (|x_j - m| + 4) U (the exponentials) + chain U (the sum, relative) + |lse| U + 4 (|log s| + 1) U (the log)."""
    m = x.amax(dim=dim, keepdim=True)
    t = x - m
    lse = torch.logsumexp(x, dim=dim, keepdim=True)
    p = torch.exp(x - lse)
    logs = (lse - m).abs()
    b = (p * exp_rel(t)).sum(dim=dim, keepdim=True) + chain * U + lse.abs() * U + 4.0 * (logs + 1.0) * U
    return b.squeeze(dim)


def infonce_bounds(S, B, F_, w_video, w_frame, gout):
    """fp32 bounds of (loss, lse_row, lse_col, dS) of hmmc_infonce_fwd / _bwd (heads_f32.hip): row LSE over 64 lanes
    (chain ceil(B/64) + 6), column LSE over 8 row lanes (online: ceil(B/8) rescales, + 8 merges), loss one 256-thread block
    over B(1+F) terms (chain ceil(B(1+F)/256) + 8), dS = g w / B (p_row + p_col - 2 [diag])."""
    C = B * (1 + F_)
    cols = infonce_cols(B, F_, S.device)
    blocks = infonce_blocks(S, B, F_)
    b_row = lse_bound(blocks, 2, math.ceil(B / 64) + 6).t()
    # the online column sum rescales the running sum by __expf(m_old - m_new) at each new maximum: the arguments add up to at
    # most the column's range, one rescale per row at most
    b_col = lse_bound(S, 0, math.ceil(B / 8) + 8) + (S.amax(0) - S.amin(0) + 4 * math.ceil(B / 8)) * U
    loss, lse_row, lse_col = infonce(S, B, F_, w_video, w_frame)
    w = torch.tensor([w_video] + [w_frame] * F_, dtype=S.dtype, device=S.device)
    d = S.gather(1, cols)
    terms = ((lse_row - d) + (lse_col[cols] - d)) * w
    b_loss = ((b_row + b_col[cols]) * w.abs()).sum() / B + (math.ceil(C / 256) + 12) * U * terms.abs().sum() / B + U * loss.abs()
    # dS
    wc = torch.cat([torch.full((B,), w_video, dtype=S.dtype, device=S.device),
                    torch.full((B * F_,), w_frame, dtype=S.dtype, device=S.device)])
    blk_of_col = torch.cat([torch.zeros(B, dtype=torch.long, device=S.device),
                            1 + torch.arange(F_, device=S.device).repeat(B)])
    lr_full = lse_row[:, blk_of_col]                              # [B, C]
    pr = torch.exp(S - lr_full)
    pc = torch.exp(S - lse_col.unsqueeze(0))
    br = b_row[:, blk_of_col]
    e = pr * (exp_rel(S - lr_full) + br) + pc * (exp_rel(S - lse_col.unsqueeze(0)) + b_col.unsqueeze(0))
    diag = torch.zeros_like(S)
    diag.scatter_(1, cols, 2.0)
    g = float(gout) * wc.abs().unsqueeze(0) / B
    b_dS = g * (e + 2 * U * (pr + pc + diag)) + 3 * U * g * (pr + pc - diag).abs() + TINY
    return b_loss, b_row, b_col, b_dS


def topk_mean(Sf, bq, bv, F_, k, base=None, lds=None, ldb=None):
    """out[i][b] = base[i*ldb + b] + mean of the k largest Sf[i*lds + b*F + f] (main_task_retrieval.py:332-336)."""
    lds = lds or bv * F_
    ldb = ldb or bv
    v = Sf.reshape(-1).as_strided((bq, bv, F_), (lds, F_, 1))
    out = torch.topk(v, k, dim=2).values.mean(dim=2)
    if base is not None:
        out = out + base.reshape(-1).as_strided((bq, bv), (ldb, 1))
    return out


def segment_max(S, offsets):
    return torch.stack([S[int(offsets[g]):int(offsets[g + 1])].amax(dim=0) for g in range(len(offsets) - 1)])


def temporal_pool(h, u, b, F_, D):
    """mean_f (h + u) / ||h + u|| per video (modules/module_cross.py:207-212)."""
    vf = h + u if u is not None else h
    return (vf / vf.norm(dim=1, keepdim=True)).view(b, F_, D).mean(dim=1)


def add_rowbias(x, table, period):
    r = torch.arange(x.shape[0], device=x.device) % period
    return x + table[r]


def attention(qkv, b, L, H, causal):
    """nn.MultiheadAttention's core on packed [b L, 3 D] rows Q | K | V, head dim 64, q scaled by 1/8, optional causal mask
    (modules/module_cross.py:127-131, module_clip.py:235,251).  -> (out [b L, D], probs [b, H, L, L])."""
    D = H * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(b, L, H, 64).transpose(1, 2) for i in range(3))
    s = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(b * L, D)
    return o, p


def attention_bounds(qkv, dout, b, L, H, causal):
    """fp32 bounds of out, probs (forward) and dqkv (backward) of hmmc_temporal_attention_*: scores are 64-long dot-product chains,
    the softmax a max, F __expf and an L-long sum, every output an L- or 64-long chain; the backward reads the kernel's probs
    (held to the probs bound) and forms delta_i = sum_j p_ij dP_ij over L terms."""
    D = H * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(b, L, H, 64).transpose(1, 2) for i in range(3))
    dO = dout.reshape(b, L, H, 64).transpose(1, 2)
    mask = torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1) if causal else None
    s = (q * 0.125) @ k.transpose(-1, -2)
    es = 64 * U * ((q * 0.125).abs() @ k.abs().transpose(-1, -2))              # score error
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
        es = es.masked_fill(mask, 0.0)
    p = torch.softmax(s, dim=-1)
    t = (s - s.amax(dim=-1, keepdim=True)).masked_fill(p == 0, 0.0)
    per = 2 * es + exp_rel(t) + U * t.abs()                                      # exp(s - m): s and the max both carry es
    rel_p = per + (p * per).sum(-1, keepdim=True) + (L + 2) * U                 # normalisation
    b_p = p * rel_p + TINY
    b_o = (b_p @ v.abs()) + L * U * (p @ v.abs())
    # backward
    dP = dO @ v.transpose(-1, -2)
    edP = 64 * U * (dO.abs() @ v.abs().transpose(-1, -2))
    delta = (p * dP).sum(-1, keepdim=True)
    edelta = (b_p * dP.abs() + p * edP).sum(-1, keepdim=True) + L * U * (p * dP).abs().sum(-1, keepdim=True)
    dS = p * (dP - delta) * 0.125
    edS = 0.125 * (b_p * (dP - delta).abs() + p * (edP + edelta + U * (dP.abs() + delta.abs()))) + 2 * U * dS.abs()
    edq = edS @ k.abs() + L * U * (dS.abs() @ k.abs())
    edk = edS.transpose(-1, -2) @ q.abs() + L * U * (dS.abs().transpose(-1, -2) @ q.abs())
    edv = b_p.transpose(-1, -2) @ dO.abs() + L * U * (p.transpose(-1, -2) @ dO.abs())
    b_dqkv = torch.cat([e.transpose(1, 2).reshape(b * L, D) for e in (edq, edk, edv)], dim=1) + TINY
    return b_o.transpose(1, 2).reshape(b * L, D) + TINY, b_p, b_dqkv


# ----------------------------------------------------------------------------- pre-training (MoCo) heads

def bn_relu(h, gamma, beta, eps):
    """relu(BatchNorm1d(h)) with train-mode batch statistics (modules/modeling.py:788-807) -> (y, mean, biased var)."""
    mean = h.mean(0)
    var = h.var(0, unbiased=False)
    return torch.relu((h - mean) / torch.sqrt(var + eps) * gamma + beta), mean, var


def bn_running(rm, rv, mean, var, n, momentum):
    """nn.BatchNorm1d's running statistics: exponential average with the unbiased variance."""
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * n / max(n - 1, 1)


def moco_loss(S, lpos, T, w):
    """w * sum_r CE([lpos_r, S_r] / T, label 0) (contrastive_loss, modules/modeling.py:286-313, summed over rows) -> (loss, lse)."""
    logits = torch.cat([lpos.unsqueeze(1), S], dim=1) / T
    lse = torch.logsumexp(logits, dim=1)
    return w * (lse - lpos / T).sum(), lse


def gelu_erf(x):
    """modules/module_cross.py:33-39."""
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ce_sum(logits, labels):
    """sum over rows with label >= 0 of CE (F.cross_entropy's ignore_index rows dropped) -> (sum, lse, count)."""
    valid = labels >= 0
    lse = torch.logsumexp(logits, dim=1)
    lab = labels.clamp_min(0)
    rows = (lse - logits.gather(1, lab.unsqueeze(1)).squeeze(1)) * valid
    return rows.sum(), lse, int(valid.sum())


def enqueue(keys, queue, col0):
    """queue[:, col0:col0+R] = F.normalize(keys, dim=1).T (modules/modeling.py:244-284)."""
    q = queue.clone()
    q[:, col0:col0 + keys.shape[0]] = F.normalize(keys, dim=1, eps=1e-12).t()
    return q


# ----------------------------------------------------------------------------- optimizer

def bert_adam_step(p, g, m, v, lr_t, wd, b1=0.9, b2=0.98, e=1e-6, max_grad_norm=1.0):
    """BertAdam.step for one tensor (modules/optimization.py:103-168) at the scheduled learning rate lr_t, as plain math."""
    if max_grad_norm > 0:
        g = g * min(1.0, max_grad_norm / (float(g.norm()) + 1e-6))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = m / (v.sqrt() + e)
    if wd > 0.0:
        u = u + wd * p
    return p - lr_t * u, m, v, g


def clip_grad_norm(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ with exact norms -> (total norm, clipped gradients)."""
    total = math.sqrt(sum(float((g.to(torch.float64) ** 2).sum()) for g in grads))
    c = min(1.0, max_norm / (total + 1e-6))
    return total, [g.to(torch.float64) * c for g in grads]


# ----------------------------------------------------------------------------- bounds of the other kernels (fp32 rounding, first order)

def l2_chain(D):
    return 4 * math.ceil(D / 256) + 6                          # f4 loads: 4 terms per step, then the 6-level butterfly


def l2norm_bounds(x, dy, eps, D):
    c = l2_chain(D)
    n = x.norm(dim=1, keepdim=True).clamp_min(eps) if eps else x.norm(dim=1, keepdim=True)
    zero = x.norm(dim=1, keepdim=True) < eps
    en = torch.where(zero, torch.full_like(n, U), torch.full_like(n, (c / 2 + 1) * U))    # relative, of the norm (eps: fp32(eps))
    ey = (c / 2 + 3) * U
    y = x / n
    s = (y * dy).sum(1, keepdim=True)
    dx = (dy - y * s) / n
    es = c * U * (y * dy).abs().sum(1, keepdim=True) + ey * (y.abs() * dy.abs()).sum(1, keepdim=True)
    b_dx = (y.abs() * es + s.abs() * y.abs() * (ey + U) + U * (dy - y * s).abs()) / n + (en + 2 * U) * dx.abs()
    return ey * y.abs(), en * n, b_dx


def pool_bounds(h, u, dout, b, F_, D):
    c = math.ceil(D / 64) + 6
    vf = h + u if u is not None else h
    n = vf.norm(dim=1, keepdim=True)
    en = (c / 2 + 2) * U
    yn = vf / n
    ey = en + 2 * U
    b_out = (yn.abs() * (ey + (math.ceil(F_ / 4) + 4) * U)).view(b, F_, D).sum(1) / F_ + U * yn.view(b, F_, D).mean(1).abs()
    do = dout.repeat_interleave(F_, 0)
    s = (yn * do).sum(1, keepdim=True)
    es = c * U * (yn * do).abs().sum(1, keepdim=True) + ey * (yn.abs() * do.abs()).sum(1, keepdim=True)
    dv = (do - yn * s) / n / F_
    b_dv = (yn.abs() * es + s.abs() * yn.abs() * (ey + U) + U * (do - yn * s).abs()) / n / F_ + (en + 3 * U) * dv.abs()
    return b_out, b_dv


def bn_fwd_bounds(hd, gamma, n, mom, rm, rv, eps):
    s1, s2 = hd.sum(0), (hd * hd).sum(0)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0)
    em = U * mean.abs()
    ev = U * ((s2 / n).abs() + 3 * mean * mean + var)
    rstd = 1 / torch.sqrt(var + eps)
    erstd = rstd * ((ev + U * (var + eps)) / (2 * (var + eps)) + 2 * U)
    xm = hd - mean
    z0 = xm * rstd * gamma
    ez = gamma.abs() * (rstd * (em + U * xm.abs()) + xm.abs() * erstd) + 2 * U * z0.abs()
    vu = var * n / max(n - 1, 1)
    erm = 3 * U * ((1 - mom) * rm.abs() + mom * mean.abs() + ((1 - mom) * rm + mom * mean).abs()) + mom * em
    erv = 3 * U * ((1 - mom) * rv.abs() + mom * vu + ((1 - mom) * rv + mom * vu).abs()) + mom * (ev * n / max(n - 1, 1) + 2 * U * vu)
    return dict(em=em, ev=ev, erstd=erstd, ez=ez, erm=erm, erv=erv, mean=mean, rstd=rstd, xm=xm)


def bn_bwd_bound(hd, dyd, gamma, fb, M, N, out_relu):
    """dh = gamma rstd (d - S_d / n - xhat S_dx / n), d = dy [z > 0]; S_d, S_dx: per-slab column sums (row lanes of
    ceil(rows_per_slab / 8) terms, an 8-term merge, then a sequential sum over <= 256 slabs)."""
    slabs = min(256, max(1, (M + 63) // 64))
    rpb = (M + slabs - 1) // slabs
    slabs = (M + rpb - 1) // rpb
    chain = math.ceil(rpb / 8) + 8 + slabs
    d = dyd * (out_relu > 0)
    rstd, xm = fb["rstd"], fb["xm"]
    xh = xm * rstd
    exh = (U * xm.abs() + fb["em"]) * rstd + xm.abs() * fb["erstd"] + 2 * U * xh.abs()
    Sd, Sdx = d.sum(0), (d * xh).sum(0)
    eSd = chain * U * d.abs().sum(0)
    eSdx = chain * U * (d * xh).abs().sum(0) + (d.abs() * exh).sum(0) + 2 * U * (d * xh).abs().sum(0)
    inner = d - Sd / M - xh * Sdx / M
    e_in = eSd / M + 2 * U * (Sd / M).abs() + exh * (Sdx / M).abs() + xh.abs() * (eSdx / M + 2 * U * (Sdx / M).abs()) \
        + 2 * U * (d.abs() + (Sd / M).abs() + (xh * Sdx / M).abs())
    dh = gamma * rstd * inner
    return gamma.abs() * (fb["erstd"] * inner.abs() + rstd * e_in) + 2 * U * dh.abs() + TINY


def moco_bounds(Sd, lpd, Kq, R_, w, g, T):
    x = torch.cat([lpd.unsqueeze(1), Sd], dim=1) / T
    chain = math.ceil(Kq / 256) + 11
    lse = torch.logsumexp(x, 1)
    e_lse = lse_bound(x, 1, chain) + 2 * U * x.abs().amax(1)              # the arguments: S * fp32(1 / T)
    rowloss = w * (lse - lpd / T)
    e_row = abs(w) * (e_lse + 2 * U * (lpd / T).abs() + U * (lse - lpd / T).abs()) + U * rowloss.abs()
    b_loss = e_row.sum() + (math.ceil(R_ / 256) + 8) * U * rowloss.abs().sum()
    gg = g * w / T
    t = Sd / T - lse.unsqueeze(1)
    dS = gg * torch.exp(t)
    b_dS = dS.abs() * (exp_rel(t) + 2 * U * (Sd / T).abs() + e_lse.unsqueeze(1) + 5 * U) + TINY
    tp = lpd / T - lse
    pp = torch.exp(tp)
    b_dl = abs(gg) * (pp * (exp_rel(tp) + 2 * U * (lpd / T).abs() + e_lse) + U * (pp + 1)) + 4 * U * (gg * (pp - 1)).abs()
    return e_lse, b_loss, b_dS, b_dl


def gelu_bounds(x, dy):
    """fwd y = (x / 2)(1 + erff(x * fp32(1/sqrt 2))): erff within 4 U of erf (absolute, |erf| <= 1) plus the argument's two
    roundings (<= U after erf's slope), then 3 roundings.  bwd dx = dy (cdf + x pdf), pdf = fp32(1/sqrt(2 pi)) __expf(-x^2 / 2):
    __expf's error grows with its argument, (x^2 + 4) U relative (exp_rel at x^2 / 2), plus the roundings of
    -0.5 x x (2 U of x^2 / 2 in the exponent)."""
    c = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    y = x * c
    b_y = 0.5 * x.abs() * (5 * U + U * 2 * c) + 2 * U * y.abs() + TINY
    e_cdf = 0.5 * (5 * U + 2 * U * c) + U * c
    e_pdf = pdf * (exp_rel(0.5 * x * x) + 2 * U * 0.5 * x * x + 2 * U)
    b_dx = dy.abs() * (e_cdf + x.abs() * e_pdf + U * (x * pdf).abs() + 2 * U * (c + x * pdf).abs()) + TINY
    return b_y, b_dx


def clip_rel(nmax, T_):
    """relative bound of the total norm: chunk sums (f4 loads: 4 terms a step over <= 32 steps, the scalar tail, block_sum's
    10 levels), <= 2 chunks a lane + 6 levels per tensor, sqrt and square, ceil(T / 256) + 10 over the tensors, sqrt."""
    chunk = 4 * math.ceil(min(nmax, 32768) / 1024) + 4 + 10
    per_t = math.ceil(math.ceil(nmax / 32768) / 64) + 6
    return (chunk + per_t + 2 + math.ceil(T_ / 256) + 10) / 2 * U + U


def detects(ref, slipped, bound):
    """the slip moves some element by more than the tolerance the family's test allows"""
    return bool(((slipped - ref).abs() > SLACK * bound).any())
