"""Plain fp64 statements of the fp16 hot path - the GEMM epilogues and the fp32 split-K slab paths of the weight gradients
(gemm_f16.hip), the fused attention (attention_f16.hip, attention_long_f16.hip) and LayerNorm (norm_elem.hip) - and the per-element rounding bounds tests/test_gpu_hotpath.py holds the
HIP kernels to.  tests/test_hotpath_reference.py pins each statement (torch.nn.functional in fp64, the oracle, autograd), shows
with a torch emulation of each kernel's arithmetic that the bounds are not too tight, and with test_slip_* that they are not too
loose.  U, SLACK and exp_rel are those of heads_ref.

Error model (first order; the tests allow SLACK times the bound for the second-order terms).  fp16 inputs are exact.  MFMA
accumulates in fp32: a K-term dot product is within K U sum|a_k b_k|.  fp32 operations round with U, a sum formed as chains of
at most c dependent additions is within c U sum|terms|, __expf / v_exp_f32 as heads_ref.exp_rel.  Every point where a kernel
rounds to fp16 contributes r16(value) = U16 |value| + SUB16 (one subnormal step: nothing is excluded below the normal range),
propagated to first order to the output.  The rounding points, as read off the kernels:
  attention, L <= 64    P = fp16(e / sum) in front of P V;  stored O;  backward: P from the saved lse in fp32, delta = rowsum(P o dP)
                        in fp32, dS = fp16(P (dP - delta) / 8) in front of the dQ / dK MFMAs, P = fp16(P) in front of dV; dP is
                        NOT rounded; stored dQ, dK, dV (x the row factor first in the row-scaled variant)
  attention, L > 64     P = fp16(e), the un-normalised exponential, in front of P V, the row normalised afterwards;  stored O;
                        backward: delta = <dO, O> from the STORED fp16 O;  dS = fp16(P (dP - delta)), the 1/8 applied to the
                        accumulated dQ / dK;  P = fp16(P) in front of dV;  stored dQ, dK, dV
  dbias_partial         fp32 sums over a sequence's rows of the fp16-rounded, unscaled dQ | dK | dV
  GEMM epilogues        h = fp16(acc + bias);  out = fp16(resid + h);  QuickGELU on fp16 tensors as torch evaluates it:
                        t = fp16(1.702 h), s = fp16(sigmoid(t)), out = fp16(h s);  aux = h, or fp16(QuickGELU'(h)) from the
                        fp32 sigmoid;  fp16(acc QuickGELU'(aux));  fp16(acc aux)
  COLSUM                fp32 sums of the fp16 values written to C: one partial row per 128 (256x256 tile) or 64 rows
  split-K slabs         fp32 partial sums per K split (no rounding to fp16), added in split order by the reduce; ONE rounding to
                        fp16 at the end, none for the grouped launch's fp32 output dW32 (wgrad_bound)
  LayerNorm             fp32 statistics; the stored y / dx (fp16 towers), the fp16 column sums of dx
Bounds are functions of the fp64 reference and the inputs only, never of a kernel's output.  Plain functions, no fixtures."""
from __future__ import annotations

import math

import torch

from heads_ref import SLACK, U, exp_rel, f64  # noqa: F401  (re-exported for the tests)

U16 = 2.0 ** -11              # unit roundoff of binary16
SUB16 = 2.0 ** -24            # one subnormal step of binary16
D64 = torch.float64

EPI_BIAS, EPI_RESID, EPI_QGELU, EPI_DGELU, EPI_COLSUM, EPI_SAVE_DGELU, EPI_MULAUX = 1, 2, 4, 8, 32, 64, 128   # include/hmmc_hip.h


def r16(x):
    """what one rounding of x to fp16 can move it by"""
    return U16 * x.abs() + SUB16


def within_ratio(got, ref, bound):
    """worst |got - ref| / (SLACK bound) over all elements (NaN -> inf)"""
    r = (got.to(D64) - ref).abs() / (SLACK * bound)
    return float(r.nan_to_num(float("inf")).max()) if r.numel() else 0.0


def detects(ref, slipped, bound):
    """the slip moves some element by more than the tolerance the family's test allows"""
    return bool(((slipped - ref).abs() > SLACK * bound).any())


# ============================================================================= attention

def key_tiles(L):
    """16-key tiles of the kernel template that takes L tokens: 2 / 4 (attention_f16.hip), ktl = 2 ceil(L / 32) above 64"""
    return 2 if L <= 32 else 4 if L <= 64 else 2 * ((L + 31) // 32)


def heads(t, nseq, L, H):
    """[nseq L, 64 H] -> [nseq, H, L, 64]"""
    return t.reshape(nseq, L, H, 64).transpose(1, 2)


def rows(t):
    """[nseq, H, L, 64] -> [nseq L, 64 H]"""
    n, H, L, _ = t.shape
    return t.transpose(1, 2).reshape(n * L, H * 64)


def split_qkv(qkv, nseq, L, H):
    D = H * 64
    return tuple(heads(qkv[:, i * D:(i + 1) * D], nseq, L, H) for i in range(3))


def key_mask(L, causal, device):
    """[L, L] True where query i does not see key j"""
    m = torch.zeros(L, L, dtype=torch.bool, device=device)
    return m | torch.ones(L, L, dtype=torch.bool, device=device).triu(1) if causal else m


def attention(qkv, nseq, L, H, causal):
    """softmax(Q K^T / 8 + mask) V per (sequence, head) on packed rows Q | K | V, head dim 64 (nn.MultiheadAttention's core,
    modules/module_clip.py:251 with the text mask of :441-447) -> (out [nseq L, 64 H], lse [nseq, H, L])."""
    q, k, v = split_qkv(qkv, nseq, L, H)
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(key_mask(L, causal, qkv.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return rows(torch.exp(s - lse.unsqueeze(-1)) @ v), lse


def attention_bwd(qkv, dout, nseq, L, H, causal):
    """d(sum(out o dout)) / d qkv by fp64 autograd"""
    x = qkv.detach().clone().requires_grad_()
    out, _ = attention(x, nseq, L, H, causal)
    out.backward(dout)
    return x.grad


def dbias_partial(dqkv, nseq, L):
    """per-sequence column sums of dqkv [nseq, 3 D]: the in-projection bias gradient's partial sums"""
    return dqkv.reshape(nseq, L, -1).sum(1)


def row_scaled(dqkv, rowstat):
    """hmmc_attention_f16_bwd_scaled: row r of dqkv times rowstat[r][0]"""
    return dqkv * rowstat[:, :1]


def attention_parts(qkv, dout, nseq, L, H, causal, slip=None, shift=1):
    """The same forward and backward written out (autograd's softmax backward dS = P o (dP - rowsum(P o dP))), so that the bounds
    can name the intermediates and test_slip_* can break one of them.  -> dict(out, lse, dqkv [, p, dP, delta, dS: per head]).
    slip: None, or the name of one plausible kernel mistake
      pad_key        the padded key L (the kernels read the clamped row L - 1 there) is not masked
      mask_last      key L - 1 is masked
      causal_edge    `key < qi` instead of `key <= qi` (query 0 keeps key 0)
      scale_tile     the 1/8 is missing on one 16-key tile (the second; the first when there is one)
      stale_pair     the (sequence, head) pair i holds the results of pair i - shift: a stale persistent-loop result
      delta_neighbour  delta taken from the next query
      lse_nomax      lse = log(sum exp(s - max)) without the max added back"""
    q, k, v = split_qkv(qkv, nseq, L, H)
    dO = heads(dout, nseq, L, H)
    dev = qkv.device
    mask = key_mask(L, causal, dev)
    if slip == "causal_edge":
        mask = torch.ones(L, L, dtype=torch.bool, device=dev).triu(0)
        mask[0, 0] = False
    if slip == "pad_key":                        # L + 1 keys: the last one a copy of row L - 1, seen by every query
        k, v = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
        mask = torch.cat([mask, torch.zeros(L, 1, dtype=torch.bool, device=dev)], 1)
    if slip == "mask_last" and L > 1:
        mask = mask.clone()
        mask[:, L - 1] = True
    s = (q @ k.transpose(-1, -2)) * 0.125
    if slip == "scale_tile":
        t0 = 16 if L > 16 else 0
        s[..., t0:t0 + 16] = s[..., t0:t0 + 16] * 8.0
    s = s.masked_fill(mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ v
    if slip == "lse_nomax":
        lse = lse - m.squeeze(-1)
    dP = dO @ v.transpose(-1, -2)
    delta = (p * dP).sum(-1, keepdim=True)
    if slip == "delta_neighbour":
        delta = delta.roll(-1, dims=2)
    dS = p * (dP - delta) * 0.125
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, p.transpose(-1, -2) @ dO
    if slip == "pad_key":                        # what reaches row L - 1 of dK / dV is its own share; the padded row's is dropped
        dk, dv, p, dP, dS = dk[:, :, :L], dv[:, :, :L], p[..., :L], dP[..., :L], dS[..., :L]
    res = dict(out=rows(o), lse=lse, dqkv=torch.cat([rows(dq), rows(dk), rows(dv)], 1), p=p, dP=dP, delta=delta, dS=dS)
    if slip == "stale_pair":
        def stale(t_pairs):                      # [nseq H, ...] in pair order
            out = t_pairs.clone()
            out[shift:] = t_pairs[:-shift]
            return out
        o_p = stale(o.reshape(nseq * H, L, 64)).reshape(nseq, H, L, 64)
        g_p = [stale(t.reshape(nseq * H, L, 64)).reshape(nseq, H, L, 64) for t in (dq, dk, dv)]
        res.update(out=rows(o_p), lse=stale(lse.reshape(nseq * H, L)).reshape(nseq, H, L),
                   dqkv=torch.cat([rows(t) for t in g_p], 1))
    return res


def attention_bounds(qkv, dout, nseq, L, H, causal, rowstat=None):
    """-> dict of bounds shaped like out, lse, dqkv, dbias (and scaled, with rowstat) of hmmc_attention_f16_fwd / _bwd /
    _bwd_scaled for the kernel that takes this L (module docstring).  The backward is held to the bound it has when it is given
    the forward kernel's own O and lse, each within its forward bound - what every caller passes."""
    long_ = L > 64
    kt = key_tiles(L)
    c = 4 * kt + 2                               # additions behind a softmax row's sum: 4 per key tile in a lane, two shuffles
    cm = 16 * kt                                 # MFMA terms of a product over the (padded) keys or queries
    r = attention_parts(qkv, dout, nseq, L, H, causal)
    q, k, v = split_qkv(qkv, nseq, L, H)
    dO = heads(dout, nseq, L, H)
    p, dP, delta, dS, lse = r["p"], r["dP"], r["delta"], r["dS"], r["lse"].unsqueeze(-1)
    mask = key_mask(L, causal, qkv.device)
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(mask, float("-inf"))
    es = (64 * U * 0.125 * (q.abs() @ k.abs().transpose(-1, -2)) + U * s.abs().masked_fill(mask, 0.0)).masked_fill(mask, 0.0)
    m = s.amax(-1, keepdim=True)
    t = (s - m).masked_fill(mask, 0.0)
    rel_e = (es + exp_rel(t)).masked_fill(mask, 0.0)
    avg = (p * rel_e).sum(-1, keepdim=True)
    b_lse = avg + c * U + 4 * U * lse.abs() + 4 * ((lse - m).abs() + 1.0) * U
    # forward: P as it enters P V (normalised before or after, the same to first order), O
    eP = p * (rel_e + avg + (c + 2) * U) + r16(p)
    o = p @ v
    e_o = eP @ v.abs() + cm * U * (p @ v.abs()) + 2 * U * o.abs()
    b_o = e_o + r16(o)
    # backward: P = exp2(s log2 e / 8 - lse log2 e) from the saved lse
    tb = (s - lse).masked_fill(mask, 0.0)
    ep = p * (es + b_lse + exp_rel(tb) + 2 * U * lse.abs())
    edP = 64 * U * (dO.abs() @ v.abs().transpose(-1, -2))
    if long_:                                    # <dO, fp16 O>: 8 terms in a lane, three shuffles
        edelta = (dO.abs() * b_o).sum(-1, keepdim=True) + 11 * U * (dO * o).abs().sum(-1, keepdim=True)
    else:
        edelta = (ep * dP.abs() + p * edP).sum(-1, keepdim=True) + c * U * (p * dP).abs().sum(-1, keepdim=True)
    edS = 0.125 * (ep * (dP - delta).abs() + p * (edP + edelta + U * (dP.abs() + delta.abs()))) + 2 * U * dS.abs() \
        + U16 * dS.abs() + SUB16
    eP16 = ep + r16(p)
    kT = lambda x: x.transpose(-1, -2)          # noqa: E731
    raw = [edS @ k.abs() + (cm + 2) * U * (dS.abs() @ k.abs()),
           kT(edS) @ q.abs() + (cm + 2) * U * (kT(dS.abs()) @ q.abs()),
           kT(eP16) @ dO.abs() + (cm + 2) * U * (kT(p) @ dO.abs())]
    raw = torch.cat([rows(x) for x in raw], 1)
    dqkv = r["dqkv"]
    b_dqkv = raw + r16(dqkv)
    out = dict(out=rows(b_o), lse=b_lse.squeeze(-1), dqkv=b_dqkv,
               dbias=dbias_partial(b_dqkv, nseq, L) + (kt + 14) * U * dbias_partial(dqkv.abs(), nseq, L))
    if rowstat is not None:
        f = rowstat[:, :1].abs()
        out["scaled"] = f * raw + 2 * U * f * dqkv.abs() + r16(f * dqkv)
    return out


def emulate_attention(qkv, dout, nseq, L, H, causal, rowstat=None):
    """The kernels' arithmetic in torch on the CPU: fp32 everywhere, .half() at the rounding points the module docstring names,
    the backward fed with the emulated forward's fp16 O and fp32 lse.  -> dict(out, lse, dqkv, dbias [, scaled])"""
    f32 = torch.float32
    LOG2E = 1.4426950408889634
    C1 = 0.125 * LOG2E
    q, k, v = (x.to(f32) for x in split_qkv(qkv, nseq, L, H))
    dO = heads(dout, nseq, L, H).to(f32)
    mask = key_mask(L, causal, qkv.device)
    raw_s = q @ k.transpose(-1, -2)
    if L > 64:
        sm = raw_s.masked_fill(mask, float("-inf"))
        m2 = sm.amax(-1, keepdim=True) * C1
        e = torch.exp2(sm * C1 - m2)
        tot = e.sum(-1, keepdim=True)
        lse = (m2 + torch.log2(tot)) * (1.0 / LOG2E)
        o16 = ((e.half().float() @ v) * (1.0 / tot)).half()
    else:
        sm = (raw_s * 0.125).masked_fill(mask, float("-inf"))
        m = sm.amax(-1, keepdim=True)
        e = torch.exp(sm - m)
        tot = e.sum(-1, keepdim=True)
        lse = m + torch.log(tot)
        o16 = ((e * (1.0 / tot)).half().float() @ v).half()
    pb = torch.exp2(raw_s * C1 - LOG2E * lse).masked_fill(mask, 0.0)
    dP = dO @ v.transpose(-1, -2)
    if L > 64:
        delta = (dO * o16.float()).sum(-1, keepdim=True)
        ds16 = (pb * (dP - delta)).half().float()
        dq, dk = (ds16 @ k) * 0.125, (ds16.transpose(-1, -2) @ q) * 0.125
    else:
        delta = (pb * dP).sum(-1, keepdim=True)
        ds16 = (pb * (dP - delta) * 0.125).half().float()
        dq, dk = ds16 @ k, ds16.transpose(-1, -2) @ q
    dv = pb.half().float().transpose(-1, -2) @ dO
    acc = torch.cat([rows(x) for x in (dq, dk, dv)], 1)
    res = dict(out=rows(o16), lse=lse.squeeze(-1), dqkv=acc.half(), dbias=dbias_partial(acc.half().float(), nseq, L))
    if rowstat is not None:
        res["scaled"] = (acc * rowstat[:, :1].to(f32)).half()
    return res


def attention_inputs(regime, nseq, L, H, causal, seed=0, device="cpu"):
    """fp16 (qkv [nseq L, 192 H], dout [nseq L, 64 H]) of one of the three input regimes of the GPU tests; every (sequence, head)
    pair has data of its own.
      flat        N(0, 1): logits of standard deviation near 1
      peaked      q = 4 k[w]: the logit of key w(query) is near 32 and the others N(0, 4^2), most rows are near one-hot.  w cycles
                  with the query through key 0, key L - 1 and a random key; causal: the diagonal (query L - 1 among them) and key 0
      structured  integer-valued v and dout (-4 .. 4) with random q, k: an error in P is not averaged away
    (generated on `device`: the large GPU shapes never cross the host)"""
    g = torch.Generator(device=device).manual_seed(1000 * seed + 7 * L + H + 3 * nseq + int(causal))
    D = 64 * H
    qkv = torch.randn(nseq * L, 3 * D, generator=g, device=device)
    dout = torch.randn(nseq * L, D, generator=g, device=device)
    if regime == "peaked":
        k = heads(qkv[:, D:2 * D], nseq, L, H)
        i = torch.arange(L, device=device)
        if causal:
            w = torch.where((L - 1 - i) % 2 == 0, i, torch.zeros_like(i))
        else:
            rnd = torch.randint(0, L, (L,), generator=g, device=device)
            w = torch.where(i % 3 == 0, torch.zeros_like(i), torch.where(i % 3 == 1, torch.full_like(i, L - 1), rnd))
        qkv[:, :D] = rows(4.0 * k[:, :, w])
    elif regime == "structured":
        qkv[:, 2 * D:] = torch.randint(-4, 5, (nseq * L, D), generator=g, device=device).float()
        dout = torch.randint(-4, 5, (nseq * L, D), generator=g, device=device).float()
    else:
        assert regime == "flat", regime
    return qkv.half(), dout.half()


ATTN_REGIMES = ("flat", "peaked", "structured")
ATTN_SLIPS = ("pad_key", "mask_last", "causal_edge", "scale_tile", "stale_pair", "delta_neighbour", "lse_nomax")


# ============================================================================= GEMM epilogues

def qgelu(h):
    """modules/module_clip.py:226-228"""
    return h * torch.sigmoid(1.702 * h)


def qgelu_grad(h, outer=1.702):
    """d QuickGELU / dh = s + 1.702 h s (1 - s), s = sigmoid(1.702 h); `outer`: the second 1.702 (test_slip_* drops it)"""
    s = torch.sigmoid(1.702 * h)
    return s + outer * h * s * (1.0 - s)


def h16(x):
    """fp16 rounding of an fp64 tensor, back in fp64"""
    return x.to(torch.float16).to(D64)


def gemm_epilogue(acc, bias, resid, aux_in, flags, rounded=False):
    """include/hmmc_hip.h's epilogue formulas on the accumulator acc [M, N] (fp64) -> (out, aux_out or None).
      BIAS h = acc + bias[n];  RESID out = resid + h;  QGELU out = QuickGELU(h), aux_out = h, with SAVE_DGELU QuickGELU'(h);
      DGELU out = acc QuickGELU'(aux_in);  MULAUX out = acc aux_in.
    rounded: with the fp16 roundings of the header (h = fp16(acc + bias), out = fp16(resid + h)) for BIAS / RESID - on integer
    data, where acc is exact, that is the result to the bit."""
    h = acc + bias if flags & EPI_BIAS else acc
    if rounded:
        assert not flags & (EPI_QGELU | EPI_DGELU | EPI_MULAUX)
        h = h16(h)
        return (h16(resid + h) if flags & EPI_RESID else h), None
    if flags & EPI_QGELU:
        return qgelu(h), (qgelu_grad(h) if flags & EPI_SAVE_DGELU else h)
    if flags & EPI_DGELU:
        return acc * qgelu_grad(aux_in), None
    if flags & EPI_MULAUX:
        return acc * aux_in, None
    if flags & EPI_RESID:
        return resid + h, None
    return h, None


def gemm_acc_bound(a_abs_b_abs, K):
    """K U sum_k |a_k b_k| from |A| |B|^T"""
    return K * U * a_abs_b_abs


def gemm_epilogue_bounds(acc, eacc, bias, resid, aux_in, flags):
    """-> (bound of out, bound of aux_out or None); eacc: the accumulator's bound (gemm_acc_bound)"""
    h = acc + bias if flags & EPI_BIAS else acc
    eh = eacc + U * h.abs() + r16(h)                                      # h = fp16(acc + bias)
    if flags & EPI_QGELU:
        t = 1.702 * h
        s = torch.sigmoid(t)
        et = 1.702 * eh + U * t.abs() + r16(t)                            # t = fp16(fp32(1.702 h))
        es32 = s * (1 - s) * et + (exp_rel(t) + 3 * U) * s * (1 - s) + 2 * U * s   # fp32 sigmoid(t): exp2, 1 +, rcp
        out = h * s
        b_out = s * eh + h.abs() * (es32 + r16(s)) + r16(out)             # s = fp16(.), out = fp16(h s)
        if not flags & EPI_SAVE_DGELU:
            return b_out, eh
        g = qgelu_grad(h)
        dg_ds = (1.0 + 1.702 * h * (1.0 - 2.0 * s)).abs()
        b_aux = dg_ds * es32 + 1.702 * s * (1 - s) * eh + 4 * U * (s + (1.702 * h * s * (1 - s)).abs()) + r16(g)
        return b_out, b_aux
    if flags & EPI_DGELU:
        x = aux_in
        s = torch.sigmoid(1.702 * x)
        es32 = (exp_rel(1.702 * x) + 3 * U) * s * (1 - s) + 2 * U * s
        g = qgelu_grad(x)
        eg = (1.0 + 1.702 * x * (1.0 - 2.0 * s)).abs() * es32 + 5 * U * (s + (1.702 * x * s * (1 - s)).abs())
        out = acc * g
        return eacc * g.abs() + acc.abs() * eg + U * out.abs() + r16(out), None
    if flags & EPI_MULAUX:
        out = acc * aux_in
        return eacc * aux_in.abs() + U * out.abs() + r16(out), None
    if flags & EPI_RESID:
        out = resid + h
        return eh + U * out.abs() + r16(out), None
    return eh, None


def emulate_gemm_epilogue(acc32, bias, resid, aux_in, flags):
    """gemm_f16.hip's epilogue_run in torch: acc32 the fp32 accumulator, bias / resid / aux_in fp16 -> (out, aux_out) fp16"""
    v = acc32 + bias.float() if flags & EPI_BIAS else acc32
    if flags & EPI_QGELU:
        h = v.half()
        p0 = 1.702 * h.float()
        t = p0.half()
        s = 1.0 / (1.0 + torch.exp2(t.float() * -1.4426950408889634))
        out = (h.double() * s.half().double()).half()                     # v_pk_mul_f16: the exact product, one rounding
        aux = (p0 * (1.0 - s) * s + s).half() if flags & EPI_SAVE_DGELU else h
        return out, aux
    if flags & EPI_DGELU:
        x = aux_in.float()
        s = 1.0 / (1.0 + torch.exp2(x * (-1.702 * 1.4426950408889634)))
        return (v * (1.702 * x * (1.0 - s) * s + s)).half(), None
    if flags & EPI_MULAUX:
        return (v * aux_in.float()).half(), None
    if flags & EPI_RESID:
        return (resid.float() + v.half().float()).half(), None
    return v.half(), None


def pick_big_tile(M, N, cus):
    """gemm_f16.hip's pick_cfg for a launch with an epilogue (no K split): the 256x256 tile when both dimensions are at least 256
    and each a multiple of 256 or at least 2048, and the 256x256 tiles number at least 3/4 of the CUs; else 128x128"""
    shaped = M >= 256 and N >= 256 and (M % 256 == 0 or M >= 2048) and (N % 256 == 0 or N >= 2048)
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    return shaped and tiles >= cus * 3 // 4


def colsum_blocks(c, block):
    """[ceil(M / block), N]: row r = the column sums of rows r block .. (r + 1) block - 1 of c, the ragged last block over its
    valid rows only"""
    M, N = c.shape
    nb = (M + block - 1) // block
    pad = torch.zeros(nb * block - M, N, dtype=c.dtype, device=c.device)
    return torch.cat([c, pad]).reshape(nb, block, N).sum(1)


def colsum_bound(c, block):
    """bound of every COLSUM partial row: block / 16 strips added in a lane, then a 16-lane tree of 4"""
    return (block // 16 + 4) * U * colsum_blocks(c.abs(), block)


# ============================================================================= weight gradients: fp32 split-K slabs + reduce

BKT = 64                      # rows of a K-tile (gemm_f16.hip)


def wgrad(dy, x):
    """dW[n][k] = sum_t dy[t][n] x[t][k]: F.linear's weight gradient (modules/module_clip.py:231-257), fp64"""
    return dy.t() @ x


def gemm_kk(a, b):
    """a [M, K] b [N, K]^T: the forward layout without an epilogue"""
    return a @ b.t()


def gemm_km(a, b):
    """a [M, K] b [K, N]: the data-gradient layout without an epilogue"""
    return a @ b


def as_wgrad(layout, a, b):
    """the operands of a kk / km / mm product as (dy [T, M], x [T, N]) with the reduction over the rows: every layout is then
    wgrad(dy, x), and the split, the slips and the emulation below are written once"""
    return {"mm": (a, b), "kk": (a.t(), b.t()), "km": (a.t(), b)}[layout]


def split_plan(T, s):
    """the host's split arithmetic (gemm_f16_one, group_plan) from the split count s the ABI reports for T reduction rows
    -> (nkt, ktps, splitk): K-tiles, K-tiles per split = ceil(nkt / s), splits that own at least one K-tile = ceil(nkt / ktps).
    The last split holds nkt - (splitk - 1) ktps K-tiles.  (Applying it to its own splitk gives the same ktps again.)"""
    nkt = (T + BKT - 1) // BKT
    ktps = (nkt + max(s, 1) - 1) // max(s, 1)
    return nkt, ktps, (nkt + ktps - 1) // ktps


def wgrad_bound(ref, abs_prod, T, ktps=None, slabs=1, half=True):
    """Bound of a product that leaves through the fp32 slabs.  The operands are exact fp16 and every product is exact in fp32; the
    accumulation error is c U sum_t |dy[t][n] x[t][k]| (abs_prod = |dy|^T |x|) with c the dependent fp32 additions behind an
    element: 64 per K-tile of a split (at most: the MFMA adds 32 terms per instruction), plus one per slab summed by the ordered
    reduce; c = T when the split is not known (ktps None: a T-term dot product).  half: the one rounding of the sum to fp16,
    r16(ref); the fp32 output dW32 is the reduce's sum itself and adds nothing.
    Two data regimes go with it, because on zero-mean data sum|ab| >> |sum ab| and the bound, dominated by r16(ref), cannot see a
    slab that was rounded to fp16: "signed" (Gaussian: cancellation exposes sign and index slips) and "same" (dy, x in [0.25, 1]:
    sum|ab| = |sum ab|, the fp32 bound is c U relative, far below U16).  The "exact" regime (small non-negative integers, every
    slab past 2048 and every sum below 2^24, wgrad_inputs) is the strict form: the fp32 path is exact there and the tests compare with torch.equal."""
    c = T if ktps is None else BKT * ktps + slabs
    b = c * U * abs_prod
    return b + r16(ref) if half else b


WGRAD_REGIMES = ("signed", "same")


def exact_top(T):
    """largest integer operand of the exact regime: the mean result (m / 2)^2 T stays at 40000 or below (the largest a few
    standard deviations higher, below 65504), which from T = 1000 on puts a 256-row split's partial, (m / 2)^2 256, past 2048;
    m^2 T < 2^24 keeps every fp32 sum exact whatever the data.  Integers 0 .. 3 would do for the reduce alone - the RUNNING sum
    passes 2048 - but a slab of 256 .. 448 rows would stay below 2048 and an fp16 slab would go unseen."""
    m = int(2.0 * (40000.0 / T) ** 0.5)
    assert m >= 3 and m * m * T < 2 ** 24, T
    return m


def wgrad_inputs(regime, T, dims, seed=0, device="cpu"):
    """fp16 ([dy_j [T, Np_j]], [x_j [T, Kp_j]]) for dims = [(Np_j, Kp_j)]; every problem has data of its own.
      signed  dy ~ N(0, 1), x ~ N(0, 1 / T): results of unit size
      same    dy, x in [0.25, 1] times a scale that keeps every T-term sum below 32768 (fp16 holds the result)
      exact   integers 0 .. m, m = exact_top(T): every partial sum is an integer below m^2 T < 2^24, so the fp32 path is exact; a
              split's partial alone passes 2048 (from 4 K-tiles per split on, what both host policies keep), where fp16 holds
              even numbers only, and the results stay near 40000, inside fp16's range"""
    g = torch.Generator(device=device).manual_seed(100 * seed + T + sum(n + 3 * k for n, k in dims))
    dys, xs = [], []
    for n, k in dims:
        if regime == "signed":
            dy, x = torch.randn(T, n, generator=g, device=device), torch.randn(T, k, generator=g, device=device) / T ** 0.5
        elif regime == "same":
            sc = min(1.0, (32768.0 / T) ** 0.5)
            dy = (0.25 + 0.75 * torch.rand(T, n, generator=g, device=device)) * sc
            x = (0.25 + 0.75 * torch.rand(T, k, generator=g, device=device)) * sc
        else:
            assert regime == "exact", regime
            m = exact_top(T)
            dy = torch.randint(0, m + 1, (T, n), generator=g, device=device).float()
            x = torch.randint(0, m + 1, (T, k), generator=g, device=device).float()
        dys.append(dy.half())
        xs.append(x.half())
    return dys, xs


def wgrad_partials(dy, x, ktps):
    """[splitk, N, K]: split s sums the rows 64 ktps s .. 64 ktps (s + 1) - 1 (the last one what is left of T)"""
    rows = BKT * ktps
    return torch.stack([dy[r:r + rows].t() @ x[r:r + rows] for r in range(0, dy.shape[0], rows)])


WGRAD_SLIPS = ("slab_f16", "reduce_f16", "split_dropped", "split_twice", "tail_rows", "acc_not_cleared")
WGRAD_GROUP_SLIPS = WGRAD_SLIPS + ("problem_swapped",)


def wgrad_slipped(dy, x, ktps, slip, tile=128):
    """wgrad(dy, x) in fp64 through the slabs with one plausible mistake (dy, x fp64; returned before the final fp16 rounding):
      slab_f16         each split's partial rounded to fp16 before the reduce
      reduce_f16       the running sum rounded to fp16 between splits
      split_dropped    the last, shorter split is missing
      split_twice      one split counted twice, as with a stale slab
      tail_rows        the rows T .. 64 nkt - 1 behind the operands are not treated as zero (here they repeat rows 0 ..)
      acc_not_cleared  an item starts from the previous item's accumulator: the output tile to the right of (or, in a single column
                       of tiles, below) a tile also holds that tile's partial of the first split"""
    parts = wgrad_partials(dy, x, ktps)
    if slip == "slab_f16":
        return h16(parts).sum(0)
    if slip == "reduce_f16":
        run = parts[0]
        for p in parts[1:]:
            run = h16(run + p)
        return run
    if slip == "split_dropped":
        return parts[:-1].sum(0)
    if slip == "split_twice":
        return parts.sum(0) + parts[0]
    if slip == "tail_rows":
        n = -dy.shape[0] % BKT
        return parts.sum(0) + dy[:n].t() @ x[:n]
    assert slip == "acc_not_cleared", slip
    out = parts.sum(0)
    if out.shape[1] > tile:
        out[:, tile:] += parts[0][:, :-tile]
    elif out.shape[0] > tile:
        out[tile:] += parts[0][:-tile]
    else:
        out += parts[0]
    return out


def wgrad_group_swapped(dys, xs, ktps):
    """problem_swapped: the grouped reduce of problem j reads from problem j - 1's slab offset (problem 0 is right).  The slabs
    lie as [problem][split][Np_j Kp_j]; the reduce adds element e of its problem at offset + split Np_j Kp_j + e."""
    parts = [wgrad_partials(dy, x, ktps) for dy, x in zip(dys, xs)]
    flat = torch.cat([p.reshape(-1) for p in parts])
    offs, o = [], 0
    for p in parts:
        offs.append(o)
        o += p.numel()
    outs = []
    for j, p in enumerate(parts):
        S, n, k = p.shape
        off = offs[max(j - 1, 0)]
        outs.append(flat[off:off + S * n * k].reshape(S, n, k).sum(0))
    return outs


def emulate_splitk(dy, x, ktps, half=True):
    """gemm_f16.hip's slab path in torch: per split an fp32 accumulator that takes the K-tiles in order, 32 rows per MFMA
    instruction; the reduce adds the slabs in split order in fp32; one rounding to fp16 (half) or none (dW32)"""
    df, xf = dy.float(), x.float()
    T, rows, total = dy.shape[0], BKT * ktps, None
    for r0 in range(0, T, rows):
        acc = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float32, device=dy.device)
        for r in range(r0, min(T, r0 + rows), 32):
            acc += df[r:r + 32].t() @ xf[r:r + 32]
        total = acc if total is None else total + acc
    return total.half() if half else total


# the shapes tests/test_gpu_hotpath.py runs and tests/test_hotpath_reference.py emulates.  Single launches (M, N, K) in the
# weight-gradient layout; the path each reaches on 256 CUs is named in test_gpu_hotpath.py
WGRAD_MM_CASES = [(136, 264, 8), (136, 264, 100), (136, 264, 1000), (136, 264, 1001), (136, 264, 2120), (1024, 1024, 6152)]
WGRAD_KX_CASES = [("kk", 128, 128, 2048), ("km", 128, 128, 2048)]
WGRAD_LAYER = [(256, 1024), (1024, 256), (256, 256), (768, 256)]         # c_proj, c_fc, out_proj, in_proj at D = 256
# grouped launches: name -> (dims, T, which problems leave as fp32 dW32)
WGRAD_GROUP_CASES = {
    "min_f16": ([(256, 256)], 512, ()),
    "two_f32": ([(256, 256), (512, 256)], 520, (0, 1)),
    "three_mix": (WGRAD_LAYER[:3], 1000, (1,)),
    "layer_f16": (WGRAD_LAYER, 512, ()),
    "layer_f32": (WGRAD_LAYER, 1001, (0, 1, 2, 3)),
    "layer_mix": (WGRAD_LAYER, 2120, (1, 3)),
    "wide_mix": ([(1024, 1280)] * 4, 512, (1, 3)),
    "wide_1k_mix": ([(1024, 1280)] * 4, 1024, (1, 3)),
}


# ============================================================================= LayerNorm

def layernorm(x, gamma, beta, eps, unbiased=False, mean_shift=0):
    """(x - mean) / sqrt(var + eps) gamma + beta over the last dim, biased variance (modules/module_clip.py:217-223,
    until_module.py:54-67) -> (y, mean [rows], rstd [rows]).  unbiased / mean_shift: the mistakes of test_slip_*."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / (D - 1 if unbiased else D)
    if mean_shift:
        mean = mean.roll(mean_shift, 0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(x, gamma, beta, eps, dy, dres=None):
    """fp64 autograd of layernorm -> (dx [+ dres], dgamma, dbeta)"""
    xr, gr, br = (t.detach().clone().requires_grad_() for t in (x, gamma, beta))
    layernorm(xr, gr, br, eps)[0].backward(dy)
    return (xr.grad + dres if dres is not None else xr.grad), gr.grad, br.grad


def ln_chain(D):
    return math.ceil(D / 64) + 6                 # a lane's elements, then the 6-level butterfly


def ln_row_chain(nrows):
    """additions behind a column sum over the rows: a wave's rows, the 4 waves of a block, the reduce's row lanes and its
    32-term merge (norm_elem.hip; up to 4096 rows a block takes 8 of them)"""
    nb = max(1, (nrows + 7) // 8)
    return math.ceil(nrows / (4 * nb)) + 4 + math.ceil(nb / 32) + 32


def layernorm_bounds(x, gamma, beta, eps, dy, dres, half):
    """-> dict(y, mean, rstd, dx, dgamma, dbeta, dxsum).  The backward reads the forward kernel's mean and rstd (each within its
    bound).  half: fp16 rows (y, dx and the dx column sums are rounded to fp16)."""
    D = x.shape[-1]
    c = ln_chain(D)
    y, mean, rstd = layernorm(x, gamma, beta, eps)
    mean, rstd = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    em = c * U * x.abs().sum(-1, keepdim=True) / D + U * mean.abs()
    d = x - mean
    ed = em + U * d.abs()
    var = (d * d).sum(-1, keepdim=True) / D
    ev = (2 * d.abs() * ed).sum(-1, keepdim=True) / D + em * em + (c + 3) * U * var
    erstd = rstd * (ev / (2 * (var + eps)) + U * eps / (var + eps) + 3 * U)
    xh = d * rstd
    exh = rstd * ed + d.abs() * erstd + 2 * U * xh.abs()
    b_y = gamma.abs() * exh + 2 * U * (xh * gamma).abs() + U * y.abs()
    g = dy * gamma
    s1 = g.sum(-1, keepdim=True) / D
    s2 = (g * xh).sum(-1, keepdim=True) / D
    es1 = (c + 2) * U * g.abs().sum(-1, keepdim=True) / D
    es2 = (c + 3) * U * (g * xh).abs().sum(-1, keepdim=True) / D + (g.abs() * exh).sum(-1, keepdim=True) / D
    inner = g - s1 - xh * s2
    dx = rstd * inner
    b_dx = erstd * inner.abs() + rstd * (es1 + exh * s2.abs() + xh.abs() * es2 + 3 * U * (g.abs() + s1.abs() + (xh * s2).abs())) \
        + 2 * U * dx.abs()
    if dres is not None:
        dx = dx + dres
        b_dx = b_dx + U * dx.abs()
    if half:
        b_y, b_dx = b_y + r16(y), b_dx + r16(dx)
    cr = ln_row_chain(x.shape[0])
    b_dg = (dy.abs() * exh).sum(0) + (cr + 1) * U * (dy * xh).abs().sum(0)
    b_db = cr * U * dy.abs().sum(0)
    b_sum = b_dx.sum(0) + cr * U * dx.abs().sum(0)
    if half:
        b_sum = b_sum + r16(dx.sum(0))
    return dict(y=b_y, mean=em.squeeze(-1), rstd=erstd.squeeze(-1), dx=b_dx, dgamma=b_dg, dbeta=b_db, dxsum=b_sum)


def emulate_layernorm(x, gamma, beta, eps, dy, dres):
    """norm_elem.hip's arithmetic in fp32 torch; x / dy / dres fp16 or fp32 (the I/O type) -> dict as layernorm_bounds"""
    T = x.dtype
    D = x.shape[-1]
    xf, eps32 = x.float(), torch.tensor(eps, dtype=torch.float32)
    mean = xf.sum(-1, keepdim=True) / D
    d = xf - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / D + eps32)
    y = (d * rstd * gamma + beta).to(T)
    xh = d * rstd
    g = dy.float() * gamma
    s1, s2 = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
    dx = rstd * (g - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres.float()
    dx = dx.to(T)
    return dict(y=y, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), dx=dx, dgamma=(dy.float() * xh).sum(0), dbeta=dy.float().sum(0),
                dxsum=dx.float().sum(0).to(T))


LN_REGIMES = ("normal", "offset", "constant", "outlier")


def layernorm_inputs(regime, nrows, D, dtype, seed=0, device="cpu"):
    """(x, gamma, beta, dy, dres) of one of the four row regimes of the GPU tests; x / dy / dres in the I/O dtype
      normal    N(0, 1)
      offset    a large common offset: mean 50, standard deviation 0.5
      constant  every second row (the first one included) is constant, each at a value of its own that fp32 sums exactly:
                variance exactly 0, rstd = 1 / sqrt(eps), y = beta; the other rows are N(0, 1)
      outlier   row 0 is 1000 times larger than the rest"""
    g = torch.Generator().manual_seed(100 * seed + D + nrows)
    x = torch.randn(nrows, D, generator=g)
    if regime == "offset":
        x = 50.0 + 0.5 * x
    elif regime == "constant":
        vals = (torch.arange(nrows) % 13 - 6).float() * 0.25 + 0.125
        x[0::2] = vals[0::2, None]
    elif regime == "outlier":
        x[0] *= 1000.0
    else:
        assert regime == "normal", regime
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy, dres = torch.randn(nrows, D, generator=g), torch.randn(nrows, D, generator=g)
    return x.to(dtype).to(device), gamma.to(device), beta.to(device), dy.to(dtype).to(device), dres.to(dtype).to(device)
