"""CPU check of the fp64 statements in tests/heads_ref.py against the oracle (itself pinned to goldens produced by the
reference, tests/test_oracle_golden.py): the GPU tests of the fp32 heads, MoCo / BatchNorm and optimizer kernels
(tests/test_gpu_heads.py) compare with these statements, so they inherit the reference's semantics."""
import math

import pytest
import torch
import torch.nn.functional as F

import heads_ref as R
from oracle import hmmc_oracle as O

D64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed), dtype=D64)


def assert_close(a, b, tol, what):
    err = float((a - b).abs().max())
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("B,F_", [(1, 0), (5, 0), (5, 3), (9, 1)])
def test_infonce_is_finetune_head(B, F_):
    """hierarchical InfoNCE on the stacked S_all = 100 n(q) [n(v); n(u)]^T with w_video = w_vtm, w_frame = w_ftm / F is
    finetune_head (modules/modeling.py:702-709); with F = 0 it is w_vtm (CrossEn(S) + CrossEn(S^T))."""
    q, v, fr = randn(B, 16, seed=1), randn(B, 16, seed=2), randn(B, max(F_, 1), 16, seed=3)[:, :F_]
    keys = torch.cat([R.l2norm(v), R.l2norm(fr.reshape(B * F_, 16))]) if F_ else R.l2norm(v)
    S = 100.0 * R.l2norm(q) @ keys.t()
    loss, lse_row, lse_col = R.infonce(S, B, F_, 0.85, 0.15 / F_ if F_ else 0.0)
    ref = O.finetune_head(q, v, fr, 0.85, 0.15, use_frame_fea=bool(F_))
    assert_close(loss, ref, 1e-12, "loss vs finetune_head")
    sv = 100.0 * R.l2norm(q) @ R.l2norm(v).t()
    assert_close(R.infonce(sv, B, 0, 1.0, 0.0)[0], O.cross_en(sv) + O.cross_en(sv.t()), 1e-12, "CrossEn(S) + CrossEn(S^T)")
    assert_close(lse_row[:, 0], torch.logsumexp(sv, dim=1), 1e-12, "row LSE of the video block")
    assert_close(lse_col[:B], torch.logsumexp(sv, dim=0), 1e-12, "column LSE of the video block")


def test_topk_mean_is_eval_scores():
    bq, bv, Fr, E = 3, 4, 6, 8
    q, v, fr = randn(bq, E, seed=4), randn(bv, E, seed=5), randn(bv, Fr, E, seed=6)
    sv, sf = O.eval_scores(q, v, fr, 2)
    mine = R.topk_mean(O.loose_similarity(q, fr).reshape(bq, bv * Fr), bq, bv, Fr, 2)
    assert_close(mine, sf, 1e-12, "top-k frame mean")
    wide = torch.zeros(bq, bv * Fr + 5, dtype=D64)                  # the strided form: rows lds apart, base rows ldb apart
    wide[:, :bv * Fr] = O.loose_similarity(q, fr).reshape(bq, bv * Fr)
    base = torch.zeros(bq, bv + 3, dtype=D64)
    base[:, :bv] = sv
    assert_close(R.topk_mean(wide, bq, bv, Fr, 2, base=base, lds=bv * Fr + 5, ldb=bv + 3), sv + sf, 1e-12, "strided")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L,H", [(4, 8), (13, 2)])
def test_attention_is_mha(L, H, causal):
    """attention() on in-projected rows, then the out-projection, is the oracle's nn.MultiheadAttention (head dim 64).  The
    oracle evaluates the softmax in fp32 (.float()), hence 1e-6 on O(1) outputs."""
    b, D = 2, H * 64
    x = randn(b, L, D, seed=7) * 0.5
    in_w, in_b = randn(3 * D, D, seed=8) / math.sqrt(D), randn(3 * D, seed=9) * 0.1
    out_w, out_b = randn(D, D, seed=10) / math.sqrt(D), randn(D, seed=11) * 0.1
    qkv = F.linear(x, in_w, in_b).reshape(b * L, 3 * D)
    o, p = R.attention(qkv, b, L, H, causal)
    ref = O.mha(x, in_w, in_b, out_w, out_b, H, O.causal_mask(L) if causal else None)
    assert_close(F.linear(o, out_w, out_b).reshape(b, L, D), ref, 1e-6, "attention vs mha")
    assert_close(p.sum(-1), torch.ones(b, H, L, dtype=D64), 1e-12, "probabilities sum to one")
    if causal:
        assert float(p.triu(1).abs().max()) == 0.0


def test_bn_relu_is_mlp_forward():
    M, K, N = 37, 12, 20
    x = randn(M, K, seed=12)
    sd = {"p.linear_hidden.1.weight": randn(N, K, seed=13), "p.linear_hidden.1.bias": randn(N, seed=14),
          "p.linear_hidden.2.weight": randn(N, seed=15), "p.linear_hidden.2.bias": randn(N, seed=16),
          "p.linear_out.weight": randn(5, N, seed=17), "p.linear_out.bias": randn(5, seed=18)}
    y, mean, var_unbiased = O.mlp_forward(x, sd, "p.")
    h = F.linear(x, sd["p.linear_hidden.1.weight"], sd["p.linear_hidden.1.bias"])
    a, m, v = R.bn_relu(h, sd["p.linear_hidden.2.weight"], sd["p.linear_hidden.2.bias"], 1e-5)
    assert_close(F.linear(a, sd["p.linear_out.weight"], sd["p.linear_out.bias"]), y, 1e-12, "MLP output")
    assert_close(m, mean, 1e-12, "batch mean")
    rm, rv = R.bn_running(torch.zeros(N, dtype=D64), torch.ones(N, dtype=D64), m, v, M, 1.0)
    assert_close(rv, var_unbiased, 1e-12, "unbiased variance of the running statistics")
    bn = torch.nn.BatchNorm1d(N, momentum=0.1).double().train()     # and the running statistics of nn.BatchNorm1d
    bn(h)
    rm, rv = R.bn_running(torch.zeros(N, dtype=D64), torch.ones(N, dtype=D64), m, v, M, 0.1)
    assert_close(bn.running_mean, rm, 1e-12, "running mean")
    assert_close(bn.running_var, rv, 1e-12, "running var")


def test_moco_loss_is_contrastive_loss():
    Rr, E, Kq = 6, 16, 40
    q, k, queue = randn(Rr, E, seed=19), randn(Rr, E, seed=20), R.l2norm(randn(Kq, E, seed=21)).t().contiguous()
    qn, kn = F.normalize(q, dim=1), F.normalize(k, dim=1)
    loss, _ = R.moco_loss(qn @ queue, (qn * kn).sum(1), 0.07, 1.0 / Rr)
    assert_close(loss, O.contrastive_loss(q, k, queue, 0.07), 1e-12, "contrastive_loss")


def test_gelu_erf_and_ce():
    x = torch.linspace(-12, 12, 97, dtype=D64)
    assert_close(R.gelu_erf(x), O.gelu_erf(x), 0.0, "gelu_erf")
    logits, labels = randn(6, 11, seed=22), torch.tensor([0, 10, -100, 3, -1, 7])
    s, _, n = R.ce_sum(logits, labels)
    keep = labels >= 0
    assert n == 4
    assert_close(s / n, F.cross_entropy(logits[keep], labels[keep], ignore_index=-100), 1e-12, "cross entropy")


def test_enqueue_is_oracle_enqueue():
    E, W, Rr = 8, 12, 3
    keys = randn(Rr, E, seed=23)
    keys[1] = 0.0
    names = ("queue_v_cross_ng", "queue_tag_cross_ng", "queue_title_cross_ng", "queue_frame_proj_ng", "queue_frame_cross_ng")
    qs = {n: torch.zeros(E, W * (2 if "frame" in n else 1), dtype=D64) for n in names}
    O.enqueue(qs, W - Rr, keys, keys, keys, keys.reshape(Rr, 1, E).repeat(1, 2, 1), keys.reshape(Rr, 1, E).repeat(1, 2, 1), W)
    assert torch.equal(R.enqueue(keys, torch.zeros(E, W, dtype=D64), W - Rr), qs["queue_v_cross_ng"])


@pytest.mark.parametrize("wd,gscale", [(0.2, 0.01), (0.0, 3.0)])
def test_bert_adam_step_is_oracle(wd, gscale):
    """the plain statement against the oracle's op-by-op fp32 one, per-parameter clip inactive (gscale 0.01) and active (3.0):
    agreement to fp32 rounding: the fp32 scalars b1, b2, 1 - b2 and four roundings per step, three steps (1e-6 relative on the
    moments); the weights round to fp32 once per step (3 U |p|) on top of 2e-8 absolute."""
    n, lr, t_total, warm = 300, 1e-3, 20, 0.1
    p, m, v = randn(n, seed=24).float(), torch.zeros(n), torch.zeros(n)
    P, Mm, V = p.double(), m.double(), v.double()
    for step in range(3):
        g = randn(n, seed=30 + step).float() * gscale
        p, m, v, gc = O.bert_adam_step(p, g, m, v, step, lr, t_total, warm, wd)
        lr_t = lr * O.warmup_cosine(step / t_total, warm)
        P, Mm, V, G = R.bert_adam_step(P, g.double(), Mm, V, lr_t, wd)
        assert_close(gc.double(), G, 1e-6 * float(G.abs().max()), "clipped gradient")
        assert_close(m.double(), Mm, 1e-6 * float(Mm.abs().max()), "m")
        assert_close(v.double(), V, 1e-6 * float(V.abs().max()), "v")
        assert_close(p.double(), P, 2e-8 + 3 * R.U * float(P.abs().max()), "p")


def test_bert_adam_and_ema_ragged_sizes_on_the_cpu():
    """clip_grad_norm() and the EMA statement against torch.nn.utils.clip_grad_norm_ / momentum_update."""
    gs = [randn(n, seed=40 + n % 7) for n in (1, 7, 300)]
    total, clipped = R.clip_grad_norm(gs, 0.5)
    ref = [g.clone() for g in gs]
    ps =[torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, ref):
        p.grad = g
    tn = torch.nn.utils.clip_grad_norm_(ps, 0.5)
    assert abs(float(tn) - total) < 1e-12
    for p, c in zip(ps, clipped):
        assert_close(p.grad, c, 1e-12, "clipped")
    a, b = randn(50, seed=50), randn(50, seed=51)
    assert_close(O.momentum_update(a, b, 0.99), 0.99 * a + 0.01 * b, 1e-15, "EMA")


# ----------------------------------------------------------------------------- sensitivity of the GPU tests' tolerances
# Each family of tests/test_gpu_heads.py has one check here: a plausible slip of its kernel (a dropped row, column block,
# chunk or frame, swapped weights), applied to the fp64 statement, must move some element by more than SLACK times the
# rounding bound that family's GPU test allows.  Computed on the CPU from the same heads_ref bounds.

EPS, T = 1e-5, 0.07
U = R.U


def test_slip_infonce():
    B, F_ = 65, 12
    wf = 0.15 / F_ * 1.37                                      # w_frame != w_video, as in the GPU test
    q = R.l2norm(randn(B, 64, seed=3))                          # 100 * cosine of real normalised vectors
    S = (100.0 * q @ R.l2norm(randn(B * (1 + F_), 64, seed=4) + 0.5 * q.repeat_interleave(1 + F_, 0)).t()).float().double()
    loss, lse_row, lse_col = R.infonce(S, B, F_, 0.85, wf)
    b_loss, b_row, b_col, _ = R.infonce_bounds(S, B, F_, 0.85, wf, 1.0)
    assert R.detects(loss, R.infonce(S, B, F_, wf, 0.85)[0], b_loss), "w_video / w_frame swapped"
    assert R.detects(lse_col, torch.logsumexp(S[:-1], dim=0), b_col), "last row dropped from the column LSE"
    assert R.detects(lse_col, torch.logsumexp(S[:-8], dim=0), b_col), "last row lane block dropped"
    assert R.detects(lse_row[:, 1], torch.logsumexp(S[:, B:B + (B - 1) * F_:F_], dim=1), b_row[:, 1]), "last video of a block dropped"
    assert R.detects(lse_row[:, -1], lse_row[:, -2], b_row[:, -1]), "one frame fewer"


def test_slip_topk():
    Sf = torch.randint(-8, 9, (5, 7 * 12), generator=gen(1)).double() / 4
    ref = R.topk_mean(Sf, 5, 7, 12, 3)
    bound = U * 2 * ref.abs()
    assert R.detects(ref, R.topk_mean(Sf.view(5, 7, 12)[:, :, :11].reshape(5, 77), 5, 7, 11, 3), bound), "one frame fewer"
    assert R.detects(ref, R.topk_mean(Sf, 5, 7, 12, 2), bound), "k - 1 values"


def test_slip_segment_max():
    S = randn(17, 50, seed=8).double()
    ref = R.segment_max(S, [0, 1, 6, 13, 17])
    assert not torch.equal(ref, R.segment_max(S, [0, 1, 6, 12, 17])), "a segment ending one row early"


def test_slip_l2norm():
    D = 260
    x = randn(9, D, seed=9).double()
    dy = randn(9, D, seed=10).double()
    b_y, _, _ = R.l2norm_bounds(x, dy, 0.0, D)
    assert R.detects(R.l2norm(x), x / x[:, :256].norm(dim=1, keepdim=True), b_y), "the last f4 step of a row dropped"


def test_slip_temporal_pool():
    b, F_, D = 3, 12, 512
    h = randn(b * F_, D, seed=11).double()
    dout = randn(b, D, seed=12).double()
    ref = R.temporal_pool(h, None, b, F_, D)
    b_out, _ = R.pool_bounds(h, None, dout, b, F_, D)
    fewer = R.temporal_pool(h.view(b, F_, D)[:, :-1].reshape(-1, D), None, b, F_ - 1, D)
    assert R.detects(ref, fewer, b_out), "one frame fewer"


def test_slip_attention():
    b, L, H = 2, 24, 1
    qkv = randn(b * L, 3 * 64, seed=15).double() * 1.5
    dout = randn(b * L, 64, seed=16).double()
    o, p = R.attention(qkv, b, L, H, False)
    b_o, b_p, _ = R.attention_bounds(qkv, dout, b, L, H, False)
    short = qkv.view(b, L, 192)[:, :-1].reshape(-1, 192)
    o_s, p_s = R.attention(short, b, L - 1, H, False)
    assert R.detects(p[..., :-1, :-1], p_s, b_p[..., :-1, :-1]), "the last key dropped"
    assert R.detects(o.view(b, L, 64)[:, :-1], o_s.view(b, L - 1, 64), b_o.view(b, L, 64)[:, :-1]), "the last key dropped (out)"
    _, p_c = R.attention(qkv, b, L, H, True)
    assert R.detects(p, p_c, b_p), "causal mask applied / not applied"


def test_slip_batchnorm():
    M, N = 40000, 4
    h = torch.randint(-8, 9, (M, N), generator=gen(2)).double()
    gamma = torch.ones(N, dtype=D64)
    fb = R.bn_fwd_bounds(h, gamma, M, 0.1, torch.zeros(N, dtype=D64), torch.ones(N, dtype=D64), EPS)
    rpb = (M + 255) // 256                                     # rows of a slab at the 256-slab cap
    assert h.sum(0).ne(h[:-1].sum(0)).any(), "the last row dropped from the (exact) column sums"
    assert R.detects(fb["mean"], h[:-rpb].sum(0) / M, fb["em"]), "the last slab dropped"
    assert R.detects(fb["rstd"], 1 / torch.sqrt(h[:-rpb].var(0, unbiased=False) + EPS), fb["erstd"]), "the last slab dropped (rstd)"


def test_slip_moco():
    S = torch.rand(5, 257, generator=gen(3)).double() * 1.6 - 0.8
    lp = torch.tensor([0.95, -0.95, 0.95, -0.95, 0.95], dtype=D64)
    loss, lse = R.moco_loss(S, lp, T, 0.37)
    e_lse, b_loss, _, _ = R.moco_bounds(S, lp, 257, 5, 0.37, 1.0, T)
    assert R.detects(lse, R.moco_loss(S[:, :-1], lp, T, 0.37)[1], e_lse), "the last negative dropped"
    assert R.detects(lse, torch.logsumexp(S / T, 1), e_lse), "lpos left out of the LSE"
    a, b = randn(5, 100, seed=5), randn(5, 100, seed=6)
    assert R.detects((a * b).sum(1), (a[:, :-1] * b[:, :-1]).sum(1), (2 + 6) * U * (a * b).abs().sum(1)), "rowdot: last column"


def test_slip_cross_entropy():
    lg = randn(4, 49408, seed=7) * 3
    e = R.lse_bound(lg, 1, math.ceil(49408 / 256) + 11)
    assert R.detects(torch.logsumexp(lg, 1), torch.logsumexp(lg[:, :-256], 1), e), "the last 256-column step dropped"


def test_slip_gelu():
    x = torch.linspace(-12, 12, 2401, dtype=D64)
    dy = torch.ones_like(x)
    b_y, _ = R.gelu_bounds(x, dy)
    tanh_form = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    assert R.detects(R.gelu_erf(x), tanh_form, b_y), "the tanh approximation instead of erf"


def test_slip_enqueue():
    keys = randn(5, 100, seed=8)
    q = torch.zeros(100, 37, dtype=D64)
    ref = R.enqueue(keys, q, 32)
    assert not torch.equal(ref, R.enqueue(keys[:-1], q, 32)), "the last key not written"


def test_slip_optimizer():
    g = torch.randn(40000, generator=gen(4), dtype=D64)
    total = float(g.norm())
    rel = R.clip_rel(40000, 1)
    assert abs(float(g[:32768].norm()) - total) > R.SLACK * rel * total, "the last chunk missing from a norm"
