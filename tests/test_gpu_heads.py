"""GPU tests of the fp32 head (heads_f32.hip), pre-training (moco.hip) and multi-tensor optimizer (optim.hip) kernels, each
called with its own inputs through hmmc_amd.ops / optimization and compared with a plain fp64 statement of the same op
(tests/heads_ref.py, pinned to the oracle by tests/test_heads_reference.py), at the shapes where their fixed structure has an
edge: 64-lane strides, 8 row lanes x 32 columns, one-block reductions, the LDS budget of the short attention kernel at F = 64,
the 256-slab cap of the BatchNorm sums, the clip's switch above 4096 tensors, tensors of more than 64 chunks.

Tolerances are the first-order fp32 rounding bounds of each kernel's arithmetic (heads_ref: U = 2^-24 per operation, chains of
dependent additions, __expf / __logf), computed per element from the fp64 reference and allowed SLACK = 2 times; where the
arithmetic is exact (integer data, one add, a copy, a max) the comparison is exact; a NaN fails every comparison.  Every family
has a sensitivity self-check (tests/test_heads_reference.py, test_slip_*, CPU only): a plausible indexing slip, applied to the
fp64 reference, must fall outside the bound that family uses here.

Entry points and the test that reaches each (through hmmc_amd.ops, clip_grad_norm_ / BertAdam / _momentum_update for the
multi-tensor kernels, or the C-ABI itself where nothing in the package calls it):
  heads_f32.hip  l2norm_fwd/bwd: test_l2norm_fwd_bwd;  infonce_fwd/bwd: test_infonce_fwd_bwd;  topk_mean: test_topk_mean*;
                 segment_max: test_segment_max;  temporal_pool_fwd/bwd: test_temporal_pool_*;  add_rowbias: test_add_rowbias_exact;
                 temporal_attention_fwd/bwd: test_attention_f32_*;  retrieval_rank: test_gpu_kernels.py
  moco.hip       bn_workspace, bn_stats, bn_finalize, bn_apply_relu, bn_bwd_reduce/apply: test_batchnorm*;  rowdot, row_axpy:
                 test_rowdot_row_axpy;  moco_loss_fwd/bwd: test_moco_loss;  gelu_erf_fwd/bwd: test_gelu_erf;  ce_fwd/bwd:
                 test_cross_entropy
  optim.hip      mt_sumsq, mt_clip_grad_norm: test_mt_sumsq_and_plain_clip_through_the_abi;  mt_clip_grad_norm_keep:
                 test_clip_*;  mt_bertadam, mt_bertadam_ext (BertAdam.step): test_bertadam_*;  mt_ema (_momentum_update): test_ema_ragged_sizes_vs_oracle;
                 mt_chunk_elems: every table;  enqueue: test_enqueue_last_columns_and_zero_key"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import heads_ref as R  # noqa: E402
from hmmc_amd import ops  # noqa: E402
from hmmc_amd import functional as Fn  # noqa: E402
from hmmc_amd._lib import call, ptr  # noqa: E402
from oracle import hmmc_oracle as O  # noqa: E402

DEV = "cuda"
U = R.U
D64 = torch.float64


def gen(seed, device=DEV):
    return torch.Generator(device=device).manual_seed(seed)


def randn(*shape, seed=0, device=DEV):
    return torch.randn(*shape, generator=gen(seed, device), device=device)


def within(got, ref, bound, what):
    """|got - ref| <= SLACK * bound elementwise (infinities must match exactly; a NaN anywhere - in the result, the reference or
    the bound - fails: every comparison with NaN is false, so the check is written as `not (err <= lim)`)."""
    got = got.detach().to(D64).to(ref.device)
    ref = ref.detach().to(D64)
    nan = torch.isnan(got)
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} of {got.numel()} elements are NaN"
    assert not bool(torch.isnan(ref).any()), f"{what}: NaN in the fp64 reference"
    inf = torch.isinf(ref) | torch.isinf(got)
    assert torch.equal(got[inf], ref[inf]), f"{what}: infinities differ"
    err = (got - ref).abs().masked_fill(inf, 0.0)
    lim = torch.as_tensor(R.SLACK * bound, dtype=D64, device=err.device).expand_as(err).masked_fill(inf, 0.0)
    bad = ~(err <= lim)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {err.numel()} elements outside the bound; worst err / bound "
                                 f"{float((err / lim).nan_to_num(0.0).max()):.2f}, max err {float(err.max()):.3e}")


# ============================================================================= fine-tune head: InfoNCE

def infonce_inputs(B, F_, dominant, seed):
    E = 64
    if dominant:              # one entry per row and column of every block stands out: 100 on the diagonal, noise elsewhere
        S = randn(B, B * (1 + F_), seed=seed, device="cpu").double() * 2.0
        S.scatter_(1, R.infonce_cols(B, F_), 100.0)
    else:                     # 100 * cosine of real normalised vectors
        q = R.l2norm(randn(B, E, seed=seed, device="cpu").double())
        keys = R.l2norm(randn(B * (1 + F_), E, seed=seed + 1, device="cpu").double() + 0.5 * q.repeat_interleave(1 + F_, 0))
        S = 100.0 * q @ keys.t()
    return S.float().to(DEV)


WV = 0.85


def wf_of(F_):
    return 0.15 / F_ * 1.37 if F_ else 0.0


@pytest.mark.parametrize("dominant", [False, True])
@pytest.mark.parametrize("F_", [0, 1, 12, 24])
@pytest.mark.parametrize("B", [1, 3, 7, 8, 64, 65, 256, 300])
def test_infonce_fwd_bwd(B, F_, dominant):
    """loss, lse_row, lse_col and dS of hmmc_infonce_fwd / _bwd against fp64 (autograd for dS, upstream gradient 1.7).  B = 65 wraps
    the row LSE's 64 lanes, B < 8 leaves column row lanes empty, C = B(1 + F) mostly not a multiple of 32; w_video != w_frame."""
    wf = wf_of(F_)
    S = infonce_inputs(B, F_, dominant, seed=B * 31 + F_)
    gout = torch.full((), 1.7, device=DEV)
    loss, lse_row, lse_col = ops.infonce_fwd(S, B, F_, WV, wf)
    dS = ops.infonce_bwd(S, lse_row, lse_col, gout, B, F_, WV, wf)
    S64 = S.double().requires_grad_()
    l64, r64, c64 = R.infonce(S64, B, F_, WV, wf)
    (l64 * 1.7).backward()
    b_loss, b_row, b_col, b_dS = R.infonce_bounds(S64.detach(), B, F_, WV, wf, 1.7)
    within(lse_row, r64, b_row, "lse_row")
    within(lse_col, c64, b_col, "lse_col")
    within(loss, l64, b_loss, "loss")
    within(dS, S64.grad, b_dS, "dS")
    loss2, lse_row2, lse_col2 = ops.infonce_fwd(S, B, F_, WV, wf)            # the fixed merge order: bit-stable
    assert torch.equal(loss, loss2) and torch.equal(lse_row, lse_row2) and torch.equal(lse_col, lse_col2)


# ============================================================================= top-k mean, segment max

@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("F_,k", [(1, 1), (12, 1), (12, 3), (12, 12), (24, 1), (24, 3), (24, 24), (64, 1), (64, 3), (64, 64)])
def test_topk_mean(F_, k, strided):
    """mean of the k largest of F frames (+ base): exact on quarter-integer data (many duplicates; sums of at most 64 of them are
    exact), so the one rounding of the mean and the one of the add are all (U |mean| + U |out|); -inf entries, some cells with fewer
    than k finite frames (-inf result)."""
    bq, bv = 5, 7
    lds, ldb = (bv * F_ + 9, bv + 3) if strided else (bv * F_, bv)
    g = gen(F_ * 100 + k)
    Sf = (torch.randint(-8, 9, (bq, lds), generator=g, device=DEV).float() / 4)
    Sf[torch.rand(bq, lds, generator=g, device=DEV) < 0.1] = float("-inf")
    Sf[0, :F_] = float("-inf")                                 # a cell with no finite frame
    base = torch.randint(-20, 21, (bq, ldb), generator=g, device=DEV).float() / 8
    for b in (None, base):
        out = ops.topk_mean(Sf, bq, bv, F_, k, base=b, lds=lds if strided else None, ldb=ldb if strided else None)
        ref = R.topk_mean(Sf.double(), bq, bv, F_, k, None if b is None else b.double(), lds, ldb)
        mean = R.topk_mean(Sf.double(), bq, bv, F_, k, None, lds, ldb)
        within(out, ref, U * (mean.abs() + ref.abs()).nan_to_num(0.0, 0.0, 0.0), f"topk_mean base={b is not None}")


def test_topk_mean_random():
    bq, bv, F_, k = 9, 33, 24, 3
    Sf = randn(bq, bv * F_, seed=5) * 30
    base = randn(bq, bv, seed=6) * 30
    out = ops.topk_mean(Sf, bq, bv, F_, k, base=base)
    top = torch.topk(Sf.double().view(bq, bv, F_), k, dim=2).values
    ref = base.double() + top.mean(2)
    within(out, ref, k * U * top.abs().sum(2) / k + U * (top.mean(2).abs() + ref.abs()), "topk_mean random")


def test_segment_max():
    """uneven segments (one of length 1), and the strided ld > V form through the C-ABI: a max is exact."""
    V, ld = 300, 345
    wide = randn(17, ld, seed=7)
    wide[:, V:] = 1e30                                         # outside the V columns: must never be read into the result
    offs = torch.tensor([0, 1, 6, 13, 17], dtype=torch.int32, device=DEV)
    ref = R.segment_max(wide[:, :V], offs.tolist())
    out = torch.empty(4, V, device=DEV)
    call("hmmc_segment_max", ptr(wide), ptr(offs), ptr(out), 4, V, ld)
    assert torch.equal(out, ref)
    assert torch.equal(ops.segment_max(wide[:, :V].contiguous(), offs), ref)


# ============================================================================= L2 normalisation

@pytest.mark.parametrize("eps", [0.0, 1e-12])
@pytest.mark.parametrize("D", [4, 12, 260, 512, 1028])
def test_l2norm_fwd_bwd(D, eps):
    """rows = 37 (not a multiple of the 4 rows of a block); with eps an all-zero row, which F.normalize clamps (y = 0,
    norm = eps, dx = dy / eps).  Backward against fp64 autograd with a non-unit upstream gradient."""
    rows = 37
    x = randn(rows, D, seed=D) * 3
    if eps:
        x[5] = 0.0
        x[-1] = 0.0
    dy = randn(rows, D, seed=D + 1) * 0.7
    y, norm = ops.l2norm_fwd(x, eps=eps)
    dx = ops.l2norm_bwd(dy, y, norm)
    x64 = x.double().requires_grad_()
    y64 = R.l2norm(x64, eps)
    y64.backward(dy.double())
    b_y, b_n, b_dx = R.l2norm_bounds(x.double(), dy.double(), eps, D)
    within(y, y64, b_y, "y")
    within(norm, x.double().norm(dim=1).clamp_min(eps), b_n.squeeze(1), "norm")
    within(dx, x64.grad, b_dx, "dx")
    assert torch.isfinite(dx).all()


# ============================================================================= temporal pooling, row bias

@pytest.mark.parametrize("with_u", [True, False])
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("F_", [1, 3, 12, 24])
def test_temporal_pool_fwd_bwd(F_, D, with_u):
    b = 3
    h = randn(b * F_, D, seed=F_ * D)
    u = randn(b * F_, D, seed=F_ * D + 1) if with_u else None
    dout = randn(b, D, seed=F_ * D + 2) * 1.3
    out, norms = ops.temporal_pool_fwd(h, u, b, F_, D)
    dvf = ops.temporal_pool_bwd(h, u, norms, dout, b, F_, D)
    h64 = h.double().requires_grad_()
    ref = R.temporal_pool(h64, None if u is None else u.double(), b, F_, D)
    ref.backward(dout.double())
    b_out, b_dv = R.pool_bounds(h.double(), None if u is None else u.double(), dout.double(), b, F_, D)
    within(out, ref, b_out, "pooled")
    vf = h.double() + (u.double() if u is not None else 0)
    within(norms.view(-1), vf.norm(dim=1), (math.ceil(D / 64) / 2 + 6) * U * vf.norm(dim=1), "norms")
    within(dvf, h64.grad, b_dv, "dvf")


def test_temporal_pool_rejects_rows_wider_than_its_lds():
    h = torch.zeros(2 * 3, 1028, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):                  # the status comes back before any launch
        ops.temporal_pool_fwd(h, None, 2, 3, 1028)


def test_add_rowbias_exact():
    """one fp32 add per element: bit-exact; 37 rows over a period of 12 (the last period partial)."""
    x = randn(37, 516, seed=13)
    table = randn(12, 516, seed=14)
    out = ops.add_rowbias(x, table, 12)
    assert torch.equal(out, x + table[torch.arange(37, device=DEV) % 12])
    assert not torch.equal(out, x + table[torch.arange(37, device=DEV) % 11]), "(the period matters)"


# ============================================================================= fp32 attention (temporal / fp32 regime)

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 8, 12])
@pytest.mark.parametrize("L", [1, 2, 12, 24, 33, 63, 64, 65, 77, 128, 197, 256])
def test_attention_f32_fwd_bwd(L, H, causal):
    """hmmc_temporal_attention_fwd / _bwd: the one-wave kernels up to 64 tokens (at 64 the backward asks for ~97 KB of LDS), the
    256-thread kernels from 65 to 256.  out, the saved probabilities (the backward reads them) and dqkv against fp64 autograd."""
    b = 2
    qkv = randn(b * L, 3 * H * 64, seed=L * 100 + H) * 1.5
    dout = randn(b * L, H * 64, seed=L * 100 + H + 1) * 0.8
    out, probs = ops.attention_f32_fwd(qkv, b, L, H, causal)
    dqkv = ops.attention_f32_bwd(qkv, probs, dout, b, L, H)
    q64 = qkv.double().requires_grad_()
    o64, p64 = R.attention(q64, b, L, H, causal)
    o64.backward(dout.double())
    b_o, b_p, b_dqkv = R.attention_bounds(qkv.double(), dout.double(), b, L, H, causal)
    within(probs, p64, b_p, "probs")
    within(out, o64, b_o, "out")
    within(dqkv, q64.grad, b_dqkv, "dqkv")


def test_attention_f32_rejects_more_than_256_tokens():
    qkv = torch.zeros(257, 3 * 64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.attention_f32_fwd(qkv, 1, 257, 1)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.attention_f32_bwd(qkv, torch.zeros(1, 1, 257, 257, device=DEV), torch.zeros(257, 64, device=DEV), 1, 257, 1)


# ============================================================================= BatchNorm (projector / predictor MLPs)

EPS = 1e-5


def bn_inputs(M, N, seed):
    g = gen(seed)
    h = torch.randint(-8, 9, (M, N), generator=g, device=DEV).float()          # integer data: column sums are exact in fp32
    gamma = torch.rand(N, generator=g, device=DEV) * 1.5 + 0.25
    beta = torch.randn(N, generator=g, device=DEV) * 0.5
    # h takes 17 values, so the pre-activation takes 17 per column: move beta until none is within 1e-3 of the ReLU's kink, so
    # the fp64 reference and the kernel agree on every mask bit and the backward can be compared with fp64 autograd of relu(bn)
    hd = h.double()
    mean, var = hd.mean(0), hd.var(0, unbiased=False)
    k = torch.arange(-8, 9, device=DEV, dtype=D64).unsqueeze(1)
    for _ in range(20):
        z = (k - mean) / torch.sqrt(var + EPS) * gamma.double() + beta.double()
        near = (z.abs() < 1e-3).any(0)
        if not bool(near.any()):
            break
        beta = beta + near.float() * 0.0123
    assert not bool(near.any())
    dy = torch.randn(M, N, generator=g, device=DEV) * 0.9
    return h, gamma, beta, dy


@pytest.mark.parametrize("N", [4, 36, 512, 4096])
@pytest.mark.parametrize("M", [2, 3, 63, 64, 65, 1000, 16385, 40000])
def test_batchnorm(M, N):
    """bn_stats (exact on integer data: torch.equal), bn_finalize on both the host-n and the device-n path (the same bits),
    the running statistics and num_batches_tracked against nn.BatchNorm1d(momentum=0.1), bn_apply_relu, and
    bn_bwd_reduce + bn_bwd_apply against fp64 autograd of relu(batchnorm(h)).  M = 16385 / 40000 pass the 256-slab cap."""
    h, gamma, beta, dy = bn_inputs(M, N, seed=M * 7 + N)
    hd, gd, bd, dyd = h.double(), gamma.double(), beta.double(), dy.double()
    sums = ops.bn_stats(h)
    ref_sums = torch.stack([hd.sum(0), (hd * hd).sum(0)]).float()
    assert torch.equal(sums, ref_sums), "column sums"
    rm0 = torch.randn(N, generator=gen(N), device=DEV) * 0.1
    rv0 = torch.rand(N, generator=gen(N + 1), device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
    mean, var, rstd = ops.bn_finalize(sums, float(M), EPS, 0.1, rm, rv, nbt)
    mean_d, var_d, rstd_d = ops.bn_finalize(sums, torch.full((1,), float(M), device=DEV), EPS, 0.0)
    assert torch.equal(mean, mean_d) and torch.equal(var, var_d) and torch.equal(rstd, rstd_d), "n on the device vs on the host"
    bn = torch.nn.BatchNorm1d(N, eps=EPS, momentum=0.1).double().to(DEV).train()
    with torch.no_grad():
        bn.running_mean.copy_(rm0.double())
        bn.running_var.copy_(rv0.double())
        bn.num_batches_tracked.fill_(3)
    bn(hd)
    assert int(nbt) == int(bn.num_batches_tracked) == 4
    fb = R.bn_fwd_bounds(hd, gd, M, 0.1, rm0.double(), rv0.double(), EPS)
    within(mean, fb["mean"], fb["em"], "mean")
    within(var, hd.var(0, unbiased=False), fb["ev"], "var")
    within(rstd, fb["rstd"], fb["erstd"], "rstd")
    within(rm, bn.running_mean, fb["erm"], "running_mean")
    within(rv, bn.running_var, fb["erv"], "running_var")
    y = ops.bn_apply_relu(h, mean, rstd, gamma, beta)
    hr = hd.clone().requires_grad_()
    yr, _, _ = R.bn_relu(hr, gd, bd, EPS)
    within(y, yr, fb["ez"] + U * bd.abs(), "y")
    yr.backward(dyd)
    sums_b = ops.bn_bwd_reduce(dy, y, h, mean, rstd)
    assert torch.equal(sums_b, ops.bn_bwd_reduce(dy, y, h, mean, rstd)), "slab order: bit-stable"
    dh = ops.bn_bwd_apply(dy, y, h, mean, rstd, gamma, sums_b, M)
    within(dh, hr.grad, R.bn_bwd_bound(hd, dyd, gd, fb, M, N, yr.detach()), "dh")


@pytest.mark.parametrize("M,N", [(1000, 36), (40000, 512)])
def test_batchnorm_sync_contract(M, N):
    """SyncBatchNorm: the column sums of two row halves added together, finalised with n = the global row count, give what one
    call over all rows gives (exactly: integer data); the backward sums of the halves added and applied per half with the global
    n give dh within the same bound."""
    h, gamma, beta, dy = bn_inputs(M, N, seed=M + N)
    m1 = M // 3
    sums = ops.bn_stats(h)
    halves = ops.bn_stats(h[:m1].contiguous()) + ops.bn_stats(h[m1:].contiguous())
    assert torch.equal(halves, sums)
    n_dev = torch.full((1,), float(M), device=DEV)
    a = ops.bn_finalize(halves, n_dev, EPS)
    b = ops.bn_finalize(sums, float(M), EPS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    mean, _, rstd = a
    y = ops.bn_apply_relu(h, mean, rstd, gamma, beta)
    parts = [(h[:m1].contiguous(), y[:m1].contiguous(), dy[:m1].contiguous()), (h[m1:].contiguous(), y[m1:].contiguous(), dy[m1:].contiguous())]
    bsum = sum(ops.bn_bwd_reduce(d_, y_, h_, mean, rstd) for h_, y_, d_ in parts)
    dh = torch.cat([ops.bn_bwd_apply(d_, y_, h_, mean, rstd, gamma, bsum, M) for h_, y_, d_ in parts])
    hd = h.double().requires_grad_()
    yr, _, _ = R.bn_relu(hd, gamma.double(), beta.double(), EPS)
    yr.backward(dy.double())
    fb = R.bn_fwd_bounds(h.double(), gamma.double(), M, 0.0, torch.zeros(N, device=DEV, dtype=D64), torch.ones(N, device=DEV, dtype=D64), EPS)
    within(dh, hd.grad, R.bn_bwd_bound(h.double(), dy.double(), gamma.double(), fb, M, N, yr.detach()), "dh (halves)")


def test_mlp_momentum_none_is_a_cumulative_average():
    """MlpFn with momentum None (nn.BatchNorm1d's cumulative average: factor 1 / num_batches_tracked) follows nn.BatchNorm1d over
    three batches; without running statistics it needs no counter."""
    K, N = 24, 36
    w1, b1 = randn(N, K, seed=20) * 0.2, randn(N, seed=21) * 0.1
    gamma, beta = torch.rand(N, generator=gen(22), device=DEV) + 0.5, randn(N, seed=23) * 0.1
    w2, b2 = randn(8, N, seed=24) * 0.2, randn(8, seed=25) * 0.1
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    nbt = torch.tensor(0, dtype=torch.int64, device=DEV)
    bn = torch.nn.BatchNorm1d(N, eps=EPS, momentum=None).double().to(DEV).train()
    for step in range(3):
        x = randn(50 + step, K, seed=30 + step)
        Fn.MlpFn.apply(x, w1, b1, gamma, beta, w2, b2, EPS, (rm, rv, nbt, None))
        bn(F.linear(x.double(), w1.double(), b1.double()))
    assert int(nbt) == int(bn.num_batches_tracked) == 3
    # three exponential-average steps of O(1) statistics in fp32, each a handful of roundings; the GEMM's fp32 sums over K = 24
    torch.testing.assert_close(rm.double(), bn.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.double(), bn.running_var, rtol=1e-5, atol=1e-6)
    Fn.MlpFn.apply(randn(10, K, seed=40), w1, b1, gamma, beta, w2, b2, EPS, (None, None, None, None))
    with pytest.raises(ValueError, match="num_batches_tracked"):
        Fn.MlpFn.apply(randn(10, K, seed=40), w1, b1, gamma, beta, w2, b2, EPS, (rm, rv, None, None))


# ============================================================================= MoCo loss, rowdot, row_axpy

T = 0.07


@pytest.mark.parametrize("Kq", [1, 255, 257, 4096, 12288, 65536])
@pytest.mark.parametrize("R_", [1, 5, 352])
def test_moco_loss(R_, Kq):
    """hmmc_moco_loss_fwd / _bwd at T = 0.07 on cosine-range logits, lpos above every negative (even rows) and below every
    negative (odd rows); the backward overwrites S with dS.  Two forward launches give the same bits."""
    g = gen(R_ * 7 + Kq)
    S = torch.rand(R_, Kq, generator=g, device=DEV) * 1.6 - 0.8
    lpos = torch.where(torch.arange(R_, device=DEV) % 2 == 0, 0.95, -0.95).float()
    w = 0.37
    gout = torch.full((), 1.3, device=DEV)
    loss, lse = ops.moco_loss_fwd(S, lpos, T, w)
    loss2, lse2 = ops.moco_loss_fwd(S, lpos, T, w)
    assert torch.equal(loss, loss2) and torch.equal(lse, lse2), "run-to-run bits"
    dS = S.clone()
    dlpos = ops.moco_loss_bwd_(dS, lpos, lse, gout, T, w)
    Sd, lpd = S.double().requires_grad_(), lpos.double().requires_grad_()
    l64, lse64 = R.moco_loss(Sd, lpd, T, w)
    (l64 * 1.3).backward()
    e_lse, b_loss, b_dS, b_dl = R.moco_bounds(S.double(), lpos.double(), Kq, R_, w, 1.3, T)
    within(lse, lse64, e_lse, "lse")
    within(loss, l64, b_loss, "loss")
    within(dS, Sd.grad, b_dS, "dS")
    within(dlpos, lpd.grad, b_dl, "dlpos")


@pytest.mark.parametrize("D", [1, 100, 513])
@pytest.mark.parametrize("R_", [1, 5, 352])
def test_rowdot_row_axpy(R_, D):
    a, b = randn(R_, D, seed=R_ + D), randn(R_, D, seed=R_ + D + 1)
    s = randn(R_, seed=R_ + D + 2)
    out = ops.rowdot(a, b)
    ad, bd = a.double(), b.double()
    within(out, (ad * bd).sum(1), (math.ceil(D / 64) + 6) * U * (ad * bd).abs().sum(1), "rowdot")
    y = randn(R_, D, seed=R_ + D + 3)
    ref = y.double() + s.double().unsqueeze(1) * ad
    ops.row_axpy_(y, s, a)
    within(y, ref, U * ((s.double().unsqueeze(1) * ad).abs() + ref.abs()), "row_axpy")


# ============================================================================= MLM head pieces: cross entropy, erf-GELU

@pytest.mark.parametrize("V", [1, 7, 49408])
def test_cross_entropy(V):
    """labels 0 and V - 1, rows ignored with -100 and -1, against F.cross_entropy on the valid rows; and a batch in which every
    row is ignored (loss sum 0, count 0, gradient 0).  Labels are always < V: the kernel does not bound-check them."""
    Rr = 9
    logits = randn(Rr, V, seed=V) * 3
    labels = torch.tensor([0, V - 1, -100, (V // 2), -1, 0, V - 1, -100, (V // 3)], dtype=torch.int64, device=DEV)
    loss_sum, lse, count = ops.ce_fwd(logits, labels)
    keep = labels >= 0
    nval = int(keep.sum())
    assert float(count) == nval
    l64 = logits.double().requires_grad_()
    ref = F.cross_entropy(l64[keep], labels[keep], ignore_index=-100)
    (ref * 0.6).backward()
    chain = math.ceil(V / 256) + 11
    e_lse = R.lse_bound(logits.double(), 1, chain)
    within(lse[keep], torch.logsumexp(logits.double(), 1)[keep], e_lse[keep], "lse")
    rows = (torch.logsumexp(logits.double(), 1) - logits.double().gather(1, labels.clamp_min(0).unsqueeze(1)).squeeze(1))[keep]
    b_sum = (e_lse[keep] + U * rows.abs()).sum() + (math.ceil(Rr / 256) + 8) * U * rows.abs().sum()
    within(loss_sum / nval, ref, b_sum / nval + U * ref.abs(), "mean loss")
    dl = ops.ce_bwd_(logits.clone(), labels, lse, torch.full((), 0.6, device=DEV), count)
    t = logits.double() - torch.logsumexp(logits.double(), 1, keepdim=True)
    p = torch.exp(t)
    gg = 0.6 / nval
    b_dl = gg * (p * (R.exp_rel(t) + e_lse.unsqueeze(1)) + U * (p + 1)) + 2 * U * l64.grad.abs() + R.TINY
    within(dl, l64.grad, b_dl * keep.unsqueeze(1), "dlogits")
    assert torch.equal(dl[~keep], torch.zeros_like(dl[~keep]))
    none = torch.tensor([-100, -1, -100], dtype=torch.int64, device=DEV)
    lg = randn(3, V, seed=V + 1)
    s0, _, c0 = ops.ce_fwd(lg, none)
    assert float(s0) == 0.0 and float(c0) == 0.0
    assert torch.equal(ops.ce_bwd_(lg.clone(), none, torch.zeros(3, device=DEV), torch.ones((), device=DEV), c0), torch.zeros_like(lg))


def test_gelu_erf():
    """x over [-12, 12] (0 included) with the derived bounds; at +-1e4 and +-1e30 erf has saturated and the fp32 results are
    exactly x (or 0) and dy (or 0), as the fp64 reference rounded to fp32 is."""
    x = torch.cat([torch.linspace(-12, 12, 24001, device=DEV), torch.zeros(1, device=DEV)])
    dy = randn(x.numel(), seed=50)
    y, dx = ops.gelu_erf_fwd(x), ops.gelu_erf_bwd(x, dy)
    x64 = x.double().requires_grad_()
    y64 = R.gelu_erf(x64)
    y64.backward(dy.double())
    b_y, b_dx = R.gelu_bounds(x.double(), dy.double())
    within(y, y64, b_y, "gelu")
    within(dx, x64.grad, b_dx, "gelu backward")
    big = torch.tensor([1e4, -1e4, 1e30, -1e30], device=DEV)
    dyb = torch.tensor([0.5, 0.5, -2.0, 3.0], device=DEV)
    xb = big.double().requires_grad_()
    yb = R.gelu_erf(xb)
    yb.backward(dyb.double())
    assert torch.equal(ops.gelu_erf_fwd(big), yb.float())
    assert torch.equal(ops.gelu_erf_bwd(big, dyb), xb.grad.float())


# ============================================================================= queue enqueue

def test_enqueue_last_columns_and_zero_key():
    """keys written to the LAST R columns (col0 = W - R) of a [E, W] queue, one key row all zero (the 1e-12 clamp: a zero
    column); every other column untouched."""
    R_, E, W = 5, 100, 37
    keys = randn(R_, E, seed=60)
    keys[2] = 0.0
    queue = torch.full((E, W), 7.0, device=DEV)
    ref = R.enqueue(keys.double(), queue.double(), W - R_)
    ops.enqueue(keys, queue, W - R_)
    assert torch.equal(queue[:, :W - R_], torch.full((E, W - R_), 7.0, device=DEV))
    assert torch.equal(queue[:, W - R_ + 2], torch.zeros(E, device=DEV))
    within(queue, ref, (math.ceil(E / 64) / 2 + 5) * U * ref.abs(), "enqueued keys")


# ============================================================================= multi-tensor optimizer kernels

def split_alloc(flat, sizes):
    """one allocation per tensor, as a model's parameters and gradients have (the kernels' 16-byte loads assume the allocator's
    alignment; views into one buffer would not have it)"""
    return [t.clone() for t in torch.split(flat, sizes)]


def ragged_params(sizes, dtype, seed, scale):
    g = torch.Generator().manual_seed(seed)
    flat_p = (torch.randn(sum(sizes), generator=g) * 0.5).to(dtype).to(DEV)
    flat_g = (torch.randn(sum(sizes), generator=g) * scale).to(dtype).to(DEV)
    ps = [torch.nn.Parameter(t) for t in split_alloc(flat_p, sizes)]
    for p, gr in zip(ps, split_alloc(flat_g, sizes)):
        p.grad = gr
    return ps


@pytest.mark.parametrize("T_", [4097, 5000])
def test_clip_above_4096_tensors(T_):
    """clip_grad_norm_ over more tensors than the single-block finish kernel takes (FINISH_COEF_MAX_T = 4096): the per-tensor
    finish and the separate coefficient kernel.  Total norm and clipped gradients against fp64; two calls on the same gradients
    give the same bits."""
    from hmmc_amd.optimization import clip_grad_norm_
    sizes = [1 + (i * 37) % 300 for i in range(T_)]
    ps = ragged_params(sizes, torch.float32, T_, 0.05)
    g0 = [p.grad.double().clone() for p in ps]
    keep = [p.grad.clone() for p in ps]
    total, clipped = R.clip_grad_norm(g0, 1.0)
    assert total > 1.0
    tn = clip_grad_norm_(ps, 1.0)
    rel = R.clip_rel(max(sizes), T_)
    within(tn, torch.tensor(total, dtype=D64), torch.tensor(rel * total, dtype=D64), "total norm")
    within(torch.cat([p.grad for p in ps]), torch.cat(clipped), (rel + 3 * U) * torch.cat(clipped).abs() + R.TINY, "clipped")
    first = torch.cat([p.grad for p in ps]).clone()
    for p, k in zip(ps, keep):
        p.grad.copy_(k)
    tn2 = clip_grad_norm_(ps, 1.0)
    assert torch.equal(tn, tn2) and torch.equal(first, torch.cat([p.grad for p in ps])), "run-to-run bits"


@pytest.mark.parametrize("T_", [100, 4097])
def test_mt_sumsq_and_plain_clip_through_the_abi(T_):
    """hmmc_mt_sumsq (per-tensor squared norms, a 65-chunk tensor among them) against fp64, and hmmc_mt_clip_grad_norm (the clip
    without the hand-over) bit-identical to the total norm and gradients of the hmmc_mt_clip_grad_norm_keep path of
    clip_grad_norm_, below and above the 4096 tensors of the single-block finish."""
    from hmmc_amd.optimization import _TensorTable, clip_grad_norm_
    sizes = [1 + (i * 37) % 300 for i in range(T_ - 1)] + [2100001]
    ps = ragged_params(sizes, torch.float32, T_ + 1, 0.05)
    keep = [p.grad.clone() for p in ps]
    tbl = _TensorTable(torch.device(DEV)).build([(0, p.grad.data_ptr(), 0, 0, p.numel(), 1) for p in ps])
    call("hmmc_mt_sumsq", ptr(tbl.tab), ptr(tbl.chunk), tbl.nchunks, ptr(tbl.sumsq), tbl.T)
    ref = torch.stack([(g.double() ** 2).sum() for g in keep])
    chain = torch.tensor([4 * math.ceil(min(n, 32768) / 1024) + 14 + math.ceil(math.ceil(n / 32768) / 64) + 6 for n in sizes],
                         dtype=D64, device=DEV)
    within(tbl.sumsq[:T_], ref, chain * U * ref, "per-tensor sums of squares")
    out = torch.empty(2, device=DEV)
    call("hmmc_mt_clip_grad_norm", ptr(tbl.tab), ptr(tbl.chunk), tbl.nchunks, ptr(tbl.sumsq), tbl.T, 1.0, ptr(out))
    plain = [p.grad.clone() for p in ps]
    for p, k in zip(ps, keep):
        p.grad.copy_(k)
    tn = clip_grad_norm_(ps, 1.0)
    assert torch.equal(out[1], tn) and all(torch.equal(a, p.grad) for a, p in zip(plain, ps))


@pytest.mark.parametrize("T_", [4097, 5000])
@pytest.mark.parametrize("max_norm,scale",[(1.0, 0.05), (1e6, 3.0)])
def test_bertadam_takes_the_clip_norms_above_4096_tensors(T_, max_norm, scale, monkeypatch):
    """With more than 4096 tensors the clip runs its other kernel pair; the BertAdam.step that takes the squared norms it left
    must be bit-identical to one that forms them itself (global clip active; per-parameter clip active)."""
    from hmmc_amd import optimization
    from hmmc_amd.optimization import BertAdam, clip_grad_norm_
    taken = []
    orig = BertAdam._norms_from_clip

    def spy(fp, grad_ptrs, grads, device):
        r = orig(fp, grad_ptrs, grads, device)
        taken.append(r is not None)
        return r

    monkeypatch.setattr(BertAdam, "_norms_from_clip", staticmethod(spy))
    sizes = [1 + (i * 37) % 300 for i in range(T_)]

    def run(shared):
        ps = ragged_params(sizes, torch.float32, 7, scale)
        opt = BertAdam(ps, lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=50, weight_decay=0.01,
                       max_grad_norm=1.0)
        monkeypatch.setattr(optimization, "_NO_SHARED_NORMS", not shared)
        for step in range(3):
            gs = split_alloc((torch.randn(sum(sizes), generator=torch.Generator().manual_seed(step)) * scale).to(DEV), sizes)
            for p, gr in zip(ps, gs):
                p.grad = gr
            clip_grad_norm_(ps, max_norm)
            opt.step()
        torch.cuda.synchronize()
        return [t.detach().clone() for p in ps for t in (p, p.grad, opt.state[p]["next_m"], opt.state[p]["next_v"])]

    ref = run(False)
    assert not any(taken)
    got = run(True)
    assert any(taken), "the hand-over was never taken"
    assert all(torch.equal(a, b) for a, b in zip(ref, got)), "shared norms changed a result"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_clip_one_tensor_of_more_than_64_chunks(dtype):
    """2 100 001 elements = 65 chunks of 32768: tensor_sumsq's lanes walk the chunk list in steps of 64, lane 0 takes two."""
    from hmmc_amd.optimization import clip_grad_norm_
    ps = ragged_params([2100001, 3], dtype, 9, 0.01)
    g0 = [p.grad.double().clone() for p in ps]
    total, clipped = R.clip_grad_norm(g0, 1.0)
    assert total > 1.0
    tn = clip_grad_norm_(ps, 1.0)
    rel = R.clip_rel(2100001, 2) + (2.0 ** -11 if dtype == torch.float16 else 0.0)   # torch rounds each norm to the tensor's dtype
    within(tn, torch.tensor(total, dtype=D64), torch.tensor(rel * total, dtype=D64), "total norm")
    out_rel = rel + 3 * U + (2.0 ** -11 if dtype == torch.float16 else 0.0)        # fp16 gradients round once more
    tiny = 2.0 ** -24 if dtype == torch.float16 else R.TINY
    within(torch.cat([p.grad for p in ps]), torch.cat(clipped), out_rel * torch.cat(clipped).abs() + tiny, "clipped")
    # the slip this catches in fp32: the 65th chunk missing from the norm (in fp16 the norm itself is rounded to 11 bits, and
    # the 2849 elements of that chunk move it by less than that: test_sumsq_of_65_chunks_exact_on_integer_gradients covers fp16)
    if dtype == torch.float32:
        short = math.sqrt(total ** 2 - float((g0[0][64 * 32768:] ** 2).sum()))
        assert abs(short - total) > R.SLACK * rel * total


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_sumsq_of_65_chunks_exact_on_integer_gradients(dtype):
    """integer-valued gradients (|g| <= 2) in one tensor of 2 100 001 elements: every partial sum of squares, and the 65-chunk total
    (<= 8.4e6 < 2^24), is an integer fp32 holds exactly, so hmmc_mt_sumsq must return sum g^2 exactly - in fp16 as in fp32, where
    the clip's own tolerance (the norm rounded to fp16) cannot see the 2849 elements of the 65th chunk, which only lane 0's second
    step of tensor_sumsq adds."""
    from hmmc_amd.optimization import _TensorTable
    n = 2100001
    g = torch.randint(-2, 3, (n,), generator=gen(65), device=DEV).to(dtype)
    tbl = _TensorTable(torch.device(DEV)).build([(0, g.data_ptr(), 0, 0, n, 0 if dtype == torch.float16 else 1)])
    assert tbl.nchunks == 65
    call("hmmc_mt_sumsq", ptr(tbl.tab), ptr(tbl.chunk), tbl.nchunks, ptr(tbl.sumsq), tbl.T)
    exact = int((g.long() ** 2).sum())
    assert float(tbl.sumsq[0]) == exact
    assert int((g[64 * 32768:].long() ** 2).sum()) > 0, "(the 65th chunk contributes)"


RAGGED = [1, 7, 32767, 32769, 65537]


def oracle_adam_step(p, g, m, v, *args):
    """oracle.bert_adam_step evaluated so that every element takes the arithmetic the golden vectors pin.  torch's CPU kernels
    evaluate an fp16 `add(g, alpha)` as an fma in their vectorised body but round alpha * g to fp16 first in the scalar remainder
    of each thread's range, so the CPU result depends on the thread split and on numel mod the vector width; the goldens
    (test_bertadam_vs_reference_golden: 64- and 128-element fp16 tensors) only ever take the body.  One thread, and zero padding to
    a multiple of 64 elements (zeros leave the norm and every other element unchanged)."""
    n = p.numel()
    pad = (-n) % 64
    ext = [torch.cat([t.reshape(-1), torch.zeros(pad, dtype=t.dtype)]) for t in (p, g, m, v)]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = O.bert_adam_step(*ext, *args)
    finally:
        torch.set_num_threads(threads)
    return [t[:n].reshape(p.shape) for t in out]


def _adam_vs_oracle(dtype, scale, steps=3):
    from hmmc_amd.optimization import BertAdam
    ps = ragged_params(RAGGED, dtype, 11, scale)
    lr, t_total, warm, wd = 1e-3, 20, 0.1, 0.01
    opt = BertAdam(ps, lr=lr, warmup=warm, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=t_total, weight_decay=wd,
                   max_grad_norm=1.0)
    ref = [(p.detach().cpu().clone(), torch.zeros(p.shape, dtype=dtype), torch.zeros(p.shape, dtype=dtype), torch.zeros(p.shape, dtype=D64))
           for p in ps]
    res = []
    for step in range(steps):
        g = torch.Generator().manual_seed(100 + step)
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * scale).to(dtype).to(DEV)
        grads = [p.grad.cpu().clone() for p in ps]
        opt.step()
        for i, p in enumerate(ps):
            rp, rm, rv, mabs = ref[i]
            rp, rm, rv, rg = oracle_adam_step(rp, grads[i], rm, rv, step, lr, t_total, warm, wd)
            mabs = 0.9 * mabs + 0.1 * rg.double().abs()          # what m would be without cancellation: the scale of its error
            ref[i] = (rp, rm, rv, mabs)
            st = opt.state[p]
            res.append((f"{p.numel()}@{step}", (p.detach().cpu(), st["next_m"].cpu(), st["next_v"].cpu(), p.grad.cpu()), (rp, rm, rv, rg),
                        mabs))
    return res


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_bertadam_ragged_sizes_vs_oracle(dtype):
    """numel % 8 != 0 (fp16) / % 4 != 0 (fp32) and sizes straddling the 32768-element chunks, per-parameter clip inactive (every
    gradient norm < max_grad_norm, so the update does not depend on how a norm was summed): fp16 weights and moments bit-identical
    to oracle.bert_adam_step on the CPU copies (oracle_adam_step), fp32 within test_bertadam_vs_reference_golden's 2e-8 abs + 2e-6 rel."""
    for what, mine, ref, _ in _adam_vs_oracle(dtype, 1e-3):
        for name, a, b in zip("pmvg", mine, ref):
            if dtype == torch.float16:
                assert torch.equal(a, b), f"{what}.{name}: {int((a != b).sum())} fp16 elements differ"
            else:
                within(a, b.double(), (2e-8 + 2e-6 * b.double().abs()) / R.SLACK, f"{what}.{name}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_bertadam_ragged_sizes_clip_active(dtype):
    """the same with every per-parameter clip active: the clip coefficient comes from norms summed in another order than torch's
    (<= 80 U ~ 5e-6 relative in fp32; for fp16 the norm and coefficient are rounded to fp16, so a rounding boundary can move
    them by one fp16 ulp, 2^-10 relative).  Gradient and v within 1e-5 (fp32) / 2^-9 (fp16, two ulps) relative; m, a sum of
    terms of both signs, within that much of the sum of their magnitudes; weights within 2e-8 + 2e-6 |p| (fp32) / one fp16 ulp
    of p (2^-10 |p| at most)."""
    f16 = dtype == torch.float16
    rel = 2.0 ** -9 if f16 else 1e-5
    for what, mine, ref, mabs in _adam_vs_oracle(dtype, 3.0):
        for name, a, b in zip("pmvg", mine, ref):
            b = b.double()
            if name == "p":
                bound = 2.0 ** -10 * b.abs() + 2.0 ** -24 if f16 else 2e-8 + 2e-6 * b.abs()
            else:
                bound = rel * (b.abs() + (mabs if name == "m" else 0)) + (2.0 ** -24 if f16 else 1e-30)
            within(a, b, bound / R.SLACK, f"{what}.{name}")


def test_ema_ragged_sizes_vs_oracle():
    """the momentum-encoder EMA (BirdPreTrainedModel._momentum_update, one hmmc_mt_ema launch) on the ragged sizes, fp16 and
    fp32 in one table: fp16 bit-identical to oracle.momentum_update, fp32 within 2e-8 abs + 2e-6 rel."""
    from hmmc_amd.modeling import BirdPreTrainedModel

    class Pairs(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.online = torch.nn.ParameterList(ragged_params(RAGGED, torch.float16, 1, 1.0) + ragged_params(RAGGED, torch.float32, 2, 1.0))
            self.key = torch.nn.ParameterList(ragged_params(RAGGED, torch.float16, 3, 1.0) + ragged_params(RAGGED, torch.float32, 4, 1.0))
            for p in self.key:
                p.requires_grad_(False)
            self.model_pairs = [(self.online, self.key)]
            self._ema_table = None
            self.contrast_momentum = 0.99

    m = Pairs()
    ref = [O.momentum_update(k.detach().cpu(), p.detach().cpu(), 0.99) for p, k in zip(m.online, m.key)]
    BirdPreTrainedModel._momentum_update(m)
    torch.cuda.synchronize()
    for k, r in zip(m.key, ref):
        if k.dtype == torch.float16:
            assert torch.equal(k.detach().cpu(), r), f"EMA fp16 numel {k.numel()}"
        else:
            within(k, r.double(), (2e-8 + 2e-6 * r.double().abs()) / R.SLACK, f"EMA fp32 numel {k.numel()}")

