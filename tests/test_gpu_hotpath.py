"""GPU tests of the fp16 hot path - fused attention (attention_f16.hip, attention_long_f16.hip), the GEMM epilogues (gemm_f16.hip)
and LayerNorm (norm_elem.hip) - each called with its own inputs through hmmc_amd.ops or the C-ABI and compared ELEMENTWISE with a
plain fp64 statement of the same op (tests/hotpath_ref.py, pinned by tests/test_hotpath_reference.py).

Entry points and the test that reaches each:
  hmmc_attention_f16_fwd / _bwd / _bwd_scaled   test_attention (every template x causal x H x regime), test_attention_persistent_loop,
                                                test_attention_benchmark_shapes
  hmmc_attention_f16_fwd_lead / _bwd_lead       test_attention (row n L against fp64; bit-identity stays with test_gpu_kernels.py)
  hmmc_gemm_f16, hmmc_gemm_f16_colsum_rows      test_gemm_epilogues (both tile configurations x kk / km x six epilogue sets x COLSUM),
                                                test_gemm_epilogue_with_reserved_cus
  hmmc_layernorm_fwd / _bwd                     test_layernorm, test_layernorm_row_gather, test_layernorm_unsupported_widths

Every tolerance is a bound of hotpath_ref (first-order rounding bound of the kernel's arithmetic from the fp64 reference and the
inputs, allowed SLACK = 2 times); where the arithmetic is exact (BIAS, BIAS | RESID on integer data) the comparison is torch.equal.
A NaN fails every comparison, no element is left out.  test_hotpath_reference.py shows on the CPU that an emulation of each
kernel lies inside these bounds and that plausible kernel mistakes (test_slip_*) fall outside them.  Outputs sit between
sentinel-filled guard bands, the rows behind the last token are NaN, and every case runs twice for bit-identical results.
The last test prints the worst err / (SLACK bound) seen per family."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import hotpath_ref as HR  # noqa: E402
from hmmc_amd import ops  # noqa: E402
from hmmc_amd._lib import call, load, ptr, query  # noqa: E402

DEV = "cuda"
D64 = torch.float64
F16, F32 = torch.float16, torch.float32
SENT = -777.0                 # exact in fp16 and fp32
GUARD = 64                    # elements in front of and behind every guarded output
WORST = {}                    # family -> worst err / (SLACK bound) against fp64


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def within(got, ref, bound, what, family):
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
    lim = torch.as_tensor(HR.SLACK * bound, dtype=D64, device=err.device).expand_as(err).masked_fill(inf, 0.0)
    bad = ~(err <= lim)
    ratio = float((err / lim).nan_to_num(0.0).max()) if err.numel() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"hotpath-ratio {family} {what}: {ratio:.3f}")
    if bool(bad.any()):
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside the bound; worst err / (SLACK bound) "
                             f"{ratio:.2f}, max err {float(err.max()):.3e}, first at {idx}: got {float(got[tuple(idx)]):.6g} "
                             f"ref {float(ref[tuple(idx)]):.6g}")


def guarded(shape, dtype):
    """a sentinel-filled output inside a larger sentinel-filled allocation -> (allocation, view)"""
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, what):
    n = buf.numel() - 2 * GUARD
    assert bool((buf[:GUARD] == SENT).all()), f"{what}: bytes in front of the buffer were written"
    assert bool((buf[GUARD + n:] == SENT).all()), f"{what}: bytes behind the buffer were written"


def poisoned(t, extra=8):
    """t followed by `extra` rows of NaN in the same allocation"""
    buf = torch.full((t.shape[0] + extra, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf


# ============================================================================= attention

ATTN_L = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 50, 63, 64, 65, 77, 96, 97, 128, 129, 160, 161, 192, 193, 197, 224, 225, 255, 256]
# nseq H in {1, 3, 7} at H = 1 (short forward: 4 waves per workgroup, short backward: 2), 12 or 36 pairs at H = 12; nseq odd
ATTN_CASES = [(L, H, (1, 3, 7)[i % 3] if H == 1 else (1, 3)[i % 2], causal)
              for i, L in enumerate(ATTN_L) for H in (1, 12) for causal in (False, True)]


def run_attention(qkv_p, dout_p, stat, nseq, L, H, causal):
    """forward, backward (with bias partials) and row-scaled backward through the C-ABI into guarded outputs"""
    T, D = nseq * L, 64 * H
    bufs = {name: guarded(shape, dt) for name, shape, dt in
            (("out", (T, D), F16), ("lse", (nseq, H, L), F32), ("dqkv", (T, 3 * D), F16), ("dbias", (nseq, 3 * D), F32),
             ("scaled", (T, 3 * D), F16), ("dbias_scaled", (nseq, 3 * D), F32))}
    v = {k: b[1] for k, b in bufs.items()}
    call("hmmc_attention_f16_fwd", ptr(qkv_p), ptr(v["out"]), ptr(v["lse"]), nseq, L, H, int(causal))
    call("hmmc_attention_f16_bwd", ptr(qkv_p), ptr(v["out"]), ptr(v["lse"]), ptr(dout_p), ptr(v["dqkv"]), ptr(v["dbias"]), nseq, L, H,
         int(causal))
    call("hmmc_attention_f16_bwd_scaled", ptr(qkv_p), ptr(v["out"]), ptr(v["lse"]), ptr(dout_p), ptr(v["scaled"]),
         ptr(v["dbias_scaled"]), ptr(stat), nseq, L, H, int(causal))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        guards_intact(b[0], f"attention {k}")
    return v


def check_attention(regime, nseq, L, H, causal, lead, chunk=None):
    T, D = nseq * L, 64 * H
    tag = f"{regime} nseq {nseq} L {L} H {H} causal {int(causal)}"
    qkv, dout = HR.attention_inputs(regime, nseq, L, H, causal, device=DEV)
    if nseq * H > 1:                             # pairs with different (n, h) have different data: a stale result cannot coincide
        k = HR.heads(qkv[:, D:2 * D], nseq, L, H).reshape(nseq * H, -1)
        assert not bool((k[1:] == k[:-1]).all(1).any())
    stat = torch.rand(T, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(L)) + 0.5
    qkv_p, dout_p = poisoned(qkv), poisoned(dout)
    res = run_attention(qkv_p, dout_p, stat, nseq, L, H, causal)
    again = run_attention(qkv_p, dout_p, stat, nseq, L, H, causal)
    for k in res:
        assert torch.equal(res[k], again[k]), f"{tag}: {k} differs between two runs"
    chunk = chunk or nseq
    for n0 in range(0, nseq, chunk):
        n = min(chunk, nseq - n0)
        r, s = slice(n0 * L, (n0 + n) * L), slice(n0, n0 + n)
        q64, d64, st64 = qkv[r].double(), dout[r].double(), stat[r].double()
        out_ref, lse_ref = HR.attention(q64, n, L, H, causal)
        g_ref = HR.attention_bwd(q64, d64, n, L, H, causal)
        b = HR.attention_bounds(q64, d64, n, L, H, causal, st64)
        within(res["out"][r], out_ref, b["out"], f"{tag}: out", "attention")
        within(res["lse"][s], lse_ref, b["lse"], f"{tag}: lse", "attention")
        within(res["dqkv"][r], g_ref, b["dqkv"], f"{tag}: dqkv", "attention")
        within(res["dbias"][s], HR.dbias_partial(g_ref, n, L), b["dbias"], f"{tag}: dbias_partial", "attention")
        within(res["scaled"][r], HR.row_scaled(g_ref, st64), b["scaled"], f"{tag}: row-scaled dqkv", "attention")
        within(res["dbias_scaled"][s], HR.dbias_partial(g_ref, n, L), b["dbias"], f"{tag}: dbias_partial (scaled)", "attention")
        if lead:                                 # query 0 of every sequence against fp64 directly (nseq is one chunk here)
            rows0 = torch.arange(nseq, device=DEV) * L
            out1, lse1 = ops.attention_f16_fwd_lead(qkv_p[:T], nseq, L, H, causal)
            within(out1[rows0], out_ref[rows0], b["out"][rows0], f"{tag}: lead out", "attention")
            within(lse1[:, :, 0], lse_ref[:, :, 0], b["lse"][:, :, 0], f"{tag}: lead lse", "attention")
            dlead_p = torch.full_like(dout_p, float("nan"))
            dlead_p[rows0] = dout[rows0]
            d0 = torch.zeros_like(d64)
            d0[rows0] = d64[rows0]
            g0 = HR.attention_bwd(q64, d0, nseq, L, H, causal)
            b0 = HR.attention_bounds(q64, d0, nseq, L, H, causal)
            d1, p1 = ops.attention_f16_bwd_lead(qkv_p[:T], res["lse"], dlead_p[:T], nseq, L, H, causal, want_dbias=True, out=res["out"])
            within(d1[:, D:], g0[:, D:], b0["dqkv"][:, D:], f"{tag}: lead dK | dV", "attention")
            within(d1[rows0, :D], g0[rows0, :D], b0["dqkv"][rows0, :D], f"{tag}: lead dQ", "attention")
            within(p1, HR.dbias_partial(g0, nseq, L), b0["dbias"], f"{tag}: lead dbias_partial", "attention")


@pytest.mark.parametrize("L,H,nseq,causal", ATTN_CASES)
def test_attention(L, H, nseq, causal):
    """Both short templates (L <= 32, <= 64) and the six long ones (ktl = 6 .. 16), each with a full, a partial and a wholly padded
    last key tile, forward and backward, causal and not, in the three input regimes: out, lse, dq | dk | dv, the bias partials, the
    row-scaled gradient and the query-0 variants against fp64 within their bounds."""
    for regime in HR.ATTN_REGIMES:
        check_attention(regime, nseq, L, H, causal, lead=True)


@pytest.mark.parametrize("L,causal", [(197, False), (97, False), (97, True)])
def test_attention_persistent_loop(L, causal):
    """2 CUs + 37 (sequence, head) pairs: every workgroup of the long backward's persistent grid walks two or three pairs, and the
    last round is partial."""
    nseq = 2 * cus() + 37
    for regime in HR.ATTN_REGIMES:
        check_attention(regime, nseq, L, 1, causal, lead=False, chunk=128)


@pytest.mark.parametrize("nseq,L,H,chunk", [(3072, 50, 12, 512), (300, 197, 12, 50)])
def test_attention_benchmark_shapes(nseq, L, H, chunk):
    """The frame tower's 3072 x 50 x 12 and ViT-B/16's 300 x 197 x 12 (what the bit-identity test of the query-0 kernels compares
    with), once per regime, the fp64 reference on the device in chunks of sequences."""
    for regime in HR.ATTN_REGIMES:
        check_attention(regime, nseq, L, H, False, lead=False, chunk=chunk)
        torch.cuda.empty_cache()


# ============================================================================= fp16 GEMM epilogues

GEMM_SETS = {"bias": HR.EPI_BIAS, "bias_resid": HR.EPI_BIAS | HR.EPI_RESID, "bias_qgelu": HR.EPI_BIAS | HR.EPI_QGELU,
             "bias_qgelu_save": HR.EPI_BIAS | HR.EPI_QGELU | HR.EPI_SAVE_DGELU, "dgelu": HR.EPI_DGELU, "mulaux": HR.EPI_MULAUX}
EXACT_SETS = ("bias", "bias_resid")
# (tile the id names, M, N, K): K = 64 (pipeline prologue and drain only) in both configurations, ragged M and N on the 256 tile
GEMM_SHAPES = [("big", 16384, 768, 64), ("big", 16384, 768, 768), ("big", 5000, 2312, 64), ("big", 5000, 2312, 768),
               ("big", 16384, 3072, 768), ("big", 16384, 768, 3072),
               ("small", 1000, 384, 256), ("small", 130, 136, 64), ("small", 130, 136, 192), ("small", 4096, 768, 768)]
PAD = 8                       # lda = K + 8, ldb = (K or N) + 8, ldc = N + 8
GROWS = 4                     # guard rows in front of and behind C / aux_out


def padded(t, fill=float("nan")):
    """t [r, c] as the leading columns of a [r, c + PAD] allocation whose pad columns hold `fill`"""
    buf = torch.full((t.shape[0], t.shape[1] + PAD), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, resid_p, auxin_p, colsum):
    """one hmmc_gemm_f16 call with padded strides into guarded, sentinel-filled C / aux_out / workspace -> (C, aux_out, partial)"""
    ldc = N + PAD
    cbuf = torch.full((GROWS + M + GROWS, ldc), SENT, dtype=F16, device=DEV)
    abuf = torch.full((GROWS + M + GROWS, ldc), SENT, dtype=F16, device=DEV) if fl & HR.EPI_QGELU else None
    rows = query("hmmc_gemm_f16_colsum_rows", M, N, K)
    ws = torch.full((rows * N + GUARD,), SENT, dtype=F32, device=DEV) if colsum else None
    call("hmmc_gemm_f16", ptr(a_p), ptr(b_p), ptr(cbuf[GROWS]), M, N, K, a_p.shape[1], b_p.shape[1], ldc, 1, int(kk),
         ptr(bias) if fl & HR.EPI_BIAS else None, ptr(resid_p) if fl & HR.EPI_RESID else None,
         ptr(abuf[GROWS]) if abuf is not None else None, ptr(auxin_p) if fl & (HR.EPI_DGELU | HR.EPI_MULAUX) else None,
         fl | (HR.EPI_COLSUM if colsum else 0), ptr(ws), rows * N * 4 if colsum else 0)
    torch.cuda.synchronize()
    for buf, what in ((cbuf, "C"), (abuf, "aux_out")):
        if buf is None:
            continue
        assert bool((buf[:GROWS] == SENT).all()) and bool((buf[GROWS + M:] == SENT).all()), f"{what}: rows outside [0, M) were written"
        assert bool((buf[GROWS:GROWS + M, N:] == SENT).all()), f"{what}: pad columns were written"
    if colsum:
        assert bool((ws[rows * N:] == SENT).all()), "the workspace past colsum_rows * N floats was written"
    return cbuf[GROWS:GROWS + M, :N], (abuf[GROWS:GROWS + M, :N] if abuf is not None else None), (ws[:rows * N].view(rows, N) if colsum else None)


def check_colsum(part, c, M, N, K, big, tag):
    block = 128 if big else 64
    rows = query("hmmc_gemm_f16_colsum_rows", M, N, K)
    assert rows == 2 * ((M + 2 * block - 1) // (2 * block)) and part.shape[0] == rows, (rows, part.shape)
    c64 = c.double()
    ref, bound = HR.colsum_blocks(c64, block), HR.colsum_bound(c64, block)
    zero = torch.zeros(rows - ref.shape[0], N, dtype=D64, device=DEV)        # row blocks wholly past M hold zeros
    within(part, torch.cat([ref, zero]), torch.cat([bound, zero]), f"{tag}: COLSUM partial rows", "gemm.colsum")
    within(part.double().sum(0), c64.sum(0), bound.sum(0), f"{tag}: sum of the COLSUM partial rows", "gemm.colsum")


@pytest.mark.parametrize("layout", ["kk", "km"])
@pytest.mark.parametrize("tile,M,N,K", GEMM_SHAPES)
def test_gemm_epilogues(tile, M, N, K, layout):
    """{BIAS, BIAS|RESID, BIAS|QGELU, BIAS|QGELU|SAVE_DGELU, DGELU, MULAUX} with and without COLSUM, forward (kk) and data-gradient
    (km) layouts, on the tile configuration the id names; lda > K, ldb padded, ldc > N shared by C, resid, aux_in and aux_out."""
    big = tile == "big"
    assert HR.pick_big_tile(M, N, cus()) == big, f"{M} x {N} does not select the {tile} tile on {cus()} CUs"
    kk = layout == "kk"
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    bshape = (N, K) if kk else (K, N)

    def product(a, b):
        return a @ (b.t() if kk else b)
    # ---- exact sets: integer data, h passes 2048 so that both fp16 roundings of BIAS | RESID matter
    a = torch.randint(-2, 3, (M, K), generator=g, device=DEV).half()
    b = torch.randint(-2, 3, bshape, generator=g, device=DEV).half()
    bias = torch.randint(-3000, 3001, (N,), generator=g, device=DEV).half()
    resid = torch.randint(-3000, 3001, (M, N), generator=g, device=DEV).half()
    a_p, b_p, resid_p = padded(a), padded(b), padded(resid)
    acc = product(a.double(), b.double())
    assert float(product(a.double().abs(), b.double().abs()).max()) < 2 ** 24      # every partial sum is exact in fp32
    for name in EXACT_SETS:
        fl = GEMM_SETS[name]
        ref = HR.gemm_epilogue(acc, bias.double(), resid.double(), None, fl, rounded=True)[0]
        c, _, _ = gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, resid_p, None, False)
        assert torch.equal(c.double(), ref), f"{name} {layout}: {int((c.double() != ref).sum())} elements differ"
        c2, _, part = gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, resid_p, None, True)
        assert torch.equal(c2, c), f"{name} {layout}: C differs with COLSUM"
        check_colsum(part, c2, M, N, K, big, f"{name} {layout} {M}x{N}x{K}")
    del acc, ref
    # ---- random data: acc ~ N(0, 1), bias and the DGELU operand spread over [-8, 8]: both tails of the sigmoid
    a = torch.randn(M, K, generator=g, device=DEV).half()
    b = (torch.randn(bshape, generator=g, device=DEV) / K ** 0.5).half()
    bias = (torch.rand(N, generator=g, device=DEV) * 16 - 8).half()
    spread = (torch.rand(M, N, generator=g, device=DEV) * 16 - 8).half()
    factor = torch.randn(M, N, generator=g, device=DEV).half()
    a_p, b_p = padded(a), padded(b)
    acc = product(a.double(), b.double())
    eacc = HR.gemm_acc_bound(product(a.double().abs(), b.double().abs()), K)
    for name, fl in GEMM_SETS.items():
        if name in EXACT_SETS:
            continue
        aux_in = spread if fl & HR.EPI_DGELU else factor
        auxin_p = padded(aux_in)
        tag = f"{name} {layout} {M}x{N}x{K}"
        ref, ref_aux = HR.gemm_epilogue(acc, bias.double(), None, aux_in.double(), fl)
        bnd, bnd_aux = HR.gemm_epilogue_bounds(acc, eacc, bias.double(), None, aux_in.double(), fl)
        c, aux, _ = gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, None, auxin_p, False)
        within(c, ref, bnd, f"{tag}: out", "gemm")
        if ref_aux is not None:
            within(aux, ref_aux, bnd_aux, f"{tag}: aux_out", "gemm")
        del ref, bnd, ref_aux, bnd_aux
        c2, aux2, part = gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, None, auxin_p, True)
        assert torch.equal(c2, c) and (aux is None or torch.equal(aux2, aux)), f"{tag}: results differ with COLSUM"
        check_colsum(part, c2, M, N, K, big, tag)
        c3, _, part3 = gemm_launch(a_p, b_p, M, N, K, kk, fl, bias, None, auxin_p, True)
        assert torch.equal(c3, c2) and torch.equal(part3, part), f"{tag}: two runs differ"
    torch.cuda.empty_cache()


def test_gemm_epilogue_with_reserved_cus():
    """hmmc_gemm_reserve_cus(16) on a 256-tile epilogue shape: the same bits (C, aux_out and the COLSUM partials)"""
    M, N, K = 16384, 768, 768
    assert HR.pick_big_tile(M, N, cus()) and HR.pick_big_tile(M, N, cus() - 16)
    g = torch.Generator(device=DEV).manual_seed(5)
    a_p = padded(torch.randn(M, K, generator=g, device=DEV).half())
    b_p = padded((torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).half())
    bias = (torch.rand(N, generator=g, device=DEV) * 16 - 8).half()
    fl = GEMM_SETS["bias_qgelu_save"]
    c, aux, part = gemm_launch(a_p, b_p, M, N, K, True, fl, bias, None, None, True)
    lib = load()
    try:
        assert lib.hmmc_gemm_reserve_cus(16) == 0
        c2, aux2, part2 = gemm_launch(a_p, b_p, M, N, K, True, fl, bias, None, None, True)
    finally:
        assert lib.hmmc_gemm_reserve_cus(0) == 0
    assert torch.equal(c, c2) and torch.equal(aux, aux2) and torch.equal(part, part2)


# ============================================================================= LayerNorm

LN_CASES = [(F16, D, 1e-5) for D in (8, 64, 128, 512, 768, 1024)] + [(F32, D, 1e-12) for D in (4, 512, 1024)]


def check_layernorm(tag, dtype, eps, x, gamma, beta, dy, dres, got):
    x64, g64, b64, dy64 = (t.double() for t in (x, gamma, beta, dy))
    dr64 = dres.double() if dres is not None else None
    y, mean, rstd = HR.layernorm(x64, g64, b64, eps)
    dx, dg, db = HR.layernorm_bwd(x64, g64, b64, eps, dy64, dr64)
    b = HR.layernorm_bounds(x64, g64, b64, eps, dy64, dr64, dtype == F16)
    fam = "layernorm.f16" if dtype == F16 else "layernorm.f32"
    for name, ref in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dg), ("dbeta", db), ("dxsum", dx.sum(0))):
        within(got[name], ref, b[name], f"{tag}: {name}", fam)


@pytest.mark.parametrize("nrows", [1, 3, 1003])
@pytest.mark.parametrize("dtype,D,eps", LN_CASES)
def test_layernorm(dtype, D, eps, nrows):
    """y, mean, rstd, dx + dres, dgamma, dbeta and the fused dx column sums against fp64, in the four row regimes"""
    for regime in HR.LN_REGIMES:
        x, gamma, beta, dy, dres = HR.layernorm_inputs(regime, nrows, D, dtype, device=DEV)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
        dx, dg, db, cs = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_colsum=True)
        got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db, dxsum=cs)
        check_layernorm(f"{regime} {dtype} rows {nrows} D {D}", dtype, eps, x, gamma, beta, dy, dres, got)
        y2, mean2, rstd2 = ops.layernorm_fwd(x, gamma, beta, eps)
        dx2, dg2, db2, cs2 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_colsum=True)
        for u, v in ((y, y2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dg, dg2), (db, db2), (cs, cs2)):
            assert torch.equal(u, v), "two runs differ"


@pytest.mark.parametrize("dtype,D,eps", [(F16, 768, 1e-5), (F32, 512, 1e-12)])
def test_layernorm_row_gather(dtype, D, eps):
    """row_index: every L-th row of a token-major buffer is normalised; the backward writes those rows of dx and no other"""
    n, L = 37, 5
    for regime in HR.LN_REGIMES:
        xa, gamma, beta, _, _ = HR.layernorm_inputs(regime, n * L, D, dtype, device=DEV)
        if regime == "outlier":
            xa[L] = xa[0]                                 # the outlier row among the addressed ones too
        dy = HR.layernorm_inputs("normal", n, D, dtype, seed=1, device=DEV)[3]
        idx = (torch.arange(n, device=DEV, dtype=torch.int32) * L).contiguous()
        y, mean, rstd = ops.layernorm_fwd(xa, gamma, beta, eps, row_index=idx)
        dxa = torch.full_like(xa, SENT)
        dx, dg, db, cs = ops.layernorm_bwd(dy, xa, gamma, mean, rstd, row_index=idx, dx=dxa, want_colsum=True)
        rest = torch.ones(n * L, dtype=torch.bool, device=DEV)
        rest[idx.long()] = False
        assert bool((dxa[rest] == SENT).all()), "rows that are not addressed were written"
        got = dict(y=y, mean=mean, rstd=rstd, dx=dxa[idx.long()], dgamma=dg, dbeta=db, dxsum=cs)
        check_layernorm(f"gather {regime} {dtype} D {D}", dtype, eps, xa[idx.long()], gamma, beta, dy, None, got)


@pytest.mark.parametrize("D", [1032, 12])
def test_layernorm_unsupported_widths(D):
    """wider than the kernels' 1024 columns, or not a multiple of the 8 halves a lane moves: a status code, no launch"""
    x = torch.zeros(8, D, dtype=F16, device=DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.layernorm_fwd(x, gamma, beta, 1e-5)
    stat = torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.layernorm_bwd(x, x, gamma, stat, stat)


def test_zz_report_worst_ratios():
    """not a check: the worst err / (SLACK bound) against fp64 per family, for the record (run with -s)"""
    for fam in sorted(WORST):
        print(f"hotpath-worst {fam}: {WORST[fam]:.3f}")
