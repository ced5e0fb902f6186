"""GPU tests of the fp16 hot path - fused attention (attention_f16.hip, attention_long_f16.hip), the GEMM epilogues and split-K
slab paths (gemm_f16.hip) and LayerNorm (norm_elem.hip) - each called with its own inputs through hmmc_amd.ops or the C-ABI and
compared ELEMENTWISE with a plain fp64 statement of the same op (tests/hotpath_ref.py, pinned by tests/test_hotpath_reference.py).

Entry points and the test that reaches each:
  hmmc_attention_f16_fwd / _bwd / _bwd_scaled   test_attention (every template x causal x H x regime), test_attention_persistent_loop,
                                                test_attention_benchmark_shapes
  hmmc_attention_f16_fwd_lead / _bwd_lead       test_attention (row n L against fp64; bit-identity stays with test_gpu_kernels.py)
  hmmc_gemm_f16, hmmc_gemm_f16_colsum_rows      test_gemm_epilogues (both tile configurations x kk / km x six epilogue sets x COLSUM),
                                                test_gemm_epilogue_with_reserved_cus
  hmmc_gemm_f16 without an epilogue: the fp32   test_splitk_single (128 and 256 tile, mm / kk / km, no split .. a shorter last split),
    split-K slabs + splitk_reduce_kernel        test_splitk_without_workspace, test_splitk_exact_integers
  hmmc_gemm_f16_wgrad_group (+ _workspace):     test_wgrad_group (1 - 4 problems, fp16 / fp32 / mixed outputs), .._with_reserved_cus,
    grouped slabs + splitk_reduce_group_kernel  .._exact_integers, .._statuses; test_zy_every_split_shape_ran closes the set of plans
  hmmc_layernorm_fwd / _bwd                     test_layernorm, test_layernorm_row_gather, test_layernorm_unsupported_widths

Every tolerance is a bound of hotpath_ref (first-order rounding bound of the kernel's arithmetic from the fp64 reference and the
inputs, allowed SLACK = 2 times); where the arithmetic is exact (BIAS, BIAS | RESID on integer data) the comparison is torch.equal.
A NaN fails every comparison, no element is left out.  test_hotpath_reference.py shows on the CPU that an emulation of each
kernel lies inside these bounds and that plausible kernel mistakes (test_slip_*) fall outside them.  Outputs sit between
sentinel-filled guard bands, the rows behind the last token are NaN, and every case runs twice for bit-identical results.
The last test prints the worst err / (SLACK bound) seen per family.

Split-K paths, worst err / (SLACK bound) measured on an MI355X (256 CUs), every test passing and every split shape reached:
  single launch  0.491 signed, 0.492 same-sign (both at one K-tile, where the fp16 rounding of the result is all there is)
  grouped, fp16  0.436 signed, 0.341 same-sign        grouped, fp32 (dW32)  0.002 signed, 0.010 same-sign
The fp32 figures are small because c U sum|ab| is a worst case over the signs of c rounding errors that in fact add like sqrt(c);
an fp16-rounded slab is 12 times outside it at the smallest grouped case (test_slip_wgrad)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import hotpath_ref as HR  # noqa: E402
from hmmc_amd import ops  # noqa: E402
from hmmc_amd._lib import STATUS, call, load, ptr, query, stream  # noqa: E402

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


# ============================================================================= fp32 split-K slabs: weight gradients

PLANS = set()                 # (path, nkt, ktps, splitk) of every launch whose split count was read through the ABI
OPAD = 64                     # NaN rows behind the last row of every operand: a whole K-tile
NAN = float("nan")


def operand(t, ld=None):
    """t [r, c] at leading dimension ld (default c) in a NaN-filled allocation with OPAD more rows behind it"""
    buf = torch.full((t.shape[0] + OPAD, ld or t.shape[1]), NAN, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf


def slab_workspace(nbytes):
    """the bytes the ABI asked for, filled with NaN (a slab that is summed without having been written shows), and a sentinel
    strip directly behind them"""
    buf = torch.full((nbytes // 4 + GUARD,), SENT, dtype=F32, device=DEV)
    buf[:nbytes // 4] = NAN
    return buf


def strip_intact(ws, nbytes, what):
    assert bool((ws[nbytes // 4:] == SENT).all()), f"{what}: the workspace was written past the {nbytes} bytes the ABI asked for"


def single_split(M, N, K):
    """-> ((nkt, ktps, splitk), workspace bytes) of an epilogue-free hmmc_gemm_f16 call: hmmc_gemm_f16_workspace reports
    splits x M x N x 4 bytes (0: no split), the host turns that count into K-tiles per split as HR.split_plan does"""
    nbytes = query("hmmc_gemm_f16_workspace", M, N, K)
    assert nbytes % (M * N * 4) == 0, (nbytes, M, N)
    return HR.split_plan(K, nbytes // (M * N * 4)), nbytes


def c_ints(v):
    return (ctypes.c_int * len(v))(*v)


def group_split(dims, T):
    """-> ((nkt, ktps, splitk), workspace bytes) of a grouped launch: hmmc_gemm_f16_wgrad_group_workspace reports
    splitk x sum Np Kp x 4 bytes; (None, 0) when the launch does not take these shapes"""
    nbytes = query("hmmc_gemm_f16_wgrad_group_workspace", c_ints([n for n, _ in dims]), c_ints([k for _, k in dims]), len(dims), T)
    elems = sum(n * k for n, k in dims)
    assert nbytes % (elems * 4) == 0, (nbytes, elems)
    return (HR.split_plan(T, nbytes // (elems * 4)) if nbytes else None), nbytes


def splitk_launch(layout, a_p, b_p, M, N, K, nbytes, no_workspace=False):
    """one epilogue-free hmmc_gemm_f16 call into a guarded C at ldc = N + PAD, with a NaN workspace of nbytes -> C [M, N]"""
    ldc = N + PAD
    cbuf = torch.full((GROWS + M + GROWS, ldc), SENT, dtype=F16, device=DEV)
    ws = slab_workspace(nbytes)
    call("hmmc_gemm_f16", ptr(a_p), ptr(b_p), ptr(cbuf[GROWS]), M, N, K, a_p.shape[1], b_p.shape[1], ldc, int(layout[0] == "k"),
         int(layout[1] == "k"), None, None, None, None, 0, None if no_workspace else ptr(ws), 0 if no_workspace else nbytes)
    torch.cuda.synchronize()
    assert bool((cbuf[:GROWS] == SENT).all()) and bool((cbuf[GROWS + M:] == SENT).all()), "C: rows outside [0, M) were written"
    assert bool((cbuf[GROWS:GROWS + M, N:] == SENT).all()), "C: pad columns were written"
    strip_intact(ws, nbytes, f"{layout} {M}x{N}x{K}")
    if no_workspace:
        assert bool(torch.isnan(ws[:nbytes // 4]).all())
    return cbuf[GROWS:GROWS + M, :N]


def single_operands(layout, dy, x):
    """dy [K, M], x [K, N] as the padded, NaN-trailed A and B of the layout: mm A = dy (lda = M + 8), B = x (ldb = N + 8);
    kk A = dy^T, B = x^T (lda = ldb = K + 8);  km A = dy^T, B = x"""
    a = dy if layout == "mm" else dy.t().contiguous()
    b = x.t().contiguous() if layout == "kk" else x
    return operand(a, a.shape[1] + PAD), operand(b, b.shape[1] + PAD)


def run_single(layout, M, N, K, regime, no_workspace=False):
    """-> (C of two bit-equal launches into fresh buffers, fp64 reference, |dy|^T |x|, plan)"""
    plan, nbytes = single_split(M, N, K)
    (dy,), (x,) = HR.wgrad_inputs(regime, K, [(M, N)], device=DEV)
    a_p, b_p = single_operands(layout, dy, x)
    c = splitk_launch(layout, a_p, b_p, M, N, K, nbytes, no_workspace)
    c2 = splitk_launch(layout, a_p, b_p, M, N, K, nbytes, no_workspace)
    assert torch.equal(c, c2), f"{layout} {M}x{N}x{K} {regime}: two runs differ"
    if not no_workspace:
        PLANS.add(("single",) + plan)
    return c, HR.wgrad(dy.double(), x.double()), HR.wgrad(dy.double().abs(), x.double().abs()), plan


# The path each shape reaches, from pick_cfg / gemm_f16_one on 256 CUs (the split itself is read through the ABI, and
# test_zy_every_split_shape_ran fails if the policy stops reaching one of them):
#   136 x 264: ragged in M and N, so the 128x128 tile: 2 x 3 tiles against 512 resident workgroups
#     K = 8      one partial K-tile, no split: the fp16 epilogue straight from the accumulators
#     K = 100    two K-tiles, the second with 36 rows, no split (a split needs 8 K-tiles)
#     K = 1000   16 K-tiles (the last with 40 rows): 4 splits of 4, the slabs and splitk_reduce_kernel writing through ldc
#     K = 1001   the same plan with a row count that is no multiple of 8 (accepted: see test_splitk_single)
#     K = 2120   34 K-tiles: 8 asked for, 5 K-tiles per split, 7 splits, the last with 4
#   1024 x 1024 x 6152: 16 tiles of 256x256 and 97 K-tiles; 16 (97 / 8) = 192 = 3/4 of the CUs, the least that keeps the 256x256
#     tile (16 x 12 with K < 6144 falls back to 128x128); 16 splits asked for, 7 K-tiles per split, 14 splits, the last with 6
#   kk / km 128 x 128 x 2048: one 128x128 tile, 32 K-tiles: 8 splits of 4 through the k-major staging
SPLITK_CASES = [("mm",) + c for c in HR.WGRAD_MM_CASES] + HR.WGRAD_KX_CASES
BIG_SPLIT = HR.WGRAD_MM_CASES[5]


@pytest.mark.parametrize("layout,M,N,K", SPLITK_CASES)
def test_splitk_single(layout, M, N, K):
    """hmmc_gemm_f16 without an epilogue, through the fp32 slabs where the host splits K: C within the bound of ITS split
    (64 ktps + splitk dependent additions, one fp16 rounding) on signed and on same-sign data.  Padded lda / ldb / ldc, NaN in the
    operand padding and in the 64 rows behind the operands (the K tail must come from the buffer descriptor's byte count, not
    from memory), NaN in the workspace, a sentinel strip behind it, guarded C, two launches for equal bits.
    K = 1001: the weight-gradient layout does NOT need a row count that is a multiple of 8 - gemm_f16_one checks lda, ldb, ldc, N
    and M only; rows are addressed at lda / ldb, every 16-byte piece lies inside one row, and the rows from K on are past a_bytes /
    b_bytes - so the call is accepted and held to the same bound (and to exactness in test_splitk_exact_integers)."""
    for regime in HR.WGRAD_REGIMES:
        c, ref, ab, (nkt, ktps, splitk) = run_single(layout, M, N, K, regime)
        within(c, ref, HR.wgrad_bound(ref, ab, K, ktps, splitk), f"{layout} {M}x{N}x{K} {regime} ({splitk} x {ktps} K-tiles)",
               f"splitk.single.{regime}")
    if (M, N, K) == BIG_SPLIT:
        # the 128x128 tile has 64 tiles here and two resident workgroups per CU: it would split at most 2 CUs / 64 ways
        assert query("hmmc_gemm_f16_workspace", M, N, K) // (M * N * 4) > 2 * cus() // 64, "not the 256x256 tile"


def test_splitk_without_workspace():
    """workspace = NULL on the 256x256 split shape: the host falls back to one split per tile; the result stays within the bound
    of a K-term dot product (c = K) and nothing but C is written (the NaN workspace that was NOT passed stays NaN)"""
    M, N, K = BIG_SPLIT
    for regime in HR.WGRAD_REGIMES:
        c, ref, ab, _ = run_single("mm", M, N, K, regime, no_workspace=True)
        within(c, ref, HR.wgrad_bound(ref, ab, K), f"mm {M}x{N}x{K} {regime} without a workspace", f"splitk.single.{regime}")


@pytest.mark.parametrize("M,N,K", [HR.WGRAD_MM_CASES[3], HR.WGRAD_MM_CASES[4], BIG_SPLIT])
def test_splitk_exact_integers(M, N, K):
    """both tile sizes (and the row count that is no multiple of 8) on integers whose slabs pass 2048: the fp32 path is exact, so
    C is the fp16 rounding of the exact sums, to the bit.  An fp16 slab or running sum would differ (test_slip_wgrad_exact_integers)."""
    c, ref, _, (nkt, ktps, splitk) = run_single("mm", M, N, K, "exact")
    assert splitk > 1 and 2048 < float(ref.max()) < 65504
    assert torch.equal(c, ref.half()), f"{int((c != ref.half()).sum())} of {c.numel()} elements differ"


def group_launch(dys_p, xs_p, dims, T, f32, nbytes, ws_bytes=None, dw32=None, dw=None):
    """one hmmc_gemm_f16_wgrad_group call: problem j leaves as fp32 into a guarded dW32[j] when j is in f32, else as fp16 into a
    guarded dW[j]; a problem with dW32[j] still gets a guarded, sentinel-filled dW[j], which must stay untouched.
    -> (status, [result views], all outputs untouched)"""
    n = len(dims)
    b16 = [guarded(d, F16) for d in dims]
    b32 = [guarded(d, F32) if j in f32 else None for j, d in enumerate(dims)]
    P = ctypes.c_void_p * n
    p16 = dw if dw is not None else [b[1].data_ptr() for b in b16]
    p32 = dw32 if dw32 is not None else [b[1].data_ptr() if b is not None else None for b in b32]
    ws = slab_workspace(nbytes)
    rc = load().hmmc_gemm_f16_wgrad_group(P(*[t.data_ptr() for t in dys_p]), P(*[t.data_ptr() for t in xs_p]), P(*p16),
                                          P(*p32) if (f32 or n > 1) else None, c_ints([d[0] for d in dims]), c_ints([d[1] for d in dims]),
                                          n, T, ptr(ws), nbytes if ws_bytes is None else ws_bytes, stream())
    torch.cuda.synchronize()
    for j in range(n):
        guards_intact(b16[j][0], f"dW[{j}]")
        if b32[j] is not None:
            guards_intact(b32[j][0], f"dW32[{j}]")
            assert bool((b16[j][1] == SENT).all()), f"dW[{j}] was written although dW32[{j}] takes the result"
    strip_intact(ws, nbytes, "grouped launch")
    untouched = all(bool((b[0] == SENT).all()) for b in b16 + b32 if b is not None) and bool(torch.isnan(ws[:nbytes // 4]).all())
    return rc, [b32[j][1] if b32[j] is not None else b16[j][1] for j in range(n)], untouched


def run_group(name, regime):
    """-> ([results of two bit-equal launches], dys, xs, plan) of HR.WGRAD_GROUP_CASES[name]"""
    dims, T, f32 = HR.WGRAD_GROUP_CASES[name]
    plan, nbytes = group_split(dims, T)
    assert plan is not None, f"{name}: the grouped launch does not take these shapes"
    dys, xs = HR.wgrad_inputs(regime, T, dims, device=DEV)
    dys_p, xs_p = [operand(t) for t in dys], [operand(t) for t in xs]
    rc, outs, _ = group_launch(dys_p, xs_p, dims, T, f32, nbytes)
    rc2, outs2, _ = group_launch(dys_p, xs_p, dims, T, f32, nbytes)
    assert rc == 0 and rc2 == 0, (rc, rc2)
    for j, (o, o2) in enumerate(zip(outs, outs2)):
        assert torch.equal(o, o2), f"{name} {regime}: problem {j} differs between two runs"
    PLANS.add(("group",) + plan)
    return outs, dys, xs, plan


def check_group(name, regime):
    dims, T, f32 = HR.WGRAD_GROUP_CASES[name]
    outs, dys, xs, (nkt, ktps, splitk) = run_group(name, regime)
    for j, (o, dy, x) in enumerate(zip(outs, dys, xs)):
        ref, ab = HR.wgrad(dy.double(), x.double()), HR.wgrad(dy.double().abs(), x.double().abs())
        half = j not in f32
        assert o.dtype == (F16 if half else F32)
        within(o, ref, HR.wgrad_bound(ref, ab, T, ktps, splitk, half),
               f"{name} {regime} problem {j} {dims[j]} T {T} {'fp16' if half else 'fp32'} ({splitk} x {ktps} K-tiles)",
               f"splitk.group.{'f16' if half else 'f32'}.{regime}")


# Grouped launches (HR.WGRAD_GROUP_CASES), 256x256 tiles only; the plan group_plan makes on 256 CUs:
#   min_f16    one 256x256 problem, 512 tokens = 8 K-tiles, the fewest the launch takes: 2 splits of 4; dW32 = NULL
#   two_f32    2 problems, 520 tokens = 9 K-tiles (the last with 8 rows): splits of 5 + 4; every problem fp32
#   three_mix  3 problems, 1000 tokens; problem 1 fp32
#   layer_f16  the four gradients of a layer at D = 256 (12 tiles), 512 tokens, every problem fp16 through an all-NULL dW32 array
#   layer_f32  the same at 1001 tokens (no multiple of 8: accepted, as in the single launch), every problem fp32
#   layer_mix  the same at 2120 tokens = 34 K-tiles with a shorter last split; problems 1 and 3 fp32: the tower's mix
#   wide_mix   4 problems of 1024 x 1280 (80 tiles), 512 tokens: the slab round trip outweighs a second split - one split, and
#              still slabs + the reduce
#   wide_1k_mix  the same at 1024 tokens: two splits (160 items in one round); with 100 CUs reserved (156 left) they would take
#              two rounds, and the plan is one split of 16 K-tiles (test_wgrad_group_with_reserved_cus)
@pytest.mark.parametrize("name", list(HR.WGRAD_GROUP_CASES))
def test_wgrad_group(name):
    """hmmc_gemm_f16_wgrad_group through the C-ABI: every problem, fp16 or fp32, within the bound of the launch's split on signed
    and on same-sign data (the fp32 results to c U relative there).  64 NaN rows behind every operand, NaN workspace + sentinel
    strip, guarded dW / dW32, an untouched dW[j] where dW32[j] is set, two launches for equal bits."""
    for regime in HR.WGRAD_REGIMES:
        check_group(name, regime)


def test_wgrad_group_with_reserved_cus():
    """hmmc_gemm_reserve_cus(100): the plan is made for the CUs that are left - another one than without the reservation, as the
    ABI reports it - and every problem stays within the bound of THAT plan"""
    name = "wide_1k_mix"
    dims, T, _ = HR.WGRAD_GROUP_CASES[name]
    lib = load()
    before = group_split(dims, T)
    try:
        assert lib.hmmc_gemm_reserve_cus(100) == 0
        assert group_split(dims, T) != before, f"the reservation leaves the plan {before} as it is"
        for regime in HR.WGRAD_REGIMES:
            check_group(name, regime)
    finally:
        assert lib.hmmc_gemm_reserve_cus(0) == 0
    assert group_split(dims, T) == before


def test_wgrad_group_exact_integers():
    """the tower's mix on integers whose slabs pass 2048: dW32 is the exact sum, dW its fp16 rounding, to the bit"""
    name = "layer_mix"
    dims, T, f32 = HR.WGRAD_GROUP_CASES[name]
    outs, dys, xs, (nkt, ktps, splitk) = run_group(name, "exact")
    assert splitk > 1
    for j, (o, dy, x) in enumerate(zip(outs, dys, xs)):
        ref = HR.wgrad(dy.double(), x.double())
        assert 2048 < float(ref.max()) < 65504
        if j in f32:
            assert torch.equal(o.double(), ref), f"dW32[{j}]: {int((o.double() != ref).sum())} elements differ"
        else:
            assert torch.equal(o, ref.half()), f"dW[{j}]: {int((o != ref.half()).sum())} elements differ"


def test_wgrad_group_statuses():
    """a status instead of a launch, and no output written: a workspace one byte short, a misaligned dW32[j], a problem without
    an output, fewer than 512 tokens"""
    dims, T = [(256, 256), (512, 256)], 512
    plan, nbytes = group_split(dims, T)
    assert plan is not None
    dys, xs = HR.wgrad_inputs("same", T, dims, device=DEV)
    dys_p, xs_p = [operand(t) for t in dys], [operand(t) for t in xs]
    rc, _, untouched = group_launch(dys_p, xs_p, dims, T, (1,), nbytes, ws_bytes=nbytes - 1)
    assert rc == STATUS["HMMC_ERR_WORKSPACE"] and untouched, (rc, untouched)
    w32 = guarded(dims[1], F32)
    rc, _, untouched = group_launch(dys_p, xs_p, dims, T, (), nbytes, dw32=[None, w32[1].data_ptr() + 4])
    assert rc == STATUS["HMMC_ERR_ARG"] and untouched and bool((w32[0] == SENT).all()), (rc, untouched)
    w16 = guarded(dims[0], F16)
    rc, _, untouched = group_launch(dys_p, xs_p, dims, T, (), nbytes, dw=[w16[1].data_ptr(), None], dw32=[None, None])
    assert rc == STATUS["HMMC_ERR_ARG"] and untouched and bool((w16[0] == SENT).all()), (rc, untouched)
    assert group_split(dims, 504) == (None, 0)
    rc, _, untouched = group_launch(dys_p, xs_p, dims, 504, (1,), nbytes)
    assert rc == STATUS["HMMC_ERR_UNSUPPORTED"] and untouched, (rc, untouched)
    rc, outs, _ = group_launch(dys_p, xs_p, dims, T, (1,), nbytes)          # and the same arguments, right, are taken
    assert rc == 0 and not bool(torch.isnan(outs[1]).any())


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


def test_zy_every_split_shape_ran():
    """from the split counts read through the ABI: the launches above reached a grouped launch with ONE split (slabs and the
    reduce all the same), splits of equal length, a shorter last split, and items of one or two K-tiles (which only an unsplit
    launch has: both host policies keep four K-tiles per split).  A change of the split policy that stops reaching one of them
    fails here instead of silently testing less (run the module as a whole)."""
    assert any(path == "group" and splitk == 1 for path, nkt, ktps, splitk in PLANS), sorted(PLANS)
    for path in ("single", "group"):
        mine = [(nkt, ktps, splitk) for p, nkt, ktps, splitk in PLANS if p == path]
        assert any(splitk > 1 and splitk * ktps == nkt for nkt, ktps, splitk in mine), f"{path}: no equal splits in {sorted(PLANS)}"
        assert any(splitk > 1 and splitk * ktps > nkt for nkt, ktps, splitk in mine), f"{path}: no shorter last split in {sorted(PLANS)}"
    assert any(ktps <= 2 for _, _, ktps, _ in PLANS), sorted(PLANS)
    print("splitk-coverage (path, K-tiles, K-tiles per split, splits): " + ", ".join(str(p) for p in sorted(PLANS)))


def test_zz_report_worst_ratios():
    """not a check: the worst err / (SLACK bound) against fp64 per family, for the record (run with -s)"""
    for fam in ("splitk.single", "splitk.group.f16", "splitk.group.f32"):
        for regime in HR.WGRAD_REGIMES:
            assert f"{fam}.{regime}" in WORST, f"no bounded comparison ran on {fam}, {regime} data"
    for fam in sorted(WORST):
        print(f"hotpath-worst {fam}: {WORST[fam]:.3f}")
