"""CPU checks of tests/gemm_f32_ref.py, the fp64 statement and rounding bound behind tests/test_gpu_gemm_f32.py:
  * the statement is pinned to F.linear and the oracle's QuickGELU in fp64, with strided operands;
  * the bound is not too tight: an fp32 emulation of the kernels' summation - four K-interleaved chains meeting as (0 + 1) + (2 + 3),
    and one in-order chain - lies inside SLACK x bound for every epilogue set in both random regimes, and equals the fp64 result on
    integer operands wherever the GPU test asks for equality;
  * the bound is not too loose (test_slip_*): each plausible kernel mistake of gemm_f32_ref.SLIPS falls outside the bound on random
    operands and / or breaks equality on integer operands, as SLIPS states per mistake;
  * hmmc_gemm_f32_plan (host only; the library loads without a GPU) sends every row of gemm_f32_ref.CASES to the instantiation the
    row names on a 256-CU device, the rows reach all 37 instantiations and both store paths of every family, and the query's
    error statuses are those of hmmc_gemm_f32's argument checks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_f32_ref as GR
from oracle import hmmc_oracle as O

D64 = torch.float64
ALL_SETS = GR.EPI_SETS + (GR.INT_SET,)
M_, N_, K_, LDC_ = 37, 45, 150, 52             # ragged in every 16 / 32 / 64 tile, K a partial 16-deep step; ldc > N


def build(regime, name, M=M_, N=N_, K=K_, ldc=LDC_, seed=0):
    """one problem in fp32 with operands at general strides -> dict of fp32 views and their flat buffers"""
    a, b = GR.operands(regime, M, N, K, seed=seed, extra_k=1)
    bias, resid, aux = GR.epilogue_operands(regime, M, N, seed=seed)
    g = torch.Generator().manual_seed(seed + 99)
    fill = (lambda n: torch.randint(-5, 6, (n,), generator=g).float()) if regime == "int" else (lambda n: torch.randn(n, generator=g))
    rbuf, xbuf = fill(M * ldc), fill(M * ldc)                                  # finite gap columns: "ld_n" reads them
    GR.strided(rbuf, M, N, ldc, 1, 0).copy_(resid)
    GR.strided(xbuf, M, N, ldc, 1, 0).copy_(aux)
    return dict(a=a[:, :K], b=b[:K], tail=(a[:, K], b[K]), bias=bias, K=K,
                resid=GR.strided(rbuf, M, N, ldc, 1, 0), aux=GR.strided(xbuf, M, N, ldc, 1, 0),
                resid_n=GR.strided(rbuf, M, N, N, 1, 0), aux_n=GR.strided(xbuf, M, N, N, 1, 0))


def ref64(p, flags, alpha, slip=None):
    d = lambda t: t.double()     # noqa: E731
    return GR.reference(d(p["a"]), d(p["b"]), alpha, flags, d(p["bias"]), d(p["resid"]), d(p["aux"]), slip=slip,
                        tail=(d(p["tail"][0]), d(p["tail"][1])), resid_n=d(p["resid_n"]), aux_n=d(p["aux_n"]))


def bounds64(p, flags, alpha):
    out, h, acc, absprod = ref64(p, flags, alpha)
    N = p["b"].shape[1]
    return out, h, GR.bounds(acc, absprod, p["K"], alpha, flags, p["bias"][:N].double(), p["resid"].double(), p["aux"].double())


# ============================================================================= the statement is pinned

def test_reference_is_linear_and_the_oracle_quickgelu():
    p = build("normal", "pin")
    a, b, bias, N = p["a"].double(), p["b"].double(), p["bias"].double(), N_
    lin = F.linear(a, b.t().contiguous(), bias[:N])
    out, h, acc, absprod = ref64(p, GR.EPI_BIAS | GR.EPI_QGELU, 1.0)
    assert torch.allclose(h, lin, rtol=0, atol=1e-12) and torch.allclose(out, O.quick_gelu(lin), rtol=0, atol=1e-12)
    assert torch.allclose(ref64(p, GR.EPI_BIAS | GR.EPI_RELU | GR.EPI_RESID, 1.0)[0], F.relu(lin) + p["resid"].double(), rtol=0, atol=1e-12)
    assert torch.allclose(ref64(p, GR.EPI_BIAS, 100.0)[0], 100.0 * (a @ b) + bias[:N], rtol=0, atol=1e-10)
    x = p["aux"].double().clone().requires_grad_()
    O.quick_gelu(x).sum().backward()                                           # QuickGELU' by autograd
    assert torch.allclose(ref64(p, GR.EPI_DGELU, 1.0)[0], (a @ b) * x.grad, rtol=0, atol=1e-11)
    assert torch.equal(absprod, a.abs() @ b.abs()) and torch.equal(acc, a @ b)
    # strided views: both orientations of an operand inside a padded, offset allocation give the same product
    buf = torch.full((7 + K_ * (M_ + 3),), float("nan"), dtype=D64)
    GR.strided(buf, M_, K_, 1, M_ + 3, 7).copy_(a)
    assert torch.equal(GR.strided(buf, M_, K_, 1, M_ + 3, 7) @ b, a @ b)


# ============================================================================= the bound is not too tight

@pytest.mark.parametrize("waves", [4, 1])
@pytest.mark.parametrize("regime", ["normal", "range"])
@pytest.mark.parametrize("name,flags,alpha", ALL_SETS)
def test_emulation_inside_bounds(name, flags, alpha, regime, waves):
    p = build(regime, name, seed=waves)
    out, h, (b_out, b_h) = bounds64(p, flags, alpha)
    got, got_h = GR.emulate(p["a"], p["b"], alpha, flags, p["bias"][:N_], p["resid"], p["aux"], waves=waves)
    r_out, r_h = GR.within_ratio(got, out, b_out), GR.within_ratio(got_h, h, b_h)
    print(f"gemm-f32-emulation {name} {regime} waves {waves}: out {r_out:.3f} aux_out {r_h:.3f}")
    assert r_out <= 1.0 and r_h <= 1.0, (name, regime, waves, r_out, r_h)
    assert r_out > 1e-3 or name in GR.EXACT_SETS, "a bound a thousand times the emulation's error checks nothing"


@pytest.mark.parametrize("waves", [4, 1])
@pytest.mark.parametrize("name,flags,alpha", [s for s in ALL_SETS if s[0] in GR.EXACT_SETS])
def test_emulation_exact_on_integers(name, flags, alpha, waves):
    p = build("int", name)
    out, h, _, _ = ref64(p, flags, alpha)
    got, got_h = GR.emulate(p["a"], p["b"], alpha, flags, p["bias"][:N_], p["resid"], p["aux"], waves=waves)
    assert torch.equal(got.double(), out) and torch.equal(got_h.double(), h)


# ============================================================================= the bound is not too loose

@pytest.mark.parametrize("slip", sorted(GR.SLIPS))
def test_slip_is_detected(slip):
    sets, checks = GR.SLIPS[slip]
    by_name = {s[0]: s for s in ALL_SETS}
    for name in sets:
        _, flags, alpha = by_name[name]
        if "bound" in checks and name != GR.INT_SET[0]:
            for regime in ("normal", "range"):
                p = build(regime, name)
                out, h, (b_out, _) = bounds64(p, flags, alpha)
                assert GR.detects(out, ref64(p, flags, alpha, slip)[0], b_out), f"{slip} on {name} ({regime}) stays inside the bound"
        if "equal" in checks and name in GR.EXACT_SETS:
            p = build("int", name)
            assert not torch.equal(ref64(p, flags, alpha)[0], ref64(p, flags, alpha, slip)[0]), f"{slip} on {name}: equal on integers"
    assert any(n in GR.EXACT_SETS for n in sets) or "equal" not in checks


def test_every_slip_is_caught_by_a_launch_every_case_makes():
    """the integer launch (alpha = 2, bias, residual) and the plain random launch run on EVERY row of the case table: together they
    see every mistake but the two that need an activation"""
    seen = {s for s, (sets, _) in GR.SLIPS.items() if GR.INT_SET[0] in sets or "none" in sets}
    assert set(GR.SLIPS) - seen == {"resid_first", "dgelu_outer"}


# ============================================================================= the plan query and the case table

def lib():
    from hmmc_amd import _lib
    return _lib, _lib.load()


BASE = (0x7f0000100000, 0x7f0000200000, 0x7f0000300000, 0x7f0000400000)       # 16-byte aligned; never dereferenced


def plan_of(case, num_cu=256, aux=True):
    _lib, L = lib()
    before = {o: _lib.get_option(o) for o in ("no_f32_wavek", "no_f32_dma")}
    try:
        for o in before:
            _lib.set_option(o, o in case.opts)
        return GR.unpack_plan(L.hmmc_gemm_f32_plan(*case.plan_args(BASE[0], BASE[1], BASE[2], BASE[3] if aux else None, num_cu)))
    finally:
        for o, v in before.items():
            _lib.set_option(o, v)


@pytest.mark.parametrize("case", GR.CASES, ids=[c.name for c in GR.CASES])
def test_plan_of_every_case_on_256_cus(case):
    assert plan_of(case) == case.expect
    assert plan_of(case, aux=False) == case.expect                              # aux_out shares C's offset: same alignment


def test_case_table_reaches_every_instantiation_and_store_path():
    assert {tuple(c.expect[:4]) for c in GR.CASES} == GR.INSTANTIATIONS
    for fam in range(4):
        assert {c.expect.cvec for c in GR.CASES if c.expect.family == fam} == {0, 1}, GR.FAMILY[fam]
        assert any(c.full for c in GR.CASES if c.expect.family == fam), GR.FAMILY[fam]
    # the edges the GPU test is to meet
    Ks, Ms, Ns = {c.K for c in GR.CASES}, {c.M for c in GR.CASES}, {c.N for c in GR.CASES}
    assert {1, 3, 15, 16, 17, 31, 33} <= Ks and {1, 2, 15, 17, 63, 65} <= Ms and {1, 2, 15, 17, 63, 65} <= Ns
    def height(p):
        return {GR.SMALL: 16, GR.TILED: 64, GR.WAVEK: 16 * p.tile, GR.DMA: 32 * p.tile}[p.family]
    ragged = {(c.expect.family, height(c.expect)) for c in GR.CASES if c.M % height(c.expect)}     # a partial last row tile
    assert ragged == {(GR.SMALL, 16), (GR.TILED, 64), (GR.DMA, 32), (GR.DMA, 64)} | {(GR.WAVEK, h) for h in (32, 48, 64, 96)}
    for fam in range(4):                                                        # a base offset by one float, ldc > N, lda / ldb > dense
        rows = [c for c in GR.CASES if c.expect.family == fam]
        assert any(c.ldc and c.ldc > c.N for c in rows) and any(c.lda for c in rows), GR.FAMILY[fam]
    assert sum(c.aoff == 1 and c.boff == 1 and c.coff == 1 for c in GR.CASES) >= 3
    assert any(c.expect.family == GR.DMA and c.al == "r" and c.M % 4 for c in GR.CASES)      # M % 4 != 0, row-contiguous A
    assert any(c.expect.cvec and c.N % 4 for c in GR.CASES)                                   # N % 4 != 0 on the 16-byte store edge
    dma_sized = [c for c in GR.CASES if c.expect.family == GR.TILED and c.M * c.N >= 2048 * 1024 and c.K >= 500]
    assert any(c.K % 4 for c in dma_sized) and any(c.K % 4 == 0 and c.K % 32 for c in dma_sized)


def test_plan_depends_on_the_cu_count_and_the_options():
    """the same arguments on another device are another kernel: the GPU test asserts the plan before it trusts a row"""
    case = next(c for c in GR.CASES if c.name == "wavek6_vv")
    assert plan_of(case, 512)[:2] == (GR.WAVEK, 3) and plan_of(case, 64).family != GR.WAVEK     # 32 x 16 tiles of 48 rows fit 512 CUs
    _lib, L = lib()
    for case, opt, with_opt in GR.OPTION_CASES:
        assert plan_of(case) == case.expect
        assert plan_of(case._replace(opts=(opt,))) == with_opt and with_opt.family != case.expect.family
    n = L.hmmc_gemm_f32_plan(*next(c for c in GR.CASES if c.name == "small_M1").plan_args(*BASE, 0))
    assert n >= 0                                                               # num_cu = 0: the current device, or 256 without one


def test_plan_error_statuses_match_gemm_f32():
    """the argument checks hmmc_gemm_f32 makes before it launches, in its order (include/hmmc_hip.h: -1 argument, -2 unsupported);
    hmmc_gemm_f32 itself returns the same statuses for the same arguments - it launches nothing on an error, so no GPU is needed"""
    _lib, L = lib()
    a, b, c, x = BASE
    ok = dict(A=a, B=b, C=c, aux=None, M=8, N=8, K=8, sam=8, sak=1, sbk=1, sbn=8, ldc=8)
    bad = [(dict(A=None), -1), (dict(B=None), -1), (dict(C=None), -1), (dict(M=0), -1), (dict(N=-1), -1), (dict(K=0), -1),
           (dict(sam=8, sak=2), -2), (dict(sbk=3, sbn=8), -2), (dict(A=a + 2), -2), (dict(B=b + 1), -2), (dict(C=c + 3), -2),
           (dict(A=None, sak=2), -1), (dict(sak=2, A=a + 2), -2)]
    for change, status in bad:
        v = dict(ok, **change)
        q = L.hmmc_gemm_f32_plan(v["A"], v["B"], v["C"], v["aux"], v["M"], v["N"], v["K"], v["sam"], v["sak"], v["sbk"], v["sbn"], v["ldc"], 256)
        g = L.hmmc_gemm_f32(v["A"], v["B"], v["C"], v["M"], v["N"], v["K"], v["sam"], v["sak"], v["sbk"], v["sbn"], v["ldc"],
                            ctypes.c_float(1.0), None, None, None, None, 0, None)
        assert q == g == status, (change, q, g, status)
    assert L.hmmc_gemm_f32_plan(a, b, c, None, 8, 8, 8, 8, 1, 1, 8, 8, 256) >= 0
    assert L.hmmc_gemm_f32_plan(a + 4, b + 4, c + 4, x + 4, 8, 8, 8, 8, 1, 1, 8, 8, 256) >= 0      # 4-byte aligned is enough
    # the epilogue's operand checks come after these in hmmc_gemm_f32 and are not part of the query
    assert L.hmmc_gemm_f32(a, b, c, 8, 8, 8, 8, 1, 1, 8, 8, ctypes.c_float(1.0), None, None, None, None, GR.EPI_BIAS, None) == -1
    assert L.hmmc_gemm_f32(None, b, c, 8, 8, 8, 8, 2, 1, 8, 8, ctypes.c_float(1.0), None, None, None, None, GR.EPI_BIAS, None) == -1
