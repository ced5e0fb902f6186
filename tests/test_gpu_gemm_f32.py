"""GPU tests of hmmc_gemm_f32 (gemm_f32.hip): every one of the 37 kernel instantiations behind the entry point, called through the
C-ABI and compared ELEMENTWISE with the fp64 statement of tests/gemm_f32_ref.py (pinned by tests/test_gemm_f32_reference.py, which
also shows on the CPU that an fp32 emulation lies inside the bound and that plausible kernel mistakes fall outside it).

Each row of gemm_f32_ref.CASES names the instantiation it is for; the test first asserts that hmmc_gemm_f32_plan gives exactly that
for the buffers it is about to pass (a device with another CU count fails there instead of testing another kernel), and
test_zy_every_instantiation_ran closes the set.  Every row runs on integer operands (alpha = 2, integer bias and residual: torch.equal
with fp64) and on random operands in two regimes (within the bound); rows marked `full` run every epilogue set of
gemm_f32_ref.EPI_SETS.  Every launch is made twice for equal bits.  Operands live inside NaN-filled allocations - row padding, the k
tail of each row, rows past M / N, 8 rows behind the end - at the row's strides and base offsets; C and aux_out sit at ldc between
sentinel-filled guard bands and gap columns that must be intact afterwards; the gaps of resid and aux_in hold NaN.
A NaN fails every comparison, no element is left out.  The last test prints the worst err / (SLACK bound) per family.

Worst err / (SLACK bound) measured on an MI355X (256 CUs), all 60 tests passing and all 37 instantiations reached:
  small 0.110 (small_kk_K16, "range" operands)   tiled 0.123 (tiled_scalar_rvec, K = 17, "range")
  wavek 0.002 (K = 1536 .. 1540)                 dma   0.015 (K = 512 .. 1024)
None is above 0.5.  The ratio falls with K because the accumulator term (K + 8) U |A| |B| is a worst case over the signs of the
rounding errors, which in fact add like sqrt(K); with an activation the largest ratios are 0.07 (aux_out) and 0.02 (C), so the
1e-5 envelope of the activation is the loose term there."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_f32_ref as GR  # noqa: E402
from hmmc_amd import _lib  # noqa: E402
from hmmc_amd._lib import call, ptr, query  # noqa: E402

DEV = "cuda"
D64 = torch.float64
SENT = -777.0
GUARD = 64                    # floats in front of and behind every output (keeps the 16-byte alignment of the allocation)
NAN = float("nan")
WORST = {}                    # family -> worst err / (SLACK bound)
SEEN = set()                  # (family, tile, a, b) of every plan a case asserted and ran


def within(got, ref, bound, what, family):
    """|got - ref| <= SLACK * bound elementwise; a NaN anywhere fails (`not (err <= lim)`), no element is left out"""
    got = got.detach().to(D64)
    nan = torch.isnan(got)
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} of {got.numel()} elements are NaN"
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{what}: the reference or its bound is not finite"
    err = (got - ref).abs()
    lim = GR.SLACK * bound
    bad = ~(err <= lim)
    ratio = float((err / lim).nan_to_num(0.0).max()) if err.numel() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"gemm-f32-ratio {family} {what}: {ratio:.3f}")
    if bool(bad.any()):
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside the bound; worst err / (SLACK bound) "
                             f"{ratio:.2f}, max err {float(err.max()):.3e}, first at {idx}: got {float(got[tuple(idx)]):.6g} "
                             f"ref {float(ref[tuple(idx)]):.6g}")


def exact(got, ref, what):
    got = got.to(D64)
    if not torch.equal(got, ref):
        bad = ~(got == ref)
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from fp64; first at {idx}: got "
                             f"{float(got[tuple(idx)]):.9g} ref {float(ref[tuple(idx)]):.9g}")


def operand(vals, layout, ld, off):
    """vals [rows, K] inside a NaN-filled allocation: "k": element (r, k) at off + r ld + k, "r": at off + k ld + r; 8 lines of
    NaN behind the last one -> (allocation, element (0, 0)'s index, (row stride, k stride))"""
    rows, K = vals.shape
    lines = rows if layout == "k" else K
    buf = torch.full((off + (lines + 8) * ld + 4,), NAN, dtype=torch.float32, device=DEV)
    s = (ld, 1) if layout == "k" else (1, ld)
    GR.strided(buf, rows, K, s[0], s[1], off).copy_(vals)
    return buf, off, s


class Out:
    """an M x N matrix at row stride ldc, `off` floats into a guarded allocation filled with `fill`"""

    def __init__(self, M, N, ldc, off, fill, vals=None):
        self.M, self.N, self.ldc, self.start, self.fill = M, N, ldc, GUARD + off, fill
        self.buf = torch.full((GUARD + off + (M - 1) * ldc + N + GUARD,), fill, dtype=torch.float32, device=DEV)
        if vals is not None:
            self.view().copy_(vals)

    def view(self):
        return GR.strided(self.buf, self.M, self.N, self.ldc, 1, self.start)

    def ptr(self):
        return ptr(self.buf[self.start:])

    def untouched(self, what):
        """everything outside the M x N addressed elements still holds the sentinel"""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        GR.strided(mask, self.M, self.N, self.ldc, 1, self.start).fill_(False)
        wrong = self.buf[mask] != self.fill
        assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} elements outside the output's rows were written"


class Problem:
    """the device buffers of one case in one data regime"""

    def __init__(self, case, regime):
        self.case = c = case
        (self.sam, self.sak), (self.sbk, self.sbn), self.ldc = c.strides()
        a, b = GR.operands(regime, c.M, c.N, c.K, device=DEV)
        bias, resid, aux = GR.epilogue_operands(regime, c.M, c.N, device=DEV)
        self.abuf, self.a0, _ = operand(a, c.al, max(self.sam, self.sak), c.aoff)
        self.bbuf, self.b0, _ = operand(b.t(), c.bl, max(self.sbk, self.sbn), c.boff)
        self.bias = torch.cat([bias[:c.N], torch.full((8,), NAN, device=DEV)])
        self.resid = Out(c.M, c.N, self.ldc, c.coff, NAN, resid)
        self.aux_in = Out(c.M, c.N, self.ldc, c.coff, NAN, aux)
        self.a64 = GR.strided(self.abuf, c.M, c.K, self.sam, self.sak, self.a0).double()
        self.b64 = GR.strided(self.bbuf, c.K, c.N, self.sbk, self.sbn, self.b0).double()
        self.acc = self.a64 @ self.b64
        self.absprod = self.a64.abs() @ self.b64.abs()

    def pa(self):
        return ptr(self.abuf[self.a0:])

    def pb(self):
        return ptr(self.bbuf[self.b0:])

    def plan(self, c_out, aux_out, num_cu=0):
        c = self.case
        return GR.unpack_plan(query("hmmc_gemm_f32_plan", self.pa(), self.pb(), c_out.ptr(), aux_out.ptr() if aux_out else None,
                                    c.M, c.N, c.K, self.sam, self.sak, self.sbk, self.sbn, self.ldc, num_cu))

    def launch(self, flags, alpha, want_aux, expect=None):
        c = self.case
        out = Out(c.M, c.N, self.ldc, c.coff, SENT)
        aux = Out(c.M, c.N, self.ldc, c.coff, SENT) if want_aux else None
        if expect is not None:
            got = self.plan(out, aux)
            assert got == expect, f"{c.name}: hmmc_gemm_f32_plan gives {tuple(got)}, the row is for {tuple(expect)} (256 CUs)"
        call("hmmc_gemm_f32", self.pa(), self.pb(), out.ptr(), c.M, c.N, c.K, self.sam, self.sak, self.sbk, self.sbn, self.ldc,
             float(alpha), ptr(self.bias) if flags & GR.EPI_BIAS else None, self.resid.ptr() if flags & GR.EPI_RESID else None,
             aux.ptr() if aux else None, self.aux_in.ptr() if flags & GR.EPI_DGELU else None, flags)
        torch.cuda.synchronize()
        out.untouched(f"{c.name}: C")
        if aux:
            aux.untouched(f"{c.name}: aux_out")
        return out.view().clone(), (aux.view().clone() if aux else None)

    def check(self, name, flags, alpha, regime, expect):
        """one epilogue set: two launches with equal bits, then torch.equal (integer operands, exact arithmetic) or the bound"""
        c = self.case
        fam = GR.FAMILY[expect.family]
        tag = f"{c.name} {name} {regime}"
        want_aux = bool(flags & GR.EPI_QGELU)
        out, aux = self.launch(flags, alpha, want_aux, expect)
        out2, aux2 = self.launch(flags, alpha, want_aux)
        assert torch.equal(out, out2) and (aux is None or torch.equal(aux, aux2)), f"{tag}: two launches differ"
        bias, resid, aux_in = self.bias[:c.N].double(), self.resid.view().double(), self.aux_in.view().double()
        ref, h = GR.reference(self.a64, self.b64, alpha, flags, bias, resid, aux_in)[:2]
        b_out, b_h = GR.bounds(self.acc, self.absprod, c.K, alpha, flags, bias, resid, aux_in)
        if regime == "int":
            if aux is not None:
                exact(aux, h, f"{tag}: aux_out")
            if name in GR.EXACT_SETS:
                exact(out, ref, f"{tag}: C")
                return
        elif aux is not None:
            within(aux, h, b_h, f"{tag}: aux_out", fam)
        within(out, ref, b_out, f"{tag}: C", fam)


def with_options(opts):
    class _Ctx:
        def __enter__(self):
            self.before = {o: _lib.get_option(o) for o in ("no_f32_wavek", "no_f32_dma")}
            for o in self.before:
                _lib.set_option(o, o in opts)

        def __exit__(self, *exc):
            for o, v in self.before.items():
                _lib.set_option(o, v)
    return _Ctx()


@pytest.mark.parametrize("case", GR.CASES, ids=[c.name for c in GR.CASES])
def test_gemm_f32_case(case):
    with with_options(case.opts):
        p = Problem(case, "int")
        p.check(*GR.INT_SET, "int", case.expect)
        if case.full:
            for name, flags, alpha in GR.EPI_SETS:
                p.check(name, flags, alpha, "int", case.expect)
        for regime in ("normal", "range"):
            p = Problem(case, regime)
            p.check("none", 0, 1.0, regime, case.expect)
            if case.full and regime == "normal":
                for name, flags, alpha in GR.EPI_SETS[1:]:
                    p.check(name, flags, alpha, regime, case.expect)
    SEEN.add(tuple(case.expect[:4]))


@pytest.mark.parametrize("case,opt,with_opt", GR.OPTION_CASES, ids=[o[0].name for o in GR.OPTION_CASES])
def test_option_switch_changes_the_plan_not_the_integers(case, opt, with_opt):
    with with_options(()):
        p = Problem(case, "int")
        out, _ = p.launch(*GR.INT_SET[1:], False, case.expect)
        with with_options((opt,)):
            other, _ = p.launch(*GR.INT_SET[1:], False, with_opt)
        assert _lib.get_option(opt) is False
        ref = GR.reference(p.a64, p.b64, GR.INT_SET[2], GR.INT_SET[1], p.bias[:case.N].double(), p.resid.view().double())[0]
        exact(out, ref, f"{case.name}: default")
        exact(other, ref, f"{case.name}: with {opt}")


def test_operand_over_2_gib_is_not_dma():
    """A k-contiguous with K % 32 == 0 and just over 2 GiB: the LDS-DMA kernel's 32-bit byte offsets do not reach, the plan must
    say so (half the rows do take it), and the kernel taken instead must index with 64 bits.  Integer operands, row chunks."""
    M, N, K = (1 << 19) + 64, 64, 1024
    try:
        a = torch.empty((M, K), dtype=torch.float32, device=DEV)
    except RuntimeError as e:                                                    # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"no {M * K * 4 / 2 ** 30:.2f} GiB allocation on this device: {e}")
    assert a.numel() * 4 > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5)
    for r0 in range(0, M, 1 << 16):
        a[r0:r0 + (1 << 16)] = torch.randint(-3, 4, a[r0:r0 + (1 << 16)].shape, device=DEV, generator=g).float()
    b = torch.randint(-3, 4, (N, K), device=DEV, generator=g).float()
    bias = torch.randint(-5, 6, (N,), device=DEV, generator=g).float()
    out = Out(M, N, N, 0, SENT)
    with with_options(()):
        args = (M, N, K, K, 1, 1, K, N)
        plan = GR.unpack_plan(query("hmmc_gemm_f32_plan", ptr(a), ptr(b), out.ptr(), None, *args, 0))
        half = GR.unpack_plan(query("hmmc_gemm_f32_plan", ptr(a), ptr(b), out.ptr(), None, M // 2, *args[1:], 0))
        assert half.family == GR.DMA and plan.family != GR.DMA, (tuple(plan), tuple(half))
        call("hmmc_gemm_f32", ptr(a), ptr(b), out.ptr(), *args, 2.0, ptr(bias), None, None, None, GR.EPI_BIAS)
        torch.cuda.synchronize()
    out.untouched("2 GiB: C")
    c = out.view()
    for r0 in range(0, M, 1 << 16):
        ref = 2.0 * (a[r0:r0 + (1 << 16)].double() @ b.double().t()) + bias.double()
        exact(c[r0:r0 + (1 << 16)], ref, f"2 GiB operand, rows from {r0}")


def test_zy_every_instantiation_ran():
    """the plans asserted and run by test_gemm_f32_case are the full list of instantiations (run the module as a whole)"""
    missing = sorted(GR.INSTANTIATIONS - SEEN)
    assert not missing and SEEN == GR.INSTANTIATIONS, f"{len(SEEN)} of 37 instantiations ran; missing {missing}"
    print(f"gemm-f32-coverage: {len(SEEN)} of {len(GR.INSTANTIATIONS)} instantiations ran")


def test_zz_report_worst_ratios():
    for fam in GR.FAMILY:
        assert fam in WORST, f"no bounded comparison ran on the {fam} kernels"
        print(f"gemm-f32-worst {fam}: {WORST[fam]:.3f}")
