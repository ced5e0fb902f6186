"""Plain fp64 statement of hmmc_gemm_f32 (gemm_f32.hip) with general strides, the per-element rounding bound
tests/test_gpu_gemm_f32.py holds every kernel behind that entry point to, and the case table both test modules share.
tests/test_gemm_f32_reference.py shows on the CPU that an fp32 emulation of the kernels' summation lies inside the bound, that
plausible kernel mistakes (SLIPS) fall outside it, and that hmmc_gemm_f32_plan sends every row of CASES to the kernel
instantiation the row names on a 256-CU device.  qgelu, qgelu_grad, U and SLACK are those of hotpath_ref.

Statement (include/hmmc_hip.h; the order is store_tile16's):
  acc = sum_k A(m, k) B(k, n),  A(m, k) = A[m sam + k sak],  B(k, n) = B[k sbk + n sbn]
  h = alpha acc (+ bias[n]);  aux_out = h;  out = QuickGELU(h) | max(h, 0) | h QuickGELU'(aux_in[m ldc + n]);  (+ resid[m ldc + n])

Error model (first order, valid for ANY summation order; the tests allow SLACK times the bound for the second-order terms):
  accumulator   K products each rounded into a running fp32 sum, in any grouping, plus the meeting of the partial sums of the
                waves: (K + 8) U |alpha| (|A| |B|)[m][n]
  fp32 ops      one U |value| per further fp32 operation: * alpha, + bias, the DGELU product, + resid
  activation    qgelu32 evaluates __expf and a division, QuickGELU' a sigmoid from the same exponential: the project's envelope,
                as tests/test_gpu_model.py::test_gemm_f32_many_tiles_exact_integers asserts it - 1e-5 absolute plus 1e-5
                (QuickGELU) / 1e-4 (QuickGELU') relative on the activation - added to h's own bound carried through the
                activation's slope.  ReLU is exact and 1-Lipschitz.
Bounds are functions of the fp64 reference and the inputs only, never of a kernel's output.  Plain functions, no fixtures."""
from __future__ import annotations

from collections import namedtuple

import torch

from hotpath_ref import SLACK, U, detects, qgelu, qgelu_grad, within_ratio  # noqa: F401  (re-exported for the tests)

D64 = torch.float64
EPI_BIAS, EPI_RESID, EPI_QGELU, EPI_DGELU, EPI_RELU = 1, 2, 4, 8, 16                    # include/hmmc_hip.h
ACT_ABS, QGELU_REL, DGELU_REL = 1e-5, 1e-5, 1e-4                                        # the activation envelope (see above)

# (name, flags, alpha): the epilogue sets the GPU test runs on every kernel family.  "bias_relu_resid" is not a set of the
# product path; it is here because only an activation AND a residual together show in which order store_tile16 applies them.
EPI_SETS = (("none", 0, 1.0), ("bias", EPI_BIAS, 1.0), ("bias_resid", EPI_BIAS | EPI_RESID, 1.0), ("resid", EPI_RESID, 1.0),
            ("bias_relu", EPI_BIAS | EPI_RELU, 1.0), ("bias_qgelu_aux", EPI_BIAS | EPI_QGELU, 1.0), ("dgelu", EPI_DGELU, 1.0),
            ("alpha100_bias", EPI_BIAS, 100.0), ("bias_relu_resid", EPI_BIAS | EPI_RELU | EPI_RESID, 1.0))
INT_SET = ("alpha2_bias_resid", EPI_BIAS | EPI_RESID, 2.0)                               # every case, on integer operands
EXACT_SETS = ("none", "bias", "bias_resid", "resid", "bias_relu", "bias_relu_resid", "alpha100_bias", "alpha2_bias_resid")

# One plausible kernel mistake each -> the epilogue sets on which it changes the result, and the check that catches it:
# "bound" (random operands, elementwise bound), "equal" (integer operands, torch.equal), or both.
SLIPS = {
    "drop_k": (("none", "bias_qgelu_aux", "dgelu", "alpha2_bias_resid"), ("bound", "equal")),      # one k-term dropped
    "k_tail": (("none", "bias_qgelu_aux", "dgelu", "alpha2_bias_resid"), ("bound", "equal")),      # k = K not zeroed: the neighbour is added
    "bias_m": (("bias", "bias_relu", "alpha100_bias", "alpha2_bias_resid"), ("bound", "equal")),   # bias[m] instead of bias[n]
    "ld_n": (("resid", "bias_resid", "dgelu", "alpha2_bias_resid"), ("bound", "equal")),           # resid / aux_in read at row stride N, not ldc
    "resid_first": (("bias_relu_resid",), ("bound", "equal")),                                     # residual added before the activation
    "alpha_late": (("alpha100_bias", "alpha2_bias_resid"), ("bound", "equal")),                    # alpha applied after the bias
    "swap16": (("none", "bias_qgelu_aux", "alpha2_bias_resid"), ("bound", "equal")),               # a 16-column block swapped with its neighbour
    "dgelu_outer": (("dgelu",), ("bound",)),                                                       # the outer 1.702 of QuickGELU' missing
}


def strided(buf, rows, cols, s_row, s_col, off):
    """the rows x cols view of the flat buffer `buf` with element (i, j) at off + i s_row + j s_col"""
    return torch.as_strided(buf, (rows, cols), (s_row, s_col), off)


def reference(a, b, alpha, flags, bias=None, resid=None, aux_in=None, slip=None, tail=None, resid_n=None, aux_n=None):
    """a [M, K], b [K, N] fp64 (strided views of the operands), bias [N], resid / aux_in [M, N] views at row stride ldc
    -> (out, aux_out = h, acc, |A| |B|), all [M, N] fp64.
    slip: None or a key of SLIPS; tail = (a[:, K], b[K, :]), the neighbours behind the k range, for "k_tail"; resid_n / aux_n:
    the views of the same buffers at row stride N, for "ld_n"; for "bias_m" bias must have max(M, N) entries."""
    M, N = a.shape[0], b.shape[1]
    acc = a @ b
    absprod = a.abs() @ b.abs()
    if slip == "drop_k":
        k0 = a.shape[1] // 2
        acc = acc - a[:, k0:k0 + 1] * b[k0:k0 + 1, :]
    if slip == "k_tail":
        acc = acc + tail[0][:, None] * tail[1][None, :]
    if slip == "swap16":
        assert N >= 32
        acc = torch.cat([acc[:, 16:32], acc[:, :16], acc[:, 32:]], 1)
    if slip == "ld_n":
        resid, aux_in = resid_n, aux_n
    bv = 0.0
    if flags & EPI_BIAS:
        bv = bias[:M, None] if slip == "bias_m" else bias[None, :N]
    h = (acc + bv) * alpha if slip == "alpha_late" else acc * alpha + bv
    t = h
    if slip == "resid_first" and flags & EPI_RESID:
        t = t + resid
    if flags & EPI_QGELU:
        t = qgelu(t)
    elif flags & EPI_RELU:
        t = t.clamp_min(0.0)
    elif flags & EPI_DGELU:
        t = t * qgelu_grad(aux_in, outer=1.0 if slip == "dgelu_outer" else 1.702)
    if flags & EPI_RESID and slip != "resid_first":
        t = t + resid
    return t, h, acc, absprod


def bounds(acc, absprod, K, alpha, flags, bias=None, resid=None, aux_in=None):
    """-> (bound of out, bound of aux_out = h), from the fp64 accumulator and |A| |B| (see the module docstring)"""
    aa = abs(alpha)
    t = acc * alpha
    e = (K + 8) * U * aa * absprod + U * t.abs()                          # the sum, * alpha
    if flags & EPI_BIAS:
        t = t + bias[None, :]
        e = e + U * t.abs()
    h, eh = t, e
    if flags & EPI_QGELU:
        t = qgelu(h)
        e = qgelu_grad(h).abs() * eh + ACT_ABS + QGELU_REL * t.abs()
    elif flags & EPI_RELU:
        t = h.clamp_min(0.0)
    elif flags & EPI_DGELU:
        g = qgelu_grad(aux_in)
        t = h * g
        e = eh * g.abs() + h.abs() * (ACT_ABS + DGELU_REL * g.abs()) + U * t.abs()
    if flags & EPI_RESID:
        t = t + resid
        e = e + U * t.abs()
    return e, eh


def fma32(acc, x, y):
    """fp32(acc + x y) with the product exact, as one lane of v_mfma_f32_16x16x4_f32 forms it"""
    return (acc.double() + x.double() * y.double()).float()


def emulate(a, b, alpha, flags, bias=None, resid=None, aux_in=None, waves=4):
    """gemm_f32.hip's arithmetic in torch fp32.  waves = 4: the small and wave-split-K kernels - wave w runs the 16-deep K-steps
    w, w + 4, ... as one chain and the four partial tiles meet as (0 + 1) + (2 + 3); waves = 1: one in-order chain (the tiled and
    LDS-DMA kernels).  Then store_tile16.  a [M, K], b [K, N], bias, resid, aux_in fp32 -> (out, aux_out) fp32."""
    M, K = a.shape
    N = b.shape[1]
    part = [torch.zeros(M, N, dtype=torch.float32) for _ in range(waves)]
    for k in range(K):
        w = (k // 16) % waves
        part[w] = fma32(part[w], a[:, k:k + 1], b[k:k + 1, :])
    v = (part[0] + part[1]) + (part[2] + part[3]) if waves == 4 else part[0]
    t = v * torch.tensor(alpha, dtype=torch.float32)
    if flags & EPI_BIAS:
        t = t + bias[None, :]
    h = t
    if flags & EPI_QGELU:
        t = h / (1.0 + torch.exp(-1.702 * h))
    elif flags & EPI_RELU:
        t = h.clamp_min(0.0)
    elif flags & EPI_DGELU:
        s = 1.0 / (1.0 + torch.exp(-1.702 * aux_in))
        t = h * (s + 1.702 * aux_in * s * (1.0 - s))
    if flags & EPI_RESID:
        t = t + resid
    return t, h


def operands(regime, M, N, K, seed=0, device="cpu", extra_k=0):
    """-> a [M, K + extra_k], b [K + extra_k, N] fp32.  "int": integers in [-3, 3] (every product and partial sum exact in fp32);
    "normal": unit normal; "range": unit normal times a per-k scale running over 1e3, largest first on A and last on B's side of
    the same k, so that single products differ by 1e3 along k while |A| |B| stays O(sqrt(K))"""
    g = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    Ke = K + extra_k
    if regime == "int":
        a = torch.randint(-3, 4, (M, Ke), generator=g).float()
        b = torch.randint(-3, 4, (Ke, N), generator=g).float()
    else:
        a = torch.randn(M, Ke, generator=g)
        b = torch.randn(Ke, N, generator=g)
        if regime == "range":
            s = torch.logspace(0, -3, Ke)
            s = s[torch.randperm(Ke, generator=g)]
            a = a * s[None, :]
            b = b * s.sqrt()[:, None]
    return a.to(device), b.to(device)


def epilogue_operands(regime, M, N, seed=0, device="cpu"):
    """-> bias [max(M, N)] (the first N are the bias), resid [M, N], aux_in [M, N] fp32: integers for "int", else normal"""
    g = torch.Generator().manual_seed(seed * 104729 + M * 31 + N)
    if regime == "int":
        r = lambda *s: torch.randint(-5, 6, s, generator=g).float()     # noqa: E731
    else:
        r = lambda *s: torch.randn(*s, generator=g)                     # noqa: E731
    return r(max(M, N)).to(device), r(M, N).to(device), r(M, N).to(device)


# ============================================================================= the case table

SMALL, TILED, WAVEK, DMA = 0, 1, 2, 3                      # HMMC_F32_SMALL .. HMMC_F32_DMA
FAMILY = ("small", "tiled", "wavek", "dma")
KVEC, RVEC, SCALAR = 0, 1, 2                               # operand staging modes of the tiled kernel

Plan = namedtuple("Plan", "family tile a b cvec")


def unpack_plan(v):
    """the fields of hmmc_gemm_f32_plan's value (HMMC_F32_PLAN_* of include/hmmc_hip.h)"""
    assert v >= 0, f"hmmc_gemm_f32_plan: status {v}"
    return Plan(v & 15, (v >> 4) & 15, (v >> 8) & 15, (v >> 12) & 15, (v >> 16) & 1)


# the 37 template instantiations hmmc_gemm_f32 can launch, as (family, tile, a, b)
INSTANTIATIONS = frozenset(
    [(SMALL, 0, a, b) for a in (0, 1) for b in (0, 1)] +
    [(WAVEK, rm, a, b) for rm in (2, 3, 4, 6) for a in (0, 1) for b in (0, 1)] +
    [(TILED, 0, a, b) for a in (KVEC, RVEC, SCALAR) for b in (KVEC, RVEC, SCALAR)] +
    [(DMA, mi, a, b) for mi in (1, 2) for a in (0, 1) for b in (0, 1)])
assert len(INSTANTIATIONS) == 37


class Case(namedtuple("Case", "name M N K al bl lda ldb aoff boff ldc coff opts full expect")):
    """One launch of hmmc_gemm_f32.  al / bl: "k" = k-contiguous (A [M, lda], B [N, ldb]), "r" = row-contiguous (A [K, lda],
    B [K, ldb]); lda / ldb / ldc None = dense; aoff / boff / coff: floats between the 16-byte aligned allocation and element
    (0, 0) (a [T, 3D] slice: the column offset; 1: a base that is 4- but not 16-byte aligned); opts: option switches set for the
    launch; full: run every epilogue set, not only the integer and the plain random launches; expect: Plan on 256 CUs."""
    __slots__ = ()

    def strides(self):
        lda = self.lda or (self.K if self.al == "k" else self.M)
        ldb = self.ldb or (self.K if self.bl == "k" else self.N)
        sa = (lda, 1) if self.al == "k" else (1, lda)                # (sam, sak)
        sb = (1, ldb) if self.bl == "k" else (ldb, 1)                # (sbk, sbn)
        return sa, sb, self.ldc or self.N

    def plan_args(self, pa, pb, pc, paux, num_cu):
        """the argument list of hmmc_gemm_f32_plan for operand allocations at the 16-byte aligned addresses pa, pb, pc, paux"""
        sa, sb, ldc = self.strides()
        return (pa + 4 * self.aoff, pb + 4 * self.boff, pc + 4 * self.coff, (paux + 4 * self.coff) if paux else None,
                self.M, self.N, self.K, sa[0], sa[1], sb[0], sb[1], ldc, num_cu)


def C(name, M, N, K, al, bl, expect, lda=None, ldb=None, aoff=0, boff=0, ldc=None, coff=0, opts=(), full=False):
    return Case(name, M, N, K, al, bl, lda, ldb, aoff, boff, ldc, coff, tuple(opts), full, Plan(*expect))


NOW, NOD = "no_f32_wavek", "no_f32_dma"
D_ = 64                                                    # the hidden width of the [T, 3D] production pattern used below

CASES = [
    # ---- small (16 x 32 tiles; av / bv = 16-byte k-contiguous loads) --------------------------------------------------------
    C("small_kk_all_epilogues", 50, 70, 64, "k", "k", (SMALL, 0, 1, 1, 1), ldc=72, full=True),
    C("small_kk_K1", 17, 33, 1, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_kk_K3", 15, 17, 3, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_kk_K15", 63, 65, 15, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_kk_K16", 65, 63, 16, "k", "k", (SMALL, 0, 1, 1, 0)),
    C("small_kk_K17", 2, 15, 17, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_kr_K31", 16, 32, 31, "k", "r", (SMALL, 0, 0, 0, 1)),
    C("small_rk_K33", 15, 64, 33, "r", "k", (SMALL, 0, 0, 0, 1), lda=16),
    C("small_M1", 1, 64, 48, "k", "k", (SMALL, 0, 1, 1, 1)),
    C("small_N1", 64, 1, 48, "k", "k", (SMALL, 0, 1, 1, 0)),
    C("small_N2", 63, 2, 33, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_M1_N1_K1", 1, 1, 1, "k", "k", (SMALL, 0, 0, 0, 0)),
    C("small_kr_vec_scalar", 48, 96, 64, "k", "r", (SMALL, 0, 1, 0, 1), lda=80, ldb=100, full=True),
    C("small_rk_scalar_vec", 50, 66, 64, "r", "k", (SMALL, 0, 0, 1, 0), lda=52, ldb=68),
    C("small_rr", 33, 47, 40, "r", "r", (SMALL, 0, 0, 0, 0), lda=36, ldb=48),
    C("small_kk_base_plus_one", 32, 64, 64, "k", "k", (SMALL, 0, 0, 0, 0), aoff=1, boff=1, coff=1),
    C("small_qkv_slices", 77, D_, D_, "k", "k", (SMALL, 0, 1, 1, 1), lda=3 * D_, aoff=D_, ldc=3 * D_, coff=2 * D_, full=True),
    C("small_class_rows", 8, 128, 64, "k", "k", (SMALL, 0, 1, 1, 1), lda=50 * 64),
    # ---- tiled (64 x 64 through LDS; amode / bmode) ---------------------------------------------------------------------------
    C("tiled_kvec_kvec_all_epilogues", 1000, 2050, 36, "k", "k", (TILED, 0, KVEC, KVEC, 0), full=True),
    C("tiled_kvec_rvec", 1024, 2048, 36, "k", "r", (TILED, 0, KVEC, RVEC, 1), lda=40, ldb=2052, ldc=2052),
    C("tiled_kvec_scalar", 1030, 2046, 36, "k", "r", (TILED, 0, KVEC, SCALAR, 0)),
    C("tiled_rvec_kvec", 1028, 2040, 44, "r", "k", (TILED, 0, RVEC, KVEC, 1), lda=1032, full=True),
    C("tiled_rvec_rvec", 1024, 2048, 33, "r", "r", (TILED, 0, RVEC, RVEC, 1)),
    C("tiled_rvec_scalar", 1024, 2048, 31, "r", "k", (TILED, 0, RVEC, SCALAR, 1)),
    C("tiled_scalar_kvec", 1026, 2048, 36, "r", "k", (TILED, 0, SCALAR, KVEC, 1), lda=1028),
    C("tiled_scalar_rvec", 1024, 2048, 17, "k", "r", (TILED, 0, SCALAR, RVEC, 1)),
    C("tiled_scalar_scalar_base_plus_one", 1023, 2049, 36, "k", "k", (TILED, 0, SCALAR, SCALAR, 0), aoff=1, boff=1, coff=1,
      full=True),
    C("tiled_qkv_backward", 4096, 3 * D_, 3 * D_, "k", "r", (TILED, 0, KVEC, RVEC, 1), lda=9 * D_, aoff=3 * D_, opts=(NOW,)),
    C("tiled_dma_shape_K_not_32", 2048, 1024, 500, "k", "k", (TILED, 0, KVEC, KVEC, 1)),
    C("tiled_dma_shape_K_not_4", 2048, 1024, 510, "k", "k", (TILED, 0, SCALAR, SCALAR, 1)),
    # ---- wave-split-K ((16 rm) x 64 tiles) --------------------------------------------------------------------------------
    C("wavek2_vv_all_epilogues", 500, 1000, 1540, "k", "k", (WAVEK, 2, 1, 1, 1), ldc=1004, full=True),
    C("wavek2_vs", 512, 1024, 1536, "k", "r", (WAVEK, 2, 1, 0, 1)),
    C("wavek2_sv", 510, 1024, 1536, "r", "k", (WAVEK, 2, 0, 1, 1), lda=512),
    C("wavek2_ss_K_mod_4", 481, 1023, 1538, "k", "k", (WAVEK, 2, 0, 0, 0), full=True),
    C("wavek3_vv", 760, 1024, 1540, "k", "k", (WAVEK, 3, 1, 1, 1), lda=1544, ldb=1548),
    C("wavek3_vs", 768, 1000, 1536, "k", "r", (WAVEK, 3, 1, 0, 1)),
    C("wavek3_sv", 721, 1024, 1536, "r", "k", (WAVEK, 3, 0, 1, 1), lda=724),
    C("wavek3_ss", 768, 1024, 1536, "r", "r", (WAVEK, 3, 0, 0, 1)),
    C("wavek4_vv", 1000, 1024, 1540, "k", "k", (WAVEK, 4, 1, 1, 1)),
    C("wavek4_vs", 1024, 1024, 1536, "k", "r", (WAVEK, 4, 1, 0, 1), opts=(NOD,)),
    C("wavek4_sv", 1024, 1024, 1536, "r", "k", (WAVEK, 4, 0, 1, 1), opts=(NOD,)),
    C("wavek4_ss_base_plus_one", 961, 1024, 1536, "k", "k", (WAVEK, 4, 0, 0, 0), aoff=1, boff=1, coff=1),
    C("wavek6_vv", 1500, 1024, 1540, "k", "k", (WAVEK, 6, 1, 1, 1)),
    C("wavek6_vs", 1536, 1024, 1536, "k", "r", (WAVEK, 6, 1, 0, 1), opts=(NOD,)),
    C("wavek6_sv", 1441, 1024, 1536, "r", "k", (WAVEK, 6, 0, 1, 1), lda=1444, opts=(NOD,)),
    C("wavek6_ss", 1536, 1001, 1537, "r", "r", (WAVEK, 6, 0, 0, 0), lda=1536, ldb=1004, ldc=1001),
    # ---- LDS-DMA ((32 mi) x 64 tiles; akc / bkc = k-contiguous) ---------------------------------------------------------------
    C("dma2_kk_all_epilogues", 2040, 1000, 512, "k", "k", (DMA, 2, 1, 1, 1), lda=544, ldb=516, ldc=1004, full=True),
    C("dma2_kr", 2048, 1022, 512, "k", "r", (DMA, 2, 1, 0, 0), ldb=1024),
    C("dma2_rk_M_mod_4", 2047, 1024, 512, "r", "k", (DMA, 2, 0, 1, 1), lda=2048, full=True),
    C("dma2_rr", 2046, 1021, 512, "r", "r", (DMA, 2, 0, 0, 1), lda=2048, ldb=1024, ldc=1024),
    C("dma1_kk", 1600, 1024, 1024, "k", "k", (DMA, 1, 1, 1, 1), opts=(NOW,)),
    C("dma1_kr", 1570, 1024, 1024, "k", "r", (DMA, 1, 1, 0, 1), opts=(NOW,), full=True),
    C("dma1_rk", 1569, 1024, 1024, "r", "k", (DMA, 1, 0, 1, 1), lda=1572, opts=(NOW,)),
    C("dma1_rr_N_mod_4", 1600, 1023, 1024, "r", "r", (DMA, 1, 0, 0, 0), ldb=1024, opts=(NOW,)),
    C("dma_qkv_slices", 4096, 512, 512, "k", "k", (DMA, 2, 1, 1, 1), lda=1536, aoff=1024, ldc=1536, coff=512),
]
assert len({c.name for c in CASES}) == len(CASES)

# a shape that takes the family, the option that forbids it, and the plan with the option set
OPTION_CASES = [
    (C("option_wavek", 512, 1024, 1536, "k", "k", (WAVEK, 2, 1, 1, 1)), NOW, Plan(TILED, 0, KVEC, KVEC, 1)),
    (C("option_dma", 2048, 1024, 512, "k", "k", (DMA, 2, 1, 1, 1)), NOD, Plan(TILED, 0, KVEC, KVEC, 1)),
]
