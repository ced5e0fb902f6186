"""GPU tests of the row and elementwise kernels of norm_elem.hip besides LayerNorm, each called with its own inputs through the
C-ABI (guarded outputs) and through hmmc_amd.ops, and compared ELEMENTWISE with a plain statement of the same op
(tests/rowops_ref.py, pinned by tests/test_rowops_reference.py): torch.equal for the gather, layout and rounding ops, a derived
bound (c U sum|x| [+ U16 |sum|], allowed SLACK = 2 times) against the fp64 sum for the two accumulating ops, torch.equal on
integer data where every fp32 sum is exact.  A NaN fails every comparison, no element is left out, outputs sit between
sentinel-filled guard bands, the accumulating kernels run twice for bit-identical results.

Entry points, the test that reaches each, and the branch each case reaches:
  hmmc_colsum (+ _workspace)   test_colsum: M = 512 (fp32: one launch) / 513 (two launches), the slab arithmetic at M = 1 .. 4097
                               (rpb, the recomputed rb, a short last slab at 65, 4097), the 1024-slab cap at M = 65 537 (asserted),
                               fp16 / fp32 in x out, round_f16, widths 4 / 8, 264 (a partial 32-chunk column block), 768, 38 400
                               test_colsum_strided: ld > N through the C-ABI, NaN behind column N (fp32 of <= 512 rows then takes
                               two launches); test_colsum_out_slice: ops.colsum(out=) into the middle of a sentinel buffer
  hmmc_text_embed_bwd          test_text_embed_bwd_long: the list-full (`!room`) path - n16384 (the list exactly full), n16385 (a
                               second batch of one), n39k (three batches inside one 65 536-row window, each ending in the middle of
                               the occurrences), dense (batches ending on a full list), both_limits (150 000 rows: batches ended by
                               the 16-bit window and by the list); the heavy id never starts at row 0
                               test_text_embed_bwd_wide: the c0 column-block loop, D = 520 and 768 (D > 512), 8 and 512 (one block),
                               fp16 and fp32 dx; ids that never occur (exactly zero rows), ids outside the table
  hmmc_patchify, _patchify_u8  test_patchify: five (H, patch), fp16 and fp32 outputs, frame_index with repeats, reversed, m > n, m = 1
                               test_patchify_grid_wrap: 1100 frames of 64 x 64 = 2 112 000 chunks > 8192 x 256 (asserted); the uint8
                               form through a 1100-entry frame_index over 3 stored frames
  hmmc_vit_embed               test_vit_embed: L x D x dtype, garbage class rows;  test_embed_grid_wrap: > 4096 x 256 chunks (asserted)
  hmmc_text_embed              test_text_embed: ids 0 and vocab - 1, ids outside the table (position row alone, error flag raised and
                               cleared);  test_embed_grid_wrap
  hmmc_eot_index               test_eot_index: L x b, unique and repeated maxima (one lane's l and l + 64, neighbouring lanes, first
                               at 0 and at L - 1), equal rows, negative rows, base / stride of a padded token-major buffer
  hmmc_cast                    test_cast: both directions, n = 1 .. 2048 x 256 + 3 (the grid wrap, asserted), ties, overflow, subnormals
  status paths                 test_statuses: eleven rejected argument sets, each refused before any launch, outputs untouched

Worst err / (SLACK bound) against fp64 measured on an MI355X (256 CUs), every test passing (test_zz_report_worst_ratios prints them):
  colsum          0.496 signed, 0.499 same-sign (both where the fp16 rounding of the sum is all there is: half an ulp of U16 |sum|)
  text_embed_bwd  0.097 signed, 0.153 same-sign (fp32 output; c U sum|dx| is a worst case over the signs of c rounding errors)"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_ref as RR  # noqa: E402
from hmmc_amd import ops  # noqa: E402
from hmmc_amd._lib import STATUS, call, load, ptr, query, stream  # noqa: E402

DEV = "cuda"
D64 = torch.float64
F16, F32 = torch.float16, torch.float32
SENT = -777.0                 # exact in fp16 and fp32
GUARD = 64                    # elements in front of and behind every guarded output
NAN = float("nan")
WORST = {}                    # family -> worst err / (SLACK bound) against fp64
KC = RR.kernel_constants()    # the grid caps and thresholds as norm_elem.hip states them


def within(got, ref, bound, what, family):
    """|got - ref| <= SLACK * bound elementwise (infinities must match exactly; a NaN anywhere fails: the check is written as
    `not (err <= lim)`)."""
    got = got.detach().to(D64).to(ref.device)
    ref = ref.detach().to(D64)
    nan = torch.isnan(got)
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} of {got.numel()} elements are NaN"
    assert not bool(torch.isnan(ref).any()), f"{what}: NaN in the fp64 reference"
    inf = torch.isinf(ref) | torch.isinf(got)
    assert torch.equal(got[inf], ref[inf]), f"{what}: infinities differ"
    err = (got - ref).abs().masked_fill(inf, 0.0)
    lim = torch.as_tensor(RR.SLACK * bound, dtype=D64, device=err.device).expand_as(err).masked_fill(inf, 0.0)
    bad = ~(err <= lim)
    ratio = float((err / lim).nan_to_num(0.0).max()) if err.numel() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    if bool(bad.any()):
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside the bound; worst err / (SLACK bound) "
                             f"{ratio:.2f}, max err {float(err.max()):.3e}, first at {idx}: got {float(got[tuple(idx)]):.6g} "
                             f"ref {float(ref[tuple(idx)]):.6g}")
    return ratio


def guarded(shape, dtype, fill=SENT):
    """an output inside a larger sentinel-filled allocation -> (allocation, view); fill: what the view itself holds"""
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if fill != SENT:
        view.fill_(fill)
    return buf, view


def guards_intact(buf, what):
    n = buf.numel() - 2 * GUARD
    assert bool((buf[:GUARD] == SENT).all()), f"{what}: bytes in front of the buffer were written"
    assert bool((buf[GUARD + n:] == SENT).all()), f"{what}: bytes behind the buffer were written"


def untouched(buf):
    return bool((buf == SENT).all())


def status(name, *args):
    """an entry point's return value on the current stream (no exception)"""
    rc = getattr(load(), name)(*args, stream())
    torch.cuda.synchronize()
    return rc


def dtc(dtype):
    return 0 if dtype == F16 else 1


def same(got, ref, what):
    """torch.equal, no NaN, with the first difference in the message"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN in the result"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: got {got[i].item()} ref {ref[i].item()}")


# ============================================================================= colsum

def run_colsum(xbuf, M, N, ld, in_dt, out_dt, rf):
    """hmmc_colsum twice through the C-ABI: guarded output, a NaN workspace of exactly the bytes the ABI asks for with a sentinel
    strip behind it -> out [N] of the two bit-equal launches"""
    nbytes = query("hmmc_colsum_workspace", M, N)
    assert nbytes == RR.colsum_workspace(M, N)
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4 + GUARD,), SENT, dtype=F32, device=DEV)
        ws[:nbytes // 4] = NAN
        buf, out = guarded((N,), out_dt)
        call("hmmc_colsum", ptr(xbuf), ptr(out), M, N, ld, dtc(in_dt), dtc(out_dt), int(rf), ptr(ws), nbytes)
        torch.cuda.synchronize()
        guards_intact(buf, "colsum out")
        assert untouched(ws[nbytes // 4:]), "colsum: the workspace was written past the bytes the ABI asked for"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and not bool(torch.isnan(outs[0].float()).any()), "colsum: two runs differ (or NaN)"
    return outs[0]


def check_colsum(M, N, in_dt, ld, dense, seed=0):
    plan = RR.colsum_plan(M, in_dt, dense)
    for family in RR.FAMILIES + ("exact",):
        x = RR.values(family, (M, N), RR.gen(M + N + seed, DEV), DEV).to(in_dt)
        xbuf = torch.full((M, ld), NAN, dtype=in_dt, device=DEV)
        xbuf[:, :N] = x
        x64 = x.double()
        ref = RR.colsum(x64)
        for out_dt in (F16, F32):
            for rf in (0, 1):
                got = run_colsum(xbuf, M, N, ld, in_dt, out_dt, rf)
                half = out_dt == F16 or bool(rf)
                tag = f"colsum M {M} N {N} ld {ld} {in_dt} -> {out_dt} round_f16 {rf} {family}"
                if family == "exact":
                    assert float(x64.abs().sum(0).max()) < 2 ** 24
                    same(got.double(), ref.half().double() if half else ref, tag)
                else:
                    within(got, ref, RR.colsum_bound(x64, ref, plan, half), tag, f"colsum.{family}")
                if rf and out_dt == F32:
                    assert torch.equal(got, got.half().float()), f"{tag}: the fp32 output is not an fp16 value"


@pytest.mark.parametrize("M", RR.COLSUM_M)
def test_colsum(M):
    """fp16 / fp32 input x fp16 / fp32 output x round_f16 at every width of the row count, signed, same-sign and integer data"""
    for in_dt in (F16, F32):
        plan = RR.colsum_plan(M, in_dt)
        if M == 512:
            assert plan["direct"] == (in_dt == F32)
        if M == 513:
            assert not plan["direct"]
        if M == 65537:                                                # past the slab cap: fewer slabs than M / 64, more rows in each
            assert (M + KC["COLSUM_SLAB_ROWS"] - 1) // KC["COLSUM_SLAB_ROWS"] > KC["COLSUM_MAX_SLABS"] and plan["rpb"] > KC["COLSUM_SLAB_ROWS"]
        for N in RR.colsum_widths(M, in_dt):
            check_colsum(M, N, in_dt, N, True)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M", [7, 65, 512, 513])
def test_colsum_strided(M):
    """ld > N: the columns behind N hold NaN and must not be read into any sum; dense-only shortcuts must not be taken"""
    for in_dt, pad in ((F16, 24), (F32, 12)):
        assert not RR.colsum_plan(M, in_dt, dense=False)["direct"]
        check_colsum(M, 264, in_dt, 264 + pad, False, seed=1)


def test_colsum_out_slice():
    """ops.colsum(out=): the sums land in the slice, the buffer around it keeps its sentinel; out_dtype follows `out`"""
    for in_dt, out_dt, M in ((F16, F32, 1234), (F32, F16, 300), (F32, F32, 777), (F16, F16, 65)):
        N = 768
        x = RR.values("signed", (M, N), RR.gen(M, DEV), DEV).to(in_dt)
        x64 = x.double()
        ref = RR.colsum(x64)
        big = torch.full((3 * N,), SENT, dtype=out_dt, device=DEV)
        got = ops.colsum(x, out=big[N:2 * N], round_f16=False)
        torch.cuda.synchronize()
        assert got.data_ptr() == big[N:2 * N].data_ptr() and untouched(big[:N]) and untouched(big[2 * N:])
        bound = RR.colsum_bound(x64, ref, RR.colsum_plan(M, in_dt), out_dt == F16)
        within(big[N:2 * N], ref, bound, f"colsum out= {in_dt} -> {out_dt} M {M}", "colsum.signed")
        fresh = ops.colsum(x, out_dtype=out_dt)
        assert torch.equal(fresh, big[N:2 * N])


# ============================================================================= text_embed_bwd

def run_text_embed_bwd(ids, dx, vocab):
    D = dx.shape[-1]
    outs = []
    for _ in range(2):
        buf, out = guarded((vocab, D), F32, fill=0.0)
        call("hmmc_text_embed_bwd", ptr(ids), ptr(dx), ptr(out), ids.numel(), D, vocab, dtc(dx.dtype))
        torch.cuda.synchronize()
        guards_intact(buf, "text_embed_bwd dtable")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "text_embed_bwd: two runs differ"
    return outs[0]


def check_text_embed_bwd(ids_cpu, vocab, D, dtypes, tag):
    ids = ids_cpu.to(DEV)
    never = (RR.te_counts(ids, vocab) == 0)
    assert bool(never.any()) and bool(((ids < 0) | (ids >= vocab)).any())
    for dt in dtypes:
        for family in RR.FAMILIES + ("exact",):
            dx = RR.values(family, (ids.numel(), D), RR.gen(ids.numel() + D, DEV), DEV).to(dt)
            got = run_text_embed_bwd(ids, dx, vocab)
            ref = RR.text_embed_bwd(ids, dx, vocab)
            assert not bool(got[never].any()), f"{tag}: a row of an id that never occurs is not zero"
            if family == "exact":
                same(got.double(), ref, f"{tag} {dt} exact")
            else:
                within(got, ref, RR.text_embed_bwd_bound(ids, dx, vocab), f"{tag} {dt} {family}", f"text_embed_bwd.{family}")
        again = ops.text_embed_bwd(ids.view(-1, 1), dx, vocab)
        assert torch.equal(again, got), f"{tag}: hmmc_amd.ops gives other bits"


@pytest.mark.parametrize("name", list(RR.TE_LONG_CASES))
def test_text_embed_bwd_long(name):
    """the occurrence list: exactly full, one more, several batches inside one window, both batch limits (module docstring)"""
    rows, vocab, heavy, first = RR.TE_LONG_CASES[name]
    ids = RR.te_pattern(rows, vocab, heavy, first, len(name))
    n = int((ids == 0).sum())
    hits = (ids == 0).nonzero().flatten()
    assert int(hits[0]) >= first > 0
    if name == "n16384":
        assert n == KC["TE_LIST"]
    elif name == "n16385":
        assert n == KC["TE_LIST"] + 1
    else:
        assert n > 2 * KC["TE_LIST"]
    if name == "both_limits":
        window = ids[:KC["TE_WINDOW"]], ids[KC["TE_WINDOW"]:2 * KC["TE_WINDOW"]]
        assert rows > 2 * KC["TE_WINDOW"] and int((window[0] == 0).sum()) < KC["TE_LIST"] < int((window[1] == 0).sum())
    else:
        assert rows < KC["TE_WINDOW"]
    check_text_embed_bwd(ids, vocab, 8, (F16, F32), name)


@pytest.mark.parametrize("rows,vocab,D", RR.TE_WIDE_CASES)
def test_text_embed_bwd_wide(rows, vocab, D):
    """one column block (D = 8, 512) and a second one of 8 or 256 columns (D = 520, 768), fp16 and fp32 dx"""
    check_text_embed_bwd(RR.te_wide_ids(rows, vocab), vocab, D, (F16, F32), f"text_embed_bwd rows {rows} D {D}")


# ============================================================================= patchify

MEAN, STD = ops.CLIP_PIXEL_MEAN, ops.CLIP_PIXEL_STD


def c3(v):
    return (ctypes.c_float * 3)(*v)


def run_patchify(img, p, dt):
    n, _, H, W = img.shape
    g = H // p
    buf, out = guarded((n * (g * g + 1), 3 * p * p), dt)
    call("hmmc_patchify", ptr(img), ptr(out), n, H, W, p, dtc(dt))
    torch.cuda.synchronize()
    guards_intact(buf, "patchify out")
    return out


def run_patchify_u8(u8, fi, p, dt):
    _, _, H, W = u8.shape
    n = u8.shape[0] if fi is None else fi.numel()
    g = H // p
    buf, out = guarded((n * (g * g + 1), 3 * p * p), dt)
    call("hmmc_patchify_u8", ptr(u8), ptr(fi), ptr(out), n, H, W, p, c3(MEAN), c3(STD), dtc(dt))
    torch.cuda.synchronize()
    guards_intact(buf, "patchify_u8 out")
    return out


@pytest.mark.parametrize("H,p", [(224, 32), (224, 16), (64, 32), (32, 8), (32, 16)])
def test_patchify(H, p):
    """the layout against its definition, fp16 and fp32 outputs; the uint8 form with the loader's normalisation (evaluated on the
    CPU) and every kind of frame_index"""
    n = 3
    img = torch.randn(n, 3, H, H, generator=RR.gen(H + p))
    u8 = torch.randint(0, 256, (n, 3, H, H), generator=RR.gen(H + p + 1), dtype=torch.uint8)
    nf = RR.normalise_u8(u8, MEAN, STD).to(DEV)
    img_d, u8_d = img.to(DEV), u8.to(DEV)
    indexes = {"none": None, "repeats": [2, 2, 0, 2], "reversed": [2, 1, 0], "m > n": [0, 1, 2, 1, 0, 2, 2], "m = 1": [1]}
    for dt in (F16, F32):
        same(run_patchify(img_d, p, dt), RR.patchify(img_d, p, dt), f"patchify {H} / {p} {dt}")
        same(ops.patchify(img_d, p, dtype=dt), RR.patchify(img_d, p, dt), f"ops.patchify {H} / {p} {dt}")
        for name, fi in indexes.items():
            fi_d = None if fi is None else torch.tensor(fi, dtype=torch.int32, device=DEV)
            ref = RR.patchify_u8(nf, fi_d, p, dt)
            same(run_patchify_u8(u8_d, fi_d, p, dt), ref, f"patchify_u8 {H} / {p} {dt} frame_index {name}")
            same(ops.patchify_u8(u8_d, p, frame_index=fi_d, dtype=dt), ref, f"ops.patchify_u8 {H} / {p} {dt} frame_index {name}")


def test_patchify_grid_wrap():
    """more 16-byte chunks than one sweep of the capped grid: idx / kc, row % L and row / L past the first sweep"""
    H, p, n = 64, 32, 1100
    chunks = n * ((H // p) ** 2 + 1) * (3 * p * p // 8)
    assert chunks > KC["PATCHIFY_CAP"] * KC["BLOCK"], "the launch no longer passes the grid cap"
    img = torch.randn(n, 3, H, H, generator=RR.gen(1, DEV), device=DEV)
    for dt in (F16, F32):
        same(run_patchify(img, p, dt), RR.patchify(img, p, dt), f"patchify grid wrap {dt}")
    del img
    u8 = torch.randint(0, 256, (3, 3, H, H), generator=RR.gen(2), dtype=torch.uint8)
    nf = RR.normalise_u8(u8, MEAN, STD).to(DEV)
    fi = torch.randint(0, 3, (n,), generator=RR.gen(3)).to(torch.int32).to(DEV)
    for dt in (F16, F32):
        same(run_patchify_u8(u8.to(DEV), fi, p, dt), RR.patchify_u8(nf, fi, p, dt), f"patchify_u8 grid wrap {dt}")
    torch.cuda.empty_cache()


# ============================================================================= vit_embed, text_embed

def embed_tables(L, D, seed):
    g = RR.gen(seed, DEV)
    return torch.randn(D, generator=g, device=DEV), torch.randn(L + 2, D, generator=g, device=DEV)


def run_vit_embed(x, cls, pos, L):
    buf, view = guarded(tuple(x.shape), x.dtype)
    view.copy_(x)
    call("hmmc_vit_embed", ptr(view), ptr(cls), ptr(pos), x.shape[0], L, x.shape[1], dtc(x.dtype))
    torch.cuda.synchronize()
    guards_intact(buf, "vit_embed x")
    return view


def run_text_embed(ids, table, pos, dt):
    b, L = ids.shape
    D = table.shape[1]
    buf, out = guarded((b * L, D), dt)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("hmmc_text_embed", ptr(ids), ptr(table), ptr(pos), ptr(out), b * L, L, D, table.shape[0], ptr(flag), dtc(dt))
    torch.cuda.synchronize()
    guards_intact(buf, "text_embed x")
    return out, bool(flag.item())


@pytest.mark.parametrize("L", [1, 10, 50, 77, 197])
def test_vit_embed(L):
    """class rows arrive holding garbage and leave as cls + pos[0]; fp16 rounds cls, pos and the sum, fp32 nothing"""
    for D in (8, 128, 768):
        cls, pos = embed_tables(L, D, L + D)
        for dt in (F16, F32):
            x = torch.randn(3 * L, D, generator=RR.gen(L, DEV), device=DEV).to(dt)
            ref = RR.vit_embed(x, cls, pos, L)
            same(run_vit_embed(x, cls, pos, L), ref, f"vit_embed L {L} D {D} {dt}")
            same(ops.vit_embed_(x.clone(), cls, pos, L), ref, f"ops.vit_embed_ L {L} D {D} {dt}")


@pytest.mark.parametrize("L", [1, 10, 50, 77, 197])
def test_text_embed(L):
    """ids 0 and vocab - 1 among random ones; then ids outside the table: the position row alone, the flag raised"""
    vocab, b = 300, 3
    for D in (8, 128, 768):
        _, pos = embed_tables(L, D, L + D)
        table = torch.randn(vocab, D, generator=RR.gen(D, DEV), device=DEV)
        ids = torch.randint(0, vocab, (b, L), generator=RR.gen(L))
        ids[0, 0], ids[b - 1, L - 1] = 0, vocab - 1
        bad = ids.clone()
        bad[1, L // 2], bad[2, 0] = vocab, -1
        ids, bad = ids.to(DEV), bad.to(DEV)
        for dt in (F16, F32):
            ref, _ = RR.text_embed(ids, table, pos, dt)
            got, flagged = run_text_embed(ids, table, pos, dt)
            assert not flagged
            same(got, ref, f"text_embed L {L} D {D} {dt}")
            same(ops.text_embed(ids, table, pos, dtype=dt), ref, f"ops.text_embed L {L} D {D} {dt}")
            ops.raise_on_device_errors()                              # nothing was flagged
            refb, any_bad = RR.text_embed(bad, table, pos, dt)
            gotb, flagged = run_text_embed(bad, table, pos, dt)
            assert any_bad and flagged, "an id outside the table did not raise the flag"
            same(gotb, refb, f"text_embed with ids outside the table L {L} D {D} {dt}")
            same(ops.text_embed(bad, table, pos, dtype=dt), refb, f"ops.text_embed with ids outside the table L {L} D {D} {dt}")
            with pytest.raises(IndexError):
                ops.raise_on_device_errors()
            ops.raise_on_device_errors()                              # the flag was cleared


def test_embed_grid_wrap():
    """more chunks than one sweep of the 4096-block grids: row % L and the table row of a chunk past the first sweep"""
    D = 768
    L, n = 197, 56
    assert n * L * (D // 8) > KC["EMBED_CAP"] * KC["BLOCK"], "vit_embed no longer passes the grid cap"
    cls, pos = embed_tables(L, D, 1)
    for dt in (F16, F32):
        x = torch.randn(n * L, D, generator=RR.gen(2, DEV), device=DEV).to(dt)
        same(run_vit_embed(x, cls, pos, L), RR.vit_embed(x, cls, pos, L), f"vit_embed grid wrap {dt}")
    L, b, vocab = 77, 142, 500
    assert b * L * (D // 8) > KC["EMBED_CAP"] * KC["BLOCK"], "text_embed no longer passes the grid cap"
    _, pos = embed_tables(L, D, 3)
    table = torch.randn(vocab, D, generator=RR.gen(4, DEV), device=DEV)
    ids = torch.randint(0, vocab, (b, L), generator=RR.gen(5)).to(DEV)
    for dt in (F16, F32):
        got, flagged = run_text_embed(ids, table, pos, dt)
        assert not flagged
        same(got, RR.text_embed(ids, table, pos, dt)[0], f"text_embed grid wrap {dt}")


# ============================================================================= eot_index

def run_eot_index(ids, base, stride):
    b, L = ids.shape
    buf, out = guarded((b,), torch.int32)
    call("hmmc_eot_index", ptr(ids), ptr(out), b, L, base, stride)
    torch.cuda.synchronize()
    guards_intact(buf, "eot_index")
    return out


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 77, 128, 1024])
def test_eot_index(L):
    """torch.argmax's first-occurrence rule across and inside lanes (RR.eot_ids' eight row patterns, rotated so that every b meets
    every pattern), plain rows (base 0, stride L) and the rows of a batch padded to Lmax = L + 3 that starts at caption 5"""
    Lmax, row0 = L + 3, 5
    for b in (1, 3, 4, 5, 257):
        for shift in range(8):
            ids_c = RR.eot_ids(b, L, shift)
            ids = ids_c.to(DEV)
            same(run_eot_index(ids, 0, L).cpu(), RR.eot_index(ids_c), f"eot_index L {L} b {b} shift {shift}")
            same(run_eot_index(ids, row0 * Lmax, Lmax).cpu(), RR.eot_index(ids_c, row0 * Lmax, Lmax), f"eot_index L {L} b {b} shift {shift} strided")
        same(ops.eot_index(ids).cpu(), RR.eot_index(ids_c), f"ops.eot_index L {L} b {b}")
        same(ops.eot_index(ids, base=row0 * Lmax, stride=Lmax).cpu(), RR.eot_index(ids_c, row0 * Lmax, Lmax), f"ops.eot_index L {L} b {b} strided")


# ============================================================================= cast

@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 3])
def test_cast(n):
    """fp32 -> fp16 (round to nearest even, overflow to inf, subnormals) and fp16 -> fp32 (exact), bit for bit with the host's
    conversion; the longest n takes a second sweep of the capped grid"""
    if n > 257:
        assert n > KC["CAST_CAP"] * KC["BLOCK"], "the launch no longer passes the grid cap"
    for to_half in (True, False):
        src_c = RR.cast_values(n, to_half)
        ref = src_c.half() if to_half else src_c.float()
        src = src_c.to(DEV)
        buf, out = guarded((n,), F16 if to_half else F32)
        call("hmmc_cast", ptr(src), ptr(out), n, int(to_half))
        torch.cuda.synchronize()
        guards_intact(buf, "cast out")
        assert not bool(torch.isnan(out).any())
        assert RR.same_bits(out.cpu(), ref), f"cast n {n} to_half {to_half}: {int((out.cpu() != ref).sum())} values differ"
        assert RR.same_bits(ops.cast(src, F16 if to_half else F32).cpu(), ref)


# ============================================================================= statuses

def test_statuses():
    """every rejected argument set comes back as its status BEFORE any launch (norm_elem.hip checks all of them on the host), and
    the sentinel-filled output is untouched.  Every pointer is valid and every buffer large enough for the nearest valid shape."""
    U, A, W = STATUS["HMMC_ERR_UNSUPPORTED"], STATUS["HMMC_ERR_ARG"], STATUS["HMMC_ERR_WORKSPACE"]
    x16 = torch.ones(520, 24, dtype=F16, device=DEV)
    x32 = torch.ones(520, 24, dtype=F32, device=DEV)
    ws = torch.full((1 << 16,), SENT, dtype=F32, device=DEV)
    out = torch.full((4096,), SENT, dtype=F32, device=DEV)

    def clean(what):
        assert untouched(out) and untouched(ws), f"{what}: an output was written"
    # colsum: N or ld not a multiple of the vector width (8 halves, 4 floats)
    for args, what in (((x16, 16, 12, 24, 0), "fp16 N = 12"), ((x16, 16, 16, 20, 0), "fp16 ld = 20"), ((x32, 16, 6, 24, 1), "fp32 N = 6"),
                       ((x32, 16, 8, 10, 1), "fp32 ld = 10")):
        x, M, N, ld, dt = args
        assert status("hmmc_colsum", ptr(x), ptr(out), M, N, ld, dt, 1, 0, ptr(ws), ws.numel() * 4) == U, what
        clean(f"colsum {what}")
    # colsum: the two-launch path with a workspace one byte short of the slabs it writes
    for x, M, dt in ((x16, 65, 0), (x32, 513, 1)):
        plan = RR.colsum_plan(M, F16 if dt == 0 else F32)
        need = plan["rb"] * 24 * 4
        assert not plan["direct"] and need <= query("hmmc_colsum_workspace", M, 24)
        assert status("hmmc_colsum", ptr(x), ptr(out), M, 24, 24, dt, 1, 0, ptr(ws), need - 1) == W
        clean("colsum short workspace")
        assert status("hmmc_colsum", ptr(x), ptr(out), M, 24, 24, dt, 1, 0, None, 0) == W
        clean("colsum without a workspace")
    # patchify: H != W; a patch that is no multiple of 8
    img = torch.ones(2, 3, 64, 64, device=DEV)
    assert status("hmmc_patchify", ptr(img), ptr(out), 1, 64, 32, 32, 1) == U
    assert status("hmmc_patchify", ptr(img), ptr(out), 1, 24, 24, 12, 1) == U
    clean("patchify")
    # patchify_u8: W no multiple of 8 (36 = 3 x 12); a frame pointer 4 bytes off an 8-byte boundary
    u8 = torch.ones(2 * 3 * 64 * 64 + 8, dtype=torch.uint8, device=DEV)
    assert u8.data_ptr() % 8 == 0
    assert status("hmmc_patchify_u8", ptr(u8), None, ptr(out), 1, 36, 36, 12, c3(MEAN), c3(STD), 1) == U
    assert status("hmmc_patchify_u8", ptr(u8[4:]), None, ptr(out), 1, 32, 32, 8, c3(MEAN), c3(STD), 1) == U
    clean("patchify_u8")
    # eot_index: L = 1025; stride < L; base + b stride past 2^31 - 1
    idx = torch.full((64,), int(SENT), dtype=torch.int32, device=DEV)
    ids = torch.ones(4, 1025, dtype=torch.int64, device=DEV)
    assert status("hmmc_eot_index", ptr(ids), ptr(idx), 4, KC["EOT_MAX_L"] + 1, 0, 1025) == A
    assert status("hmmc_eot_index", ptr(ids), ptr(idx), 4, 77, 0, 76) == U
    assert status("hmmc_eot_index", ptr(ids), ptr(idx), 4, 77, 2 ** 31 - 1 - 4 * 77 + 1, 77) == U
    assert status("hmmc_eot_index", ptr(ids), ptr(idx), 4, 77, 0, 2 ** 29) == U
    assert bool((idx == int(SENT)).all()), "eot_index: the output was written"
    # text_embed_bwd and vit_embed: D no multiple of 8
    tok = torch.zeros(16, dtype=torch.int64, device=DEV)
    assert status("hmmc_text_embed_bwd", ptr(tok), ptr(x16), ptr(out), 16, 12, 4, 0) == U
    clean("text_embed_bwd D = 12")
    xin = torch.full((16, 12), SENT, dtype=F16, device=DEV)
    assert status("hmmc_vit_embed", ptr(xin), ptr(x32), ptr(x32), 16, 4, 12, 0) == A
    assert untouched(xin), "vit_embed D = 12: x was written"
    # and the nearest valid arguments are taken
    assert status("hmmc_eot_index", ptr(ids), ptr(idx), 4, 77, 2 ** 31 - 1 - 4 * 77, 77) == 0
    assert status("hmmc_colsum", ptr(x16), ptr(out), 65, 24, 24, 0, 1, 0, ptr(ws), RR.colsum_plan(65, F16)["rb"] * 24 * 4) == 0
    assert float(out[0]) == 65.0


def test_zz_report_worst_ratios():
    """not a check of the kernels: the worst err / (SLACK bound) against fp64 per family, for the record (run the module as a
    whole, with -s)"""
    for fam in ("colsum", "text_embed_bwd"):
        for family in RR.FAMILIES:
            assert f"{fam}.{family}" in WORST, f"no bounded comparison ran on {fam}, {family} data"
    for fam in sorted(WORST):
        print(f"rowops-worst {fam}: {WORST[fam]:.3f}")
