"""CPU checks of tests/rowops_ref.py, the statements and bounds behind tests/test_gpu_rowops.py:
  * the constants the cases are sized by are those norm_elem.hip states (a changed grid cap or threshold fails here);
  * every statement is pinned against an independent formulation: F.unfold, F.embedding and its autograd, index_add_ and a
    one-hot product in fp64, torch.argmax, hand-computed fp16 roundings;
  * the bounds are not too tight: a torch emulation of each accumulating kernel's summation order lies inside SLACK x bound on
    every shape and input family the GPU test runs, and is exact on the integer family;
  * the checks are not too loose (test_slip_*): each plausible kernel mistake falls outside the bound, or fails the equality, on
    a case the GPU test runs."""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as RR

D64 = torch.float64
F16, F32 = torch.float16, torch.float32


def test_constants_are_those_of_the_source():
    kc = RR.kernel_constants()
    for name, value in kc.items():
        assert getattr(RR, name) == value, f"{name}: rowops_ref has {getattr(RR, name)}, norm_elem.hip {value}"


# ============================================================================= the statements are pinned

@pytest.mark.parametrize("H,p", [(224, 32), (224, 16), (64, 32), (32, 8), (32, 16)])
def test_patchify_is_unfold(H, p):
    n, g = 3, H // p
    img = torch.randn(n, 3, H, H, generator=RR.gen(H + p))
    ref = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2)                   # [n, g g, 3 p p], columns (c, ky, kx)
    for dt in (F16, F32):
        out = RR.patchify(img, p, dt).view(n, g * g + 1, -1)
        assert out.dtype == dt and torch.equal(out[:, 1:], ref.to(dt)) and not bool(out[:, 0].any())
    # and one element by hand: frame 1, patch (gy, gx) = (g - 1, 0), channel 2, ky 3, kx 5
    out = RR.patchify(img, p, F32).view(n, g * g + 1, -1)
    assert float(out[1, 1 + (g - 1) * g, 2 * p * p + 3 * p + 5]) == float(img[1, 2, (g - 1) * p + 3, 5])
    # conv1 on the frame == the patch rows times the flattened weight
    w = torch.randn(4, 3, p, p, generator=RR.gen(1), dtype=D64)
    conv = F.conv2d(img.double(), w, stride=p).flatten(2).transpose(1, 2)
    assert float((out[:, 1:].double() @ w.flatten(1).t() - conv).abs().max()) < 1e-10


def test_patchify_u8_is_the_loader_normalisation():
    from hmmc_amd import ops
    u8 = torch.randint(0, 256, (4, 3, 32, 32), generator=RR.gen(5), dtype=torch.uint8)
    mean = torch.tensor(ops.CLIP_PIXEL_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(ops.CLIP_PIXEL_STD).view(1, 3, 1, 1)
    f32 = (u8.float().div(255.0) - mean) / std
    nf = RR.normalise_u8(u8, ops.CLIP_PIXEL_MEAN, ops.CLIP_PIXEL_STD)
    assert nf.dtype == F32 and torch.equal(nf, f32)
    fi = torch.tensor([3, 3, 0, 2, 1, 0], dtype=torch.int32)
    out = RR.patchify_u8(nf, fi, 8, F16).view(6, 17, -1)
    for i, s in enumerate(fi.tolist()):
        assert torch.equal(out[i], RR.patchify(f32[s:s + 1], 8, F16))
    assert torch.equal(RR.patchify_u8(nf, None, 8, F32), RR.patchify(f32, 8, F32))


@pytest.mark.parametrize("dt", [F16, F32])
def test_vit_embed_is_class_token_plus_position(dt):
    L, D, n = 10, 16, 3
    g = RR.gen(3)
    x = torch.randn(n * L, D, generator=g).to(dt)
    cls, pos = torch.randn(D, generator=g), torch.randn(L, D, generator=g)
    ref = x.clone().view(n, L, D)
    ref[:, 0] = cls.to(dt)                                            # torch.cat([class_embedding.to(x.dtype) + zeros, x[:, 1:]])
    ref = (ref + pos.to(dt)).view(n * L, D)                           # x + positional_embedding.to(x.dtype), in x's own arithmetic
    assert torch.equal(RR.vit_embed(x, cls, pos, L), ref)


@pytest.mark.parametrize("dt", [F16, F32])
def test_text_embed_is_embedding_plus_position(dt):
    b, L, D, vocab = 5, 7, 16, 30
    g = RR.gen(4)
    ids = torch.randint(0, vocab, (b, L), generator=g)
    ids[0, 0], ids[1, 1] = 0, vocab - 1
    table, pos = torch.randn(vocab, D, generator=g), torch.randn(L + 2, D, generator=g)
    x, bad = RR.text_embed(ids, table, pos, dt)
    assert not bad and torch.equal(x, (F.embedding(ids, table).to(dt) + pos[:L].to(dt)).view(b * L, D))
    ids[2, 3], ids[4, 6] = vocab, -1
    x2, bad = RR.text_embed(ids, table, pos, dt)
    assert bad
    x2, x = x2.view(b, L, D), x.view(b, L, D)
    assert torch.equal(x2[2, 3], pos[3].to(dt)) and torch.equal(x2[4, 6], pos[6].to(dt))
    keep = torch.ones(b, L, dtype=torch.bool)
    keep[2, 3] = keep[4, 6] = False
    assert torch.equal(x2[keep], x[keep])


def test_eot_index_is_argmax():
    for L in (1, 2, 63, 64, 65, 77, 128, 1024):
        for shift in range(8):
            ids = RR.eot_ids(5, L, shift)
            am = torch.argmax(ids, dim=-1)                            # the first of several maxima
            assert torch.equal(RR.eot_index(ids), (torch.arange(5) * L + am).to(torch.int32))
            assert torch.equal(RR.eot_index(ids, base=35, stride=L + 3), (35 + torch.arange(5) * (L + 3) + am).to(torch.int32))
            for i in range(5):                                        # and by the definition, row by row
                row = ids[i].tolist()
                assert int(am[i]) == row.index(max(row))


def test_eot_patterns_hold_what_they_promise():
    """ties inside one lane's positions (l, l + 64), in neighbouring lanes, first occurrence at 0 and at L - 1, equal rows, negative rows"""
    for L in (65, 77, 128, 1024):
        ids = RR.eot_ids(8, L, 0)
        top = ids.max(1, keepdim=True).values
        where = [(ids[i] == top[i]).nonzero().flatten().tolist() for i in range(8)]
        assert len(where[0]) == 1
        assert len(where[1]) == 2 and (where[1][1] - where[1][0]) % 64 == 0
        assert len(where[2]) == 2 and where[2][1] - where[2][0] == 1
        assert where[3] == [0, L - 1] and where[4] == [L - 1]
        assert len(where[5]) == L and bool((ids[6] < 0).all()) and len(where[6]) == 2
        assert where[7][-1] == L - 1 and len(where[7]) > 1


def test_text_embed_bwd_is_embedding_autograd():
    rows, vocab, D = 300, 12, 16
    ids = RR.te_wide_ids(rows, vocab)
    dx = torch.randn(rows, D, generator=RR.gen(1), dtype=D64)
    ref = RR.text_embed_bwd(ids, dx, vocab)
    ok = (ids >= 0) & (ids < vocab)
    w = torch.zeros(vocab, D, dtype=D64, requires_grad=True)
    F.embedding(ids[ok], w).backward(dx[ok])
    assert float((ref - w.grad).abs().max()) < 1e-12
    onehot = (ids[:, None] == torch.arange(vocab)[None, :]).to(D64)   # a row of an id outside the table matches no column
    assert float((ref - onehot.t() @ dx).abs().max()) < 1e-12
    assert not bool(ref[vocab - 1].any()) and int(RR.te_counts(ids, vocab)[vocab - 1]) == 0


def test_colsum_is_a_product_with_ones():
    x = torch.randn(37, 24, generator=RR.gen(2), dtype=D64)
    assert float((RR.colsum(x) - torch.ones(37, dtype=D64) @ x).abs().max()) < 1e-12
    assert RR.colsum(x.half()).dtype == D64


def test_cast_roundings_by_hand():
    v = RR.cast_values(64, True)
    h = v.half()
    expect = {1.0 + 2.0 ** -11: 1.0, 1.0 + 3 * 2.0 ** -11: 1.0 + 2.0 ** -9, 2049.0: 2048.0, 2051.0: 2052.0, 65504.0: 65504.0,
              65520.0: float("inf"), -65520.0: float("-inf"), 2.0 ** -24: 2.0 ** -24, 2.0 ** -25: 0.0, 3 * 2.0 ** -25: 2.0 ** -23,
              1e-10: 0.0}
    seen = 0
    expect = {float(torch.tensor(k, dtype=F32)): d for k, d in expect.items()}
    for src, dst in zip(v.tolist(), h.tolist()):
        if src in expect:
            assert dst == expect[src], (src, dst)
            seen += 1
    assert seen >= len(expect)
    assert float(h[2]) == 1.0 + 2.0 ** -10 and float(h[6]) == 65504.0 and float(h[12]) == 2.0 ** -24      # just past a tie: up
    back = RR.cast_values(300, False)
    assert back.dtype == F16 and not bool(torch.isnan(back).any()) and bool(torch.isinf(back).any())
    assert RR.same_bits(back.float().half(), back) and not RR.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_colsum_plans():
    """the 512 / 513 switch, the slab arithmetic and the 1024-slab cap, as hmmc_colsum computes them"""
    P = RR.colsum_plan
    assert P(512, F32)["direct"] and not P(513, F32)["direct"] and not P(512, F16)["direct"] and not P(512, F32, dense=False)["direct"]
    assert P(64, F16) == dict(direct=False, rb=1, rpb=64) and P(65, F16) == dict(direct=False, rb=2, rpb=33)
    assert P(513, F32) == dict(direct=False, rb=9, rpb=57) and P(4097, F16) == dict(direct=False, rb=65, rpb=64)
    big = P(65537, F16)
    assert big == dict(direct=False, rb=1009, rpb=65) and (65537 + 63) // 64 > RR.COLSUM_MAX_SLABS       # crosses the cap
    assert RR.colsum_workspace(65537, 8) == 1024 * 8 * 4 >= big["rb"] * 8 * 4
    assert min(RR.colsum_chain(P(M, dt)) for M in RR.COLSUM_M for dt in (F16, F32)) == 10


def test_te_batches():
    import numpy as np
    hits = np.arange(7, 40000)                                        # "dense": 32 chunks fill the list exactly
    b = RR.te_batches(hits, 40000)
    assert [x.size for x in b] == [16384, 16384, 40000 - 7 - 32768] and int(b[1][0]) == 7 + 16384
    ids = RR.te_pattern(*_long("n16384"))
    h = (ids.numpy() == 0).nonzero()[0]
    assert h.size == 16384 and h[0] >= 5 and [x.size for x in RR.te_batches(h, ids.numel()) if x.size] == [16384]
    ids = RR.te_pattern(*_long("n16385"))
    h = (ids.numpy() == 0).nonzero()[0]
    sizes = [x.size for x in RR.te_batches(h, ids.numel()) if x.size]
    assert sizes == [16384, 1]                                        # a list that is exactly full, then the one that is left
    ids = RR.te_pattern(*_long("n39k"))
    h = (ids.numpy() == 0).nonzero()[0]
    sizes = [x.size for x in RR.te_batches(h, ids.numel())]
    assert ids.numel() < RR.TE_WINDOW and 38000 < h.size and len(sizes) == 3
    assert RR.TE_LIST - RR.TE_THREADS < sizes[0] < RR.TE_LIST and sizes[0] == sizes[1]      # ends in the middle of the occurrences, room left
    ids = RR.te_pattern(*_long("both_limits"))
    h = (ids.numpy() == 0).nonzero()[0]
    b = RR.te_batches(h, ids.numel())
    spans = [(int(x[0]), int(x[-1]), x.size) for x in b if x.size]
    assert any(n < RR.TE_LIST - RR.TE_THREADS and hi - lo > RR.TE_WINDOW - 2 * RR.TE_THREADS for lo, hi, n in spans), spans    # ended by the window
    assert any(n > RR.TE_LIST - RR.TE_THREADS for lo, hi, n in spans), spans                                                # ended by the list
    for x in b:                                                       # every offset fits 16 bits, every batch the list
        assert x.size <= RR.TE_LIST and (x.size == 0 or int(x[-1]) - int(x[0]) < RR.TE_WINDOW)
    assert sum(x.size for x in b) == h.size


def _long(name):
    rows, vocab, heavy, first = RR.TE_LONG_CASES[name]
    return rows, vocab, heavy, first, len(name)


# ============================================================================= the emulations lie inside the bounds

def colsum_inputs(M, N, dt, family):
    return RR.values(family, (M, N), RR.gen(M + N)).to(dt)


@pytest.mark.parametrize("M", RR.COLSUM_M)
def test_emulated_colsum_is_within_the_bound(M):
    worst = 0.0
    for dt in (F16, F32):
        plan = RR.colsum_plan(M, dt)
        for N in RR.colsum_widths(M, dt):
            for family in RR.FAMILIES + ("exact",):
                x = colsum_inputs(M, N, dt, family)
                x64 = x.double()
                ref = RR.colsum(x64)
                for out_dt in (F16, F32):
                    for rf in (0, 1):
                        got = RR.emulate_colsum(x, plan, out_dt, rf)
                        half = out_dt == F16 or bool(rf)
                        if family == "exact":
                            assert float(x64.abs().sum(0).max()) < 2 ** 24
                            assert torch.equal(got.double(), ref.half().double() if half else ref), (M, N, dt, out_dt, rf)
                        else:
                            r = RR.within_ratio(got, ref, RR.colsum_bound(x64, ref, plan, half))
                            worst = max(worst, r)
                            assert r <= 1.0, (M, N, dt, family, out_dt, rf, r)
    print(f"rowops-emulation colsum M {M}: worst err / (SLACK bound) {worst:.3f}")


def te_case(name_or_shape, family, dt):
    if isinstance(name_or_shape, str):
        ids = RR.te_pattern(*_long(name_or_shape))
        vocab, D = RR.TE_LONG_CASES[name_or_shape][1], 8
    else:
        rows, vocab, D = name_or_shape
        ids = RR.te_wide_ids(rows, vocab)
    dx = RR.values(family, (ids.numel(), D), RR.gen(ids.numel() + D)).to(dt)
    return ids, dx, vocab


@pytest.mark.parametrize("case", list(RR.TE_LONG_CASES) + RR.TE_WIDE_CASES, ids=str)
def test_emulated_text_embed_bwd_is_within_the_bound(case):
    for dt in (F16, F32):
        for family in RR.FAMILIES + ("exact",):
            if isinstance(case, str) and (dt, family) not in ((F16, "same"), (F32, "signed"), (F16, "exact")):
                continue                                              # the long cases: one pass per family is enough on the CPU
            ids, dx, vocab = te_case(case, family, dt)
            ref = RR.text_embed_bwd(ids, dx, vocab)
            got = RR.emulate_text_embed_bwd(ids, dx, vocab)
            if family == "exact":
                assert torch.equal(got.double(), ref), (case, dt)
            else:
                b = RR.text_embed_bwd_bound(ids, dx, vocab)
                never = RR.te_counts(ids, vocab) == 0
                assert bool(never.any()) and not bool(b[never].any()) and not bool(got[never].any())
                bad = ~((got.double() - ref).abs() <= RR.SLACK * b)
                assert not bool(bad.any()), (case, dt, family, int(bad.sum()))
                r = RR.within_ratio(got[~never], ref[~never], b[~never])
                print(f"rowops-emulation text_embed_bwd {case} {dt} {family}: worst err / (SLACK bound) {r:.3f}")


# ============================================================================= plausible mistakes are seen

@pytest.mark.parametrize("slip", RR.COLSUM_SLIPS)
def test_slip_colsum(slip):
    """seen at every M of the GPU test where the mistake changes anything, in both bounded families, fp32 output (the tighter
    bound) and fp16 output; tail_row and short_slab are also unequal on the integer family"""
    seen = []
    for M in RR.COLSUM_M:
        if slip == "acc_f16" and M > 4097:
            continue                                                  # (a row-by-row loop; 4097 rows show it)
        for dt in (F16, F32):
            plan = RR.colsum_plan(M, dt)
            N = RR.colsum_widths(M, dt)[1]
            for family in RR.FAMILIES:
                x64 = colsum_inputs(M, N, dt, family).double()
                ref = RR.colsum(x64)
                bad = RR.colsum_slipped(x64, plan, slip)
                if bad is None or torch.equal(bad, ref):
                    continue
                if slip == "acc_f16" and (M < 513 or family == "signed"):
                    continue                                          # a short or cancelling fp16 sum stays within the fp16 OUTPUT's bound
                for half in ((False, True) if M <= 65 or slip == "acc_f16" else (False,)):      # one row of thousands is below fp16's step
                    assert RR.detects(ref, bad, RR.colsum_bound(x64, ref, plan, half)), (slip, M, dt, family, half)
                seen.append((M, dt, family))
            if slip != "acc_f16":
                xi = colsum_inputs(M, N, dt, "exact").double()
                bi = RR.colsum_slipped(xi, plan, slip)
                if bi is not None and slip == "short_slab":
                    assert not torch.equal(bi, RR.colsum(xi)), (slip, M, dt)
    Ms = {m for m, _, _ in seen}
    want = {"tail_row": {1, 9, 65, 513, 65537}, "short_slab": {65, 4097, 65537}, "acc_f16": {4097}}[slip]
    assert want <= Ms, (slip, sorted(Ms))


def test_slip_text_embed_bwd_first_batch_only():
    """everything after the first list batch dropped: unequal on the integer family at 16 385 occurrences (ONE dropped row, which
    the bound of a 16 385-term sum cannot see), outside the bound on same-sign data from three batches on"""
    ids, dx, vocab = te_case("n16385", "exact", F16)
    ref = RR.text_embed_bwd(ids, dx, vocab)
    bad = RR.emulate_text_embed_bwd(ids, dx, vocab, first_batch_only=True).double()
    assert torch.equal(bad[1:], ref[1:]) and not torch.equal(bad[0], ref[0])
    ids, dx, vocab = te_case("n16384", "exact", F16)                  # and nothing is lost where one batch holds everything
    assert torch.equal(RR.emulate_text_embed_bwd(ids, dx, vocab, first_batch_only=True).double(), RR.text_embed_bwd(ids, dx, vocab))
    for name in ("n39k", "dense", "both_limits"):
        ids, dx, vocab = te_case(name, "same", F16)
        ref, b = RR.text_embed_bwd(ids, dx, vocab), RR.text_embed_bwd_bound(ids, dx, vocab)
        import numpy as np
        h = (ids.numpy() == 0).nonzero()[0]
        first = RR.te_batches(h, ids.numel())[0]
        bad = ref.clone()
        bad[0] = dx.double()[torch.from_numpy(np.asarray(first))].sum(0)
        assert RR.detects(ref, bad, b), name


def test_slip_text_embed_bwd_second_column_block():
    for rows, vocab, D in RR.TE_WIDE_CASES:
        for family in RR.FAMILIES:
            ids, dx, vocab = te_case((rows, vocab, D), family, F16)
            ref, b = RR.text_embed_bwd(ids, dx, vocab), RR.text_embed_bwd_bound(ids, dx, vocab)
            bad = ref.clone()
            bad[:, 512:] = 0
            assert RR.detects(ref, bad, b) == (D > 512), (D, family)


def test_slip_eot_index_last_maximum():
    hit = 0
    for L in (2, 63, 64, 65, 77, 128, 1024):
        for shift in range(8):
            ids = RR.eot_ids(5, L, shift)
            hit += int(not torch.equal(RR.eot_index(ids), RR.eot_index(ids, last=True)))
        assert hit, L
    ids = RR.eot_ids(1, 1, 0)
    assert torch.equal(RR.eot_index(ids), RR.eot_index(ids, last=True))


def test_slip_patchify_ky_kx_swapped():
    for H, p in [(224, 32), (224, 16), (64, 32), (32, 8), (32, 16)]:
        img = torch.randn(2, 3, H, H, generator=RR.gen(H))
        assert not torch.equal(RR.patchify(img, p, F16), RR.patchify(img, p, F16, swap=True))


def embed_inputs(L, D, dt, n=3):
    g = RR.gen(L + D)
    x = torch.randn(n * L, D, generator=g).to(dt)                     # class rows hold garbage too
    return x, torch.randn(D, generator=g), torch.randn(L + 2, D, generator=g)


def test_slip_vit_embed_adds_to_the_class_row():
    for dt in (F16, F32):
        for L in (1, 10, 50):
            x, cls, pos = embed_inputs(L, 8, dt)
            assert not torch.equal(RR.vit_embed(x, cls, pos, L), RR.vit_embed(x, cls, pos, L, add_cls=True))
    x, cls, pos = embed_inputs(10, 8, F16)
    x.view(3, 10, 8)[:, 0] = 0                                        # with zero class rows the mistake is invisible: hence the garbage
    assert torch.equal(RR.vit_embed(x, cls, pos, 10), RR.vit_embed(x, cls, pos, 10, add_cls=True))


def test_slip_embed_rounds_once():
    for L, D in [(1, 8), (10, 128), (50, 768)]:
        x, cls, pos = embed_inputs(L, D, F16)
        assert not torch.equal(RR.vit_embed(x, cls, pos, L), RR.vit_embed(x, cls, pos, L, once=True))
        table = torch.randn(30, D, generator=RR.gen(D))
        ids = torch.randint(0, 30, (3, L), generator=RR.gen(L))
        assert not torch.equal(RR.text_embed(ids, table, pos, F16)[0], RR.text_embed(ids, table, pos, F16, once=True)[0])
        assert torch.equal(RR.text_embed(ids, table, pos, F32)[0], RR.text_embed(ids, table, pos, F32, once=True)[0])   # fp32 rounds nothing
