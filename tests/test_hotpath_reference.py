"""CPU checks of tests/hotpath_ref.py, the fp64 statements and rounding bounds behind tests/test_gpu_hotpath.py:
  * every statement is pinned: attention and LayerNorm to torch.nn.functional in fp64 and to the oracle, the written-out attention
    backward to autograd, QuickGELU and its derivative to the oracle and autograd, the GEMM epilogue formulas to F.linear + autograd, the weight
    gradient to torch.matmul and F.linear's autograd;
  * the bounds are not too tight: a torch emulation of each kernel's arithmetic (fp32, .half() at the kernel's rounding points) lies
    inside SLACK x bound in every input regime the GPU tests use (the worst err / (SLACK bound) per output is in the message and,
    with -s, on stdout);
  * the bounds are not too loose (test_slip_*): a plausible kernel mistake, applied to the fp64 reference, falls outside the bound
    in every input regime the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

import hotpath_ref as HR
from oracle import hmmc_oracle as O

D64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed), dtype=D64)


def assert_close(a, b, tol, what):
    err = float((a.detach() - b.detach()).abs().max())
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.1e}"


# (nseq, L, H, causal): both short templates and the long kernel, each with a partial last key tile; nseq H = 6 pairs
ATTN_CASES = [(3, 13, 2, False), (3, 50, 2, False), (3, 45, 2, True), (2, 77, 3, True), (2, 130, 3, False)]


# ============================================================================= the statements are pinned

@pytest.mark.parametrize("nseq,L,H,causal", ATTN_CASES)
def test_attention_is_sdpa_and_mha(nseq, L, H, causal):
    D = 64 * H
    qkv = randn(nseq * L, 3 * D, seed=L)
    out, lse = HR.attention(qkv, nseq, L, H, causal)
    q, k, v = HR.split_qkv(qkv, nseq, L, H)
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal)              # scale 1 / sqrt(64) = 1 / 8
    assert_close(out, HR.rows(ref), 1e-12, "out vs scaled_dot_product_attention")
    s = (q @ k.transpose(-1, -2)) / 8.0
    if causal:
        s = s + O.causal_mask(L).to(D64)
    assert_close(lse, torch.logsumexp(s, -1), 1e-12, "lse")
    # the oracle's nn.MultiheadAttention with these rows as its in-projection (softmax in fp32 there: 1e-6)
    x = randn(nseq, L, D, seed=L + 1) * 0.5
    in_w, in_b = randn(3 * D, D, seed=2) / D ** 0.5, randn(3 * D, seed=3) * 0.1
    rows = F.linear(x, in_w, in_b).reshape(nseq * L, 3 * D)
    mha = O.mha(x, in_w, in_b, torch.eye(D, dtype=D64), torch.zeros(D, dtype=D64), H, O.causal_mask(L) if causal else None)
    assert_close(HR.attention(rows, nseq, L, H, causal)[0].reshape(nseq, L, D), mha, 1e-6, "out vs the oracle's mha")


@pytest.mark.parametrize("nseq,L,H,causal", ATTN_CASES)
def test_attention_parts_is_autograd(nseq, L, H, causal):
    qkv, dout = randn(nseq * L, 192 * H, seed=L), randn(nseq * L, 64 * H, seed=L + 1)
    r = HR.attention_parts(qkv, dout, nseq, L, H, causal)
    out, lse = HR.attention(qkv, nseq, L, H, causal)
    assert_close(r["out"], out, 1e-13, "out")
    assert_close(r["lse"], lse, 1e-13, "lse")
    assert_close(r["dqkv"], HR.attention_bwd(qkv, dout, nseq, L, H, causal), 1e-12, "dqkv vs autograd")
    qr = qkv.clone().requires_grad_()
    sdpa = F.scaled_dot_product_attention(*HR.split_qkv(qr, nseq, L, H), is_causal=causal)
    HR.rows(sdpa).backward(dout)
    assert_close(r["dqkv"], qr.grad, 1e-12, "dqkv vs autograd of scaled_dot_product_attention")
    part = HR.dbias_partial(r["dqkv"], nseq, L)
    assert_close(part.sum(0), r["dqkv"].sum(0), 1e-11, "bias partials add up to the column sums")
    stat = torch.rand(nseq * L, 2, generator=gen(5), dtype=D64) + 0.5
    assert_close(HR.row_scaled(r["dqkv"], stat), torch.diag(stat[:, 0]) @ r["dqkv"], 1e-13, "row-scaled variant")


def test_quick_gelu_and_its_derivative():
    h = torch.linspace(-9, 9, 721, dtype=D64).requires_grad_()
    assert_close(HR.qgelu(h), O.quick_gelu(h), 0.0, "QuickGELU vs the oracle")
    O.quick_gelu(h).sum().backward()
    assert_close(HR.qgelu_grad(h.detach()), h.grad, 1e-14, "QuickGELU' vs autograd")


def test_gemm_epilogue_is_linear_and_autograd():
    M, N, K = 9, 16, 24
    a, w, bias, resid = randn(M, K, seed=1), randn(N, K, seed=2), randn(N, seed=3), randn(M, N, seed=4)
    acc = a @ w.t()
    B, R, Q, S, Dg, Mx = HR.EPI_BIAS, HR.EPI_RESID, HR.EPI_QGELU, HR.EPI_SAVE_DGELU, HR.EPI_DGELU, HR.EPI_MULAUX
    assert_close(HR.gemm_epilogue(acc, bias, None, None, B)[0], F.linear(a, w, bias), 1e-13, "BIAS")
    assert_close(HR.gemm_epilogue(acc, bias, resid, None, B | R)[0], resid + F.linear(a, w, bias), 1e-13, "BIAS | RESID")
    h = F.linear(a, w, bias).requires_grad_()
    g, aux = HR.gemm_epilogue(acc, bias, None, None, B | Q)
    assert_close(g, O.quick_gelu(h), 1e-13, "QGELU")
    assert_close(aux, h, 1e-13, "QGELU: aux = h")
    dy = randn(M, N, seed=5)                                  # the backward GEMM's accumulator: the gradient reaching QuickGELU
    O.quick_gelu(h).backward(dy)
    saved = HR.gemm_epilogue(acc, bias, None, None, B | Q | S)[1]
    assert_close(HR.gemm_epilogue(dy, None, None, h.detach(), Dg)[0], h.grad, 1e-13, "DGELU vs autograd")
    assert_close(HR.gemm_epilogue(dy, None, None, saved, Mx)[0], h.grad, 1e-13, "SAVE_DGELU then MULAUX vs autograd")
    # the rounded form on integer data is the kernel's arithmetic to the bit
    ai, wi = torch.randint(-2, 3, (M, K), generator=gen(6)).double(), torch.randint(-2, 3, (N, K), generator=gen(7)).double()
    bi = torch.randint(-3000, 3001, (N,), generator=gen(8)).half()
    ri = torch.randint(-3000, 3001, (M, N), generator=gen(9)).half()
    acci = ai @ wi.t()
    for fl in (B, B | R):
        emu = HR.emulate_gemm_epilogue(acci.float(), bi, ri, None, fl)[0]
        assert torch.equal(HR.gemm_epilogue(acci, bi.double(), ri.double(), None, fl, rounded=True)[0], emu.double()), fl


@pytest.mark.parametrize("D,eps", [(8, 1e-5), (768, 1e-5), (512, 1e-12)])
def test_layernorm_is_layer_norm(D, eps):
    x, gamma, beta, dy = randn(7, D, seed=D), 1 + 0.1 * randn(D, seed=1), 0.1 * randn(D, seed=2), randn(7, D, seed=3)
    y, mean, rstd = HR.layernorm(x, gamma, beta, eps)
    xr, gr, br = (t.clone().requires_grad_() for t in (x, gamma, beta))
    ref = F.layer_norm(xr, (D,), gr, br, eps)
    assert_close(y, ref, 1e-12, "y vs F.layer_norm")
    assert_close(y, O.layer_norm_tf(x, gamma, beta, eps), 1e-12, "y vs the oracle's TF-style LayerNorm")
    if eps == 1e-5:
        assert_close(y, O.layer_norm_clip(x, gamma, beta), 1e-4, "y vs the oracle's CLIP LayerNorm (fp32 there)")
    assert_close(mean, x.mean(-1), 1e-14, "mean")
    assert_close(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + eps), 1e-9 * float(rstd.max()), "rstd")
    ref.backward(dy)
    dres = randn(7, D, seed=4)
    dx, dg, db = HR.layernorm_bwd(x, gamma, beta, eps, dy, dres)
    assert_close(dx, xr.grad + dres, 1e-11, "dx + dres")
    assert_close(dg, gr.grad, 1e-11, "dgamma")
    assert_close(db, br.grad, 1e-12, "dbeta")


def test_pick_big_tile_restates_the_dispatch_rule():
    cus = 256
    for (M, N), big in {(16384, 768): True, (5000, 2312): True, (16384, 3072): True, (1000, 384): False, (130, 136): False,
                        (4096, 768): False, (2048, 2048): False, (22172, 768): True}.items():
        assert HR.pick_big_tile(M, N, cus) == big, (M, N)
    assert [HR.key_tiles(L) for L in (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256)] == \
        [2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 16, 16]


# ============================================================================= the bounds are not too tight

def worst(ratios, got, ref, bound, name):
    ratios[name] = max(ratios.get(name, 0.0), HR.within_ratio(got, ref, bound))


@pytest.mark.parametrize("regime", HR.ATTN_REGIMES)
def test_emulation_inside_bounds_attention(regime):
    ratios = {}
    for nseq, L, H, causal in ATTN_CASES + [(1, 1, 1, False), (3, 2, 1, True), (1, 16, 1, False), (1, 64, 2, True), (1, 197, 2, False),
                                            (1, 256, 1, True)]:
        qkv, dout = HR.attention_inputs(regime, nseq, L, H, causal)
        stat = torch.rand(nseq * L, 2, generator=gen(L)) + 0.5
        emu = HR.emulate_attention(qkv, dout, nseq, L, H, causal, stat)
        q64, d64 = qkv.double(), dout.double()
        ref = HR.attention_parts(q64, d64, nseq, L, H, causal)
        b = HR.attention_bounds(q64, d64, nseq, L, H, causal, stat.double())
        for name in ("out", "lse", "dqkv"):
            worst(ratios, emu[name], ref[name], b[name], name)
        worst(ratios, emu["dbias"], HR.dbias_partial(ref["dqkv"], nseq, L), b["dbias"], "dbias")
        worst(ratios, emu["scaled"], HR.row_scaled(ref["dqkv"], stat.double()), b["scaled"], "scaled")
    print(f"hotpath-emulation attention {regime}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, f"attention, {regime}: worst err / (SLACK bound) per output {ratios}"


GEMM_SETS = {"bias": HR.EPI_BIAS, "bias_resid": HR.EPI_BIAS | HR.EPI_RESID, "bias_qgelu": HR.EPI_BIAS | HR.EPI_QGELU,
             "bias_qgelu_save": HR.EPI_BIAS | HR.EPI_QGELU | HR.EPI_SAVE_DGELU, "dgelu": HR.EPI_DGELU, "mulaux": HR.EPI_MULAUX}


def gemm_random(M, N, K, seed=0):
    """the GPU tests' random regime: acc ~ N(0, 1), bias and the DGELU operand spread over [-8, 8]"""
    g = gen(seed + M + N + K)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias = (torch.rand(N, generator=g) * 16 - 8).half()
    resid = torch.randn(M, N, generator=g).half()
    spread = (torch.rand(M, N, generator=g) * 16 - 8).half()
    return a, w, bias, resid, spread


def test_emulation_inside_bounds_gemm():
    ratios = {}
    for M, N, K in [(130, 136, 64), (70, 72, 768)]:
        a, w, bias, resid, spread = gemm_random(M, N, K)
        acc32 = a.float() @ w.float().t()
        acc = a.double() @ w.double().t()
        eacc = HR.gemm_acc_bound(a.double().abs() @ w.double().abs().t(), K)
        for name, fl in GEMM_SETS.items():
            aux_in = spread if fl & HR.EPI_DGELU else resid
            out, aux = HR.emulate_gemm_epilogue(acc32, bias, resid, aux_in, fl)
            ref, ref_aux = HR.gemm_epilogue(acc, bias.double(), resid.double(), aux_in.double(), fl)
            b, b_aux = HR.gemm_epilogue_bounds(acc, eacc, bias.double(), resid.double(), aux_in.double(), fl)
            worst(ratios, out, ref, b, name)
            if ref_aux is not None:
                worst(ratios, aux, ref_aux, b_aux, name + ".aux")
        c = HR.emulate_gemm_epilogue(acc32, bias, None, None, HR.EPI_BIAS)[0]
        part = torch.stack([c[r:r + 64].float().sum(0) for r in range(0, M, 64)])
        worst(ratios, part, HR.colsum_blocks(c.double(), 64), HR.colsum_bound(c.double(), 64), "colsum")
    print("hotpath-emulation gemm: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, f"GEMM epilogues: worst err / (SLACK bound) per output {ratios}"


LN_CASES = [(torch.float16, D, 1e-5) for D in (8, 64, 128, 512, 768, 1024)] + [(torch.float32, D, 1e-12) for D in (4, 512, 1024)]


@pytest.mark.parametrize("regime", HR.LN_REGIMES)
def test_emulation_inside_bounds_layernorm(regime):
    ratios = {}
    for dtype, D, eps in LN_CASES:
        for nrows in (1, 3, 37):
            x, gamma, beta, dy, dres = HR.layernorm_inputs(regime, nrows, D, dtype)
            emu = HR.emulate_layernorm(x, gamma, beta, eps, dy, dres)
            x64, g64, b64, dy64, dr64 = (t.double() for t in (x, gamma, beta, dy, dres))
            y, mean, rstd = HR.layernorm(x64, g64, b64, eps)
            dx, dg, db = HR.layernorm_bwd(x64, g64, b64, eps, dy64, dr64)
            b = HR.layernorm_bounds(x64, g64, b64, eps, dy64, dr64, dtype == torch.float16)
            tag = "f16." if dtype == torch.float16 else "f32."
            for name, ref in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dg), ("dbeta", db), ("dxsum", dx.sum(0))):
                worst(ratios, emu[name], ref, b[name], tag + name)
    print(f"hotpath-emulation layernorm {regime}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, f"LayerNorm, {regime}: worst err / (SLACK bound) per output {ratios}"


# ============================================================================= the bounds are not too loose

SLIP_CASES = [(3, 50, 2, False), (3, 45, 2, True), (2, 77, 3, True), (2, 130, 3, False)]


@pytest.mark.parametrize("regime", HR.ATTN_REGIMES)
@pytest.mark.parametrize("slip", HR.ATTN_SLIPS)
def test_slip_attention(slip, regime):
    """pad_key: one padded key unmasked;  mask_last: key L - 1 masked;  causal_edge: `key < qi`;  scale_tile: the 1/8 missing on one
    key tile;  stale_pair: a pair holding the results of the pair `shift` before it;  delta_neighbour: delta of the next query;
    lse_nomax: lse without the max added back - each outside the bound of out, lse or dqkv, on both kernels, in every regime."""
    for nseq, L, H, causal in SLIP_CASES:
        if slip == "causal_edge" and not causal:
            continue
        qkv, dout = (t.double() for t in HR.attention_inputs(regime, nseq, L, H, causal))
        ref = HR.attention_parts(qkv, dout, nseq, L, H, causal)
        bad = HR.attention_parts(qkv, dout, nseq, L, H, causal, slip=slip, shift=2)
        b = HR.attention_bounds(qkv, dout, nseq, L, H, causal)
        hit = [name for name in ("out", "lse", "dqkv") if HR.detects(ref[name], bad[name], b[name])]
        assert hit, f"{slip} hides inside the bounds at nseq {nseq} L {L} H {H} causal {causal}, {regime} inputs"
        if slip == "delta_neighbour":
            assert hit == ["dqkv"]
        if slip == "lse_nomax":
            assert hit == ["lse"]


def test_slip_gemm_bias_of_the_next_column():
    M, N, K = 130, 136, 64
    a, w, bias, resid, spread = gemm_random(M, N, K)
    acc = a.double() @ w.double().t()
    eacc = HR.gemm_acc_bound(a.double().abs() @ w.double().abs().t(), K)
    for name in ("bias", "bias_qgelu", "bias_qgelu_save"):
        fl = GEMM_SETS[name]
        ref, ref_aux = HR.gemm_epilogue(acc, bias.double(), None, None, fl)
        bad, bad_aux = HR.gemm_epilogue(acc, bias.double().roll(-1), None, None, fl)
        b, b_aux = HR.gemm_epilogue_bounds(acc, eacc, bias.double(), None, None, fl)
        assert HR.detects(ref, bad, b), name
        if ref_aux is not None:
            assert HR.detects(ref_aux, bad_aux, b_aux), name + " (aux)"
    # the exact regime of BIAS and BIAS | RESID: integer data, compared with torch.equal
    ai, wi = torch.randint(-2, 3, (M, K), generator=gen(1)).double(), torch.randint(-2, 3, (N, K), generator=gen(2)).double()
    bi = torch.randint(-3000, 3001, (N,), generator=gen(3)).half().double()
    ri = torch.randint(-3000, 3001, (M, N), generator=gen(4)).half().double()
    for fl in (HR.EPI_BIAS, HR.EPI_BIAS | HR.EPI_RESID):
        ref = HR.gemm_epilogue(ai @ wi.t(), bi, ri, None, fl, rounded=True)[0]
        assert not torch.equal(ref, HR.gemm_epilogue(ai @ wi.t(), bi.roll(-1), ri, None, fl, rounded=True)[0]), fl


def test_slip_gemm_resid_added_before_the_first_rounding():
    """out = fp16(resid + acc + bias) instead of fp16(resid + fp16(acc + bias)): BIAS | RESID runs on integer data whose h passes
    2048, where fp16 holds even numbers only - the two differ and the GPU test compares with torch.equal."""
    M, N, K = 130, 136, 64
    ai, wi = torch.randint(-2, 3, (M, K), generator=gen(1)).double(), torch.randint(-2, 3, (N, K), generator=gen(2)).double()
    bi = torch.randint(-3000, 3001, (N,), generator=gen(3)).half().double()
    ri = torch.randint(-3000, 3001, (M, N), generator=gen(4)).half().double()
    acc = ai @ wi.t()
    ref = HR.gemm_epilogue(acc, bi, ri, None, HR.EPI_BIAS | HR.EPI_RESID, rounded=True)[0]
    once = HR.h16(ri + acc + bi)
    assert not torch.equal(ref, once)
    assert float((acc + bi).abs().max()) > 2048 and float((ref - once).abs().max()) >= 1.0


def test_slip_qgelu_grad_with_1702_applied_once():
    M, N, K = 130, 136, 64
    a, w, bias, resid, spread = gemm_random(M, N, K)
    acc = a.double() @ w.double().t()
    eacc = HR.gemm_acc_bound(a.double().abs() @ w.double().abs().t(), K)
    fl = GEMM_SETS["bias_qgelu_save"]
    _, ref_aux = HR.gemm_epilogue(acc, bias.double(), None, None, fl)
    _, b_aux = HR.gemm_epilogue_bounds(acc, eacc, bias.double(), None, None, fl)
    assert HR.detects(ref_aux, HR.qgelu_grad(acc + bias.double(), outer=1.0), b_aux), "SAVE_DGELU"
    x = spread.double()
    ref = HR.gemm_epilogue(acc, None, None, x, HR.EPI_DGELU)[0]
    b = HR.gemm_epilogue_bounds(acc, eacc, None, None, x, HR.EPI_DGELU)[0]
    assert HR.detects(ref, acc * HR.qgelu_grad(x, outer=1.0), b), "DGELU"


@pytest.mark.parametrize("M,block", [(1000, 64), (130, 64), (5000, 128)])
def test_slip_colsum_without_the_last_ragged_row_block(M, block):
    c = torch.randn(M, 16, generator=gen(M)).half().double()
    ref, b = HR.colsum_blocks(c, block), HR.colsum_bound(c, block)
    assert ref.shape[0] == (M + block - 1) // block
    dropped = ref.clone()
    dropped[-1] = 0.0
    assert HR.detects(ref, dropped, b), "per partial row"
    assert HR.detects(ref.sum(0), dropped.sum(0), b.sum(0)), "in the sum of the partial rows"
    full = ref.clone()                                        # the ragged block summed over a whole block of rows (stale rows past M)
    full[-1] = ref[-1] + c[:block - M % block].sum(0)
    assert HR.detects(ref, full, b), "rows past M counted"


@pytest.mark.parametrize("regime", HR.LN_REGIMES)
@pytest.mark.parametrize("dtype,D,eps", [(torch.float16, 64, 1e-5), (torch.float16, 768, 1e-5), (torch.float16, 1024, 1e-5),
                                         (torch.float32, 512, 1e-12)])
def test_slip_layernorm(dtype, D, eps, regime):
    """the unbiased variance instead of the biased one; the mean of the neighbouring row"""
    x, gamma, beta, dy, dres = (t.double() for t in HR.layernorm_inputs(regime, 3, D, dtype))
    ref = HR.layernorm(x, gamma, beta, eps)
    b = HR.layernorm_bounds(x, gamma, beta, eps, dy, dres, dtype == torch.float16)
    names = ("y", "mean", "rstd")
    unb = HR.layernorm(x, gamma, beta, eps, unbiased=True)
    assert any(HR.detects(r, s, b[n]) for r, s, n in zip(ref, unb, names)), "unbiased variance"
    nb = HR.layernorm(x, gamma, beta, eps, mean_shift=1)
    assert HR.detects(ref[0], nb[0], b["y"]) and HR.detects(ref[1], nb[1], b["mean"]), "mean of the neighbouring row"


# ============================================================================= weight gradients: split-K slabs + reduce

def split_counts(T):
    """split counts to emulate a shape with: none, two, and the most either host policy grants (four K-tiles per split)"""
    nkt = (T + HR.BKT - 1) // HR.BKT
    return sorted({1, min(2, nkt), max(1, nkt // 4)})


def wgrad_case(regime, T, dims, seed=0):
    dys, xs = HR.wgrad_inputs(regime, T, dims, seed)
    return dys, xs, [d.double() for d in dys], [x.double() for x in xs]


def test_wgrad_is_matmul_and_autograd():
    T, N, K = 70, 24, 40
    dy, x, w = randn(T, N, seed=1), randn(T, K, seed=2), randn(N, K, seed=3).requires_grad_()
    assert_close(HR.wgrad(dy, x), torch.matmul(dy.transpose(0, 1), x), 0.0, "wgrad vs torch.matmul")
    F.linear(x, w).backward(dy)
    assert_close(HR.wgrad(dy, x), w.grad, 1e-13, "wgrad vs autograd of F.linear")
    a, b, bt = randn(N, T, seed=4), randn(K, T, seed=5), randn(T, K, seed=6)
    assert_close(HR.gemm_kk(a, b), torch.matmul(a, b.transpose(0, 1)), 0.0, "kk")
    assert_close(HR.gemm_km(a, bt), torch.matmul(a, bt), 0.0, "km")
    assert_close(HR.wgrad(*HR.as_wgrad("kk", a, b)), HR.gemm_kk(a, b), 1e-13, "kk as a weight gradient")
    assert_close(HR.wgrad(*HR.as_wgrad("km", a, bt)), HR.gemm_km(a, bt), 1e-13, "km as a weight gradient")
    # the slabs add up, whatever the split; a split count is turned into (nkt, ktps, splitk) as the host does
    for ktps in (1, 2):
        assert_close(HR.wgrad_partials(dy, x, ktps).sum(0), HR.wgrad(dy, x), 1e-12, "partials")
    assert HR.split_plan(2120, 8) == (34, 5, 7) and HR.split_plan(2120, 7) == (34, 5, 7)       # a shorter last split: 34 - 30 = 4
    assert HR.split_plan(1000, 4) == (16, 4, 4) and HR.split_plan(8, 0) == (1, 1, 1) and HR.split_plan(100, 1) == (2, 2, 1)
    assert HR.split_plan(520, 2) == (9, 5, 2) and HR.split_plan(6152, 16) == (97, 7, 14)


WGRAD_SHAPES = [(K, [(M, N)]) for M, N, K in HR.WGRAD_MM_CASES] + [(K, [(M, N)]) for _, M, N, K in HR.WGRAD_KX_CASES] + \
    [(T, dims) for dims, T, _ in HR.WGRAD_GROUP_CASES.values()]


@pytest.mark.parametrize("regime", HR.WGRAD_REGIMES)
@pytest.mark.parametrize("T,dims", WGRAD_SHAPES, ids=[f"T{T}-{len(d)}x{d[0][0]}x{d[0][1]}" for T, d in WGRAD_SHAPES])
def test_emulation_inside_bounds_wgrad(T, dims, regime):
    """the slab path's arithmetic (fp32 per split in K-tile order, the ordered reduce, one fp16 rounding or none) lies inside the
    bound of its split, and the unsplit emulation inside the c = T bound, at every shape the GPU tests run"""
    ratios = {}
    seen = set()
    for (n, k), dy, x, d64, x64 in zip(dims, *wgrad_case(regime, T, dims)):
        if (n, k) in seen:
            continue
        seen.add((n, k))
        ref, ab = HR.wgrad(d64, x64), HR.wgrad(d64.abs(), x64.abs())
        assert float(ref.abs().max()) < 65504
        for s in split_counts(T):
            nkt, ktps, splitk = HR.split_plan(T, s)
            for half in (True, False):
                emu = HR.emulate_splitk(dy, x, ktps, half)
                worst(ratios, emu, ref, HR.wgrad_bound(ref, ab, T, ktps, splitk, half), "f16" if half else "f32")
                if splitk == 1:
                    worst(ratios, emu, ref, HR.wgrad_bound(ref, ab, T, half=half), ("f16" if half else "f32") + ".cT")
    print(f"hotpath-emulation wgrad {regime} T {T}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, f"weight gradient, {regime}: worst err / (SLACK bound) per output {ratios}"


def test_emulation_is_exact_on_integers():
    """the exact regime: the emulated fp32 path gives the integers themselves, past 2048 (where fp16 no longer holds them all)"""
    M, N, K = HR.WGRAD_MM_CASES[4]
    dys, xs, d64, x64 = wgrad_case("exact", K, [(M, N)])
    ref = HR.wgrad(d64[0], x64[0])
    assert 2048 < float(ref.max()) < 65504
    _, ktps, _ = HR.split_plan(K, 8)
    assert torch.equal(HR.emulate_splitk(dys[0], xs[0], ktps, half=False).double(), ref)
    assert torch.equal(HR.emulate_splitk(dys[0], xs[0], ktps, half=True), ref.half())
    assert not torch.equal(ref.half().double(), ref)


SLIP_MM = HR.WGRAD_MM_CASES[2]                   # 136 x 264 x 1000: the smallest single launch with a split (4 of 4 K-tiles, 24 tail rows)
SLIP_GROUP = HR.WGRAD_GROUP_CASES["two_f32"]     # the smallest grouped launch with two problems (520 tokens: splits of 5 + 4 K-tiles)


@pytest.mark.parametrize("slip", HR.WGRAD_SLIPS)
def test_slip_wgrad(slip):
    """every slip of hotpath_ref.wgrad_slipped falls outside the bound in at least one data regime, at the smallest split shape of
    the single launch (fp16 result) and of the grouped launch (fp32 result).  The slips that only round differently - slab_f16,
    reduce_f16 - stay inside the bound of an fp16 RESULT by construction (they add roundings of the size the result's own rounding
    has): they are caught by the fp32 result's bound on same-sign data and, by inequality, in the exact regime
    (test_slip_wgrad_exact_integers)."""
    rounding_only = slip in ("slab_f16", "reduce_f16")
    (M, N, K), (dims, T, _) = SLIP_MM, SLIP_GROUP
    for what, Tn, shape, s, half, tile in (("single", K, (M, N), 4, True, 128), ("grouped", T, dims[1], 2, False, 256)):
        _, ktps, splitk = HR.split_plan(Tn, s)
        assert splitk > 1
        hit = {}
        for regime in HR.WGRAD_REGIMES:
            _, _, d64, x64 = wgrad_case(regime, Tn, [shape])
            ref, ab = HR.wgrad(d64[0], x64[0]), HR.wgrad(d64[0].abs(), x64[0].abs())
            bad = HR.wgrad_slipped(d64[0], x64[0], ktps, slip, tile)
            hit[regime] = HR.detects(ref, bad, HR.wgrad_bound(ref, ab, Tn, ktps, splitk, half))
        if rounding_only and half:
            continue
        assert any(hit.values()), f"{slip} hides inside the {what} bound in both regimes: {hit}"
        if not rounding_only:
            assert hit["same"], f"{slip} hides inside the {what} bound on same-sign data"


def test_slip_wgrad_group_problem_swapped():
    dims, T, _ = SLIP_GROUP
    _, ktps, splitk = HR.split_plan(T, 2)
    for regime in HR.WGRAD_REGIMES:
        _, _, d64, x64 = wgrad_case(regime, T, dims)
        bad = HR.wgrad_group_swapped(d64, x64, ktps)
        ref0 = HR.wgrad(d64[0], x64[0])
        assert torch.equal(bad[0], HR.wgrad_partials(d64[0], x64[0], ktps).sum(0)) and float((bad[0] - ref0).abs().max()) < 1e-9
        ref, ab = HR.wgrad(d64[1], x64[1]), HR.wgrad(d64[1].abs(), x64[1].abs())
        for half in (True, False):
            assert HR.detects(ref, bad[1], HR.wgrad_bound(ref, ab, T, ktps, splitk, half)), (regime, half)


@pytest.mark.parametrize("slip", ["slab_f16", "reduce_f16"])
def test_slip_wgrad_exact_integers(slip):
    """the exact regime's integers over 1000 and more rows: every split's partial passes 2048, an fp16 slab or running sum loses
    low bits, and the result differs from the exact one - in the fp32 output, and in the fp16 output after its own rounding.  At
    every shape the GPU tests run this regime on, with the split each gets on 256 CUs."""
    for (M, N, K), s in ((SLIP_MM, 4), (HR.WGRAD_MM_CASES[3], 4), (HR.WGRAD_MM_CASES[4], 8), (HR.WGRAD_MM_CASES[5], 16), ((768, 256, 2120), 7)):
        _, ktps, splitk = HR.split_plan(K, s)
        _, _, d64, x64 = wgrad_case("exact", K, [(M, N)])
        ref = HR.wgrad(d64[0], x64[0])
        bad = HR.wgrad_slipped(d64[0], x64[0], ktps, slip)
        assert float(HR.wgrad_partials(d64[0], x64[0], ktps)[:-1].median()) > 2048 and float(ref.max()) < 65504
        assert not torch.equal(bad, ref), "fp32 result"
        assert not torch.equal(bad.half(), ref.half()), "fp16 result"
