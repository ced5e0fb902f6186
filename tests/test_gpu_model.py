"""GPU parity tests of the drop-in model/optimizer API (through the C-ABI) against
 (a) golden vectors produced by the reference itself (tests/golden/*.npz) and
 (b) the CPU oracle on the same seeded inputs.
Tolerances: fp32 heads — logits within 1e-3 (north_star), ranks identical; fp16 towers — the
as-written regime's own envelope (reference-as-written vs reference-fp32 differ by ~2e-2 on x100 logits,
SURVEY.md section 7), features compared at 3e-2 abs+rel like the oracle-vs-golden as-written test."""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import golden  # noqa: E402
from hmmc_amd import ops, synth  # noqa: E402
from hmmc_amd import functional as Fn  # noqa: E402
from oracle import hmmc_oracle as O  # noqa: E402

DEV = "cuda"


def task_config(**kw):
    d = dict(local_rank=0, rank=0, use_temp=True, language="english", top_frames=2, max_frames=4, n_display=100000,
             logdir=None, use_frame_fea=True, dataset="msrvtt", contrast_momentum=0.99, contrast_temperature=0.07,
             contrast_num_negative=16, pretrained_text=None, lr=1e-4, text_lr=3e-5, coef_lr=1e-3, weight_decay=0.2,
             warmup_proportion=0.1)
    d.update(kw)
    return Namespace(**d)


def close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    lim = atol + rtol * np.abs(b.astype(np.float64))
    assert (err <= lim).all(), f"{what}: max abs err {err.max():.3e} (atol {atol}, rtol {rtol}); worst ratio {(err/lim).max():.2f}"


# ----------------------------------------------------------------------------- fp32 kernels

def relerr(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def test_gemm_f32_all_orientations():
    g = torch.Generator().manual_seed(0)
    for (M, N, K) in [(64, 64, 16), (100, 36, 52), (50, 40, 203), (384, 512, 2048), (256, 3328, 512), (3328, 512, 256)]:
        a = torch.randn(M, K, generator=g).to(DEV)
        b = torch.randn(N, K, generator=g).to(DEV)
        ref = a.double() @ b.double().t()
        tol = 1e-4 * max(1.0, K / 512)                                           # fp32 accumulation error grows with K
        c = ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K))                          # x W^T
        close(c, ref, tol, 1e-5, "kk")
        bt = b.t().contiguous()                                                   # [K, N]
        c = ops.gemm_f32(a, bt, M, N, K, (K, 1), (N, 1), alpha=2.0)              # dy W
        close(c, 2 * ref, 2 * tol, 1e-5, "kn")
        at = a.t().contiguous()                                                   # [K, M]
        c = ops.gemm_f32(at, bt, M, N, K, (1, M), (N, 1))                        # dy^T x
        close(c, ref, tol, 1e-5, "tn")
    x, w, bias, res = torch.randn(77, 512).to(DEV), torch.randn(2048, 512).to(DEV) * 0.05, torch.randn(2048).to(DEV), None
    gq, h = ops.linear_f32(x, w, bias=bias, epilogue=ops.EPI_QGELU, want_aux=True)
    href = x @ w.t() + bias
    close(h, href, 1e-4, 1e-5, "h")
    close(gq, href * torch.sigmoid(1.702 * href), 1e-4, 1e-5, "qgelu")


@pytest.mark.parametrize("M,N,K", [(3072, 512, 2048), (1536, 512, 2048), (2048, 512, 1536), (700, 512, 4096), (1000, 500, 2052),
                                   (333, 260, 3001)])
def test_gemm_f32_long_k_single_round_exact_integers(M, N, K):
    """Long-K shapes of the fp32 path.  By hmmc_gemm_f32_plan on a 256-CU part the 2nd to 5th take the wave-split-K kernel (tile
    heights 48 / 64 / 32 / 32), the first the LDS-DMA kernel's 32 x 64 tiles and the last (K % 4 != 0) the 16 x 32 kernel's
    scalar-load variant; tests/test_gpu_gemm_f32.py asserts the plan of every instantiation it runs, the 96-row tiles included.
    In the three operand orientations of the path
    (x W^T, dy W, dy^T x; reference modules/module_cross.py:114-149).  Integer-valued operands: every product and partial
    sum is exact in fp32, so the result must EQUAL the fp64 product whatever the order of the four waves' partial tiles."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float().to(DEV)
    b = torch.randint(-3, 4, (N, K), generator=g).float().to(DEV)
    bias = torch.randint(-5, 6, (N,), generator=g).float().to(DEV)
    ref = (a.double() @ b.double().t()).float()
    bt, at = b.t().contiguous(), a.t().contiguous()
    c1 = ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K))
    c2 = ops.gemm_f32(a, bt, M, N, K, (K, 1), (N, 1), alpha=2.0, bias=bias)
    c3 = ops.gemm_f32(at, bt, M, N, K, (1, M), (N, 1))
    assert torch.equal(c1, ref), "x W^T"
    assert torch.equal(c2, 2 * ref + bias), "dy W (+ alpha, bias)"
    assert torch.equal(c3, ref), "dy^T x"
    x = torch.randn(M, K, generator=g).to(DEV)
    w = torch.randn(N, K, generator=g).to(DEV)
    y = ops.gemm_f32(x, w, M, N, K, (K, 1), (1, K))
    close(y, x.double() @ w.double().t(), 1e-4 * K / 512, 1e-5, "random operands")
    assert torch.equal(y, ops.gemm_f32(x, w, M, N, K, (K, 1), (1, K))), "two launches, same bits"


@pytest.mark.parametrize("M,N,K", [(3072, 1536, 512), (3072, 2048, 512), (3000, 1540, 512), (2048, 4100, 544), (1540, 3000, 1024),
                                   (2048, 512, 3072)])
def test_gemm_f32_many_tiles_exact_integers(M, N, K):
    """Shapes the fp32 dispatcher gives to the LDS-DMA kernel on a 256-CU part (16-byte aligned rows, K % 32 == 0, at least two
    of its 64x64 or 32x64 tiles per CU: the temporal transformer at 3 072 tokens, the MoCo projector and logits, the MLM head;
    reference modules/module_cross.py:114-149, modules/modeling.py:286-313,788-807), with ragged M / N edges, in the orientations
    of the path and with every epilogue.  Integer-valued operands: every product and partial sum is exact in fp32, so the result
    must EQUAL the fp64 product.  (The kernel forced on 150 random shapes per tile size: no mismatch.)"""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float().to(DEV)
    b = torch.randint(-3, 4, (N, K), generator=g).float().to(DEV)
    bias = torch.randint(-5, 6, (N,), generator=g).float().to(DEV)
    res = torch.randint(-5, 6, (M, N), generator=g).float().to(DEV)
    ref = (a.double() @ b.double().t()).float()
    bt, at = b.t().contiguous(), a.t().contiguous()
    assert torch.equal(ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K)), ref), "x W^T"
    assert torch.equal(ops.gemm_f32(a, bt, M, N, K, (K, 1), (N, 1), alpha=2.0, bias=bias), 2 * ref + bias), "dy W (+ alpha, bias)"
    assert torch.equal(ops.gemm_f32(at, bt, M, N, K, (1, M), (N, 1), resid=res), ref + res), "dy^T x (+ residual)"
    assert torch.equal(ops.gemm_f32(at, b, M, N, K, (1, M), (1, K)), ref), "row-contiguous A, k-contiguous B"
    assert torch.equal(ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K), bias=bias, epilogue=ops.EPI_RELU), (ref + bias).clamp_min(0)), "ReLU"
    y, h = ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K), bias=bias, epilogue=ops.EPI_QGELU, want_aux=True)
    assert torch.equal(h, ref + bias), "saved pre-activation"
    close(y, h * torch.sigmoid(1.702 * h), 1e-5, 1e-5, "QuickGELU")
    dy = torch.randint(-3, 4, (M, N), generator=g).float().to(DEV)
    dx = ops.gemm_f32(a, b, M, N, K, (K, 1), (1, K), aux_in=dy, epilogue=ops.EPI_DGELU)
    sg = torch.sigmoid(1.702 * dy)
    close(dx, ref * (sg * (1 + 1.702 * dy * (1 - sg))), 1e-5, 1e-4, "x QuickGELU'(aux)")
    x = torch.randn(M, K, generator=g).to(DEV)
    w = torch.randn(N, K, generator=g).to(DEV)
    yr = ops.gemm_f32(x, w, M, N, K, (K, 1), (1, K))
    close(yr, x.double() @ w.double().t(), 1e-4 * K / 512, 1e-5, "random operands")
    assert torch.equal(yr, ops.gemm_f32(x, w, M, N, K, (K, 1), (1, K))), "two launches, same bits"


@pytest.mark.parametrize("tag", ["head_ft_small", "head_ft_c2"])
def test_finetune_head_vs_reference_golden(tag):
    g = golden(tag)
    B, Fr = int(g["B"]), int(g["F"])
    q = synth.normal(f"{tag}.q", (B, 512)).to(DEV).requires_grad_()
    v = synth.normal(f"{tag}.v", (B, 512)).to(DEV).requires_grad_()
    u = synth.normal(f"{tag}.u", (B, Fr, 512)).to(DEV).requires_grad_()
    loss = Fn.FinetuneHeadFn.apply(q, v, u, 0.85, 0.15, 100.0)
    loss.backward()
    close(loss, g["loss"], 2e-5, what="loss")
    qn, _ = ops.l2norm_fwd(q.detach())
    vn, _ = ops.l2norm_fwd(v.detach())
    S = ops.gemm_f32(qn, vn, B, B, 512, (512, 1), (1, 512), alpha=100.0)
    if "S_video" in g:
        close(S, g["S_video"], 1e-3, what="S_video (1e-3 logits)")
        close(q.grad, g["dQ"], 2e-6, 1e-4, "dQ")
        close(v.grad, g["dV"], 2e-6, 1e-4, "dV")
        close(u.grad, g["dU"], 2e-6, 1e-4, "dU")
    else:
        close(S[:8], g["S_video_rows"], 1e-3, what="S_video rows")
        close(q.grad[:8], g["dQ_rows"], 2e-6, 1e-4, "dQ rows")
        close(u.grad[:4], g["dU_rows"], 2e-6, 1e-4, "dU rows")
        close(q.grad.norm(), g["dQ_norm"], 1e-6, 1e-4, "dQ norm")
        close(v.grad.norm(), g["dV_norm"], 1e-6, 1e-4, "dV norm")


def test_eval_scorer_ranks_identical():
    from hmmc_amd.modeling import BirdModel
    g = golden("head_eval")
    q = synth.normal("head_eval.q", (48, 512))
    v = synth.normal("head_eval.v", (48, 512))
    u = synth.normal("head_eval.u", (48, 12, 512))
    q = (q + 0.7 * v).to(DEV)
    v, u = v.to(DEV), u.to(DEV)
    model = BirdModel.from_pretrained("cross-base", state_dict=synth.finetune_state(synth.TINY), task_config=task_config())
    with torch.no_grad():
        sf = model.loose_similarity(q, u)
        close(sf, g["S_frame"], 1e-3, what="S_frame")
        for k in (1, 2, 3, 12):
            sv, fk = model.eval_scores(q, v, u, top_frames=k)
            close(sv, g["S_video"], 1e-3, what="S_video")
            close(fk, g[f"topk{k}"], 1e-3, what=f"topk{k}")
            ref_rank = np.argsort(-(g["S_video"] + g[f"topk{k}"]), axis=1)
            got_rank = np.argsort(-(sv + fk).cpu().numpy(), axis=1)
            assert np.array_equal(got_rank, ref_rank), f"retrieval ranks differ at k={k}"
            m = O.compute_metrics((sv + fk).cpu().numpy())
            close([m["R1"], m["R5"], m["R10"], m["MR"], m["MeanR"]], g[f"metrics{k}"], 1e-9, what="metrics")
            from hmmc_amd import metrics as M      # rank metrics with the ranking on the device
            md, mvt = M.compute_metrics_t2v_v2t(sv + fk)
            close([md["R1"], md["R5"], md["R10"], md["MR"], md["MeanR"]], g[f"metrics{k}"], 1e-9, what="device metrics")
            assert np.array_equal(M.ranks(sv + fk), m["ranks"])
            mo = O.compute_metrics((sv + fk).cpu().numpy().T)
            assert np.array_equal(M.ranks(sv + fk, transposed=True), mo["ranks"]) and mvt["R1"] == mo["R1"]


@pytest.mark.parametrize("width,heads,L,nseq,layers,fold", [(128, 2, 10, 37, 3, False), (768, 12, 50, 96, 2, False), (768, 12, 50, 96, 3, True),
                                                            (768, 12, 197, 16, 2, True), (768, 12, 50, 83, 2, False),
                                                            (768, 12, 50, 83, 2, True)])
def test_tower_lead_only_equals_full_tower(width, heads, L, nseq, layers, fold, monkeypatch):
    """hmmc_tower_fwd/bwd with lead_only run the last block's per-token half - and, for sequences of at most 64 tokens, its
    Q projection and attention (round 4) - on the class-token rows alone: those rows of the output must EQUAL the full
    computation's, the input gradient and every parameter gradient agree with it (no gradient reaches the skipped rows; weight
    gradients differ only in the order of their fp32 partial sums).  fold: the training path of the frame tower
    (hmmc_tower_fwd_fused(keep_acts) + hmmc_tower_bwd_fold with the last block on the unfolded kernels); 197 tokens: the
    long-sequence attention, which keeps the all-query path; 83 x 50 = 4 150 tokens: above 4 096 rows, where the LayerNorm
    backward's partial row count for the tokens and for the nseq class rows follow different formulas."""
    from hmmc_amd import module_clip
    import hmmc_amd.functional as Fn
    torch.manual_seed(3)
    tw = module_clip.Transformer(width, layers, heads)
    if fold:
        monkeypatch.setattr(Fn, "_FOLD_LN_TRAIN", "vit")
        tw.fold_ln = True
    for prm in tw.parameters():
        torch.nn.init.normal_(prm, std=0.05 if prm.dim() > 1 else 0.1)
    for blk in tw.resblocks:
        blk.ln_1.weight.data.add_(1.0)
        blk.ln_2.weight.data.add_(1.0)
    module_clip.convert_weights(tw)
    tw = tw.to(DEV)
    x0 = (torch.randn(nseq * L, width) * 0.5).half().to(DEV)
    wsel = torch.randn(nseq, width).to(DEV)
    res = []
    for lead in (False, True):
        for prm in tw.parameters():
            prm.grad = None
        x = x0.clone().requires_grad_()
        y = tw(x, nseq, L, lead_only=lead)
        cls = y.view(nseq, L, width)[:, 0, :]
        (cls.float() * wsel).sum().backward()
        res.append((cls.detach().clone(), x.grad.clone(), {n: q.grad.clone() for n, q in tw.named_parameters()}))
    (c0, dx0, g0), (c1, dx1, g1) = res
    assert torch.equal(c0, c1), f"class-token rows differ: {(c0.float() - c1.float()).abs().max()}"
    assert relerr(dx1, dx0) < 1e-3, relerr(dx1, dx0)
    for n in g0:
        assert relerr(g1[n], g0[n]) < 2e-3, (n, relerr(g1[n], g0[n]))


def test_temporal_fn_vs_oracle():
    dims = synth.TINY
    sd = synth.finetune_state(dims)
    b, F, E = 5, 4, 512
    u = synth.normal("temporal.u", (b, F, E))
    from hmmc_amd.modeling import BirdModel
    model = BirdModel.from_pretrained("cross-base", state_dict=sd, task_config=task_config()).to(DEV)
    ve = model.visual_encoder
    ug = u.to(DEV).requires_grad_()
    out = Fn.TemporalFn.apply(ug, 8, ve.frame_position_embeddings.weight, *ve.temporal_transformer.flat_params())
    w = synth.normal("temporal.w", (b, E)).to(DEV)
    (out * w).sum().backward()
    # oracle
    sdo = {k: t.clone().requires_grad_(t.is_floating_point()) for k, t in sd.items()}
    uo = u.clone().requires_grad_()
    h = uo + sdo["visual_encoder.frame_position_embeddings.weight"][:F]
    h = O.transformer(h, sdo, "visual_encoder.temporal_transformer", 8, torch.zeros(F, F), torch.float32, tf_ln=True) + uo
    ref = (h / h.norm(dim=-1, keepdim=True)).mean(1)
    (ref * w.cpu()).sum().backward()
    close(out, ref, 2e-5, 1e-4, "video_emb")
    close(ug.grad, uo.grad, 2e-5, 1e-3, "du")
    P = dict(model.named_parameters())
    for k in ("visual_encoder.temporal_transformer.resblocks.0.attn.in_proj_weight",
              "visual_encoder.temporal_transformer.resblocks.3.mlp.c_proj.bias",
              "visual_encoder.temporal_transformer.resblocks.1.ln_2.weight",
              "visual_encoder.frame_position_embeddings.weight"):
        close(P[k].grad, sdo[k].grad, 2e-5, 2e-3, k)


def test_temporal_without_a_transformer_takes_an_input_that_records_no_graph():
    """use_temp = False: module_cross.py calls Fn.temporal(frame_output, 0, None).  With the grad mode on and a frame_output
    that does not require grad (a frozen frame tower) the pass records no graph and computes what the recording one does."""
    u = synth.normal("temporal.nograph.u", (5, 4, 512)).to(DEV)
    assert torch.is_grad_enabled()
    out = Fn.temporal(u, 0, None)
    assert not out.requires_grad
    ug = u.clone().requires_grad_()
    rec = Fn.temporal(ug, 0, None)
    assert rec.requires_grad and torch.equal(out, rec.detach())
    with torch.no_grad():
        assert torch.equal(out, Fn.temporal(ug, 0, None))
    close(out, (u / u.norm(dim=-1, keepdim=True)).mean(1).cpu(), 2e-5, 1e-4, "video_emb")   # the bound test_temporal_fn_vs_oracle holds this output to


# ----------------------------------------------------------------------------- full model

def build(dims, use_temp=True, **tc):
    from hmmc_amd.modeling import BirdModel
    sd = synth.finetune_state(dims, use_temp=use_temp)
    model = BirdModel.from_pretrained("cross-base", state_dict=sd, task_config=task_config(use_temp=use_temp, **tc))
    return model.to(DEV).train(), sd


ENC = [("enc_tiny", synth.TINY, True), ("enc_tiny_notemp", synth.TINY, False), ("enc_b32", synth.VIT_B32, True),
       ("enc_tiny16", synth.TINY16, True),       # patch 16: 197 tokens per frame (the ViT-B/16 attention path)
       ("enc_b16", synth.VIT_B16, True)]         # true ViT-B/16 dims: 197 tokens x 12 heads x 12 layers (SURVEY config 5)


@pytest.mark.parametrize("name,dims,use_temp", ENC)
def test_model_vs_reference_golden(name, dims, use_temp):
    mode = "aswritten" if name != "enc_tiny_notemp" else "fp32"
    g = golden(f"{name}_{mode}")
    B, Fr, L = int(g["B"]), int(g["F"]), int(g["L"])
    model, sd = build(dims, use_temp)
    ids, mask, vid, vf, idx = [t.to(DEV) for t in synth.finetune_batch(B, Fr, L, dims.image_res, tag=name)]
    q = model.text_encoder(ids, mask)
    v, u = model.visual_encoder(vid, vf)
    loss = model(ids, mask, vid, vf, idx, 1)
    loss.backward()
    tol = 3e-2
    close(q, g["text_feat"], tol, tol, "text_feat")
    close(u, g["frame_output"], tol, tol, "frame_output")
    close(v, g["video_emb"], tol, tol, "video_emb")
    close(loss, g["loss"], 3e-2, what="loss")
    if mode == "aswritten":
        # the envelope the reference itself has: its fp16-as-written and fp32-upcast regimes on the same weights and inputs.
        # This path must sit as close to the as-written reference as that reference sits to its own fp32 run (x ENVELOPE).
        gf = golden(f"{name}_fp32")
        for mine, key in ((q, "text_feat"), (u, "frame_output"), (v, "video_emb")):
            own = relerr(torch.from_numpy(g[key]), torch.from_numpy(gf[key]))
            got = relerr(mine.detach().cpu(), torch.from_numpy(g[key]))
            print(f"{name} {key}: rel-L2 vs as-written {got:.3e}; the reference's own regimes differ by {own:.3e}")
            assert got <= ENVELOPE * own, f"{key}: {got:.3e} > {ENVELOPE} x {own:.3e}"
    # retrieval ranks of this batch identical to the reference's
    with torch.no_grad():
        S = model.loose_similarity(q.detach(), v.detach()).cpu().numpy()
    Sref = O.loose_similarity(torch.from_numpy(g["text_feat"]), torch.from_numpy(g["video_emb"])).numpy()
    assert np.array_equal(np.argsort(-S, 1), np.argsort(-Sref, 1)), "ranks differ"
    # gradients: per-parameter norms against the reference's own (as-written fp16 autograd is noisy)
    names = [str(n) for n in g["grad_norm_names"]]
    ref = dict(zip(names, g["grad_norm_values"]))
    P = dict(model.named_parameters())
    bad = []
    for n in names:
        assert P[n].grad is not None, f"no grad for {n}"
        gn = float(P[n].grad.float().norm())
        if abs(gn - ref[n]) > 0.15 * ref[n] + 2e-4:
            bad.append((n, gn, float(ref[n])))
    assert not bad, f"{len(bad)} of {len(names)} grad norms off: {bad[:8]}"


ENVELOPE = 1.5      # x the reference's own fp16-as-written vs fp32-upcast gap


def test_envelope_at_true_vit_b32_dims():
    """True ViT-B/32 dimensions, 8 captions x 8 videos of 4 frames (tests/golden/enc_b32x8_*.npz, both regimes of the
    reference): features, the x100 video-text logits and the mean top-2 frame logits (modules/module_cross.py:178-237,
    main_task_retrieval.py:332-336) within 1.5 x the reference's own regime gap - element-wise maximum and relative L2 -
    and the rank rule of test_retrieval_ranks_b32_vs_reference: a pair of candidates may swap only if the reference's own
    logits for the two are closer than that envelope."""
    ga, gf = golden("enc_b32x8_aswritten"), golden("enc_b32x8_fp32")
    B, Fr, L, k = int(ga["B"]), int(ga["F"]), int(ga["L"]), int(ga["k"])
    model, sd = build(synth.VIT_B32, max_frames=Fr, top_frames=k)
    ids, mask, vid, vf, idx = [t.to(DEV) for t in synth.finetune_batch(B, Fr, L, synth.VIT_B32.image_res, tag="enc_b32x8")]
    with torch.no_grad():
        q = model.text_encoder(ids, mask)
        v, u = model.visual_encoder(vid, vf)
        sv, fk = model.eval_scores(q, v, u, top_frames=k)
        loss = model(ids, mask, vid, vf, idx, 1)
    got = {"text_feat": q, "video_emb": v, "frame_output": u, "S_video": sv, "S_frame_topk": fk}
    fails = []
    for key, mine in got.items():
        mine = mine.cpu().numpy()
        own_max, own_l2 = float(np.abs(ga[key] - gf[key]).max()), float(np.linalg.norm(ga[key] - gf[key]) / np.linalg.norm(gf[key]))
        my_max, my_l2 = float(np.abs(mine - ga[key]).max()), float(np.linalg.norm(mine - ga[key]) / np.linalg.norm(ga[key]))
        f32_max, f32_l2 = float(np.abs(mine - gf[key]).max()), float(np.linalg.norm(mine - gf[key]) / np.linalg.norm(gf[key]))
        print(f"{key}: max |HIP - as-written| {my_max:.3e} (reference regimes {own_max:.3e}), rel-L2 {my_l2:.3e} ({own_l2:.3e}); "
              f"against the reference's fp32 regime max {f32_max:.3e}, rel-L2 {f32_l2:.3e}")
        if my_max > ENVELOPE * own_max:
            fails.append(f"{key}: max abs {my_max:.3e} > {ENVELOPE} x {own_max:.3e}")
        if my_l2 > ENVELOPE * own_l2:
            fails.append(f"{key}: rel-L2 {my_l2:.3e} > {ENVELOPE} x {own_l2:.3e}")
    assert not fails, fails
    assert abs(float(loss) - float(ga["loss"])) <= ENVELOPE * max(abs(float(ga["loss"]) - float(gf["loss"])), 1e-3)
    for key in ("S_video", "S_frame_topk"):
        mine, ra = got[key].cpu().numpy(), ga[key]
        env = ENVELOPE * float(np.abs(ga[key] - gf[key]).max())
        gap = ra[:, :, None] - ra[:, None, :]
        far = np.abs(gap) > 2 * env
        mygap = mine[:, :, None] - mine[:, None, :]
        assert (np.sign(mygap[far]) == np.sign(gap[far])).all(), f"{key}: a pair the reference separates clearly is out of order"
        ref_rank = (ra > np.diag(ra)[:, None]).sum(1)
        my_rank = (mine > np.diag(mine)[:, None]).sum(1)
        amb = (np.abs(ra - np.diag(ra)[:, None]) <= 2 * env).sum(1) - 1
        assert (np.abs(my_rank - ref_rank) <= amb).all() and (my_rank == ref_rank)[amb == 0].all(), (key, my_rank, ref_rank, amb)


def test_frame_loss_member_vs_reference_golden():
    """BirdModel.frame_loss(query, frames) as a callable member (reference modules/modeling.py:665-672), value and gradients
    against the reference's own (tests/golden/head_ft_small.npz stores frame_loss; its gradient is checked against autograd
    through the oracle's restatement)."""
    g = golden("head_ft_small")
    B, Fr = int(g["B"]), int(g["F"])
    model, _ = build(synth.TINY)
    q = synth.normal("head_ft_small.q", (B, 512)).to(DEV).requires_grad_()
    u = synth.normal("head_ft_small.u", (B, Fr, 512)).to(DEV).requires_grad_()
    fl = model.frame_loss(q, u)
    close(fl, g["frame_loss"], 2e-5, what="frame_loss")
    fl.backward()
    qo, uo = q.detach().cpu().requires_grad_(), u.detach().cpu().requires_grad_()
    ref = O.frame_loss(qo, uo)
    ref.backward()
    close(fl, ref, 2e-5, what="frame_loss vs oracle")
    close(q.grad, qo.grad, 2e-6, 1e-4, "dQ")
    close(u.grad, uo.grad, 2e-6, 1e-4, "dU")


def test_retrieval_ranks_b32_vs_reference():
    """End-to-end acceptance on a batch where ranks CAN differ: 32 captions x 32 videos (4 frames) through the HIP towers,
    the 32 x 32 video-text matrix and the eval score S_video + mean top-2 frame logits (main_task_retrieval.py:332-336)
    against the reference's own outputs (tests/golden/enc_rank_*.npz).  The reference's two regimes (fp16 as written, fp32
    upcast) already disagree with each other in 24 / 54 / 36 of the 1 024 argsort positions of these matrices (adjacent
    logits are a median 0.03 apart, fp16 noise is 0.014), so "identical ranks" is asserted as: (1) every logit within the
    fp16 envelope of the as-written reference, (2) every pair of candidates the reference separates by more than twice
    that envelope in the same order (so every ground-truth rank equals the reference's unless a competitor is that close), (3) no more than twice as many argsort positions away from either regime of the reference
    as its regimes are from each other, (4) the rank metrics of metrics.py equal up to those near ties."""
    from hmmc_amd import metrics as M
    ga, gf = golden("enc_rank_aswritten"), golden("enc_rank_fp32")
    B, Fr, L, k = int(ga["B"]), int(ga["F"]), int(ga["L"]), int(ga["k"])
    model, sd = build(synth.TINY, max_frames=Fr, top_frames=k)
    ids, mask, vid, vf, idx = [t.to(DEV) for t in synth.finetune_batch(B, Fr, L, synth.TINY.image_res, tag="enc_rank")]
    with torch.no_grad():
        q = model.text_encoder(ids, mask)
        v, u = model.visual_encoder(vid, vf)
        sv, fk = model.eval_scores(q, v, u, top_frames=k)
    sv, fk = sv.cpu().numpy(), fk.cpu().numpy()
    # envelope: 1.5 x the largest difference between the reference's own two regimes on these logits (0.0143 -> 0.0215)
    env = 1.5 * max(float(np.abs(ga[k_] - gf[k_]).max()) for k_ in ("S_video", "S_frame_topk"))
    for mine, key in ((sv, "S_video"), (fk, "S_frame_topk"), (sv + fk, None)):
        ra = ga[key] if key else ga["S_video"] + ga["S_frame_topk"]
        rf = gf[key] if key else gf["S_video"] + gf["S_frame_topk"]
        what = key or "score"
        err = np.abs(mine - ra).max()
        print(f"{what}: max |logit - reference| = {err:.4f} (envelope {env * (2 if key is None else 1):.4f})")
        assert err <= env * (2 if key is None else 1), f"{what}: logits off by {err}"
        gap = ra[:, :, None] - ra[:, None, :]
        far = np.abs(gap) > 2 * env * (2 if key is None else 1)
        mygap = mine[:, :, None] - mine[:, None, :]
        assert (np.sign(mygap[far]) == np.sign(gap[far])).all(), f"{what}: a pair the reference separates clearly is out of order"
        flips = int((np.argsort(-mine, 1) != np.argsort(-ra, 1)).sum())
        own = int((np.argsort(-rf, 1) != np.argsort(-ra, 1)).sum())
        # two independent fp16 evaluations differ by sqrt(2) x the noise of one fp16 evaluation against fp32: allow 2 x
        assert flips <= 2 * own, f"{what}: {flips} argsort positions differ from the reference; its own regimes differ in {own}"
        vs32 = int((np.argsort(-mine, 1) != np.argsort(-rf, 1)).sum())
        assert vs32 <= 2 * own, f"{what}: {vs32} argsort positions differ from the reference's fp32 regime ({own} for its fp16 one)"
    # rank of the ground-truth video per caption (metrics.py:20-28, computed on the device): equal to the reference's
    # wherever no competitor sits within the envelope of the ground truth's own logit, and never further away than the
    # number of such competitors; R@K / median / mean follow
    for mine, key, width in ((sv + fk, "metrics_score", 2), (sv, "metrics_video", 1)):
        ra = ga["S_video"] + ga["S_frame_topk"] if width == 2 else ga["S_video"]
        ref_rank = (ra > np.diag(ra)[:, None]).sum(1)
        amb = (np.abs(ra - np.diag(ra)[:, None]) <= 2 * env * width).sum(1) - 1
        my_rank = M.ranks(torch.from_numpy(np.ascontiguousarray(mine)).to(DEV))
        assert (np.abs(my_rank - ref_rank) <= amb).all(), (key, my_rank, ref_rank, amb)
        assert (my_rank == ref_rank)[amb == 0].all()
        mt = M.metrics_from_ranks(my_rank)
        got = np.array([mt["R1"], mt["R5"], mt["R10"], mt["MR"], mt["MeanR"]])
        moved = int((my_rank != ref_rank).sum())
        assert np.abs(got[:3] - ga[key][:3]).max() <= 100.0 * moved / B + 1e-9, (key, got, ga[key])
        assert abs(got[4] - ga[key][4]) <= float(np.abs(my_rank - ref_rank).sum()) / B + 1e-6, (key, got, ga[key])


@pytest.mark.parametrize("dims,name", [(synth.TINY, "enc_tiny"), (synth.VIT_B32, "enc_b32")])
def test_model_vs_oracle_fp32_gradients(dims, name):
    """Direction check of every gradient against the fp32 oracle (cosine similarity): the tiny model, and the true
    ViT-B/32 dimensions (12 layers, 12 heads, K = 3072: the shapes that take the 256x256 GEMM tile, split-K and the fused
    bias-gradient partials in production)."""
    g = golden(f"{name}_fp32")
    B, Fr, L = int(g["B"]), int(g["F"]), int(g["L"])
    model, sd = build(dims)
    batch = synth.finetune_batch(B, Fr, L, dims.image_res, tag=name)
    ids, mask, vid, vf, idx = [t.to(DEV) for t in batch]
    model(ids, mask, vid, vf, idx, 1).backward()
    sdo = {k: t.clone().requires_grad_(t.is_floating_point()) for k, t in sd.items()}
    loss, _ = O.finetune_loss(batch[0], batch[2], sdo, mode="fp32")
    loss.backward()
    worst = []
    for n, p in model.named_parameters():
        a, b = p.grad.float().cpu().flatten(), sdo[n].grad.flatten()
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-20))
        if cos < 0.98:
            worst.append((n, cos, float(a.norm()), float(b.norm())))
    assert not worst, f"gradient direction mismatches: {worst[:10]}"


def test_bertadam_vs_reference_golden():
    from hmmc_amd.optimization import BertAdam
    g = golden("bertadam")
    specs = [("a32", (37,), torch.float32, 0.2, 1e-4, 3.0), ("b32", (8, 9), torch.float32, 0.0, 3e-5, 0.01),
             ("c16", (64,), torch.float16, 0.2, 1e-4, 2.0), ("d16", (4, 32), torch.float16, 0.0, 1e-7, 0.05)]
    params, groups = [], []
    for name, shape, dt, wd, lr, gscale in specs:
        p = torch.nn.Parameter(synth.normal(f"bertadam.{name}.p", shape, 0.5).to(dt).to(DEV))
        params.append(p)
        groups.append({"params": [p], "weight_decay": wd, "lr": lr})
    opt = BertAdam(groups, lr=1e-4, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=20,
                   weight_decay=0.2, max_grad_norm=1.0)
    for step in range(5):
        for (name, shape, dt, wd, lr, gscale), p in zip(specs, params):
            p.grad = synth.normal(f"bertadam.{name}.g{step}", shape, gscale).to(dt).to(DEV)
        opt.step()
        close(opt.get_lr(), g[f"lr{step}"], 1e-12, what="lr")
        for (name, shape, dt, *_), p in zip(specs, params):
            st = opt.state[p]
            for nm, mine in (("p", p.data), ("m", st["next_m"]), ("v", st["next_v"]), ("g", p.grad)):
                ref = torch.from_numpy(g[f"{name}.{nm}{step}"])
                if dt == torch.float16:
                    nbad = int((mine.float().cpu() != ref).sum())
                    assert nbad == 0, f"{name}.{nm}{step}: {nbad} fp16 elements differ from the reference"
                else:
                    close(mine, ref, 2e-8, 2e-6, f"{name}.{nm}{step}")


def test_bertadam_skipped_steps_and_many_groups():
    """A parameter whose gradient was None for a step has its own step count, hence its own scheduled lr; 40 groups with 40
    learning rates exceed the 32 hyper-parameter rows of one launch.  Every tensor must still follow
    modules/optimization.py:103-168 (the oracle's op-by-op restatement), as the reference optimizer would."""
    from hmmc_amd.optimization import BertAdam
    n_groups, t_total = 40, 20
    ps = [torch.nn.Parameter(synth.normal(f"ba2.p{i}", (33 + i,), 0.5).to(DEV)) for i in range(n_groups)]
    groups = [{"params": [p], "lr": 1e-3 * (1 + i), "weight_decay": 0.1 * (i % 3)} for i, p in enumerate(ps)]
    opt = BertAdam(groups, lr=1e-3, warmup=0.2, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=t_total,
                   weight_decay=0.0, max_grad_norm=1.0)
    ref = [(p.detach().cpu().clone(), torch.zeros(p.shape), torch.zeros(p.shape), 0) for p in ps]
    for step in range(4):
        for i, p in enumerate(ps):
            skip = (i == 5 and step == 1) or (i == 17 and step in (0, 2))
            p.grad = None if skip else synth.normal(f"ba2.g{i}.{step}", tuple(p.shape), 0.3).to(DEV)
        opt.step()
        for i, p in enumerate(ps):
            if p.grad is None:
                continue
            rp, rm, rv, rs = ref[i]
            rp, rm, rv, _ = O.bert_adam_step(rp, p.grad.cpu(), rm, rv, rs, 1e-3 * (1 + i), t_total, 0.2, 0.1 * (i % 3))
            ref[i] = (rp, rm, rv, rs + 1)
    for i, p in enumerate(ps):
        close(p.data, ref[i][0], 1e-7, 2e-6, f"param {i}")
        assert opt.state[p]["step"] == ref[i][3]


def prep_optimizer(model, cfg, t_total):
    from hmmc_amd.optimization import BertAdam
    named = list(model.named_parameters())
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    dec = [(n, p) for n, p in named if not any(nd in n for nd in no_decay)]
    nod = [(n, p) for n, p in named if any(nd in n for nd in no_decay)]
    wd, lrc = cfg.weight_decay, cfg.lr * cfg.coef_lr
    groups = [
        {"params": [p for n, p in dec if "visual_encoder.visual." in n], "weight_decay": wd, "lr": lrc},
        {"params": [p for n, p in dec if "text_encoder." in n], "weight_decay": wd, "lr": cfg.text_lr},
        {"params": [p for n, p in dec if "visual_encoder.visual." not in n and "text_encoder." not in n], "weight_decay": wd},
        {"params": [p for n, p in nod if "visual_encoder.visual." in n], "weight_decay": 0.0, "lr": lrc},
        {"params": [p for n, p in nod if "text_encoder." in n], "weight_decay": 0.0, "lr": cfg.text_lr},
        {"params": [p for n, p in nod if "visual_encoder.visual." not in n and "text_encoder." not in n], "weight_decay": 0.0},
    ]
    return BertAdam(groups, lr=cfg.lr, warmup=cfg.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
                    t_total=t_total, weight_decay=wd, max_grad_norm=1.0)


SAMPLED = ["text_encoder.text_projection", "visual_encoder.visual.conv1.weight", "visual_encoder.visual.class_embedding",
           "visual_encoder.visual.transformer.resblocks.1.mlp.c_proj.weight",
           "visual_encoder.visual.transformer.resblocks.0.ln_1.weight",
           "visual_encoder.temporal_transformer.resblocks.2.attn.in_proj_weight",
           "text_encoder.transformer.resblocks.0.attn.in_proj_bias", "text_encoder.ln_final.bias"]


def test_train_steps_vs_reference_golden():
    """4 full steps (forward, backward, global clip, BertAdam) of the reference's loop (main_task_retrieval.py:272-302).
    The optimizer itself is pinned bit-for-bit by test_bertadam_vs_reference_golden on identical gradients.  Here the
    gradients come from two different fp16 back-propagations, and BertAdam without bias correction turns every
    gradient element into a step of ~0.7*lr*sign(g) (fp16 second moments underflow to 0 below |g| ~ 2.4e-4), so
    post-update weights are compared by the DIRECTION of their movement, and post-update losses loosely."""
    from hmmc_amd.optimization import clip_grad_norm_
    g = golden("train_ft_aswritten")
    model, sd = build(synth.TINY, lr=2e-3, text_lr=1e-3, coef_lr=0.5)
    cfg = model.task_config
    opt = prep_optimizer(model, cfg, 10)
    P = dict(model.named_parameters())
    init = {k: P[k].data.reshape(-1)[:16].float().cpu().clone() for k in SAMPLED}
    for step in range(4):
        ids, mask, vid, vf, idx = [t.to(DEV) for t in synth.finetune_batch(4, 4, 32, tag=f"train_ft.s{step}")]
        loss = model(ids, mask, vid, vf, idx, step + 1)
        loss.backward()
        tn = clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        close(loss, g[f"loss{step}"], 4e-2 if step < 2 else 0.25, what=f"loss{step}")
        close(tn, g[f"gnorm{step}"], 0.0, 0.15 if step < 2 else 0.4, f"gnorm{step}")
        if step == 0:       # first step has lr 0 (state['step'] starts at 0): weights must not move
            for k in SAMPLED:
                close(P[k].data.reshape(-1)[:16], g[f"p0:{k}"], 1e-6, 1e-3, f"p0:{k}")
        else:
            cos = []
            for k in SAMPLED:
                mine = P[k].data.reshape(-1)[:16].float().cpu() - init[k]
                ref = torch.from_numpy(g[f"p{step}:{k}"]) - init[k]
                cos.append(float(torch.dot(mine, ref) / (mine.norm() * ref.norm() + 1e-12)))
            assert np.mean(cos) > 0.6, f"step {step}: weight movement disagrees with the reference: {cos}"


def test_encode_image_all_tokens_and_class_token_paths_agree():
    """encode_image(return_hidden=True) runs the full last block and returns every token's projection (the reference's
    `hidden`, module_cross.py:228-236); the default path prunes the last block to the class token.  Both give the same
    class-token feature, bit for bit, and module_clip.VisualTransformer.forward() still returns all tokens."""
    model, _ = build(synth.TINY)
    model.eval()
    _, _, vid, _, _ = synth.finetune_batch(3, 4, 32, tag="hid")
    frames = vid.view(-1, *vid.shape[2:]).to(DEV)
    enc = model.visual_encoder
    with torch.no_grad():
        feat = enc.encode_image(frames)
        feat_h, hidden = enc.encode_image(frames, return_hidden=True)
        tokens = enc.visual(frames)
    L = enc.visual.tokens
    assert hidden.shape == (frames.shape[0], L, feat.shape[-1]) and tokens.shape[:2] == (frames.shape[0], L)
    assert torch.equal(feat, feat_h) and torch.equal(feat_h, hidden[:, 0, :])
    assert bool(torch.isfinite(hidden).all()) and bool(torch.isfinite(tokens.float()).all())
    assert float(hidden[:, 1:].float().abs().mean()) > 0          # the other tokens are computed, not left undefined


def test_uint8_frames_equal_normalised_fp32_frames():
    """raw uint8 frames with the loader's normalisation fused into the patch extraction give the
    same loss and gradients as the fp32 frames the reference's loader hands over."""
    from hmmc_amd.modeling import BirdModel
    from hmmc_amd import ops as _ops
    sd = synth.finetune_state(synth.TINY)
    ids, mask, vid, vf, idx = synth.finetune_batch(4, 4, 32, tag="u8")
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, vid.shape, generator=g, dtype=torch.uint8)
    mean = torch.tensor(_ops.CLIP_PIXEL_MEAN).view(1, 1, 3, 1, 1)
    std = torch.tensor(_ops.CLIP_PIXEL_STD).view(1, 1, 3, 1, 1)
    f32 = (u8.float().div(255.0) - mean) / std
    out = []
    for video in (u8, f32):
        model = BirdModel.from_pretrained("cross-base", state_dict=sd, task_config=task_config(max_frames=4)).to(DEV).train()
        loss = model(ids.to(DEV), mask.to(DEV), video.to(DEV), vf.to(DEV), idx.to(DEV), 1)
        loss.backward()
        out.append((float(loss), model.visual_encoder.visual.conv1.weight.grad.clone()))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])


def test_frames_sampled_on_the_device_equal_gathered_frames():
    """The loader's frame sampling (dataloader_msrvtt_retrieval.py:296-312) with the clip's 30 stored uint8 frames in HBM:
    the encoder reads the sampled frames in place through a device index.  Features equal, bit for bit, those of the same
    frames gathered and normalised to fp32 on the host first (the reference's path), for all three policies."""
    import random
    from hmmc_amd import ops as _ops, sampling
    model, _ = build(synth.TINY, max_frames=6)
    model.eval()
    bs, stored, frames = 3, 30, 6
    g = torch.Generator().manual_seed(9)
    clips = torch.randint(0, 256, (bs, stored, 3, 224, 224), generator=g, dtype=torch.uint8)
    mean = torch.tensor(_ops.CLIP_PIXEL_MEAN).view(1, 1, 3, 1, 1)
    std = torch.tensor(_ops.CLIP_PIXEL_STD).view(1, 1, 3, 1, 1)
    clips_dev = clips.to(DEV)
    for policy in sampling.POLICIES:
        random.seed(4)
        index = sampling.batch_frame_index(policy, bs, stored, frames, DEV)
        random.seed(4)
        picked = torch.stack([clips[v, sampling.frame_indices(policy, stored, frames)] for v in range(bs)])
        f32 = (picked.float().div(255.0) - mean) / std
        with torch.no_grad():
            v0, u0 = model.visual_encoder(clips_dev, None, frame_index=index)
            v1, u1 = model.visual_encoder(f32.to(DEV), None)
        assert u0.shape == (bs, frames, 512)
        assert torch.equal(u0, u1) and torch.equal(v0, v1), policy


def test_step_is_deterministic_across_runs_and_stream_modes():
    """Two fresh models, same weights and batch: loss and every gradient bit-identical from run to run, and identical with
    the multi-stream overlap (text tower beside the frame tower, weight gradients on their own stream) switched off.  A
    missing event between the streams would show up here as a run-to-run difference."""
    from hmmc_amd.modeling import BirdModel
    import hmmc_amd.modeling as M
    import hmmc_amd.functional as Fn2
    dims = synth.TINY
    sd = synth.finetune_state(dims)
    batch = [t.to(DEV) for t in synth.finetune_batch(16, 6, 32, tag="det")]

    def run():
        model = BirdModel.from_pretrained("cross-base", state_dict=sd, task_config=task_config(max_frames=6)).to(DEV).train()
        loss = model(*batch, 1)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    saved = (M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM)
    try:
        M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM = True, True
        l1, g1 = run()
        l2, g2 = run()
        M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM = False, False
        l3, g3 = run()
    finally:
        M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM = saved
    assert l1 == l2 == l3, (l1, l2, l3)
    for n in g1:                     # every gradient, the token-embedding scatter included (owner rows, no atomics)
        assert torch.equal(g1[n], g2[n]), f"run-to-run difference in {n}"
        assert torch.equal(g1[n], g3[n]), f"overlap on/off difference in {n}"


def test_training_steps_are_deterministic_including_the_updated_weights():
    """Three optimizer steps (forward, backward, global clip, BertAdam) from identical state, repeated: losses and every
    weight bit-identical from run to run and between the stream modes.  The norms behind the clip coefficient and the
    per-parameter clip are sums over chunks of a tensor; with fp32 atomics their order, and with it every updated weight,
    changed from run to run (found by scratch/soak_determinism.py; the single-step test above cannot see it)."""
    import copy
    from hmmc_amd.modeling import BirdModel
    from hmmc_amd.optimization import clip_grad_norm_
    import hmmc_amd.modeling as M
    import hmmc_amd.functional as Fn2
    cfg = task_config(max_frames=4, pretrained_clip_name="ViT-B/32")
    model = BirdModel.from_pretrained("cross-base", state_dict=synth.finetune_state(synth.VIT_B32), task_config=cfg).to(DEV).train()
    batch = [t.to(DEV) for t in synth.finetune_batch(8, 4, 32, tag="det3")]
    sd0 = copy.deepcopy(model.state_dict())
    params = [p for p in model.parameters() if p.requires_grad]

    def run(overlap):
        M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM = overlap, overlap
        model.load_state_dict(sd0)
        opt = prep_optimizer(model, cfg, 50)
        losses = []
        for i in range(3):
            loss = model(*batch, i + 1)
            loss.backward()
            clip_grad_norm_(params, 1.0)
            opt.step()
            opt.zero_grad()
            losses.append(float(loss))
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in params]

    saved = (M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM)
    try:
        ref_l, ref_w = run(False)
        for overlap in (False, True, True, True, False, True):
            l, w = run(overlap)
            assert l == ref_l, (overlap, l, ref_l)
            bad = [i for i, (a, b) in enumerate(zip(w, ref_w)) if not torch.equal(a, b)]
            assert not bad, f"overlap={overlap}: {len(bad)} weight tensors differ from run to run"
    finally:
        M._OVERLAP_TOWERS, Fn2._WGRAD_STREAM = saved


@pytest.mark.parametrize("B,Fr,L", [(5, 3, 20), (2, 1, 32), (3, 7, 77), (7, 5, 9)])
def test_model_vs_oracle_odd_shapes(B, Fr, L):
    """Ragged sizes through the whole fine-tune path against the fp32 oracle: batch / frame counts that are not multiples of
    any tile, one frame per video, and a 77-token text (the causal long-sequence attention kernel inside the text tower).
    Loss within the as-written envelope, every gradient's direction (cosine >= 0.98)."""
    dims = synth.TINY
    model, sd = build(dims, max_frames=Fr)
    batch = synth.finetune_batch(B, Fr, L, dims.image_res, tag=f"odd{B}.{Fr}.{L}")
    ids, mask, vid, vf, idx = [t.to(DEV) for t in batch]
    loss = model(ids, mask, vid, vf, idx, 1)
    loss.backward()
    sdo = {k: t.clone().requires_grad_(t.is_floating_point()) for k, t in sd.items()}
    ref, _ = O.finetune_loss(batch[0], batch[2], sdo, mode="fp32")
    ref.backward()
    close(loss, ref, 3e-2, 3e-2, "loss")
    worst = []
    for n, p in model.named_parameters():
        if p.grad is None:
            assert sdo[n].grad is None or float(sdo[n].grad.abs().max()) == 0.0, n
            continue
        a, b = p.grad.float().cpu().flatten(), sdo[n].grad.flatten()
        if float(b.norm()) < 1e-9:                      # e.g. frame position rows beyond Fr
            assert float(a.norm()) < 1e-6, (n, float(a.norm()))
            continue
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-20))
        if cos < 0.98:
            worst.append((n, cos, float(a.norm()), float(b.norm())))
    assert not worst, f"gradient direction mismatches: {worst[:10]}"


def test_clip_grad_norm_follows_the_gradients_it_is_given():
    """Two gradient sets with the same tensor count and total size but other dtypes / a different split of the sizes, clipped
    one after the other in one process: the cached table must follow the tensors it is given (round 2 keyed its static
    columns on count and total size alone and would have read the second set with the first one's sizes and dtypes)."""
    from hmmc_amd.optimization import clip_grad_norm_
    g = torch.Generator().manual_seed(5)
    for sizes, dtype in (((1000, 24, 4096), torch.float32), ((1000, 24, 4096), torch.float16), ((4096, 24, 1000), torch.float16),
                         ((1000, 24, 4096), torch.float32)):
        ps = [torch.nn.Parameter(torch.zeros(n, dtype=dtype, device=DEV)) for n in sizes]
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 3).to(dtype).to(DEV)
        ref = [p.grad.float().clone() for p in ps]
        total = torch.sqrt(sum((r.double() ** 2).sum() for r in ref))
        tn = clip_grad_norm_(ps, 1.0)
        close(tn, total, 0.0, 2e-3 if dtype == torch.float16 else 1e-5, "total norm")
        coef = min(1.0, 1.0 / (float(total) + 1e-6))
        for p, r in zip(ps, ref):
            close(p.grad, r * coef, 1e-6, 2e-3 if dtype == torch.float16 else 1e-5, "clipped gradient")


def _clip_and_step(shared, max_norm, scales, touch_after_clip=False, other_stream=False):
    """One `clip_grad_norm_; optimizer.step()` pair (twice: the first step plans the optimizer's fast path) on a fixed mix of
    fp16 / fp32 tensors in two parameter groups whose order differs from the order the clip sees; returns every resulting tensor."""
    from hmmc_amd import optimization
    from hmmc_amd.optimization import BertAdam, clip_grad_norm_
    g = torch.Generator().manual_seed(11)
    sizes = [(40000, torch.float16), (77, torch.float32), (32768, torch.float16), (5, torch.float16), (100003, torch.float32), (4096, torch.float16)]
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dt).to(DEV)) for n, dt in sizes]
    groups = [{"params": [ps[3], ps[0], ps[4]], "weight_decay": 0.01}, {"params": [ps[5], ps[1], ps[2]], "weight_decay": 0.0, "lr": 3e-4}]
    opt = BertAdam(groups, lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=50, max_grad_norm=1.0)
    old = optimization._NO_SHARED_NORMS
    optimization._NO_SHARED_NORMS = not shared
    try:
        for step in range(3):
            for i, p in enumerate(ps):
                p.grad = (torch.randn(p.shape, generator=g) * scales[i % len(scales)] * (1 + step)).to(p.dtype).to(DEV)
            clip_grad_norm_(ps, max_norm)                      # the order of model.parameters(), not the optimizer's
            if touch_after_clip and step == 2:
                ps[0].grad.mul_(3.0)                            # a version bump the hand-over must notice
            if other_stream and step == 2:
                s2 = torch.cuda.Stream()
                s2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s2):
                    opt.step()
                torch.cuda.current_stream().wait_stream(s2)
            else:
                opt.step()
    finally:
        optimization._NO_SHARED_NORMS = old
    torch.cuda.synchronize()
    return [t.detach().clone() for p in ps for t in (p, p.grad, opt.state[p]["next_m"], opt.state[p]["next_v"])]


@pytest.mark.parametrize("max_norm,scales", [(1.0, (3.0, 0.5)), (1e6, (0.001, 0.0005)), (1e6, (30.0, 0.01)), (0.05, (2.0, 2.0))])
def test_optimizer_takes_the_norms_the_clip_left_bit_identical(max_norm, scales):
    """`clip_grad_norm_` hands the per-tensor squared norms of the clipped gradients to the `BertAdam.step()` that follows
    (reference loop main_task_retrieval.py:291-296; BertAdam clips per parameter inside step(), modules/optimization.py:140-150),
    which then skips its own pass over every gradient.  Weights, moments and gradients must be BIT-identical to the path that
    forms the norms itself: global clip active and inactive (coefficient 1: the first pass's sums are handed on), per-parameter
    clip active (gradient norms > 1 after a no-op global clip) and inactive, fp16 and fp32 tensors, tensor order differing
    between the two calls; and the hand-over must be dropped when a gradient is written to after the clip or the step runs on
    another stream."""
    ref = _clip_and_step(False, max_norm, scales)
    got = _clip_and_step(True, max_norm, scales)
    assert all(torch.equal(a, b) for a, b in zip(ref, got)), "shared norms changed a result"
    ref_t = _clip_and_step(False, max_norm, scales, touch_after_clip=True)
    got_t = _clip_and_step(True, max_norm, scales, touch_after_clip=True)
    assert all(torch.equal(a, b) for a, b in zip(ref_t, got_t)), "a gradient modified after the clip must not use the stale norms"
    assert not all(torch.equal(a, b) for a, b in zip(ref, ref_t)), "(the modification matters)"
    got_s = _clip_and_step(True, max_norm, scales, other_stream=True)
    assert all(torch.equal(a, b) for a, b in zip(ref, got_s)), "step on another stream"


def test_class_token_gradient_buffer_is_not_zero_filled_and_not_read(monkeypatch):
    """Round 5: the backward of ln_post / proj hands the frame tower a gradient buffer in which only the class-token rows are
    written (LnProjFn rows_only; the tower ran lead_only and reads those rows alone, include/hmmc_hip.h) instead of zero-filling
    [tokens, D].  Loss and every gradient must be bit-identical to the zero-filled form, with the allocator's free blocks
    poisoned with NaN right before the backward."""
    model, sd = build(synth.TINY)
    batch = [t.to(DEV) for t in synth.finetune_batch(6, 4, 32, tag="rows_only")]

    def run(rows_only):
        orig = Fn.LnProjFn.forward

        def fwd(ctx, x, row_index, ln_w, ln_b, proj, ro=False):
            return orig(ctx, x, row_index, ln_w, ln_b, proj, ro and rows_only)
        monkeypatch.setattr(Fn.LnProjFn, "forward", staticmethod(fwd))
        model.zero_grad(set_to_none=True)
        loss = model(*batch, 1)
        torch.cuda.synchronize()
        junk = [torch.full((n,), float("nan"), dtype=torch.float16, device=DEV) for n in (6 * 4 * 50 * 128, 6 * 4 * 50 * 128, 1 << 20)]
        del junk                                            # the caching allocator hands these blocks to the backward's empty_like
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    l0, g0 = run(False)
    l1, g1 = run(True)
    assert torch.equal(l0, l1)
    assert all(torch.isfinite(g).all() for g in g1.values())
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad[:5]


def test_tower_release_gives_back_the_event_sets_and_the_next_backward_recreates_them():
    """hmmc_tower_release (round 5): the seven events a (stream, weight-gradient stream) pair got on its first hmmc_tower_bwd call
    are destroyed on request; the pair's next backward creates a fresh set and computes the same bits."""
    from hmmc_amd import _lib
    model, sd = build(synth.TINY)
    batch = [t.to(DEV) for t in synth.finetune_batch(4, 4, 32, tag="release")]

    def run():
        model.zero_grad(set_to_none=True)
        loss = model(*batch, 1)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]

    l0, g0 = run()
    lib = _lib.load()
    n = lib.hmmc_tower_release(None, None)                   # every pair: nothing of this process is in flight (synchronised above)
    assert n >= 1, "the backward above used a weight-gradient stream: at least one pair had its events"
    assert lib.hmmc_tower_release(None, None) == 0
    l1, g1 = run()
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert lib.hmmc_tower_release(None, None) >= 1


def test_fast_path_with_parameters_that_never_get_a_gradient():
    """The pre-training model hands BertAdam parameters that never receive a gradient (t_projector is built and never used,
    reference modules/modeling.py:113-114; the momentum encoders do not require grad).  Round 5: the steady-state fast path of
    step() covers the parameters that do get one and holds while exactly the others stay without; results must be bit-identical
    to an optimizer that was never given the idle parameters, and a gradient turning up on an idle parameter must fall back."""
    from hmmc_amd.optimization import BertAdam, clip_grad_norm_
    g = torch.Generator().manual_seed(31)
    sizes = [(40000, torch.float16), (77, torch.float32), (32768, torch.float16), (1000, torch.float32), (4096, torch.float16)]

    def make():
        return [torch.nn.Parameter((torch.randn(n, generator=torch.Generator().manual_seed(100 + i)) * 0.1).to(dt).to(DEV))
                for i, (n, dt) in enumerate(sizes)]
    ps_a, ps_b = make(), make()
    idle = [1, 3]                                                  # these never get a gradient
    live_b = [p for i, p in enumerate(ps_b) if i not in idle]
    kw = dict(lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=50, max_grad_norm=1.0)
    opt_a = BertAdam([{"params": ps_a[:3], "weight_decay": 0.01}, {"params": ps_a[3:], "weight_decay": 0.0}], **kw)
    opt_b = BertAdam([{"params": [ps_b[0], ps_b[2]], "weight_decay": 0.01}, {"params": [ps_b[4]], "weight_decay": 0.0}], **kw)
    for step in range(4):
        grads = [(torch.randn(n, generator=g) * 2.0).to(dt).to(DEV) for n, dt in sizes]
        for i, (pa, pb) in enumerate(zip(ps_a, ps_b)):
            pa.grad = None if i in idle else grads[i].clone()
            pb.grad = None if i in idle else grads[i].clone()
        clip_grad_norm_(ps_a, 1.0)
        clip_grad_norm_(live_b, 1.0)
        opt_a.step()
        opt_b.step()
        if step >= 1:
            assert opt_a._fast is not None and len(opt_a._fast["idle"]) == 2, "the fast path must hold with idle parameters"
    torch.cuda.synchronize()
    for i, (pa, pb) in enumerate(zip(ps_a, ps_b)):
        assert torch.equal(pa, pb), i
        if i not in idle:
            assert torch.equal(opt_a.state[pa]["next_m"], opt_b.state[pb]["next_m"]) and torch.equal(opt_a.state[pa]["next_v"], opt_b.state[pb]["next_v"])
            assert opt_a.state[pa]["step"] == 4
        else:
            assert len(opt_a.state[pa]) == 0                       # never stepped
    # an idle parameter gets a gradient: the plan no longer holds, the slow path steps it (its own step count starts at 0)
    for i, pa in enumerate(ps_a):
        pa.grad = (torch.randn(sizes[i][0], generator=g) * 0.5).to(sizes[i][1]).to(DEV)
    before = ps_a[1].detach().clone()
    opt_a.step()
    torch.cuda.synchronize()
    assert opt_a.state[ps_a[1]]["step"] == 1 and opt_a.state[ps_a[0]]["step"] == 5
    assert torch.equal(ps_a[1], before), "lr is 0 at step 0 of the warm-up: the first update of a late parameter moves nothing"


def _clip_skip_then_step(shared, via_optimizer_zero_grad):
    """clip, NO step (a skipped iteration), gradients dropped, new gradients (other values, version 0 again, and - the caching
    allocator being what it is - at the old addresses), step WITHOUT a clip."""
    from hmmc_amd import optimization
    from hmmc_amd.optimization import BertAdam, clip_grad_norm_
    g = torch.Generator().manual_seed(21)
    sizes = [(40000, torch.float16), (77, torch.float32), (32768, torch.float16), (100003, torch.float32)]
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dt).to(DEV)) for n, dt in sizes]
    opt = BertAdam(ps, lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=50, max_grad_norm=1.0)
    old = optimization._NO_SHARED_NORMS
    optimization._NO_SHARED_NORMS = not shared
    reused = 0
    try:
        for step in range(2):                                   # the first step plans the fast path
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=g) * 2.0).to(p.dtype).to(DEV)
            clip_grad_norm_(ps, 1.0)
            opt.step()
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 5.0).to(p.dtype).to(DEV)
        clip_grad_norm_(ps, 1.0)                                # leaves norms for a step() that never comes
        addrs = [p.grad.data_ptr() for p in ps]
        if via_optimizer_zero_grad:
            opt.zero_grad()
        else:
            for p in ps:
                p.grad = None
        for p in ps:                                            # in reverse size order the allocator hands each block back
            p.grad = (torch.randn(p.shape, generator=g) * 0.3).to(p.dtype).to(DEV)
        reused = sum(int(p.grad.data_ptr() == a and p.grad._version == 0) for p, a in zip(ps, addrs))
        opt.step()
    finally:
        optimization._NO_SHARED_NORMS = old
    torch.cuda.synchronize()
    return [t.detach().clone() for p in ps for t in (p, p.grad, opt.state[p]["next_m"], opt.state[p]["next_v"])], reused


@pytest.mark.parametrize("via_optimizer_zero_grad", [False, True])
def test_stale_clip_norms_are_not_taken_by_a_later_step(via_optimizer_zero_grad):
    """Advisor, round 4: the hand-over of per-tensor norms from `clip_grad_norm_` to `BertAdam.step()` was keyed on gradient
    address and version counter; the library's raw-pointer kernels never bump a version and the allocator returns the same
    addresses, so `clip; (no step); zero_grad(set_to_none); backward; step` passed both checks with the PREVIOUS gradients'
    norms.  The record now names the gradient tensors themselves (weak references) and is dropped by `zero_grad()` and by the
    slow path of `step()`."""
    ref, _ = _clip_skip_then_step(False, via_optimizer_zero_grad)
    got, reused = _clip_skip_then_step(True, via_optimizer_zero_grad)
    assert all(torch.equal(a, b) for a, b in zip(ref, got)), f"stale norms were used ({reused} gradient addresses were reused)"


@pytest.mark.parametrize("width,heads,L,nseq,causal", [(256, 4, 50, 48, False), (512, 8, 32, 80, True)])
def test_tower_grouped_weight_gradients_streams_and_oracle(width, heads, L, nseq, causal):
    """A tower backward with enough tokens (>= 2048) and 256-multiple widths takes the grouped weight-gradient launch
    (hmmc_gemm_f16_wgrad_group: one launch per layer on the weight-gradient stream, transient gradients alternating between
    two sets, events per layer parity).  Every gradient must be bit-identical with the second stream on and off and from run
    to run - a missing event between the chain and the grouped launch would show here - and agree with the fp32 oracle of
    the same blocks (modules/module_clip.py:231-268)."""
    from hmmc_amd import module_clip
    import hmmc_amd.functional as Fn2
    T = nseq * L
    assert T >= 2048 and width % 256 == 0
    torch.manual_seed(11)
    layers = 3
    tw = module_clip.Transformer(width, layers, heads, attn_mask="causal" if causal else None)
    for prm in tw.parameters():
        torch.nn.init.normal_(prm, std=0.04 if prm.dim() > 1 else 0.1)
    for blk in tw.resblocks:
        blk.ln_1.weight.data.add_(1.0)
        blk.ln_2.weight.data.add_(1.0)
    module_clip.convert_weights(tw)
    sd = {f"t.{k}": v.detach().float().clone().requires_grad_() for k, v in tw.state_dict().items()}
    tw = tw.to(DEV)
    x0 = (torch.randn(T, width) * 0.5).half()
    wsel = torch.randn(T, width) * 0.1

    def run(wgrad_stream):
        Fn2._WGRAD_STREAM = wgrad_stream
        for prm in tw.parameters():
            prm.grad = None
        x = x0.to(DEV).requires_grad_()
        y = tw(x, nseq, L)
        (y.float() * wsel.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), x.grad.clone(), {n: q.grad.clone() for n, q in tw.named_parameters()}

    saved = Fn2._WGRAD_STREAM
    try:
        y1, dx1, g1 = run(True)
        y2, dx2, g2 = run(True)
        y3, dx3, g3 = run(False)
    finally:
        Fn2._WGRAD_STREAM = saved
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(dx1, dx2) and torch.equal(dx1, dx3)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), f"run-to-run difference in {n}"
        assert torch.equal(g1[n], g3[n]), f"weight-gradient stream on / off difference in {n}"
    xo = x0.float().view(nseq, L, width).clone().requires_grad_()
    yo = O.transformer(xo, sd, "t", heads, O.causal_mask(L) if causal else None, torch.float32)
    (yo * wsel.view(nseq, L, width)).sum().backward()
    assert relerr(y1.cpu(), yo.detach().view(T, width)) < 5e-3
    assert relerr(dx1.cpu(), xo.grad.view(T, width)) < 2e-2
    for n in g1:
        e = relerr(g1[n].cpu(), sd["t." + n].grad)
        assert e < 2e-2, (n, e)
