"""The Chinese text branch on the GPU, everything through the C-ABI: the new kernels against their fp64 definition
(tests/bert_ref.py), the whole model against the reference's own fp32 run (tests/golden/zh_*.npz), determinism, dropout.

Kernel bound (no fixed figure): for each output the fp32 CPU restatement's own max error against fp64 on the same inputs is
measured; the kernel may err 4x that (summation order, exp / erf / tanh implementations differ) plus an absolute floor of
4 fp32 ulp of the output's largest magnitude.  Every check prints its ratio (kernel error / allowed)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bert_ref  # noqa: E402
from conftest import golden  # noqa: E402
from hmmc_amd import synth  # noqa: E402
from test_gpu_model import DEV, close, prep_optimizer  # noqa: E402
from zh_common import build as build_cpu  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


def held(what, got, ref64, ref32):
    """|got - fp64| <= 4 |fp32 restatement - fp64| + 4 ulp32 max|fp64|"""
    r64 = ref64.detach().double().cpu()
    err = float((got.detach().double().cpu() - r64).abs().max())
    own = float((ref32.detach().double().cpu() - r64).abs().max())
    lim = 4.0 * own + 4.0 * EPS32 * float(r64.abs().max())
    print(f"[zh-bound] {what}: kernel err {err:.3e}, fp32 restatement err {own:.3e}, allowed {lim:.3e}, ratio {err / max(lim, 1e-300):.3f}")
    assert err <= lim, f"{what}: kernel err {err:.3e} > allowed {lim:.3e} (fp32 restatement's own err {own:.3e})"


def rnd(name, shape, std=1.0):
    return synth.normal("zh_gpu." + name, shape, std)


def build(dims, bdims, **tc):
    return build_cpu(dims, bdims, **tc).to(DEV).train()


# ----------------------------------------------------------------------------- kernels against fp64

def test_embed_ln_fwd_bwd_vs_fp64():
    from hmmc_amd import ops
    b, L, D, vocab, P, TV = 6, 24, 128, 50, 40, 2                                    # repeated ids, L below the table length
    ids = torch.from_numpy(np.random.default_rng(0).integers(0, 12, size=(b, L)))
    W = [rnd("emb.word", (vocab, D), 0.5), rnd("emb.pos", (P, D), 0.5), rnd("emb.type", (TV, D), 0.5),
         1 + rnd("emb.g", (D,), 0.1), rnd("emb.b", (D,), 0.05)]
    dy = rnd("emb.dy", (b, L, D))

    def ref(dt):
        w = [t.detach().clone().to(dt).requires_grad_() for t in W]
        y = bert_ref.embed_ln(ids, *w)
        y.backward(dy.to(dt))
        return [y] + [t.grad for t in w]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    g = [t.to(DEV) for t in W]
    y, e, mean, rstd = ops.bert_embed_fwd(ids.to(DEV), *g, 1e-12)
    grads = ops.bert_embed_bwd(ids.to(DEV), dy.to(DEV).view(-1, D).contiguous(), e, g[3], mean, rstd, vocab, P, TV)
    for name, got, a, c in zip(("y", "dword", "dpos", "dtype", "dgamma", "dbeta"), [y.view(b, L, D)] + list(grads), r64, r32):
        held("embed " + name, got, a, c)
    assert float(grads[1][L:].abs().max()) == 0 and float(grads[2][1:].abs().max()) == 0


def test_embed_flags_ids_outside_the_table():
    from hmmc_amd import ops
    ids = torch.tensor([[1, 99]], device=DEV)
    ops.bert_embed_fwd(ids, torch.zeros(8, 64, device=DEV), torch.zeros(4, 64, device=DEV), torch.zeros(2, 64, device=DEV),
                       torch.ones(64, device=DEV), torch.zeros(64, device=DEV), 1e-12)
    with pytest.raises(IndexError):
        ops.raise_on_device_errors(DEV)


def _masks(b, L):
    m = torch.ones(b, L, dtype=torch.int64)
    for i in range(b):
        kind = i % 3
        if kind == 0:
            m[i, max(1, (L * (i + 1)) // (b + 1)):] = 0                               # a prefix
        elif kind == 1:
            m[i] = torch.from_numpy(np.random.default_rng(i).integers(0, 2, size=L))  # any pattern
            m[i, L // 2] = 1
        else:
            m[i] = 0
            m[i, (i * 7) % L] = 1                                                     # a single valid key
    return m


@pytest.mark.parametrize("L", [1, 16, 32, 45, 64, 65, 128, 256])
def test_masked_attention_fwd_bwd_vs_fp64(L):
    from hmmc_amd import ops
    b, H = 6, 2
    D = 64 * H
    qkv = rnd(f"att.qkv{L}", (b, L, 3 * D))
    dout = rnd(f"att.do{L}", (b, L, D))
    mask = _masks(b, L)

    def ref(dt):
        x = qkv.detach().clone().to(dt).requires_grad_()
        out, probs, _ = bert_ref.masked_attention(x, mask, H)
        out.backward(dout.to(dt))
        return out, probs, x.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    dead = (mask == 0)[:, :, None].expand(b, L, D)
    results = []
    for fill in (0.0, 1e30):                       # what the K / V rows of masked keys hold must not reach any output bit
        x = qkv.clone().view(b, L, 3, D)
        x[:, :, 1][dead] = fill
        x[:, :, 2][dead] = fill
        xg = x.view(b * L, 3 * D).contiguous().to(DEV)
        out, probs, _ = ops.masked_attention_fwd(xg, mask.to(DEV), b, L, H)
        dqkv = ops.masked_attention_bwd(xg, mask.to(DEV), probs, None, dout.view(b * L, D).contiguous().to(DEV), b, L, H)
        results.append((out.cpu(), probs.cpu(), dqkv.cpu()))
    for a, c in zip(*results):
        assert torch.equal(a, c), "K / V rows of masked keys changed an output bit"
    out, probs, dqkv = results[0]
    dq = dqkv.view(b, L, 3, D)
    if bool((mask == 0).any()):
        assert float(probs[(mask == 0)[:, None, None, :].expand_as(probs)].abs().max()) == 0.0
        assert float(dq[:, :, 1][dead].abs().max()) == 0.0 and float(dq[:, :, 2][dead].abs().max()) == 0.0
    held(f"attention L={L} out", out.view(b, L, D), r64[0], r32[0])
    held(f"attention L={L} probs", probs, r64[1], r32[1])
    held(f"attention L={L} dqkv", dqkv.view(b, L, 3 * D), r64[2], r32[2])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_long_masked_attention_with_dropout_vs_fp64(p):
    """The dropout instantiations of the 65..256-token kernels, forward and backward, with the keep mask recovered from the
    saved probabilities of an all-valid run at the same (seed, site)."""
    from hmmc_amd import ops
    b, L, H, seed, site = 3, 80, 1, 24680, 7
    D = 64 * H
    qkv, dout, mask = rnd("attd.qkv", (b, L, 3 * D)), rnd("attd.do", (b, L, D)), _masks(b, L)
    xg = qkv.view(b * L, 3 * D).contiguous().to(DEV)
    allv = torch.ones(b, L, dtype=torch.int64, device=DEV)
    keep = (ops.masked_attention_fwd(xg, allv, b, L, H, p, seed, site)[1] != 0).cpu()

    def ref(dt):
        x = qkv.detach().clone().to(dt).requires_grad_()
        out, probs, raw = bert_ref.masked_attention(x, mask, H, keep, p)
        out.backward(dout.to(dt))
        return out, probs, raw, x.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    out, probs, raw = ops.masked_attention_fwd(xg, mask.to(DEV), b, L, H, p, seed, site)
    dqkv = ops.masked_attention_bwd(xg, mask.to(DEV), probs, raw, dout.view(b * L, D).contiguous().to(DEV), b, L, H, p, seed, site)
    for name, got, a, c in zip(("out", "probs", "softmax", "dqkv"), (out.view(b, L, D), probs, raw, dqkv.view(b, L, 3 * D)), r64, r32):
        held(f"attention L={L} p={p} {name}", got, a, c)


def test_text_encoder_rejects_sequences_it_cannot_take():
    """L above the position table, and L above the attention kernels' 256 tokens."""
    model = build(synth.TINY, synth.ZH_TINY)                                         # 64 positions
    ids = torch.full((2, 65), 200, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="position embedding table"):
        model.text_encoder(ids, torch.ones_like(ids))
    wide = synth.BertDims(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=512,
                          max_position_embeddings=512)
    model = build(synth.TINY, wide)
    ids = torch.full((1, 257), 200, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="256 tokens"):
        model.text_encoder(ids, torch.ones_like(ids))


def test_masked_attention_rejects_more_than_256_tokens():
    from hmmc_amd import ops
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.masked_attention_fwd(torch.zeros(257, 192, device=DEV), torch.ones(1, 257, dtype=torch.int64, device=DEV), 1, 257, 1)


def test_pooler_fwd_bwd_vs_fp64():
    from hmmc_amd import ops
    b, L, D = 5, 7, 128
    x, w, bias, dy = rnd("pool.x", (b, L, D)), rnd("pool.w", (D, D), D ** -0.5), rnd("pool.b", (D,), 0.1), rnd("pool.dy", (b, D))

    def ref(dt):
        t = [v.detach().clone().to(dt).requires_grad_() for v in (x, w, bias)]
        y = bert_ref.pooler(*t)
        y.backward(dy.to(dt))
        return y, t[0].grad, t[1].grad, t[2].grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    xg = x.view(b * L, D).contiguous().to(DEV)
    y = ops.bert_pooler_fwd(xg, w.to(DEV), bias.to(DEV), b, L)
    dx = torch.zeros_like(xg)
    dW, db = ops.bert_pooler_bwd(dy.to(DEV), y, xg, w.to(DEV), b, L, dx)
    for name, got, a, c in zip(("y", "dx", "dW", "db"), (y, dx.view(b, L, D), dW, db), r64, r32):
        held("pooler " + name, got, a, c)


# ----------------------------------------------------------------------------- whole model against the reference's goldens

def _batch(g, name, bdims, dims):
    B, Fr, L = int(g["B"]), int(g["F"]), int(g["L"])
    return [t.to(DEV) for t in synth.finetune_batch_zh(B, Fr, L, bdims.vocab_size, dims.image_res, tag=name,
                                                       lens=[int(x) for x in g["lens"]])]


@pytest.mark.parametrize("name,dims,bdims", [("zh_tiny_fp32", synth.TINY, synth.ZH_TINY), ("zh_b32_fp32", synth.VIT_B32, synth.ZH_BASE)])
def test_model_vs_reference_golden(name, dims, bdims):
    """tests/test_gpu_fp32_regime.py's tolerances: features 2e-4, loss 1e-4, per-parameter gradient norms 2e-3, slices."""
    g = golden(name)
    model = build(dims, bdims, max_frames=int(g["F"]))
    ids, mask, vid, vf, idx = _batch(g, name, bdims, dims)
    q = model.text_encoder(ids, mask)
    hidden = model.text_encoder(ids, mask, return_hidden=True)
    v, u = model.visual_encoder(vid, vf)
    loss = model(ids, mask, vid, vf, idx, 1)
    loss.backward()
    close(q, g["text_feat"], 2e-4, 2e-4, "text_feat")
    close(hidden[:, :, :g["hidden"].shape[2]], g["hidden"], 2e-4, 2e-4, "hidden")
    close(u, g["frame_output"], 2e-4, 2e-4, "frame_output")
    close(v, g["video_emb"], 2e-4, 2e-4, "video_emb")
    close(loss, g["loss"], 1e-4, what="loss")
    names = [str(n) for n in g["grad_norm_names"]]
    ref = dict(zip(names, g["grad_norm_values"]))
    P = dict(model.named_parameters())
    for n in names:
        assert P[n].grad is not None and P[n].grad.dtype == torch.float32, n
        gn = float(P[n].grad.norm())
        if n.endswith("attention.self.key.bias"):
            # exactly zero in exact arithmetic (softmax ignores a per-query constant): the reference's value is rounding noise,
            # and so must this one be - below 1e-5 of the key weight's gradient norm (see tests/test_zh_cpu.py)
            wn = ref[n[:-4] + "weight"]
            assert gn <= 1e-5 * wn and ref[n] <= 1e-5 * wn, f"grad norm {n}: {gn} vs {ref[n]}"
            continue
        assert abs(gn - ref[n]) <= 2e-3 * max(ref[n], 1e-6) + 1e-7, f"grad norm {n}: {gn} vs {ref[n]}"
    for key in g.files:
        if key.startswith("g:") and "[" not in key:
            full = P[key[2:]].grad
            close(full[tuple(slice(0, s) for s in g[key].shape)], g[key], 1e-5, 2e-3, key)
    wg = P["text_encoder.chinese_encoder.embeddings.word_embeddings.weight"].grad
    close(wg[synth.ZH_CLS, :8], g["g:word_embeddings[CLS]"], 1e-6, 2e-3, "word CLS")
    close(wg[synth.ZH_SEP, :8], g["g:word_embeddings[SEP]"], 1e-6, 2e-3, "word SEP")


def test_eval_logits_1e3_identical_ranks_and_eval_similarity():
    name, dims, bdims = "zh_b32_fp32", synth.VIT_B32, synth.ZH_BASE
    g = golden(name)
    k = int(g["eval_topk"])
    model = build(dims, bdims, max_frames=int(g["F"]), top_frames=k).eval()
    ids, mask, vid, vf, idx = _batch(g, name, bdims, dims)
    with torch.no_grad():
        q = model.text_encoder(ids, mask)
        v, u = model.visual_encoder(vid, vf)
        sv, fk = model.eval_scores(q, v, u, top_frames=k)
        sim = model.eval_similarity([q[:3], q[3:]], [v[:5], v[5:]], [u[:5], u[5:]])
    close(sv, g["eval_video_logits"], 1e-3, what="x100 video logits")
    close(sv + fk, g["eval_logits"], 1e-3, what="x100 eval logits")
    close(sim, g["eval_logits"], 1e-3, what="eval_similarity")
    for got in ((sv + fk).cpu().numpy(), sim.cpu().numpy()):
        assert np.array_equal(np.argsort(-got, 1), np.argsort(-g["eval_logits"], 1)), "ranks differ"
        assert np.array_equal((got > np.diag(got)[:, None]).sum(1), g["eval_ranks"])
    assert np.array_equal(np.argsort(-sv.cpu().numpy(), 1), np.argsort(-g["eval_video_logits"], 1))


def test_train_steps_vs_reference_golden():
    from hmmc_amd.optimization import clip_grad_norm_
    from zh_names import SAMPLED, TRAIN_LENS
    g = golden("zh_train_ft_fp32")
    dims, bdims = synth.TINY, synth.ZH_TINY
    model = build(dims, bdims, lr=2e-3, text_lr=1e-3, coef_lr=0.5)
    opt = prep_optimizer(model, model.task_config, 10)
    P = dict(model.named_parameters())
    for step in range(4):
        batch = synth.finetune_batch_zh(4, 4, 16, bdims.vocab_size, tag=f"zh_train_ft.s{step}", lens=TRAIN_LENS[step])
        ids, mask, vid, vf, idx = [t.to(DEV) for t in batch]
        loss = model(ids, mask, vid, vf, idx, step + 1)
        loss.backward()
        tn = clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        close(loss, g[f"loss{step}"], 2e-3, what=f"loss{step}")
        close(tn, g[f"gnorm{step}"], 0, 5e-3, f"gnorm{step}")
        if step < 2:
            for k in SAMPLED:
                close(P[k].data.reshape(-1)[:16], g[f"p{step}:{k}"], 2e-4, 1e-3, f"p{step}:{k}")


# ----------------------------------------------------------------------------- determinism

def _step(model, batch, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    loss = model(*batch, 1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_bit_identical_across_runs_and_stream_overlap(monkeypatch):
    from hmmc_amd import modeling
    dims, bdims = synth.TINY, synth.ZH_TINY
    model = build(dims, bdims)
    batch = [t.to(DEV) for t in synth.finetune_batch_zh(4, 4, 16, bdims.vocab_size, tag="zh_det", lens=[16, 1, 9, 5])]
    a, b = _step(model, batch), _step(model, batch)
    assert _same(a, b)
    monkeypatch.setattr(modeling, "_OVERLAP_TOWERS", not modeling._OVERLAP_TOWERS)
    assert _same(a, _step(model, batch))


# ----------------------------------------------------------------------------- dropout

@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_eval_seed_and_zero(p):
    dims, bdims = synth.TINY, synth.ZH_TINY
    batch = [t.to(DEV) for t in synth.finetune_batch_zh(4, 4, 16, bdims.vocab_size, tag="zh_drop", lens=[16, 2, 9, 5])]
    plain = build(dims, bdims)
    drop = build(dims, bdims, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    with torch.no_grad():
        q0 = plain.eval().text_encoder(batch[0], batch[1])
        assert torch.equal(q0, drop.eval().text_encoder(batch[0], batch[1])), "eval mode must ignore dropout"
        assert torch.equal(q0, plain.train().text_encoder(batch[0], batch[1])), "p = 0 in train mode"
        torch.manual_seed(3)
        qa = drop.train().text_encoder(batch[0], batch[1])                  # active under no_grad too, as in HuggingFace
        torch.manual_seed(3)
        assert torch.equal(qa, drop.text_encoder(batch[0], batch[1]))
        assert not torch.equal(qa, q0)
    a, b, c = _step(drop, batch, seed=11), _step(drop, batch, seed=11), _step(drop, batch, seed=12)
    assert _same(a, b) and not torch.equal(a[0], c[0])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_fraction_and_distinct_sites(p):
    from hmmc_amd import ops
    n, seed = 1 << 20, 123456789
    ones = torch.ones(n, device=DEV)
    sd5 = 5 * (p * (1 - p) / n) ** 0.5
    masks = []
    for site in range(4):
        y = ops.dropout_fwd(ones, p, seed, site)
        keep = y != 0
        assert torch.allclose(y[keep], torch.tensor(1 / (1 - p), device=DEV))
        assert abs(float(keep.float().mean()) - (1 - p)) <= sd5, (site, float(keep.float().mean()))
        assert torch.equal(ops.dropout_bwd(ones, p, seed, site), y)
        masks.append(keep)
    b, L, H = 16, 256, 1                                                     # 16 * 256 * 256 = 2^20 probabilities
    qkv = rnd("drop.qkv", (b * L, 192)).to(DEV)
    valid = torch.ones(b, L, dtype=torch.int64, device=DEV)
    _, probs, raw = ops.masked_attention_fwd(qkv, valid, b, L, H, p, seed, 4)
    keep = (probs != 0).view(-1)
    assert float((raw == 0).float().mean()) == 0.0
    assert abs(float(keep.float().mean()) - (1 - p)) <= sd5
    masks.append(keep)
    for i in range(len(masks)):
        for j in range(i):
            assert not torch.equal(masks[i], masks[j]), (i, j)
            agree = float((masks[i] == masks[j]).float().mean())
            assert abs(agree - (p * p + (1 - p) * (1 - p))) <= 0.01, (i, j, agree)     # independent masks agree this often
    assert not torch.equal(ops.dropout_fwd(ones, p, seed + 1, 0) != 0, masks[0])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_the_definition_with_the_recovered_masks(p):
    """One BertLayer behind the embedding through hmmc_bert_fwd / hmmc_bert_bwd with dropout; the keep masks are recovered
    from kernel OUTPUTS at the same (seed, site) - elementwise: y != 0 on ones; attention: saved probabilities != 0 with
    every key valid - and fed to bert_ref in fp64.  Forward and every gradient are held to the 4x bound."""
    from hmmc_amd import functional as Fn, ops
    b, L, H, inter, seed = 3, 24, 2, 256, 987654321
    D = 64 * H
    bd = synth.BertDims(hidden_size=D, num_hidden_layers=1, num_attention_heads=H, intermediate_size=inter, vocab_size=256,
                        max_position_embeddings=32)
    cfg = dict(bd.to_config(), hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    sd = synth.bert_state(bd, seed=5)
    ids, mask = synth.zh_token_ids("zh_drop_def", b, L, bd.vocab_size, lens=[24, 3, 17])
    dout = rnd("drop.dout", (b, L, 512))
    ones = torch.ones(b * L * D, device=DEV)
    keeps = {s: (ops.dropout_fwd(ones, p, seed, s) != 0).view(b, L, D).cpu() for s in (0, 2, 3)}
    allv = torch.ones(b, L, dtype=torch.int64, device=DEV)
    keeps[1] = (ops.masked_attention_fwd(rnd("drop.q2", (b * L, 3 * D)).to(DEV), allv, b, L, H, p, seed, 1)[1] != 0).cpu()

    def ref(dt):
        w = {k: v.detach().clone().to(dt).requires_grad_() for k, v in sd.items()}
        y = bert_ref.text_encoder(w, ids, mask, cfg, want="hidden", keeps=keeps)
        y.backward(dout.to(dt))
        return y, w

    (y64, w64), (y32, w32) = ref(torch.float64), ref(torch.float32)
    model_sd = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in sd.items()}
    pre = "text_encoder.chinese_encoder."
    emb = [model_sd[pre + "embeddings." + n] for n in ("word_embeddings.weight", "position_embeddings.weight",
                                                      "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")]
    layer = bert_ref.layer_params(model_sd, "text_encoder.", 0)
    y = Fn.bert_text(ids.to(DEV), mask.to(DEV), (H, inter, 1e-12, p, p, seed), "hidden", model_sd[pre + "pooler.dense.weight"],
                     model_sd[pre + "pooler.dense.bias"], model_sd["text_encoder.text_proj.weight"],
                     model_sd["text_encoder.text_proj.bias"], *emb, *layer)
    y.backward(dout.to(DEV))
    held(f"dropout p={p} hidden", y, y64, y32)
    for k in sd:
        if "pooler" in k:
            continue
        held(f"dropout p={p} d {k[len('text_encoder.'):]}", model_sd[k].grad, w64[k].grad, w32[k].grad)


def test_p_zero_is_bit_identical_to_the_entry_path_without_dropout():
    """hmmc_bert_fwd / hmmc_bert_bwd with p = 0 (a train-mode model whose config says 0) against the same kernels called one by
    one with no dropout argument in play, forward AND backward: GEMMs with their residual epilogues, hmmc_masked_attention_*
    at p = 0, LayerNorm (its backward's column sums are the output-projection bias gradients), GELU, column sums."""
    from hmmc_amd import ops
    from hmmc_amd._lib import call, ptr
    dims, bdims = synth.TINY, synth.ZH_TINY
    model = build(dims, bdims)
    enc = model.text_encoder
    ids, mask = [t.to(DEV) for t in synth.zh_token_ids("zh_p0", 4, 16, bdims.vocab_size, lens=[16, 1, 9, 5])]
    b, L = ids.shape
    H, D = bdims.num_attention_heads, bdims.hidden_size
    dout = rnd("p0.dout", (b, L, 512)).to(DEV)
    got = enc(ids, mask, return_hidden=True)
    got.backward(dout)
    G = {n: p.grad for n, p in enc.named_parameters()}

    def colsum_ld(x, col, n, ld):                          # hmmc_colsum over columns col .. col + n of a [rows, ld] buffer
        out = torch.empty(n, dtype=torch.float32, device=DEV)
        wsb = ops.query("hmmc_colsum_workspace", x.shape[0], n)
        ws = ops.workspace(wsb, DEV, "p0")
        call("hmmc_colsum", ptr(x.view(-1)[col:]), ptr(out), x.shape[0], n, ld, 1, 1, 0, ptr(ws), wsb)
        return out

    with torch.no_grad():
        be = enc.chinese_encoder
        e = be.embeddings
        x, e_pre, e_mean, e_rstd = ops.bert_embed_fwd(ids, e.word_embeddings.weight, e.position_embeddings.weight,
                                                      e.token_type_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias, 1e-12)
        saved = []
        for lay in be.encoder.layer:
            s_, a = lay.attention.self, lay.attention.output
            qkv = torch.cat([ops.linear_f32(x, m.weight, bias=m.bias) for m in (s_.query, s_.key, s_.value)], dim=1).contiguous()
            att, probs, _ = ops.masked_attention_fwd(qkv, mask, b, L, H)
            pre1 = ops.linear_f32(att, a.dense.weight, bias=a.dense.bias, resid=x)
            x1, m1, r1 = ops.layernorm_fwd(pre1, a.LayerNorm.weight, a.LayerNorm.bias, 1e-12)
            h = ops.linear_f32(x1, lay.intermediate.dense.weight, bias=lay.intermediate.dense.bias)
            g = ops.gelu_erf_fwd(h)
            pre2 = ops.linear_f32(g, lay.output.dense.weight, bias=lay.output.dense.bias, resid=x1)
            y, m2, r2 = ops.layernorm_fwd(pre2, lay.output.LayerNorm.weight, lay.output.LayerNorm.bias, 1e-12)
            saved.append((x, qkv, probs, att, pre1, x1, m1, r1, h, g, pre2, m2, r2))
            x = y
        want = ops.linear_f32(x, enc.text_proj.weight, bias=enc.text_proj.bias).view(b, L, -1)
        assert torch.equal(got, want)
        # backward, in hmmc_bert_bwd's order of operations
        d = dout.view(b * L, -1)
        W = {"text_proj.bias": ops.colsum(d), "text_proj.weight": ops.wgrad_f32(d, x)}
        gin = ops.dgrad_f32(d, enc.text_proj.weight)
        T = b * L
        for i in reversed(range(len(saved))):
            lay = be.encoder.layer[i]
            xi, qkv, probs, att, pre1, x1, m1, r1, h, g, pre2, m2, r2 = saved[i]
            pre = f"chinese_encoder.encoder.layer.{i}."
            a, o, it = lay.attention.output, lay.output, lay.intermediate.dense
            dA, W[pre + "output.LayerNorm.weight"], W[pre + "output.LayerNorm.bias"], W[pre + "output.dense.bias"] = \
                ops.layernorm_bwd(gin, pre2, o.LayerNorm.weight, m2, r2, want_colsum=True)
            W[pre + "output.dense.weight"] = ops.wgrad_f32(dA, g)
            dh = ops.gelu_erf_bwd(h, ops.dgrad_f32(dA, o.dense.weight))
            W[pre + "intermediate.dense.bias"] = ops.colsum(dh)
            W[pre + "intermediate.dense.weight"] = ops.wgrad_f32(dh, x1)
            dC = ops.gemm_f32(dh, it.weight, T, D, it.weight.shape[0], (it.weight.shape[0], 1), (D, 1), resid=dA)
            dD, W[pre + "attention.output.LayerNorm.weight"], W[pre + "attention.output.LayerNorm.bias"], \
                W[pre + "attention.output.dense.bias"] = ops.layernorm_bwd(dC, pre1, a.LayerNorm.weight, m1, r1, want_colsum=True)
            W[pre + "attention.output.dense.weight"] = ops.wgrad_f32(dD, att)
            dqkv = ops.masked_attention_bwd(qkv, mask, probs, None, ops.dgrad_f32(dD, a.dense.weight), b, L, H)
            acc = dD
            for j, n in enumerate(("query", "key", "value")):
                w = getattr(lay.attention.self, n).weight
                W[pre + f"attention.self.{n}.bias"] = colsum_ld(dqkv, j * D, D, 3 * D)
                W[pre + f"attention.self.{n}.weight"] = ops.gemm_f32(dqkv.view(-1)[j * D:], xi, D, D, T, (1, 3 * D), (D, 1))
                acc = ops.gemm_f32(dqkv.view(-1)[j * D:], w, T, D, D, (3 * D, 1), (D, 1), resid=acc)
            gin = acc
        emb = ops.bert_embed_bwd(ids, gin, e_pre, e.LayerNorm.weight, e_mean, e_rstd, bdims.vocab_size,
                                 bdims.max_position_embeddings, bdims.type_vocab_size)
        for n, t in zip(("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight",
                         "LayerNorm.bias"), emb):
            W["chinese_encoder.embeddings." + n] = t
    assert set(W) == {n for n in G if "pooler" not in n}
    for n, t in W.items():
        assert torch.equal(G[n], t), n
    # and the dropout entry points at p = 0 pass values through bit for bit
    v = rnd("p0.v", (1024,)).to(DEV)
    assert torch.equal(ops.dropout_fwd(v, 0.0, 5, 1), v) and torch.equal(ops.dropout_bwd(v, 0.0, 5, 1), v)
