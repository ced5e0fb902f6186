"""The fp16 regime of the Chinese text encoder on the GPU (hmmc_amd/csrc/bert_f16.hip), tests/test_gpu_zh.py's method: every
output is compared with the fp64 definition (tests/bert_ref.py) on the same fp16-valued inputs, and may err 4x what the
regime's own CPU restatement (tests/bert16_ref.py: fp32 with .half() at the kernels' rounding points) errs, plus 4 fp16 ulp of
the output's largest magnitude.  Every check prints `[zh16-bound] <what> ratio` (kernel error / allowed).  Keep masks of the
dropout cases come from the existing hmmc_dropout_fwd on ones: the keep decision is a function of (seed, site, index) alone."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bert16_ref as R16  # noqa: E402
import bert_ref  # noqa: E402
from conftest import golden  # noqa: E402
from hmmc_amd import synth  # noqa: E402
from test_gpu_model import DEV, close, prep_optimizer  # noqa: E402
from zh_common import build as build_cpu  # noqa: E402

ULP16 = 2.0 ** -10


def held(what, got, ref64, ref16):
    """|got - fp64| <= 4 |fp16 restatement - fp64| + 4 ulp16 max|fp64|"""
    r64 = ref64.detach().double().cpu()
    g = got.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: not finite"
    err = float((g - r64).abs().max())
    own = float((ref16.detach().double().cpu() - r64).abs().max())
    lim = 4.0 * own + 4.0 * ULP16 * float(r64.abs().max())
    print(f"[zh16-bound] {what} ratio {err / max(lim, 1e-300):.3f} (kernel err {err:.3e}, restatement err {own:.3e}, allowed {lim:.3e})")
    assert err <= lim, f"{what}: kernel err {err:.3e} > allowed {lim:.3e} (restatement's own err {own:.3e})"


def rnd(name, shape, std=1.0):
    return synth.normal("zh16_gpu." + name, shape, std).half().float()           # fp16 values, held in fp32


def keep_mask(n, p, seed, site):
    from hmmc_amd import ops
    return (ops.dropout_fwd(torch.ones(n, device=DEV), p, seed, site) != 0).cpu()


def attn_keep(b, H, L, p, seed, site):
    return keep_mask(b * H * L * 64, p, seed, site).view(b, H, L, 64)[..., :L]


# ----------------------------------------------------------------------------- attention

def _masks(b, L):
    """all valid | a ragged tail | holes in the middle | a single valid key at a non-zero position, as far as L allows"""
    out = [torch.ones(b, L, dtype=torch.int64)]
    if L >= 2:
        tail = torch.ones(b, L, dtype=torch.int64)
        for i in range(b):
            tail[i, max(1, (L * (i + 1)) // (b + 1)):] = 0
        single = torch.zeros(b, L, dtype=torch.int64)
        for i in range(b):
            single[i, 1 + (5 * i) % (L - 1)] = 1
        out += [tail, single]
    if L >= 5:
        holes = torch.ones(b, L, dtype=torch.int64)
        for i in range(b):
            holes[i, 1 + i:L - 1:2 + i] = 0
        out.append(holes)
    return out


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("L", [1, 5, 16, 17, 45, 63, 64])
def test_masked_attention_f16_fwd_bwd_vs_fp64(L, p):
    from hmmc_amd import ops
    b, H, seed, site = 3, 2, 13579, 4
    D = 64 * H
    qkv, dout = rnd(f"att.qkv{L}", (b, L, 3 * D)), rnd(f"att.do{L}", (b, L, D))
    keep = attn_keep(b, H, L, p, seed, site) if p > 0 else None
    for mi, mask in enumerate(_masks(b, L)):
        x64 = qkv.double().requires_grad_()
        o64, _, _ = bert_ref.masked_attention(x64, mask, H, keep, p)
        o64.backward(dout.double())
        o16, _ = R16.attention_fwd(qkv, mask, H, keep, p)
        d16 = R16.attention_bwd(qkv, mask, H, dout, keep, p)
        dead = (mask == 0)[:, :, None].expand(b, L, D)
        x = qkv.clone().view(b, L, 3, D)
        x[:, :, 1][dead] = float("nan")                                           # masked K / V rows must never be used
        x[:, :, 2][dead] = float("nan")
        xg = x.view(b * L, 3 * D).half().to(DEV)
        dg = dout.view(b * L, D).half().to(DEV)
        out, lse = ops.masked_attention_f16_fwd(xg, mask.to(DEV), b, L, H, p, seed, site)
        dqkv, dbias = ops.masked_attention_f16_bwd(xg, mask.to(DEV), lse, dg, b, L, H, p, seed, site, want_dbias=True)
        out2, lse2 = ops.masked_attention_f16_fwd(xg, mask.to(DEV), b, L, H, p, seed, site)
        dqkv2 = ops.masked_attention_f16_bwd(xg, mask.to(DEV), lse2, dg, b, L, H, p, seed, site)
        assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2), "two launches differ"
        assert bool(torch.isfinite(lse).all())
        dq = dqkv.view(b, L, 3, D).cpu()
        if bool(dead.any()):
            assert float(dq[:, :, 1][dead].abs().max()) == 0.0 and float(dq[:, :, 2][dead].abs().max()) == 0.0
        what = f"attention L={L} p={p} mask{mi}"
        held(what + " out", out.view(b, L, D), o64, o16)
        held(what + " dqkv", dqkv.view(b, L, 3 * D), x64.grad, d16)
        held(what + " dbias", dbias, x64.grad.sum(1), d16.sum(1))


def test_masked_attention_f16_rejects_more_than_64_tokens():
    from hmmc_amd import ops
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.masked_attention_f16_fwd(torch.zeros(65, 192, dtype=torch.float16, device=DEV),
                                     torch.ones(1, 65, dtype=torch.int64, device=DEV), 1, 65, 1)


# ----------------------------------------------------------------------------- GELU, dropout, pooler

@pytest.mark.parametrize("n", [8, 8 * 257, 1 << 16])
def test_gelu_and_dropout_f16_vs_fp64(n):
    from hmmc_amd import ops
    x, dy, res = rnd(f"el.x{n}", (n,), 2.0), rnd(f"el.dy{n}", (n,)), rnd(f"el.r{n}", (n,))
    x[:3] = torch.tensor([6.0, -6.0, 0.0])
    xg, dg, rg = x.half().to(DEV), dy.half().to(DEV), res.half().to(DEV)
    x64 = x.double().requires_grad_()
    y64 = torch.nn.functional.gelu(x64)
    y64.backward(dy.double())
    held(f"gelu n={n} y", ops.gelu_erf_f16_fwd(xg), y64, R16.gelu_fwd(x))
    held(f"gelu n={n} dx", ops.gelu_erf_f16_bwd(xg, dg), x64.grad, R16.gelu_bwd(x, dy))
    assert torch.equal(ops.dropout_f16_fwd(xg, 0.0, 5, 1), xg) and torch.equal(ops.dropout_f16_bwd(dg, 0.0, 5, 1), dg)
    held(f"dropout n={n} p=0 +resid", ops.dropout_f16_fwd(xg, 0.0, 5, 1, resid=rg), x.double() + res.double(), R16.r(x + res))
    for p in (0.1, 0.5):
        keep = keep_mask(n, p, 777, 3)
        y64 = bert_ref.dropout(x.double(), keep, p)
        held(f"dropout n={n} p={p} y", ops.dropout_f16_fwd(xg, p, 777, 3), y64, R16.dropout_fwd(x, keep, p))
        held(f"dropout n={n} p={p} y+resid", ops.dropout_f16_fwd(xg, p, 777, 3, resid=rg), y64 + res.double(),
             R16.dropout_fwd(x, keep, p, res))
        held(f"dropout n={n} p={p} dx", ops.dropout_f16_bwd(dg, p, 777, 3), bert_ref.dropout(dy.double(), keep, p),
             R16.dropout_bwd(dy, keep, p))
        alias = xg.clone()
        assert torch.equal(ops.dropout_f16_fwd(alias, p, 777, 3, out=alias), ops.dropout_f16_fwd(xg, p, 777, 3)), "y aliasing x"


@pytest.mark.parametrize("b", [1, 4])
def test_pooler_f16_fwd_bwd_vs_fp64(b):
    from hmmc_amd import ops
    L, D = 16, 128
    x, w, bias, dy = rnd("pool.x", (b, L, D)), rnd("pool.w", (D, D), D ** -0.5), rnd("pool.b", (D,), 0.1), rnd("pool.dy", (b, D))
    t = [v.double().requires_grad_() for v in (x, w, bias)]
    y64 = bert_ref.pooler(*t)
    y64.backward(dy.double())
    y16 = R16.pooler_fwd(x, w, bias)
    dx16, dW16, db16 = R16.pooler_bwd(dy, y16, x, w)
    xg = x.view(b * L, D).half().to(DEV)
    y = ops.bert_pooler_f16_fwd(xg, w.half().to(DEV), bias.half().to(DEV), b, L)
    dx = torch.full_like(xg, 7.0)                                                   # sentinel: only the class rows may change
    dW, db = ops.bert_pooler_f16_bwd(dy.half().to(DEV), y, xg, w.half().to(DEV), b, L, dx)
    dx = dx.view(b, L, D)
    assert bool((dx[:, 1:] == 7.0).all()), "a row other than the class rows changed"
    held(f"pooler b={b} y", y, y64, y16)
    held(f"pooler b={b} dx", dx[:, 0], t[0].grad[:, 0], dx16)
    held(f"pooler b={b} dW", dW, t[1].grad, dW16)
    held(f"pooler b={b} db", db, t[2].grad, db16)


# ----------------------------------------------------------------------------- tower

PRE = "text_encoder."
LENS = [16, 1, 9, 5]


def _tower_params(sd, fp16=True):
    """GPU leaves in the converted layout (fp16 = False: all fp32) + the argument list of functional.bert_text"""
    half = {k for k in sd if fp16 and not ("embeddings." in k or "LayerNorm." in k)}
    g = {k: (v.half() if k in half else v.clone()).to(DEV).requires_grad_() for k, v in sd.items()}
    e = PRE + "chinese_encoder.embeddings."
    emb = [g[e + n] for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                              "LayerNorm.weight", "LayerNorm.bias")]
    layers = [t for i in range(synth.ZH_TINY.num_hidden_layers) for t in bert_ref.layer_params(g, PRE, i)]
    head = [g[PRE + "chinese_encoder.pooler.dense.weight"], g[PRE + "chinese_encoder.pooler.dense.bias"], g[PRE + "text_proj.weight"],
            g[PRE + "text_proj.bias"]]
    return g, head + emb + layers


def _keeps(b, L, D, H, nl, p, seed):
    if p == 0:
        return None
    k = {0: keep_mask(b * L * D, p, seed, 0).view(b, L, D)}
    for i in range(nl):
        k[1 + 3 * i] = attn_keep(b, H, L, p, seed, 1 + 3 * i)
        k[2 + 3 * i] = keep_mask(b * L * D, p, seed, 2 + 3 * i).view(b, L, D)
        k[3 + 3 * i] = keep_mask(b * L * D, p, seed, 3 + 3 * i).view(b, L, D)
    return k


def _noise(n):
    """attention.self.key.bias gradients are exactly zero in exact arithmetic: rounding noise only"""
    return n.endswith("attention.self.key.bias")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("want", ["feat", "hidden"])
def test_tower_fwd_bwd_vs_fp64(want, p):
    from hmmc_amd import functional as Fn
    bd = synth.ZH_TINY
    b, L, H, D, seed = 4, 16, bd.num_attention_heads, bd.hidden_size, 24680
    cfg = dict(bd.to_config(), hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    sd = R16.convert_state(synth.bert_state(bd, seed=5))
    ids, mask = synth.zh_token_ids("zh16_tower", b, L, bd.vocab_size, lens=LENS)
    dout = rnd("tower.dout", (b, L, 512) if want == "hidden" else (b, 512))
    keeps = _keeps(b, L, D, H, bd.num_hidden_layers, p, seed)
    w64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    y64 = bert_ref.text_encoder(w64, ids, mask, cfg, want=want, keeps=keeps)
    y64.backward(dout.double())
    y16, g16 = R16.text_encoder(sd, ids, mask, cfg, dout, want=want, keeps=keeps)
    g, args = _tower_params(sd)
    call_cfg = (H, bd.intermediate_size, 1e-12, p, p, seed)
    y = Fn.bert_text(ids.to(DEV), mask.to(DEV), call_cfg, want, *args)
    assert y.dtype == torch.float32
    y.backward(dout.to(DEV))
    with torch.no_grad():
        assert torch.equal(Fn.bert_text(ids.to(DEV), mask.to(DEV), call_cfg, want, *args), y), "keep_acts = 0 output differs"
    held(f"tower {want} p={p} out", y, y64, y16)
    for k in sd:
        if _noise(k) or (want == "hidden" and "pooler" in k):
            continue
        assert g[k].grad.dtype == g[k].dtype, k
        held(f"tower {want} p={p} d {k[len(PRE):]}", g[k].grad, w64[k].grad, g16[k])


@pytest.mark.parametrize("L", [7, 64])
@pytest.mark.parametrize("regime", ["fp32", "fp16"])
def test_reused_slab_equals_kept_slabs_and_the_backward_repeats(regime, L):
    """The slab aliasing of the one tower runtime (csrc/bert_tower.hip), both regimes, with dropout at every site: a pass that
    keeps no activations (every layer in ONE slab, its output in the slab's own input slot) returns the bits of a pass that keeps
    one slab per layer, and a second forward + backward through freshly kept activations reproduces every gradient bit for bit.
    (test_tower_fwd_bwd_vs_fp64 asserts the first half for fp16 at L = 16 on its way.)"""
    from hmmc_amd import functional as Fn
    bd = synth.ZH_TINY
    b, p, seed = 3, 0.1, 97531
    sd = synth.bert_state(bd, seed=5)
    ids, mask = [t.to(DEV) for t in synth.zh_token_ids("zh_slab", b, L, bd.vocab_size, lens=[L, 1, max(2, 2 * L // 3)])]
    cfg = (bd.num_attention_heads, bd.intermediate_size, 1e-12, p, p, seed)
    for want in ("feat", "hidden"):
        dout = rnd(f"slab.dout.{want}", (b, L, 512) if want == "hidden" else (b, 512)).to(DEV)

        def kept():
            g, args = _tower_params(sd, fp16=regime == "fp16")
            y = Fn.bert_text(ids, mask, cfg, want, *args)
            y.backward(dout)
            return y.detach(), {k: v.grad for k, v in g.items() if v.grad is not None}, args

        y1, g1, args = kept()
        y2, g2, _ = kept()
        with torch.no_grad():
            y0 = Fn.bert_text(ids, mask, cfg, want, *args)
        assert bool(torch.isfinite(y1).all()) and len(g1) >= len(sd) - 2
        assert torch.equal(y0, y1), f"{regime} {want} L={L}: the one reused slab and the kept slabs differ"
        assert torch.equal(y1, y2) and g1.keys() == g2.keys()
        for k in g1:
            assert torch.equal(g1[k], g2[k]), f"{regime} {want} L={L}: d {k} differs between two backwards"


def test_merged_encode_many_pass_vs_fp64_sum_of_separate_passes():
    from hmmc_amd import functional as Fn
    bd = synth.ZH_TINY
    H = bd.num_attention_heads
    cfg = bd.to_config()
    sd = R16.convert_state(synth.bert_state(bd, seed=5))
    parts = [("feat", 3, 16, [16, 2, 7]), ("hidden", 3, 16, [9, 16, 1]), ("feat", 2, 9, [9, 4])]
    inputs = [synth.zh_token_ids(f"zh16_many{i}", b, L, bd.vocab_size, lens=lens) for i, (_, b, L, lens) in enumerate(parts)]
    douts = [rnd(f"many.dout{i}", (b, L, 512) if want == "hidden" else (b, 512)) for i, (want, b, L, _) in enumerate(parts)]
    w64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    g16 = {}
    y64s, y16s = [], []
    for (want, _, _, _), (ids, mask), dout in zip(parts, inputs, douts):
        y64 = bert_ref.text_encoder(w64, ids, mask, cfg, want=want)
        y64.backward(dout.double())                                               # fp64 gradients accumulate: the sum
        y16, gi = R16.text_encoder(sd, ids, mask, cfg, dout, want=want)
        for k, v in gi.items():
            g16[k] = v if k not in g16 else g16[k] + v
        y64s.append(y64)
        y16s.append(y16)
    g, args = _tower_params(sd)
    Lmax = 16
    pad = torch.nn.functional.pad
    ids = torch.cat([pad(i, (0, Lmax - i.shape[1])) for i, _ in inputs]).to(DEV)
    mask = torch.cat([pad(m, (0, Lmax - m.shape[1])) for _, m in inputs]).to(DEV)
    segs, row0 = [], 0
    for want, b, _, _ in parts:
        segs.append((row0, b, want))
        row0 += b
    outs = Fn.bert_text_many(ids, mask, (H, bd.intermediate_size, 1e-12, 0.0, 0.0, 0), segs, *args)
    torch.autograd.backward(list(outs), [d.to(DEV) for d in douts])
    for i, (o, y64, y16) in enumerate(zip(outs, y64s, y16s)):
        held(f"merged out{i}", o, y64, y16)
    for k in sd:
        if not _noise(k):
            held(f"merged d {k[len(PRE):]}", g[k].grad, w64[k].grad, g16[k])


# ----------------------------------------------------------------------------- model

def _converted(**tc):
    from hmmc_amd.module_cross import convert_bert_weights
    model = build_cpu(synth.TINY, synth.ZH_TINY, **tc).to(DEV).train()
    convert_bert_weights(model.text_encoder)
    return model


def test_model_step_in_the_fp16_regime_and_the_fp32_regime_beside_it():
    g = golden("zh_tiny_fp32")
    dims, bdims = synth.TINY, synth.ZH_TINY
    batch = [t.to(DEV) for t in synth.finetune_batch_zh(int(g["B"]), int(g["F"]), int(g["L"]), bdims.vocab_size, dims.image_res,
                                                        tag="zh_tiny_fp32", lens=[int(x) for x in g["lens"]])]
    model = _converted(max_frames=int(g["F"]))
    ids, mask = batch[0], batch[1]
    # text features against fp64 / the restatement on the converted weights
    cfg = json.loads(str(g["bert"]))
    sd = R16.convert_state(synth.bert_state(bdims))
    with torch.no_grad():
        q64 = bert_ref.text_encoder({k: v.double() for k, v in sd.items()}, ids.cpu(), mask.cpu(), cfg, want="feat")
    q16, _ = R16.text_encoder(sd, ids.cpu(), mask.cpu(), cfg, torch.zeros(q64.shape), want="feat")
    with torch.no_grad():
        q = model.text_encoder(ids, mask)
    assert q.dtype == torch.float32
    held("model text_feat", q, q64, q16)
    loss = model(*batch, 1)
    loss.backward()
    assert bool(torch.isfinite(loss))
    opt = prep_optimizer(model, model.task_config, 10)
    opt.step()
    for n, prm in model.named_parameters():
        assert bool(torch.isfinite(prm).all()), n
        assert prm.grad is None or prm.grad.dtype == prm.dtype, n
    lin = model.text_encoder.chinese_encoder.encoder.layer[0].intermediate.dense.weight
    st = opt.state[lin]
    assert lin.dtype == torch.float16 and st["next_m"].dtype == torch.float16 and st["next_v"].dtype == torch.float16
    model.eval()
    with torch.no_grad():
        qe = model.text_encoder(ids, mask)
        v, u = model.visual_encoder(batch[2], batch[3])
        sim = model.eval_similarity([qe], [v], [u])
    assert bool(torch.isfinite(sim).all())
    # an fp32-regime model in the same process still reproduces the reference's run: the dispatch did not leak
    plain = build_cpu(dims, bdims, max_frames=int(g["F"])).to(DEV).train()
    close(plain.text_encoder(ids, mask), g["text_feat"], 2e-4, 2e-4, "fp32 text_feat")
    close(plain(*batch, 1), g["loss"], 1e-4, what="fp32 loss")


def test_model_loss_and_text_gradients_vs_fp64_composed_with_the_oracles_head():
    """BirdModel(language="chinese") after convert_bert_weights, through the model's own forward and backward: the loss and
    every text-side gradient against bert_ref in fp64 / bert16_ref, each composed with the oracle's fine-tune head on the
    video features the model itself produced (the visual side is fp32 and not under test here)."""
    from oracle import hmmc_oracle as O
    g = golden("zh_tiny_fp32")
    dims, bdims = synth.TINY, synth.ZH_TINY
    batch = [t.to(DEV) for t in synth.finetune_batch_zh(int(g["B"]), int(g["F"]), int(g["L"]), bdims.vocab_size, dims.image_res,
                                                        tag="zh_tiny_fp32", lens=[int(x) for x in g["lens"]])]
    model = _converted(max_frames=int(g["F"]))
    ids, mask = batch[0].cpu(), batch[1].cpu()
    loss = model(*batch, 1)
    loss.backward()
    with torch.no_grad():
        v, u = [t.cpu() for t in model.visual_encoder(batch[2], batch[3])]
    cfg = json.loads(str(g["bert"]))
    sd = R16.convert_state(synth.bert_state(bdims))
    w64 = {k: t.double().requires_grad_() for k, t in sd.items()}
    l64 = O.finetune_head(bert_ref.text_encoder(w64, ids, mask, cfg, want="feat"), v.double(), u.double())
    l64.backward()
    q16, _ = R16.text_encoder(sd, ids, mask, cfg, torch.zeros(ids.shape[0], 512), want="feat")
    q16 = q16.detach().requires_grad_()
    l16 = O.finetune_head(q16, v.float(), u.float())
    l16.backward()
    _, g16 = R16.text_encoder(sd, ids, mask, cfg, q16.grad, want="feat")
    held("model loss", loss, l64, l16)
    P = dict(model.named_parameters())
    for k in sd:
        if _noise(k):
            continue
        assert P[k].grad is not None and P[k].grad.dtype == P[k].dtype, k
        held(f"model d {k[len(PRE):]}", P[k].grad, w64[k].grad, g16[k])


def test_text_encoder_rejects_more_than_64_tokens_in_fp16_and_other_layouts():
    from hmmc_amd.module_cross import convert_bert_weights
    wide = synth.BertDims(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=512,
                          max_position_embeddings=128)
    model = build_cpu(synth.TINY, wide).to(DEV)
    ids = torch.full((1, 65), 200, dtype=torch.int64, device=DEV)
    assert model.text_encoder(ids, torch.ones_like(ids)).shape == (1, 512)         # fp32 takes it
    convert_bert_weights(model.text_encoder)
    with pytest.raises(ValueError, match="at most 64 tokens in the fp16 regime"):
        model.text_encoder(ids, torch.ones_like(ids))
    with pytest.raises(ValueError, match="at most 64 tokens in the fp16 regime"):
        model.text_encoder.encode_many([ids], ["feat"], [torch.ones_like(ids)])
    model.text_encoder.chinese_encoder.embeddings.LayerNorm.half()
    with pytest.raises(TypeError, match="convert_bert_weights"):
        model.text_encoder(ids[:, :8], torch.ones_like(ids[:, :8]))


def test_pretraining_step_with_both_encoders_converted_and_a_mismatch_refused():
    import zh_pretrain_ref as ZR
    from hmmc_amd.module_cross import convert_bert_weights
    from hmmc_amd.optimization import clip_grad_norm_
    dims, bdims = synth.TINY, synth.ZH_TINY
    model = ZR.build(dims, bdims, lr=2e-3, text_lr=1e-3, coef_lr=0.5, weight_decay=0.05).to(DEV).train()
    batch = [t.to(DEV) for t in synth.pretrain_batch_zh(4, 4, bdims.vocab_size, 16, 9, tag="zh16_pt", title_lens=[16, 1, 9, 5],
                                                         tag_lens=[9, 2, 5, 3])]
    convert_bert_weights(model.text_encoder)
    with pytest.raises(TypeError, match="text_encoder_k"):
        model(*batch, 1)
    convert_bert_weights(model.text_encoder_k)
    opt = prep_optimizer(model, model.task_config, 50)
    half_k = {n: t for n, t in model.text_encoder_k.named_parameters() if t.dtype == torch.float16}
    half_q = {n: t for n, t in model.text_encoder.named_parameters() if t.dtype == torch.float16}
    assert half_k and half_k.keys() == half_q.keys()

    def step(i):
        torch.manual_seed(50 + i)
        loss = model(*batch, i + 1)
        loss.backward()
        clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        assert bool(torch.isfinite(loss)), i

    step(0)
    # the EMA runs inside the next forward, before the optimizer touches the online weights: with the online fp16 weights moved
    # far enough from the key ones for the increment to exceed an fp16 ulp, every key tensor must become
    # fp16(m k + (1 - m) q), within one fp16 ulp of it (the kernel may fuse the two products)
    with torch.no_grad():
        for t in half_q.values():
            t.mul_(1.5)
    m = float(model.contrast_momentum)
    before = {n: t.detach().clone() for n, t in half_k.items()}
    want = {n: (before[n].float() * m + half_q[n].detach().float() * (1.0 - m)).half() for n in half_k}
    step(1)
    for n, t in half_k.items():
        assert t.dtype == torch.float16 and bool(torch.isfinite(t).all()), n
        err = (t.float() - want[n].float()).abs()
        assert bool((err <= ULP16 * want[n].float().abs() + 2.0 ** -24).all()), f"{n}: not the fp16 EMA (max err {float(err.max()):.3e})"
        assert torch.equal(want[n], before[n]) or not torch.equal(t, before[n]), f"{n} did not move"
    assert any(not torch.equal(t, before[n]) for n, t in half_k.items()), "no fp16 tensor of text_encoder_k moved by the EMA"
