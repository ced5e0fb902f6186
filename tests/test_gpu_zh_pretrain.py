"""Pre-training with the Chinese text branch on the GPU: hmmc_mlm_mask against the torch statement of mask() (exact), the masked
multi-input pass of the BERT tower against fp64 and against separate passes, the MLM head at BERT vocabularies, and the whole
step against the reference's own fp32 runs (tests/golden/moco_zh*_fp32.npz) and the CPU restatement tests/zh_pretrain_ref.py.

Kernel bound: tests/test_gpu_zh.py's - 4 x the fp32 CPU restatement's own error against fp64 + 4 fp32 ulp of the largest
magnitude; model tolerances: those of tests/test_gpu_fp32_regime.py::test_fp32_pretrain_*_vs_reference_golden."""
import io
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bert_ref  # noqa: E402
import zh_pretrain_ref as R  # noqa: E402
from conftest import golden  # noqa: E402
from hmmc_amd import functional as Fn  # noqa: E402
from hmmc_amd import ops, synth  # noqa: E402
from oracle import hmmc_oracle as O  # noqa: E402
from test_gpu_model import DEV, close, prep_optimizer  # noqa: E402
from test_gpu_zh import EPS32, held  # noqa: E402
from zh_common import build as build_finetune  # noqa: E402

CLIP_IDS, BERT_IDS = (49407, 49406, 49394, 49408), (0, 101, 103, 21128)          # pad, cls, mask, vocabulary


# ----------------------------------------------------------------------------- hmmc_mlm_mask

@pytest.mark.parametrize("consts", [CLIP_IDS, BERT_IDS], ids=["clip", "bert"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (4, 45), (128, 45)])
def test_mlm_mask_kernel_equals_the_torch_statement(shape, consts):
    pad, cls, mask_id, vocab = consts
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    n = shape[0] * shape[1]
    ids = torch.from_numpy(rng.integers(0, vocab, size=shape))
    ids.view(-1)[rng.integers(0, n, size=max(1, n // 5))] = pad
    ids.view(-1)[rng.integers(0, n, size=max(1, n // 7))] = cls                     # [CLS] anywhere, not only in front
    ids[-1] = pad                                                                   # a row that is all [PAD]
    ids[0, 0] = cls
    random = [torch.from_numpy(rng.integers(0, 2, size=shape)) for _ in range(3)] + [torch.from_numpy(rng.integers(0, vocab, size=shape))]
    ones, zeros = torch.ones(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.int64)
    for name, draws in (("random", random), ("all ones", [ones, ones, ones, random[3]]), ("all zeros", [zeros, zeros, zeros, random[3]]),
                        ("never replaced", [ones, zeros, ones, random[3]]), ("kept", [ones, zeros, zeros, random[3]])):
        want_ids, want_labels = R.apply_mask(ids, draws, pad, cls, mask_id)
        dev = [d.bool().to(DEV) if i < 3 else d.to(DEV) for i, d in enumerate(draws)]
        got_ids, got_labels = ids.clone().to(DEV), torch.full(shape, 7, dtype=torch.int64, device=DEV)
        ops.mlm_mask_(got_ids, *dev, pad, cls, mask_id, labels=got_labels)
        assert torch.equal(got_ids.cpu(), want_ids) and torch.equal(got_labels.cpu(), want_labels), name
        only_ids = ids.clone().to(DEV)
        ops.mlm_mask_(only_ids, *dev, pad, cls, mask_id, labels=None)               # labels_out = NULL
        assert torch.equal(only_ids.cpu(), want_ids), name + " (no labels)"
    if shape == (4, 45):                                                            # mask() itself: in place, both return forms
        model = R.build(synth.TINY, synth.ZH_TINY)
        model.PAD_ID, model.CLS_ID, model.MASK_ID = pad, cls, mask_id
        model._mlm_draws = random
        a, lab = ids.clone().to(DEV), ids.clone().to(DEV)
        out = model.mask(a, vocab, DEV, targets=lab)
        want_ids, want_labels = R.apply_mask(ids, random, pad, cls, mask_id)
        assert out[0] is a and out[1] is lab and torch.equal(a.cpu(), want_ids) and torch.equal(lab.cpu(), want_labels)
        b = ids.clone().to(DEV)
        assert model.mask(b, vocab, DEV) is b and torch.equal(b.cpu(), want_ids)


# ----------------------------------------------------------------------------- the masked multi-input pass

def _limit(r64, r32):
    return 4.0 * float((r32.double() - r64).abs().max()) + 4.0 * EPS32 * float(r64.abs().max())


def test_encode_many_vs_fp64_and_vs_separate_passes():
    """(3 x 16 feat), (3 x 16 hidden), (2 x 9 feat) with ragged masks through ONE pass: every output and every parameter
    gradient against the fp64 restatement, and the merged pass's gradients against the sum of three separate passes'."""
    dims, bdims = synth.TINY, synth.ZH_TINY
    enc = build_finetune(dims, bdims).to(DEV).train().text_encoder
    cfg = bdims.to_config()
    texts = [synth.zh_token_ids("zh_many.a", 3, 16, bdims.vocab_size, lens=[16, 1, 9]),
             synth.zh_token_ids("zh_many.b", 3, 16, bdims.vocab_size, lens=[5, 16, 2]),
             synth.zh_token_ids("zh_many.c", 2, 9, bdims.vocab_size, lens=[9, 4])]
    wants = ["feat", "hidden", "feat"]
    ws = [synth.normal("zh_many.w0", (3, 512)), synth.normal("zh_many.w1", (3, 16, 512)), synth.normal("zh_many.w2", (2, 512))]
    src = synth.bert_state(bdims)

    def ref(dt):
        w = {k: v.detach().clone().to(dt).requires_grad_() for k, v in src.items()}
        outs = [bert_ref.text_encoder(w, ids, mask, cfg, want=want) for (ids, mask), want in zip(texts, wants)]
        sum((o * x.to(dt)).sum() for o, x in zip(outs, ws)).backward()
        return outs, {k: v.grad for k, v in w.items()}

    (o64, g64), (o32, g32) = ref(torch.float64), ref(torch.float32)
    P = {"text_encoder." + n: p for n, p in enc.named_parameters()}
    assert set(P) == set(src)

    def run(merged):
        for p in P.values():
            p.grad = None
        dev = [(i.to(DEV), m.to(DEV)) for i, m in texts]
        if merged:
            outs = enc.encode_many([i for i, _ in dev], wants, masks=[m for _, m in dev])
        else:
            outs = [enc(i, m, return_hidden=want == "hidden") for (i, m), want in zip(dev, wants)]
        sum((o * x.to(DEV)).sum() for o, x in zip(outs, ws)).backward()
        return outs, {k: p.grad.clone() for k, p in P.items()}

    om, gm = run(True)
    osep, gsep = run(False)
    for i, want in enumerate(wants):
        assert om[i].shape == o64[i].shape
        held(f"encode_many out {i} ({want})", om[i], o64[i], o32[i])
    for k in src:
        if k.endswith("attention.self.key.bias"):
            # exactly zero in exact arithmetic (softmax ignores a per-query constant): every side holds rounding noise, which
            # has no common value; it must BE noise - below 1e-5 of the key weight's gradient norm (tests/test_zh_cpu.py)
            wn = float(g64[k[:-4] + "weight"].norm())
            assert float(gm[k].norm()) <= 1e-5 * wn, k
            continue
        held("encode_many d " + k[len("text_encoder."):], gm[k], g64[k], g32[k])
        lim = _limit(g64[k].double(), g32[k])
        err = float((gm[k] - gsep[k]).double().abs().max())
        print(f"[zh-bound] merged vs separate d {k[len('text_encoder.'):]}: diff {err:.3e}, allowed {lim:.3e}, ratio {err / max(lim, 1e-300):.3f}")
        assert err <= lim, f"merged vs separate passes, {k}: {err:.3e} > {lim:.3e}"


def test_padded_positions_of_a_hidden_segment_reach_no_gradient_and_no_output_bit():
    """A 2 x 9 "hidden" input beside a 3 x 16 "feat" input is padded to 16 with TextEncoder.pad_id.  No input holds that id
    here (every sequence is full), so it occurs at the padded positions ALONE: its word-embedding gradient row must be exactly
    zero - the backward's assembled dy is zero there, the positions are masked as keys, and everything else is per token - and
    a different pad id must change no bit of any output or of any other gradient."""
    dims, bdims = synth.TINY, synth.ZH_TINY
    enc = build_finetune(dims, bdims).to(DEV).train().text_encoder
    a, am = [t.to(DEV) for t in synth.zh_token_ids("zh_pad.a", 3, 16, bdims.vocab_size, lens=[16, 16, 16])]
    b, bm = [t.to(DEV) for t in synth.zh_token_ids("zh_pad.b", 2, 9, bdims.vocab_size, lens=[9, 9])]
    w = synth.normal("zh_pad.w", (2, 9, 512)).to(DEV)
    word = enc.chinese_encoder.embeddings.word_embeddings.weight

    def run(pad):
        assert not bool((a == pad).any()) and not bool((b == pad).any())
        enc.pad_id = pad
        enc.zero_grad(set_to_none=True)
        feat, hid = enc.encode_many([a, b], ["feat", "hidden"], masks=[am, bm])
        assert tuple(feat.shape) == (3, 512) and tuple(hid.shape) == (2, 9, 512)
        ((hid * w).sum() + feat.sum()).backward()
        return feat.detach(), hid.detach(), {n: p.grad.clone() for n, p in enc.named_parameters()}

    f1, h1, g1 = run(77)
    f2, h2, g2 = run(5)
    name = "chinese_encoder.embeddings.word_embeddings.weight"
    assert float(g1[name][77].abs().max()) == 0.0 and float(g2[name][5].abs().max()) == 0.0, "gradient reached a padded position"
    assert float(g1[name][int(b[0, 3])].abs().max()) > 0.0 and word.grad is not None
    assert torch.equal(f1, f2) and torch.equal(h1, h2), "the padding's content changed an output bit"
    for n in g1:
        assert torch.equal(g1[n], g2[n]), f"the padding's content changed a bit of d {n}"


# ----------------------------------------------------------------------------- the MLM head at BERT vocabularies

@pytest.mark.parametrize("V", [21128, 2048])
def test_mlm_head_fn_at_bert_vocabularies_vs_fp64(V):
    """tests/test_gpu_pretrain.py::test_mlm_head_fn_vs_oracle's tolerances, the reference in fp64."""
    e = 512
    sd = {"cls.bias": synth.normal("zh_mlm.bias", (V,), 0.02), "cls.transform.dense.weight": synth.normal("zh_mlm.dw", (e, e), e ** -0.5),
          "cls.transform.dense.bias": synth.normal("zh_mlm.db", (e,), 0.02),
          "cls.transform.LayerNorm.weight": synth.normal("zh_mlm.lw", (e,), 0.1, 1.0),
          "cls.transform.LayerNorm.bias": synth.normal("zh_mlm.lb", (e,), 0.05), "cls.decoder.weight": synth.normal("zh_mlm.dec", (V, e), 0.02)}
    hidden = synth.normal("zh_mlm.hidden", (3, 20, 512), 0.5)
    labels = torch.full((3, 20), -100, dtype=torch.long)
    labels[0, 3], labels[1, 7], labels[2, 19], labels[2, 1], labels[0, 0] = 0, V - 1, V // 2, 5, 103
    ho = hidden.double().requires_grad_()
    sdo = {k: v.double().requires_grad_() for k, v in sd.items()}
    scores = O.mlm_head(ho, sdo)
    ref = torch.nn.functional.cross_entropy(scores.view(-1, V), labels.view(-1), ignore_index=-100)
    ref.backward()
    hg = hidden.to(DEV).requires_grad_()
    P = {k: v.clone().to(DEV).requires_grad_() for k, v in sd.items()}
    loss = Fn.MlmHeadFn.apply(hg, labels.to(DEV), P["cls.transform.dense.weight"], P["cls.transform.dense.bias"],
                              P["cls.transform.LayerNorm.weight"], P["cls.transform.LayerNorm.bias"], P["cls.decoder.weight"], P["cls.bias"])
    loss.backward()
    close(loss, ref, 1e-5, 1e-5, "mlm loss")
    close(hg.grad, ho.grad, 1e-6, 2e-3, "dhidden")
    close(P["cls.decoder.weight"].grad, sdo["cls.decoder.weight"].grad, 1e-6, 2e-3, "ddecoder")
    close(P["cls.bias"].grad, sdo["cls.bias"].grad, 1e-6, 2e-3, "dbias")
    close(P["cls.transform.dense.weight"].grad, sdo["cls.transform.dense.weight"].grad, 1e-6, 2e-3, "ddense")


# ----------------------------------------------------------------------------- the whole step against the reference

TRAIN = dict(lr=2e-3, text_lr=1e-3, coef_lr=0.5, weight_decay=0.05)


def _model(g, dims, bdims, **tc):
    model = R.build(dims, bdims, contrast_num_negative=int(g["K"]), max_frames=int(g["F"]), **tc).to(DEV).train()
    return model, prep_optimizer(model, model.task_config, 10)


def _step(model, opt, batch, step):
    from hmmc_amd.optimization import clip_grad_norm_
    loss = model(*batch, step + 1)
    loss.backward()
    tn = clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    opt.zero_grad()
    return loss.detach(), tn


def _check_losses(model, g, step, loss):
    fam, vtm, ftm, mlm = [float(x.detach()) for x in model.last_losses]
    close(fam, g[f"fam{step}"], 2e-3, what=f"fam{step}")
    close(ftm, g[f"ftm{step}"], 2e-3, what=f"ftm{step}")
    close(mlm, g[f"mlm{step}"], 2e-3, what=f"mlm{step}")
    close(loss, g[f"loss{step}"], 2e-3, what=f"loss{step}")
    assert int(model.queue_ptr) == int(g[f"ptr{step}"][0]), "queue pointer"


def _check_state(model, g, step, atol_s=1e-5, atol_q=1e-5, rtol_s=1e-4, ema_bits=True):
    S = model.state_dict()
    for key in g.files:
        name = key.split(":", 1)[-1]
        if key.startswith(f"s{step}:"):
            mine = S[name].reshape(-1)[:16].float().cpu()
            if ema_bits and name.startswith(("text_encoder_k.chinese_encoder.", "text_encoder_k.text_proj.")):
                assert torch.equal(mine, torch.from_numpy(g[key])), f"EMA {name}: {mine} vs {g[key]}"       # fp32 EMA: bit patterns
            elif name.startswith("text_encoder."):
                close(mine, g[key], 2e-4, 1e-3, key)          # a BertAdam-updated weight: tests/test_gpu_zh.py's bound for those
            else:
                close(mine, g[key], atol_s, rtol_s, key)
        if key.startswith(f"q{step}:"):
            close(S[name][:32, :64], g[key], atol_q, what=key)


def test_five_steps_vs_reference_golden():
    name, dims, bdims = "moco_zh_fp32", synth.TINY, synth.ZH_TINY
    g = golden(name)
    K, B = int(g["K"]), int(g["B"])
    model, opt = _model(g, dims, bdims, **TRAIN)
    for step in range(5):
        batch = [t.to(DEV) for t in R.batch_of(name, g, dims, bdims, "tiny", step)]
        model._mlm_draws = R.draws_of(g, step)
        loss, tn = _step(model, opt, batch, step)
        _check_losses(model, g, step, loss)
        if step == 0:
            close(tn, g["gnorm0"], 0, 5e-3, "gnorm0")
            _check_state(model, g, 0)
        if step == 4:
            assert int(model.queue_ptr) == B                                       # wrapped: 5 x 4 keys into 16 columns
            for qn in ("queue_v_cross_ng", "queue_frame_cross_ng", "queue_title_cross_ng"):
                q = model.state_dict()[qn].float().cpu().numpy()
                assert np.isfinite(q).all()
                close(np.linalg.norm(q, axis=0), 1.0, 1e-4, what=f"{qn} column norms")
    ops.raise_on_device_errors(DEV)
    # the model keeps a host copy of queue_ptr (no device read per step); a checkpoint load must invalidate it
    S = {k: v.clone() for k, v in model.state_dict().items()}
    S["queue_ptr"] = torch.tensor([2 * B], dtype=torch.long)
    model.load_state_dict(S)
    model._mlm_draws = None
    before = model.queue_v_cross_ng.clone()
    model(*[t.to(DEV) for t in R.batch_of(name, g, dims, bdims, "tiny", 0)], 6)
    assert int(model.queue_ptr) == (3 * B) % K
    changed = (model.queue_v_cross_ng != before).any(dim=0).nonzero().view(-1).tolist()
    assert changed == list(range(2 * B, 3 * B)), changed


def test_step_0_gradients_vs_cpu_restatement():
    """Every parameter gradient of step 0 against the fp32 restatement: direction (cosine) and norm, as
    tests/test_gpu_pretrain.py::test_pretrain_gradients_vs_oracle."""
    name, dims, bdims = "moco_zh_fp32", synth.TINY, synth.ZH_TINY
    g = golden(name)
    K, Fr = int(g["K"]), int(g["F"])
    model, _ = _model(g, dims, bdims)
    batch = R.batch_of(name, g, dims, bdims, "tiny", 0)
    model._mlm_draws = R.draws_of(g, 0)
    loss = model(*[t.to(DEV) for t in batch], 1)
    loss.backward()
    sd = R.trainable_state(synth.pretrain_state_zh(dims, bdims, K, Fr))
    queues = {k: sd[k] for k in sd if k.startswith("queue_") and k != "queue_ptr"}
    ref, _, _ = R.pretrain_loss(batch, sd, queues, 0, K, json.loads(str(g["bert"])), R.draws_of(g, 0))
    ref.backward()
    close(loss, ref, 2e-3, what="loss")
    bad = []
    for n, p in model.named_parameters():
        if not p.requires_grad or "t_projector" in n:
            continue
        key = "cls.bias" if n == "cls.decoder.bias" else n
        assert p.grad is not None, n
        a, b = p.grad.float().cpu().flatten(), sd[key].grad.flatten()
        if n.endswith("attention.self.key.bias"):
            # zero in exact arithmetic: both sides hold rounding noise, below 1e-5 of the key weight's gradient
            wn = float(sd[key[:-4] + "weight"].grad.norm())
            assert float(a.norm()) <= 1e-5 * wn and float(b.norm()) <= 1e-5 * wn, n
            continue
        if float(b.norm()) < 1e-6:        # biases in front of BatchNorm: the true gradient is zero, both sides hold noise
            assert float(a.norm()) < 1e-4, n
            continue
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-20))
        ratio = float(a.norm() / (b.norm() + 1e-20))
        if cos < 0.97 or abs(ratio - 1) > 0.1:
            bad.append((n, round(cos, 4), round(ratio, 3), float(b.norm())))
    assert not bad, f"{len(bad)} gradients disagree with the restatement: {bad[:12]}"


def test_bird_step_vs_reference_golden():
    """dataset = "bird": separate tag passes and two MLM losses.  This model masks the tags before the titles, the reference
    the titles first: the recorded draws are handed over in this model's order."""
    name, dims, bdims = "moco_zh_bird_fp32", synth.TINY, synth.ZH_TINY
    g = golden(name)
    model, opt = _model(g, dims, bdims, dataset="bird", **TRAIN)
    model._mlm_draws = [R.draws_of(g, 0, tag=True), R.draws_of(g, 0)]
    loss, tn = _step(model, opt, [t.to(DEV) for t in R.batch_of(name, g, dims, bdims, "tiny", 0)], 0)
    _check_losses(model, g, 0, loss)
    close(tn, g["gnorm0"], 0, 5e-3, "gnorm0")
    _check_state(model, g, 0)


def test_two_steps_at_true_dimensions_vs_reference_golden():
    """ViT-B/32 beside BERT-base (vocabulary 21 128), K = 1 024, title 45 / tag 25; the tolerances of
    tests/test_gpu_fp32_regime.py::test_fp32_pretrain_at_true_vit_b32_dims_vs_reference_golden."""
    name, dims, bdims = "moco_zh_b32_fp32", synth.VIT_B32, synth.ZH_BASE
    g = golden(name)
    B = int(g["B"])
    model, opt = _model(g, dims, bdims, **TRAIN)
    for step in range(2):
        model._mlm_draws = R.draws_of(g, step)
        loss, tn = _step(model, opt, [t.to(DEV) for t in R.batch_of(name, g, dims, bdims, "b32", step)], step)
        _check_losses(model, g, step, loss)
        close(tn, g[f"gnorm{step}"], 0, 5e-3, f"gnorm{step}")
        assert int(model.queue_ptr) == B * (step + 1)
        _check_state(model, g, step, 2e-5 if step == 0 else 2e-4, 1e-5 if step == 0 else 2e-4, 1e-3, ema_bits=step == 0)
    ops.raise_on_device_errors(DEV)


# ----------------------------------------------------------------------------- resume, dropout, error flag, streams

def _fresh(**tc):
    dims, bdims = synth.TINY, synth.ZH_TINY
    model = R.build(dims, bdims, **TRAIN, **tc).to(DEV).train()
    batch = [t.to(DEV) for t in synth.pretrain_batch_zh(4, 4, bdims.vocab_size, 16, 9, tag="zh_pt", title_lens=[16, 1, 9, 5],
                                                         tag_lens=[9, 2, 5, 3])]
    return model, prep_optimizer(model, model.task_config, 50), batch


def test_resume_from_checkpoint_is_bit_identical():
    def steps(m, opt, batch, lo, hi):
        for i in range(lo, hi):
            torch.manual_seed(100 + i)                  # the MLM mask draws
            _step(m, opt, batch, i)

    m, opt, batch = _fresh()
    steps(m, opt, batch, 0, 2)
    buf = io.BytesIO()
    torch.save({"model": m.state_dict(), "opt": opt.state_dict()}, buf)
    steps(m, opt, batch, 2, 4)
    ref = {k: v.clone() for k, v in m.state_dict().items()}
    m2, opt2, batch2 = _fresh()
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    m2.load_state_dict(ck["model"])
    opt2.load_state_dict(ck["opt"])
    steps(m2, opt2, batch2, 2, 4)
    bad = [k for k, v in m2.state_dict().items() if not torch.equal(v, ref[k])]
    assert not bad, f"{len(bad)} tensors differ after the resume: {bad[:8]}"


def _loss_and_grads(model, batch, seed):
    torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    loss = model(*batch, 1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_dropout_step_is_finite_seeded_and_draws_a_seed_per_tower_call(monkeypatch):
    model, _, batch = _fresh(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    seeds, orig = [], Fn.bert_seed

    def spy():
        seeds.append(orig())
        return seeds[-1]

    monkeypatch.setattr(Fn, "bert_seed", spy)
    runs = []
    for seed in (11, 11, 12):
        model.load_state_dict(state)                    # the step moves the key encoders, the queues and the BN statistics
        del seeds[:]
        runs.append(_loss_and_grads(model, batch, seed))
        assert len(seeds) == 2 and seeds[0] != seeds[1], seeds      # the online and the momentum pass
    a, b, c = runs
    assert bool(torch.isfinite(a[0])) and all(bool(torch.isfinite(v).all()) for v in a[1].values())
    assert _same(a, b) and not torch.equal(a[0], c[0])
    plain, _, _ = _fresh()
    assert not torch.equal(_loss_and_grads(plain, batch, 11)[0], a[0]), "dropout changed nothing"


def test_a_title_id_outside_the_embedding_table_raises_the_device_flag():
    model, _, batch = _fresh()
    ops.raise_on_device_errors(DEV)
    batch[4] = batch[4].clone()
    batch[4][1, 0] = synth.ZH_TINY.vocab_size + 5
    model._mlm_draws = [torch.zeros(4, 16, dtype=torch.int64)] * 4
    model(*batch, 1)
    with pytest.raises(IndexError):
        ops.raise_on_device_errors(DEV)


def test_bit_identical_with_and_without_the_side_stream(monkeypatch):
    from hmmc_amd import modeling
    model, _, batch = _fresh()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    a = _loss_and_grads(model, batch, 5)
    model.load_state_dict(state)
    assert _same(a, _loss_and_grads(model, batch, 5))
    monkeypatch.setattr(modeling, "_OVERLAP_TOWERS", not modeling._OVERLAP_TOWERS)
    model.load_state_dict(state)
    assert _same(a, _loss_and_grads(model, batch, 5))
