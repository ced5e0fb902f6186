"""Plain-torch restatement of the pre-training step with the Chinese text branch (reference modules/modeling.py:334-436 with
language = "chinese"), assembled from tests/bert_ref.py (the BERT tower) and the oracle's heads, MoCo and optimizer pieces.
CPU, any float dtype; the comparison partner of tests/test_gpu_zh_pretrain.py, itself pinned to the reference's own run by
tests/test_zh_pretrain_cpu.py."""
import json
from argparse import Namespace

import torch
import torch.nn.functional as F

import bert_ref
from hmmc_amd import synth
from oracle import hmmc_oracle as O
from zh_common import bert_config_dir, cross_dir
from zh_pretrain_names import PRETRAIN_LENS

DRAW_NAMES = ("masked", "replaced", "randsel", "words")


def text_dir(bdims, vocab_lines=None, **over):
    """<pretrained_text> as a user of the reference has it: config.json and the BertTokenizer's vocab.txt."""
    d = bert_config_dir(bdims, **over)
    synth.write_bert_vocab(d, bdims, vocab_lines)
    return d


def task_config(bdims, vocab_lines=None, **kw):
    over = {k: kw.pop(k) for k in ("hidden_dropout_prob", "attention_probs_dropout_prob") if k in kw}
    d = dict(local_rank=0, rank=0, use_temp=True, language="chinese", top_frames=2, max_frames=4, n_display=100000, logdir=None,
             use_frame_fea=True, dataset="chvtt", contrast_momentum=0.99, contrast_temperature=0.07, contrast_num_negative=16,
             pretrained_text=text_dir(bdims, vocab_lines, **over), lr=1e-4, text_lr=3e-5, coef_lr=1e-3, weight_decay=0.2,
             warmup_proportion=0.1)
    d.update(kw)
    return Namespace(**d)


def build(dims, bdims, sd=None, **tc):
    """BirdPreTrainedModel(language = "chinese") with the synthetic state loaded, fp32 throughout (model.float())."""
    from hmmc_amd.modeling import BirdPreTrainedModel
    cfg = task_config(bdims, **tc)
    sd = sd if sd is not None else synth.pretrain_state_zh(dims, bdims, cfg.contrast_num_negative, cfg.max_frames)
    return BirdPreTrainedModel.from_pretrained(cross_dir(bdims), state_dict=sd, task_config=cfg).float()


def batch_of(name, g, dims, bdims, size, step):
    return synth.pretrain_batch_zh(int(g["B"]), int(g["F"]), bdims.vocab_size, int(g["title_len"]), int(g["tag_len"]), dims.image_res,
                                   tag=f"{name}.s{step}", title_lens=PRETRAIN_LENS[size]["title"][step],
                                   tag_lens=PRETRAIN_LENS[size]["tag"][step])


def draws_of(g, step, tag=False):
    """The four recorded draws of a mask() call as int64 tensors (the form BirdPreTrainedModel._mlm_draws takes)."""
    return [torch.from_numpy(g[f"mlm_{'tag_' if tag else ''}{n}{step}"]) for n in DRAW_NAMES]


def apply_mask(ids, draws, pad=synth.ZH_PAD, cls=synth.ZH_CLS, mask_id=synth.ZH_MASK):
    """modules/modeling.py:181-205 with the four draws passed in -> (masked ids, labels)."""
    masked, replaced, randsel, words = draws
    ids = ids.clone()
    labels = ids.clone()
    masked = masked.bool().clone()
    masked[ids == pad] = False
    masked[ids == cls] = False
    labels[~masked] = -100
    rep = replaced.bool() & masked
    ids[rep] = mask_id
    rnd = randsel.bool() & masked & ~rep
    ids[rnd] = words[rnd]
    return ids, labels


def trainable_state(raw, dtype=torch.float32):
    """synth.pretrain_state_zh -> the dict pretrain_loss works on: floating tensors in `dtype`, the online ones requiring grad."""
    sd = {}
    for k, v in raw.items():
        trainable = v.is_floating_point() and not any(s in k for s in ("_k.", "queue_", "running_", "num_batches"))
        sd[k] = v.clone().to(dtype).requires_grad_(trainable) if v.is_floating_point() else v.clone()
    sd["cls.decoder.bias"] = sd["cls.bias"]
    return sd


def pretrain_loss(batch, sd, queues, ptr, K, cfg, draws, tag_draws=None, m=0.99, T=0.07, weights=(0.05, 0.45, 0.45, 0.05)):
    """BirdPreTrainedModel.forward with language = "chinese", world size 1, fp32 regime.  cfg: the encoder's config dict;
    tag_draws given = dataset "bird".  Mutates sd (EMA, BN running statistics) and queues -> (loss, parts, new pointer)."""
    video, _, tag_ids, tag_mask, title_ids, title_mask = batch
    bird = tag_draws is not None

    def text(ids, mask, prefix="text_encoder.", want="feat"):
        return bert_ref.text_encoder(sd, ids, mask, cfg, prefix=prefix, want=want)

    v_fea, frame_fea = O.visual_encoder(video.to(sd["cls.bias"].dtype), sd, "visual_encoder.", "fp32")
    tag_fea = text(tag_ids, tag_mask) if bird else None
    title_fea = text(title_ids, title_mask)
    b, f, e = frame_fea.shape
    frame_proj, mu1, var1 = O.mlp_forward(frame_fea.reshape(-1, e), sd, "v_projector.")
    frame_pred, mu2, var2 = O.mlp_forward(frame_proj, sd, "v_predictor.")
    frame_proj, frame_pred = frame_proj.reshape(b, f, e), frame_pred.reshape(b, f, e)
    with torch.no_grad():
        for pair in ("visual_encoder", "text_encoder", "v_projector", "t_projector"):
            for k in list(sd.keys()):
                if k.startswith(pair + ".") and "running_" not in k and "num_batches" not in k:
                    kk = k.replace(pair + ".", pair + "_k.", 1)
                    sd[kk] = O.momentum_update(sd[kk], sd[k], m)
        tag_fea_k = text(tag_ids, tag_mask, "text_encoder_k.")
        title_fea_k = text(title_ids, title_mask, "text_encoder_k.")
        v_fea_k, frame_fea_k = O.visual_encoder(video.to(sd["cls.bias"].dtype), sd, "visual_encoder_k.", "fp32")
        frame_proj_k, mu3, var3 = O.mlp_forward(frame_fea_k.reshape(-1, e), sd, "v_projector_k.")
        frame_proj_k = frame_proj_k.reshape(b, f, e)
        for p, mu, var in (("v_projector.", mu1, var1), ("v_predictor.", mu2, var2), ("v_projector_k.", mu3, var3)):
            sd[p + "linear_hidden.2.running_mean"] = 0.9 * sd[p + "linear_hidden.2.running_mean"] + 0.1 * mu.detach()
            sd[p + "linear_hidden.2.running_var"] = 0.9 * sd[p + "linear_hidden.2.running_var"] + 0.1 * var.detach()
            sd[p + "linear_hidden.2.num_batches_tracked"] = sd[p + "linear_hidden.2.num_batches_tracked"] + 1
    q = queues
    fam = O.frame_self_loss(frame_pred, frame_proj_k, q["queue_frame_proj_ng"], T)
    vtm = O.contrastive_loss(v_fea, title_fea_k, q["queue_title_cross_ng"], T) + O.contrastive_loss(title_fea, v_fea_k, q["queue_v_cross_ng"], T)
    ftm = O.frame_cross_loss(frame_fea, frame_fea_k, q["queue_frame_cross_ng"], title_fea, title_fea_k, q["queue_title_cross_ng"], T)
    if bird:
        vtag = O.contrastive_loss(v_fea, tag_fea_k, q["queue_tag_cross_ng"], T) + O.contrastive_loss(tag_fea, v_fea_k, q["queue_v_cross_ng"], T)
        vtm = (vtag + vtm) / 2
        ftm = (O.frame_cross_loss(frame_fea, frame_fea_k, q["queue_frame_cross_ng"], tag_fea, tag_fea_k, q["queue_tag_cross_ng"], T) + ftm) / 2
    with torch.no_grad():
        new_ptr = O.enqueue(queues, ptr, v_fea_k, tag_fea_k, title_fea_k, frame_fea_k, frame_proj_k, K)

    def mlm_of(ids, mask, dr):
        masked_ids, labels = apply_mask(ids, dr)
        scores = O.mlm_head(text(masked_ids, mask, want="hidden"), sd)
        return F.cross_entropy(scores.reshape(-1, scores.shape[-1]), labels.reshape(-1), ignore_index=-100)

    mlm = mlm_of(title_ids, title_mask, draws)
    if bird:
        mlm = (mlm_of(tag_ids, tag_mask, tag_draws) + mlm) / 2
    w = weights
    return w[0] * fam + w[1] * vtm + w[2] * ftm + w[3] * mlm, (fam, vtm, ftm, mlm), new_ptr


def groups(names, lr, text_lr, coef_lr, wd):
    """main_pretrain.py's parameter groups (as main_task_retrieval.py:171-205): (lr, weight_decay) per parameter name."""
    out = {}
    for n in names:
        nod = any(nd in n for nd in ("bias", "LayerNorm.bias", "LayerNorm.weight"))
        lr_n = lr * coef_lr if "visual_encoder.visual." in n else (text_lr if "text_encoder." in n else lr)
        out[n] = (lr_n, 0.0 if nod else wd)
    return out


def run(name, g, dims, bdims, size, nsteps, bird=False):
    """The reference's main_pretrain.py loop on the restatement: forward, backward, clip, BertAdam.  Yields per step
    (step, sd, queues, loss, parts, total norm, pointer); sd holds the gradients of the step until the next one starts."""
    K, Fr = int(g["K"]), int(g["F"])
    cfg = json.loads(str(g["bert"]))
    sd = trainable_state(synth.pretrain_state_zh(dims, bdims, K, Fr))
    queues = {k: sd[k] for k in sd if k.startswith("queue_") and k != "queue_ptr"}
    names = [k for k, v in sd.items() if v.is_floating_point() and v.requires_grad and k != "cls.decoder.bias"]
    hp = groups(names, 2e-3, 1e-3, 0.5, 0.05)
    state = {k: (torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in names}
    ptr = 0
    for step in range(nsteps):
        batch = batch_of(name, g, dims, bdims, size, step)
        for k in names:
            sd[k].grad = None
        loss, parts, ptr = pretrain_loss(batch, sd, queues, ptr, K, cfg, draws_of(g, step), draws_of(g, step, tag=True) if bird else None)
        loss.backward()
        grads = {k: sd[k].grad.clone() for k in names if sd[k].grad is not None}
        tn = torch.nn.utils.clip_grad_norm_([sd[k] for k in grads], 1.0)
        with torch.no_grad():
            for k in grads:
                mm, vv = state[k]
                p, mm, vv, _ = O.bert_adam_step(sd[k].data, sd[k].grad, mm, vv, step, hp[k][0], 10, 0.1, hp[k][1])
                sd[k].data.copy_(p)
                state[k] = (mm, vv)
        yield step, sd, queues, loss.detach(), parts, tn, ptr, grads
