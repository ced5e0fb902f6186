#!/usr/bin/env python
"""Golden vectors of PRE-TRAINING with the Chinese text branch, produced by running the REFERENCE itself on CPU
(BirdPreTrainedModel with language = "chinese": BertTokenizer + AutoModel loaded from a LOCAL directory).

    python tests/golden/make_golden_zh_pretrain.py [--only NAME]

The harness is make_golden.py's and make_golden_zh.py's; the synthetic BertModel directory additionally gets the synthetic
vocab.txt of hmmc_amd.synth.bert_vocab_lines, which the tests write too.  Both dropout probabilities are 0, the regime is fp32
(model.float()), and the four MLM draws of every mask() call are recorded.  Only arrays and a JSON manifest are stored."""
import argparse
import json
import os
import sys
import tempfile

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_zh as Z  # noqa: E402
from make_golden import import_reference, save, synth, task_config  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from zh_pretrain_names import PRETRAIN_LENS, PRETRAIN_SAMPLED  # noqa: E402  (tests/zh_pretrain_names.py: shared with the tests)


def build(mclip, mmodel, dims, bdims, sd, **tc):
    """The reference's BirdPreTrainedModel(language = "chinese") in fp32 with the synthetic state loaded."""
    clip_sd = synth.clip_state_from(synth.finetune_state(dims), dims)       # the reference builds a whole CLIP for logit_scale
    mclip.CLIP.get_config = staticmethod(lambda pretrained_clip_name="ViT-B/32": {k: v.clone() for k, v in clip_sd.items()})
    text_dir = Z.bert_dir(bdims)
    synth.write_bert_vocab(text_dir, bdims)
    cfg = task_config(language="chinese", pretrained_text=text_dir, **tc)
    model = mmodel.BirdPreTrainedModel.from_pretrained(Z.cross_dir(bdims), cache_dir=tempfile.mkdtemp(), state_dict=None,
                                                       task_config=cfg)
    tok = model.tokenizer
    assert (tok.vocab_size, tok.pad_token_id, tok.cls_token_id, tok.mask_token_id) == \
        (bdims.vocab_size, synth.ZH_PAD, synth.ZH_CLS, synth.ZH_MASK), "the synthetic vocab.txt is not read as intended"
    missing, unexpected = model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert not missing, missing
    model.float()
    model.train()
    return model, cfg


def _fixture(mclip, mmodel, mopt, name, dims, bdims, K, B, Fr, steps, dataset, size, queue_steps):
    Lt, Lg = PRETRAIN_LENS[size]["title_len"], PRETRAIN_LENS[size]["tag_len"]
    sd = synth.pretrain_state_zh(dims, bdims, K, Fr)
    model, cfg = build(mclip, mmodel, dims, bdims, sd, contrast_num_negative=K, max_frames=Fr, dataset=dataset, lr=2e-3,
                       text_lr=1e-3, coef_lr=0.5, weight_decay=0.05)
    opt = G._prep_optimizer(mopt, model, cfg, t_total=10)
    parts = {}
    for nm in ("frame_self_loss", "frame_cross_loss", "calculate_mlm_loss"):
        orig = getattr(model, nm)

        def wrap(*a, _o=orig, _n=nm, **k):
            r = _o(*a, **k)
            parts.setdefault(_n, []).append(r.detach().clone())
            return r
        setattr(model, nm, wrap)
    out = {"K": K, "B": B, "F": Fr, "title_len": Lt, "tag_len": Lg, "bert": json.dumps(bdims.to_config())}
    torch.manual_seed(1234)
    for step in range(steps):
        parts.clear()
        batch = synth.pretrain_batch_zh(B, Fr, bdims.vocab_size, Lt, Lg, dims.image_res, tag=f"{name}.s{step}",
                                        title_lens=PRETRAIN_LENS[size]["title"][step], tag_lens=PRETRAIN_LENS[size]["tag"][step])
        vid, vf, tg, gm, ti, tm = batch
        with G._Recorder() as rec:
            loss = model(vid, vf, tg, gm, ti, tm, step + 1)
        # the reference masks the titles first, then (dataset = "bird") the tags: four draws each
        assert len(rec.draws) == (8 if dataset == "bird" else 4), len(rec.draws)
        for i, nm in enumerate(("masked", "replaced", "randsel", "words")):
            out[f"mlm_{nm}{step}"] = rec.draws[i].numpy().astype(np.int64)
            if dataset == "bird":
                out[f"mlm_tag_{nm}{step}"] = rec.draws[4 + i].numpy().astype(np.int64)
        loss.backward()
        if step == 0:
            gn = G.grad_norms(model)
            names = sorted(gn)
            out["grad_norm_names"], out["grad_norm_values"] = np.array(names), np.array([gn[n] for n in names])
        tn = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        out[f"loss{step}"], out[f"gnorm{step}"] = loss.detach().clone(), tn.detach().clone()
        mean = lambda xs: torch.stack(xs).mean()                     # noqa: E731  (bird: the mean of the tag and title terms)
        out[f"fam{step}"], out[f"ftm{step}"], out[f"mlm{step}"] = parts["frame_self_loss"][0], mean(parts["frame_cross_loss"]), \
            mean(parts["calculate_mlm_loss"])
        out[f"ptr{step}"] = model.queue_ptr.clone()
        S = model.state_dict()
        for k in PRETRAIN_SAMPLED:
            out[f"s{step}:{k}"] = S[k].reshape(-1)[:16].clone()
        if step in queue_steps:
            for qn in ("queue_v_cross_ng", "queue_title_cross_ng", "queue_tag_cross_ng", "queue_frame_proj_ng",
                       "queue_frame_cross_ng"):
                out[f"q{step}:{qn}"] = S[qn][:32, :64].clone()
    save(name, **out)


def fx_moco_zh(mclip, mmodel, mopt, mmetrics):
    """K = 16, B = 4: the queue pointer wraps at step 4."""
    _fixture(mclip, mmodel, mopt, "moco_zh_fp32", synth.TINY, synth.ZH_TINY, 16, 4, 4, 5, "chvtt", "tiny", (0, 3, 4))


def fx_moco_zh_bird(mclip, mmodel, mopt, mmetrics):
    """dataset = "bird": the tag passes and two MLM losses."""
    _fixture(mclip, mmodel, mopt, "moco_zh_bird_fp32", synth.TINY, synth.ZH_TINY, 16, 4, 4, 1, "bird", "tiny", (0,))


def fx_moco_zh_b32(mclip, mmodel, mopt, mmetrics):
    """True dimensions: ViT-B/32 beside BERT-base (vocabulary 21 128), K = 1 024, title 45 / tag 25."""
    _fixture(mclip, mmodel, mopt, "moco_zh_b32_fp32", synth.VIT_B32, synth.ZH_BASE, 1024, 4, 2, 2, "chvtt", "b32", (0, 1))


def fx_manifest(mclip, mmodel, mopt, mmetrics):
    out = {}
    for tag, dims, bdims, K, Fr in (("pretrain_zh_tiny", synth.TINY, synth.ZH_TINY, 16, 4),
                                    ("pretrain_zh_b32", synth.VIT_B32, synth.ZH_BASE, 1024, 2)):
        model, _ = build(mclip, mmodel, dims, bdims, synth.pretrain_state_zh(dims, bdims, K, Fr), contrast_num_negative=K,
                         max_frames=Fr, dataset="chvtt")
        out[tag] = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
        out[tag + ":trainable"] = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    path = os.path.join(HERE, "statedict_manifest_zh_pretrain.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(f"wrote {path} ({os.path.getsize(path)/1024:.1f} KiB)")


FIXTURES = {"manifest": fx_manifest, "moco_zh": fx_moco_zh, "moco_zh_bird": fx_moco_zh_bird, "moco_zh_b32": fx_moco_zh_b32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.set_num_threads(8)
    mods = import_reference()
    for name, fn in FIXTURES.items():
        if args.only and name != args.only:
            continue
        print(f"== {name}")
        fn(*mods)


if __name__ == "__main__":
    main()
