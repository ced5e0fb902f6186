"""Times, with HIP events in one process, the PRE-TRAINING step with the Chinese text encoder at config 4's shape: B = 128, F = 12,
K = 1 024, title 45 / tag 25, ViT-B/32 beside fp32 BERT-base (vocabulary 21 128), dropout 0.1; forward + backward + clip +
BertAdam.  Prints one JSON line.  The English step of the same shape is `python bench.py --mode pretrain`.  --text-dtype selects
the Chinese encoders' regime (fp16: module_cross.convert_bert_weights on text_encoder and text_encoder_k); --abba times both
regimes in the order fp32, fp16, fp16, fp32 in this one process and reports each regime's mean.

    python scratch/zh_pretrain_step_times.py [--batch 128] [--frames 12] [--steps 5] [--warmup 2] [--dropout 0.1]
                                             [--text-dtype fp32|fp16] [--abba]
"""
import argparse
import json
import os
import sys
import tempfile
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hmmc_amd import synth  # noqa: E402
from hmmc_amd.modeling import BirdPreTrainedModel  # noqa: E402
from hmmc_amd.module_cross import convert_bert_weights  # noqa: E402
from hmmc_amd.optimization import BertAdam, clip_grad_norm_  # noqa: E402
from zh_step_times import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--negatives", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--text-dtype", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--abba", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dims, bd = synth.VIT_B32, synth.ZH_BASE
    B, Fr, K = args.batch, args.frames, args.negatives
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(dict(bd.to_config(), hidden_dropout_prob=args.dropout, attention_probs_dropout_prob=args.dropout), fh)
    synth.write_bert_vocab(d, bd)
    cfg = Namespace(local_rank=0, rank=0, use_temp=True, language="chinese", pretrained_text=d, top_frames=2, max_frames=Fr,
                    n_display=10 ** 9, logdir=None, use_frame_fea=True, dataset="chvtt", contrast_momentum=0.99,
                    contrast_temperature=0.07, contrast_num_negative=K)
    vid, vf, tg, gm, ti, tm = synth.pretrain_batch_zh(8, Fr, bd.vocab_size, tag="zh_pretrain_bench")
    rep = lambda t: t.repeat(B // 8, *([1] * (t.dim() - 1))).to(dev)                 # noqa: E731
    batch = [rep(vid), torch.full((B,), Fr, dtype=torch.long, device=dev), rep(tg), rep(gm), rep(ti), rep(tm)]


    def run(regime):
        model = BirdPreTrainedModel.from_pretrained("cross-base", state_dict=synth.pretrain_state_zh(dims, bd, K, Fr), task_config=cfg)
        model = model.to(dev).train()
        if regime == "fp16":
            convert_bert_weights(model.text_encoder)
            convert_bert_weights(model.text_encoder_k)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = BertAdam(params, lr=1e-4, warmup=0.1, t_total=10 ** 6, schedule="warmup_cosine", b1=0.9, b2=0.98, weight_decay=0.2)

        def step():
            model(*batch, 1).backward()
            clip_grad_norm_(params, 1.0)
            opt.step()
            opt.zero_grad()

        return timed(step, args.steps, args.warmup)

    order = ("fp32", "fp16", "fp16", "fp32") if args.abba else (args.text_dtype,)
    runs = {}
    for regime in order:
        runs.setdefault(regime, []).append(run(regime))
        torch.cuda.empty_cache()
    out = {"mode": "pretrain, language chinese", "batch": B, "frames": Fr, "negatives": K, "title_len": 45, "tag_len": 25,
           "dropout": args.dropout, "order": list(order)}
    for regime, r in runs.items():
        ms = sum(r) / len(r)
        out.update({f"step_ms_{regime}": ms, f"videos_per_s_{regime}": B / ms * 1e3, f"runs_{regime}": r})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
