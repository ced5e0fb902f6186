"""Times, with HIP events in one process: the fine-tune step at B = 256, F = 12, L = 32 with the english and with the Chinese
text encoder (BERT-base), and the Chinese text tower alone forward + backward; prints one JSON line with the times and the
tower's GEMM rate (2·T·(4D² + 2·D·I)·layers·3 FLOP over the tower's time).  --text-dtype selects the Chinese encoder's
regime (fp16: module_cross.convert_bert_weights); --abba times both regimes in the order fp32, fp16, fp16, fp32 in this one
process and reports each regime's mean, and times the fp16 masked attention kernels alone at the tower's shape.

    python scratch/zh_step_times.py [--batch 256] [--frames 12] [--steps 5] [--warmup 2] [--text-dtype fp32|fp16] [--abba]
"""
import argparse
import json
import os
import sys
import tempfile
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hmmc_amd import ops, synth  # noqa: E402
from hmmc_amd.modeling import BirdModel  # noqa: E402
from hmmc_amd.module_cross import convert_bert_weights  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--text-dtype", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--abba", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dims, bd = synth.VIT_B32, synth.ZH_BASE
    B, Fr, L = args.batch, args.frames, args.length
    base = dict(local_rank=0, rank=0, use_temp=True, top_frames=2, max_frames=Fr, n_display=10 ** 9, logdir=None, use_frame_fea=True,
                dataset="msrvtt")
    vid = synth.video("zh_bench.video", 8, Fr).repeat(B // 8, 1, 1, 1, 1).to(dev)
    vf, idx = torch.full((B,), Fr, dtype=torch.long, device=dev), torch.arange(B, device=dev)
    out = {"batch": B, "frames": Fr, "length": L}

    def step_of(model, ids, mask):
        def step():
            model.zero_grad(set_to_none=True)
            model(ids, mask, vid, vf, idx, 1).backward()
        return step

    en = BirdModel.from_pretrained("cross-base", state_dict=synth.finetune_state(dims), task_config=Namespace(language="english", **base))
    en = en.to(dev).train()
    ids, mask = [t.to(dev) for t in synth.token_ids("zh_bench.en", B, L)]
    out["step_ms_english"] = timed(step_of(en, ids, mask), args.steps, args.warmup)
    del en
    torch.cuda.empty_cache()
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(bd.to_config(), fh)
    ids, mask = [t.to(dev) for t in synth.zh_token_ids("zh_bench.zh", B, L, bd.vocab_size)]
    g = torch.ones(B, 512, device=dev)
    T, D, I = B * L, bd.hidden_size, bd.intermediate_size
    flop = 3.0 * 2.0 * T * (4 * D * D + 2 * D * I) * bd.num_hidden_layers
    out["text_tower_gemm_tflop"] = flop / 1e12

    def chinese(regime):
        """(step ms, tower-alone forward + backward ms) of a fresh model in `regime`"""
        zh = BirdModel.from_pretrained("cross-base", state_dict=synth.finetune_state_zh(dims, bd),
                                       task_config=Namespace(language="chinese", pretrained_text=d, **base)).to(dev).train()
        if regime == "fp16":
            convert_bert_weights(zh.text_encoder)

        def tower():
            zh.zero_grad(set_to_none=True)
            zh.text_encoder(ids, mask).backward(g)

        return timed(step_of(zh, ids, mask), args.steps, args.warmup), timed(tower, args.steps, args.warmup)

    order = ("fp32", "fp16", "fp16", "fp32") if args.abba else (args.text_dtype,)
    runs = {}
    for regime in order:
        runs.setdefault(regime, []).append(chinese(regime))
        torch.cuda.empty_cache()
    out["order"] = list(order)
    for regime, r in runs.items():
        out[f"step_ms_chinese_{regime}"] = sum(x[0] for x in r) / len(r)
        out[f"text_tower_fwd_bwd_ms_{regime}"] = sum(x[1] for x in r) / len(r)
        out[f"text_tower_{regime}_tflops"] = flop / (out[f"text_tower_fwd_bwd_ms_{regime}"] * 1e-3) / 1e12
        out[f"runs_{regime}"] = r
    if "fp16" in runs:
        # the masked attention kernels alone at the tower's shape: 4 L^2 64 FLOP forward (QK^T, PV) and 10 L^2 64 backward (five
        # products) per (sequence, head)
        H = bd.num_attention_heads
        qkv = torch.randn(T, 3 * D, device=dev).half()
        dout = torch.randn(T, D, device=dev).half()
        for p in (0.0, 0.1):
            _, lse = ops.masked_attention_f16_fwd(qkv, mask, B, L, H, p, 1, 1)
            f = timed(lambda: ops.masked_attention_f16_fwd(qkv, mask, B, L, H, p, 1, 1), 20, 3)
            w = timed(lambda: ops.masked_attention_f16_bwd(qkv, mask, lse, dout, B, L, H, p, 1, 1), 20, 3)
            out[f"attention_f16_p{p}"] = {"fwd_us": f * 1e3, "bwd_us": w * 1e3,
                                          "fwd_tflops": 4.0 * L * L * 64 * B * H / (f * 1e-3) / 1e12,
                                          "bwd_tflops": 10.0 * L * L * 64 * B * H / (w * 1e-3) / 1e12,
                                          "share_of_tower_fwd_bwd": (f + w) * bd.num_hidden_layers / out["text_tower_fwd_bwd_ms_fp16"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
