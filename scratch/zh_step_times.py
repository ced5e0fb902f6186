"""Times, with HIP events in one process: the fine-tune step at B = 256, F = 12, L = 32 with the english and with the Chinese
text encoder (fp32 BERT-base), and the Chinese text tower alone forward + backward; prints one JSON line with the three
times and the tower's fp32 GEMM rate (2·T·(4D² + 2·D·I)·layers·3 FLOP over the tower's time).

    python scratch/zh_step_times.py [--batch 256] [--frames 12] [--steps 5] [--warmup 2]
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
from hmmc_amd.modeling import BirdModel  # noqa: E402


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
    zh = BirdModel.from_pretrained("cross-base", state_dict=synth.finetune_state_zh(dims, bd),
                                   task_config=Namespace(language="chinese", pretrained_text=d, **base)).to(dev).train()
    ids, mask = [t.to(dev) for t in synth.zh_token_ids("zh_bench.zh", B, L, bd.vocab_size)]
    out["step_ms_chinese"] = timed(step_of(zh, ids, mask), args.steps, args.warmup)
    g = torch.ones(B, 512, device=dev)

    def tower():
        zh.zero_grad(set_to_none=True)
        zh.text_encoder(ids, mask).backward(g)

    out["text_tower_fwd_bwd_ms"] = timed(tower, args.steps, args.warmup)
    T, D, I = B * L, bd.hidden_size, bd.intermediate_size
    flop = 3.0 * 2.0 * T * (4 * D * D + 2 * D * I) * bd.num_hidden_layers
    out["text_tower_gemm_tflop"] = flop / 1e12
    out["text_tower_f32_tflops"] = flop / (out["text_tower_fwd_bwd_ms"] * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
