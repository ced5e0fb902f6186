"""Times of the top-N gallery search ("Gallery search"): HIP events, warm-up then timed repetitions,
variants alternated A-B-C-C-B-A in one process; median and min over the rounds, one JSON line per measurement.

  (a) hmmc_topn_select (n = 10, n = 128; lists formed from the block alone) against the hmmc_eval_score launch that wrote the
      block, on random features and on the ascending-row worst case, at [4 096 x 1 500] F = 24 and [4 096 x 16 384] F = 12
  (b) model.search(topn = 10) against eval_similarity + torch.topk(sim, 10) at 15 000 x 1 500 x 24 (bench.py --mode eval
      --frames 24), same process, same inputs

  (c) Gallery.search(frames=True) against Gallery.search() at 4 096 queries x 1 500 videos, topn 10 and 128, F 12 and 24:
      the added time, and the gathered bytes per second pairs * (F + 1) * E * 4 / t over it and over the hmmc_hit_frames
      launch alone on the final lists

    python scratch/search_times.py [--rounds 5] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hmmc_amd import _lib, ops  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, rounds, reps, warmup=3):
    """{name: fn} -> {name: {"median_ms", "min_ms", "max_ms"}}, each round runs the variants forwards then backwards"""
    names = list(variants)
    for name in names:
        for _ in range(warmup):
            variants[name]()
    torch.cuda.synchronize()
    samples = {name: [] for name in names}
    for _ in range(rounds):
        for name in names + names[::-1]:
            samples[name].append(timed(variants[name], reps))
    return {name: {"median_ms": round(statistics.median(s), 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4)}
            for name, s in samples.items()}


def select_vs_scorer(nq, nv, F, rounds, reps, emit):
    E, k = 512, 3
    gen = torch.Generator(device=DEV).manual_seed(1)
    qn, _ = ops.l2norm_fwd(torch.randn(nq, E, device=DEV, generator=gen))
    packed = ops.eval_pack(torch.randn(nv, E, device=DEV, generator=gen), torch.randn(nv, F, E, device=DEV, generator=gen))
    block = torch.empty(nq, nv, device=DEV)
    lists = {n: (torch.empty(nq, n, device=DEV), torch.empty(nq, n, dtype=torch.int32, device=DEV)) for n in (10, 128)}

    def select(S, n):
        return lambda: _lib.call("hmmc_topn_select", _lib.ptr(S), nq, nv, nv, 0, _lib.ptr(lists[n][0]), _lib.ptr(lists[n][1]), n, 0)

    variants = {"scorer": lambda: ops.eval_score(qn, packed, nv, F, k, 100.0, want=("score",), out=block)}
    variants["scorer"]()
    variants.update({"select_n10": select(block, 10), "select_n128": select(block, 128)})
    res = alternate(variants, rounds, reps)
    base = res["scorer"]["median_ms"]
    for name in ("select_n10", "select_n128"):
        res[name]["share_of_scorer"] = round(res[name]["median_ms"] / base, 4)
        res[name]["GB_per_s"] = round(nq * nv * 4 / res[name]["median_ms"] / 1e6, 1)
    emit({"what": "select pass vs the scorer launch of its block, random scores", "block": [nq, nv], "F": F, **res})
    ascending = torch.arange(nv, device=DEV, dtype=torch.float32).repeat(nq, 1)
    worst = alternate({"select_n10": select(ascending, 10), "select_n128": select(ascending, 128)}, max(2, rounds // 2), max(2, reps // 4))
    for name in worst:
        worst[name]["share_of_scorer"] = round(worst[name]["median_ms"] / base, 4)
    emit({"what": "select pass on ascending rows (every column enters the list): no bound", "block": [nq, nv], **worst})


def search_vs_eval(rounds, reps, emit):
    from bench import task_config
    from hmmc_amd.modeling import BirdModel
    nq, nv, F, E = 15000, 1500, 24, 512
    torch.manual_seed(42)
    model = BirdModel.from_pretrained("cross-base", state_dict=None,
                                      task_config=task_config(max_frames=F, pretrained_clip_name="ViT-B/32")).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(7)
    qs = [torch.randn(min(64, nq - s), E, generator=gen, device=DEV) for s in range(0, nq, 64)]
    vs = [torch.randn(min(64, nv - s), E, generator=gen, device=DEV) for s in range(0, nv, 64)]
    us = [torch.randn(min(64, nv - s), F, E, generator=gen, device=DEV) for s in range(0, nv, 64)]
    gallery = model.build_gallery(vs, us)

    def pair():
        return torch.topk(model.eval_similarity(qs, vs, us), 10, dim=1)

    def search_only():
        return model.search(qs, gallery, 10)

    def build_and_search():
        return model.search(qs, model.build_gallery(vs, us), 10)

    a, b = pair(), build_and_search()
    same = bool(torch.equal(a[0], b[0]))          # scores; torch.topk's order among equal scores is its own
    res = alternate({"eval_similarity_then_topk": pair, "build_gallery_then_search": build_and_search, "search_resident_gallery": search_only},
                    rounds, max(2, reps // 4))
    base = res["eval_similarity_then_topk"]["median_ms"]
    for name in ("build_gallery_then_search", "search_resident_gallery"):
        res[name]["vs_pair"] = round(res[name]["median_ms"] / base, 4)
    emit({"what": "whole search vs eval_similarity + torch.topk(sim, 10)", "size": [nq, nv, F], "scores_equal": same, **res})


def frames_vs_plain_search(nq, nv, F, topn, rounds, reps, emit):
    from hmmc_amd.search import Gallery
    E, k = 512, 3
    gen = torch.Generator(device=DEV).manual_seed(2)
    q = torch.randn(nq, E, device=DEV, generator=gen)
    gallery = Gallery(k, 100.0)
    gallery.add(torch.randn(nv, E, device=DEV, generator=gen), torch.randn(nv, F, E, device=DEV, generator=gen))
    qn, _ = ops.l2norm_fwd(q)
    _, index = gallery.search(q, topn)
    pair_video = index.int().contiguous()
    pair_query = torch.arange(nq, dtype=torch.int32, device=DEV)[:, None].expand(nq, topn).contiguous()
    out = ops.hit_frames(qn, gallery.chunks[0], nv, F, k, 100.0, pair_query, pair_video)
    res = alternate({"search": lambda: gallery.search(q, topn), "search_frames": lambda: gallery.search(q, topn, frames=True),
                     "hit_frames_launch": lambda: ops.hit_frames(qn, gallery.chunks[0], nv, F, k, 100.0, pair_query, pair_video, out=out)},
                    rounds, reps)
    gathered = nq * topn * (F + 1) * E * 4
    added = res["search_frames"]["median_ms"] - res["search"]["median_ms"]
    emit({"what": "search(frames=True) vs search()", "size": [nq, nv, F], "topn": topn, "pairs": nq * topn,
          "gathered_MB": round(gathered / 1e6, 1), "added_ms": round(added, 4),
          "added_share_of_search": round(added / res["search"]["median_ms"], 4),
          "GB_per_s_over_added": round(gathered / added / 1e6, 1) if added > 0 else None,
          "GB_per_s_over_launch": round(gathered / res["hit_frames_launch"]["median_ms"] / 1e6, 1), **res})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    select_vs_scorer(4096, 1500, 24, args.rounds, args.reps, emit)
    select_vs_scorer(4096, 16384, 12, args.rounds, max(2, args.reps // 4), emit)
    search_vs_eval(args.rounds, args.reps, emit)
    for F in (12, 24):
        for topn in (10, 128):
            frames_vs_plain_search(4096, 1500, F, topn, args.rounds, args.reps, emit)


if __name__ == "__main__":
    main()
