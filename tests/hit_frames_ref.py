"""numpy restatement of hmmc_hit_frames (include/hmmc_hip.h): for given (query, video) pairs the k largest frame logits and
their frame numbers, plus the video logit - in fp64, and in fp32 for data whose sums are exact in any order.

Conventions, as the header states them: the order is (logit descending, frame ascending), a total order; NaN counts as, and is
returned as, -inf; -0 is returned as +0; a pair whose query lies outside 0..nq-1 or whose video lies outside
video_base .. video_base + nv - 1 leaves its outputs as they were (-1 marks an empty list slot)."""
import numpy as np


def eval_slots(F):
    """hmmc_eval_slots: rows per video of the packed matrix"""
    return 16 if F + 1 <= 16 else 32 if F + 1 <= 32 else 0


def pack(visual, frames, dtype=np.float64):
    """hmmc_eval_pack: [nv, E], [nv, F, E] -> [nv * P, E]: slot 0 visual / |visual|, slots 1..F frames / |frames|, rest zero"""
    visual, frames = np.asarray(visual, dtype), np.asarray(frames, dtype)
    nv, F, E = frames.shape
    P = eval_slots(F)
    out = np.zeros((nv, P, E), dtype)
    out[:, 0] = visual / np.linalg.norm(visual, axis=-1, keepdims=True)
    out[:, 1:F + 1] = frames / np.linalg.norm(frames, axis=-1, keepdims=True)
    return out.reshape(nv * P, E)


def canonical(x):
    """NaN -> -inf, -0 -> +0"""
    x = np.where(np.isnan(x), -np.inf, x)
    return np.where(x == 0, np.zeros_like(x), x)


def logits(queries_unit, packed, pair_query, pair_video, nv, F, scale, video_base=0, dtype=np.float64):
    """-> (valid [pairs] bool, frame logits [pairs, F], video logits [pairs]) in `dtype`, as computed (not canonical); rows of
    invalid pairs are zero"""
    q = np.asarray(queries_unit, dtype)
    nq, E = q.shape
    P = eval_slots(F)
    rows = np.asarray(packed, dtype).reshape(nv, P, E)
    pq = np.asarray(pair_query).astype(np.int64).ravel()
    pv = np.asarray(pair_video).astype(np.int64).ravel() - video_base
    valid = (pq >= 0) & (pq < nq) & (pv >= 0) & (pv < nv)
    frame = np.zeros((pq.size, F), dtype)
    video = np.zeros(pq.size, dtype)
    s = dtype(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        for start in range(0, pq.size, 4096):                    # [4096, F + 1, E] at a time
            m = np.flatnonzero(valid[start:start + 4096]) + start
            if m.size:
                dots = np.einsum("me,mse->ms", q[pq[m]], rows[pv[m], :F + 1]).astype(dtype)
                video[m], frame[m] = s * dots[:, 0], s * dots[:, 1:]
    return valid, frame, video


def hit_frames(queries_unit, packed, pair_query, pair_video, nv, F, k, scale, video_base=0, frame_score=None, frame_index=None,
               video_logit=None, dtype=np.float64):
    """-> (frame_score [pairs, k] `dtype`, frame_index [pairs, k] int32, video_logit [pairs] `dtype`); the three arrays given
    (or (-inf, -1, NaN) fills) keep their values for the pairs outside the chunk"""
    assert 1 <= k <= F and eval_slots(F)
    valid, frame, video = logits(queries_unit, packed, pair_query, pair_video, nv, F, scale, video_base, dtype)
    pairs = valid.size
    fs = np.full((pairs, k), -np.inf, dtype) if frame_score is None else np.array(frame_score, dtype).reshape(pairs, k)
    fi = np.full((pairs, k), -1, np.int32) if frame_index is None else np.array(frame_index, np.int32).reshape(pairs, k)
    vl = np.full(pairs, np.nan, dtype) if video_logit is None else np.array(video_logit, dtype).reshape(pairs)
    x = canonical(frame)
    order = np.argsort(-x, axis=1, kind="stable")[:, :k]          # stable: equal logits stay in frame order
    fs[valid] = np.take_along_axis(x, order, 1)[valid]
    fi[valid] = order[valid]
    vl[valid] = video[valid]
    return fs, fi, vl
