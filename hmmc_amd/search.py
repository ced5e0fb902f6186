"""Top-N gallery search beside the eval leg: a packed gallery that stays on the device and is queried many times.

The eval leg (BirdPreTrainedModel.eval_similarity) ends at the [all queries, all videos] score matrix, which the rank metrics
need in full.  A search needs the N best candidates of every query only, so here the matrix is never held: one
[query chunk x gallery chunk] block is scored by the fused eval scorer exactly as eval_similarity scores it
(ops.eval_score), folded into running per-query lists by one streaming pass (ops.topn_select), and overwritten by the next
block.  The order of a list is (score descending, index ascending), a total order, so the result does not depend on how the
gallery or the queries were cut.  With frames=True a search also says where in each hit the match is: once the lists are
final, ops.hit_frames gathers the top_frames best frame logits of every (query, hit) pair and their frame numbers."""
import torch

from . import ops


class Gallery:
    """Videos packed once for the fused scorer (ops.eval_pack), in chunks the scorer's fast kernel takes.

    top_frames, scale: the k of the mean-of-top-k frame term and the min(exp(logit_scale), 100) of eval_similarity.
    chunk_videos: videos per packed chunk; None = the largest count that still meets the LDS-DMA conditions of
    hmmc_eval_score (nv * P * E * 4 + 64 * E * 4 < 2^31 and nv * P < 2^31, P = ops.eval_slots(F))."""

    def __init__(self, top_frames, scale, chunk_videos=None):
        if chunk_videos is not None and int(chunk_videos) < 1:
            raise ValueError("chunk_videos must be at least 1")
        self.top_frames = int(top_frames)
        self.scale = float(scale)
        self.chunk_videos = None if chunk_videos is None else int(chunk_videos)
        self.F = self.E = self.P = None
        self.chunks = []               # packed [count * P, E] tensors; all but the last hold chunk_videos videos
        self.counts = []
        self._block = {}               # tag -> the reused score block (and its transposed copy for search_texts)

    def __len__(self):
        return sum(self.counts)

    @staticmethod
    def max_chunk_videos(P, E):
        """largest nv with nv * P * E * 4 + 64 * E * 4 < 2^31 and nv * P < 2^31"""
        return max(1, min(((1 << 31) - 1 - 256 * E) // (4 * P * E), ((1 << 31) - 1) // P))

    def add(self, visual, frames):
        """visual [nv, E], frames [nv, F, E] -> (first, last): the new videos are indices first .. last - 1."""
        if frames.dim() != 3 or visual.dim() != 2 or visual.shape[0] != frames.shape[0] or visual.shape[1] != frames.shape[2]:
            raise ValueError(f"add: expected visual [nv, E] and frames [nv, F, E], got {tuple(visual.shape)} and {tuple(frames.shape)}")
        nv, F, E = frames.shape
        P = ops.eval_slots(F)
        if P == 0:
            raise ValueError(f"Gallery: F + 1 = {F + 1} slots per video, the fused scorer packs at most 32 (F <= 31)")
        if self.F is not None and (F, E) != (self.F, self.E):
            raise ValueError(f"Gallery: holds videos of F = {self.F}, E = {self.E}; cannot add F = {F}, E = {E}")
        if self.top_frames < 1 or self.top_frames > F:
            raise ValueError(f"Gallery: top_frames = {self.top_frames} outside 1 .. F = {F}")
        self.F, self.E, self.P = F, E, P
        if self.chunk_videos is None:
            self.chunk_videos = self.max_chunk_videos(P, E)
        visual, frames = visual.float().contiguous(), frames.float().contiguous()
        first, done = len(self), 0
        while done < nv:
            room = self.chunk_videos - self.counts[-1] if self.counts and self.counts[-1] < self.chunk_videos else 0
            take = min(nv - done, room or self.chunk_videos)
            packed = ops.eval_pack(visual[done:done + take], frames[done:done + take])
            if room:                   # packing is per video, so filling a chunk up equals packing it in one go
                self.chunks[-1] = torch.cat([self.chunks[-1], packed])
                self.counts[-1] += take
            else:
                self.chunks.append(packed)
                self.counts.append(take)
            done += take
        return first, first + nv

    # ---- the two searches ------------------------------------------------------------------------------------------------

    def _check(self, queries, topn):
        if topn < 1 or topn > ops.TOPN_MAX:
            raise ValueError(f"topn = {topn} outside 1 .. {ops.TOPN_MAX} (HMMC_TOPN_MAX of hmmc_topn_select)")
        if queries.dim() != 2 or (self.E is not None and queries.shape[1] != self.E):
            raise ValueError(f"queries must be [nq, E = {self.E}], got {tuple(queries.shape)}")

    def _buffer(self, tag, numel, device):
        buf = self._block.get(tag)
        if buf is None or buf.numel() < numel or buf.device != device:
            buf = self._block[tag] = torch.empty(numel, dtype=torch.float32, device=device)
        return buf

    @staticmethod
    def _lists(rows, topn, device):
        return (torch.full((rows, topn), float("-inf"), dtype=torch.float32, device=device),
                torch.full((rows, topn), -1, dtype=torch.int32, device=device))

    def _score(self, block, qn, c, use_frame_fea):
        ops.eval_score(qn, self.chunks[c], self.counts[c], self.F, self.top_frames, self.scale,
                       want=("score",) if use_frame_fea else ("video",), out=block)

    def _frame_lists(self, rows, topn, device):
        return (torch.full((rows, topn, self.top_frames), float("-inf"), dtype=torch.float32, device=device),
                torch.full((rows, topn, self.top_frames), -1, dtype=torch.int32, device=device))

    def _hit_frames(self, qn, c, base, pair_query, pair_video, out):
        """fill `out` for the pairs whose video lies in chunk c (videos base .. base + counts[c] - 1); the others keep theirs"""
        ops.hit_frames(qn, self.chunks[c], self.counts[c], self.F, self.top_frames, self.scale, pair_query, pair_video,
                       video_base=base, out=out)

    @torch.no_grad()
    def search(self, queries, topn, use_frame_fea=True, query_chunk=4096, frames=False):
        """text -> video: for every row of queries [nq, E] its topn videos -> (scores [nq, topn] fp32, indices [nq, topn]
        int64), best first, ties by index; (-inf, -1) past the end of a gallery smaller than topn.  Stays on the device.
        frames=True -> (scores, indices, frame_scores [nq, topn, top_frames] fp32, frame_indices, the same shape, int64): for
        the hit indices[r, j] its top_frames largest frame logits and their frame numbers, best first, ties by frame number -
        the terms whose mean the score adds to the video logit; (-inf, -1) in an empty slot.  They are gathered once a query
        chunk's lists are final (ops.hit_frames, one call per gallery chunk); with use_frame_fea=False the lists are ranked by
        the video logit alone and the frames are still those of each hit."""
        topn, query_chunk = int(topn), int(query_chunk)
        self._check(queries, topn)
        nq, dev = queries.shape[0], queries.device
        score, index = self._lists(nq, topn, dev)
        if frames:
            frame_score, frame_index = self._frame_lists(nq, topn, dev)
        q = queries.float().contiguous()
        rows = min(query_chunk, nq)
        buf = self._buffer("block", rows * max(self.counts, default=0), dev)
        for q0 in range(0, nq, query_chunk):
            q1 = min(nq, q0 + query_chunk)
            qn, _ = ops.l2norm_fwd(q[q0:q1])
            lists, base = (score[q0:q1], index[q0:q1]), 0
            for c, count in enumerate(self.counts):
                block = buf[:(q1 - q0) * count].view(q1 - q0, count)
                self._score(block, qn, c, use_frame_fea)
                ops.topn_select(block, topn, col_base=base, out=lists)
                base += count
            if frames:
                pair_query = torch.arange(q1 - q0, dtype=torch.int32, device=dev)[:, None].expand(q1 - q0, topn).contiguous()
                base = 0
                for c, count in enumerate(self.counts):
                    self._hit_frames(qn, c, base, pair_query, index[q0:q1], (frame_score[q0:q1], frame_index[q0:q1]))
                    base += count
        if frames:
            return score, index.long(), frame_score, frame_index.long()
        return score, index.long()

    @torch.no_grad()
    def search_texts(self, queries, topn, use_frame_fea=True, query_chunk=4096, frames=False):
        """video -> text: for every gallery video the topn rows of queries, same score -> (scores [len(g), topn] fp32,
        indices [len(g), topn] int64).  Each scored block is transposed into a second reused buffer and selected row-wise.
        frames=True adds frame_scores / frame_indices [len(g), topn, top_frames] as search() does: entry [v, j] holds the best
        frames of video v for the query indices[v, j].  The unit queries are resident whole here, so the gather is one
        ops.hit_frames call per gallery chunk."""
        topn, query_chunk = int(topn), int(query_chunk)
        self._check(queries, topn)
        nq, dev = queries.shape[0], queries.device
        score, index = self._lists(len(self), topn, dev)
        if frames:
            frame_score, frame_index = self._frame_lists(len(self), topn, dev)
        if nq == 0:
            return (score, index.long(), frame_score, frame_index.long()) if frames else (score, index.long())
        qn, _ = ops.l2norm_fwd(queries.float().contiguous())
        rows = min(query_chunk, nq)
        most = rows * max(self.counts, default=0)
        buf, tbuf = self._buffer("block", most, dev), self._buffer("transposed", most, dev)
        base = 0
        for c, count in enumerate(self.counts):
            lists = (score[base:base + count], index[base:base + count])
            for q0 in range(0, nq, query_chunk):
                q1 = min(nq, q0 + query_chunk)
                block = buf[:(q1 - q0) * count].view(q1 - q0, count)
                self._score(block, qn[q0:q1], c, use_frame_fea)
                turned = tbuf[:(q1 - q0) * count].view(count, q1 - q0)
                turned.copy_(block.t())
                ops.topn_select(turned, topn, col_base=q0, out=lists)
            base += count
        if frames:
            base = 0
            for c, count in enumerate(self.counts):
                pair_video = torch.arange(base, base + count, dtype=torch.int32, device=dev)[:, None].expand(count, topn).contiguous()
                self._hit_frames(qn, c, base, index[base:base + count], pair_video,
                                 (frame_score[base:base + count], frame_index[base:base + count]))
                base += count
            return score, index.long(), frame_score, frame_index.long()
        return score, index.long()
