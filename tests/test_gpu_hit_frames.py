"""GPU tests of hmmc_hit_frames (hmmc_amd/csrc/hit_frames.hip), ops.hit_frames and the frames=True searches of
hmmc_amd/search.py against tests/hit_frames_ref.py: bit for bit on data whose fp32 sums are exact, inside the any-order fp32
dot-product bound on random features, inside the two kernels' bounds against the fused scorer, and at gallery level."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hit_frames_ref as R  # noqa: E402
from conftest import golden  # noqa: E402
from hmmc_amd import _lib, ops, synth  # noqa: E402
from hmmc_amd.search import Gallery  # noqa: E402
from test_gpu_eval import model  # noqa: E402,F401  (the synthetic BirdModel fixture of the eval tests)

DEV = "cuda"
INF = float("inf")
U = 2.0 ** -24                       # unit roundoff of fp32
SENTINEL = (42.0, -7, 13.0)          # pre-fill of frame_score, frame_index, video_logit: what an untouched pair must still hold


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- exact data ------------------------------------------------------------------------------------------------------------

def exact_problem(E, F, seed):
    """integers in {-2, .., 2}: every product and every partial sum (|sum| <= 4 E) is an fp32 integer, and scale = +-0.5 keeps
    it exact - any summation order gives the same bits.  6 videos of a chunk whose global indices start at 1000, 5 queries."""
    rng = np.random.default_rng(seed)
    nq, nv, P = 5, 6, R.eval_slots(F)
    q = rng.integers(-2, 3, (nq, E)).astype(np.float32)
    packed = rng.integers(-2, 3, (nv, P, E)).astype(np.float32)      # slots past F hold values too: they are not frames
    if F >= 2:
        packed[0, 2] = packed[0, 1]                                  # frames 0 and 1 of video 0: one logit twice
    if F >= 4:
        packed[1, 1:F + 1] = packed[1, 1]                            # video 1: every frame the same, the list is 0, 1, 2, ..
        packed[4, F] = packed[4, 1]                                  # first and last frame of video 4
    packed[2, F, E - 1] = np.nan                                     # video 2: its last frame holds a NaN in the row's last element
    packed[3, 1] = 0                                                 # video 3, frame 0: a zero row; with scale < 0 its logit is -0
    return q, packed.reshape(nv * P, E), nq, nv


def exact_pairs(pairs, nq, nv, base, rng):
    pq = rng.integers(0, nq, pairs).astype(np.int32)
    pv = (base + rng.integers(0, nv, pairs)).astype(np.int32)
    if pairs >= 5:
        pq[1], pv[1] = -1, -1                                        # an empty list slot
        pv[3] = base + nv                                            # the first video of the next chunk
        pq[4], pv[4] = pq[0], pv[0]                                  # a repeated pair
    if pairs >= 20:
        pv[7] = base - 1                                             # the last video of the chunk before
        pq[8] = nq
        pq[9] = -1
        pv[10] = -1
        pq[11:19], pv[11:19] = np.arange(8) % nq, base + np.arange(8) % 6    # every planted video, with queries 0..4
        pq[pairs - 1], pv[pairs - 1] = 2, base + 2                   # the NaN video in the last, partly filled workgroup
    return pq, pv


def run_exact(q, packed, nq, nv, F, k, scale, pq, pv, base, want_video=True):
    pairs = pq.size
    out = [torch.full((pairs, k), SENTINEL[0], device=DEV), torch.full((pairs, k), SENTINEL[1], dtype=torch.int32, device=DEV)]
    if want_video:
        out.append(torch.full((pairs,), SENTINEL[2], device=DEV))
    got = ops.hit_frames(torch.from_numpy(q).to(DEV), torch.from_numpy(packed).to(DEV), nv, F, k, scale,
                         torch.from_numpy(pq).to(DEV), torch.from_numpy(pv).to(DEV), video_base=base, out=tuple(out),
                         want_video=want_video)
    assert len(got) == (3 if want_video else 2) and all(a is b for a, b in zip(got, out))
    return got


def check_exact(q, packed, nq, nv, F, k, scale, pq, pv, base):
    pairs = pq.size
    rs, ri, rv = R.hit_frames(q, packed, pq, pv, nv, F, k, scale, video_base=base, dtype=np.float32,
                              frame_score=np.full((pairs, k), SENTINEL[0], np.float32),
                              frame_index=np.full((pairs, k), SENTINEL[1], np.int32),
                              video_logit=np.full(pairs, SENTINEL[2], np.float32))
    fs, fi, vl = run_exact(q, packed, nq, nv, F, k, scale, pq, pv, base)
    what = f"E={q.shape[1]} F={F} k={k} pairs={pairs} scale={scale}"
    assert np.array_equal(fs.cpu().numpy().view(np.int32), rs.view(np.int32)), what      # bits: -0 would differ from +0
    assert np.array_equal(fi.cpu().numpy(), ri), what
    assert np.array_equal(vl.cpu().numpy(), rv), what
    valid = (pq >= 0) & (pq < nq) & (pv >= base) & (pv < base + nv)
    assert (rs[~valid] == SENTINEL[0]).all() and (ri[~valid] == SENTINEL[1]).all() and (rv[~valid] == SENTINEL[2]).all()
    fs2, fi2 = run_exact(q, packed, nq, nv, F, k, scale, pq, pv, base, want_video=False)  # video_logit = NULL: slot 0 is skipped
    assert torch.equal(bits(fs2), bits(fs)) and torch.equal(fi2, fi), what
    return rs, ri, valid


@pytest.mark.parametrize("F", [1, 12, 15, 16, 31])
@pytest.mark.parametrize("E", [4, 260, 512, 516])
def test_exact_data_bit_for_bit(E, F):
    """E: below one wave's span of 256, a ragged tail, the real width (the last with the query row in registers), and 516, the
    first width of the kernel that re-reads the query row.  F: both sides of the 16-slot and the 32-slot packing."""
    q, packed, nq, nv = exact_problem(E, F, seed=E * 100 + F)
    base = 1000
    rng = np.random.default_rng(7)
    seen_invalid = seen_tie = seen_nan = 0
    for pairs in (1, 5, 259):
        pq, pv = exact_pairs(pairs, nq, nv, base, rng)
        for k in sorted({1, (F + 1) // 2, F}):
            rs, ri, valid = check_exact(q, packed, nq, nv, F, k, 0.5, pq, pv, base)
            seen_invalid += int((~valid).sum())
            seen_nan += int(np.isneginf(rs[valid]).sum())
            full_tie = valid & (pv == base + 1)
            if F >= 4 and full_tie.any():
                assert (ri[full_tie] == np.arange(k)).all()          # equal logits come out in frame order
                seen_tie += 1
    assert seen_invalid > 0 and seen_nan > 0 and (F < 4 or seen_tie > 0)


def test_minus_zero_logit_comes_back_as_plus_zero():
    """scale = -0.5 on the zero frame row: the sum is +0, the logit -0.  Ranked as 0 and returned as +0."""
    E, F = 260, 12
    q, packed, nq, nv = exact_problem(E, F, seed=3)
    pq = np.arange(nq, dtype=np.int32)
    pv = np.full(nq, 1003, np.int32)
    rs, ri, _ = check_exact(q, packed, nq, nv, F, F, -0.5, pq, pv, 1000)
    at = ri == 0
    assert at.sum() == nq and (rs[at] == 0).all() and not np.signbit(rs[at]).any()


def test_more_pairs_than_waves_in_the_grid():
    """the launch holds 64 workgroups of four waves per compute unit; beyond that a wave strides over the pairs"""
    E, F, k = 4, 1, 1
    q, packed, nq, nv = exact_problem(E, F, seed=11)
    pairs = torch.cuda.get_device_properties(0).multi_processor_count * 64 * 4 + 7
    pq, pv = exact_pairs(pairs, nq, nv, 1000, np.random.default_rng(5))
    check_exact(q, packed, nq, nv, F, k, 0.5, pq, pv, 1000)


# ---- random features: the fp64 bound, and the fused scorer -------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_problem():
    """per (E, F): unit queries, a chunk packed by the real hmmc_eval_pack, and - from those fp32 rows - the fp64 logits L and
    the bound B of every (query, video, slot): B = scale * (E + 3) * 2^-24 * sum_e |q_e| |u_e|.  A sum of E products in any
    order, each operation rounded once (a fused multiply-add rounds less), is within (E - 1 + 1) u (1 + O(E u)) of the exact
    one relative to sum |q_e u_e| [Higham, Accuracy and Stability, (3.5)]; the product with scale adds one rounding; E + 3
    leaves two units for the second-order terms (E u < 4e-5)."""
    cache = {}
    nq, nv, scale = 40, 30, 100.0

    def get(E, F):
        if (E, F) not in cache:
            gen = torch.Generator(device=DEV).manual_seed(E + F)
            qn, _ = ops.l2norm_fwd(torch.randn(nq, E, device=DEV, generator=gen))
            packed = ops.eval_pack(torch.randn(nv, E, device=DEV, generator=gen), torch.randn(nv, F, E, device=DEV, generator=gen))
            P = ops.eval_slots(F)
            q64 = qn.cpu().double().numpy()
            r64 = packed.cpu().double().numpy().reshape(nv, P, E)[:, :F + 1]
            L = scale * np.einsum("qe,vse->qvs", q64, r64)
            B = scale * (E + 3) * U * np.einsum("qe,vse->qvs", np.abs(q64), np.abs(r64))
            cache[(E, F)] = dict(qn=qn, packed=packed, L=L, B=B, nq=nq, nv=nv, scale=scale)
        return cache[(E, F)]

    return get


@pytest.mark.parametrize("F", [12, 24])
@pytest.mark.parametrize("E", [64, 512])
def test_random_features_within_the_fp64_bound(random_problem, E, F):
    p = random_problem(E, F)
    nq, nv = p["nq"], p["nv"]
    perm = torch.randperm(nq * nv, generator=torch.Generator().manual_seed(1))
    pq, pv = (perm // nv).int().to(DEV), (perm % nv).int().to(DEV)
    for k in (3, F):
        fs, fi, vl = ops.hit_frames(p["qn"], p["packed"], nv, F, k, p["scale"], pq, pv, want_video=True)
        again = ops.hit_frames(p["qn"], p["packed"], nv, F, k, p["scale"], pq, pv, want_video=True)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((fs, fi, vl), again)), "two runs differ"
        back = torch.argsort(perm).to(DEV)                          # a pair's result does not depend on its position
        ordered = ops.hit_frames(p["qn"], p["packed"], nv, F, k, p["scale"], pq[back].contiguous(), pv[back].contiguous(), want_video=True)
        assert all(torch.equal(bits(a[back]), bits(b)) for a, b in zip((fs, fi, vl), ordered))
        s, i = fs.cpu().double().numpy(), fi.cpu().numpy().astype(np.int64)
        m = np.arange(nq * nv)
        L = p["L"][pq.cpu().numpy(), pv.cpu().numpy()]              # [pairs, 1 + F]
        B = p["B"][pq.cpu().numpy(), pv.cpu().numpy()]
        Lf, Bf = L[:, 1:], B[:, 1:]
        assert i.min() >= 0 and i.max() < F
        err = np.abs(s - np.take_along_axis(Lf, i, 1))
        bound = np.take_along_axis(Bf, i, 1)
        print(f"E={E} F={F} k={k}: worst error / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all()
        assert (np.abs(vl.cpu().double().numpy() - L[:, 0]) <= B[:, 0]).all()
        # each list sorted by (its own score descending, index ascending), k distinct frames
        assert ((s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (i[:, :-1] < i[:, 1:]))).all()
        assert all(len(set(row)) == k for row in i.tolist())
        # no omitted frame is better in fp64 than a returned one by more than the two bounds together
        omitted = np.ones((nq * nv, F), bool)
        omitted[m[:, None], i] = False
        if k < F:
            gap = (Lf - Bf)[:, None, :] - np.take_along_axis(Lf + Bf, i, 1)[:, :, None]      # [pairs, returned, frame]
            assert (gap[np.broadcast_to(omitted[:, None, :], gap.shape)] <= 0).all()
        else:
            assert not omitted.any()


@pytest.mark.parametrize("F", [12, 24])
@pytest.mark.parametrize("E", [64, 512])
def test_agrees_with_the_fused_scorer(random_problem, E, F):
    """mean(frame_score) against hmmc_eval_score's frame term, video_logit against its video term.  Both kernels compute every
    logit L_f inside B_f (random_problem; the scorer's MFMA sums are fp32 sums in another order).  The mean of the k largest
    is 1-Lipschitz in the maximum norm, so the two top-k means of the two sets of computed logits differ by at most
    max_f |x_f - y_f| <= 2 max_f B_f.  This side's mean is taken in fp64 here; the scorer's fp32 mean - k - 1 additions and a
    division, or a rounded reciprocal and a product - adds at most (k + 2) u max_f (|L_f| + B_f).  The video logits: 2 B_0."""
    p = random_problem(E, F)
    nq, nv, k = p["nq"], p["nv"], 3
    video, frame, _ = ops.eval_score(p["qn"], p["packed"], nv, F, k, p["scale"], want=("video", "frame"))
    pq = torch.arange(nq, dtype=torch.int32, device=DEV)[:, None].expand(nq, nv).contiguous()
    pv = torch.arange(nv, dtype=torch.int32, device=DEV)[None, :].expand(nq, nv).contiguous()
    fs, fi, vl = ops.hit_frames(p["qn"], p["packed"], nv, F, k, p["scale"], pq, pv, want_video=True)
    assert fs.shape == (nq, nv, k) and fi.shape == (nq, nv, k) and vl.shape == (nq, nv)
    L, B = p["L"], p["B"]
    margin = 2 * B[:, :, 1:].max(-1) + (k + 2) * U * (np.abs(L[:, :, 1:]) + B[:, :, 1:]).max(-1)
    diff = np.abs(fs.cpu().double().numpy().mean(-1) - frame.cpu().double().numpy())
    print(f"E={E} F={F}: worst frame-term difference / margin = {(diff / margin).max():.4f}")
    assert (diff <= margin).all()
    assert (np.abs(vl.cpu().double().numpy() - video.cpu().double().numpy()) <= 2 * B[:, :, 0]).all()


# ---- status returns --------------------------------------------------------------------------------------------------------

def test_status_returns():
    E, F, k, nq, nv, pairs = 8, 3, 2, 2, 2, 3
    q = torch.zeros(nq * E + 4, device=DEV)
    packed = torch.zeros(nv * 16 * E, device=DEV)
    pq, pv = torch.zeros(pairs, dtype=torch.int32, device=DEV), torch.zeros(pairs, dtype=torch.int32, device=DEV)
    fs, fi = torch.full((pairs, k), 1.0, device=DEV), torch.full((pairs, k), 5, dtype=torch.int32, device=DEV)
    lib, ptr = _lib.load(), _lib.ptr

    def call(q_=q, packed_=packed, pq_=pq, pv_=pv, fs_=fs, fi_=fi, pairs_=pairs, nq_=nq, nv_=nv, F_=F, E_=E, k_=k):
        return lib.hmmc_hit_frames(ptr(q_), ptr(packed_), ptr(pq_), ptr(pv_), ptr(fs_), ptr(fi_), None, pairs_, nq_, nv_, 0, F_,
                                   E_, k_, 1.0, _lib.stream())

    arg, unsupported = _lib.STATUS["HMMC_ERR_ARG"], _lib.STATUS["HMMC_ERR_UNSUPPORTED"]
    for bad in (dict(q_=None), dict(packed_=None), dict(pq_=None), dict(pv_=None), dict(fs_=None), dict(fi_=None), dict(k_=0),
                dict(k_=F + 1), dict(pairs_=-1), dict(nq_=-1), dict(nv_=-1), dict(F_=0)):
        assert call(**bad) == arg, bad
    for bad in (dict(F_=32, k_=2), dict(E_=6), dict(q_=q[1:]), dict(packed_=packed[1:])):
        assert call(**bad) == unsupported, bad
    assert call(pairs_=0) == 0
    torch.cuda.synchronize()
    assert bool((fs == 1.0).all()) and bool((fi == 5).all()), "nothing is launched on an error or for no pairs"
    assert call() == 0                                              # video_logit = NULL is allowed
    torch.cuda.synchronize()
    assert bool((fs == 0).all()) and fi.tolist() == [[0, 1]] * pairs        # all logits equal: frame order
    with pytest.raises(TypeError):
        ops.hit_frames(q[:nq * E].view(nq, E), packed.view(nv * 16, E), nv, F, k, 1.0, pq.long(), pv)
    with pytest.raises(ValueError, match="rows"):
        ops.hit_frames(q[:nq * E].view(nq, E), packed.view(nv * 16, E), nv + 1, F, k, 1.0, pq, pv)
    a, b = ops.hit_frames(q[:nq * E].view(nq, E), packed.view(nv * 16, E), nv, F, k, 1.0, pq - 1, pv)
    assert a.shape == (pairs, k) and bool((a == -INF).all()) and bool((b == -1).all())  # allocated here: pre-filled (-inf, -1)


# ---- gallery level ---------------------------------------------------------------------------------------------------------

NQ, NV, GF, GE, K = 23, 40, 12, 512, 3


@pytest.fixture(scope="module")
def features():
    q = synth.normal("hit.q", (NQ, GE)).to(DEV)
    v = synth.normal("hit.v", (NV, GE)).to(DEV)
    u = synth.normal("hit.u", (NV, GF, GE)).to(DEV)
    u[3, 5] = u[3, 2]                                               # two equal frame logits inside a video
    return q, v, u


def gallery_of(v, u, chunk_videos=None, scale=100.0):
    g = Gallery(K, scale, chunk_videos=chunk_videos)
    g.add(v, u)
    return g


def direct(g, q, pair_query, pair_video):
    """ops.hit_frames on a one-chunk gallery"""
    assert len(g.chunks) == 1
    qn, _ = ops.l2norm_fwd(q.float().contiguous())
    fs, fi = ops.hit_frames(qn, g.chunks[0], g.counts[0], g.F, g.top_frames, g.scale, pair_query.int().contiguous(),
                            pair_video.int().contiguous())
    return fs, fi.long()


@pytest.mark.parametrize("use_frame_fea", [True, False])
def test_search_frames_do_not_depend_on_the_chunking(features, use_frame_fea):
    q, v, u = features
    topn, first = 10, None
    for chunk_videos in (None, 7, 1):
        g = gallery_of(v, u, chunk_videos)
        plain = g.search(q, topn, use_frame_fea=use_frame_fea)
        for query_chunk in (4096, 5):
            got = g.search(q, topn, use_frame_fea=use_frame_fea, query_chunk=query_chunk, frames=True)
            assert len(got) == 4 and got[2].shape == (NQ, topn, K) and got[3].shape == (NQ, topn, K)
            assert got[2].dtype == torch.float32 and got[3].dtype == torch.int64 and got[2].is_cuda and got[3].is_cuda
            assert torch.equal(bits(got[0]), bits(plain[0])) and torch.equal(got[1], plain[1])
            if first is None:
                first = got
                rows = torch.arange(NQ, device=DEV)[:, None].expand(NQ, topn)
                fs, fi = direct(g, q, rows, got[1])
                assert torch.equal(bits(got[2]), bits(fs)) and torch.equal(got[3], fi)
                assert bool((got[3] >= 0).all()) and bool(torch.isfinite(got[2]).all())
            assert all(torch.equal(bits(a), bits(b)) if a.dtype == torch.float32 else torch.equal(a, b) for a, b in zip(got, first)), \
                f"chunk_videos={chunk_videos} query_chunk={query_chunk}"


def test_gallery_smaller_than_topn_leaves_empty_frame_tails(features):
    q, v, u = features
    g = gallery_of(v[:5], u[:5])
    scores, indices, fs, fi = g.search(q, 10, frames=True)
    assert bool((indices[:, 5:] == -1).all()) and bool((fs[:, 5:] == -INF).all()) and bool((fi[:, 5:] == -1).all())
    assert bool((indices[:, :5] >= 0).all()) and bool(torch.isfinite(fs[:, :5]).all()) and bool((fi[:, :5] >= 0).all())
    scores, indices, fs, fi = Gallery(K, 100.0).search(q, 3, frames=True)
    assert fs.shape == (NQ, 3, K) and bool((fs == -INF).all()) and bool((fi == -1).all())


def test_search_texts_frames_equal_direct_calls(features):
    q, v, u = features
    one = gallery_of(v, u)
    topn = 30                                                       # 23 queries: (-inf, -1) tails
    for chunk_videos, query_chunk in ((None, 4096), (7, 5)):
        g = gallery_of(v, u, chunk_videos)
        plain = g.search_texts(q, topn, query_chunk=query_chunk)
        scores, indices, fs, fi = g.search_texts(q, topn, query_chunk=query_chunk, frames=True)
        assert torch.equal(bits(scores), bits(plain[0])) and torch.equal(indices, plain[1])
        assert fs.shape == (NV, topn, K) and fi.dtype == torch.int64
        cols = torch.arange(NV, device=DEV)[:, None].expand(NV, topn)
        ds, di = direct(one, q, indices, cols)                      # entry [v, j]: the pair (indices[v, j], v)
        assert torch.equal(bits(fs), bits(ds)) and torch.equal(fi, di)
        assert bool((indices[:, NQ:] == -1).all()) and bool((fs[:, NQ:] == -INF).all()) and bool((fi[:, NQ:] == -1).all())
        assert bool((fi[:, :NQ] >= 0).all())


def test_model_search_frames_vs_reference_golden(model):  # noqa: F811
    """scores = video logit + mean of the top_frames best frame logits: what is left after taking the returned frames' mean
    away is the reference's S_video at the hit"""
    g = golden("head_eval")
    q = synth.normal("head_eval.q", (48, 512))
    v = synth.normal("head_eval.v", (48, 512))
    u = synth.normal("head_eval.u", (48, 12, 512))
    q = (q + 0.7 * v).to(DEV)
    v, u = v.to(DEV), u.to(DEV)
    model.top_frames = K
    gallery = model.build_gallery([v[:20], v[20:]], [u[:20], u[20:]], chunk_videos=20)
    scores, indices, fs, fi = model.search([q[:7], q[7:]], gallery, 48, frames=True)
    assert fs.shape == (48, 48, K) and bool((indices >= 0).all())
    ref = torch.from_numpy(g["S_video"]).to(DEV).gather(1, indices)
    err = float((scores - fs.mean(-1) - ref).abs().max())
    print(f"scores - frame mean against the golden S_video: {err:.2e}")
    assert err < 1e-3
    plain = model.search([q], gallery, 48)
    assert torch.equal(bits(scores), bits(plain[0])) and torch.equal(indices, plain[1])


def test_gallery_still_refuses_32_frames_by_name():
    with pytest.raises(ValueError, match="F <= 31"):
        Gallery(K, 100.0).add(torch.randn(3, GE, device=DEV), torch.randn(3, 32, GE, device=DEV))
