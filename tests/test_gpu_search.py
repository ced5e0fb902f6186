"""GPU tests of the top-N gallery search (hmmc_amd/search.py, BirdPreTrainedModel.build_gallery / search) against the
unchanged eval path: model.eval_similarity's full matrix, sorted stably, is the reference - indices equal, scores bit-equal
(both sides go through the same scorer kernel, and a (query, video) score is formed from the same operands in the same K
order whatever block it lands in)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hmmc_amd import metrics as M  # noqa: E402
from hmmc_amd import synth  # noqa: E402
from hmmc_amd.search import Gallery  # noqa: E402
from test_gpu_eval import model  # noqa: E402,F401  (the synthetic BirdModel fixture of the eval tests)

DEV = "cuda"
NQ, NV, E, K = 70, 150, 512, 3
COPIES = (5, 17, 90, 149)          # videos 5, 90 and 149 are copies of video 17: with chunk_videos = 64, three different chunks
INF = float("inf")


@pytest.fixture(scope="module")
def problem(model):  # noqa: F811
    """per F: features, the reference matrices of the unchanged eval path (computed once), galleries per chunk_videos"""
    model.top_frames = K
    cache = {}

    def get(F):
        if F not in cache:
            q = synth.normal("search.q", (NQ, E)).to(DEV)
            v = synth.normal("search.v", (NV, E)).to(DEV)
            u = synth.normal(f"search.u{F}", (NV, F, E)).to(DEV)
            for c in COPIES:
                v[c], u[c] = v[17], u[17]
            sims = {fea: model.eval_similarity([q[:33], q[33:]], [v[:100], v[100:]], [u[:100], u[100:]], use_frame_fea=fea)
                    for fea in (True, False)}
            cache[F] = {"q": q, "v": v, "u": u, "sim": sims, "gallery": {}}
        return cache[F]

    def gallery(F, chunk_videos):
        p = get(F)
        if chunk_videos not in p["gallery"]:
            p["gallery"][chunk_videos] = model.build_gallery([p["v"][:100], p["v"][100:]], [p["u"][:100], p["u"][100:]],
                                                             chunk_videos=chunk_videos)
        return p["gallery"][chunk_videos]

    get.gallery = gallery
    return get


def sorted_reference(sim, topn):
    """first topn columns of the stable descending sort of every row, padded with (-inf, -1)"""
    val, idx = torch.sort(sim, dim=1, descending=True, stable=True)
    rows, cols = sim.shape
    score = torch.full((rows, topn), -INF, device=sim.device)
    index = torch.full((rows, topn), -1, dtype=torch.int64, device=sim.device)
    m = min(topn, cols)
    score[:, :m], index[:, :m] = val[:, :m], idx[:, :m]
    return score, index


def assert_is_sorted_sim(scores, indices, sim, topn, what=""):
    rs, ri = sorted_reference(sim.cpu(), topn)
    assert scores.dtype == torch.float32 and indices.dtype == torch.int64 and scores.is_cuda and indices.is_cuda
    assert torch.equal(indices.cpu(), ri), what
    m = min(topn, sim.shape[1])
    assert torch.equal(scores[:, :m], sim.gather(1, indices[:, :m])), f"{what}: scores are not bit-equal to eval_similarity's"
    assert torch.equal(scores.cpu(), rs), what


@pytest.mark.parametrize("use_frame_fea", [True, False])
@pytest.mark.parametrize("topn", [1, 10, 128])
@pytest.mark.parametrize("F", [12, 24])
def test_search_vs_unchanged_eval_path(model, problem, F, topn, use_frame_fea):  # noqa: F811
    p = problem(F)
    sim = p["sim"][use_frame_fea]
    assert sim.shape == (NQ, NV)
    for chunk_videos in (150, 64, 7):
        g = problem.gallery(F, chunk_videos)
        assert len(g) == NV and max(g.counts) <= chunk_videos
        for query_chunk in (4096, 32):
            scores, indices = model.search([p["q"][:20], p["q"][20:]], g, topn, use_frame_fea=use_frame_fea, query_chunk=query_chunk)
            assert_is_sorted_sim(scores, indices, sim, topn, what=f"chunk_videos={chunk_videos} query_chunk={query_chunk}")


@pytest.mark.parametrize("F", [12, 24])
def test_exact_ties_come_in_index_order(model, problem, F):  # noqa: F811
    p = problem(F)
    sim = p["sim"][True]
    for c in COPIES:
        assert torch.equal(sim[:, c], sim[:, 17]), "copies of a video must score identically"
    g = problem.gallery(F, 64)
    assert g.counts == [64, 64, 22]
    for topn in (10, 128):
        _, indices = model.search([p["q"]], g, topn)
        seen = 0
        for row in indices.cpu().tolist():
            pos = [row.index(c) for c in COPIES if c in row]
            got = [c for c in row if c in COPIES]
            assert got == sorted(got), row
            assert not pos or max(pos) - min(pos) == len(pos) - 1, "equal scores are neighbours in the list"
            seen += len(got)
        assert seen > 0


def test_incremental_add_equals_one_add(model, problem):  # noqa: F811
    p = problem(12)
    v, u = p["v"], p["u"]
    g = Gallery(model.top_frames, problem.gallery(12, 64).scale, chunk_videos=64)
    assert len(g) == 0
    assert g.add(v[:40], u[:40]) == (0, 40)
    assert g.add(v[40:41], u[40:41]) == (40, 41)
    assert g.add(v[41:], u[41:]) == (41, 150)
    assert len(g) == 150 and g.counts == [64, 64, 22]
    one = problem.gallery(12, 64)
    for a, b in zip(g.chunks, one.chunks):
        assert torch.equal(a, b)
    s1, i1 = g.search(p["q"], 10)
    s2, i2 = one.search(p["q"], 10)
    assert torch.equal(s1, s2) and torch.equal(i1, i2)
    assert_is_sorted_sim(s1, i1, p["sim"][True], 10)


@pytest.mark.parametrize("chunk_videos,query_chunk", [(150, 4096), (64, 32), (7, 32)])
def test_search_texts_is_the_sorted_transpose(model, problem, chunk_videos, query_chunk):  # noqa: F811
    p = problem(12)
    g = problem.gallery(12, chunk_videos)
    for fea in (True, False):
        simt = p["sim"][fea].t().contiguous()
        for topn in (1, 10, 70, 128):                       # 70 queries: 128 leaves (-inf, -1) tails
            scores, indices = g.search_texts(p["q"], topn, use_frame_fea=fea, query_chunk=query_chunk)
            assert scores.shape == (NV, topn)
            assert_is_sorted_sim(scores, indices, simt, topn, what=f"topn={topn}")


def test_topn_beyond_the_gallery_leaves_empty_tails(model, problem):  # noqa: F811
    p = problem(12)
    g = model.build_gallery([p["v"][:5]], [p["u"][:5]])
    scores, indices = model.search([p["q"]], g, 10)
    assert bool((indices[:, 5:] == -1).all()) and bool((scores[:, 5:] == -INF).all())
    assert_is_sorted_sim(scores, indices, p["sim"][True][:, :5].contiguous(), 10)
    empty = Gallery(K, 100.0)
    scores, indices = empty.search(p["q"], 3)
    assert bool((indices == -1).all()) and bool((scores == -INF).all()) and indices.shape == (NQ, 3)


def test_recall_from_topn_equals_compute_metrics(model):  # noqa: F811
    """the head_eval problem of test_gpu_eval.py (ground truth = the diagonal).  Checked on the CPU when this test was written:
    no row of the reference matrix (tests/golden/head_eval.npz, S_video + topk3) holds its diagonal value twice, so the
    strict-count rank of compute_metrics and the position in a list agree."""
    q = synth.normal("head_eval.q", (48, 512))
    v = synth.normal("head_eval.v", (48, 512))
    u = synth.normal("head_eval.u", (48, 12, 512))
    q = (q + 0.7 * v).to(DEV)
    v, u = v.to(DEV), u.to(DEV)
    model.top_frames = K
    sim = model.eval_similarity([q], [v], [u])
    full = M.compute_metrics(sim)
    _, indices = model.search([q], model.build_gallery([v], [u], chunk_videos=20), 10)
    got = M.recall_from_topn(indices)
    assert got == {k: full[k] for k in ("R1", "R5", "R10")}
    assert M.recall_from_topn(indices, target=torch.arange(48, dtype=torch.int32, device=DEV), ks=(1, 10)) == \
        {"R1": full["R1"], "R10": full["R10"]}
    with pytest.raises(ValueError):
        M.recall_from_topn(indices, ks=(1, 11))


def test_search_never_holds_the_score_matrix(model):  # noqa: F811
    nq, nv, F, e, topn = 4096, 16384, 3, 32, 10
    gen = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn(nq, e, device=DEV, generator=gen)
    v = torch.randn(nv, e, device=DEV, generator=gen)
    u = torch.randn(nv, F, e, device=DEV, generator=gen)
    model.top_frames = K
    g = model.build_gallery([v], [u], chunk_videos=2048)
    assert g.counts == [2048] * 8
    model.search([q], g, topn, query_chunk=512)                    # warm-up: the gallery's block buffer exists from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    scores, indices = model.search([q], g, topn, query_chunk=512)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"search peak above the level before it: {peak / 2 ** 20:.2f} MiB (score matrix: {nq * nv * 4 / 2 ** 20:.0f} MiB)")
    assert peak < nq * nv * 4 // 2
    sim = model.eval_similarity([q], [v], [u])
    rs, ri = sorted_reference(sim, topn)                           # on the device: 67 M scores
    assert torch.equal(indices, ri) and torch.equal(scores, rs)
    assert torch.equal(scores, sim.gather(1, indices))


def test_refusals_name_the_limit(model, problem):  # noqa: F811
    p = problem(12)
    g = Gallery(K, 100.0)
    with pytest.raises(ValueError, match="F <= 31"):
        g.add(torch.randn(3, E, device=DEV), torch.randn(3, 32, E, device=DEV))
    with pytest.raises(ValueError, match="F <= 31"):
        model.build_gallery([torch.randn(3, E, device=DEV)], [torch.randn(3, 32, E, device=DEV)])
    assert len(g) == 0
    g.add(p["v"][:4], p["u"][:4])
    with pytest.raises(ValueError, match="F = 12"):
        g.add(p["v"][:4], torch.randn(4, 24, E, device=DEV))
    with pytest.raises(ValueError, match="E = 512"):
        g.add(torch.randn(4, 256, device=DEV), torch.randn(4, 12, 256, device=DEV))
    assert len(g) == 4
    for call in (g.search, g.search_texts, lambda x, n: model.search([x], g, n)):
        with pytest.raises(ValueError, match="128"):
            call(p["q"], 129)
