"""GPU tests of hmmc_topn_select alone, on matrices the test supplies: the running top-N lists must equal, exactly, the first n
columns of the stable descending sort of the row (NaN as -inf), padded with (-inf, -1).

The reference keeps infinities as they are (torch.nan_to_num would otherwise turn them into the largest finite values):
x = S.nan_to_num(nan=-inf, posinf=inf, neginf=-inf);  torch.sort(x, dim=1, descending=True, stable=True)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hmmc_amd import _lib, ops  # noqa: E402

DEV = "cuda"
INF = float("inf")
NS = [1, 3, 10, 64, 128]


def reference(S_cpu, n, col_base=0):
    x = S_cpu.nan_to_num(nan=-INF, posinf=INF, neginf=-INF)
    val, idx = torch.sort(x, dim=1, descending=True, stable=True)
    rows, cols = x.shape
    score = torch.full((rows, n), -INF)
    index = torch.full((rows, n), -1, dtype=torch.int64)
    m = min(n, cols)
    score[:, :m] = val[:, :m]
    index[:, :m] = idx[:, :m] + col_base
    return score, index


def strided(S_cpu):
    """the matrix as columns 1 .. cols of a [rows, cols + 3] device tensor: ld = cols + 3, rows start on every residue mod 16 bytes"""
    rows, cols = S_cpu.shape
    big = torch.full((rows, cols + 3), 7e37, device=DEV)
    big[:, 1:cols + 1] = S_cpu.to(DEV)
    return big[:, 1:cols + 1]


def check(S_cpu, n, col_base=0, what=""):
    score, index = ops.topn_select(strided(S_cpu), n, col_base=col_base)
    rs, ri = reference(S_cpu, n, col_base)
    assert index.dtype == torch.int32 and score.dtype == torch.float32
    assert torch.equal(index.cpu().long(), ri), what
    assert torch.equal(score.cpu(), rs), what


@pytest.mark.parametrize("col_base", [0, 1000003])
@pytest.mark.parametrize("n", NS)
def test_sizes(n, col_base):
    gen = torch.Generator().manual_seed(100 * n + (col_base & 1))
    for cols in sorted({1, n - 1, n, n + 1, 63, 64, 65, 257, 1000, 4099}):        # n = 1: n - 1 = 0 columns, empty lists
        for rows in (1, 5, 67):
            S = torch.randn(rows, cols, generator=gen)
            S[::2] = (S[::2] * 4).round() / 4                                     # every other row: many exact ties
            check(S, n, col_base, what=f"n={n} cols={cols} rows={rows}")


@pytest.mark.parametrize("n", NS)
def test_rows_that_break_selection_kernels(n):
    gen = torch.Generator().manual_seed(7 + n)
    for cols in sorted({max(n - 1, 1), n + 1, 65, 1000, 4099}):
        asc = torch.arange(cols, dtype=torch.float32) - cols / 2                  # every element beats the list so far
        two = torch.randint(0, 2, (cols,), generator=gen).float() * 3 - 1
        # only n - 2 finite scores: the list's end is filled from the -inf and NaN columns, in index order
        few = torch.full((cols,), -INF)
        perm = torch.randperm(cols, generator=gen)
        few[perm[:max(n - 2, 0)]] = torch.randn(max(n - 2, 0), generator=gen)[:cols]
        few[perm[min(n, cols - 1)]] = float("nan")
        mixed = torch.randn(cols, generator=gen)                                  # one NaN, one -inf, +inf twice, both zeros
        mixed[perm[0]], mixed[perm[-1]] = float("nan"), -INF
        if cols >= 6:
            mixed[perm[1]] = mixed[perm[2]] = INF
            mixed[perm[3]], mixed[perm[4]] = 0.0, -0.0
        S = torch.stack([asc, asc.flip(0), torch.full((cols,), 1.5), two, few, mixed])
        check(S, n, 0, what=f"n={n} cols={cols}")
        check(S, n, 1000003, what=f"n={n} cols={cols} col_base")


def test_real_minus_inf_precedes_empty_slots():
    S = torch.tensor([[0.5, float("nan"), -INF, 2.0]])
    score, index = ops.topn_select(S.to(DEV), 10, col_base=5)
    assert index.cpu().tolist() == [[8, 5, 6, 7] + [-1] * 6]
    assert score.cpu().tolist() == [[2.0, 0.5, -INF, -INF] + [-INF] * 6]


@pytest.mark.parametrize("n", [1, 10, 128])
def test_merging_is_independent_of_the_cut_and_the_order(n):
    gen = torch.Generator().manual_seed(11)
    rows, widths = 5, (1, 63, 64, 129, 743)
    S = (torch.randn(rows, 1000, generator=gen) * 4).round() / 4
    S[:, 0] = S[:, 1] = 50.0                                   # one duplicated value either side of every block boundary
    S[:, 63] = S[:, 64] = 40.0
    S[:, 127] = S[:, 128] = 50.0
    S[:, 256] = S[:, 257] = -0.25
    Sd = S.to(DEV)
    whole = ops.topn_select(Sd, n)
    starts = [sum(widths[:i]) for i in range(len(widths))]
    assert starts[-1] + widths[-1] == 1000
    results = []
    for order in (range(len(widths)), reversed(range(len(widths)))):
        out = None
        for b in order:
            block = Sd[:, starts[b]:starts[b] + widths[b]]     # a strided, mostly unaligned view
            if out is None:
                out = ops.topn_select(block, n, col_base=starts[b])
            else:
                got = ops.topn_select(block, n, col_base=starts[b], out=out)
                assert got[0] is out[0] and got[1] is out[1]
        results.append(out)
    rs, ri = reference(S, n)
    for score, index in [whole] + results:
        assert torch.equal(index.cpu().long(), ri) and torch.equal(score.cpu(), rs)
        assert torch.equal(score, whole[0]) and torch.equal(index, whole[1])


def test_arguments_are_refused_before_any_launch():
    S = torch.randn(4, 40, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.topn_select(S, 0)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.topn_select(S, 129)
    assert ops.TOPN_MAX == 128
    score = torch.full((4, 8), 3.0, device=DEV)
    index = torch.full((4, 8), 9, dtype=torch.int32, device=DEV)
    args = lambda cols, ld, base, n: (_lib.ptr(S), 4, cols, ld, base, _lib.ptr(score), _lib.ptr(index), n, 0)  # noqa: E731
    assert _lib.call_status("hmmc_topn_select", *args(40, 40, 0, 129), allow="HMMC_ERR_UNSUPPORTED") == _lib.STATUS["HMMC_ERR_UNSUPPORTED"]
    for bad in (args(40, 39, 0, 8), args(40, 40, 0, 0), args(40, 40, -1, 8), args(40, 40, 2 ** 31 - 40, 8)):
        assert _lib.call_status("hmmc_topn_select", *bad, allow="HMMC_ERR_ARG") == _lib.STATUS["HMMC_ERR_ARG"]
    torch.cuda.synchronize()
    assert bool((score == 3.0).all()) and bool((index == 9).all()), "a refused call must not launch"
    assert _lib.call_status("hmmc_topn_select", *args(40, 40, 2 ** 31 - 41, 8)) == 0      # col_base + cols = INT_MAX: allowed
    assert 2 ** 31 - 41 <= int(index.min()) and int(index.max()) <= 2 ** 31 - 2
    with pytest.raises(TypeError):
        ops.topn_select(S.double(), 3)
    with pytest.raises(ValueError):
        ops.topn_select(S.t(), 3)
