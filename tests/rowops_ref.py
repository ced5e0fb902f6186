"""Plain statements of the row and elementwise ops of hmmc_amd/csrc/norm_elem.hip besides LayerNorm - hmmc_colsum, hmmc_patchify,
hmmc_patchify_u8, hmmc_vit_embed, hmmc_text_embed, hmmc_text_embed_bwd, hmmc_eot_index, hmmc_cast - and the per-element bounds
tests/test_gpu_rowops.py holds the HIP kernels to.  tests/test_rowops_reference.py pins each statement against an independent
formulation, shows with a torch emulation of each accumulating kernel's summation order that the bounds are not too tight, and
with test_slip_* that a plausible kernel mistake is seen.  U, SLACK are those of heads_ref, U16 and the helpers those of hotpath_ref.

Gather, layout and rounding ops (patchify, patchify_u8, vit_embed, text_embed, cast, eot_index) accumulate nothing: the
comparison is torch.equal with a torch statement that rounds where the kernel rounds.
  fp16 forms   table, position and class values are rounded to fp16 BEFORE the add, the sum is rounded to fp16 again (the sum of
               two fp16 values formed in fp32 and rounded to fp16 is the correctly rounded sum: 24 >= 2 x 11 + 2 bits)
  fp32 forms   nothing is rounded: one fp32 add
  patchify_u8  ((float) byte / 255 - mean[c]) / std[c], every step in fp32 (the data loader's ToTensor + Normalize)

Accumulating ops (colsum, text_embed_bwd) are compared with the fp64 sum.  Error model: inputs are exact (fp16 -> fp32 is exact),
a sum formed as chains of at most c dependent fp32 additions is within c U sum|terms|; an fp16 output (or round_f16) adds one
rounding, U16 |sum|.  c is read off the kernels:
  colsum, two launches   colsum_partial_kernel: a row lane takes the rows r0 + rl + 8 k of its slab of rpb rows, two per step
                         (acc += x[k] + x[k + 1]: ceil(ceil(rpb / 8) / 2) additions to acc behind the one of the pair), then the
                         8 row lanes are added in order (8).  colreduce_kernel over the rb slab rows: two accumulators per row
                         lane (ceil(rb / 16) additions each), their sum (1), the 8 row lanes in order (8)
  colsum, one launch     dense fp32 input of at most 512 rows: colreduce_kernel alone over the M rows
  text_embed_bwd         the 8 waves of the owning workgroup each add every 8th listed occurrence, batch after batch into the
                         same accumulator (ceil(n_b / 8) <= n_b / 8 + 1 per batch of n_b), then the 8 waves in order (7).  A
                         batch ends when the 16 384-entry list cannot take the next 512-row chunk (it then holds more than
                         16 384 - 512 occurrences) or when the next chunk would pass a 16-bit offset (it then spans more than
                         65 536 - 512 rows), which bounds the number of batches
The bound has no term for fp16's subnormal step.  It needs none: the bounded input families keep |x| >= 0.25, so wherever a sum
is rounded to fp16, c U sum|x| >= 10 x 2^-24 x 0.25 > 2^-25, half a subnormal step (c >= 10 in every plan).
On the "exact" family (integers -4 .. 4, every partial sum below 2^24) every fp32 sum is exact and the comparison is torch.equal.
Bounds are functions of the fp64 reference and the inputs only, never of a kernel's output.  Plain functions, no fixtures."""
from __future__ import annotations

import math
import os
import re

import torch

from heads_ref import SLACK, U  # noqa: F401  (re-exported for the tests)
from hotpath_ref import U16, detects, within_ratio  # noqa: F401

D64 = torch.float64
F16, F32 = torch.float16, torch.float32

# ---- the constants of norm_elem.hip the cases below are sized by; test_rowops_reference.py compares them with the source
BLOCK = 256                   # threads of an elementwise block
PATCHIFY_CAP = 8192           # blocks of a patchify / patchify_u8 launch at most (one 16-byte chunk per thread and sweep)
EMBED_CAP = 4096              # vit_embed, text_embed
CAST_CAP = 2048               # cast (one element per thread and sweep)
TE_THREADS, TE_WAVES, TE_LIST = 512, 8, 16384
TE_WINDOW = 65536             # rows a list batch spans at most (16-bit offsets)
COLSUM_SLAB_ROWS, COLSUM_MAX_SLABS, COLSUM_DIRECT_MAX = 64, 1024, 512
EOT_MAX_L = 1024

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hmmc_amd", "csrc", "norm_elem.hip")


def kernel_constants(path=SOURCE):
    """the same constants as norm_elem.hip states them -> dict; a pattern that no longer matches raises (the cases that rely on
    a grid cap or a threshold then fail loudly instead of silently testing less)"""
    src = open(path).read()

    def only(pattern, what):
        found = set(re.findall(pattern, src))
        assert len(found) == 1, f"{what}: expected one value in norm_elem.hip, found {sorted(found)}"
        return found.pop()
    te = only(r"TE_THREADS = (\d+), TE_WAVES = (\d+), TE_LIST = (\d+);", "text_embed_bwd constants")
    return dict(
        BLOCK=int(only(r"inline int grid_for\(long work_items, int block = (\d+), int cap = \d+\)", "block size")),
        PATCHIFY_CAP=int(only(r"grid_for\(total, 256, (\d+)\)", "patchify grid cap")),
        EMBED_CAP=int(only(r"grid_for\(rows \* \(D / 8\), 256, (\d+)\)", "embed grid cap")),
        CAST_CAP=int(only(r"inline int grid_for\(long work_items, int block = \d+, int cap = (\d+)\)", "default grid cap")),
        TE_THREADS=int(te[0]), TE_WAVES=int(te[1]), TE_LIST=int(te[2]),
        TE_WINDOW=int(only(r"base \+ TE_THREADS - start > (\d+)", "list window")),
        COLSUM_SLAB_ROWS=int(only(r"int rb = \(M \+ \d+\) / (\d+);", "rows per slab")),
        COLSUM_MAX_SLABS=int(only(r"if \(rb > (\d+)\) rb = \d+;", "slab cap")),
        COLSUM_DIRECT_MAX=int(only(r"in_dtype != 0 && ld == N && M <= (\d+)", "one-launch threshold")),
        EOT_MAX_L=int(only(r"L <= 0 \|\| L > (\d+)", "longest caption")),
    )


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


FAMILIES = ("signed", "same")          # the bounded families; "exact" is compared with torch.equal


def values(family, shape, g, device="cpu"):
    """fp32 values of one input family (exact in fp16 only after .half(); the tests convert before they take the reference)
      signed  +-(0.25 + |N(0, 1)|): cancellation exposes sign and index slips
      same    [0.25, 1]: sum|x| = |sum x|, the fp32 bound is c U relative
      exact   integers -4 .. 4: every partial sum of up to 2^21 terms is exact in fp32"""
    if family == "signed":
        r = torch.randn(shape, generator=g, device=device)
        return torch.where(r < 0, r - 0.25, r + 0.25)
    if family == "same":
        return 0.25 + 0.75 * torch.rand(shape, generator=g, device=device)
    assert family == "exact", family
    return torch.randint(-4, 5, shape, generator=g, device=device).float()


# ============================================================================= gather, layout and rounding ops

def patchify(img, p, dtype, swap=False):
    """img [n, 3, H, H] fp32 -> [n (g g + 1), 3 p p] in `dtype`, g = H / p: per frame a zero row (the class-token slot), then
    patch (gy, gx) in row 1 + gy g + gx with its pixels in (c, ky, kx) order - the input rows of conv1 (kernel = stride = p,
    weight [width, 3, p, p]; modules/module_clip.py:307-310).  swap: ky and kx exchanged (test_slip_*)."""
    n, c, H, W = img.shape
    assert c == 3 and H == W and H % p == 0
    g = H // p
    x = img.reshape(n, 3, g, p, g, p)                                    # [n, c, gy, ky, gx, kx]
    x = x.permute(0, 2, 4, 1, 5, 3) if swap else x.permute(0, 2, 4, 1, 3, 5)
    x = x.reshape(n, g * g, 3 * p * p)
    zero = torch.zeros(n, 1, 3 * p * p, dtype=img.dtype, device=img.device)
    return torch.cat([zero, x], 1).reshape(n * (g * g + 1), 3 * p * p).to(dtype)


def normalise_u8(u8, mean, std):
    """uint8 [n, 3, H, W] -> fp32: ToTensor (x / 255) and Normalize ((x - mean[c]) / std[c]), each step in fp32
    (dataloaders/dataloader_msrvtt_retrieval.py:242-247).  The tests evaluate it on the CPU (IEEE division)."""
    m = torch.tensor(mean, dtype=F32, device=u8.device).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=F32, device=u8.device).view(1, 3, 1, 1)
    return (u8.float().div(255.0) - m) / s


def patchify_u8(frames_f32, frame_index, p, dtype):
    """patchify of the normalised stored frames frame_index names (None: all of them, in order)"""
    return patchify(frames_f32 if frame_index is None else frames_f32[frame_index.long()], p, dtype)


def rnd(x, dtype):
    """what a value becomes when the reference holds it in a tensor of `dtype`, as fp32"""
    return x.to(dtype).float()


def vit_embed(x, cls, pos, L, add_cls=False, once=False):
    """x [rows, D] (fp16 or fp32): the class rows (row % L == 0) become cls, whatever they held; every row gets pos[row % L]
    (modules/module_clip.py:311-312).  fp16: rnd(rnd(t) + rnd(pos)).  add_cls: the class value is ADDED to the class row; once:
    the unrounded fp32 values are added and the sum is rounded once (test_slip_*)."""
    T = x.dtype
    rows, D = x.shape
    l = torch.arange(rows, device=x.device) % L
    t = x.float()
    c = cls.float() if once else rnd(cls, T)
    is_cls = (l == 0)[:, None]
    t = torch.where(is_cls, (t + c) if add_cls else c.expand_as(t), t)
    p = pos.float()[l] if once else rnd(pos, T)[l]
    return (t + p).to(T)


def text_embed(ids, table, pos, dtype, once=False):
    """ids [b, L] -> [b L, D]: rnd(table[id]) + rnd(pos[l]), rounded to `dtype` (modules/module_cross.py:288-291); an id outside
    the table never indexes it: its row is the position embedding alone -> (x, any id outside)"""
    b, L = ids.shape
    vocab = table.shape[0]
    ok = (ids >= 0) & (ids < vocab)
    tv = table.float()[ids.clamp(0, vocab - 1)] * ok[..., None]
    if once:
        return (tv + pos.float()[:L]).to(dtype).reshape(b * L, -1), bool((~ok).any())
    return (rnd(tv, dtype) + rnd(pos, dtype)[:L]).to(dtype).reshape(b * L, -1), bool((~ok).any())


def eot_index(ids, base=0, stride=None, last=False):
    """int32 [b]: base + i stride + the FIRST position of row i's largest id (last: the last one, test_slip_*)"""
    b, L = ids.shape
    stride = L if stride is None else stride
    top = ids.max(1, keepdim=True).values
    posn = torch.arange(L, device=ids.device).expand(b, L)
    if last:
        first = torch.where(ids == top, posn, torch.full_like(posn, -1)).max(1).values
    else:
        first = torch.where(ids == top, posn, torch.full_like(posn, L)).min(1).values
    return (base + torch.arange(b, device=ids.device) * stride + first).to(torch.int32)


def eot_ids(b, L, shift, seed=0):
    """[b, L] int64 captions; row i follows pattern (i + shift) % 8 (L = 1: every pattern is the one-token row)
      0  a unique largest id at a random position          1  the largest id twice in ONE lane's positions (l and l + 64; L <= 64:
      2  the largest id at l and l + 1: neighbouring lanes     positions 0 and L - 1)
      3  the largest id at 0 and again at L - 1            4  a unique largest id at L - 1
      5  every id equal                                    6  negative ids only, the largest (-3) at two positions
      7  the largest id at L - 1 and at every 7th position from a random one on"""
    g = gen(1000 * seed + 31 * L + 7 * b + shift)
    ids = torch.randint(1, 40000, (b, L), generator=g)
    top = 49407
    for i in range(b):
        pat = (i + shift) % 8
        l = int(torch.randint(0, L, (1,), generator=g))
        if pat == 0:
            ids[i, l] = top
        elif pat == 1:
            lo = l % (L - 64) if L > 64 else 0
            ids[i, lo] = top
            ids[i, lo + 64 if L > 64 else L - 1] = top
        elif pat == 2:
            l = min(l, max(L - 2, 0))
            ids[i, l] = top
            ids[i, min(l + 1, L - 1)] = top
        elif pat == 3:
            ids[i, 0] = top
            ids[i, L - 1] = top
        elif pat == 4:
            ids[i, L - 1] = top
        elif pat == 5:
            ids[i] = 320
        elif pat == 6:
            ids[i] = -torch.randint(4, 40000, (L,), generator=g)
            ids[i, l] = -3
            ids[i, (l + 65) % L if (l + 65) % L != l else (l + 1) % L] = -3
        else:
            ids[i, L - 1] = top
            ids[i, l::7] = top
    return ids


# ============================================================================= colsum

COLSUM_M = [1, 7, 8, 9, 16, 17, 63, 64, 65, 512, 513, 4097, 65537]
COLSUM_WIDE = 38400           # 50 x 768: the positional-embedding gradient of ViT-B/32
COLSUM_WIDE_M = (1, 9, 65, 513)


def colsum_widths(M, dtype):
    """the widths the GPU test runs at M rows: the vector width itself, 264 (33 fp16 chunks: a partial 32-chunk column block, and
    8.25 blocks of 32 columns in the second stage), 768, and 38 400 at a few M; at 65 537 rows the two narrow ones"""
    vn = 8 if dtype == F16 else 4
    w = [vn, 264] if M > 4097 else [vn, 264, 768]
    return w + [COLSUM_WIDE] if M in COLSUM_WIDE_M else w


def colsum(x):
    return x.to(D64).sum(0)


def colsum_plan(M, dtype, dense=True):
    """hmmc_colsum's host arithmetic -> dict(direct, rb, rpb): one launch (colreduce over the M rows) for dense fp32 input of
    at most 512 rows, else rb slabs of rpb rows (at least 64 rows per slab, at most 1024 slabs, rb recomputed from rpb)"""
    if dtype == F32 and dense and M <= COLSUM_DIRECT_MAX:
        return dict(direct=True, rb=1, rpb=M)
    rb = min(max((M + COLSUM_SLAB_ROWS - 1) // COLSUM_SLAB_ROWS, 1), COLSUM_MAX_SLABS)
    rpb = (M + rb - 1) // rb
    return dict(direct=False, rb=(M + rpb - 1) // rpb, rpb=rpb)


def colsum_workspace(M, N):
    """bytes hmmc_colsum_workspace reports: the slab count BEFORE it is recomputed"""
    return min(max((M + COLSUM_SLAB_ROWS - 1) // COLSUM_SLAB_ROWS, 1), COLSUM_MAX_SLABS) * N * 4


def colsum_chain(plan):
    """c: the longest chain of dependent fp32 additions the two stages can form (module docstring)"""
    def reduce(R):
        return math.ceil(R / 16) + 1 + 8
    if plan["direct"]:
        return reduce(plan["rpb"])
    return math.ceil(math.ceil(plan["rpb"] / 8) / 2) + 1 + 8 + reduce(plan["rb"])


def colsum_bound(x64, ref, plan, half):
    """c U sum_m |x[m][n]| per column, + U16 |sum| when the sum is rounded to fp16 (fp16 output or round_f16)"""
    b = colsum_chain(plan) * U * x64.abs().sum(0)
    return b + U16 * ref.abs() if half else b


def _colreduce(p):
    """colreduce_kernel's order over the fp32 rows p [R, N]: row lane rl adds the rows rl + 16 i into a0 and rl + 8 + 16 i into
    a1, a0 + a1, then the 8 row lanes in order.  (Rows past R are zeros here: x + 0 is exact.)"""
    R, N = p.shape
    K = (R + 15) // 16
    q = torch.cat([p, torch.zeros(K * 16 - R, N, dtype=F32)]).reshape(K, 2, 8, N)
    a0, a1 = torch.zeros(8, N, dtype=F32), torch.zeros(8, N, dtype=F32)
    for i in range(K):
        a0, a1 = a0 + q[i, 0], a1 + q[i, 1]
    red = a0 + a1
    t = torch.zeros(N, dtype=F32)
    for k in range(8):
        t = t + red[k]
    return t


def emulate_colsum(x, plan, out_dtype, round_f16):
    """hmmc_colsum's arithmetic in fp32 torch on the CPU, in the kernels' summation order -> [N] in out_dtype"""
    M, N = x.shape
    xf = x.float()
    if plan["direct"]:
        t = _colreduce(xf)
    else:
        rb, rpb = plan["rb"], plan["rpb"]
        K = (rpb + 15) // 16
        flat = torch.zeros(rb * rpb, N, dtype=F32)
        flat[:M] = xf
        buf = torch.zeros(rb, K * 16, N, dtype=F32)
        buf[:, :rpb] = flat.reshape(rb, rpb, N)
        q = buf.reshape(rb, K, 2, 8, N)                                # slab row = 16 i + 8 j + rl
        acc = torch.zeros(rb, 8, N, dtype=F32)
        for i in range(K):
            acc = acc + (q[:, i, 0] + q[:, i, 1])
        part = torch.zeros(rb, N, dtype=F32)
        for k in range(8):
            part = part + acc[:, k]
        t = _colreduce(part)
    if round_f16:
        t = t.half().float()
    return t.to(out_dtype)


COLSUM_SLIPS = ("tail_row", "short_slab", "acc_f16")


def colsum_slipped(x64, plan, slip):
    """the fp64 column sum with one plausible mistake, or None where the mistake has no effect at this shape
      tail_row    the first stage's `if (r < r1)`: a row lane with an odd number of rows in its slab loses the last one
      short_slab  the last slab is dropped when it is shorter than the others (two launches only)
      acc_f16     the running sum is kept in fp16"""
    M, N = x64.shape
    rpb = plan["rpb"]
    if slip == "tail_row":
        keep = torch.ones(M, dtype=torch.bool)
        for r0 in range(0, M, rpb):
            n = min(rpb, M - r0)
            for rl in range(min(8, n)):
                cnt = (n - rl + 7) // 8
                if cnt % 2:
                    keep[r0 + rl + 8 * (cnt - 1)] = False
        return (x64 * keep[:, None]).sum(0)
    if slip == "short_slab":
        if plan["direct"] or M % rpb == 0:
            return None
        return x64[:M - M % rpb].sum(0)
    assert slip == "acc_f16", slip
    run = torch.zeros(N, dtype=F16)
    for m in range(M):
        run = (run.float() + x64[m].float()).half()
    return run.to(D64)


# ============================================================================= text_embed_bwd

def text_embed_bwd(ids, dx, vocab):
    """dtable [vocab, D] fp64: row id = the sum of dx's rows r with ids[r] == id; ids outside [0, vocab) contribute nothing"""
    ids = ids.reshape(-1)
    ok = (ids >= 0) & (ids < vocab)
    out = torch.zeros(vocab, dx.shape[-1], dtype=D64, device=dx.device)
    return out.index_add_(0, ids[ok], dx.to(D64)[ok])


def te_counts(ids, vocab):
    ids = ids.reshape(-1)
    ok = (ids >= 0) & (ids < vocab)
    return torch.bincount(ids[ok], minlength=vocab)


def te_chain(n, rows):
    """c for an id with n occurrences among `rows` rows (module docstring); n: int64 tensor [vocab]"""
    nbatch = n // (TE_LIST - TE_THREADS + 1) + rows // (TE_WINDOW - TE_THREADS + 1) + 1
    return (n + 7) // 8 + nbatch + 7


def text_embed_bwd_bound(ids, dx, vocab):
    """c U sum over the occurrences of |dx| per table element; rows of ids that never occur: 0"""
    rows = ids.numel()
    c = te_chain(te_counts(ids, vocab), rows).to(D64)
    return c[:, None] * U * text_embed_bwd(ids, dx.to(D64).abs(), vocab)


def te_batches(hits, rows):
    """the list batches of the workgroup that owns an id: hits = the sorted rows holding it (numpy int64, hits[0] the owner).
    A batch starts at `start`, takes 512-row chunks while the chunk stays within 65 536 rows of `start` and the list has room
    for ALL of its hits, and ends in front of the first chunk that does not -> [array of the rows of each batch]"""
    import numpy as np
    out, start = [], int(hits[0])
    while start < rows:
        cnt, nxt, base = 0, rows, start
        while base < rows:
            if base + TE_THREADS - start > TE_WINDOW:
                nxt = base
                break
            tot = int(np.searchsorted(hits, base + TE_THREADS) - np.searchsorted(hits, base))
            if cnt + tot > TE_LIST:
                nxt = base
                break
            cnt += tot
            base += TE_THREADS
        out.append(hits[np.searchsorted(hits, start):np.searchsorted(hits, nxt)])
        start = nxt
    return out


def emulate_text_embed_bwd(ids, dx, vocab, first_batch_only=False):
    """text_embed_bwd_kernel's arithmetic in fp32 torch on the CPU -> [vocab, D] fp32.  Wave w adds the list entries w, w + 8, ..
    of every batch into one accumulator, then the waves are added in order.  first_batch_only: test_slip_*."""
    ids = ids.reshape(-1)
    rows, D = ids.numel(), dx.shape[-1]
    xf = dx.float()
    out = torch.zeros(vocab, D, dtype=F32)
    idn = ids.numpy()
    for v in range(vocab):
        hits = (idn == v).nonzero()[0]
        if hits.size == 0:
            continue
        acc = torch.zeros(TE_WAVES, D, dtype=F32)
        batches = te_batches(hits, rows)
        for occ in (batches[:1] if first_batch_only else batches):
            n = occ.size
            K = (n + 7) // 8
            sel = torch.zeros(K * 8, D, dtype=F32)
            sel[:n] = xf[torch.from_numpy(occ)]
            sel = sel.reshape(K, 8, D)
            for i in range(K):
                acc = acc + sel[i]
        s = acc[0]
        for w in range(1, TE_WAVES):
            s = s + acc[w]
        out[v] = s
    return out


def te_pattern(rows, vocab, heavy, first, seed):
    """ids [rows] int64 on the CPU: random ids of [1, vocab - 1) (the last id of the table never occurs), a few outside the
    table (row 0 always: the heavy id may take the other rows), and the heavy id 0 where `heavy(r)` (a bool tensor over the rows)
    says, never in front of row `first` > 0"""
    g = gen(seed)
    ids = torch.randint(1, vocab - 1, (rows,), generator=g)
    ids[torch.randint(0, rows, (5,), generator=g)] = torch.tensor([-1, vocab, vocab + 7, -2 ** 40, 2 ** 40])
    r = torch.arange(rows)
    ids[heavy(r) & (r >= first)] = 0
    assert first > 0
    ids[0] = -1
    return ids


def _two_in_three(count=None, first=5):
    """heavy id on the rows r >= first with r % 3 != 2, cut after `count` occurrences: 48 chunks of 512 rows hold exactly 16 384"""
    def f(r):
        m = (r % 3 != 2) & (r >= first)
        if count is not None:
            m = m & (torch.cumsum(m.long(), 0) <= count)
        return m
    return f


# name -> (rows, vocab, heavy, first row of the heavy id): D = 8 in all of them
TE_LONG_CASES = {
    "n16384": (30000, 24, _two_in_three(16384), 5),          # exactly one full list: `base_cnt + tot <= TE_LIST` with equality
    "n16385": (30000, 24, _two_in_three(16385), 5),          # one occurrence more: a second batch of one
    # three rows in five, ~39 000 occurrences inside one 65 536-row window: 307 or 308 per chunk, which does not divide 16 384 -
    # every batch ends in the middle of the occurrences, with room left in the list
    "n39k": (65000, 24, lambda r: r % 5 < 3, 5),
    "dense": (40000, 24, lambda r: r >= 7, 7),               # every row from 7 on: 512 hits per chunk, batches end on a full list
    # more than 65 536 rows and more than 16 384 occurrences per window: one in eight up to row 70 000 (the window ends the batch
    # there, 8 192 listed), three in five behind it (the list ends the batches); the other ids end theirs at the window
    "both_limits": (150000, 24, lambda r: torch.where(r < 70000, r % 8 == 3, r % 5 < 3), 3),
}
# (rows, vocab, D): the column-block loop.  D = 520 and 768 run a second block (8 and 256 columns of it), 512 exactly one
TE_WIDE_CASES = [(1500, 40, D) for D in (8, 512, 520, 768)]


def te_wide_ids(rows, vocab, seed=0):
    """random ids with a heavy id 3 on two rows in five (from row 11 on), the last id of the table unused, a few outside it"""
    g = gen(seed + rows + vocab)
    ids = torch.randint(0, vocab - 1, (rows,), generator=g)
    r = torch.arange(rows)
    ids[(r % 5 < 2) & (r >= 11)] = 3
    ids[torch.randint(0, rows, (4,), generator=g)] = torch.tensor([-1, vocab, -7, 2 ** 33])
    ids[0] = vocab - 2
    return ids


# ============================================================================= cast

def cast_values(n, to_half, seed=0):
    """n values of the source type (fp32 when to_half) with the awkward ones in front (as many as fit): ties that round to even
    and to odd's neighbour, the largest finite fp16 and the first value that overflows to inf, fp16 subnormals and values below
    half the smallest one, signed zeros, infinities"""
    g = gen(seed + n)
    if to_half:
        special = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 2049.0, 2051.0, 65504.0, 65519.99,
                                65520.0, -65520.0, 1e30, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,
                                6e-8, 1e-10, -0.0, 0.0, float("inf"), float("-inf"), -2.0 ** -24, 5.5e-5], dtype=F32)
        body = torch.randn(n, generator=g) * torch.tensor(10.0) ** torch.randint(-8, 5, (n,), generator=g).float()
        body[:min(n, special.numel())] = special[:n]
        return body
    special = torch.tensor([65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 0.0, -0.0, float("inf"),
                            float("-inf"), 1.0009765625], dtype=F16)
    body = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g).to(torch.int16).view(F16)
    body = torch.where(torch.isnan(body), torch.ones_like(body), body)
    body[:min(n, special.numel())] = special[:n]
    return body


def same_bits(a, b):
    """equal bit for bit (torch.equal treats -0 and +0 alike)"""
    it = torch.int16 if a.dtype == F16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))
