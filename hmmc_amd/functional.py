"""torch.autograd.Function shims over the HIP kernels, one per fused stage of the hot path, so
DDP and the optimizer see ordinary parameter gradients.  Activations are kept token-major
([tokens, D], a sequence's tokens contiguous); the reference's LND layout is a pure permutation.

Stage -> reference lines:
  VitEmbedFn        modules/module_clip.py:307-313   conv1 patchify, class token, pos-emb, ln_pre
  TextEmbedFn       modules/module_cross.py:288-291  token embedding + positional embedding
  ClipTransformerFn modules/module_clip.py:231-268   N x ResidualAttentionBlock (fp16 tower)
  LnProjFn          modules/module_cross.py:228-237,296-305   ln_post/ln_final + projection (+ row pick)
  TemporalFn        modules/module_cross.py:193-212  frame pos-emb, 4 fp32 blocks, residual, normalise, mean
  FinetuneHeadFn    modules/modeling.py:665-672,702-709       hierarchical InfoNCE
"""
from __future__ import annotations

import os

import torch

from . import ops

PER_LAYER = 12   # parameters of one ResidualAttentionBlock, in the order of block_params()


def block_params(block):
    """Flat parameter list of a ResidualAttentionBlock (names as in the reference state_dict)."""
    return [block.ln_1.weight, block.ln_1.bias, block.attn.in_proj_weight, block.attn.in_proj_bias,
            block.attn.out_proj.weight, block.attn.out_proj.bias, block.ln_2.weight, block.ln_2.bias,
            block.mlp.c_fc.weight, block.mlp.c_fc.bias, block.mlp.c_proj.weight, block.mlp.c_proj.bias]


def _wgrad16(dy, x):
    """dW[N',K'] = dy[T,N']^T x[T,K'] (fp16, split-K over tokens)."""
    T, Np = dy.shape
    return ops.gemm_f16(dy, x, Np, x.shape[1], T, a_kmajor=False, b_kmajor=False)


def _dgrad16(dy, w, aux_in=None, epilogue=0):
    """dx[T,K'] = dy[T,N'] w[N',K']."""
    T, Np = dy.shape
    return ops.gemm_f16(dy, w, T, w.shape[1], Np, a_kmajor=True, b_kmajor=False, aux_in=aux_in, epilogue=epilogue)


# The CLIP towers run in the dtype of their weights: fp16 as the reference builds them (convert_weights), or fp32 after
# model.float() (the reference's fp32-upcast regime, modules/module_clip.py:566-577 + .float()): the same stages on the
# exact-f32 MFMA GEMM, fp32 LayerNorm / attention / embeddings, nothing rounded to fp16.  A parity regime: correct, not tuned.
def _linear(x, w):
    """x[M,K] w[N,K]^T in the operands' dtype."""
    if x.dtype != w.dtype:
        raise RuntimeError(f"expected the activations ({x.dtype}) and the weights ({w.dtype}) to have the same dtype: after "
                           "model.float() set text_encoder.dtype = torch.float32 as well, as with the reference")
    if w.dtype == torch.float16:
        return ops.gemm_f16(x, w, x.shape[0], w.shape[0], x.shape[1])
    return ops.linear_f32(x, w)


def _wgrad(dy, x):
    return _wgrad16(dy, x) if dy.dtype == torch.float16 else ops.wgrad_f32(dy, x)


# The im2col of a step's frames depends on the frames alone.  The pre-training model encodes the SAME frames with the online and
# the momentum tower (reference modules/modeling.py:347,356): inside `share_patches()` the second VitEmbedFn call on the same
# tensor (same storage, version, stream, patch size and dtype) takes the first one's patch matrix instead of re-reading the video.
# `ref` keeps the keyed frames alive while their patches are shared, so the caching allocator cannot hand the same address to a
# different batch inside the window.
_PATCH_SHARE = {"on": False, "key": None, "val": None, "ref": None}


class share_patches:
    def __enter__(self):
        _PATCH_SHARE.update(on=True, key=None, val=None, ref=None)
        return self

    def __exit__(self, *exc):
        _PATCH_SHARE.update(on=False, key=None, val=None, ref=None)
        return False


def _patches_of(video4d, p, dtype, frame_index):
    key = None
    if _PATCH_SHARE["on"] and video4d.is_cuda and not os.environ.get("HMMC_NO_PATCH_SHARE"):
        key = (video4d.data_ptr(), video4d._version, tuple(video4d.shape), video4d.dtype, p, dtype,
               None if frame_index is None else (frame_index.data_ptr(), frame_index._version, tuple(frame_index.shape)),
               torch.cuda.current_stream(video4d.device).cuda_stream)
        if _PATCH_SHARE["key"] == key:
            return _PATCH_SHARE["val"]
    if video4d.dtype == torch.uint8:
        patches = ops.patchify_u8(video4d, p, frame_index=frame_index, dtype=dtype)
    else:
        if frame_index is not None:
            raise TypeError("frame sampling on the device takes the stored uint8 frames")
        patches = ops.patchify(video4d, p, dtype=dtype)
    if key is not None:
        _PATCH_SHARE.update(key=key, val=patches, ref=video4d)
    return patches


class VitEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, video4d, conv_w, cls, pos, ln_w, ln_b, frame_index=None, want_stat=False):
        n = video4d.shape[0] if frame_index is None else frame_index.numel()
        D, _, p, _ = conv_w.shape
        L = pos.shape[0]
        # [n*L, 3pp] in the conv weight's dtype (image.type(self.dtype), modules/module_cross.py:224), class rows zero; uint8
        # frames are normalised on the fly (CLIP mean / std) and, with a frame index, picked out of the stored frames in place
        # (the loader's frame sampling)
        patches = _patches_of(video4d, p, conv_w.dtype, frame_index)
        x0 = _linear(patches, conv_w.view(D, -1))
        stat = None
        if x0.dtype == torch.float16:                 # class / positional embedding and ln_pre in one pass (bit-identical)
            x, mean, rstd, stat = ops.vit_embed_ln_(x0, cls, pos, ln_w, ln_b, L, want_stat=want_stat)
        else:
            ops.vit_embed_(x0, cls, pos, L)
            x, mean, rstd = ops.layernorm_fwd(x0, ln_w, ln_b, 1e-5)
        ctx.save_for_backward(patches, x0, mean, rstd, ln_w, conv_w)
        ctx.dims = (n, L, D, p)
        if stat is None:
            return x
        ctx.mark_non_differentiable(stat)             # the row pairs of x for a folded tower (a by-product, no gradient)
        return x, stat

    @staticmethod
    def backward(ctx, dx, _dstat=None):
        patches, x0, mean, rstd, ln_w, conv_w = ctx.saved_tensors
        n, L, D, p = ctx.dims
        dx0, dlw, dlb = ops.layernorm_bwd(dx.contiguous(), x0, ln_w, mean, rstd)
        dconv = _wgrad(dx0, patches).view(conv_w.shape)
        dpos = ops.colsum(dx0.view(n, L * D), out_dtype=torch.float32, round_f16=dx0.dtype == torch.float16).view(L, D)
        return None, dconv, dpos[0].clone(), dpos, dlw, dlb, None, None


def vit_embed(video4d, conv_w, cls, pos, ln_w, ln_b, frame_index=None):
    """VitEmbedFn.apply -> (x, row statistics of x or None).  Passes that record no graph in fp16 skip the autograd node, do
    not write the embedded rows back, and get the row pairs the folded tower forward needs from the same kernel."""
    if conv_w.dtype != torch.float16:
        return VitEmbedFn.apply(video4d, conv_w, cls, pos, ln_w, ln_b, frame_index), None
    if torch.is_grad_enabled() and any(t.requires_grad for t in (conv_w, cls, pos, ln_w, ln_b)):
        if _fold_off(_FOLD_LN_TRAIN):                      # no tower folds in training: nobody reads the row pairs
            return VitEmbedFn.apply(video4d, conv_w, cls, pos, ln_w, ln_b, frame_index), None
        return VitEmbedFn.apply(video4d, conv_w, cls, pos, ln_w, ln_b, frame_index, True)      # (x, row pairs of x)
    D, _, p, _ = conv_w.shape
    L = pos.shape[0]
    patches = _patches_of(video4d, p, conv_w.dtype, frame_index)
    x0 = _linear(patches, conv_w.view(D, -1))
    x, _, _, stat = ops.vit_embed_ln_(x0, cls, pos, ln_w, ln_b, L, want_stat=fold_enabled(True), write_x0=False)
    return x, stat


class TextEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table, pos, dtype=torch.float16):
        ctx.save_for_backward(ids)
        ctx.dims = (table.shape[0], pos.shape[0])
        return ops.text_embed(ids.contiguous(), table, pos, dtype=dtype)

    @staticmethod
    def backward(ctx, dx):
        (ids,) = ctx.saved_tensors
        vocab, ctx_len = ctx.dims
        b, L = ids.shape
        dx = dx.contiguous()
        D = dx.shape[-1]
        dtable = ops.text_embed_bwd(ids, dx, vocab)
        dpos = torch.zeros((ctx_len, D), dtype=torch.float32, device=dx.device)
        ops.colsum(dx.view(b, L * D), out_dtype=torch.float32, round_f16=dx.dtype == torch.float16, out=dpos[:L].view(-1))
        return None, dtable, dpos, None


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# Forward passes of an fp16 tower that keep no activations (eval, the momentum encoders) can run with ln_1 / ln_2 folded into
# in_proj / c_fc (hmmc_tower_fwd_fused: no LayerNorm pass over the residual stream).  The folded form rounds gamma o W where the
# reference rounds LN(x): against the reference's fp32 regime it is as accurate as the reference's own fp16 regime (rel-L2 1.22e-3
# vs 1.18e-3 on text features, 1.217e-3 vs 1.218e-3 on frame features at true ViT-B/32 dims), but its fp16 errors are independent
# of the reference's, so against the AS-WRITTEN goldens it sits at ~sqrt(2) x the regime gap.  The frame tower passes the 1.5 x
# envelope of tests/test_gpu_model.py::test_envelope_at_true_vit_b32_dims that way; the text tower does not (text_feat max-abs
# 1.85 x, rel-L2 1.34 x), so the default folds the frame tower only.  HMMC_FOLD_LN: "vit" (default), "all", "0" (never).  This
# switch governs the passes that keep no activations; the training forward has its own, HMMC_FOLD_LN_TRAIN below.
_FOLD_LN = os.environ.get("HMMC_FOLD_LN", "vit")


# The same fold in the TRAINING forward and backward of the frame tower (hmmc_tower_fwd_fused(keep_acts) / hmmc_tower_bwd_fold):
# no ln_1 / ln_2 pass in either direction's critical data, no normalised activations kept; the tower's last layer stays on the
# unfolded kernels.  HMMC_FOLD_LN_TRAIN: "vit" (default), "all", "0".
_FOLD_LN_TRAIN = os.environ.get("HMMC_FOLD_LN_TRAIN", "vit")

# Policy, not capability: the token count from which the training fold has been validated on the product path.  The library
# takes towers of 512 tokens and more (hmmc_tower_fold_supported); folding those below this count would change their numerics.
_FOLD_TRAIN_MIN_TOKENS = 2048


def _fold_off(switch):
    return switch in ("0", "", "off")


def _fold_policy(switch, tower_default):
    """The value of one of the two switches above (read when a pass starts: bench.py and the tests assign them) -> whether a
    tower folds.  tower_default: True for a tower that folds under the default policy (the ViT frame tower)."""
    return not _fold_off(switch) and (switch in ("all", "1") or bool(tower_default))


def fold_enabled(tower_default):
    """Whether this tower's passes that keep no activations fold (HMMC_FOLD_LN); _tower_forward asks the library for the shape."""
    return _fold_policy(_FOLD_LN, tower_default)


def fold_train_enabled(tower_default, T, D, L):
    """Whether this tower's training pass folds at T tokens of width D in sequences of L: the switch (HMMC_FOLD_LN_TRAIN), the
    policy's token count and the library's shape limits - hmmc_tower_fold_supported, which knows the grouped weight-gradient
    launch the folded backward needs and the "no_wgrad_group" option (hmmc_amd/_lib.py sets it from HMMC_NO_WGRAD_GROUP)."""
    from ._lib import query
    return (_fold_policy(_FOLD_LN_TRAIN, tower_default) and T >= _FOLD_TRAIN_MIN_TOKENS
            and bool(query("hmmc_tower_fold_supported", T, D, L, 1)))


def _tower_forward(x, params, nseq, L, heads, causal, eps, fp32, keep, lead_only=False, x_stat=None, fold=False, last_exact=False):
    """Run all layers through the native layer runtime.  Returns (y, what _tower_backward needs or None).
    lead_only: only token 0 of every sequence of y is defined (see include/hmmc_hip.h).  fold (fp16 towers): run with ln_1 / ln_2
    folded into the GEMMs (hmmc_tower_fwd_fused) where the library takes the shape; with keep, last_exact leaves the last layer
    on the unfolded kernels.  x_stat: the row pairs of x for a folded pass, when its producer has them."""
    from ._lib import call, call_status, ptr, query
    T, D = x.shape
    nl = len(params) // PER_LAYER
    slab = query("hmmc_tower_act_bytes", T, D, nseq, L, heads, int(fp32))
    fold = bool(fold) and not fp32
    if fold and not keep and query("hmmc_tower_fold_supported", T, D, L, 0):
        acts = torch.empty(slab, dtype=torch.uint8, device=x.device)
        fwb = query("hmmc_tower_fold_bytes", T, D, nl, 0)
        fws = ops.workspace(fwb, x.device, "tower_fold")
        y = torch.empty_like(x)
        call("hmmc_tower_fwd_fused", ptr(x), ptr(x_stat), ptr(y), _ptr_array(params), ptr(acts), 0, nseq, L, heads, D, nl, int(causal),
             float(eps), int(lead_only), 0, ptr(fws), fwb)
        return y, None
    if fold and keep:
        # training: folded layers keep no normalised activations (a smaller slab each); the fold workspace (folded weights, fp32
        # weight-gradient sums) lives until the backward call
        nfold = nl - int(last_exact)
        acts = torch.empty(query("hmmc_tower_act_bytes_fold", T, D, nseq, L, heads) * nfold + slab * (nl - nfold), dtype=torch.uint8,
                           device=x.device)
        fwb = query("hmmc_tower_fold_bytes", T, D, nl, 1)
        fws = torch.empty(fwb, dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x)
        rc = call_status("hmmc_tower_fwd_fused", ptr(x), ptr(x_stat), ptr(y), _ptr_array(params), ptr(acts), 1, nseq, L, heads, D, nl,
                         int(causal), float(eps), int(lead_only), int(last_exact), ptr(fws), fwb, allow="HMMC_ERR_UNSUPPORTED")
        if rc == 0:
            return y, (acts, fws, int(last_exact))
        # HMMC_ERR_UNSUPPORTED (nothing was launched): a shape or setting the folded training runtime does not take after all - the unfolded
        # kernels below compute the same function
        del acts, fws, y
    acts = torch.empty(slab * (nl if keep else 1), dtype=torch.uint8, device=x.device)
    wsb = query("hmmc_tower_workspace_bytes", T, D, nseq, int(fp32), 0)
    ws = ops.workspace(wsb, x.device, "tower")
    y = torch.empty_like(x)
    call("hmmc_tower_fwd", ptr(x), ptr(y), _ptr_array(params), ptr(acts), int(keep), nseq, L, heads, D, nl, int(causal),
         float(eps), int(fp32), int(lead_only), ptr(ws), wsb)
    return y, (acts if keep else None)


_WGRAD_STREAM = os.environ.get("HMMC_WGRAD_STREAM", "1") != "0"


def _tower_backward(dy, x0, params, acts, nseq, L, heads, causal, fp32, lead_only=False):
    from ._lib import call, ptr, query
    T, D = x0.shape
    nl = len(params) // PER_LAYER
    grads = [torch.empty_like(p) for p in params]
    scratch = torch.empty(query("hmmc_tower_bwd_scratch_bytes", T, D, int(fp32)), dtype=torch.uint8, device=x0.device)
    wsb = query("hmmc_tower_workspace_bytes", T, D, nseq, int(fp32), nl)
    ws = ops.workspace(wsb, x0.device, "tower")
    dx = torch.empty_like(x0)
    # weight gradients on their own stream (leaves of the backward): the library orders the two streams itself
    wst = ops.aux_stream(x0.device, "wgrad").cuda_stream if _WGRAD_STREAM else None
    if isinstance(acts, tuple):                    # a forward that ran folded (hmmc_tower_fwd_fused, keep_acts = 1)
        acts, fws, last_exact = acts
        call("hmmc_tower_bwd_fold", ptr(dy), ptr(dx), ptr(x0), _ptr_array(params), _ptr_array(grads), ptr(acts), ptr(fws), fws.numel(),
             ptr(scratch), nseq, L, heads, D, nl, int(causal), int(lead_only), last_exact, ptr(ws), wsb, wst)
        return dx, grads
    call("hmmc_tower_bwd", ptr(dy), ptr(dx), ptr(x0), _ptr_array(params), _ptr_array(grads), ptr(acts), ptr(scratch), nseq, L,
         heads, D, nl, int(causal), int(fp32), int(lead_only), ptr(ws), wsb, wst)
    return dx, grads


def _tower_args(x, params, lead_only):
    """The checks of a CLIP tower's arguments -> (contiguous x, fp32, lead_only as the library takes it)."""
    for prm in params:
        if not prm.is_contiguous():
            raise ValueError("tower parameters must be contiguous")
    if any(prm.dtype != (x.dtype if prm.dim() == 2 else prm.dtype) for prm in params):
        raise RuntimeError(f"expected the activations ({x.dtype}) and the tower weights to have the same dtype: after "
                           "model.float() set text_encoder.dtype = torch.float32 as well, as with the reference")
    fp32 = x.dtype == torch.float32
    return x.contiguous(), fp32, bool(lead_only and not fp32)        # the class-token pruning exists for the fp16 tower only


class ClipTransformerFn(torch.autograd.Function):
    """All layers of a CLIP tower in one autograd node and ONE native call each way (fp16 activations, fp32
    LayerNorm statistics); the per-layer activations live in a single slab laid out by the library."""

    @staticmethod
    def forward(ctx, x, nseq, L, heads, causal, lead_only, fold_train, last_exact, x_stat, *params):
        keep = any(ctx.needs_input_grad)       # no_grad passes never get here: clip_transformer() below
        x, fp32, lead_only = _tower_args(x, params, lead_only)
        fold = bool(fold_train and keep)
        y, acts = _tower_forward(x, params, nseq, L, heads, causal, 1e-5, fp32, keep, lead_only, x_stat=x_stat if fold else None,
                                 fold=fold, last_exact=last_exact)
        ctx.acts, ctx.x0, ctx.params = acts, (x if keep else None), params
        ctx.cfg = (nseq, L, heads, causal, lead_only, fp32)
        return y

    @staticmethod
    def backward(ctx, dy):
        nseq, L, heads, causal, lead_only, fp32 = ctx.cfg
        dx, grads = _tower_backward(dy.contiguous(), ctx.x0, ctx.params, ctx.acts, nseq, L, heads, causal, fp32, lead_only)
        ctx.acts = ctx.x0 = None
        return (dx, None, None, None, None, None, None, None, None, *grads)


def clip_transformer(x, nseq, L, heads, causal, lead_only, *params, x_stat=None, fold_no_acts=False, fold_train=False, last_exact=False):
    """One run of a CLIP tower's layers; the caller (module_clip.Transformer.forward) has decided the fold: fold_no_acts for a
    pass that keeps no activations, fold_train for a training pass, which with last_exact leaves its last layer unfolded.
    A pass that records a graph is ClipTransformerFn.apply.  One that records none (torch.no_grad(): eval, the momentum encoders
    of modules/modeling.py:347-357) goes straight to the forward-only runtime: inside a Function `ctx.needs_input_grad` reports
    the inputs' requires_grad whatever the grad mode, and the pass would keep - and write - every layer's activations."""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return ClipTransformerFn.apply(x, nseq, L, heads, causal, lead_only, fold_train, last_exact, x_stat, *params)
    x, fp32, lead_only = _tower_args(x, params, lead_only)
    return _tower_forward(x, params, nseq, L, heads, causal, 1e-5, fp32, False, lead_only, x_stat=x_stat, fold=fold_no_acts)[0]


def _temporal_forward(u, heads, pos_table, params, keep):
    """-> (video_emb, (acts, x0, x, u2, norms): what TemporalFn.backward needs)."""
    b, F, E = u.shape
    u2 = u.contiguous().view(b * F, E)
    acts = x0 = None
    if len(params) // PER_LAYER:
        x0 = ops.add_rowbias(u2, pos_table, F)
        x, acts = _tower_forward(x0, params, b, F, heads, False, 1e-12, True, keep)
        out, norms = ops.temporal_pool_fwd(x, u2, b, F, E)
    else:
        x = u2
        out, norms = ops.temporal_pool_fwd(x, None, b, F, E)
    return out, (acts, x0, x, u2, norms)


def temporal(u, heads, pos_table, *params):
    """TemporalFn.apply; a pass that records no graph keeps no activations (see clip_transformer)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (u, pos_table) + params):
        return TemporalFn.apply(u, heads, pos_table, *params)
    return _temporal_forward(u, heads, pos_table, params, False)[0]


class LnProjFn(torch.autograd.Function):
    """feat = float( LN(x[rows]) @ proj ); rows = row_index (CLS / EOT rows) or all rows."""

    @staticmethod
    def forward(ctx, x, row_index, ln_w, ln_b, proj, rows_only=False):
        """rows_only: the producer of x reads its gradient at the rows of row_index ALONE (a lead_only tower: hmmc_tower_bwd
        reads dy at the class-token rows only), so the backward leaves the other rows of dx unwritten instead of zero-filling the
        whole [tokens, D] buffer (236 MB at config 2)."""
        D, E = proj.shape
        y, mean, rstd = ops.layernorm_fwd(x, ln_w, ln_b, 1e-5, row_index=row_index)
        R = y.shape[0]
        if y.dtype != proj.dtype:
            raise RuntimeError(f"expected the activations ({y.dtype}) and the projection ({proj.dtype}) to have the same dtype")
        ctx.rows_only = bool(rows_only and row_index is not None)
        ctx.save_for_backward(x, row_index, ln_w, proj, y, mean, rstd)
        if proj.dtype == torch.float32:
            return ops.dgrad_f32(y, proj)                 # y @ proj, fp32 regime
        return ops.gemm_f16(y, proj, R, E, D, a_kmajor=True, b_kmajor=False).float()

    @staticmethod
    def backward(ctx, dout):
        x, row_index, ln_w, proj, y, mean, rstd = ctx.saved_tensors
        D, E = proj.shape
        R = y.shape[0]
        if proj.dtype == torch.float32:
            d32 = dout.contiguous()
            dy = ops.linear_f32(d32, proj)                                           # d @ proj^T
            dproj = ops.wgrad_f32(y, d32)                                            # y^T d
        else:
            d16 = dout.contiguous().half()
            dy = ops.gemm_f16(d16, proj, R, D, E, a_kmajor=True, b_kmajor=True)      # dy = d16 @ proj^T
            dproj = ops.gemm_f16(y, d16, D, E, R, a_kmajor=False, b_kmajor=False)    # y^T d16
        if row_index is not None:
            dx = torch.empty_like(x) if ctx.rows_only else torch.zeros_like(x)
            dx, dlw, dlb = ops.layernorm_bwd(dy, x, ln_w, mean, rstd, row_index=row_index, dx=dx)
        else:
            dx, dlw, dlb = ops.layernorm_bwd(dy, x, ln_w, mean, rstd)
        return dx, None, dlw, dlb, dproj, None


class TemporalFn(torch.autograd.Function):
    """video_emb = mean_f normalise( TemporalTransformer(u + pos) + u ); fp32 throughout, TF-style LN eps 1e-12."""

    @staticmethod
    def forward(ctx, u, heads, pos_table, *params):
        out, (acts, x0, x, u2, norms) = _temporal_forward(u, heads, pos_table, params, any(ctx.needs_input_grad))
        ctx.acts, ctx.x0, ctx.params = acts, x0, params
        ctx.fin = (x, u2, norms, pos_table)
        ctx.cfg = (*u.shape, heads)
        return out

    @staticmethod
    def backward(ctx, dout):
        b, F, E, heads = ctx.cfg
        x, u2, norms, pos_table = ctx.fin
        params = ctx.params
        nl = len(params) // PER_LAYER
        dvf = ops.temporal_pool_bwd(x, u2 if nl else None, norms, dout.contiguous(), b, F, E)
        if not nl:
            return dvf.view(b, F, E), None, None
        dx, grads = _tower_backward(dvf, ctx.x0, params, ctx.acts, b, F, heads, False, True)
        if F == pos_table.shape[0]:
            dpos = ops.colsum(dx.view(b, F * E)).view(F, E)
        else:
            dpos = torch.zeros_like(pos_table)
            ops.colsum(dx.view(b, F * E), out=dpos[:F].view(-1))
        du = dx + dvf                                   # through (u + pos) and through the residual
        ctx.acts = ctx.x0 = None
        return (du.view(b, F, E), None, dpos, *grads)


class FinetuneHeadFn(torch.autograd.Function):
    """loss = w_vtm (CE(S) + CE(S^T)) + w_ftm/F sum_f (CE(S_f) + CE(S_f^T)),  S = 100 n(q) n(.)^T."""

    @staticmethod
    def forward(ctx, q, v, u, w_vtm, w_ftm, scale):
        B, E = q.shape
        F = u.shape[1] if u is not None else 0
        keys = torch.empty((B * (1 + F), E), dtype=torch.float32, device=q.device)
        qn, qnorm = ops.l2norm_fwd(q.contiguous())
        _, vnorm = ops.l2norm_fwd(v.contiguous(), out=keys[:B])
        unorm = None
        if F:
            _, unorm = ops.l2norm_fwd(u.contiguous().view(B * F, E), out=keys[B:])
        C = B * (1 + F)
        S = ops.gemm_f32(qn, keys, B, C, E, (E, 1), (1, E), alpha=scale)
        wf = w_ftm / F if F else 0.0
        loss, lse_row, lse_col = ops.infonce_fwd(S, B, F, w_vtm, wf)
        ctx.save_for_backward(qn, qnorm, keys, vnorm, unorm, S, lse_row, lse_col)
        ctx.cfg = (B, F, E, w_vtm, wf, scale)
        return loss

    @staticmethod
    def backward(ctx, gout):
        qn, qnorm, keys, vnorm, unorm, S, lse_row, lse_col = ctx.saved_tensors
        B, F, E, w_vtm, wf, scale = ctx.cfg
        C = B * (1 + F)
        dS = ops.infonce_bwd(S, lse_row, lse_col, gout, B, F, w_vtm, wf)
        dqn = ops.gemm_f32(dS, keys, B, E, C, (C, 1), (E, 1), alpha=scale)          # dS @ keys
        dkeys = ops.gemm_f32(dS, qn, C, E, B, (1, C), (E, 1), alpha=scale)          # dS^T @ qn
        dq = ops.l2norm_bwd(dqn, qn, qnorm)
        dv = ops.l2norm_bwd(dkeys[:B], keys[:B], vnorm)
        du = ops.l2norm_bwd(dkeys[B:], keys[B:], unorm).view(B, F, E) if F else None
        return dq, dv, du, None, None, None


# ----------------------------------------------------------------------------- pre-training (MoCo) stages

# HMMC_FORCE_COLLECTIVES=1: issue every collective of the path even in a process group of ONE rank (where each is the
# identity and the product path normally skips it).  One GPU cannot host two RCCL ranks, so this is how the RCCL calls
# themselves (all_gather_into_tensor / reduce_scatter_tensor / all_reduce on RCCL's stream, ordered against the tower
# streams) are executed and checked bit-for-bit on a one-GPU box (tests/test_gpu_ddp.py).
_FORCE_COLLECTIVES = os.environ.get("HMMC_FORCE_COLLECTIVES", "0") == "1"


def collectives_active():
    """True when the path's collectives must run: a process group of more than one rank (or the forcing switch above)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or _FORCE_COLLECTIVES


def _sync_sum(t):
    """Sum a small statistics tensor over ranks (SyncBatchNorm's exchange, modules/modeling.py:115-129)."""
    import torch.distributed as dist
    if collectives_active():
        t = t.contiguous()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


class MlpFn(torch.autograd.Function):
    """Linear(512,4096) -> BatchNorm1d (batch statistics over all ranks' rows) -> ReLU -> Linear(4096,512)
    (reference MLP, modules/modeling.py:788-807).  Returns (y, batch_mean, batch_var_biased, n_rows_global)."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, eps, running=None):
        """running: (running_mean, running_var, num_batches_tracked, momentum) of the BatchNorm1d to update in place (train mode)."""
        x = x.contiguous()
        h = ops.linear_f32(x, w1, bias=b1)
        sums = ops.bn_stats(h)
        N = h.shape[1]
        if collectives_active():
            n_local = torch.full((1,), float(h.shape[0]), device=h.device)      # a fill kernel: torch.tensor(..., device=) is a blocking copy
            packed = _sync_sum(torch.cat([sums.view(-1), n_local]))
            n = packed[-1:]                                                      # the global row count, on the device
            sums = packed[:-1].view(2, N)
        else:
            n = float(h.shape[0])
        rm, rv, nbt, mom = running if running is not None else (None, None, None, 0.0)
        if mom is None:                                  # nn.BatchNorm1d(momentum=None): cumulative average, factor 1 / batches seen
            if rm is None:
                mom = 0.0                                # no running statistics to update
            elif nbt is None:
                raise ValueError("BatchNorm1d(momentum=None) keeps a cumulative average: it needs num_batches_tracked")
            else:
                mom = 1.0 / (float(nbt) + 1.0)           # a host read of the counter, as nn.BatchNorm1d does; hmmc_bn_finalize adds 1
        mean, var, rstd = ops.bn_finalize(sums, n, eps, mom, rm, rv, nbt)        # one launch: statistics + running statistics
        y = ops.bn_apply_relu(h, mean, rstd, gamma, beta)
        out = ops.linear_f32(y, w2, bias=b2)
        ctx.n = n
        ctx.save_for_backward(x, w1, gamma, w2, h, y, mean, rstd)
        ctx.mark_non_differentiable(mean, var)
        return out, mean, var

    @staticmethod
    def backward(ctx, dout, _dm, _dv):
        x, w1, gamma, w2, h, y, mean, rstd = ctx.saved_tensors
        n = ctx.n
        dout = dout.contiguous()
        dw2 = ops.wgrad_f32(dout, y)
        db2 = ops.colsum(dout)
        dy = ops.dgrad_f32(dout, w2)
        local = ops.bn_bwd_reduce(dy, y, h, mean, rstd)
        # dgamma / dbeta are this rank's sums (DDP averages parameter gradients afterwards, as with SyncBatchNorm);
        # dx needs the sums over every rank's rows
        dbeta, dgamma = local[0], local[1]
        if collectives_active():
            # sums / n on the device (n is the all-reduced row count): reading n on the host would stall the launch stream
            sums = _sync_sum(local.clone())
            dh = ops.bn_bwd_apply(dy, y, h, mean, rstd, gamma, (sums / n).contiguous(), n_global=1.0)
        else:
            dh = ops.bn_bwd_apply(dy, y, h, mean, rstd, gamma, local, n_global=n)
        dw1 = ops.wgrad_f32(dh, x)
        db1 = ops.colsum(dh)
        dx = ops.dgrad_f32(dh, w1)
        return dx, dw1, db1, dgamma, dbeta, dw2, db2, None, None


class MocoLossFn(torch.autograd.Function):
    """sum over rows of w * CE([q.k, q.queue]/T, label 0) with q, k L2-normalised (F.normalize, eps 1e-12):
    contrastive_loss of modules/modeling.py:286-313 for R stacked (q, k) pairs that share one queue.
    k and the queue receive no gradient (keys come from the momentum encoders under no_grad)."""

    @staticmethod
    def forward(ctx, q, k, queue, temperature, w):
        q, k = q.contiguous(), k.contiguous()
        R, E = q.shape
        Kq = queue.shape[1]
        qn, qnorm = ops.l2norm_fwd(q, eps=1e-12)
        kn, _ = ops.l2norm_fwd(k, eps=1e-12)
        lpos = ops.rowdot(qn, kn)
        S = ops.gemm_f32(qn, queue, R, Kq, E, (E, 1), (Kq, 1))
        loss, lse = ops.moco_loss_fwd(S, lpos, temperature, w)
        ctx.save_for_backward(qn, qnorm, kn, lpos, S, lse, queue)
        ctx.cfg = (temperature, w)
        return loss

    @staticmethod
    def backward(ctx, gout):
        qn, qnorm, kn, lpos, S, lse, queue = ctx.saved_tensors
        temperature, w = ctx.cfg
        R, E = qn.shape
        Kq = queue.shape[1]
        dlpos = ops.moco_loss_bwd_(S, lpos, lse, gout, temperature, w)       # S now holds dS
        dqn = ops.gemm_f32(S, queue, R, E, Kq, (Kq, 1), (1, Kq))             # dS @ queue^T
        ops.row_axpy_(dqn, dlpos, kn)
        dq = ops.l2norm_bwd(dqn, qn, qnorm)
        return dq, None, None, None, None


def _mlm_capacity(n, p):
    """rows the MLM head is evaluated on: every position for small inputs, otherwise the expected number of labelled
    positions plus eight standard deviations of Binomial(n, p) (exceeded with probability < 1e-15)."""
    import math
    if n <= 4096 or p <= 0 or p >= 1:
        return n
    return min(n, int(n * p + 8.0 * math.sqrt(n * p * (1.0 - p))) + 16)


class MlmHeadFn(torch.autograd.Function):
    """BertLMPredictionHead + cross-entropy with ignore_index -100 (modules/module_cross.py:308-357,
    modules/modeling.py:171-179): dense, erf-GELU, TF-LayerNorm(1e-12), decoder to the vocabulary, mean CE.

    The reference runs the head over all b*L positions and lets the loss ignore the ~85 % whose label is -100; neither
    the loss nor any gradient depends on those rows, so the head (a [rows, 512] x [512, 49408] fp32 GEMM and its two
    backward GEMMs) is evaluated on the labelled rows only.  Their number is data dependent; to keep the host from
    reading it (a stall of the launch stream every step) the labelled rows are compacted on the device into a buffer of
    fixed capacity (_mlm_capacity: mean + 8 sigma of the mask's binomial), the unused slots carry label -100, and a
    labelled count above the capacity raises the device error flag (ops.raise_on_device_errors) instead of going unnoticed."""

    @staticmethod
    def forward(ctx, hidden, labels, dw, db, lnw, lnb, decw, decb, mask_prob=0.15):
        x_all = hidden.contiguous().view(-1, hidden.shape[-1])
        labels = labels.contiguous().view(-1)
        n = labels.numel()
        cap = _mlm_capacity(n, mask_prob)
        flag = labels >= 0
        pos = torch.cumsum(flag.to(torch.int64), 0) - 1                       # slot of every labelled row, in order
        keep = flag & (pos < cap)
        # slot -> row (unused slots point at the dump row n); every tensor below has a static shape: no host read
        rows = torch.full((cap + 1,), n, dtype=torch.int64, device=labels.device)
        rows.scatter_(0, torch.where(keep, pos, torch.full_like(pos, cap)), torch.arange(n, device=labels.device))
        rows = rows[:cap]
        if cap < n:
            ops.device_error_flag(labels.device).add_((pos[-1] >= cap).to(torch.int32))
        used = rows < n
        gather = rows.clamp(max=n - 1)
        x = x_all.index_select(0, gather)
        lab = torch.where(used, labels.index_select(0, gather), torch.full_like(rows, -100))
        ctx.shape = hidden.shape
        a = ops.linear_f32(x, dw, bias=db)
        g = ops.gelu_erf_fwd(a)
        t, mean, rstd = ops.layernorm_fwd(g, lnw, lnb, 1e-12)
        logits = ops.linear_f32(t, decw, bias=decb)
        loss_sum, lse, count = ops.ce_fwd(logits, lab)
        ctx.save_for_backward(x, lab, rows, dw, lnw, decw, a, g, t, mean, rstd, logits, lse, count)
        return loss_sum / count.clamp(min=1.0)[0]

    @staticmethod
    def backward(ctx, gout):
        x, lab, rows, dw, lnw, decw, a, g, t, mean, rstd, logits, lse, count = ctx.saved_tensors
        dlogits = ops.ce_bwd_(logits, lab, lse, gout, count)
        d_decw = ops.wgrad_f32(dlogits, t)
        d_decb = ops.colsum(dlogits)
        dt = ops.dgrad_f32(dlogits, decw)
        dg, d_lnw, d_lnb = ops.layernorm_bwd(dt, g, lnw, mean, rstd)
        da = ops.gelu_erf_bwd(a, dg)
        d_dw = ops.wgrad_f32(da, x)
        d_db = ops.colsum(da)
        dx_rows = ops.dgrad_f32(da, dw)
        n = ctx.shape[:-1].numel()
        # unused slots (zero gradient: their label is -100) all land in the dump row n
        dx = dx_rows.new_zeros(n + 1, ctx.shape[-1]).index_copy_(0, rows, dx_rows)[:n]
        return dx.view(ctx.shape), None, d_dw, d_db, d_lnw, d_lnb, d_decw, d_decb, None


class LmLogitsFn(torch.autograd.Function):
    """BertLMPredictionHead.forward as a differentiable op (reference modules/module_cross.py:308-357): logits =
    decoder(TF-LayerNorm(erf-GELU(dense(x)))) + bias for EVERY row.  The training step does not come this way (MlmHeadFn
    evaluates the head on the labelled rows only and never hands the logits out); this is the module's own call surface."""

    @staticmethod
    def forward(ctx, hidden, dw, db, lnw, lnb, decw, decb):
        x = hidden.contiguous().view(-1, hidden.shape[-1])
        a = ops.linear_f32(x, dw, bias=db)
        g = ops.gelu_erf_fwd(a)
        t, mean, rstd = ops.layernorm_fwd(g, lnw, lnb, 1e-12)
        logits = ops.linear_f32(t, decw, bias=decb)
        ctx.save_for_backward(x, dw, lnw, decw, a, g, t, mean, rstd)
        ctx.shape = hidden.shape
        return logits.view(*hidden.shape[:-1], decw.shape[0])

    @staticmethod
    def backward(ctx, dlogits):
        x, dw, lnw, decw, a, g, t, mean, rstd = ctx.saved_tensors
        dl = dlogits.contiguous().view(-1, decw.shape[0])
        d_decw = ops.wgrad_f32(dl, t)
        d_decb = ops.colsum(dl)
        dt = ops.dgrad_f32(dl, decw)
        dg, d_lnw, d_lnb = ops.layernorm_bwd(dt, g, lnw, mean, rstd)
        da = ops.gelu_erf_bwd(a, dg)
        d_dw = ops.wgrad_f32(da, x)
        d_db = ops.colsum(da)
        dx = ops.dgrad_f32(da, dw)
        return dx.view(ctx.shape), d_dw, d_db, d_lnw, d_lnb, d_decw, d_decb


class LooseSimFn(torch.autograd.Function):
    """scale * normalise(q) normalise(v)^T, differentiable in both operands (reference modules/modeling.py:207-229).  The
    training heads do not come this way (FinetuneHeadFn fuses the similarity with the InfoNCE terms)."""

    @staticmethod
    def forward(ctx, q, v, scale):
        q, v = q.contiguous(), v.contiguous()
        E = q.shape[-1]
        qn, qnorm = ops.l2norm_fwd(q)
        vn, vnorm = ops.l2norm_fwd(v)
        ctx.save_for_backward(qn, qnorm, vn, vnorm)
        ctx.scale = scale
        return ops.gemm_f32(qn, vn, qn.shape[0], vn.shape[0], E, (E, 1), (1, E), alpha=scale)

    @staticmethod
    def backward(ctx, dS):
        qn, qnorm, vn, vnorm = ctx.saved_tensors
        dS = dS.contiguous()
        nq, nv, E = qn.shape[0], vn.shape[0], qn.shape[1]
        dqn = ops.gemm_f32(dS, vn, nq, E, nv, (nv, 1), (E, 1), alpha=ctx.scale)          # dS @ vn
        dvn = ops.gemm_f32(dS, qn, nv, E, nq, (1, nv), (E, 1), alpha=ctx.scale)          # dS^T @ qn
        return ops.l2norm_bwd(dqn, qn, qnorm), ops.l2norm_bwd(dvn, vn, vnorm), None


def bert_seed():
    """A fresh 62-bit dropout seed from torch's default (host) generator: torch.manual_seed reproduces a run, no device sync."""
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())


_BERT_LN_SLOTS = (8, 9, 14, 15)                      # the LayerNorm weight / bias of a layer's 16 entries (hmmc_bert_fwd's order)


def bert_layout_regime(pool_w, pool_b, proj_w, proj_b, params):
    """The regime a dtype layout selects (dtypes only; module_cross.bert_regime is this function on a TextEncoder's tensors):
    torch.float32 when every parameter is fp32; torch.float16 for exactly module_cross.convert_bert_weights' layout (every
    dense weight and bias fp16; the embedding tables and every LayerNorm parameter fp32).  Anything else raises."""
    fixed = list(params[:ops.BERT_EMB_PARAMS])
    dense = [pool_w, pool_b, proj_w, proj_b]
    for i, prm in enumerate(params[ops.BERT_EMB_PARAMS:]):
        (fixed if i % ops.BERT_LAYER_PARAMS in _BERT_LN_SLOTS else dense).append(prm)
    if all(t.dtype == torch.float32 for t in fixed):
        for dt in (torch.float32, torch.float16):
            if all(t.dtype == dt for t in dense):
                return dt
    mixed = sorted({str(t.dtype) for t in fixed + dense})
    raise TypeError(f"the Chinese text encoder's parameters ({', '.join(mixed)}) are in neither regime: fp32 throughout, or fp16 as "
                    "module_cross.convert_bert_weights(text_encoder) converts them (nn.Linear weights and biases fp16, embedding "
                    "tables and LayerNorms fp32)")


def bert_param_regime(pool_w, pool_b, proj_w, proj_b, params):
    """bert_layout_regime of the tensors a tower call received, which must be contiguous and on the GPU."""
    for prm in (pool_w, pool_b, proj_w, proj_b) + tuple(params):
        if not prm.is_cuda or not prm.is_contiguous():
            raise TypeError("the Chinese text encoder runs on contiguous CUDA parameters")
    return bert_layout_regime(pool_w, pool_b, proj_w, proj_b, params)


def _lin(x, w, bias):
    if x.dtype == torch.float16:
        return ops.gemm_f16(x, w, x.shape[0], w.shape[0], x.shape[1], bias=bias)
    return ops.linear_f32(x, w, bias=bias)


def _dgrad(dy, w, out=None):
    """dy [M, N'] @ w [N', K'] (into `out`: contiguous rows of a larger buffer)."""
    M, Np = dy.shape
    Kp = w.shape[1]
    if dy.dtype == torch.float16:
        return ops.gemm_f16(dy, w, M, Kp, Np, True, False, out=out)
    return ops.gemm_f32(dy, w, M, Kp, Np, (Np, 1), (Kp, 1), out=out)


def _wgrad(dy, x):
    if dy.dtype == torch.float16:
        return ops.gemm_f16(dy, x, dy.shape[1], x.shape[1], dy.shape[0], False, False)
    return ops.wgrad_f32(dy, x)


def _pooler_fwd(x, w, bias, b, L):
    return (ops.bert_pooler_f16_fwd if x.dtype == torch.float16 else ops.bert_pooler_fwd)(x, w, bias, b, L)


def _pooler_bwd(dy, y, x, w, b, L, dx):
    return (ops.bert_pooler_f16_bwd if x.dtype == torch.float16 else ops.bert_pooler_bwd)(dy, y, x, w, b, L, dx)


def _bert_tower_forward(ids, mask, params, cfg, keep, dtype=torch.float32):
    """hmmc_bert_fwd / hmmc_bert_f16_fwd: -> (last_hidden_state [b*L, D] in `dtype`, acts or None)."""
    from ._lib import call, ptr, query
    heads, inter, eps, p_hidden, p_attn, seed = cfg
    b, L = ids.shape
    vocab, D = params[0].shape
    nl = (len(params) - ops.BERT_EMB_PARAMS) // ops.BERT_LAYER_PARAMS
    half = dtype == torch.float16
    nbytes = (query("hmmc_bert_f16_act_bytes", b, L, heads, D, inter, nl, int(keep)) if half else
              query("hmmc_bert_act_bytes", b, L, heads, D, inter, nl, int(keep), int(p_attn > 0)))
    acts = torch.empty(nbytes, dtype=torch.uint8, device=ids.device)
    y = torch.empty((b * L, D), dtype=dtype, device=ids.device)
    call("hmmc_bert_f16_fwd" if half else "hmmc_bert_fwd", ptr(ids), ptr(mask), ptr(y), _ptr_array(params), ptr(acts), int(keep), b, L,
         heads, D, inter, nl, vocab, float(eps), float(p_hidden), float(p_attn), int(seed), ptr(ops.device_error_flag(ids.device)))
    return y, (acts if keep else None)


def _bert_tower_backward(dy, ids, mask, params, acts, cfg):
    """The regime is dy's dtype (that of the forward's last_hidden_state)."""
    from ._lib import call, ptr, query
    heads, inter, eps, p_hidden, p_attn, seed = cfg
    b, L = ids.shape
    vocab, D = params[0].shape
    nl = (len(params) - ops.BERT_EMB_PARAMS) // ops.BERT_LAYER_PARAMS
    pre = "hmmc_bert_f16" if dy.dtype == torch.float16 else "hmmc_bert"
    grads = [torch.empty_like(p) for p in params]
    scratch = torch.empty(query(pre + "_bwd_scratch_bytes", b, L, D, inter), dtype=torch.uint8, device=dy.device)
    wsb = query(pre + "_workspace_bytes", b, L, D, inter)
    ws = ops.workspace(wsb, dy.device, "bert")
    call(pre + "_bwd", ptr(dy), ptr(ids), ptr(mask), _ptr_array(params), _ptr_array(grads), ptr(acts), ptr(scratch), b, L, heads, D,
         inter, nl, vocab, params[1].shape[0], params[2].shape[0], float(p_hidden), float(p_attn), int(seed), ptr(ws), wsb)
    return grads


class BertFn(torch.autograd.Function):
    """The Chinese text tower in one autograd node (reference modules/module_cross.py:273-277): BertModel(ids, attention_mask),
    then text_proj of the pooler output (want = "feat" -> [b, E]) or of every hidden row (want = "hidden" -> [b, L, E]).  The
    parameters' dtype layout selects the regime (bert_param_regime): fp32 throughout, or the fp16 kernels of csrc/bert_f16.hip
    with fp16 pooler and text_proj; the features leave in fp32 either way.  cfg = (heads, intermediate size, LayerNorm eps,
    p_hidden, p_attn, seed); params: hmmc_bert_fwd's order."""

    @staticmethod
    def forward(ctx, ids, mask, cfg, want, keep, pool_w, pool_b, proj_w, proj_b, *params):
        dtype = bert_param_regime(pool_w, pool_b, proj_w, proj_b, params)
        b, L = ids.shape
        y, acts = _bert_tower_forward(ids, mask, params, cfg, keep, dtype)
        pooled = None
        if want == "feat":
            pooled = _pooler_fwd(y, pool_w, pool_b, b, L)
            out = _lin(pooled, proj_w, proj_b)
        else:
            out = _lin(y, proj_w, proj_b).view(b, L, -1)
        if keep:
            ctx.save_for_backward(ids, mask, y, pooled, pool_w, proj_w)
            ctx.acts, ctx.params, ctx.cfg, ctx.want = acts, params, cfg, want
        return ops.cast(out, torch.float32)

    @staticmethod
    def backward(ctx, dout):
        ids, mask, y, pooled, pool_w, proj_w = ctx.saved_tensors
        b, L = ids.shape
        d = ops.cast(dout.contiguous().view(-1, dout.shape[-1]), y.dtype)
        dproj_b = ops.colsum(d)
        dpool_w = dpool_b = None
        if ctx.want == "feat":
            dproj_w = _wgrad(d, pooled)
            dpooled = _dgrad(d, proj_w)
            dy = torch.zeros_like(y)                       # no gradient reaches the other rows of last_hidden_state
            dpool_w, dpool_b = _pooler_bwd(dpooled, pooled, y, pool_w, b, L, dy)
        else:
            dproj_w = _wgrad(d, y)
            dy = _dgrad(d, proj_w)
        grads = _bert_tower_backward(dy, ids, mask, ctx.params, ctx.acts, ctx.cfg)
        ctx.acts = None
        return (None, None, None, None, None, dpool_w, dpool_b, dproj_w, dproj_b, *grads)


def bert_text(ids, mask, cfg, want, pool_w, pool_b, proj_w, proj_b, *params):
    """BertFn.apply; a pass that records no graph (torch.no_grad(): eval) keeps no activations."""
    keep = torch.is_grad_enabled() and any(p.requires_grad for p in (pool_w, pool_b, proj_w, proj_b) + params)
    return BertFn.apply(ids, mask, cfg, want, keep, pool_w, pool_b, proj_w, proj_b, *params)


class BertManyFn(torch.autograd.Function):
    """Several text inputs through ONE pass of the Chinese tower (TextEncoder.encode_many): ids / mask [R, L] hold the
    inputs' rows one after the other, padded to the longest; segs = ((row0, b, want), ...).  want = "feat": pooler + text_proj
    on the segment's class rows, addressed in place -> [b, E]; "hidden": text_proj of ALL L positions of the segment's rows
    -> [b, L, E] (the caller slices a shorter input's positions off outside this node, so the padded ones get exact zeros on
    the way back).  The backward assembles one dy and runs one hmmc_bert_bwd: one gradient per parameter.  Regimes as BertFn."""

    @staticmethod
    def forward(ctx, ids, mask, cfg, segs, keep, pool_w, pool_b, proj_w, proj_b, *params):
        dtype = bert_param_regime(pool_w, pool_b, proj_w, proj_b, params)
        R, L = ids.shape
        y, acts = _bert_tower_forward(ids, mask, params, cfg, keep, dtype)
        outs, pooled = [], []
        for row0, b, want in segs:
            rows = y[row0 * L:(row0 + b) * L]
            if want == "feat":
                pooled.append(_pooler_fwd(rows, pool_w, pool_b, b, L))
                outs.append(ops.cast(_lin(pooled[-1], proj_w, proj_b), torch.float32))
            else:
                pooled.append(None)
                outs.append(ops.cast(_lin(rows, proj_w, proj_b), torch.float32).view(b, L, -1))
        if keep:
            ctx.save_for_backward(ids, mask, y, pool_w, proj_w, *[t for t in pooled if t is not None])
            ctx.acts, ctx.params, ctx.cfg, ctx.segs = acts, params, cfg, segs
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        ids, mask, y, pool_w, proj_w, *kept = ctx.saved_tensors
        R, L = ids.shape
        dy = torch.zeros_like(y)                           # the pooler backward writes class rows only
        acc = {}

        def add(name, g):
            acc[name] = g if name not in acc else acc[name].add_(g)

        for (row0, b, want), dout in zip(ctx.segs, douts):
            d = ops.cast(dout.contiguous().view(-1, dout.shape[-1]), y.dtype)
            rows, drows = y[row0 * L:(row0 + b) * L], dy[row0 * L:(row0 + b) * L]
            add("proj_b", ops.colsum(d))
            if want == "feat":
                pooled = kept.pop(0)
                add("proj_w", _wgrad(d, pooled))
                dpool_w, dpool_b = _pooler_bwd(_dgrad(d, proj_w), pooled, rows, pool_w, b, L, drows)
                add("pool_w", dpool_w)
                add("pool_b", dpool_b)
            else:
                add("proj_w", _wgrad(d, rows))
                _dgrad(d, proj_w, out=drows)                                             # d @ proj_w into the segment's rows
        grads = _bert_tower_backward(dy, ids, mask, ctx.params, ctx.acts, ctx.cfg)
        ctx.acts = None
        return (None, None, None, None, None, acc.get("pool_w"), acc.get("pool_b"), acc["proj_w"], acc["proj_b"], *grads)


def bert_text_many(ids, mask, cfg, segs, pool_w, pool_b, proj_w, proj_b, *params):
    """BertManyFn.apply; a pass that records no graph (the momentum encoder) keeps no activations."""
    keep = torch.is_grad_enabled() and any(p.requires_grad for p in (pool_w, pool_b, proj_w, proj_b) + params)
    return BertManyFn.apply(ids, mask, cfg, tuple(segs), keep, pool_w, pool_b, proj_w, proj_b, *params)
