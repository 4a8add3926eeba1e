"""The decoder with a backward pass: the reference's ``MUSt3R.forward`` and ``CausalMUSt3R.forward`` (must3r/model/decoder.py:267-350, :435-553) over the
memory schedule, under ``torch.autograd``::

    dec = MUSt3R.from_decoder(native_decoder)                         # fp32 copies under the reference's state-dict keys
    mem, pts0 = dec(x0, pos0, shape0)                                 # x [B, nimgs, N, Denc], pos int64 [B, nimgs, N, 2], true_shape [B, nimgs, 2]
    mem, pts1 = dec(x1, pos1, shape1, mem)                            # the memory tensors stay in the graph from call to call
    _, pts = dec(x, pos, shape, mem, render=True)
    loss(pts).backward()                                              # x0.grad, x1.grad, x.grad, dec.*.grad
    native_decoder.load_state_dict(dec.state_dict(), strict=True)     # serve what was trained

The forward is the reference's, on flattened rows: ``feat_embed_enc_to_dec`` (``train_block.linear``), ``image2_embed`` (a broadcast add under torch autograd),
the ``train_cross.CachedDecoderBlock`` layers with the self-attention table of the views and the cross-attention table of the call -- ``memory_views`` for an
update, and two tables built here: a lone first view over an empty memory attends its own pre-feedback tokens, a render reads the scene's memory rows -- then
``train_head.PredictionHead``.  After the layers of an update the feedback offset ``feedback_layer(feedback_norm(x_{L-1}))`` (``feedback_offset``: one
Function that saves its inputs and recomputes) is added to the new tokens of all layers but the last and each layer's ``norm_y`` is applied: for all layers
in one launch each way (``feedback_prepare``: ``must3r_hip_feedback_prepare_forward`` / ``_grad``, include/must3r_hip.h "ABI 21, additive", csrc/train_decoder.hip),
followed by the k | v Linears in the ``kv`` mode; the results are ``torch.cat``-ed behind the old memory.  Without feedback the post-feedback rows are the
``prepare_y`` rows already computed for the keys: they are reused and nothing is launched.

Everything runs in fp32 -- or, inside ``with train_block.linear_precision("bf16"):``, with the products of every Linear but the head's on the 16-bit MFMA
(bf16 operands, fp32 accumulation; the norms, the attention cores, the feedback add, the head and all storage stay fp32; ``backward()`` may be called after
the block has ended: each Function runs its backward in the mode of its forward); ``train_block.attention_precision("bf16")`` moves the products of the
attention cores there as well, and ``train_block.amp("bf16")`` is both.  Only the gradients ``needs_input_grad`` asks for are computed (frozen parts cost no launches); first order only; CPU tensors
raise.  ``landscape_only=True`` (the recipe's constructor value; False by default, and never taken from the native decoder) takes a batch stored landscape whose
portrait views carry true_shape rows of (W, H): ``dec(x, pos, true_shape, mem, img_shape=(H, W))`` (``train_head.PredictionHead``).  List inputs
(``forward_list``) and aspect ratios beyond that pair are not built; memory dropout is ``train_dropout.CausalMUSt3R``, which hands the key masks of a
call to this forward.  The memory is concatenated per call, not appended in place.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import train_block as TB
from ._train_common import HEAD, _Affine, _back, _check_params, _check_x, _dev, _f32, _new, _Proj, _record_modes, _recorded_modes, _rows, _scratch, _stream
from .train_attention import _table, memory_views, self_views
from .train_block import ROPE_NPOS, _MlpParams
from .train_cross import MEMORY_MODES, CachedDecoderBlock, memory_rows
from .train_head import PredictionHead

FEEDBACK_TYPES = ("single_mlp", "single_linear", None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# feedback add + norm_y of all layers: the operator forms, on contiguous fp32 GPU tensors [R, D]
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fb_args(xs, offset, gammas, betas, add_layers, eps):
    a = _lib.FeedbackPrepareArgs()
    for l, x in enumerate(xs):
        a.x[l] = x.data_ptr()
        if gammas is not None:
            a.gamma[l], a.beta[l] = gammas[l].data_ptr(), betas[l].data_ptr()
    a.offset = None if offset is None else C.c_void_p(offset.data_ptr())
    a.L, a.R, a.D, a.add_layers, a.eps = len(xs), int(xs[0].shape[0]), int(xs[0].shape[1]), int(add_layers), float(eps)
    a.stream = _stream(xs[0].device)
    return a


def feedback_prepare_forward(xs, offset, gammas, betas, add_layers, eps=1e-6):
    """``must3r_hip_feedback_prepare_forward``: ``[LN_l(xs[l] + (l < add_layers ? offset : 0))]``; ``gammas = betas = None``: the add alone."""
    lib, dev = _lib.load(), xs[0].device
    a = _fb_args(xs, offset, gammas, betas, add_layers, eps)
    ys = [torch.empty_like(x) for x in xs]
    for l, y in enumerate(ys):
        a.y[l] = y.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.must3r_hip_feedback_prepare_forward(C.byref(a), None, 0))
    return ys


def feedback_prepare_grad(xs, offset, gammas, dys, add_layers, eps=1e-6, want_dx=None, want_doffset=True, want_dgamma=None, want_dbeta=None):
    """``must3r_hip_feedback_prepare_grad``: ``(dxs, doffset, dgammas, dbetas)``, ``None`` where the ``want`` lists (one flag per layer) say so."""
    lib, dev, L = _lib.load(), xs[0].device, len(xs)
    R, D = int(xs[0].shape[0]), int(xs[0].shape[1])
    norm = gammas is not None
    want_dx = [True] * L if want_dx is None else list(want_dx)
    want_dgamma = [norm] * L if want_dgamma is None else [bool(w) and norm for w in want_dgamma]
    want_dbeta = [norm] * L if want_dbeta is None else [bool(w) and norm for w in want_dbeta]
    dxs = [_new(w, dev, R, D) for w in want_dx]
    dgs, dbs = [_new(w, dev, D) for w in want_dgamma], [_new(w, dev, D) for w in want_dbeta]
    doffset = _new(want_doffset, dev, R, D)
    if not (any(want_dx) or want_doffset or any(want_dgamma) or any(want_dbeta)):
        return dxs, doffset, dgs, dbs
    a = _fb_args(xs, offset, gammas, gammas, add_layers, eps)   # the backward does not read beta: any non-null pointer stands for "this layer has a norm"
    for l in range(L):
        a.dy[l] = dys[l].data_ptr()
        for arr, t in ((a.dx, dxs[l]), (a.dgamma, dgs[l]), (a.dbeta, dbs[l])):
            if t is not None:
                arr[l] = t.data_ptr()
    a.doffset = None if doffset is None else C.c_void_p(doffset.data_ptr())
    with torch.cuda.device(dev):
        nbytes, scratch = 0, None
        if any(want_dgamma) or any(want_dbeta):
            nbytes = lib.must3r_hip_feedback_prepare_scratch_bytes(L, R, D)
            scratch = _scratch(nbytes, dev)
        _lib.check(lib.must3r_hip_feedback_prepare_grad(C.byref(a), None if scratch is None else C.c_void_p(scratch.data_ptr()), nbytes))
    return dxs, doffset, dgs, dbs


class _FeedbackPrepare(torch.autograd.Function):
    @staticmethod
    def forward(ctx, L, add_layers, eps, norm, offset, *rest):
        xs = rest[:L]
        gammas, betas = (rest[L:2 * L], rest[2 * L:3 * L]) if norm else (None, None)
        ctx.save_for_backward(*([offset] if offset is not None else []), *rest)
        ctx.geom = (L, add_layers, eps, norm, offset is not None)
        ys = feedback_prepare_forward([_rows(x) for x in xs], None if offset is None else _rows(offset), None if not norm else [_f32(g) for g in gammas],
                                      None if not norm else [_f32(b) for b in betas], add_layers, eps)
        return tuple(y.view(x.shape) for y, x in zip(ys, xs))

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        L, add_layers, eps, norm, has_offset = ctx.geom
        saved = list(ctx.saved_tensors)
        offset = saved.pop(0) if has_offset else None
        xs = saved[:L]
        gammas = saved[L:2 * L] if norm else None
        need = ctx.needs_input_grad
        want_dx = need[5:5 + L]
        want_dg = need[5 + L:5 + 2 * L] if norm else None
        want_db = need[5 + 2 * L:5 + 3 * L] if norm else None
        dxs, doffset, dgs, dbs = feedback_prepare_grad([_rows(x) for x in xs], None if offset is None else _rows(offset),
                                                       None if not norm else [_f32(g) for g in gammas], [_rows(d) for d in dys], add_layers, eps,
                                                       want_dx, bool(need[4]) and has_offset, want_dg, want_db)
        grads = list(dxs) + (list(dgs) + list(dbs) if norm else [])
        return (None, None, None, None, None if doffset is None else doffset.reshape(offset.shape).to(offset.dtype), *_back(grads, saved))


def feedback_prepare(xs, offset, norm_weights=None, norm_biases=None, add_layers=None, eps=1e-6):
    """``[LN_l(xs[l] + offset) for l < add_layers] + [LN_l(xs[l]) for the rest]``, all layers in one launch each way; ``xs``: L <= 32 tensors ``[..., D]`` of one
    shape, ``offset`` of that shape (``None`` with ``add_layers = 0``), ``add_layers`` L - 1 by default (the reference's feedback: every layer but the last).
    ``norm_weights = norm_biases = None``: the add alone (the ``raw`` memory mode).  Differentiable at the tokens, the offset and the norms; a layer without
    the add has the bits of ``train_block.layer_norm``."""
    xs = list(xs)
    L = len(xs)
    if not 1 <= L <= _lib.FEEDBACK_MAX_LAYERS:
        raise ValueError(f"feedback_prepare: {L} layers, expected 1 to {_lib.FEEDBACK_MAX_LAYERS}")
    add_layers = L - 1 if add_layers is None else int(add_layers)
    if not 0 <= add_layers <= L:
        raise ValueError(f"feedback_prepare: add_layers {add_layers} outside [0, {L}]")
    D = _check_x(xs[0], "feedback_prepare: xs[0]")
    if D % 64 or D > 1024:
        raise ValueError(f"feedback_prepare: width {D}, expected a multiple of 64 and at most 1024")
    for l, x in enumerate(xs):
        _dev(x, f"xs[{l}]")
        if x.shape != xs[0].shape:
            raise ValueError(f"feedback_prepare: xs[{l}] of shape {tuple(x.shape)} beside xs[0] of shape {tuple(xs[0].shape)}")
    if add_layers == 0:
        offset = None
    else:
        _dev(offset, "offset")
        if offset.shape != xs[0].shape:
            raise ValueError(f"feedback_prepare: offset of shape {tuple(offset.shape)} beside tokens of shape {tuple(xs[0].shape)}")
    norm = norm_weights is not None
    if norm != (norm_biases is not None) or (norm and (len(norm_weights) != L or len(norm_biases) != L)):
        raise ValueError("feedback_prepare: norm_weights and norm_biases come together, one per layer (both None: the add alone)")
    params = (list(norm_weights) + list(norm_biases)) if norm else []
    _check_params("feedback_prepare", D, **{f"norm[{i}]": (t, (D,)) for i, t in enumerate(params)})
    inputs = [t for t in (offset, *xs, *params) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs):
        return list(_FeedbackPrepare.apply(L, add_layers, float(eps), norm, offset, *xs, *params))
    ys = feedback_prepare_forward([_rows(x) for x in xs], None if offset is None else _rows(offset), None if not norm else [_f32(g) for g in norm_weights],
                                  None if not norm else [_f32(b) for b in norm_biases], add_layers, float(eps))
    return [y.view(x.shape) for y, x in zip(ys, xs)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the feedback offset: feedback_layer(feedback_norm(x)), a Mlp WITHOUT a residual or a Linear (feedback_mechanism.py:11-23, :48)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _offset_forward(x, norm_w, norm_b, w1, b1, w2, b2, eps):
    y = TB.layernorm_forward(_rows(x), _f32(norm_w), _f32(norm_b), eps)
    if w2 is None:
        out = TB.linear_forward(y, _f32(w1), _f32(b1))
    else:
        out = TB.linear_forward(TB.linear_forward(y, _f32(w1), _f32(b1), _lib.LIN_BIAS_GELU), _f32(w2), _f32(b2))
    return out.view(x.shape)


class _FeedbackOffset(torch.autograd.Function):
    """Composed from the operator forms of ``train_block``; saves its inputs and recomputes.  (Not ``mlp_sublayer(x) - x``, which cancels.)"""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, w1, b1, w2, b2, eps):
        ctx.save_for_backward(x, norm_w, norm_b, w1, b1, *([w2, b2] if w2 is not None else []))
        ctx.eps, ctx.mlp = eps, w2 is not None
        _record_modes(ctx, linear=True)
        return _offset_forward(x, norm_w, norm_b, w1, b1, w2, b2, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        with _recorded_modes(ctx):   # the Linears recomputed and differentiated below multiply as the forward's did
            return _FeedbackOffset._backward(ctx, grad_out)

    @staticmethod
    def _backward(ctx, grad_out):
        saved = ctx.saved_tensors
        x, g, b, w1, b1 = (_f32(t) for t in saved[:5])
        need = ctx.needs_input_grad
        x, dy = x.view(-1, x.shape[-1]), _rows(grad_out)
        want_ln = tuple(need[:3])
        y = TB.layernorm_forward(x, g, b, ctx.eps)
        if ctx.mlp:
            w2 = _f32(saved[5])
            want_first = any(want_ln) or need[3] or need[4]
            h, z = TB.linear_forward(y, w1, b1, _lib.LIN_BIAS_GELU, want_z=True)
            dh, dw2, db2 = TB.linear_grad(h, w2, dy, want=(want_first, need[5], need[6]))
            dz = TB.gelu_grad(dh, z, out=dh) if want_first else None
        else:
            dz, dw2, db2 = dy, None, None
        dyn, dw1, db1 = TB.linear_grad(y, w1, dz, want=(any(want_ln), need[3], need[4])) if dz is not None else (None, None, None)
        dx, dg, db = TB.layernorm_grad(x, g, dyn, ctx.eps, want=want_ln) if dyn is not None else (None, None, None)
        grads = [dx, dg, db, dw1, db1] + ([dw2, db2] if ctx.mlp else [])
        out = _back(grads, saved)
        return (*out, *(() if ctx.mlp else (None, None)), None)


def feedback_offset(x, norm_w, norm_b, fc1_w, fc1_b, fc2_w=None, fc2_b=None, eps=1e-5):
    """``fc2(gelu(fc1(LN(x))))`` (``single_mlp``) or, with ``fc2_w = fc2_b = None``, ``fc1(LN(x))`` (``single_linear``); x ``[..., D]``."""
    D = _check_x(x, "feedback_offset: x")
    if D % 64 or D > 1024:
        raise ValueError(f"feedback_offset: width {D}, expected a multiple of 64 and at most 1024")
    Hd = int(fc1_w.shape[0])
    shapes = dict(norm_w=(norm_w, (D,)), norm_b=(norm_b, (D,)), fc1_w=(fc1_w, (Hd, D)), fc1_b=(fc1_b, (Hd,)))
    if fc2_w is not None:
        shapes.update(fc2_w=(fc2_w, (D, Hd)), fc2_b=(fc2_b, (D,)))
    elif Hd != D:
        raise ValueError(f"feedback_offset: a Linear of {Hd} outputs for tokens of width {D}")
    _check_params("feedback_offset", D, **shapes)
    inputs = (x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        return _FeedbackOffset.apply(*inputs, float(eps))
    return _offset_forward(*inputs, float(eps))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------------------------
class MUSt3R(PredictionHead):
    """The reference's ``MUSt3R`` (decoder.py:14) as a trainable fp32 module; the parameters live under its state-dict keys (``feat_embed_enc_to_dec.*``,
    ``image2_embed``, ``blocks_dec.{i}.*``, ``feedback_layer.fc1|fc2.*`` or ``feedback_layer.weight|bias``, ``feedback_norm.*``, ``norm_dec.*``,
    ``head_dec.proj.*``), so that ``state_dict()`` loads into ``must3r_amd.model.MUSt3R`` with ``strict=True``."""

    _causal = False

    def __init__(self, enc_embed_dim=1024, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, feedback_type=None, memory_mode="norm_y",
                 rope=(100.0, 1.0), eps=1e-6, npos=ROPE_NPOS, head_dtype=_lib.F16, landscape_only=False):
        super().__init__(embed_dim, eps, head_dtype, landscape_only)
        if memory_mode not in MEMORY_MODES:
            raise ValueError(f"MUSt3R: memory_mode {memory_mode!r}, expected one of {MEMORY_MODES}")
        feedback_type = feedback_type or None
        if feedback_type not in FEEDBACK_TYPES:
            raise ValueError(f"MUSt3R: feedback_type {feedback_type!r}, expected one of {FEEDBACK_TYPES}")
        if not 1 <= int(depth) <= _lib.FEEDBACK_MAX_LAYERS:
            raise ValueError(f"MUSt3R: depth {depth}, expected 1 to {_lib.FEEDBACK_MAX_LAYERS}")
        self.enc_embed_dim, self.depth, self.attn_num_heads = int(enc_embed_dim), int(depth), int(num_heads)
        self.memory_mode, self.feedback_type, self.freeze = memory_mode, feedback_type, "none"
        # the reference's order of registration: the head's two modules move behind the rest
        norm_dec, head_dec = self.norm_dec, self.head_dec
        del self.norm_dec, self.head_dec
        self.feat_embed_enc_to_dec = _Proj(self.enc_embed_dim, self.embed_dim)
        self.image2_embed = nn.Parameter(torch.zeros(1, 1, self.embed_dim))
        nn.init.normal_(self.image2_embed, std=0.02)
        self.blocks_dec = nn.ModuleList([CachedDecoderBlock(self.embed_dim, self.attn_num_heads, mlp_ratio, memory_mode, rope, eps, npos)
                                         for _ in range(self.depth)])
        if feedback_type == "single_mlp":           # inactive at the start, as the reference's (feedback_mechanism.py:26-36)
            self.feedback_layer = _MlpParams(self.embed_dim, 4 * self.embed_dim)
            nn.init.zeros_(self.feedback_layer.fc2.weight)
        elif feedback_type == "single_linear":
            self.feedback_layer = _Proj(self.embed_dim, self.embed_dim)
            nn.init.zeros_(self.feedback_layer.weight)
        else:
            self.feedback_layer = None
        self.feedback_norm = _Affine(self.embed_dim) if feedback_type else None
        self.feedback_eps = 1e-5                    # nn.LayerNorm's default (feedback_mechanism.py:14)
        self.norm_dec, self.head_dec = norm_dec, head_dec

    @classmethod
    def from_decoder(cls, decoder, memory_mode=None, head_dtype=_lib.F16, **kw):
        """fp32 copies of a loaded ``must3r_amd.model.MUSt3R`` (or anything with its state-dict keys and attributes); the source is left alone.
        ``landscape_only`` is not among the attributes read: it is the constructor's keyword (``from_decoder(dec, landscape_only=True)``), False by default."""
        sd = decoder.state_dict()
        w = sd["feat_embed_enc_to_dec.weight"]
        D, Denc = int(w.shape[0]), int(w.shape[1])
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks_dec."))
        hidden = int(sd["blocks_dec.0.mlp.fc1.weight"].shape[0])
        cfg = getattr(decoder, "cfg", None)
        rope = (float(cfg.rope_freq), float(cfg.rope_f0)) if cfg is not None else (100.0, 1.0)
        mode = memory_mode if memory_mode is not None else getattr(decoder, "memory_mode", "norm_y")
        dec = cls(enc_embed_dim=Denc, embed_dim=D, depth=depth, num_heads=int(getattr(decoder, "attn_num_heads", D // HEAD)), mlp_ratio=hidden / D,
                  feedback_type=getattr(decoder, "feedback_type", None) or None, memory_mode=mode, rope=rope,
                  eps=float(getattr(decoder.norm_dec, "eps", 1e-6)), head_dtype=head_dtype, **kw)
        dec.load_state_dict({k: v.detach().to(torch.float32).clone() for k, v in sd.items()}, strict=True)
        return dec.to(w.device)

    def set_freeze(self, freeze="none"):
        """The reference's (decoder.py:98-111): ``'not_head'`` freezes everything but ``norm_dec`` and ``head_dec``; like the reference's it never unfreezes."""
        frozen = {"none": [], "not_head": [self.feat_embed_enc_to_dec, self.image2_embed, self.blocks_dec, self.feedback_layer, self.feedback_norm]}[freeze]
        self.freeze = freeze
        for m in frozen:
            if isinstance(m, nn.Parameter):
                m.requires_grad = False
            elif m is not None:
                for p in m.parameters():
                    p.requires_grad = False

    def change_memory_mode(self, memory_mode="norm_y"):
        if memory_mode not in MEMORY_MODES:
            raise ValueError(f"change_memory_mode: {memory_mode!r}, expected one of {MEMORY_MODES}")
        for blk in self.blocks_dec:
            blk.memory_mode = memory_mode
        self.memory_mode = memory_mode

    # the tail of the memory tuple: every image is protected (decoder.py:337)
    def _memory_tail(self, n_imgs, n_tokens, prot_imgs, prot_tokens, n_new, N):
        return n_imgs, n_tokens

    def _post_feedback(self, new, pre):
        """The rows the memory keeps of an update: ``prepare_y`` of the new tokens of every layer after the feedback offset was added to all but the last."""
        L = self.depth
        if self.feedback_type is None or L == 1:
            return pre                                  # nothing was added: the rows computed for the keys are the rows to keep
        fl, fn = self.feedback_layer, self.feedback_norm
        if self.feedback_type == "single_mlp":
            offset = feedback_offset(new[-1], fn.weight, fn.bias, fl.fc1.weight, fl.fc1.bias, fl.fc2.weight, fl.fc2.bias, self.feedback_eps)
        else:
            offset = feedback_offset(new[-1], fn.weight, fn.bias, fl.weight, fl.bias, None, None, self.feedback_eps)
        if self.memory_mode == "raw":
            return feedback_prepare(new[:-1], offset, None, None, L - 1) + [new[-1]]
        ys = feedback_prepare(new, offset, [b.norm_y.weight for b in self.blocks_dec], [b.norm_y.bias for b in self.blocks_dec], L - 1, self.blocks_dec[0].eps)
        if self.memory_mode == "norm_y":
            return ys
        out = []
        for y, blk in zip(ys, self.blocks_dec):
            c = blk.cross_attn
            out.append(torch.cat([TB.linear(y, c.projk.weight, c.projk.bias), TB.linear(y, c.projv.weight, c.projv.bias)], dim=-1))
        return out

    def forward(self, x, pos, true_shape, current_mem=None, render=False, return_tokens=False, key_mask=None, view_mask=None, img_shape=None):
        """x ``[B, nimgs, N, Denc]``, pos int64 ``[B, nimgs, N, 2]`` (or flattened ``[B nimgs N, 2]``: ``train_block.check_positions`` then recognises
        the tensor from call to call and does not read it on the host again), true_shape ``[B, nimgs, 2]`` (all views of a call share (H, W)) ->
        ``(mem, pointmaps [B, nimgs, H, W, 7])``; ``mem`` is the reference's 5-tuple ``([L tensors [B, Nm, W]], labels int64 [B, Nm], mem_nimgs,
        protected_imgs, protected_tokens)`` whose tensors stay in the autograd graph (a detached memory, or one made under ``torch.no_grad()``, is fine).
        ``render``: the memory is read, not updated, and comes back as it was given.  ``return_tokens``: also the last layer's tokens ``[B, nimgs, N, D]``
        (before ``norm_dec``).  ``key_mask`` / ``view_mask``: packed key masks over the key rows of the call's cross attention and each view's row of them
        (``train_attention.pack_key_mask``; ``train_dropout``), the same for every layer.  A decoder built with ``landscape_only=True`` takes a batch
        stored landscape whose portrait views have true_shape rows of (W, H), with the tokens and positions of their own grid (``ManyAR_PatchEmbed``); the
        blocks see the orientation through ``pos`` alone, the head turns those views back into the stored layout.  ``img_shape``: the stored (H, W), with
        which the head reads nothing back to the host (``PredictionHead.forward``)."""
        if isinstance(x, (list, tuple)) or isinstance(pos, (list, tuple)):
            raise TypeError("train_decoder.MUSt3R.forward takes tensors [B, nimgs, N, Denc]: list inputs (forward_list, mixed aspect ratios) are not built")
        _dev(x, "x")
        _dev(pos, "pos")
        if x.ndim != 4 or int(x.shape[-1]) != self.enc_embed_dim or x.numel() == 0:
            raise ValueError(f"MUSt3R: x of shape {tuple(x.shape)}, expected [B, nimgs, N, {self.enc_embed_dim}]")
        if render and current_mem is None:
            raise ValueError("MUSt3R: a render needs a memory")
        B, V, N, _ = (int(s) for s in x.shape)
        D, L, M = self.embed_dim, self.depth, B * V * N
        W = 2 * D if self.memory_mode == "kv" else D
        if pos.numel() != 2 * M:
            raise ValueError(f"MUSt3R: pos of shape {tuple(pos.shape)} for x of shape {tuple(x.shape)}")
        pos = pos if tuple(pos.shape) == (M, 2) else pos.reshape(M, 2)     # flattened already: the same object reaches check_positions again
        if current_mem is None:
            mem_vals, labels, n_imgs, prot_imgs, prot_tokens, Nm = [None] * L, torch.zeros((B, 0), dtype=torch.int64, device=x.device), 0, 0, 0, 0
        else:
            mem_vals, labels, n_imgs, prot_imgs, prot_tokens = current_mem
            mem_vals = list(mem_vals)
            Nm = int(mem_vals[0].shape[1])
            if len(mem_vals) != L or any(_dev(m, "memory").shape != (B, Nm, W) for m in mem_vals):
                raise ValueError(f"MUSt3R: a memory of {len(mem_vals)} tensors of shape {tuple(mem_vals[0].shape)}, expected {L} of [{B}, Nm, {W}] "
                                 f"(memory_mode {self.memory_mode!r})")
            if render and Nm == 0:
                raise ValueError("MUSt3R: a render needs a memory with rows")
        t = TB.linear(x.reshape(M, self.enc_embed_dim), self.feat_embed_enc_to_dec.weight, self.feat_embed_enc_to_dec.bias).view(B, V, N, D)
        # image2_embed: every view but the reference view of an initialising call -- one broadcast add over the call's tokens
        e = self.image2_embed.to(t.dtype).view(1, 1, 1, D)
        if current_mem is None:
            first = torch.ones((1, V, 1, 1), dtype=t.dtype, device=t.device)
            first[0, 0] = 0
            e = e * first
        xr = (t + e).reshape(M, D)
        sv = _table(self_views(B, V, N))
        if render:
            cross = [[(b * V + j) * N, N, b * Nm, Nm, 0, 0] for b in range(B) for j in range(V)]
        elif V == 1 and Nm == 0:
            cross = [[b * N, N, b * N, N, 0, 0] for b in range(B)]           # a lone first view attends its own pre-feedback tokens (decoder.py:293)
        else:
            cross = memory_views(B, V, N, Nm, mask=True, causal=self._causal)
        cross = _table(cross)
        new, pre = [], []
        for blk, mem_l in zip(self.blocks_dec, mem_vals):
            if render:
                keys = mem_l.reshape(B * Nm, W)
            else:
                new.append(xr)
                pre.append(blk.prepare_y(xr))
                keys = memory_rows(mem_l, pre[-1], B)
            xr = blk(xr, keys, pos, sv, cross, key_mask, view_mask)
        if render:
            out = current_mem
        else:
            rows = [r.view(B, V * N, W) for r in self._post_feedback(new, pre)]
            mem = rows if Nm == 0 else [torch.cat([m.to(r.dtype), r], dim=1) for m, r in zip(mem_vals, rows)]
            new_labels = torch.arange(V, dtype=torch.int64, device=x.device).view(1, V, 1).repeat(B, 1, N).view(B, V * N) + int(n_imgs)
            labels = torch.cat([labels.to(x.device), new_labels], dim=1)
            n_imgs = int(n_imgs) + V
            out = (mem, labels, n_imgs, *self._memory_tail(n_imgs, int(labels.shape[1]), prot_imgs, prot_tokens, V, N))
        tokens = xr.view(B, V, N, D)
        pts = PredictionHead.forward(self, tokens, true_shape, img_shape)
        return (out, pts, tokens) if return_tokens else (out, pts)


class CausalMUSt3R(MUSt3R):
    """The class the reference trains (decoder.py:353-553) at memory dropout 0: in an update view j attends the old memory and the new tokens of the views
    before it; at initialisation view 0 attends view 1 (``memory_views(..., causal=True)``).  ``use_mem_mask`` and ``use_xformers_mask`` choose between
    equivalent ways of masking in the reference and change nothing here.  Renders and lone views are ``MUSt3R``'s."""

    _causal = True

    def __init__(self, protected_imgs=1, mem_dropout=0.0, **kw):
        if float(mem_dropout) > 0.0:
            raise NotImplementedError("CausalMUSt3R(mem_dropout > 0): the random token dropout of the training recipe (decoder.py:469-480) is not built")
        super().__init__(**kw)
        self.protected_imgs = int(protected_imgs)

    # decoder.py:456-459
    def _memory_tail(self, n_imgs, n_tokens, prot_imgs, prot_tokens, n_new, N):
        prot = min(self.protected_imgs, int(prot_imgs) + int(n_new))
        return prot, int(prot_tokens) + (prot - int(prot_imgs)) * int(N)
