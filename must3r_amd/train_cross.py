"""The decoder's block with a backward pass: the reference's ``CachedDecoderBlock`` (blocks/layers.py:57-99) under ``torch.autograd``.  Two of its three
residual sublayers are ``train_block``'s; the third is here, the cross attention of the tokens over the token memory::

    cross sublayer       x + proj(attn(projq(norm2 x), projk y, projv y))     ``cross_attention_sublayer``  (no RoPE: cross_attn has pos_embed=None)

    blk = CachedDecoderBlock.from_params(decoder.blocks_dec[3], memory_mode="norm_y")     # fp32 copies under the reference's state-dict keys
    y = memory_rows(mem, blk.prepare_y(x), n_scenes)                  # per scene [Nm memory rows | V n new rows]: the rows ``memory_views`` indexes
    out = blk(x, y, pos, self_views(B, V, n), memory_views(B, V, n, Nm))
    loss(out).backward()                                              # x.grad, mem.grad, blk.*.grad

Queries and keys are rows of different tensors, several views of a scene read the same key rows (the key groups of ``train_attention``), and the gradient also
arrives at the memory -- which is how it reaches earlier frames and, during an update, the block's own input through ``norm_y``.  The memory modes are the
reference's: ``norm_y`` (the memory holds ``norm_y`` of the tokens), ``raw`` (the tokens; ``norm_y`` runs inside the block) and ``kv`` (``[projk | projv]`` of
``norm_y`` of the tokens, ``[Rm, 2 D]``: nothing is projected in the block, the gradient reaches ``projk`` / ``projv`` through ``prepare_y``).

Everything runs in fp32 on the fp32 MFMA (``must3r_hip_cross_sublayer_forward`` / ``_grad``, include/must3r_hip.h "ABI 21, additive"; the stream travels in
the descriptor).  Under ``train_block.linear_precision("bf16")`` the products of projq, projk, projv and proj and of their gradients (``dmem = dK Wk + dV Wv``
included) take bf16 operands on the 16-bit MFMA; ``norm2``, ``norm_y``, the attention core, the biases and the residual stay fp32, and so does all storage;
under ``train_block.attention_precision("bf16")`` (or ``train_block.amp``) the products of the attention core do the same, its softmax staying fp32.  A forward saves its inputs and nothing else; the backward recomputes the sublayer's forward into scratch and differentiates it.  Only the
gradients ``needs_input_grad`` asks for are computed (a detached memory and frozen ``projk`` / ``projv``: no dK / dV launch; a frozen ``x``, ``norm2`` and
``projq``: no dQ launch).  First order only (``once_differentiable``); gradients come back in the shape and dtype of their inputs; CPU tensors raise.

Key masks (memory dropout): ``cross_attention_sublayer(..., key_mask=bits, view_mask=rows)`` and ``CachedDecoderBlock.forward(..., key_mask=, view_mask=)``
hand the packed masks of ``train_attention.pack_key_mask`` to the sublayer's attention core (``must3r_hip_cross_sublayer_masked_forward`` / ``_grad``); the
mask bits index the key rows of a view like the table does.  Without them every call path is the one it was.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import train_block as TB
from ._train_common import HEAD, _Affine, _back, _call_sublayer, _check_params, _check_x, _dev, _f32, _ld, _new, _Proj, _ptr, _record_modes, _recorded_modes, _rows, _scratch, _stream
from ._train_common import _strided_rows as _mem_rows
from .train_attention import _check_table, _mask, _table, n_groups
from .train_attention import self_views as _self_views
from .train_block import ROPE_NPOS, _AttnParams, _MlpParams

MEMORY_MODES = ("norm_y", "kv", "raw")
CROSS_OUTPUTS = ("dx", "dmem", "dgamma", "dbeta", "dWq", "dbq", "dWk", "dbk", "dWv", "dbv", "dWproj", "dbproj")


def _cross_args(x, mem, tab, gamma, beta, Wq, bq, Wk, bk, Wv, bv, Wproj, bproj, eps):
    a = _lib.CrossSublayerArgs()
    a.x, a.mem, a.gamma, a.beta = (_ptr(t) for t in (x, mem, gamma, beta))
    a.Wq, a.bq, a.Wk, a.bk, a.Wv, a.bv, a.Wproj, a.bproj = (_ptr(t) for t in (Wq, bq, Wk, bk, Wv, bv, Wproj, bproj))
    a.views = C.c_void_p(tab.data_ptr())
    a.M, a.Rm, a.D, a.n_views, a.ldmem, a.eps = int(x.shape[0]), int(mem.shape[0]), int(x.shape[1]), int(tab.shape[0]), _ld(mem), float(eps)
    a.stream = _stream(x.device)
    return a


def _call_masked(entry, a, mask, nbytes, dev, **tensors):
    """``_call_sublayer`` for the masked entry points: the filled descriptor ``a`` travels inside a ``CrossSublayerMaskedArgs`` with the masks ``(bits, rows)``
    of ``train_attention._mask``; the stream is the one ``a`` carries."""
    for n, t in tensors.items():
        setattr(a, n, _ptr(t))
    m = _lib.CrossSublayerMaskedArgs()
    m.core = a
    bits, vm = mask
    m.mask_bits, m.view_mask, m.mask_rows, m.mask_ld = _ptr(bits), C.c_void_p(vm.data_ptr()), int(bits.shape[0]), int(bits.shape[1])
    with torch.cuda.device(dev):
        scratch = _scratch(nbytes, dev)
        _lib.check(entry(C.byref(m), _ptr(scratch), nbytes))


def cross_forward(x, mem, tab, gamma, beta, Wq, bq, Wk, bk, Wv, bv, Wproj, bproj, eps=1e-6, mask=None):
    """``must3r_hip_cross_sublayer_forward`` on fp32 GPU tensors (x contiguous, mem row-strided) and an int32 CPU table; ``Wk = bk = Wv = bv = None``: mem holds
    k | v.  ``mask``: ``(bits, rows)`` of ``train_attention._mask``, through ``must3r_hip_cross_sublayer_masked_forward``."""
    lib = _lib.load()
    out = torch.empty_like(x)
    a = _cross_args(x, mem, tab, gamma, beta, Wq, bq, Wk, bk, Wv, bv, Wproj, bproj, eps)
    if mask is None:
        nbytes = lib.must3r_hip_cross_sublayer_scratch_bytes(a.M, a.Rm, a.D, a.n_views, 1 if Wk is None else 0)
        _call_sublayer(lib.must3r_hip_cross_sublayer_forward, a, nbytes, x.device, out=out)
    else:
        nbytes = lib.must3r_hip_cross_sublayer_masked_scratch_bytes(a.M, a.Rm, a.D, a.n_views, 1 if Wk is None else 0)
        _call_masked(lib.must3r_hip_cross_sublayer_masked_forward, a, mask, nbytes, x.device, out=out)
    return out


def cross_grad(x, mem, tab, gamma, beta, Wq, bq, Wk, bk, Wv, bv, Wproj, bproj, dy, eps=1e-6, want=(True,) * 12, dmem=None, mask=None):
    """``must3r_hip_cross_sublayer_grad``: the gradients of CROSS_OUTPUTS, ``None`` where ``want`` says so (and for Wk, bk, Wv, bv where mem holds k | v).
    ``dmem``: a row-strided fp32 buffer ``[Rm, D or 2 D]`` to write the memory's gradient into instead of a new tensor."""
    lib = _lib.load()
    dev, M, D, Rm = x.device, int(x.shape[0]), int(x.shape[1]), int(mem.shape[0])
    kv_ready = Wk is None
    want = [bool(w) and not (kv_ready and 6 <= i < 10) for i, w in enumerate(want)]
    shapes = ((M, D), (Rm, 2 * D if kv_ready else D), (D,), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,))
    outs = [_new(w, dev, *s) for w, s in zip(want, shapes)]
    if want[1] and dmem is not None:
        outs[1] = dmem
    if not any(want):
        return outs
    a = _cross_args(x, mem, tab, gamma, beta, Wq, bq, Wk, bk, Wv, bv, Wproj, bproj, eps)
    a.lddmem = _ld(outs[1]) if outs[1] is not None else 0
    if mask is None:
        nbytes = lib.must3r_hip_cross_sublayer_scratch_bytes(M, Rm, D, a.n_views, 1 if kv_ready else 0)
        _call_sublayer(lib.must3r_hip_cross_sublayer_grad, a, nbytes, dev, dy=dy, **dict(zip(CROSS_OUTPUTS, outs)))
    else:
        nbytes = lib.must3r_hip_cross_sublayer_masked_scratch_bytes(M, Rm, D, a.n_views, 1 if kv_ready else 0)
        _call_masked(lib.must3r_hip_cross_sublayer_masked_grad, a, mask, nbytes, dev, dy=dy, **dict(zip(CROSS_OUTPUTS, outs)))
    return outs


def _opt(t):
    return None if t is None else _f32(t)


class _Cross(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mem, norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b, tab, eps, mask=None):
        ctx.save_for_backward(x, mem, norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b)
        ctx.tab, ctx.eps, ctx.mask = tab, eps, mask
        _record_modes(ctx, linear=True, attention=True)
        width = int(mem.shape[1])
        return cross_forward(_rows(x), _mem_rows(mem, width), tab, *(_opt(t) for t in (norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b)), eps,
                             mask).view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        x, mem = saved[0], saved[1]
        with _recorded_modes(ctx):
            grads = cross_grad(_rows(x), _mem_rows(mem, int(mem.shape[1])), ctx.tab, *(_opt(t) for t in saved[2:]), _rows(grad_out), ctx.eps,
                               want=tuple(ctx.needs_input_grad[:12]), mask=ctx.mask)
        # CROSS_OUTPUTS is in the order of the inputs
        return (*_back(grads, [t if t is not None else x for t in saved]), None, None, None)


def cross_attention_sublayer(x, mem, views, heads, norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b, eps=1e-6, key_mask=None, view_mask=None):
    """``x + proj(attn(projq(LN(x)), projk(mem), projv(mem)))``; x [..., D] with D = heads * 64 (flattened to rows), mem [Rm, D] -- or
    ``k_w = k_b = v_w = v_b = None`` with mem [Rm, 2 D] = k | v (the ``kv`` memory mode).  ``views``: the 6-int table of ``train_attention`` whose query rows
    index the rows of x and whose key rows index mem (``memory_views``; ragged tables are fine).  Differentiable at x, mem and the ten parameters.  mem may be
    a row-strided view with a contiguous last dimension: the stride is passed through.  ``key_mask`` / ``view_mask``: the packed key masks of
    ``train_attention.attention`` over the key rows of each view, saved for the backward like the table."""
    D = _check_x(x, "cross_attention_sublayer: x")
    if int(heads) * HEAD != D:
        raise ValueError(f"cross_attention_sublayer: width {D} is not heads * 64 = {int(heads) * HEAD}")
    kv = [k_w, k_b, v_w, v_b]
    kv_ready = all(t is None for t in kv)
    if not kv_ready and any(t is None for t in kv):
        raise ValueError("cross_attention_sublayer: k_w, k_b, v_w, v_b come together (all None: mem holds k | v)")
    _dev(mem, "mem")
    width = 2 * D if kv_ready else D
    if mem.ndim != 2 or int(mem.shape[1]) != width or int(mem.shape[0]) == 0:
        raise ValueError(f"cross_attention_sublayer: mem of shape {tuple(mem.shape)}, expected [rows, {width}] with rows")
    shapes = dict(norm_w=(norm_w, (D,)), norm_b=(norm_b, (D,)), q_w=(q_w, (D, D)), q_b=(q_b, (D,)), proj_w=(proj_w, (D, D)), proj_b=(proj_b, (D,)))
    if not kv_ready:
        shapes.update(k_w=(k_w, (D, D)), k_b=(k_b, (D,)), v_w=(v_w, (D, D)), v_b=(v_b, (D,)))
    _check_params("cross_attention_sublayer", D, **shapes)
    tab = _table(views)
    _check_table(tab, x.numel() // D, int(mem.shape[0]))
    mask = _mask(key_mask, view_mask, tab, x.device)
    inputs = (x, mem, norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        n_groups(tab)   # a table the backward would refuse is refused here, before the forward runs
        return _Cross.apply(*inputs, tab, float(eps), mask)
    return cross_forward(_rows(x), _mem_rows(mem, width), tab, *(_opt(t) for t in inputs[2:]), float(eps), mask).view(x.shape)


def memory_rows(current_mem, new_rows, n_scenes):
    """The key rows of a memory update: per scene ``[Nm memory rows | V n new rows]``, the layout ``memory_views`` indexes, flattened to ``[B (Nm + V n), W]``.
    ``current_mem`` ``[B Nm, W]`` / ``[B, Nm, W]`` (``None`` or no rows: an empty memory), ``new_rows`` ``[B V n, W]`` / ``[B, V n, W]``; a ``torch.cat`` under
    autograd, so that the gradient of the key rows splits into the memory's and the new rows'."""
    B, W = int(n_scenes), int(new_rows.shape[-1])
    if B <= 0 or new_rows.numel() == 0 or (new_rows.numel() // W) % B:
        raise ValueError(f"memory_rows: {new_rows.numel() // max(W, 1)} new rows do not split into {B} scenes")
    new = new_rows.reshape(B, -1, W)
    if current_mem is None or current_mem.numel() == 0:
        return new.reshape(-1, W)
    if int(current_mem.shape[-1]) != W or (current_mem.numel() // W) % B:
        raise ValueError(f"memory_rows: a memory of shape {tuple(current_mem.shape)} beside new rows of width {W} for {B} scenes")
    return torch.cat([current_mem.reshape(B, -1, W), new], dim=1).reshape(-1, W)


class _CrossParams(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.projq, self.projk, self.projv, self.proj = _Proj(dim, dim), _Proj(dim, dim), _Proj(dim, dim), _Proj(dim, dim)


class CachedDecoderBlock(nn.Module):
    """The reference's ``CachedDecoderBlock`` as a trainable fp32 module; the parameters live under its state-dict keys (``norm1.*``, ``attn.qkv.*``,
    ``attn.proj.*``, ``norm2.*``, ``norm_y.*``, ``cross_attn.projq|projk|projv|proj.*``, ``norm3.*``, ``mlp.fc1.*``, ``mlp.fc2.*``)."""

    def __init__(self, dim=768, num_heads=12, mlp_ratio=4.0, memory_mode="norm_y", rope=(100.0, 1.0), eps=1e-6, npos=ROPE_NPOS):
        super().__init__()
        if memory_mode not in MEMORY_MODES:
            raise ValueError(f"CachedDecoderBlock: memory_mode {memory_mode!r}, expected one of {MEMORY_MODES}")
        self.dim, self.num_heads, self.eps, self.npos, self.memory_mode = int(dim), int(num_heads), float(eps), int(npos), memory_mode
        self.rope = (float(rope[0]), float(rope[1]))
        if self.dim != self.num_heads * HEAD:
            raise ValueError(f"CachedDecoderBlock: width {dim} is not num_heads * 64")
        self.norm1 = _Affine(self.dim)
        self.attn = _AttnParams(self.dim)
        self.norm2 = _Affine(self.dim)
        self.norm_y = _Affine(self.dim)
        self.cross_attn = _CrossParams(self.dim)
        self.norm3 = _Affine(self.dim)
        self.mlp = _MlpParams(self.dim, int(self.dim * mlp_ratio))

    @classmethod
    def from_params(cls, params, memory_mode=None, rope=(100.0, 1.0), npos=ROPE_NPOS):
        """fp32 copies of a loaded ``DecBlockParams`` (or anything with the same state-dict keys); the source is left alone.  ``memory_mode``: the source's
        by default."""
        sd = params.state_dict()
        dim, hidden = int(sd["norm1.weight"].shape[0]), int(sd["mlp.fc1.weight"].shape[0])
        mode = memory_mode if memory_mode is not None else getattr(params, "memory_mode", "norm_y")
        blk = cls(dim, dim // HEAD, hidden / dim, mode, rope, float(getattr(params.norm1, "eps", 1e-6)), npos)
        blk.load_state_dict({k: v.detach().to(torch.float32).clone() for k, v in sd.items()}, strict=True)
        return blk.to(sd["norm1.weight"].device)

    def prepare_y(self, y):
        """What the memory keeps of the tokens y (the reference's ``prepare_y``): y itself (``raw``), ``norm_y(y)`` (``norm_y``), or
        ``[projk(norm_y y) | projv(norm_y y)]`` (``kv``)."""
        if self.memory_mode == "raw":
            return y
        y_ = TB.layer_norm(y, self.norm_y.weight, self.norm_y.bias, self.eps)
        if self.memory_mode == "norm_y":
            return y_
        c = self.cross_attn
        return torch.cat([TB.linear(y_, c.projk.weight, c.projk.bias), TB.linear(y_, c.projv.weight, c.projv.bias)], dim=-1)

    def forward(self, x, y, pos, self_views=None, mem_views=None, key_mask=None, view_mask=None):
        """x ``[R, D]`` or ``[B, N, D]``, pos int64 ``[R, 2]`` / ``[B, N, 2]``, y the key rows in this block's memory mode, ``[Rk, W]`` or ``[B, Nk, W]``
        (W = 2 D in the ``kv`` mode, else D).  ``self_views`` / ``mem_views``: the tables of the self and the cross attention over the flattened rows of x
        (and of y).  Without tables: one view per batch entry that attends all of that entry's y (the reference's own calling form), one view for 2-d x.
        ``key_mask`` / ``view_mask``: packed key masks of the cross attention (``train_attention.pack_key_mask``) and each view's row of them."""
        B, N = (int(x.shape[0]), int(x.shape[1])) if x.ndim == 3 else (1, int(x.shape[0]))
        if self_views is None:
            self_views = _self_views(1, B, N)
        yk = y.reshape(-1, y.shape[-1])
        if mem_views is None:
            if int(yk.shape[0]) % B:
                raise ValueError(f"CachedDecoderBlock: {int(yk.shape[0])} key rows for {B} batch entries")
            Nk = int(yk.shape[0]) // B
            mem_views = [[b * N, N, b * Nk, Nk, 0, 0] for b in range(B)]
        c = self.cross_attn
        x = TB.attention_sublayer(x, pos, self_views, self.num_heads, self.norm1.weight, self.norm1.bias, self.attn.qkv.weight, self.attn.qkv.bias,
                                  self.attn.proj.weight, self.attn.proj.bias, self.rope, self.eps, self.npos)
        if self.memory_mode == "raw":
            yk = TB.layer_norm(yk, self.norm_y.weight, self.norm_y.bias, self.eps)
        kv = (None,) * 4 if self.memory_mode == "kv" else (c.projk.weight, c.projk.bias, c.projv.weight, c.projv.bias)
        x = cross_attention_sublayer(x, yk, mem_views, self.num_heads, self.norm2.weight, self.norm2.bias, c.projq.weight, c.projq.bias, *kv, c.proj.weight,
                                     c.proj.bias, self.eps, key_mask, view_mask)
        return TB.mlp_sublayer(x, self.norm3.weight, self.norm3.bias, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight, self.mlp.fc2.bias, self.eps)
