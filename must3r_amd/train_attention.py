"""The attention core with a backward pass: ``softmax(Q K^T / 8) V`` per head of 64 (``CoreAttention.attention``, blocks/attention.py) under
``torch.autograd``, driven by the 6-int view table of the native decoder (q_row0, nq, kv_row0, nk, skip_lo, skip_hi)::

    qkv = ...                                                         # [R, 3 D] fp32, D = heads * 64
    views = self_views(n_scenes, views_per_scene, n)                  # or memory_views(...) for the cross attention over a scene's memory
    o = attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], views, heads)
    loss(o).backward()                                                # qkv.grad

The fp32 forward (``must3r_hip_attn_forward_f32``) and the backward (``must3r_hip_attn_grad``, include/must3r_hip.h ABI 20) run fp32 operands on the fp32
MFMA; the forward saves q, k, v and the host table and nothing else, the backward recomputes the scores.  ``dtype=_lib.F16`` / ``_lib.BF16`` runs the
native inference forward (``must3r_hip_op_attention``) on cast operands instead, so that a fine-tuned model sees the arithmetic it will be served with; the
backward is the same fp32 one.  Inside ``with attention_precision("bf16"):`` (``must3r_hip_train_attention_mode``, a mode of the calling thread) both
entry points, masked forms included, run their bf16 siblings on the 16-bit MFMA (csrc/train_attn16.hip): Q, K, V, dO, and P and dS as operands, rounded to
bf16 in registers, fp32 softmax, accumulation and storage; a backward runs in the mode of its forward.  Only the gradients ``needs_input_grad`` asks for are computed.  dK and dV sum over every view that reads a key row:
views that share key rows must share ``kv_row0`` (one key group; the decoder's tables do), and overlapping groups are refused.  A query row without a
valid key has O = 0 and zero gradients (the reference would give NaN).  First order only (``once_differentiable``); CPU tensors raise.

Key masks (memory dropout): ``attention(..., key_mask=bits, view_mask=rows)`` hides further keys from a view.  ``bits`` is a packed GPU tensor ``[rows, ld]``
(``pack_key_mask(keep)`` from a bool ``[rows, nk]``: bit ``j % 32`` of word ``j // 32`` set where key j is kept, ``ld`` even), ``view_mask`` names each view's
row of it, -1 for none; rows are shared freely among views.  The fp32 kernels test the bits on top of the table (``must3r_hip_attn_masked_forward`` /
``_grad``, ABI 21, additive) and skip a key tile whose 64 bits are all zero; the 16-bit inference forward has no masks.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._train_common import HEAD, _dev, _ld, _ptr, _record_modes, _recorded_modes, _stream, _strided_rows
from ._train_common import attention_precision, current_attention_precision   # noqa: F401  (re-exported: ``with train_attention.attention_precision("bf16"):``)


def self_views(n_scenes, views_per_scene, n):
    """The decoder's self-attention table (model.hip, decode_tables): view j of scene b attends its own ``n`` tokens at rows ``(b V + j) n``."""
    return [[(b * views_per_scene + j) * n, n, (b * views_per_scene + j) * n, n, 0, 0] for b in range(n_scenes) for j in range(views_per_scene)]


def memory_views(n_scenes, views_per_scene, n, Nm, mask=True, causal=False):
    """The decoder's cross-attention table of a memory update (model.hip, decode_tables): scene b's keys are ``Nm`` memory rows followed by the ``V n`` new
    tokens, at rows ``b (Nm + V n)``; the queries are the scene's views at rows ``(b V + j) n``.  ``mask``: view j does not attend its own tokens (skip
    ``[Nm + j n, Nm + (j + 1) n)``); ``causal`` (with ``mask``): view j attends the memory and the views before it, a prefix of ``Nm + j n`` rows -- with
    an empty memory view 0 attends view 1's tokens instead, rows ``[n, 2 n)`` behind an excluded ``[0, n)``.  A lone view attends the memory alone."""
    V, Rs = views_per_scene, views_per_scene * n
    out = []
    for b in range(n_scenes):
        for j in range(V):
            q0, k0 = (b * V + j) * n, b * (Nm + Rs)
            if V == 1:
                out.append([q0, n, k0, Nm, 0, 0])
            elif mask and causal:
                out.append([q0, n, k0, 2 * n, 0, n] if Nm == 0 and j == 0 else [q0, n, k0, Nm + j * n, 0, 0])
            elif mask:
                out.append([q0, n, k0, Nm + Rs, Nm + j * n, Nm + (j + 1) * n])
            else:
                out.append([q0, n, k0, Nm + Rs, 0, 0])
    return out


def _table(views):
    t = torch.as_tensor(views, dtype=torch.int32).cpu().contiguous()
    if t.ndim != 2 or t.shape[1] != 6 or t.shape[0] == 0:
        raise ValueError(f"attention: views of shape {tuple(t.shape)}, expected [n, 6] with n > 0")
    return t


def n_groups(views):
    """Number of key groups of a table (``must3r_hip_attn_train_groups``); raises where the backward would refuse the table."""
    t = _table(views)
    n = _lib.load().must3r_hip_attn_train_groups(C.c_void_p(t.data_ptr()), int(t.shape[0]))
    if n < 0:
        raise _lib.HipError(_lib.load().must3r_hip_last_error().decode("utf-8", "replace"))
    return n


def _covers(spans, rows):
    """Do the half-open spans cover [0, rows)?"""
    end = 0
    for lo, hi in sorted(s for s in spans if s[1] > s[0]):
        if lo > end:
            return False
        end = max(end, hi)
    return end >= rows


def q_spans(tab):
    return [(int(v[0]), int(v[0] + v[1])) for v in tab.tolist()]


def kv_spans(tab):
    ext = {}
    for v in tab.tolist():
        ext[v[2]] = max(ext.get(v[2], 0), v[3])
    return [(k, k + e) for k, e in ext.items()]


def _fp32_rows(t, what, heads):
    """fp32 [R, heads * 64] with a contiguous last dimension and a row stride the kernels take, without a copy where possible."""
    if t.ndim != 2 or t.shape[1] != heads * HEAD:
        raise ValueError(f"attention: {what} of shape {tuple(t.shape)}, expected [rows, {heads * HEAD}]")
    return _strided_rows(t, heads * HEAD)


def _check_table(tab, Rq, Rk):
    """Runs on the host before the first launch of every forward: numpy on the CPU table's own memory (a third of the time of the same torch expressions)."""
    v = tab.numpy().astype(np.int64)
    if (v < 0).any():
        raise ValueError("attention: negative table entry")
    if (v[:, 0] + v[:, 1]).max() > Rq or (v[:, 2] + v[:, 3]).max() > Rk:
        raise ValueError(f"attention: the table reaches past the {Rq} query rows or the {Rk} key rows")
    if (v[:, 4] > v[:, 5]).any() or (v[:, 5] > v[:, 3]).any():
        raise ValueError("attention: a skip range needs skip_lo <= skip_hi <= nk")


def pack_key_mask(keep):
    """bool ``[rows, nk]`` (True: the key is kept) -> int32 ``[rows, ld]`` on the same device, bit ``j % 32`` of word ``j // 32`` for key j, ``ld`` the even
    number of words that covers nk (at least 2); the bits past nk are zero.  Torch ops on the tensor's device, no host synchronisation."""
    if keep.ndim != 2 or keep.dtype != torch.bool:
        raise ValueError(f"pack_key_mask: a {keep.dtype} tensor of shape {tuple(keep.shape)}, expected bool [rows, nk]")
    rows, nk = int(keep.shape[0]), int(keep.shape[1])
    ld = max(2, (nk + 63) // 64 * 2)
    bits = torch.zeros((rows, ld * 32), dtype=torch.int64, device=keep.device)
    bits[:, :nk] = keep
    weights = torch.ones(32, dtype=torch.int64, device=keep.device) << torch.arange(32, dtype=torch.int64, device=keep.device)
    words = (bits.view(rows, ld, 32) * weights).sum(dim=2)                       # in [0, 2^32)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)   # the same 32 bits as an int32


def _mask(key_mask, view_mask, tab, dev):
    """``(bits, rows)`` checked against the table -- an int32 / uint32 GPU tensor ``[rows, ld]`` with ld even and an int32 CPU tensor ``[n_views]`` -- or
    ``None`` without masks."""
    if key_mask is None and view_mask is None:
        return None
    if key_mask is None or view_mask is None:
        raise ValueError("attention: key_mask and view_mask come together")
    if not isinstance(key_mask, torch.Tensor) or key_mask.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or key_mask.ndim != 2:
        raise ValueError("attention: key_mask must be a packed int32 or uint32 tensor [rows, ld] (pack_key_mask)")
    if key_mask.device != dev:
        raise ValueError(f"attention: key_mask on {key_mask.device}, the operands on {dev}")
    rows, ld = int(key_mask.shape[0]), int(key_mask.shape[1])
    if ld <= 0 or ld % 2:
        raise ValueError(f"attention: key_mask of {ld} words per row, expected a positive even number")
    vm = torch.as_tensor(view_mask, dtype=torch.int32).cpu().contiguous()
    if vm.ndim != 1 or int(vm.shape[0]) != int(tab.shape[0]):
        raise ValueError(f"attention: view_mask of shape {tuple(vm.shape)} for a table of {int(tab.shape[0])} views")
    r = vm.numpy()
    if (r < -1).any() or (r >= rows).any():
        raise ValueError(f"attention: a view_mask entry outside [-1, {rows})")
    if (tab.numpy()[:, 3][r >= 0] > 32 * ld).any():
        raise ValueError(f"attention: a mask row of {32 * ld} bits is shorter than the nk of a view that names it")
    return key_mask.contiguous(), vm


def _masked_args(a, mask, dev):
    m = _lib.AttnMaskedArgs()
    m.core = a
    bits, vm = mask
    m.mask_bits, m.view_mask = _ptr(bits), C.c_void_p(vm.data_ptr())
    m.mask_rows, m.mask_ld = int(bits.shape[0]), int(bits.shape[1])
    m.stream = _stream(dev)
    return m


def _args(q, k, v, tab, heads):
    a = _lib.AttnTrainArgs()
    a.q, a.k, a.v = _ptr(q), _ptr(k), _ptr(v)
    a.ldq, a.ldk, a.ldv = _ld(q), _ld(k), _ld(v)
    a.heads, a.n_views, a.views = heads, int(tab.shape[0]), C.c_void_p(tab.data_ptr())
    return a


def _scratch(tab, heads, dev, masked=False):
    lib = _lib.load()
    v = tab.to(torch.int64)
    nbytes = (lib.must3r_hip_attn_masked_scratch_bytes if masked else lib.must3r_hip_attn_train_scratch_bytes)(int(tab.shape[0]), int((v[:, 0] + v[:, 1]).max()), int((v[:, 2] + v[:, 3]).max()), heads)
    if not nbytes:
        raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def _new(rows, cols, dev, covered):
    return (torch.empty if covered else torch.zeros)((rows, cols), dtype=torch.float32, device=dev)


def attention_forward(q, k, v, tab, heads, want_lse=False, mask=None):
    """``must3r_hip_attn_forward_f32`` on fp32 row-strided tensors and an int32 CPU table: O [Rq, heads * 64] (zeros in rows of no view), and lse
    [Rq, heads] (natural log) with ``want_lse``.  ``mask``: ``(bits, rows)`` of ``_mask``, through ``must3r_hip_attn_masked_forward``."""
    lib = _lib.load()
    dev, Rq = q.device, int(q.shape[0])
    covered = _covers(q_spans(tab), Rq)
    o = _new(Rq, heads * HEAD, dev, covered)
    lse = _new(Rq, heads, dev, covered) if want_lse else None
    a = _args(q, k, v, tab, heads)
    a.O, a.ldo, a.lse = _ptr(o), heads * HEAD, _ptr(lse)
    with torch.cuda.device(dev):
        scratch, nbytes = _scratch(tab, heads, dev, mask is not None)
        if mask is None:
            _lib.check(lib.must3r_hip_attn_forward_f32(C.byref(a), _ptr(scratch), nbytes, _stream(dev)))
        else:
            _lib.check(lib.must3r_hip_attn_masked_forward(C.byref(_masked_args(a, mask, dev)), _ptr(scratch), nbytes))
    return (o, lse) if want_lse else o


def attention_forward16(q, k, v, tab, heads, dtype):
    """The native inference forward (``must3r_hip_op_attention``) on operands cast to the 16-bit type of ``dtype``, cast back to fp32."""
    lib = _lib.load()
    if dtype not in (_lib.F16, _lib.BF16):
        raise ValueError("attention: dtype must be None, _lib.F16 or _lib.BF16")
    dev, Rq = q.device, int(q.shape[0])
    td = torch.float16 if dtype == _lib.F16 else torch.bfloat16
    q16, k16, v16 = (t.to(td).contiguous() for t in (q, k, v))
    o16 = (torch.empty if _covers(q_spans(tab), Rq) else torch.zeros)((Rq, heads * HEAD), dtype=td, device=dev)
    tab_dev = tab.to(dev)
    D = heads * HEAD
    with torch.cuda.device(dev):
        _lib.check(lib.must3r_hip_op_attention(dtype, _ptr(q16), _ptr(k16), _ptr(v16), _ptr(o16), D, D, D, D, heads, _ptr(tab_dev), int(tab.shape[0]),
                                               int(tab[:, 1].max()), 0, None, 0, _stream(dev)))
    return o16.to(torch.float32)


def attention_grad(q, k, v, dO, tab, heads, want=(True, True, True), mask=None):
    """``must3r_hip_attn_grad`` on fp32 row-strided tensors: ``(dQ, dK, dV)``, ``None`` where ``want`` says so; zeros in rows the table leaves out.
    ``mask``: ``(bits, rows)`` of ``_mask``, through ``must3r_hip_attn_masked_grad``."""
    lib = _lib.load()
    dev, D = q.device, heads * HEAD
    dq = _new(int(q.shape[0]), D, dev, _covers(q_spans(tab), int(q.shape[0]))) if want[0] else None
    kv_covered = _covers(kv_spans(tab), int(k.shape[0]))
    dk = _new(int(k.shape[0]), D, dev, kv_covered) if want[1] else None
    dv = _new(int(v.shape[0]), D, dev, kv_covered) if want[2] else None
    if not any(want):
        return None, None, None
    a = _args(q, k, v, tab, heads)
    a.dO, a.lddo = _ptr(dO), _ld(dO)
    a.dQ, a.dK, a.dV, a.lddq, a.lddk, a.lddv = _ptr(dq), _ptr(dk), _ptr(dv), D, D, D
    with torch.cuda.device(dev):
        scratch, nbytes = _scratch(tab, heads, dev, mask is not None)
        if mask is None:
            _lib.check(lib.must3r_hip_attn_grad(C.byref(a), _ptr(scratch), nbytes, _stream(dev)))
        else:
            _lib.check(lib.must3r_hip_attn_masked_grad(C.byref(_masked_args(a, mask, dev)), _ptr(scratch), nbytes))
    return dq, dk, dv


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, tab, heads, dtype, mask=None):
        ctx.save_for_backward(q, k, v)
        ctx.tab, ctx.heads, ctx.mask = tab, heads, mask
        _record_modes(ctx, attention=True)
        return _forward(q, k, v, tab, heads, dtype, mask)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v = ctx.saved_tensors
        heads = ctx.heads
        f = [_fp32_rows(t, n, heads) for t, n in ((q, "q"), (k, "k"), (v, "v"), (grad_out, "the upstream gradient"))]
        with _recorded_modes(ctx):   # autograd's thread starts in the default mode, and backward() may run after the block has ended
            grads = attention_grad(*f, ctx.tab, heads, want=tuple(ctx.needs_input_grad[:3]), mask=ctx.mask)
        out = [None if g is None else g.to(t.dtype) for g, t in zip(grads, (q, k, v))]
        return (*out, None, None, None, None)


def _forward(q, k, v, tab, heads, dtype, mask=None):
    f = [_fp32_rows(t, n, heads) for t, n in ((q, "q"), (k, "k"), (v, "v"))]
    return attention_forward(*f, tab, heads, mask=mask) if dtype is None else attention_forward16(*f, tab, heads, int(dtype))


def attention(q, k, v, views, heads, dtype=None, key_mask=None, view_mask=None):
    """O ``[Rq, heads * 64]`` fp32 from q ``[Rq, heads * 64]`` and k, v ``[Rk, heads * 64]`` (fp32 GPU tensors, possibly column slices of one packed tensor:
    the last dimension contiguous, the row stride is passed through) and ``views`` (int32 CPU tensor or list ``[n][6]``); differentiable at q, k and v.
    ``dtype``: ``None`` for the fp32 forward, ``_lib.F16`` / ``_lib.BF16`` for the native inference forward on cast operands.  ``key_mask`` / ``view_mask``:
    packed key masks ``[rows, ld]`` on the GPU (``pack_key_mask``) and each view's row of them (list or int32 CPU tensor, -1: none); they need ``dtype=None``
    and are saved for the backward like the table."""
    heads = int(heads)
    if heads <= 0:
        raise ValueError("attention: heads must be positive")
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        _dev(t, what)
        if t.ndim != 2 or t.shape[1] != heads * HEAD:
            raise ValueError(f"attention: {what} of shape {tuple(t.shape)}, expected [rows, {heads * HEAD}]")
    if k.shape[0] != v.shape[0]:
        raise ValueError("attention: k and v differ in their row counts")
    if dtype is not None and int(dtype) not in (_lib.F16, _lib.BF16):
        raise ValueError("attention: dtype must be None, _lib.F16 or _lib.BF16")
    tab = _table(views)
    _check_table(tab, int(q.shape[0]), int(k.shape[0]))
    mask = _mask(key_mask, view_mask, tab, q.device)
    if mask is not None and dtype is not None:
        raise ValueError("attention: key masks need dtype=None (the native 16-bit inference forward has no masks)")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        n_groups(tab)   # a table the backward would refuse is refused here, before the forward runs
        return _Attention.apply(q, k, v, tab, heads, dtype, mask)
    return _forward(q, k, v, tab, heads, dtype, mask)
