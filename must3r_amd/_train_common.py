"""What the training modules (``train_head``, ``train_attention``, ``train_block``, ``train_cross``, ``train_decoder``) share on the host: the checks that a tensor is on the GPU
and has the expected shape, the fp32 views handed to the library, scratch and output allocation, the one calling pattern of the sublayer entry points, and
the two parameter holders, and the precision switches of the training Linears and of the attention core (``linear_precision`` / ``current_precision``,
``attention_precision`` / ``current_attention_precision`` and ``amp``, re-exported by ``train_block``).
Everything else here is private to the package."""
import contextlib
import ctypes as C

import torch
import torch.nn as nn

from . import _lib

HEAD = 64

# ---------------------------------------------------------------------------------------------------------------------------------------
# the two per-thread precision switches (include/must3r_hip.h "ABI 21, additive"), independent of each other: the training Linears' products
# (must3r_hip_train_linear_mode) and the attention core's (must3r_hip_train_attention_mode)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _precision_switch(name, entry, modes, current_doc, doc):
    """``(current, switch)`` of the per-thread mode behind the library's ``entry``: ``current()`` names the calling thread's mode, ``switch(mode)`` is the context
    manager ``name`` that enters one of ``modes`` (``None``: leaves the mode alone, and calls nothing) and restores the previous mode on exit."""
    names = {v: k for k, v in modes.items()}

    def current():
        return names[getattr(_lib.load(), entry)(-1)]

    @contextlib.contextmanager
    def switch(mode):
        if mode is None:
            yield
            return
        if mode not in modes:
            raise ValueError(f"{name}: mode {mode!r}, expected one of {sorted(modes)} or None")
        lib = _lib.load()
        swap = getattr(lib, entry)
        prev = swap(modes[mode])
        if prev < 0:
            raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
        try:
            yield
        finally:
            swap(prev)

    current.__doc__, switch.__doc__ = current_doc, doc
    switch.__name__ = switch.__qualname__ = name
    return current, switch


PRECISIONS = {"fp32": _lib.TRAIN_LINEAR_F32, "bf16": _lib.TRAIN_LINEAR_BF16}
current_precision, linear_precision = _precision_switch(
    "linear_precision", "must3r_hip_train_linear_mode", PRECISIONS,
    """``"fp32"`` or ``"bf16"``: the mode in which the calling thread's training Linears multiply.""",
    """``with linear_precision("bf16"):`` -- inside, every Linear of the training path (``linear``, the MLP, attention and cross sublayers, the decoder's
    embedding and feedback Linears) rounds the two operands of its product to bf16 as it stages them, multiplies on the 16-bit MFMA and accumulates in fp32,
    like ``torch.autocast(dtype=torch.bfloat16)`` does for ``nn.Linear``; ``"fp32"`` is the default of every thread; ``None`` leaves the mode alone.  The mode
    belongs to the calling thread and is restored on exit, also after an exception.  Every training ``Function`` records the mode of its forward and runs its
    backward in it, whichever thread autograd uses and whether or not the ``with`` block has ended: a backward recomputes the forward it differentiates.

    Narrower than autocast: everything in memory stays fp32 (activations, weights, gradients, scratch), and LayerNorm, the attention core (scores, softmax,
    P V), RoPE, GELU, the bias and residual additions, bias gradients, the head (``train_head``), the losses and the optimizer compute in fp32 in either mode.""")

ATTENTION_PRECISIONS = {"fp32": _lib.TRAIN_ATTENTION_F32, "bf16": _lib.TRAIN_ATTENTION_BF16}
current_attention_precision, attention_precision = _precision_switch(
    "attention_precision", "must3r_hip_train_attention_mode", ATTENTION_PRECISIONS,
    """``"fp32"`` or ``"bf16"``: the mode in which the calling thread's training attention core multiplies.""",
    """``with attention_precision("bf16"):`` -- inside, the attention core of the training path (``train_attention.attention``, the attention and cross
    sublayers, masked forms included, and everything composed of them) rounds Q, K, V and dO, and P and dS as operands of the products that follow them, to
    bf16 in registers and multiplies on the 16-bit MFMA with fp32 accumulation, as the core does under ``torch.autocast(dtype=torch.bfloat16)``; the scores,
    the softmax, its row sum, lse, delta and dS are computed in fp32 and all storage stays fp32.  ``"fp32"`` is the default of every thread; ``None`` leaves the
    mode alone.  The contract is ``linear_precision``'s: the mode belongs to the calling thread, is restored on exit (also after an exception), and every
    ``Function`` whose backward reaches the core records the mode of its forward and runs its backward in it.  The two modes do not touch each other;
    ``amp`` enters both.""")


def _record_modes(ctx, linear=False, attention=False):
    """A ``Function``'s forward: note on ``ctx`` the calling thread's mode of each switch that its backward reaches (``None`` for one it does not)."""
    ctx.modes = (current_precision() if linear else None, current_attention_precision() if attention else None)


@contextlib.contextmanager
def _recorded_modes(ctx):
    """The ``Function``'s backward runs inside this: the modes ``_record_modes`` noted in its forward, whichever thread autograd uses and whether or not the
    caller's ``with`` block has ended -- a backward recomputes the forward it differentiates."""
    linear, attention = ctx.modes
    with linear_precision(linear), attention_precision(attention):
        yield


@contextlib.contextmanager
def amp(mode):
    """``with amp("bf16"):`` -- the recipe's ``--amp bf16`` for the training path: ``linear_precision(mode)`` and ``attention_precision(mode)`` together
    (``"fp32"``, ``"bf16"``, or ``None`` for no change)."""
    if mode is not None and mode not in PRECISIONS:
        raise ValueError(f"amp: mode {mode!r}, expected one of {sorted(PRECISIONS)} or None")
    with linear_precision(mode), attention_precision(mode):
        yield


def _dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"must3r_amd training: {what} must be a tensor on the GPU (there is no CPU path)")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _stream(dev):
    return C.c_void_p(_lib.stream_ptr(dev))


def _scratch(nbytes, dev):
    """``nbytes`` is the answer of a scratch query: 0 means the query refused the shape and left its reason in the library's last error."""
    if not nbytes:
        raise _lib.HipError(_lib.load().must3r_hip_last_error().decode("utf-8", "replace") or "bad shape")
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def _new(need, dev, *shape):
    return torch.empty(shape, dtype=torch.float32, device=dev) if need else None


def _ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _rows(t):
    return _f32(t).view(-1, t.shape[-1])


def _strided_rows(t, width):
    """fp32 [R, width] with a contiguous last dimension and a row stride the kernels take, without a copy where possible."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.stride(1) != 1 or t.data_ptr() % 16 or (t.shape[0] > 1 and (t.stride(0) % 4 or t.stride(0) < width)):
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _back(grads, saved):
    return [None if g is None else g.reshape(t.shape).to(t.dtype) for g, t in zip(grads, saved)]


def _check_x(x, what):
    _dev(x, what)
    if x.ndim < 2 or x.numel() == 0:
        raise ValueError(f"{what} of shape {tuple(x.shape)}, expected [..., D] with rows")
    return int(x.shape[-1])


def _check_params(name, D, **shapes):
    for n, (t, shape) in shapes.items():
        _dev(t, n)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {n} of shape {tuple(t.shape)}, expected {shape} for tokens of width {D}")


def _call_sublayer(entry, a, nbytes, dev, **tensors):
    """The common end of the sublayer wrappers: set ``tensors`` in the descriptor ``a`` by name, allocate the ``nbytes`` of scratch its scratch query asked for
    and call ``entry``.  The stream travels in the descriptor where it has a field for it (set by whoever built ``a``), else as the last argument."""
    for n, t in tensors.items():
        setattr(a, n, _ptr(t))
    with torch.cuda.device(dev):
        scratch = _scratch(nbytes, dev)
        _lib.check(entry(C.byref(a), _ptr(scratch), nbytes, *(() if hasattr(a, "stream") else (_stream(dev),))))


class _Affine(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _Proj(nn.Module):
    def __init__(self, dim, out):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out, dim))
        self.bias = nn.Parameter(torch.zeros(out))
        nn.init.xavier_uniform_(self.weight)
