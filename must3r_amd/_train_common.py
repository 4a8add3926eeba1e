"""What the training modules (``train_head``, ``train_attention``, ``train_block``, ``train_cross``, ``train_decoder``) share on the host: the checks that a tensor is on the GPU
and has the expected shape, the fp32 views handed to the library, scratch and output allocation, the one calling pattern of the sublayer entry points, and
the two parameter holders.  Everything here is private to the package."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib

HEAD = 64


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
