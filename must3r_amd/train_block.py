"""The transformer block with a backward pass: the reference's ``Block`` (blocks/layers.py:36-54, the encoder's block; its two residual sublayers are also
two of the three of ``CachedDecoderBlock``) under ``torch.autograd``::

    blk = Block.from_params(encoder.blocks_enc[3])                    # fp32 copies under the reference's state-dict keys
    y = blk(x, pos)                                                   # x [B, N, D] or [R, D], pos int64 [.., 2]; views default to one per batch entry
    loss(y).backward()                                                # x.grad, blk.*.grad
    train_optim.AdamW(blk.parameters()).step()                        # the native step (must3r_amd/train_optim.py); torch.optim.AdamW works too

    attention sublayer   x + proj(attn(rope(qkv(norm1 x))))           ``attention_sublayer``
    MLP sublayer         x + fc2(gelu(fc1(norm2 x)))                  ``mlp_sublayer``

Everything is stored in fp32 and, by default, runs on the fp32 MFMA (``must3r_hip_*_sublayer_forward`` / ``_grad``, include/must3r_hip.h ABI 21).  Inside
``with linear_precision("bf16"):`` the products of the Linears (``linear``, qkv, proj, fc1, fc2 and their data and weight gradients) round their operands to
bf16 and run on the 16-bit MFMA with fp32 accumulation, as ``--amp bf16`` does for ``nn.Linear``; LayerNorm, the attention core and its softmax, RoPE, GELU,
the bias and residual additions and the bias gradients stay fp32 in either mode.  ``with attention_precision("bf16"):`` does the same for the products of
the attention core (csrc/train_attn16.hip; the softmax stays fp32), and ``with amp("bf16"):`` enters both.  Each Function records ``current_precision()``
(and, where its backward reaches the core, ``current_attention_precision()``) in its forward and runs its backward in that mode, wherever and whenever ``backward()`` is called.  A forward saves its inputs and
nothing else; the backward recomputes the sublayer's forward into scratch and differentiates it.  Only the gradients ``needs_input_grad`` asks for are
computed (frozen weights: no weight-gradient launch; frozen norms: no column sums; a frozen ``x`` and frozen norms: no LayerNorm backward).  ``linear`` and
``layer_norm`` are the pieces on their own.  First order only (``once_differentiable``); gradients come back in the shape and dtype of their inputs; CPU
tensors raise.  Drop-path and dropout are not built (0 in this model).
"""
import ctypes as C
import weakref

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._train_common import HEAD, _Affine, _back, _call_sublayer, _check_params, _check_x, _dev, _f32, _new, _Proj, _ptr, _record_modes, _recorded_modes, _rows, _scratch, _stream
from ._train_common import current_precision, linear_precision   # noqa: F401  (re-exported: ``with train_block.linear_precision("bf16"):``)
from ._train_common import amp, attention_precision, current_attention_precision   # noqa: F401  (re-exported: ``with train_block.amp("bf16"):``)
from .train_attention import _check_table, _table, n_groups, self_views

ROPE_NPOS = 256          # positions of the default table (a 4096-pixel side), as the native model's
_rope_tables = {}


def rope_table(device, freq=100.0, f0=1.0, npos=ROPE_NPOS):
    """The fp32 table of ``must3r_hip_rope_table`` (``[npos, 16, 2]`` cos, sin) on ``device``; built once per (freq, f0, npos, device)."""
    key = (float(freq), float(f0), int(npos), str(torch.device(device)))
    if key not in _rope_tables:
        host = torch.empty((int(npos), 16, 2), dtype=torch.float32)
        _lib.check(_lib.load().must3r_hip_rope_table(float(freq), float(f0), int(npos), C.c_void_p(host.data_ptr())))
        _rope_tables[key] = host.to(device)
    return _rope_tables[key]


_checked_positions = [None]   # (weak reference, version, npos) of the last tensor that passed


def check_positions(pos, npos):
    """Refuses a position outside ``[0, npos)``: the kernels clamp, they do not report.  One reduction and one copy to the host per tensor: a tensor that
    passed and has not changed since (the same object at the same version) is not read again."""
    if pos.dtype != torch.int64 or pos.ndim < 1 or pos.shape[-1] != 2:
        raise ValueError(f"positions of dtype {pos.dtype} and shape {tuple(pos.shape)}, expected int64 [..., 2]")
    last = _checked_positions[0]
    if pos.numel() and not (last is not None and last[0]() is pos and last[1:] == (pos._version, int(npos))):
        lo, hi = torch.stack(torch.aminmax(pos)).tolist()
        if lo < 0 or hi >= int(npos):
            raise ValueError(f"a position outside [0, {int(npos)}): the RoPE table has {int(npos)} positions")
        _checked_positions[0] = (weakref.ref(pos), pos._version, int(npos))
    return pos


def _positions_checked(pos, npos):
    """Registers ``pos`` as a tensor that passed ``check_positions(pos, npos)`` without reading it: for a producer whose positions lie in ``[0, npos)`` by
    construction (``train_encoder``: a grid the host has compared with ``npos``), so that the blocks that follow do not copy its extremes to the host."""
    _checked_positions[0] = (weakref.ref(pos), pos._version, int(npos))
    return pos


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operator forms, on fp32 GPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
def linear_forward(x, W, b, epi=_lib.LIN_BIAS, res=None, want_z=False, out=None):
    """``must3r_hip_op_linear_f32``: x [M, K] (row stride >= K), W [N, K], b [N] or None -> out [M, N] (and z with ``want_z``, LIN_BIAS_GELU)."""
    M, K, N, dev = int(x.shape[0]), int(x.shape[1]), int(W.shape[0]), x.device
    out = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else out
    z = torch.empty((M, N), dtype=torch.float32, device=dev) if want_z else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_op_linear_f32(int(epi), _ptr(x), int(x.stride(0)) if M > 1 else K, _ptr(W), _ptr(b), _ptr(res),
                                                        0 if res is None else (int(res.stride(0)) if M > 1 else N), _ptr(out),
                                                        int(out.stride(0)) if M > 1 else N, _ptr(z), N, M, N, K, _stream(dev)))
    return (out, z) if want_z else out


def gelu_eval(z, want=(True, True)):
    """``must3r_hip_op_gelu_f32``: (gelu(z), gelu'(z)) of a contiguous fp32 tensor."""
    g, dg = (torch.empty_like(z) if w else None for w in want)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().must3r_hip_op_gelu_f32(_ptr(z), _ptr(g), _ptr(dg), z.numel(), _stream(z.device)))
    return g, dg


def gelu_grad(dh, z, out=None):
    """``must3r_hip_op_gelu_grad_f32``: dh gelu'(z) over [M, N] row-strided tensors; ``out=dh`` runs in place."""
    M, N = int(dh.shape[0]), int(dh.shape[1])
    out = torch.empty((M, N), dtype=torch.float32, device=dh.device) if out is None else out
    ld = lambda t: int(t.stride(0)) if M > 1 else N
    with torch.cuda.device(dh.device):
        _lib.check(_lib.load().must3r_hip_op_gelu_grad_f32(_ptr(dh), ld(dh), _ptr(z), ld(z), _ptr(out), ld(out), M, N, _stream(dh.device)))
    return out


def rope_rows(t, pos, tab, rope_cols, direction=1):
    """``must3r_hip_op_rope_f32`` in place over the first ``rope_cols`` columns of t [R, ld]; pos int64 [R, 2] and tab on the device."""
    R = int(t.shape[0])
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().must3r_hip_op_rope_f32(_ptr(t), int(t.stride(0)) if R > 1 else int(t.shape[1]), _ptr(pos), _ptr(tab), int(tab.shape[0]), R,
                                                      int(rope_cols), int(direction), _stream(t.device)))
    return t


def layernorm_forward(x, gamma, beta, eps):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().must3r_hip_op_layernorm_f32(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), int(x.shape[0]), int(x.shape[1]), float(eps),
                                                           _stream(x.device)))
    return y


def layernorm_grad(x, gamma, dy, eps, add=None, want=(True, True, True)):
    """``must3r_hip_op_layernorm_grad_add`` (``add=None``: ``must3r_hip_op_layernorm_grad``): ``(dx, dgamma, dbeta)``, ``None`` where ``want`` says so."""
    lib = _lib.load()
    M, D, dev = int(x.shape[0]), int(x.shape[1]), x.device
    dx, dg, db = _new(want[0], dev, M, D), _new(want[1], dev, D), _new(want[2], dev, D)
    if not any(want):
        return dx, dg, db
    with torch.cuda.device(dev):
        nbytes = lib.must3r_hip_op_layernorm_grad_scratch_bytes(M, D)
        scratch = _scratch(nbytes, dev)
        if add is None:
            _lib.check(lib.must3r_hip_op_layernorm_grad(_ptr(x), _ptr(gamma), _ptr(dy), _ptr(dx), _ptr(dg), _ptr(db), M, D, float(eps), _ptr(scratch), nbytes,
                                                        _stream(dev)))
        else:
            _lib.check(lib.must3r_hip_op_layernorm_grad_add(_ptr(x), _ptr(gamma), _ptr(dy), _ptr(add), _ptr(dx), _ptr(dg), _ptr(db), M, D, float(eps),
                                                            _ptr(scratch), nbytes, _stream(dev)))
    return dx, dg, db


def linear_grad(x, W, dy, want=(True, True, True)):
    """``(dx, dW, db)`` of ``x W^T + b`` through ``must3r_hip_op_linear_dgrad_f32`` / ``_wgrad_f32``."""
    lib = _lib.load()
    M, K, N, dev = int(x.shape[0]), int(x.shape[1]), int(W.shape[0]), x.device
    dx, dW, db = _new(want[0], dev, M, K), _new(want[1], dev, N, K), _new(want[2], dev, N)
    with torch.cuda.device(dev):
        if want[0]:
            _lib.check(lib.must3r_hip_op_linear_dgrad_f32(_ptr(dy), N, _ptr(W), _ptr(dx), M, N, K, _stream(dev)))
        if want[1] or want[2]:
            nbytes = lib.must3r_hip_op_linear_wgrad_scratch_bytes(M, N, K)
            scratch = _scratch(nbytes, dev)
            _lib.check(lib.must3r_hip_op_linear_wgrad_f32(_ptr(dy), N, _ptr(x), K, _ptr(dW), _ptr(db), M, N, K, _ptr(scratch), nbytes, _stream(dev)))
    return dx, dW, db


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sublayers, on contiguous fp32 GPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
MLP_OUTPUTS = ("dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2")
ATTN_OUTPUTS = ("dx", "dgamma", "dbeta", "dWqkv", "dbqkv", "dWproj", "dbproj")


def _mlp_args(x, gamma, beta, W1, b1, W2, b2, eps):
    a = _lib.MlpSublayerArgs()
    a.x, a.gamma, a.beta, a.W1, a.b1, a.W2, a.b2 = (_ptr(t) for t in (x, gamma, beta, W1, b1, W2, b2))
    a.M, a.D, a.hidden, a.eps = int(x.shape[0]), int(x.shape[1]), int(W1.shape[0]), float(eps)
    return a


def mlp_forward(x, gamma, beta, W1, b1, W2, b2, eps=1e-6):
    lib = _lib.load()
    a = _mlp_args(x, gamma, beta, W1, b1, W2, b2, eps)
    out = torch.empty_like(x)
    _call_sublayer(lib.must3r_hip_mlp_sublayer_forward, a, lib.must3r_hip_mlp_sublayer_scratch_bytes(a.M, a.D, a.hidden), x.device, out=out)
    return out


def mlp_grad(x, gamma, beta, W1, b1, W2, b2, dy, eps=1e-6, want=(True,) * 7):
    """``must3r_hip_mlp_sublayer_grad``: the gradients of MLP_OUTPUTS, ``None`` where ``want`` says so."""
    lib = _lib.load()
    a = _mlp_args(x, gamma, beta, W1, b1, W2, b2, eps)
    dev, D, Hd = x.device, a.D, a.hidden
    outs = [_new(w, dev, *s) for w, s in zip(want, (x.shape, (D,), (D,), (Hd, D), (Hd,), (D, Hd), (D,)))]
    if any(want):
        _call_sublayer(lib.must3r_hip_mlp_sublayer_grad, a, lib.must3r_hip_mlp_sublayer_scratch_bytes(a.M, D, Hd), dev, dy=dy, **dict(zip(MLP_OUTPUTS, outs)))
    return outs


def _attn_args(x, pos, tab, rope_tab, gamma, beta, Wqkv, bqkv, Wproj, bproj, eps):
    a = _lib.AttnSublayerArgs()
    a.x, a.gamma, a.beta, a.Wqkv, a.bqkv, a.Wproj, a.bproj = (_ptr(t) for t in (x, gamma, beta, Wqkv, bqkv, Wproj, bproj))
    a.pos, a.rope_tab, a.views = _ptr(pos), _ptr(rope_tab), C.c_void_p(tab.data_ptr())
    a.M, a.D, a.n_views, a.rope_npos, a.eps = int(x.shape[0]), int(x.shape[1]), int(tab.shape[0]), int(rope_tab.shape[0]), float(eps)
    return a


def attn_forward(x, pos, tab, rope_tab, gamma, beta, Wqkv, bqkv, Wproj, bproj, eps=1e-6):
    lib = _lib.load()
    a = _attn_args(x, pos, tab, rope_tab, gamma, beta, Wqkv, bqkv, Wproj, bproj, eps)
    out = torch.empty_like(x)
    _call_sublayer(lib.must3r_hip_attn_sublayer_forward, a, lib.must3r_hip_attn_sublayer_scratch_bytes(a.M, a.D, a.n_views), x.device, out=out)
    return out


def attn_grad(x, pos, tab, rope_tab, gamma, beta, Wqkv, bqkv, Wproj, bproj, dy, eps=1e-6, want=(True,) * 7):
    """``must3r_hip_attn_sublayer_grad``: the gradients of ATTN_OUTPUTS, ``None`` where ``want`` says so."""
    lib = _lib.load()
    a = _attn_args(x, pos, tab, rope_tab, gamma, beta, Wqkv, bqkv, Wproj, bproj, eps)
    dev, D = x.device, a.D
    outs = [_new(w, dev, *s) for w, s in zip(want, (x.shape, (D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,)))]
    if any(want):
        _call_sublayer(lib.must3r_hip_attn_sublayer_grad, a, lib.must3r_hip_attn_sublayer_scratch_bytes(a.M, D, a.n_views), dev, dy=dy, **dict(zip(ATTN_OUTPUTS, outs)))
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight, bias)
        _record_modes(ctx, linear=True)
        return linear_forward(_rows(x), _f32(weight), _f32(bias)).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight, bias = ctx.saved_tensors
        with _recorded_modes(ctx):
            grads = linear_grad(_rows(x), _f32(weight), _rows(grad_out), want=tuple(ctx.needs_input_grad[:3]))
        return tuple(_back(grads, (x, weight, bias)))


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ctx.save_for_backward(x, weight, bias)
        ctx.eps = eps
        return layernorm_forward(_rows(x), _f32(weight), _f32(bias), eps).view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight, bias = ctx.saved_tensors
        grads = layernorm_grad(_rows(x), _f32(weight), _rows(grad_out), ctx.eps, want=tuple(ctx.needs_input_grad[:3]))
        return (*_back(grads, (x, weight, bias)), None)


class _Mlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b, eps):
        ctx.save_for_backward(x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)
        ctx.eps = eps
        _record_modes(ctx, linear=True)
        return mlp_forward(_rows(x), *(_f32(t) for t in (norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)), eps).view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        with _recorded_modes(ctx):
            grads = mlp_grad(_rows(saved[0]), *(_f32(t) for t in saved[1:]), _rows(grad_out), ctx.eps, want=tuple(ctx.needs_input_grad[:7]))
        return (*_back(grads, saved), None)


class _Attn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b, pos, tab, rope_tab, eps):
        ctx.save_for_backward(x, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b, pos)
        ctx.tab, ctx.rope_tab, ctx.eps = tab, rope_tab, eps
        _record_modes(ctx, linear=True, attention=True)
        return attn_forward(_rows(x), pos, tab, rope_tab, *(_f32(t) for t in (norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b)), eps).view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        *saved, pos = ctx.saved_tensors
        with _recorded_modes(ctx):
            grads = attn_grad(_rows(saved[0]), pos, ctx.tab, ctx.rope_tab, *(_f32(t) for t in saved[1:]), _rows(grad_out), ctx.eps,
                              want=tuple(ctx.needs_input_grad[:7]))
        return (*_back(grads, saved), None, None, None, None)


def linear(x, weight, bias):
    """``x @ weight.T + bias`` in fp32 on the fp32 MFMA (under ``linear_precision("bf16")``: bf16 operands, fp32 accumulation and bias); x [..., K] with K % 16 == 0, weight [N, K] with N % 4 == 0, bias [N]."""
    K = _check_x(x, "linear: x")
    _check_params("linear", K, weight=(weight, (int(weight.shape[0]), K)), bias=(bias, (int(weight.shape[0]),)))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, weight, bias)):
        return _Linear.apply(x, weight, bias)
    return linear_forward(_rows(x), _f32(weight), _f32(bias)).view(*x.shape[:-1], weight.shape[0])


def layer_norm(x, weight, bias, eps=1e-6):
    """``nn.LayerNorm`` over the last dimension (a multiple of 64, at most 1024 for the backward) in fp32."""
    D = _check_x(x, "layer_norm: x")
    _check_params("layer_norm", D, weight=(weight, (D,)), bias=(bias, (D,)))
    if D % 64 or D > 1024:
        raise ValueError(f"layer_norm: width {D}, expected a multiple of 64 and at most 1024")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, weight, bias)):
        return _LayerNorm.apply(x, weight, bias, float(eps))
    return layernorm_forward(_rows(x), _f32(weight), _f32(bias), float(eps)).view(x.shape)


def mlp_sublayer(x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b, eps=1e-6):
    """``x + fc2(gelu(fc1(LN(x))))``; x [..., D], fc1_w [hidden, D], fc2_w [D, hidden]; differentiable at x and the six parameters."""
    D = _check_x(x, "mlp_sublayer: x")
    Hd = int(fc1_w.shape[0])
    _check_params("mlp_sublayer", D, norm_w=(norm_w, (D,)), norm_b=(norm_b, (D,)), fc1_w=(fc1_w, (Hd, D)), fc1_b=(fc1_b, (Hd,)), fc2_w=(fc2_w, (D, Hd)),
                  fc2_b=(fc2_b, (D,)))
    inputs = (x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs):
        return _Mlp.apply(*inputs, float(eps))
    return mlp_forward(_rows(x), *(_f32(t) for t in inputs[1:]), float(eps)).view(x.shape)


def attention_sublayer(x, pos, views, heads, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b, rope=(100.0, 1.0), eps=1e-6, npos=ROPE_NPOS):
    """``x + proj(attn(rope(qkv(LN(x)))))``; x [..., D] with D = heads * 64, pos int64 [..., 2] (y, x) per row on the GPU, ``views`` the 6-int table of
    ``train_attention`` over the flattened rows (``self_views``; ragged tables are fine), ``rope = (freq, f0)``; differentiable at x and the six
    parameters.  A position outside the table's ``npos`` positions is refused, and so is a table with a bad skip range (``skip_lo <= skip_hi <= nk``): with
    ``ValueError`` here, as in ``cross_attention_sublayer`` (it used to surface as ``HipError`` from the attention core)."""
    D = _check_x(x, "attention_sublayer: x")
    if int(heads) * HEAD != D:
        raise ValueError(f"attention_sublayer: width {D} is not heads * 64 = {int(heads) * HEAD}")
    _check_params("attention_sublayer", D, norm_w=(norm_w, (D,)), norm_b=(norm_b, (D,)), qkv_w=(qkv_w, (3 * D, D)), qkv_b=(qkv_b, (3 * D,)),
                  proj_w=(proj_w, (D, D)), proj_b=(proj_b, (D,)))
    _dev(pos, "pos")
    R = x.numel() // D
    check_positions(pos, npos)
    if pos.numel() != 2 * R:
        raise ValueError(f"attention_sublayer: {pos.numel() // 2} positions for {R} rows")
    pos = pos.reshape(R, 2).contiguous()
    tab = _table(views)
    _check_table(tab, R, R)
    rope_tab = rope_table(x.device, rope[0], rope[1], npos)
    inputs = (x, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b)
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs):
        n_groups(tab)   # a table the backward would refuse is refused here, before the forward runs
        return _Attn.apply(*inputs, pos, tab, rope_tab, float(eps))
    return attn_forward(_rows(x), pos, tab, rope_tab, *(_f32(t) for t in inputs[1:]), float(eps)).view(x.shape)


class _AttnParams(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv, self.proj = _Proj(dim, 3 * dim), _Proj(dim, dim)


class _MlpParams(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = _Proj(dim, hidden), _Proj(hidden, dim)


class Block(nn.Module):
    """The reference's ``Block`` as a trainable fp32 module; the parameters live under its state-dict keys (``norm1.*``, ``attn.qkv.*``, ``attn.proj.*``,
    ``norm2.*``, ``mlp.fc1.*``, ``mlp.fc2.*``)."""

    def __init__(self, dim=1024, num_heads=16, mlp_ratio=4.0, rope=(100.0, 1.0), eps=1e-6, npos=ROPE_NPOS):
        super().__init__()
        self.dim, self.num_heads, self.eps, self.npos = int(dim), int(num_heads), float(eps), int(npos)
        self.rope = (float(rope[0]), float(rope[1]))
        if self.dim != self.num_heads * HEAD:
            raise ValueError(f"Block: width {dim} is not num_heads * 64")
        self.norm1 = _Affine(self.dim)
        self.attn = _AttnParams(self.dim)
        self.norm2 = _Affine(self.dim)
        self.mlp = _MlpParams(self.dim, int(self.dim * mlp_ratio))

    @classmethod
    def from_params(cls, params, rope=(100.0, 1.0), npos=ROPE_NPOS):
        """fp32 copies of a loaded ``EncBlockParams`` (or anything with the same state-dict keys); the source is left alone."""
        sd = params.state_dict()
        dim, hidden = int(sd["norm1.weight"].shape[0]), int(sd["mlp.fc1.weight"].shape[0])
        blk = cls(dim, dim // HEAD, hidden / dim, rope, float(getattr(params.norm1, "eps", 1e-6)), npos)
        blk.load_state_dict({k: v.detach().to(torch.float32).clone() for k, v in sd.items()}, strict=True)
        return blk.to(sd["norm1.weight"].device)

    def forward(self, x, pos, views=None):
        """x ``[R, D]`` (one view of R tokens by default) or ``[B, N, D]`` (one view per batch entry by default), pos int64 ``[R, 2]`` / ``[B, N, 2]``."""
        if views is None:
            views = self_views(1, int(x.shape[0]), int(x.shape[1])) if x.ndim == 3 else self_views(1, 1, int(x.shape[0]))
        x = attention_sublayer(x, pos, views, self.num_heads, self.norm1.weight, self.norm1.bias, self.attn.qkv.weight, self.attn.qkv.bias,
                               self.attn.proj.weight, self.attn.proj.bias, self.rope, self.eps, self.npos)
        return mlp_sublayer(x, self.norm2.weight, self.norm2.bias, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight, self.mlp.fc2.bias, self.eps)
