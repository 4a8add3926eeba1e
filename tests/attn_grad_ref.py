"""Yardstick of the attention training path (csrc/train_attention.hip): the formulas of include/must3r_hip.h ABI 20 in plain torch, with a boolean
mask built from the 6-int view table.  Runs under CPU autograd in fp64 (truth) and in fp32 (the reference's own precision).  A view without a valid
key gives O = 0 through ``masked_fill`` after the softmax (whose input is left unmasked there), so nothing here ever produces NaN.  Also the case
makers of tests/test_attn_grad_gpu.py, with fixed seeds."""
import torch

from must3r_amd import train_attention as TA

HEAD = 64
NAMES = ("O", "dQ", "dK", "dV")


def valid_mask(view):
    """bool [nk]: which keys of the view's range a query attends."""
    _, _, _, nk, lo, hi = view
    j = torch.arange(nk)
    return ~((j >= lo) & (j < hi))


def attention(q, k, v, views, heads):
    """O [Rq, heads * 64] in the dtype of q; rows of no view stay 0."""
    o = q.new_zeros(q.shape)
    for view in views:
        q0, nq, k0, nk, _, _ = view
        if nq == 0:
            continue
        valid = valid_mask(view).to(q.device)
        qh = q[q0:q0 + nq].reshape(nq, heads, HEAD).transpose(0, 1)
        kh = k[k0:k0 + nk].reshape(nk, heads, HEAD).transpose(0, 1)
        vh = v[k0:k0 + nk].reshape(nk, heads, HEAD).transpose(0, 1)
        s = qh @ kh.transpose(1, 2) / 8
        if bool(valid.any()):
            s = s.masked_fill(~valid, float("-inf"))
        p = torch.softmax(s, dim=-1).masked_fill(~valid, 0) if nk else s
        o[q0:q0 + nq] = (p @ vh).transpose(0, 1).reshape(nq, heads * HEAD)
    return o


def bool_mask(view):
    """[nq, nk] for torch.nn.functional.scaled_dot_product_attention."""
    return valid_mask(view)[None, :].expand(view[1], view[3])


def grads(case, dtype):
    """dict O, dQ, dK, dV of the case under CPU autograd in ``dtype``."""
    q, k, v = (case[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v"))
    o = attention(q, k, v, case["views"], case["heads"])
    o.backward(case["dO"].to(dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(O=o.detach(), dQ=zero(q), dK=zero(k), dV=zero(v))


def _tensors(Rq, Rk, heads, seed, q_scale, packed=False):
    g = torch.Generator().manual_seed(seed)
    D = heads * HEAD
    if packed:
        assert Rq == Rk
        qkv = torch.randn((Rq, 3 * D), generator=g)
        qkv[:, :D] *= q_scale
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        qkv = None
        q, k, v = torch.randn((Rq, D), generator=g) * q_scale, torch.randn((Rk, D), generator=g), torch.randn((Rk, D), generator=g)
    return dict(q=q, k=k, v=v, qkv=qkv, dO=torch.randn((Rq, D), generator=g) * 1e-7, heads=heads)


def make_case(name):
    """The cases of the GPU tests: the smallest shapes at which each mechanism can fail (tests/test_attn_grad_gpu.py)."""
    if name == "self_ragged":        # 70 = one full 64-tile and a 6-row tail on both axes; q, k, v are the column blocks of one packed [210][384]
        c = _tensors(210, 210, 2, 11, 2.0, packed=True)
        c["views"] = TA.self_views(1, 3, 70)
    elif name == "self_tiny":        # all tail
        c = _tensors(6, 6, 2, 12, 1.0)
        c["views"] = TA.self_views(1, 1, 6)
    elif name == "self_12h":         # full tiles, the model's 12 heads, a peaked softmax
        c = _tensors(128, 128, 12, 13, 3.0)
        c["views"] = TA.self_views(1, 1, 128)
    elif name == "cross_shared":     # nk = 224; skips [80,128) (ends on a tile boundary), [128,176) (starts on one), [176,224) (ends at nk)
        c = _tensors(2 * 3 * 48, 2 * 224, 2, 14, 2.0)
        c["views"] = TA.memory_views(2, 3, 48, 80, mask=True)
    elif name == "cross_whole_tile":  # nk = 288; the skip of view 1, [128,208), contains the whole key tile [128,192)
        c = _tensors(3 * 80, 288, 2, 15, 4.0)
        c["views"] = TA.memory_views(1, 3, 80, 48, mask=True)
    elif name == "causal":           # nested prefixes of one group per scene; view 0 has the excluded [0, n) form
        c = _tensors(2 * 3 * 48, 2 * 144, 2, 16, 2.0)
        c["views"] = TA.memory_views(2, 3, 48, 0, mask=True, causal=True)
    elif name == "degenerate":       # a normal view, one without keys, one whose skip covers all its keys: one group
        c = _tensors(90, 70, 2, 17, 2.0)
        c["views"] = [[0, 40, 0, 70, 0, 0], [40, 20, 0, 0, 0, 0], [60, 30, 0, 70, 0, 70]]
    else:
        raise KeyError(name)
    return c


CASES = ("self_ragged", "self_tiny", "self_12h", "cross_shared", "cross_whole_tile", "causal", "degenerate")
