"""Yardstick of the decoder block's training path (csrc/train_cross.hip, must3r_amd/train_cross.py): the cross-attention sublayer of the reference's
CachedDecoderBlock (blocks/layers.py:57-99) and the block itself in plain torch, generic in dtype, over flattened rows and the 6-int view tables of
must3r_amd.train_attention (query rows index x, key rows index the memory).  Runs under CPU autograd in fp64 (truth) and in fp32 (the reference's own precision).
The leaves are the oracle's (oracle/must3r_ref.py: layer_norm), the attention core of tests/attn_grad_ref.py and the two sublayers of tests/block_ref.py.  Also
the seeded case makers of tests/test_cross_grad_gpu.py and tests/test_cross_grad_host.py."""
import torch

import attn_grad_ref as AR
import block_ref as BR
from must3r_amd import train_attention as TA
from oracle import must3r_ref as R

HEAD = 64
MODES = ("norm_y", "kv", "raw")
ATTN_PARAMS = BR.ATTN_PARAMS
NORM_Y = ("norm_y.weight", "norm_y.bias")
CROSS_PARAMS = ("norm2.weight", "norm2.bias", "cross_attn.projq.weight", "cross_attn.projq.bias", "cross_attn.projk.weight", "cross_attn.projk.bias",
                "cross_attn.projv.weight", "cross_attn.projv.bias", "cross_attn.proj.weight", "cross_attn.proj.bias")
CROSS_PARAMS_KV = CROSS_PARAMS[:4] + CROSS_PARAMS[8:]          # the memory holds k | v: nothing is projected in the sublayer
MLP_PARAMS = ("norm3.weight", "norm3.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
# the reference's state-dict order
PARAMS = ATTN_PARAMS + CROSS_PARAMS[:2] + NORM_Y + CROSS_PARAMS[2:] + MLP_PARAMS


def cross_sublayer(x, mem, views, heads, p, kv_ready=False, eps=1e-6, keep=None):
    """x + proj(attn(projq(norm2 x), projk mem, projv mem)) on rows x [M, D] and mem [Rm, D]; kv_ready: mem [Rm, 2 D] holds k | v.  No RoPE.
    keep: a dict that receives the projected keys with their gradient retained (dK: the magnitude of what cancels in the key bias's gradient)."""
    D = heads * HEAD
    y = R.layer_norm(x, p["norm2.weight"], p["norm2.bias"], eps)
    q = y @ p["cross_attn.projq.weight"].t() + p["cross_attn.projq.bias"]
    if kv_ready:
        k, v = mem[:, :D], mem[:, D:]
    else:
        k = mem @ p["cross_attn.projk.weight"].t() + p["cross_attn.projk.bias"]
        v = mem @ p["cross_attn.projv.weight"].t() + p["cross_attn.projv.bias"]
        if keep is not None and k.requires_grad:
            k.retain_grad()
            keep["k"] = k
    o = AR.attention(q, k, v, views, heads)
    return x + o @ p["cross_attn.proj.weight"].t() + p["cross_attn.proj.bias"]


def mlp_sublayer(x, p, eps=1e-6):
    """x + fc2(gelu(fc1(norm3 x))): block_ref's MLP sublayer under the decoder block's norm."""
    q = {k: p[k] for k in MLP_PARAMS[2:]}
    q.update({"norm2.weight": p["norm3.weight"], "norm2.bias": p["norm3.bias"]})
    return BR.mlp_sublayer(x, q, eps)


def prepare_y(y, p, mode, eps=1e-6):
    """What the memory keeps of the tokens y (the reference's prepare_y)."""
    if mode == "raw":
        return y
    y_ = R.layer_norm(y, p["norm_y.weight"], p["norm_y.bias"], eps)
    if mode == "norm_y":
        return y_
    return torch.cat([y_ @ p["cross_attn.projk.weight"].t() + p["cross_attn.projk.bias"], y_ @ p["cross_attn.projv.weight"].t() + p["cross_attn.projv.bias"]], dim=1)


def memory_rows(mem, new, n_scenes):
    """per scene [Nm memory rows | V n new rows], flattened"""
    W = new.shape[-1]
    return torch.cat([mem.reshape(n_scenes, -1, W), new.reshape(n_scenes, -1, W)], dim=1).reshape(-1, W)


def block(x, y, pos, self_views, mem_views, heads, p, mode, rope=(100.0, 1.0), eps=1e-6, keep=None):
    """CachedDecoderBlock.forward on rows: y [Rk, W] are the key rows in the memory mode `mode`."""
    x = BR.attention_sublayer(x, pos, self_views, heads, p, rope, eps)
    y_ = R.layer_norm(y, p["norm_y.weight"], p["norm_y.bias"], eps) if mode == "raw" else y
    x = cross_sublayer(x, y_, mem_views, heads, p, mode == "kv", eps, keep)
    return mlp_sublayer(x, p, eps)


def make_params(D, hidden, g):
    """weights of the scale a trained Linear has (x 1.5 for the query and key projections: a softmax that is not flat), norms around 1, biases around 0.1"""
    rn = lambda *s: torch.randn(s, generator=g)
    p = {}
    for k in PARAMS:
        if k.startswith("norm"):
            p[k] = 1 + 0.1 * rn(D) if k.endswith("weight") else 0.1 * rn(D)
            continue
        out, inp = {"attn.qkv": (3 * D, D), "mlp.fc1": (hidden, D), "mlp.fc2": (D, hidden)}.get(k.rsplit(".", 1)[0], (D, D))
        if k.endswith("bias"):
            p[k] = 0.1 * rn(out)
        else:
            p[k] = rn(out, inp) * inp ** -0.5 * (1.5 if k.rsplit(".", 1)[0] in ("attn.qkv", "cross_attn.projq", "cross_attn.projk") else 1.0)
    return p


def make_cross_case(D, heads, views, M, Rm, seed, kv=False):
    """The cross sublayer alone: x [M, D], a memory of randn rows [Rm, D] (or [Rm, 2 D] = k | v), a table, an upstream gradient of order 1e-7."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    p = make_params(D, 4 * D, g)
    return dict(D=D, heads=heads, M=M, Rm=Rm, kv=kv, mode="kv" if kv else "norm_y", x=rn(M, D), mem=rn(Rm, 2 * D if kv else D), dy=rn(M, D) * 1e-7, params=p,
                views=[list(v) for v in views], eps=1e-6)


def make_block_case(D, heads, hidden, scenes, V, n, Nm, seed, mode="norm_y", width=8):
    """The block in the update form: `scenes` scenes of V views of n tokens on a grid `width` wide over Nm memory rows per scene; the key rows are
    memory_rows(mem, prepare_y(x)), masked so that a view does not attend its own tokens.  x and mem are the leaves."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    p = make_params(D, hidden, g)
    M = scenes * V * n
    return dict(D=D, heads=heads, hidden=hidden, scenes=scenes, V=V, n=n, Nm=Nm, M=M, mode=mode, x=rn(M, D), mem=rn(scenes * Nm, 2 * D if mode == "kv" else D),
                dy=rn(M, D) * 1e-7, params=p, self_views=TA.self_views(scenes, V, n), views=TA.memory_views(scenes, V, n, Nm, mask=True),
                pos=torch.cat([BR.grid_positions(n, width) for _ in range(scenes * V)]), rope=(100.0, 1.0), eps=1e-6)


def block_forward(case, x, mem, p, keep=None):
    y = memory_rows(mem, prepare_y(x, p, case["mode"], case["eps"]), case["scenes"])
    return block(x, y, case["pos"], case["self_views"], case["views"], case["heads"], p, case["mode"], case["rope"], case["eps"], keep)


def param_names(case, which):
    if which == "cross":
        return CROSS_PARAMS_KV if case["mode"] == "kv" else CROSS_PARAMS
    return PARAMS


def grads(case, dtype, which="block", extra=None):
    """dict out, dx, dmem and one entry per parameter (param_names) under CPU autograd in ``dtype``.  which: "cross" (a make_cross_case) or "block" (a
    make_block_case).  extra: a dict that receives "dK_colsum" = max_c sum_r |dK_rc| where the sublayer projects its keys."""
    x = case["x"].to(dtype).clone().requires_grad_(True)
    mem = case["mem"].to(dtype).clone().requires_grad_(True)
    p = {k: case["params"][k].to(dtype).clone().requires_grad_(True) for k in param_names(case, which)}
    keep = {}
    if which == "cross":
        out = cross_sublayer(x, mem, case["views"], case["heads"], p, case["kv"], case["eps"], keep)
    else:
        out = block_forward(case, x, mem, p, keep)
    out.backward(case["dy"].to(dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = dict(out=out.detach(), dx=x.grad, dmem=zero(mem))
    res.update({k: zero(t) for k, t in p.items()})
    if extra is not None and "k" in keep:
        extra["dK_colsum"] = float(keep["k"].grad.abs().sum(dim=0).max())
    return res
