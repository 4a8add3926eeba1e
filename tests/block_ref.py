"""Yardstick of the block training path (csrc/train_block.hip, must3r_amd/train_block.py): the two residual sublayers of the reference's Block
(blocks/layers.py:36-54) and the block itself in plain torch, generic in dtype, over flattened rows [R, D] and the 6-int view table of
must3r_amd.train_attention.  Runs under CPU autograd in fp64 (truth) and in fp32 (the reference's own precision).  The leaves are the oracle's
(oracle/must3r_ref.py: layer_norm, the erf GELU, rope2d with its fp32 table) and the attention core of tests/attn_grad_ref.py.  Also the seeded case maker
of tests/test_block_grad_gpu.py and tests/test_block_grad_host.py."""
import torch

import attn_grad_ref as AR
from oracle import must3r_ref as R

HEAD = 64
ATTN_PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias")
MLP_PARAMS = ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
PARAMS = ATTN_PARAMS + MLP_PARAMS
WHICH = {"attn": ATTN_PARAMS, "mlp": MLP_PARAMS, "block": PARAMS}


def rope_rows(t, pos, heads, rope):
    """RoPE2D (oracle/must3r_ref.py rope2d, with its fp32 table) on rows t [R, heads * 64] with pos int64 [R, 2], on the device of t."""
    r = t.shape[0]
    cos, sin = R.rope_tables(int(pos.max()) + 1, rope[0], rope[1])
    cos, sin = cos.to(device=t.device, dtype=t.dtype), sin.to(device=t.device, dtype=t.dtype)
    th = t.reshape(r, heads, 2, 2, 16)                       # per head: (y | x) halves of the pairs (a, b) = (i, i + 16)
    c = torch.stack([cos[pos[:, 0]], cos[pos[:, 1]]], dim=1)[:, None]     # [R, 1, 2, 16]
    s = torch.stack([sin[pos[:, 0]], sin[pos[:, 1]]], dim=1)[:, None]
    a, b = th[:, :, :, 0], th[:, :, :, 1]
    return torch.stack([a * c - b * s, b * c + a * s], dim=3).reshape(r, heads * HEAD)


def attention_sublayer(x, pos, views, heads, p, rope=(100.0, 1.0), eps=1e-6):
    """x + proj(attn(rope(qkv(norm1 x)))) on rows x [R, D]; p: the six tensors of ATTN_PARAMS by name."""
    D = heads * HEAD
    y = R.layer_norm(x, p["norm1.weight"], p["norm1.bias"], eps)
    qkv = y @ p["attn.qkv.weight"].t() + p["attn.qkv.bias"]
    q, k, v = rope_rows(qkv[:, :D], pos, heads, rope), rope_rows(qkv[:, D:2 * D], pos, heads, rope), qkv[:, 2 * D:]
    o = AR.attention(q, k, v, views, heads)
    return x + o @ p["attn.proj.weight"].t() + p["attn.proj.bias"]


def mlp_sublayer(x, p, eps=1e-6):
    """x + fc2(gelu(fc1(norm2 x))); p: the six tensors of MLP_PARAMS by name."""
    y = R.layer_norm(x, p["norm2.weight"], p["norm2.bias"], eps)
    h = R.gelu(y @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"])
    return x + h @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"]


def block(x, pos, views, heads, p, rope=(100.0, 1.0), eps=1e-6):
    return mlp_sublayer(attention_sublayer(x, pos, views, heads, p, rope, eps), p, eps)


def grid_positions(n, width):
    """Row-major (y, x) positions of the first n cells of a grid `width` wide."""
    i = torch.arange(n)
    return torch.stack([i // width, i % width], dim=1)


def make_case(D, heads, hidden, tokens, seed, width=8):
    """x [sum(tokens), D], one self-attention view per entry of `tokens` on a grid `width` wide, the twelve parameters (weights of the scale a trained
    Linear has, norms around 1, biases around 0.1) and an upstream gradient of order 1e-7."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    M = sum(tokens)
    p = {"norm1.weight": 1 + 0.1 * rn(D), "norm1.bias": 0.1 * rn(D), "attn.qkv.weight": rn(3 * D, D) * D ** -0.5 * 1.5, "attn.qkv.bias": 0.1 * rn(3 * D),
         "attn.proj.weight": rn(D, D) * D ** -0.5, "attn.proj.bias": 0.1 * rn(D), "norm2.weight": 1 + 0.1 * rn(D), "norm2.bias": 0.1 * rn(D),
         "mlp.fc1.weight": rn(hidden, D) * D ** -0.5, "mlp.fc1.bias": 0.1 * rn(hidden), "mlp.fc2.weight": rn(D, hidden) * hidden ** -0.5,
         "mlp.fc2.bias": 0.1 * rn(D)}
    views, r0 = [], 0
    for n in tokens:
        views.append([r0, n, r0, n, 0, 0])
        r0 += n
    return dict(D=D, heads=heads, hidden=hidden, tokens=list(tokens), M=M, x=rn(M, D), dy=rn(M, D) * 1e-7, params=p, views=views,
                pos=torch.cat([grid_positions(n, width) for n in tokens]), rope=(100.0, 1.0), eps=1e-6)


def grads(case, dtype, which="block"):
    """dict out, dx and one entry per parameter of WHICH[which], under CPU autograd in ``dtype``."""
    x = case["x"].to(dtype).clone().requires_grad_(True)
    p = {k: case["params"][k].to(dtype).clone().requires_grad_(True) for k in WHICH[which]}
    if which == "attn":
        out = attention_sublayer(x, case["pos"], case["views"], case["heads"], p, case["rope"], case["eps"])
    elif which == "mlp":
        out = mlp_sublayer(x, p, case["eps"])
    else:
        out = block(x, case["pos"], case["views"], case["heads"], p, case["rope"], case["eps"])
    out.backward(case["dy"].to(dtype))
    res = dict(out=out.detach(), dx=x.grad)
    res.update({k: t.grad for k, t in p.items()})
    return res
