"""Yardstick of the trainable encoder (must3r_amd/train_encoder.py, csrc/train_encoder.hip): the reference's Dust3rEncoder (must3r/model/encoder.py:13-52)
with dust3r's PatchEmbedDust3R or ManyAR_PatchEmbed in plain torch, generic in dtype, over flattened rows: the patch rows by reshape / permute (a portrait view
of a batch stored landscape is swapped first), rows @ W.view(E, 768).T + b, tests/block_ref.py's block per layer on one self-attention view per image, and the
oracle's layer_norm.  Runs under CPU autograd in fp64 (truth) and in fp32 (the reference's own precision).  Also the seeded case maker of
tests/test_encoder_grad_host.py and tests/test_encoder_grad_gpu.py."""
import torch

import block_ref as BR
from oracle import must3r_ref as R

PATCH = 16
COLS = 3 * PATCH * PATCH


def portrait_flags(true_shape, many_ar):
    """bool [V]: the views ManyAR_PatchEmbed transposes (h > w); none without it"""
    ts = torch.as_tensor(true_shape)
    return (ts[:, 0] > ts[:, 1]) if many_ar else torch.zeros(ts.shape[0], dtype=torch.bool)


def view_rows(im):
    """One image [3, H, W] -> (rows [N, 768] in the column order of the flattened conv weight, k = c 256 + dy 16 + dx; positions int64 [N, 2] of the row-major
    H/16 x W/16 grid)"""
    h, w = im.shape[1] // PATCH, im.shape[2] // PATCH
    rows = im.reshape(3, h, PATCH, w, PATCH).permute(1, 3, 0, 2, 4).reshape(h * w, COLS)
    return rows, torch.cartesian_prod(torch.arange(h, device=im.device), torch.arange(w, device=im.device)).view(h * w, 2)


def patch_rows(img, flags=None):
    """img [V, 3, H, W] -> rows [V N, 768], pos int64 [V N, 2]; flags bool [V]: the views that are swapped before the gather"""
    out = [view_rows(im.swapaxes(-1, -2) if flags is not None and bool(flags[v]) else im) for v, im in enumerate(img)]
    return torch.cat([r for r, _ in out]), torch.cat([p for _, p in out])


def param_names(depth):
    """the reference's state-dict order"""
    return (("patch_embed.proj.weight", "patch_embed.proj.bias") + tuple(f"blocks_enc.{i}.{k}" for i in range(depth) for k in BR.PARAMS)
            + ("norm_enc.weight", "norm_enc.bias"))


def encoder(img, flags, p, heads, depth, rope=(100.0, 1.0), eps=1e-6):
    """-> (x [V N, E], pos [V N, 2]); p: the tensors of param_names(depth) by name, patch_embed.proj.weight in the conv shape"""
    rows, pos = patch_rows(img, flags)
    w = p["patch_embed.proj.weight"]
    x = rows @ w.reshape(w.shape[0], COLS).t() + p["patch_embed.proj.bias"]
    V, n = img.shape[0], rows.shape[0] // img.shape[0]
    views = [[v * n, n, v * n, n, 0, 0] for v in range(V)]
    for i in range(depth):
        x = BR.block(x, pos, views, heads, {k: p[f"blocks_enc.{i}.{k}"] for k in BR.PARAMS}, rope, eps)
    return R.layer_norm(x, p["norm_enc.weight"], p["norm_enc.bias"], eps), pos


def make_case(D, heads, hidden, depth, V, H, W, true_shape=None, many_ar=False, seed=81):
    """V images of H x W in [-1, 1], the parameters in the scale of block_ref.make_case (the patch weight randn * 768 ** -0.5, norms around 1, biases
    around 0.1) and an upstream gradient of order 1e-7 on x.  true_shape: (h, w) per view, (H, W) for every view by default."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    img = torch.rand((V, 3, H, W), generator=g) * 2 - 1
    p = {"patch_embed.proj.weight": rn(D, 3, PATCH, PATCH) * COLS ** -0.5, "patch_embed.proj.bias": 0.1 * rn(D)}
    for i in range(depth):
        p.update({f"blocks_enc.{i}.{k}": v for k, v in BR.make_case(D, heads, hidden, [1], seed + 1 + i)["params"].items()})
    p.update({"norm_enc.weight": 1 + 0.1 * rn(D), "norm_enc.bias": 0.1 * rn(D)})
    assert tuple(p) == param_names(depth)
    n = (H // PATCH) * (W // PATCH)
    ts = torch.tensor(true_shape if true_shape is not None else [(H, W)] * V, dtype=torch.int64)
    return dict(D=D, heads=heads, hidden=hidden, depth=depth, V=V, H=H, W=W, n=n, img=img, true_shape=ts, many_ar=many_ar, params=p, dy=rn(V * n, D) * 1e-7,
                rope=(100.0, 1.0), eps=1e-6)


def grads(case, dtype):
    """dict x [V N, E] and one entry per parameter under CPU autograd in ``dtype``, and the positions"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case["params"].items()}
    x, pos = encoder(case["img"].to(dtype), portrait_flags(case["true_shape"], case["many_ar"]), p, case["heads"], case["depth"], case["rope"], case["eps"])
    x.backward(case["dy"].to(dtype))
    res = dict(x=x.detach())
    res.update({k: t.grad for k, t in p.items()})
    return res, pos
