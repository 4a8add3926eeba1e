"""Yardstick of the prediction head tests: ``MUSt3R._compute_prediction_head`` restated in plain torch (decoder.py:149-156 ``norm_dec``,
blocks/head.py:63-72 ``proj`` + ``pixel_shuffle``, tools/image.py:9-14), run under CPU autograd in fp64 (truth) and in fp32 (the
reference's own precision) on the same fp32 inputs; plus the head activation of engine/inference.py:16-27 for the end-to-end chain.
Nothing here imports the code under test."""
import math

import torch
import torch.nn.functional as F

PATCH, CHANNELS = 16, 7
OUT = CHANNELS * PATCH * PATCH
NAMES = ("dx", "dgamma", "dbeta", "dW", "db")


def head(x, gamma, beta, W, b, n_views, H, Wd, eps=1e-6):
    """x [n_views * N, D] -> pointmaps [n_views, H, Wd, 7]"""
    D = x.shape[-1]
    gh, gw = H // PATCH, Wd // PATCH
    y = F.layer_norm(x, (D,), gamma, beta, eps)
    z = F.linear(y, W, b)
    z = z.view(n_views, gh, gw, OUT).permute(0, 3, 1, 2)
    return F.pixel_shuffle(z, PATCH).permute(0, 2, 3, 1)


def pixel_shuffle_loop(z, n_views, H, Wd):
    """The indexing of the header, one element at a time: pointmaps[v, 16 gy + i, 16 gx + j, c] = z[v N + gy gw + gx, c 256 + i 16 + j]."""
    gh, gw = H // PATCH, Wd // PATCH
    out = torch.empty((n_views, H, Wd, CHANNELS), dtype=z.dtype)
    for v in range(n_views):
        for gy in range(gh):
            for gx in range(gw):
                row = z[v * gh * gw + gy * gw + gx]
                for c in range(CHANNELS):
                    for i in range(PATCH):
                        for j in range(PATCH):
                            out[v, PATCH * gy + i, PATCH * gx + j, c] = row[c * PATCH * PATCH + i * PATCH + j]
    return out


def unshuffle(G):
    """dZ [n_views * N, 1792] of an upstream gradient G [n_views, H, Wd, 7]: the gather the backward performs."""
    n, H, Wd, _ = G.shape
    gh, gw = H // PATCH, Wd // PATCH
    return G.view(n, gh, PATCH, gw, PATCH, CHANNELS).permute(0, 1, 3, 5, 2, 4).reshape(n * gh * gw, OUT)


def make_case(n_views, H, Wd, D=768, seed=0, g_scale=1e-7):
    """Seeded fp32 inputs: rows of x with their own offset and scale (so that mu and rstd matter), gamma around 1 and beta around 0 with 0.2
    noise, xavier-uniform W, and an upstream gradient of the magnitude a mean-reduced loss hands down -- below fp16's range on purpose."""
    g = torch.Generator().manual_seed(1000 * seed + n_views * 7919 + H * 31 + Wd)
    R = n_views * (H // PATCH) * (Wd // PATCH)
    x = torch.randn((R, D), generator=g) * (0.5 + 2.0 * torch.rand((R, 1), generator=g)) + 3.0 * torch.randn((R, 1), generator=g)
    gamma = 1.0 + 0.2 * torch.randn((D,), generator=g)
    beta = 0.2 * torch.randn((D,), generator=g)
    a = math.sqrt(6.0 / (D + OUT))
    W = (torch.rand((OUT, D), generator=g) * 2 - 1) * a
    b = 0.1 * torch.randn((OUT,), generator=g)
    G = torch.randn((n_views, H, Wd, CHANNELS), generator=g) * g_scale
    return dict(x=x, gamma=gamma, beta=beta, W=W, b=b, G=G, n_views=n_views, H=H, Wd=Wd, D=D)


def forward(case, dtype):
    t = {k: case[k].to(dtype) for k in ("x", "gamma", "beta", "W", "b")}
    with torch.no_grad():
        return head(t["x"], t["gamma"], t["beta"], t["W"], t["b"], case["n_views"], case["H"], case["Wd"])


def grads(case, dtype, G=None):
    """(dx, dgamma, dbeta, dW, db) by autograd in ``dtype``, as a dict."""
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("x", "gamma", "beta", "W", "b")]
    out = head(*leaves, case["n_views"], case["H"], case["Wd"])
    out.backward((case["G"] if G is None else G).to(dtype))
    return {n: t.grad for n, t in zip(NAMES, leaves)}


def postprocess(raw):
    """engine/inference.py:16-27 with 'norm_exp': direction * expm1(norm) on channels 0:3 and 3:6, conf = 1 + exp(channel 6)."""
    def norm_exp(xyz):
        d = xyz.norm(dim=-1, keepdim=True)
        return xyz / d.clip(min=1e-8) * torch.expm1(d)
    return dict(pts3d=norm_exp(raw[..., 0:3]), pts3d_local=norm_exp(raw[..., 3:6]), conf=1.0 + raw[..., 6].exp())
