"""Yardstick of the mixed-orientation head tests: the reference's ``transpose_to_landscape(head, activate=True)`` (blocks/head.py:24-60, ``wrapper_yes``)
over ``norm_dec`` + ``LinearHead`` (decoder.py:149-156), restated in plain torch on top of tests/head_ref.py and run under CPU autograd in fp64 (truth)
and fp32 (the reference's own precision) on the same fp32 inputs.  The batch is stored landscape, ``[V, H, W, 7]`` with ``H <= W``; a portrait view has the
``true_shape`` row ``(W, H)``, its tokens are those of its own grid of ``W/16`` rows of ``H/16`` columns, and its result is ``head(tokens, (W, H))`` with
the two image axes swapped.  Nothing here imports the code under test."""
import torch

import head_ref as HR

NAMES = HR.NAMES


def true_shape(flags, H, Wd):
    """int64 [V, 2]: (H, W) rows, (W, H) where ``flags`` says portrait"""
    return torch.tensor([[Wd, H] if f else [H, Wd] for f in flags], dtype=torch.int64)


def head(x, gamma, beta, W, b, flags, H, Wd, eps=1e-6):
    """x [V * N, D], flags: a bool per view -> pointmaps [V, H, Wd, 7] in the stored layout.  View by view, which is what the reference's boolean gathers and
    index assignments come to: the head has no arithmetic across rows."""
    V = len(flags)
    N = (H // HR.PATCH) * (Wd // HR.PATCH)
    out = []
    for v, f in enumerate(flags):
        xv = x[v * N:(v + 1) * N]
        if f:
            out.append(HR.head(xv, gamma, beta, W, b, 1, Wd, H, eps).swapaxes(1, 2))
        else:
            out.append(HR.head(xv, gamma, beta, W, b, 1, H, Wd, eps))
    assert len(out) == V
    return torch.cat(out, dim=0)


def shuffle_loop(z, flags, H, Wd):
    """The indexing of the header, one element at a time: landscape S[v, 16 gy + i, 16 gx + j, c], portrait S[v, 16 px + j, 16 py + i, c] = z[v N + t, c 256 + 16 i + j]
    with t = gy gw + gx and t = py gh + px."""
    P = HR.PATCH
    gh, gw = H // P, Wd // P
    out = torch.empty((len(flags), H, Wd, HR.CHANNELS), dtype=z.dtype)
    for v, f in enumerate(flags):
        for t in range(gh * gw):
            row = z[v * gh * gw + t].view(HR.CHANNELS, P, P)
            if f:
                py, px = divmod(t, gh)
                out[v, P * px:P * px + P, P * py:P * py + P] = row.permute(2, 1, 0)      # [j, i, c]
            else:
                gy, gx = divmod(t, gw)
                out[v, P * gy:P * gy + P, P * gx:P * gx + P] = row.permute(1, 2, 0)      # [i, j, c]
    return out


def make_case(n_views, H, Wd, flags, D=64, seed=0, g_scale=1e-7):
    """tests/head_ref.py's seeded inputs plus the flags"""
    assert len(flags) == n_views and H <= Wd
    case = HR.make_case(n_views, H, Wd, D=D, seed=seed, g_scale=g_scale)
    case["flags"] = tuple(bool(f) for f in flags)
    return case


def forward(case, dtype):
    t = {k: case[k].to(dtype) for k in ("x", "gamma", "beta", "W", "b")}
    with torch.no_grad():
        return head(t["x"], t["gamma"], t["beta"], t["W"], t["b"], case["flags"], case["H"], case["Wd"])


def grads(case, dtype, G=None):
    """(dx, dgamma, dbeta, dW, db) by autograd in ``dtype``, as a dict."""
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("x", "gamma", "beta", "W", "b")]
    out = head(*leaves, case["flags"], case["H"], case["Wd"])
    out.backward((case["G"] if G is None else G).to(dtype))
    return {n: t.grad for n, t in zip(NAMES, leaves)}
