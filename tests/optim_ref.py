"""Yardstick of the optimizer step (must3r_amd/train_optim.py, csrc/train_optim.hip), on the CPU:

* ``yardstick_step``: fp64 ``torch.optim.AdamW(foreach=False)`` behind ``torch.nn.utils.clip_grad_norm_`` and the unscale, the non-finite test and the update
  rule of ``torch.amp.GradScaler`` -- what the reference's training loop runs, in twice the precision;
* ``emulate32``: the kernel's documented operation sequence (include/must3r_hip.h) in fp32, every operation rounded, and five planted defects of it;
* ``bound_ratio``: the error bound of the step, see its docstring for the count of roundings behind ``K``.

Nothing here imports must3r_amd."""
import math

import numpy as np
import torch

U = 2.0 ** -24
K = 28
DEFECTS = ("no_bias_correction", "l2_decay", "eps_in_sqrt", "no_clip", "coef_once_in_v")


def scaler_update(scale, tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """``GradScaler.update()``: (scale, tracker) after a step"""
    if found_inf:
        return scale * backoff_factor, 0
    tracker += 1
    if tracker == growth_interval:
        return scale * growth_factor, 0
    return scale, tracker


def yardstick_step(tensors, grads, groups, scale=None, max_norm=None):
    """One step in fp64.  ``tensors``: dicts ``p, m, v`` (fp32 CPU tensors), ``step`` (number), ``group`` (index); ``grads``: fp32 tensors as backward wrote
    them (scaled), ``None`` for a parameter without one; ``groups``: dicts ``lr, weight_decay, betas, eps``.  Returns per tensor ``p, m, v`` (fp64), ``step``
    and the bound's pieces ``p0, m0, g1`` (the unscaled, clipped gradient), ``denom, lr, bc1, beta1``; and ``norm`` (fp64, before the clip), ``found_inf``."""
    inv = 1.0 if scale is None else 1.0 / float(scale)
    live = [i for i, g in enumerate(grads) if g is not None]
    params = [torch.nn.Parameter(t["p"].double().clone()) for t in tensors]
    for i in live:
        params[i].grad = grads[i].double() * inv
    total = sum(float((params[i].grad ** 2).sum()) for i in live)
    found_inf = not math.isfinite(total)
    norm = math.sqrt(total) if not found_inf else float("nan")
    out = [dict(p=t["p"].double().clone(), m=t["m"].double().clone(), v=t["v"].double().clone(), step=float(t["step"])) for t in tensors]
    if found_inf:
        return out, norm, True
    if max_norm is not None and max_norm > 0:
        got = torch.nn.utils.clip_grad_norm_([params[i] for i in live], float(max_norm))
        assert abs(float(got) - norm) <= 1e-12 * norm
    pgs = []
    for k, g in enumerate(groups):
        pgs.append(dict(params=[params[i] for i, t in enumerate(tensors) if t["group"] == k], lr=g["lr"], weight_decay=g["weight_decay"],
                        betas=tuple(g["betas"]), eps=g["eps"]))
    opt = torch.optim.AdamW([pg for pg in pgs if pg["params"]], foreach=False)
    for i in live:
        t = tensors[i]
        opt.state[params[i]] = dict(step=torch.tensor(float(t["step"])), exp_avg=t["m"].double().clone(), exp_avg_sq=t["v"].double().clone())
    opt.step()
    for i in live:
        t, g = tensors[i], groups[tensors[i]["group"]]
        st = opt.state[params[i]]
        n = float(t["step"]) + 1
        bc1, bc2 = 1 - g["betas"][0] ** n, 1 - g["betas"][1] ** n
        out[i] = dict(p=params[i].detach().clone(), m=st["exp_avg"], v=st["exp_avg_sq"], step=float(st["step"]),
                      p0=t["p"].double(), m0=t["m"].double(), g1=params[i].grad.clone(), denom=st["exp_avg_sq"].sqrt() / math.sqrt(bc2) + g["eps"],
                      lr=g["lr"], bc1=bc1, beta1=g["betas"][0])
    return out, norm, False


def coef32(total, scale=None, max_norm=None):
    """the control record as optim_norm computes it from the fp64 sum of squares: (norm, coef, inv_scale, clip), fp32"""
    f = np.float32
    inv_scale = f(1.0) / f(scale) if scale is not None else f(1.0)
    norm = f(math.sqrt(total) * float(inv_scale))
    clip = f(1.0)
    if max_norm is not None and max_norm > 0:
        clip = min(f(1.0), f(max_norm) / (norm + f(1e-6)))
    return norm, f(inv_scale * clip), inv_scale, clip


def emulate32(p, g, m, v, step, group, inv_scale=1.0, clip=1.0, defect=None):
    """the step kernel's sequence on numpy fp32 arrays: (p, m, v) after the step.  ``defect``: one of DEFECTS"""
    f = np.float32
    lr, wd, (b1, b2), eps = group["lr"], group["weight_decay"], group["betas"], group["eps"]
    n = float(step) + 1
    bc1, bc2 = 1 - b1 ** n, 1 - b2 ** n
    if defect == "no_bias_correction":
        bc1 = bc2 = 1.0
    step_size, sbc2 = f(lr / bc1), f(math.sqrt(bc2))
    coef = f(inv_scale) if defect == "no_clip" else f(f(inv_scale) * f(clip))
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    gs = g * coef
    if defect == "l2_decay":
        gs = gs + f(wd) * p
    else:
        p = p * f(1.0 - lr * wd)
    m = f(b1) * m + f(1.0 - b1) * gs
    v = f(b2) * v + (f(1.0 - b2) * (g if defect == "coef_once_in_v" else gs)) * gs
    if defect == "eps_in_sqrt":
        denom = np.sqrt(v / (sbc2 * sbc2) + f(eps))
    else:
        denom = np.sqrt(v) / sbc2 + f(eps)
    p = p - step_size * (m / denom)
    return p, m, v


def bound_ratio(y, p, m, v, k=K):
    """The largest of |error| / bound over the elements of one tensor and over p, m and v; ``y``: the tensor's entry of ``yardstick_step``.  With u = 2^-24,
    M = |b1 m0| + |(1 - b1) g'| and U = (lr / bc1) M / denom, all from the fp64 yardstick:

        |p - p64| <= k u (|p0| + U)          |m - m64| <= k u M          |v - v64| <= k u v64

    The count of roundings behind k (each at most u relative, first order; a fused multiply-add only removes some):
      coef     6   1 / scale, the norm's store, norm + 1e-6, max_norm as fp32, the division, inv_scale * clip
      g'       7   coef, the product
      m       10   on M: the g' term carries 7 + (1 - b1 as fp32) + its product = 9, the m0 term b1 as fp32 + its product = 2; the sum 1
      v       18   the g' g' term 7 + 7 + (1 - b2 as fp32) + two products = 17, the v0 term 2; the sum 1 (all terms are >= 0: relative)
      denom   13   sqrt halves v's 18 to 9, + its own 1, sqrt(bc2) as fp32 1, the division 1 = 12 on that term; eps as fp32 1; the sum 1
      m/denom 24   10 (m, on M) + 13 (denom) + the division 1
      update  26   lr / bc1 as fp32 1, the product 1:  26 u U
      p       27   p0 (1 - lr wd): the constant 1 + the product 1 = 2 u |p0|; the last subtraction u (|p0| + U):  3 u |p0| + 27 u U
    K = 28: the 27 of p and one unit for what the count leaves out (second-order terms, the last bit of pow on either side, 1e-6 as fp32)."""
    p, m, v = (torch.as_tensor(np.asarray(x)).double().reshape(y["p"].shape) for x in (p, m, v))
    M = (y["beta1"] * y["m0"]).abs() + ((1 - y["beta1"]) * y["g1"]).abs()
    bp = k * U * (y["p0"].abs() + (y["lr"] / y["bc1"]) * M / y["denom"])
    bm = k * U * M
    bv = k * U * y["v"]
    worst = 0.0
    for err, b in (((p - y["p"]).abs(), bp), ((m - y["m"]).abs(), bm), ((v - y["v"]).abs(), bv)):
        bad = err > 0
        if bool(bad.any()):
            worst = max(worst, float((err[bad] / b[bad]).max()))
    return worst


def rounded(y):
    """the yardstick's state after a step, rounded to the fp32 the next step starts from"""
    return dict(p=y["p"].float(), m=y["m"].float(), v=y["v"].float(), step=y["step"])
