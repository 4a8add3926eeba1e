"""The prediction head over a batch stored landscape with portrait views (csrc/train_head.hip ``must3r_hip_head_forward_many_ar`` /
``must3r_hip_head_grad_many_ar``; must3r_amd.train_head) beside the existing landscape-only head and beside the reference's method, on the same tensors in
the same run.  One JSON line per size (append them to profiles/head_many_ar_bench.jsonl).  Sizes: one scene (20 views) and 28 scenes x 20 views of 384 x 512;
D = 768.  Device events around the call (output and scratch allocation included: the caching allocator's), the forms of a figure alternated inside every
round, ``warmup`` rounds first: median, min and max.

  (a) forward and backward with all-zero flags against the existing entry points (and, with ``--parent-lib``, against the same entry points of a library built
      from the parent commit, loaded beside this one); the bits are compared.
  (b) every second view flagged, against (a): the cost of the orientation passes in ms and the bytes they move -- forward 4 x, backward 2 x the flagged views'
      pointmaps (turn: read + write; copy back: read + write) -- as a share of 6.3 TB/s.  No counters are taken.
  (c) the mixed batch the reference's way under autograd over the existing head: two head calls on boolean-gathered rows, index-assign into the result
      (blocks/head.py:36-58), forward + backward, beside ``prediction_head(..., transposed=flags)``.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_ref as HR  # noqa: E402
from must3r_amd import _lib, train_head as TH  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
H, W, D, O = 384, 512, 768, HR.OUT
N = (H // 16) * (W // 16)


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def alternate(forms, args):
    """forms: name -> callable.  Every round runs each form once, in turn, between device events."""
    ms = {k: [] for k in forms}
    for r in range(args.warmup + args.rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            if r >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    return {k: _stats(v, unit="ms") for k, v in ms.items()}


def make_inputs(n_views, seed=0):
    """seeded, generated on the device: the magnitudes of tests/head_ref.make_case"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    R = n_views * N
    x = torch.randn((R, D), generator=g, device=DEV) * (0.5 + 2.0 * torch.rand((R, 1), generator=g, device=DEV)) + 3.0 * torch.randn((R, 1), generator=g, device=DEV)
    gamma = 1.0 + 0.2 * torch.randn((D,), generator=g, device=DEV)
    beta = 0.2 * torch.randn((D,), generator=g, device=DEV)
    Wt = (torch.rand((O, D), generator=g, device=DEV) * 2 - 1) * (6.0 / (D + O)) ** 0.5
    b = 0.1 * torch.randn((O,), generator=g, device=DEV)
    G = torch.randn((n_views, H, W, 7), generator=g, device=DEV) * 1e-7
    return dict(x=x, gamma=gamma, beta=beta, W=Wt, b=b, G=G, n_views=n_views, R=R)


class ParentLib:
    """the existing entry points of a second library (built from the parent commit), called with this library's prototypes"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("must3r_hip_head_forward_scratch_bytes", "must3r_hip_head_forward", "must3r_hip_head_grad_scratch_bytes", "must3r_hip_head_grad"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.PROTOTYPES[name]

    def forward(self, t):
        n = t["n_views"]
        out = torch.empty((n, H, W, 7), device=DEV)
        nb = self.lib.must3r_hip_head_forward_scratch_bytes(n, H, W, D)
        scratch = torch.empty((nb,), dtype=torch.uint8, device=DEV)
        p = lambda k: C.c_void_p(t[k].data_ptr())
        rc = self.lib.must3r_hip_head_forward(_lib.F16, p("x"), p("gamma"), p("beta"), p("W"), p("b"), n, H, W, D, 1e-6, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV))))
        assert rc == 0
        return out

    def grad(self, t):
        n = t["n_views"]
        outs = [torch.empty(s, device=DEV) for s in ((t["R"], D), (D,), (D,), (O, D), (O,))]
        a = _lib.HeadGradArgs()
        a.x, a.gamma, a.beta, a.W, a.G = (t[k].data_ptr() for k in ("x", "gamma", "beta", "W", "G"))
        a.n_views, a.H, a.Wimg, a.D, a.eps = n, H, W, D, 1e-6
        a.dx, a.dgamma, a.dbeta, a.dW, a.db = (o.data_ptr() for o in outs)
        nb = self.lib.must3r_hip_head_grad_scratch_bytes(n, H, W, D)
        scratch = torch.empty((nb,), dtype=torch.uint8, device=DEV)
        rc = self.lib.must3r_hip_head_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV))))
        assert rc == 0
        return outs


def reference_way(leaves, flags_bool, n):
    """wrapper_yes over the existing head: boolean gathers, two calls, index-assign"""
    x, g, b_, w, bias = leaves
    xv = x.view(n, N, D)
    land, port = ~flags_bool, flags_bool
    l_res = TH.prediction_head(xv[land], (H, W), g, b_, w, bias)
    p_res = TH.prediction_head(xv[port], (W, H), g, b_, w, bias).swapaxes(1, 2)
    out = l_res.new_empty((n, *l_res.shape[1:]))
    out[land] = l_res
    out[port] = p_res
    return out


def bench(n, args, parent):
    t = make_inputs(n)
    a = (t["x"], t["gamma"], t["beta"], t["W"], t["b"])
    zeros = torch.zeros(n, dtype=torch.int32, device=DEV)
    half = (torch.arange(n, device=DEV) % 2).to(torch.int32)
    flagged = int(half.sum())
    view_bytes = H * W * 7 * 4
    rec = dict(figure="head_many_ar", views=n, flagged_views=flagged, H=H, W=W, D=D, rows=t["R"], pointmap_bytes=n * view_bytes)
    # bits
    f0, fz, fh = TH.head_forward(*a, n, H, W), TH.head_forward(*a, n, H, W, transposed=zeros), TH.head_forward(*a, n, H, W, transposed=half)
    g0, gz = TH.head_grad(*a[:4], t["G"], n, H, W), TH.head_grad(*a[:4], t["G"], n, H, W, transposed=zeros)
    rec["bits"] = dict(forward_zero_flags_equal_existing=bool(torch.equal(f0, fz)), backward_zero_flags_equal_existing=all(torch.equal(p, q) for p, q in zip(g0, gz)),
                       forward_unflagged_views_equal_existing=bool(torch.equal(f0[0::2], fh[0::2])))
    if parent:
        rec["bits"]["forward_equal_parent_build"] = bool(torch.equal(parent.forward(t), f0))
        rec["bits"]["backward_equal_parent_build"] = all(torch.equal(p, q) for p, q in zip(parent.grad(t), g0))
    del f0, fz, fh, g0, gz
    fwd = {"existing": lambda: TH.head_forward(*a, n, H, W), "zero_flags": lambda: TH.head_forward(*a, n, H, W, transposed=zeros),
           "half_flagged": lambda: TH.head_forward(*a, n, H, W, transposed=half)}
    bwd = {"existing": lambda: TH.head_grad(*a[:4], t["G"], n, H, W), "zero_flags": lambda: TH.head_grad(*a[:4], t["G"], n, H, W, transposed=zeros),
           "half_flagged": lambda: TH.head_grad(*a[:4], t["G"], n, H, W, transposed=half)}
    if parent:
        fwd["parent_build"] = lambda: parent.forward(t)
        bwd["parent_build"] = lambda: parent.grad(t)
    rec["forward_ms"], rec["backward_ms"] = alternate(fwd, args), alternate(bwd, args)
    for name, mult in (("forward", 4), ("backward", 2)):
        ms = rec[f"{name}_ms"]
        extra = ms["half_flagged"]["median"] - ms["zero_flags"]["median"]
        moved = mult * flagged * view_bytes
        rec[f"{name}_orientation_passes"] = dict(extra_ms=extra, bytes_moved=moved, share_of_6p3_TBps=(moved / (extra * 1e-3) / HBM_BYTES_PER_S) if extra > 0 else None)
    # (c) forward + backward under autograd
    leaves = [v.clone().requires_grad_(True) for v in a]
    flags_bool = half.bool()

    def step(fn):
        for v in leaves:
            v.grad = None
        fn().backward(t["G"])
        return [v.grad for v in leaves]
    native = lambda: TH.prediction_head(leaves[0].view(n, N, D), (H, W), *leaves[1:], transposed=half)
    ref = lambda: reference_way(leaves, flags_bool, n)
    plain = lambda: TH.prediction_head(leaves[0].view(n, N, D), (H, W), *leaves[1:])
    g_n = [v.clone() for v in step(native)]
    g_r = step(ref)
    rec["step_ms"] = alternate({"landscape_only_all_landscape": lambda: step(plain), "mixed_native": lambda: step(native), "mixed_reference_way": lambda: step(ref)}, args)
    rec["step_max_abs_grad_difference_native_vs_reference_way"] = {k: float((p - q).abs().max()) for k, p, q in zip(HR.NAMES, g_n, g_r)}
    rec["step_dx_bits_equal_reference_way"] = bool(torch.equal(g_n[0], g_r[0]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[20, 28 * 20])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default=None, help="libmust3r_hip.so built from the parent commit: its existing head entry points are timed and compared too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_many_ar: needs a GPU (no CPU fallback)")
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    f = open(args.out, "a") if args.out else None
    for n in args.views:
        line = json.dumps(bench(n, args, parent))
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
