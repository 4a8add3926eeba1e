"""The prediction head's training forward and backward (csrc/train_head.hip ``must3r_hip_head_forward`` / ``must3r_hip_head_grad``;
must3r_amd.train_head) beside the reference's method (tests/head_ref.py: LayerNorm, Linear, pixel shuffle under torch autograd in fp32, on the
same GPU and the same tensors, in the same run).  One JSON line per size (append them to profiles/head_grad_bench.jsonl).
Sizes: one scene (20 views) and 28 scenes x 20 views of 384 x 512; D = 768.

  (a) the entry point on preallocated buffers, device events: the whole backward; the weight-gradient half alone (dW and db: statistics, split
      GEMM, reduce); the data-gradient half alone (dx, dgamma, dbeta: statistics, weight permutation, GEMM, LayerNorm backward); the forward.
  (b) per launch, from a kernel trace (``--kernel-stats FILE``: the kernel_stats CSV of a separate
      ``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_head_grad.py --kernels-only --views N`` run): average time, and
      for the two GEMMs the achieved TFLOP/s (2 R O D each) against the 157.3 TFLOP/s fp32 matrix peak, for the statistics pass (R D floats read)
      and the LayerNorm backward (3 R D floats: x and dY read, dx written) the GB/s against 6.3 TB/s.
  (c) wall clock of forward + backward through ``prediction_head`` beside the yardstick's, and the largest difference of their gradients.
The scratch of the backward is reported beside the size of the upstream gradient.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_ref as HR  # noqa: E402
from must3r_amd import _lib, train_head as TH  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S, FP32_MATRIX_FLOPS = 6.3e12, 157.3e12
H, W, D, O = 384, 512, 768, HR.OUT


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _events(fn, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _wall(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def make_inputs(n_views, seed=0):
    """seeded, generated on the device: the magnitudes of tests/head_ref.make_case"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    R = n_views * (H // 16) * (W // 16)
    x = torch.randn((R, D), generator=g, device=DEV) * (0.5 + 2.0 * torch.rand((R, 1), generator=g, device=DEV)) + 3.0 * torch.randn((R, 1), generator=g, device=DEV)
    gamma = 1.0 + 0.2 * torch.randn((D,), generator=g, device=DEV)
    beta = 0.2 * torch.randn((D,), generator=g, device=DEV)
    Wt = (torch.rand((O, D), generator=g, device=DEV) * 2 - 1) * (6.0 / (D + O)) ** 0.5
    b = 0.1 * torch.randn((O,), generator=g, device=DEV)
    G = torch.randn((n_views, H, W, 7), generator=g, device=DEV) * 1e-7
    return dict(x=x, gamma=gamma, beta=beta, W=Wt, b=b, G=G, n_views=n_views, R=R)


def grad_call(t, want, scratch, nbytes):
    """``must3r_hip_head_grad`` on preallocated buffers: nothing but the entry point inside the timed call."""
    lib = _lib.load()
    sizes = dict(dx=(t["R"], D), dgamma=(D,), dbeta=(D,), dW=(O, D), db=(O,))
    outs = {k: torch.empty(sizes[k], device=DEV) for k, w in zip(HR.NAMES, want) if w}
    a = _lib.HeadGradArgs()
    a.x, a.gamma, a.beta, a.W, a.G = (t[k].data_ptr() for k in ("x", "gamma", "beta", "W", "G"))
    a.n_views, a.H, a.Wimg, a.D, a.eps = t["n_views"], H, W, D, 1e-6
    for k, v in outs.items():
        setattr(a, k, v.data_ptr())
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))

    def call(_keep=(outs, a)):
        _lib.check(lib.must3r_hip_head_grad(C.byref(a), scratch.data_ptr(), nbytes, stream))
    return call


def bench_entry_points(t, args):
    lib = _lib.load()
    n = t["n_views"]
    nbytes = lib.must3r_hip_head_grad_scratch_bytes(n, H, W, D)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    gemm_flops = 2.0 * t["R"] * O * D
    out = dict(scratch_bytes=int(nbytes), upstream_gradient_bytes=int(t["G"].numel() * 4), gemm_flops_each=gemm_flops)
    for name, want, flops in (("backward_all", (True,) * 5, 2 * gemm_flops), ("backward_dW_db", (False, False, False, True, True), gemm_flops),
                              ("backward_dx_dgamma_dbeta", (True, True, True, False, False), gemm_flops)):
        st = _stats(_events(grad_call(t, want, scratch, nbytes), args), unit="ms")
        out[name] = dict(ms=st, tflops_of_the_whole_call=flops / (st["median"] * 1e-3) / 1e12,
                         fraction_of_157p3_TFLOPs_whole_call=flops / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
    fwd = lambda: TH.head_forward(t["x"], t["gamma"], t["beta"], t["W"], t["b"], n, H, W)
    out["forward"] = dict(ms=_stats(_events(fwd, args), unit="ms"))
    return out


KERNELS = {   # substring of the kernel symbol -> (figure, work per launch as a function of R)
    "dgrad_kernel": ("flops", lambda R: 2.0 * R * O * D),
    "wgrad_kernel": ("flops", lambda R: 2.0 * R * O * D),
    "row_stats_kernel": ("bytes", lambda R: 4.0 * R * D),
    "ln_grad_kernel": ("bytes", lambda R: 12.0 * R * D),
    "wgrad_reduce_kernel": ("bytes", lambda R: 4.0 * O * D * (TH.wgrad_splits(R) + 1)),
    "ln_grad_reduce_kernel": ("bytes", lambda R: 8.0 * D * min(1024, -(-R // 16))),
    "perm_w_kernel": ("bytes", lambda R: 8.0 * O * D),
}


def kernel_rows(path, R):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            for key, (kind, work) in KERNELS.items():
                if key in name and not (key == "wgrad_kernel" and "reduce" in name) and not (key == "ln_grad_kernel" and "reduce" in name):
                    avg_s = float(r["AverageNs"]) * 1e-9
                    row = dict(calls=int(r["Calls"]), avg_us=avg_s * 1e6, min_us=float(r["MinNs"]) * 1e-3, max_us=float(r["MaxNs"]) * 1e-3)
                    if kind == "flops":
                        row.update(tflops=work(R) / avg_s / 1e12, fraction_of_157p3_TFLOPs=work(R) / avg_s / FP32_MATRIX_FLOPS)
                    else:
                        row.update(GBps=work(R) / avg_s / 1e9, fraction_of_6p3_TBps=work(R) / avg_s / HBM_BYTES_PER_S)
                    rows[key] = row
    return rows


def bench_step(t, args):
    n = t["n_views"]
    keys = ("x", "gamma", "beta", "W", "b")
    leaves = [t[k].clone().requires_grad_(True) for k in keys]

    def step(fn):
        for v in leaves:
            v.grad = None
        fn(*leaves).backward(t["G"])
        return [v.grad for v in leaves]
    native = lambda x, g, b_, w, bias: TH.prediction_head(x.view(n, -1, D), (H, W), g, b_, w, bias)
    yard = lambda x, g, b_, w, bias: HR.head(x, g, b_, w, bias, n, H, W)
    g_n = [v.clone() for v in step(native)]
    g_y = step(yard)
    rec = dict(native_s=_stats(_wall(lambda: step(native), args.rounds, args.warmup), unit="s"),
               yardstick_torch_fp32_s=_stats(_wall(lambda: step(yard), args.yardstick_rounds, 1), unit="s"),
               max_abs_grad_difference={k: float((a - b).abs().max()) for k, a, b in zip(HR.NAMES, g_n, g_y)},
               max_abs_grad={k: float(b.abs().max()) for k, b in zip(HR.NAMES, g_y)})
    rec["speedup_median"] = rec["yardstick_torch_fp32_s"]["median"] / rec["native_s"]["median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[20, 28 * 20])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--yardstick-rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a --kernels-only run under rocprofv3 at the LAST of --views: figure (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_grad: needs a GPU (no CPU fallback)")
    f = open(args.out, "a") if args.out else None
    for n in args.views:
        t = make_inputs(n)
        rec = dict(figure="head_grad", views=n, H=H, W=W, D=D, rows=t["R"], wgrad_splits=TH.wgrad_splits(t["R"]), entry_points=bench_entry_points(t, args))
        if args.kernel_stats and n == args.views[-1]:
            rec["kernels"] = kernel_rows(args.kernel_stats, t["R"])
        if not args.kernels_only:
            rec["step"] = bench_step(t, args)
        line = json.dumps(rec)
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
        del t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
