"""The attention core's training forward and backward (csrc/train_attention.hip ``must3r_hip_attn_forward_f32`` / ``must3r_hip_attn_grad``;
must3r_amd.train_attention) beside the yardstick's formulas in fp32 under torch autograd, on the same GPU and the same tensors, in the same run.
One JSON line per shape (append them to profiles/attn_grad_bench.jsonl).  Shapes, the decoder's own (12 heads of 64):

  self   28 x 20 views of 768 tokens, each over its own tokens (``self_views``)
  cross  one schedule step of 28 scenes in the render form: one view of 768 tokens per scene over its scene's memory of 20 x 768 rows (nk = Nm)

  (a) the entry points on preallocated buffers, device events: the forward; the backward asked for dQ alone (statistics launch + dq), for dK and dV
      alone (statistics launch + dkv) and for all three.
  (b) per launch, from a kernel trace (``--kernel-stats FILE``: the kernel_stats CSV of a separate
      ``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_attn_grad.py --kernels-only --shapes S`` run): average time and
      the achieved TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak.  Flops per (view, head): forward 4 nq nk_valid 64 (two products), dkv twice
      that (four products), dq one and a half times (three).
  (c) forward + backward through ``attention`` under autograd beside torch's: ``F.scaled_dot_product_attention`` on the batched views (these shapes
      have no excluded keys, so no mask is needed) and the yardstick's per-view loop (tests/attn_grad_ref.py), both fp32, and the largest
      difference of the gradients.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
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
import attn_grad_ref as AR  # noqa: E402
from must3r_amd import _lib, train_attention as TA  # noqa: E402

DEV = "cuda:0"
FP32_MATRIX_FLOPS = 157.3e12
HEADS, D, N, V, S = 12, 768, 768, 20, 28


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


def make_inputs(shape, scenes, seed=0):
    """seeded, generated on the device: the magnitudes of tests/attn_grad_ref.make_case"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if shape == "self":
        views, Rq, Rk = TA.self_views(scenes, V, N), scenes * V * N, scenes * V * N
        batch = (scenes * V, N, N)
    else:
        views, Rq, Rk = TA.memory_views(scenes, 1, N, V * N), scenes * N, scenes * (V * N + N)   # a scene's key rows: its memory, then the view's own tokens (not read)
        batch = (scenes, N, V * N)
    q = torch.randn((Rq, D), generator=g, device=DEV) * 2
    k, v = torch.randn((Rk, D), generator=g, device=DEV), torch.randn((Rk, D), generator=g, device=DEV)
    dO = torch.randn((Rq, D), generator=g, device=DEV) * 1e-7
    pair_flops = sum(4.0 * w[1] * (w[3] - (w[5] - w[4])) * 64 for w in views) * HEADS
    return dict(shape=shape, q=q, k=k, v=v, dO=dO, views=views, tab=torch.tensor(views, dtype=torch.int32), batch=batch, forward_flops=pair_flops)


def entry_calls(t):
    """name -> (call on preallocated buffers with nothing but the entry point inside, flops of the call)"""
    lib = _lib.load()
    scratch, nbytes = TA._scratch(t["tab"], HEADS, t["q"].device)
    outs = dict(O=torch.empty_like(t["q"]), dQ=torch.empty_like(t["q"]), dK=torch.empty_like(t["k"]), dV=torch.empty_like(t["v"]))
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    F = t["forward_flops"]

    def make(fn, names):
        a = TA._args(t["q"], t["k"], t["v"], t["tab"], HEADS)
        a.dO, a.lddo, a.ldo, a.lddq, a.lddk, a.lddv = t["dO"].data_ptr(), D, D, D, D, D
        for n in names:
            setattr(a, n, outs[n].data_ptr())

        def call(_keep=(a, outs, scratch)):
            _lib.check(fn(C.byref(a), scratch.data_ptr(), nbytes, stream))
        return call
    return dict(forward=(make(lib.must3r_hip_attn_forward_f32, ("O",)), F),
                backward_dQ=(make(lib.must3r_hip_attn_grad, ("dQ",)), F + 1.5 * F),
                backward_dK_dV=(make(lib.must3r_hip_attn_grad, ("dK", "dV")), F + 2 * F),
                backward_all=(make(lib.must3r_hip_attn_grad, ("dQ", "dK", "dV")), F + 1.5 * F + 2 * F)), int(nbytes)


def bench_entry_points(t, args):
    calls, nbytes = entry_calls(t)
    out = dict(scratch_bytes=nbytes, forward_flops=t["forward_flops"])
    for name, (call, flops) in calls.items():
        st = _stats(_events(call, args), unit="ms")
        out[name] = dict(ms=st, flops=flops, tflops_of_the_whole_call=flops / (st["median"] * 1e-3) / 1e12,
                         fraction_of_157p3_TFLOPs_whole_call=flops / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
    return out


KERNELS = {"attn_fwd_f32": 1.0, "attn_dkv_f32": 2.0, "attn_dq_f32": 1.5}   # kernel symbol -> flops as a multiple of the forward's


def kernel_rows(path, forward_flops):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, mult in KERNELS.items():
                if key in r["Name"]:
                    avg_s = float(r["AverageNs"]) * 1e-9
                    rows[key] = dict(calls=int(r["Calls"]), avg_ms=avg_s * 1e3, min_ms=float(r["MinNs"]) * 1e-6, max_ms=float(r["MaxNs"]) * 1e-6,
                                     flops=mult * forward_flops, tflops=mult * forward_flops / avg_s / 1e12,
                                     fraction_of_157p3_TFLOPs=mult * forward_flops / avg_s / FP32_MATRIX_FLOPS)
    return rows


def bench_step(t, args):
    leaves = [t[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
    B, nq, nk = t["batch"]

    def step(fn):
        for x in leaves:
            x.grad = None
        fn(*leaves).backward(t["dO"])
        return [x.grad for x in leaves]

    def sdpa(q, k, v):
        split = lambda x, n: x.view(B, -1, HEADS, 64)[:, :n].transpose(1, 2)
        return torch.nn.functional.scaled_dot_product_attention(split(q, nq), split(k, nk), split(v, nk)).transpose(1, 2).reshape(B * nq, D)
    native = lambda q, k, v: TA.attention(q, k, v, t["tab"], HEADS)
    loop = lambda q, k, v: AR.attention(q, k, v, t["views"], HEADS)
    g_n = [x.clone() for x in step(native)]
    rec = dict(native_s=_stats(_wall(lambda: step(native), args.rounds, args.warmup), unit="s"))
    for name, fn in (("torch_sdpa_fp32_s", sdpa), ("torch_per_view_loop_fp32_s", loop)):
        try:
            g_t = step(fn)
            rec["max_abs_grad_difference_" + name[:-2]] = {n: float((a - b).abs().max()) for n, a, b in zip(("dQ", "dK", "dV"), g_n, g_t)}
            rec["max_abs_grad"] = {n: float(b.abs().max()) for n, b in zip(("dQ", "dK", "dV"), g_t)}
            del g_t
            rec[name] = _stats(_wall(lambda: step(fn), args.torch_rounds, 1), unit="s")
        except RuntimeError as e:                     # e.g. out of memory in the score matrices: said, not hidden
            rec[name] = dict(failed=str(e)[:200])
        torch.cuda.empty_cache()
    best = min((rec[n]["median"] for n in ("torch_sdpa_fp32_s", "torch_per_view_loop_fp32_s") if "median" in rec[n]), default=None)
    if best is not None:
        rec["speedup_median_over_the_faster_torch_form"] = best / rec["native_s"]["median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["self", "cross"], choices=["self", "cross"])
    ap.add_argument("--scenes", type=int, default=S)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="SHAPE=kernel_stats.csv of a --kernels-only run of that shape under rocprofv3: figure (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_grad: needs a GPU (no CPU fallback)")
    stats = dict(s.split("=", 1) for s in args.kernel_stats)
    f = open(args.out, "a") if args.out else None
    for shape in args.shapes:
        t = make_inputs(shape, args.scenes)
        rec = dict(figure="attn_grad", shape=shape, scenes=args.scenes, heads=HEADS, views=len(t["views"]), nq=t["views"][0][1], nk=t["views"][0][3],
                   q_rows=int(t["q"].shape[0]), kv_rows=int(t["k"].shape[0]), key_groups=TA.n_groups(t["tab"]),
                   conditions="clocks not pinned, shared machine; device events around the C entry points on preallocated buffers, medians",
                   entry_points=bench_entry_points(t, args))
        if shape in stats:
            rec["kernels"] = kernel_rows(stats[shape], t["forward_flops"])
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
