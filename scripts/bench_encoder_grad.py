"""The trainable encoder (csrc/train_encoder.hip; must3r_amd.train_encoder) beside the yardstick's formulas (tests/encoder_ref.py) under torch autograd, on
the same GPU and the same tensors, in the same run.  One JSON line per run (append it to profiles/encoder_grad_bench.jsonl).  The shape: ``--views`` views
(20) stored ``--height`` x ``--width`` (384 x 512: 768 tokens), the released encoder geometry (D 1024, 16 heads, hidden 4096, ``--depth`` 24 layers).

  (a) ``patch_rows_f32`` through its C entry point on preallocated buffers, all views landscape and all views portrait: ``--launches`` launches between two
      device events, per launch, and the bytes it has to move (the image once in, the rows once out, the positions) against the 6.3 TB/s the project uses
      for a float4 copy.  47 MB of image fit the chip's last-level cache: the figure is a rate of the launch, not of the HBM.
  (b) the patch embedding, ``patch_embed`` forward (no graph) and forward + backward (weight and bias gradients), host clock around a synchronise.
  (c) ``Dust3rEncoder`` forward + backward (every parameter gradient) and the peak of allocated memory above what is resident before the step (the weights
      and the inputs: the last step's gradients are dropped first), with ``precision="fp32"`` and ``"bf16"``.
  (d) the same for tests/encoder_ref.py's encoder under torch autograd in fp32, and under ``torch.autocast("cuda", bfloat16)``; and the largest relative
      difference of the fp32 gradients (max |a - b| / max |b| per tensor).

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
"""
import argparse
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
import encoder_ref as ER  # noqa: E402
from must3r_amd import _lib, train_encoder as TE  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


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


def _wall_and_peak(fn, rounds, warmup, clear):
    """(seconds per round, the largest peak of allocated bytes above what was allocated before the round); ``clear`` drops the last round's gradients first,
    so that what is resident before a round is the weights and the inputs"""
    for _ in range(warmup):
        fn()
    out, peak = [], 0
    for _ in range(rounds):
        clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return out, int(peak)


def bench_gather(img, args):
    """(a): per launch, device events around ``--launches`` launches"""
    lib = _lib.load()
    V, _, H, W = img.shape
    R = V * (H // 16) * (W // 16)
    rows = torch.empty((R, 768), dtype=torch.float32, device=DEV)
    pos = torch.empty((R, 2), dtype=torch.int64, device=DEV)
    nbytes = 2.0 * img.numel() * 4 + R * 16
    out = dict(bytes=nbytes, launches_per_round=args.launches)
    for name, flag in (("landscape", 0), ("portrait", 1)):
        flags = torch.full((V,), flag, dtype=torch.int32, device=DEV)
        a = _lib.PatchRowsArgs()
        a.img, a.transposed, a.rows, a.pos = img.data_ptr(), flags.data_ptr(), rows.data_ptr(), pos.data_ptr()
        a.V, a.H, a.W = V, H, W
        a.stream = _lib.stream_ptr(torch.device(DEV))
        call = lambda: _lib.check(lib.must3r_hip_patch_rows(C.byref(a)))
        for _ in range(args.warmup * args.launches):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.launches)
        st = _stats(us, unit="us per launch")
        out[name] = dict(us=st, fraction_of_6p3_TBps=nbytes / (st["median"] * 1e-6) / HBM_BYTES_PER_S,
                         fraction_of_6p3_TBps_min_max=[nbytes / (st["max"] * 1e-6) / HBM_BYTES_PER_S, nbytes / (st["min"] * 1e-6) / HBM_BYTES_PER_S])
    return out


def bench_embed(enc, img, ts, args):
    """(b)"""
    w, b = enc.patch_embed.proj.weight, enc.patch_embed.proj.bias
    E = int(w.shape[0])
    R = img.shape[0] * (img.shape[2] // 16) * (img.shape[3] // 16)
    dy = torch.randn((img.shape[0], R // img.shape[0], E), device=DEV) * 1e-7

    def forward():
        with torch.no_grad():
            TE.patch_embed(img, w, b, ts, True)

    def both():
        w.grad = b.grad = None
        TE.patch_embed(img, w, b, ts, True)[0].backward(dy)
    return dict(flops_forward=2.0 * R * E * 768, forward_s=_stats(_wall(forward, args.rounds, args.warmup), unit="s"),
                forward_backward_s=_stats(_wall(both, args.rounds, args.warmup), unit="s"))


def bench_encoder(enc, img, ts, dy, args):
    """(c) and (d)"""
    rec = {}

    def native(precision):
        def step():
            enc.precision = precision
            enc.zero_grad(set_to_none=True)
            enc(img, ts)[0].backward(dy)
        return step
    for precision in ("fp32", "bf16"):
        s, peak = _wall_and_peak(native(precision), args.rounds, args.warmup, lambda: enc.zero_grad(set_to_none=True))
        rec[f"native_{precision}"] = dict(forward_backward_s=_stats(s, unit="s"), peak_allocated_bytes_above_resident=peak)
    native("fp32")()
    torch.cuda.synchronize()
    g_n = {k: p.grad.clone() for k, p in enc.named_parameters()}
    enc.zero_grad(set_to_none=True)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    heads, depth = enc.blocks_enc[0].num_heads, enc.depth
    flags = ER.portrait_flags(ts.cpu(), True)

    def clear():
        for v in leaves.values():
            v.grad = None

    def ref():
        clear()
        x, _ = ER.encoder(img, flags, leaves, heads, depth, enc.rope, enc.eps)
        x.backward(dy.view(x.shape))

    def ref16():
        clear()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x, _ = ER.encoder(img, flags, leaves, heads, depth, enc.rope, enc.eps)
        x.backward(dy.view(x.shape).to(x.dtype))
    try:
        ref()
        torch.cuda.synchronize()
        diff = {k: float((g_n[k] - leaves[k].grad).abs().max() / leaves[k].grad.abs().max()) for k in g_n}
        rec["largest_relative_grad_difference_fp32"] = max(diff.values())
        rec["largest_relative_grad_difference_fp32_at"] = max(diff, key=diff.get)
        del g_n
        for name, fn in (("restated_fp32", ref), ("restated_autocast_bf16", ref16)):
            s, peak = _wall_and_peak(fn, args.torch_rounds, 1, clear)
            rec[name] = dict(forward_backward_s=_stats(s, unit="s"), peak_allocated_bytes_above_resident=peak)
        for precision, name in (("fp32", "restated_fp32"), ("bf16", "restated_autocast_bf16")):
            rec[f"restated_over_native_{precision}_median"] = rec[name]["forward_backward_s"]["median"] / rec[f"native_{precision}"]["forward_backward_s"]["median"]
    except RuntimeError as e:                     # e.g. out of memory: said, not hidden
        rec["restated"] = dict(failed=str(e)[:200])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--portrait-every", type=int, default=4, help="every n-th view of the encoder runs is a portrait view (0: none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--gather-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_grad: needs a GPU (no CPU fallback)")
    V, H, W, D = args.views, args.height, args.width, args.dim
    g = torch.Generator(device=DEV).manual_seed(0)
    img = torch.rand((V, 3, H, W), generator=g, device=DEV) * 2 - 1
    n = (H // 16) * (W // 16)
    portrait = [args.portrait_every > 0 and v % args.portrait_every == 1 for v in range(V)]
    ts = torch.tensor([(W, H) if p else (H, W) for p in portrait], device=DEV)
    rec = dict(figure="encoder_grad", views=V, H=H, W=W, tokens=n, rows=V * n, D=D, heads=args.heads, hidden=4 * D, depth=args.depth, portrait_views=sum(portrait),
               conditions="clocks not pinned, shared machine; medians with min and max; (a) device events around the C entry point on preallocated buffers, "
                          "(b)-(d) host clock around a synchronise")
    rec["patch_rows"] = bench_gather(img, args)
    if not args.gather_only:
        torch.manual_seed(0)
        enc = TE.Dust3rEncoder(img_size=(H, W), embed_dim=D, depth=args.depth, num_heads=args.heads, mlp_ratio=4, patch_embed="ManyAR_PatchEmbed").to(DEV)
        dy = torch.randn((V, n, D), generator=g, device=DEV) * 1e-7
        rec["patch_embed"] = bench_embed(enc, img, ts, args)
        rec["encoder"] = bench_encoder(enc, img, ts, dy, args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
