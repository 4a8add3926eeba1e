"""The optimizer step (must3r_amd.train_optim; csrc/train_optim.hip) on the GPU, on the parameter shapes of the released decoder
(``synthetic.make_decoder_state_dict(MUST3R_512)``).  One JSON line per figure (append them to profiles/optim_bench.jsonl).

  (a) protocol   the whole protocol of one accumulated step -- the norm with a clip, the step, the scaler update -- in three forms on the same tensors,
                 alternated inside one run:
                   native          ``AdamW.grad_norm(max_norm, scaler)`` + ``AdamW.step(control=...)``
                   torch_foreach   ``GradScaler.unscale_`` + ``clip_grad_norm_`` + ``GradScaler.step(torch.optim.AdamW(foreach=True))`` + ``GradScaler.update``
                   torch_fused     the same with ``torch.optim.AdamW(fused=True)``
                 per form: the synchronised wall time, the GPU time between two events on the stream, the host time until the calls have returned, and the
                 number of kernel launches with the kernels' own durations in one profiled round (torch.profiler); for the native form its algorithmic bytes (32 B per parameter) over its GPU time against the
                 6.3 TB/s a float4 copy reaches.  torch unscales the gradients in place, so every form gets its gradients restored before each round,
                 outside the timed region.
  (b) parts      the native norm pass and the native step alone, GPU time between events: 4 B and 28 B per parameter.  The time between the events contains
                 the host's preparation of the call (the table of ~300 tensors is refreshed in Python before anything is queued), which an idle stream
                 does not hide: the kernels' own rates are those of ``kernel_us`` in (a).

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_decoder_grad import CONDITIONS, DEV, _stats, _verdict  # noqa: E402
from must3r_amd import synthetic as S, train_optim as TO  # noqa: E402
from must3r_amd.config import MUST3R_512  # noqa: E402

COPY_TBPS = 6.3
SCALE, MAX_NORM = 65536.0, 1.0
HYPER = dict(lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)


def _shapes():
    return [tuple(v.shape) for v in S.make_decoder_state_dict(MUST3R_512, 0).values() if v.is_floating_point() and v.numel() > 0]


class Form:
    def __init__(self, name, shapes, grads):
        self.name = name
        g = torch.Generator(device=DEV).manual_seed(1)
        self.params = [torch.nn.Parameter(torch.randn(s, generator=g, device=DEV) * 0.02) for s in shapes]
        self.master = grads
        for p, m in zip(self.params, grads):
            p.grad = m.clone()
        if name == "native":
            self.opt, self.scaler = TO.AdamW(self.params, **HYPER), TO.LossScaler()
        else:
            self.opt = torch.optim.AdamW(self.params, foreach=name == "torch_foreach", fused=name == "torch_fused", **HYPER)
            self.scaler = torch.amp.GradScaler("cuda")
            self.scaler.scale(torch.zeros((1,), device=DEV))           # creates the scale, as the loop's scaler.scale(loss) would

    def restore(self):
        torch._foreach_copy_([p.grad for p in self.params], self.master)

    def run(self):
        if self.name == "native":
            self.opt.step(control=self.opt.grad_norm(max_norm=MAX_NORM, scaler=self.scaler))
        else:
            self.scaler.unscale_(self.opt)
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.scaler.step(self.opt)
            self.scaler.update()

    def launches(self):
        """(kernel launches of one round, microseconds per kernel name) from the profiler; the reason as a string where it records no device events"""
        try:
            from torch.profiler import ProfilerActivity, profile
            self.restore()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                self.run()
                torch.cuda.synchronize()
            n, per = 0, {}
            for e in prof.events():
                if not str(getattr(e, "device_type", "")).endswith("CUDA") or "emcpy" in e.name or "emset" in e.name or e.name.startswith("Optimizer."):
                    continue                                # copies, and the range torch's optimizers annotate their step with
                n += 1
                us = getattr(e, "device_time", None)
                us = getattr(e, "cuda_time", 0.0) if us is None else us
                per[e.name[:60]] = per.get(e.name[:60], 0.0) + float(us)
            return (n, per) if n else ("the profiler recorded no device events", {})
        except Exception as e:                              # said, not hidden
            return f"profiler failed: {str(e)[:120]}", {}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b), host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU (no CPU fallback)")
    shapes = _shapes()
    n_params = sum(torch.Size(s).numel() for s in shapes)
    g = torch.Generator(device=DEV).manual_seed(0)
    grads = [torch.randn(s, generator=g, device=DEV) * 1e-3 * SCALE for s in shapes]
    forms = [Form(n, shapes, grads) for n in ("native", "torch_foreach", "torch_fused")]
    times = {f.name: dict(wall=[], gpu=[], host=[]) for f in forms}
    for r in range(args.warmup + args.rounds):
        for f in forms:
            f.restore()
            wall, gpu, host = _timed(f.run)
            if r >= args.warmup:
                for k, x in zip(("wall", "gpu", "host"), (wall, gpu, host)):
                    times[f.name][k].append(x)
    rec = dict(figure="protocol", tensors=len(shapes), parameters=n_params, max_norm=MAX_NORM, scale=SCALE, warmup=args.warmup, conditions=CONDITIONS)
    for f in forms:
        t = times[f.name]
        n, per = f.launches()
        rec[f.name] = dict(wall_ms=_stats(t["wall"]), gpu_ms=_stats(t["gpu"]), host_ms=_stats(t["host"]), kernel_launches=n)
        if f.name == "native":
            rec[f.name]["kernel_us"] = per       # one profiled round: the kernels alone, without the host's share of the time between the events
            rec[f.name]["kernel_tbps"] = {k: b * n_params / (us * 1e-6) / 1e12 for k, us in per.items() for w, b in (("sumsq", 4), ("adamw", 28)) if w in k and us > 0}
        else:
            rec[f.name]["kernel_us_total"] = sum(per.values())
    nat = rec["native"]
    nat["algorithmic_bytes"] = 32 * n_params
    nat["tbps_of_gpu_time"] = 32 * n_params / (nat["gpu_ms"]["median"] * 1e-3) / 1e12
    nat["fraction_of_copy_rate"] = nat["tbps_of_gpu_time"] / COPY_TBPS
    for other in ("torch_foreach", "torch_fused"):
        rec[f"native_vs_{other}"] = dict(gpu=_verdict(nat["gpu_ms"], rec[other]["gpu_ms"]).replace("fused", "native"),
                                         wall=_verdict(nat["wall_ms"], rec[other]["wall_ms"]).replace("fused", "native"),
                                         gpu_ratio_median=rec[other]["gpu_ms"]["median"] / nat["gpu_ms"]["median"])
    lines = [rec]
    # (b) the two native passes alone
    f = forms[0]
    parts = dict(norm=[], step=[])
    for r in range(args.warmup + args.rounds):
        _, gn, _ = _timed(lambda: f.opt.grad_norm(max_norm=MAX_NORM, scaler=f.scaler))
        _, gs, _ = _timed(lambda: f.opt.step(control=f.opt._layout["control"]))
        if r >= args.warmup:
            parts["norm"].append(gn)
            parts["step"].append(gs)
    prec = dict(figure="parts", parameters=n_params, conditions=CONDITIONS)
    for k, b in (("norm", 4), ("step", 28)):
        st = _stats(parts[k])
        prec[k] = dict(gpu_ms=st, bytes=b * n_params, tbps=b * n_params / (st["median"] * 1e-3) / 1e12)
        prec[k]["fraction_of_copy_rate"] = prec[k]["tbps"] / COPY_TBPS
    lines.append(prec)
    out = open(args.out, "a") if args.out else None
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")


if __name__ == "__main__":
    main()
