"""The training Linears on the 16-bit MFMA (csrc/train_lin16.hip; ``train_block.linear_precision("bf16")``) against the fp32 mode of the same run, which is the
code as it was before the switch existed.  One JSON line per figure (append them to profiles/linear16_bench.jsonl).

  (a) linear_forms    the three operator forms (forward with bias, data gradient, weight gradient with its reduction and the bias gradient) at the decoder's
                      Linear shapes, M = 15360 rows, N x K = 2304 x 768, 768 x 768, 3072 x 768, 768 x 3072, 1536 x 768, and at the encoder's, K = 1024:
                      3072 x 1024, 1024 x 1024, 4096 x 1024, 1024 x 4096.  Per round the two modes are timed one after the other on the same buffers;
                      a timing is ``inner`` back-to-back calls between two synchronisations, divided by ``inner``.
  (b) decoder_step    figure (b) of scripts/bench_decoder_grad.py -- one scene of 10 views of 768 tokens at the released decoder geometry, schedule [2, 1 x 8]
                      plus a render of all 10 views, forward + backward -- in both modes, alternated round by round; then one profiled pass per mode
                      (torch.profiler, kernel times) for the share of the GPU time that is Linear kernels.

Timings: ``warmup`` rounds, then ``rounds`` rounds: median, min and max.  "faster" means a gap of the medians larger than the two min-max spreads.  Clocks are
not pinned and the machine is shared: the record says so.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decoder_ref as DF  # noqa: E402
from must3r_amd import train_block as TB, train_decoder as TD  # noqa: E402

DEV = "cuda:0"
CONDITIONS = "clocks not pinned, shared machine; wall time around synchronised calls, medians; the two modes alternated round by round in one process"
MODES = ("fp32", "bf16")
DECODER_SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072), (1536, 768)]
ENCODER_SHAPES = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]
# the kernels of the four switched host functions, by the names a kernel trace shows (the gather forms of the head, <true, ...>, are not among them)
LINEAR_KERNELS = ("linear_fwd_f32", "linear_fwd_bf16", "dgrad_kernel<false", "dgrad_bf16", "wgrad_kernel<false", "wgrad_bf16")


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _verdict(new, old):
    gap = old["median"] - new["median"]
    spreads = (new["max"] - new["min"]) + (old["max"] - old["min"])
    return "bf16 faster beyond the spread" if gap > spreads else ("bf16 slower beyond the spread" if -gap > spreads else "equal within the spread")


def _alternate(fn, rounds, warmup, inner=1):
    """{mode: [ms per call]}: every round times fp32, then bf16"""
    out = {m: [] for m in MODES}
    for r in range(warmup + rounds):
        for m in MODES:
            with TB.linear_precision(m):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                if r >= warmup:
                    out[m].append((time.perf_counter() - t0) * 1e3 / inner)
    return out


def bench_linear_forms(args):
    M = args.rows
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)
    recs = []
    for family, shapes in (("decoder", DECODER_SHAPES), ("encoder", ENCODER_SHAPES)):
        for N, K in shapes:
            x, W, b, dy = rn(M, K), rn(N, K) * K ** -0.5, rn(N), rn(M, N)
            out = torch.empty((M, N), device=DEV)
            forms = dict(forward=lambda: TB.linear_forward(x, W, b, out=out), dgrad=lambda: TB.linear_grad(x, W, dy, want=(True, False, False)),
                         wgrad=lambda: TB.linear_grad(x, W, dy, want=(False, True, True)))
            rec = dict(figure="linear_forms", family=family, M=M, N=N, K=K, inner=args.inner, gflop=2.0 * M * N * K / 1e9, conditions=CONDITIONS)
            for name, fn in forms.items():
                t = _alternate(fn, args.rounds, args.warmup, args.inner)
                f32, b16 = _stats(t["fp32"], unit="ms"), _stats(t["bf16"], unit="ms")
                rec[name] = dict(fp32_ms=f32, bf16_ms=b16, fp32_over_bf16_median=f32["median"] / b16["median"], verdict=_verdict(b16, f32))
            recs.append(rec)
            del x, W, b, dy, out
            torch.cuda.empty_cache()
    return recs


def _kernel_times(fn):
    """(GPU microseconds of all kernels, of the Linear kernels, the Linear kernels by name) of one profiled call"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total, lin, by = 0.0, 0.0, {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and e.device_time > 0:
            total += e.device_time
            hit = [k for k in LINEAR_KERNELS if k in e.name]
            if hit:
                lin += e.device_time
                by[hit[0]] = by.get(hit[0], 0.0) + e.device_time
    return total, lin, by


def bench_decoder_step(args):
    schedule = ((2, False),) + ((1, False),) * 8 + ((10, True),)
    case = DF.make_case(Denc=1024, D=768, heads=12, hidden=3072, depth=12, feedback_type="single_mlp", mode="norm_y", causal=False, scenes=1, grid=(24, 32),
                        seed=5, schedule=schedule)
    n, H, W = case["n"], case["H"], case["W"]
    dec = TD.MUSt3R(enc_embed_dim=1024, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, feedback_type="single_mlp", memory_mode="norm_y")
    dec.load_state_dict(case["params"], strict=True)
    dec = dec.to(DEV)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    Gs = [c["G"].to(DEV) for c in case["calls"]]
    pos = [case["pos"].to(DEV).view(1, 1, n, 2).expand(1, c["V"], n, 2).contiguous() for c in case["calls"]]
    ts = [torch.tensor([H, W]).view(1, 1, 2).expand(1, c["V"], 2).contiguous() for c in case["calls"]]

    def step():
        dec.zero_grad(set_to_none=True)
        for x in xs:
            x.grad = None
        mem, loss = None, 0
        for c, x, p, t, G in zip(case["calls"], xs, pos, ts, Gs):
            mem, pts = dec(x, p, t, mem, render=c["render"])
            loss = loss + (pts * G).sum()
        loss.backward()
    rec = dict(figure="decoder_step", schedule=[v for v, _ in schedule], render_views=10, tokens=n, Denc=1024, D=768, heads=12, depth=12, feedback="single_mlp",
               memory_mode="norm_y", conditions=CONDITIONS)
    t = _alternate(step, args.rounds, args.warmup)
    f32, b16 = _stats(t["fp32"], unit="ms"), _stats(t["bf16"], unit="ms")
    rec.update(fp32_ms=f32, bf16_ms=b16, fp32_over_bf16_median=f32["median"] / b16["median"], verdict=_verdict(b16, f32))
    grads = {}
    for m in MODES:
        with TB.linear_precision(m):
            step()
            torch.cuda.synchronize()
            grads[m] = {k: p.grad.clone() for k, p in dec.named_parameters()}
            try:
                total, lin, by = _kernel_times(step)
                rec[f"{m}_kernel_ms"] = dict(all_kernels=total / 1e3, linear_kernels=lin / 1e3, linear_share=lin / total if total else None,
                                             by_kernel_ms={k: v / 1e3 for k, v in sorted(by.items())})
            except Exception as e:                # said, not hidden
                rec[f"{m}_kernel_ms"] = dict(failed=str(e)[:200])
    rel = {k: float((grads["bf16"][k] - grads["fp32"][k]).abs().max() / grads["fp32"][k].abs().max()) for k in grads["fp32"]
           if not k.endswith("cross_attn.projk.bias")}
    rec["largest_relative_grad_difference_bf16_vs_fp32"] = max(rel.values())
    rec["largest_relative_grad_difference_at"] = max(rel, key=rel.get)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--figures", nargs="*", default=["linear_forms", "decoder_step"], choices=["linear_forms", "decoder_step"])
    ap.add_argument("--rows", type=int, default=15360)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear16: needs a GPU (no CPU fallback)")
    f = open(args.out, "a") if args.out else None
    for fig in args.figures:
        for rec in (bench_linear_forms(args) if fig == "linear_forms" else bench_decoder_step(args)):
            line = json.dumps(rec)
            print(line, flush=True)
            if f:
                f.write(line + "\n")
                f.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
