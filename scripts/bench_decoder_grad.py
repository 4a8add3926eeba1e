"""The trainable decoder (must3r_amd.train_decoder; csrc/train_decoder.hip) on the GPU.  One JSON line per figure (append them to
profiles/decoder_grad_bench.jsonl).

  (a) feedback_prepare    the feedback add + norm_y of all layers, L 12, R 15360, D 768, add_layers 11: the fused operator (one launch each way) against the
                          composed form built from the parent's own operators on the same tensors in the same run -- a torch add per layer but the last plus
                          ``train_block.layer_norm`` per layer, with its backward under autograd.  Forward alone (no_grad) and forward + backward (autograd, an
                          upstream gradient per layer), both forms through their public functions, allocations included.
  (b) decoder_step        one scene of 10 views of 768 tokens (384 x 512) at the released decoder geometry (Denc 1024, D 768, 12 heads, depth 12, single_mlp,
                          ``norm_y``): the schedule [2, 1 x 8] plus a render of all 10 views, forward + backward with a gradient on every call's pointmaps;
                          time and ``max_memory_allocated``, beside the restated decoder (tests/decoder_ref.py) in fp32 under torch autograd on the same GPU.
                          Recorded, not gated.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
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
CONDITIONS = "clocks not pinned, shared machine; wall time around a synchronised call, medians"


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
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _verdict(fused, composed):
    """the criterion: the fused median below the composed one by more than the two min-max spreads"""
    gap = composed["median"] - fused["median"]
    spreads = (fused["max"] - fused["min"]) + (composed["max"] - composed["min"])
    return "fused faster beyond the spread" if gap > spreads else ("fused slower beyond the spread" if -gap > spreads else "equal within the spread")


def bench_feedback_prepare(args):
    L, R, D = args.layers, args.rows, args.width
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)
    xs, dys, offset = [rn(R, D) for _ in range(L)], [rn(R, D) * 1e-7 for _ in range(L)], rn(R, D)
    gammas, betas = [1 + 0.1 * rn(D) for _ in range(L)], [0.1 * rn(D) for _ in range(L)]
    leaves = [t.requires_grad_(True) for t in (*xs, offset, *gammas, *betas)]

    def composed():
        return [TB.layer_norm(x + offset if l < L - 1 else x, gammas[l], betas[l]) for l, x in enumerate(xs)]

    def fused():
        return TD.feedback_prepare(xs, offset, gammas, betas, L - 1)

    def step(fn):
        def run():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(fn(), dys)
        return run

    def forward(fn):
        def run():
            with torch.no_grad():
                fn()
        return run
    rec = dict(figure="feedback_prepare", L=L, R=R, D=D, add_layers=L - 1, conditions=CONDITIONS)
    step(fused)()
    got = [t.grad.clone() for t in leaves]
    step(composed)()
    rec["largest_relative_grad_difference"] = max(float((a - t.grad).abs().max() / t.grad.abs().max()) for a, t in zip(got, leaves))
    with torch.no_grad():
        rec["forward_bit_equal"] = all(torch.equal(a, b) for a, b in zip(fused(), composed()))
    del got
    for name, wrap in (("forward", forward), ("forward_backward", step)):
        f, c = _stats(_wall(wrap(fused), args.rounds, args.warmup), unit="ms"), _stats(_wall(wrap(composed), args.rounds, args.warmup), unit="ms")
        rec[name] = dict(fused_ms=f, composed_ms=c, composed_over_fused_median=c["median"] / f["median"], verdict=_verdict(f, c))
    rec["launches"] = dict(fused_forward=1, fused_backward=2, composed_forward=2 * L - 1, composed_backward=f"{3 * L} LayerNorm backward launches + {L - 1} adds")
    return rec


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

    def native():
        dec.zero_grad(set_to_none=True)
        for x in xs:
            x.grad = None
        mem, loss = None, 0
        for c, x, p, t, G in zip(case["calls"], xs, pos, ts, Gs):
            mem, pts = dec(x, p, t, mem, render=c["render"])
            loss = loss + (pts * G).sum()
        loss.backward()
    dcase = dict(case, pos=case["pos"].to(DEV))
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in case["params"].items()}

    def ref():
        for t in (*leaves.values(), *xs):
            t.grad = None
        outs, _ = DF.run(dcase, leaves, xs)
        sum((pts * G).sum() for (_, pts), G in zip(outs, Gs)).backward()
    rec = dict(figure="decoder_step", schedule=[v for v, _ in schedule], render_views=10, tokens=n, Denc=1024, D=768, heads=12, depth=12, feedback="single_mlp",
               memory_mode="norm_y", conditions=CONDITIONS)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    native()
    torch.cuda.synchronize()
    rec["native_peak_bytes"], rec["resident_before_bytes"] = int(torch.cuda.max_memory_allocated()), int(base)
    g_n = {f"dx{i}": x.grad.clone() for i, x in enumerate(xs)}
    g_n.update({k: p.grad.clone() for k, p in dec.named_parameters()})
    rec["native_ms"] = _stats(_wall(native, args.rounds, args.warmup), unit="ms")
    try:
        dec.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        ref()
        torch.cuda.synchronize()
        rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        g_t = {f"dx{i}": x.grad for i, x in enumerate(xs)}
        g_t.update({k: v.grad for k, v in leaves.items()})
        # cross_attn.projk.bias: the true gradient is zero (every key carries the bias; both sides hold rounding noise): left out of the ratio
        rel = {k: float((g_n[k] - g_t[k]).abs().max() / g_t[k].abs().max()) for k in g_n if not k.endswith("cross_attn.projk.bias")}
        rec["largest_relative_grad_difference"] = max(rel.values())
        rec["largest_relative_grad_difference_at"] = max(rel, key=rel.get)
        del g_t
        rec["torch_decoder_ref_fp32_ms"] = _stats(_wall(ref, args.torch_rounds, 1), unit="ms")
        rec["speedup_median"] = rec["torch_decoder_ref_fp32_ms"]["median"] / rec["native_ms"]["median"]
    except Exception as e:                        # e.g. out of memory: said, not hidden
        rec["torch_decoder_ref_fp32_ms"] = dict(failed=str(e)[:200])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--figures", nargs="*", default=["feedback_prepare", "decoder_step"], choices=["feedback_prepare", "decoder_step"])
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rows", type=int, default=15360)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder_grad: needs a GPU (no CPU fallback)")
    f = open(args.out, "a") if args.out else None
    for fig in args.figures:
        rec = bench_feedback_prepare(args) if fig == "feedback_prepare" else bench_decoder_step(args)
        line = json.dumps(rec)
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
